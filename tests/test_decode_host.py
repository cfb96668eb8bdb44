"""CPU-only checks of the KV-cached decoding surface: the VideoGPT module (train_videogpt.py) builds without a GPU with the reference's
parameters and state_dict keys, and the decode entry points refuse what they do not support before touching a device."""
import pytest
import torch

from vitamd import lib, ops


def test_videogpt_reference_defaults_state_dict():
    import train_videogpt as V
    cfg = V.VideoGPTConfig(64, 1024, "B", 16, 0.0)              # the reference's argparse defaults (train_videogpt.py:69-73)
    assert (cfg.max_tokens, cfg.n_embd) == (1024, 768)
    tc = cfg.trans_config
    assert tc.causal and tc.block_size == 1024 and (tc.n_layers, tc.n_heads) == (12, 12)
    model = V.VideoGPT(cfg)
    sd = model.state_dict()
    assert tuple(sd["tok_embed.weight"].shape) == (1025, 768)
    assert tuple(sd["pos_embed.weight"].shape) == (1024, 768)
    assert tuple(sd["proj.weight"].shape) == (1024, 768) and tuple(sd["proj.bias"].shape) == (1024,)
    layer = {"multi_attn.qkv.weight": (2304, 768), "multi_attn.qkv.bias": (2304,), "multi_attn.mask": (1024, 1024),
             "mlp.0.weight": (3072, 768), "mlp.0.bias": (3072,), "mlp.2.weight": (768, 3072), "mlp.2.bias": (768,)}
    want = {"tok_embed.weight", "pos_embed.weight", "proj.weight", "proj.bias"}
    for i in range(12):
        for k, shape in layer.items():
            key = f"transformer.layers.{i}.{k}"
            want.add(key)
            assert tuple(sd[key].shape) == shape, key
    assert set(sd) == want
    assert float(sd["transformer.layers.0.multi_attn.mask"][0, 1]) == float("-inf")
    D = 768
    per_layer = 3 * D * D + 3 * D + 4 * D * D + 4 * D + 4 * D * D + D
    assert sum(p.numel() for p in model.parameters()) == 1025 * D + 1024 * D + 12 * per_layer + D * 1024 + 1024
    assert all(not p.is_cuda for p in model.parameters())


def test_cache_refusals_without_a_gpu():
    import transformer as T
    import train_videogpt as V
    with pytest.raises(ValueError):
        T.Transformer(T.S(block_size=32)).new_cache(2)                                 # not causal
    drop = T.Transformer(T.S(block_size=32, causal=True, dropout=0.1))
    with pytest.raises(ValueError):
        drop.new_cache(2)
    with pytest.raises(ValueError):
        drop.forward_cached(torch.zeros(2, 1, 512), None)
    model = V.VideoGPT(V.VideoGPTConfig(16, 256, "S", 4, 0.1))
    tokens = torch.zeros(2, 8, dtype=torch.long)
    with pytest.raises(ValueError):
        model.generate(tokens, n=2, use_cache=True)                                    # dropout > 0
    with pytest.raises(ValueError):
        model.generate(tokens, n=57)                                                   # 8 + 57 > max_tokens = 64
    with pytest.raises(ValueError):
        model.generate_frames(tokens.view(2, 1, 8), n=4, use_cache=False)             # 8 + 64 > 64


def test_decode_ops_refuse_cpu_tensors():
    a = torch.zeros(4, 768, dtype=torch.bfloat16)
    w = torch.zeros(768, 768, dtype=torch.bfloat16)
    with pytest.raises(lib.VitamdError):
        ops.gemm_skinny(a, w, ops.EPI_BIAS_BF16)
    kc = torch.zeros(4, 12, 64, 64, dtype=torch.bfloat16)
    length = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(lib.VitamdError):
        ops.kv_append(torch.zeros(4, 3 * 768, dtype=torch.bfloat16), kc, kc, length, 4, 1, 12)
    with pytest.raises(lib.VitamdError):
        ops.decode_attention(torch.zeros(4, 3 * 768, dtype=torch.bfloat16), kc, kc, length, 4, 12)


def test_decode_entry_points_are_bound():
    for name in ("vitamd_kv_append", "vitamd_decode_attention", "vitamd_decode_attention_ws_bytes", "vitamd_gemm_skinny_bf16",
                 "vitamd_gemm_skinny_ws_bytes"):
        assert name in lib.SIGNATURES
    L = lib.load()
    assert L.vitamd_abi_version() == 9
    # shape rules of the size queries (no device needed): M > 64, K % 64, N % 4, Lmax > 16384 are refused
    assert L.vitamd_gemm_skinny_ws_bytes(65, 768, 768) < 0
    assert L.vitamd_gemm_skinny_ws_bytes(32, 768, 700) < 0
    assert L.vitamd_gemm_skinny_ws_bytes(32, 766, 768) < 0
    assert L.vitamd_decode_attention_ws_bytes(32, 12, 16385) < 0
