"""CPU-only checks of the captured decode step's surface: the two new entry points are bound, the new ops and the graph=True paths refuse
what they do not support before touching a device, and the default arguments of generate are the old ones."""
import inspect

import pytest
import torch

from vitamd import lib, ops


def test_new_entry_points_are_bound_and_the_abi_is_additive():
    for name in ("vitamd_decode_embed", "vitamd_gemm_skinny_qkv_append"):
        assert name in lib.SIGNATURES
    L = lib.load()
    assert L.vitamd_abi_version() == 9 and lib.ABI_VERSION == 9
    assert hasattr(L, "vitamd_decode_embed") and hasattr(L, "vitamd_gemm_skinny_qkv_append")


def test_new_ops_refuse_cpu_tensors():
    tok, pos = torch.zeros(9, 64), torch.zeros(8, 64)
    ids, length = torch.zeros(3, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(lib.VitamdError):
        ops.decode_embed(tok, pos, ids, length)
    a, w = torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(384, 128, dtype=torch.bfloat16)
    kc = torch.zeros(4, 2, 96, 64, dtype=torch.bfloat16)
    with pytest.raises(lib.VitamdError):
        ops.gemm_skinny_qkv_append(a, w, torch.zeros(384), kc, kc.clone(), length, 2, host_len=0)


def test_graphed_decoder_refuses_non_causal_and_dropout():
    import transformer as T
    with pytest.raises(ValueError):
        T.Transformer(T.S(block_size=32)).graphed_decoder(2)                           # not causal
    with pytest.raises(ValueError):
        T.Transformer(T.S(block_size=32, causal=True, dropout=0.1)).graphed_decoder(2)


def test_generate_graph_refusals_and_old_defaults():
    import train_videogpt as V
    tokens = torch.zeros(2, 8, dtype=torch.long)
    model = V.VideoGPT(V.VideoGPTConfig(16, 256, "S", 4, 0.0))
    with pytest.raises(ValueError):
        model.generate(tokens, n=2, graph=True, use_cache=False)
    with pytest.raises(ValueError):
        model.generate_frames(tokens.view(2, 1, 8), n=1, graph=True, use_cache=False)
    drop = V.VideoGPT(V.VideoGPTConfig(16, 256, "S", 4, 0.1))
    with pytest.raises(ValueError):
        drop.generate(tokens, n=2, graph=True)
    for fn in (V.VideoGPT.generate, V.VideoGPT.generate_frames):
        p = inspect.signature(fn).parameters
        assert list(p)[:4] == ["self", "tokens" if fn is V.VideoGPT.generate else "video_tokens", "n", "use_cache"]
        assert p["n"].default == 1 and p["use_cache"].default is None and p["seed"].default == 0
        assert all(p[k].default is None for k in ("temperature", "top_k", "top_p"))
        assert p["graph"].default is False and p["graph"].kind is inspect.Parameter.KEYWORD_ONLY
