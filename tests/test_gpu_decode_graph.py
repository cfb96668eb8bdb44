"""One decode step as a captured graph, on a real MI355X: the token-embedding kernel and the QKV GEMM with the K/V append in its epilogue
against the launches they replace, the captured stack against the eager cached stack, and VideoGPT.generate(graph=True) against
graph=False - all bit for bit (the captured step runs the same kernels on the same operands, so nothing here has a tolerance)."""
import pytest
import torch

import weights as W
from vitamd import lib, ops
from vitamd.functions import WEIGHTS

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def _randn(seed, *shape, scale=1.0, dtype=BF16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ embed kernel
@pytest.mark.parametrize("D", [64, 512])
def test_decode_embed_equals_torch_gather_and_add(hip, D):
    tok_rows, pos_rows = 257, 64                     # 256 codes + the SOS row
    tok, pos = _randn(1, tok_rows, D, dtype=F32), _randn(2, pos_rows, D, dtype=F32)
    tok_e, pos_e = torch.nn.Embedding(tok_rows, D, _weight=tok), torch.nn.Embedding(pos_rows, D, _weight=pos)
    for B in (1, 3, 65):
        ids = W.randint(3, f"ids{B}", (B,), tok_rows).cuda()
        ids[0] = tok_rows - 1                         # the last table row (SOS)
        if B > 1:
            ids[-1] = 0
        else:
            assert torch.equal(ops.decode_embed(tok, pos, torch.zeros(1, dtype=torch.int64, device="cuda"),
                                                torch.zeros(1, dtype=torch.int32, device="cuda")), tok[:1] + pos[:1])
        for n in (0, 1, pos_rows - 1):
            length = torch.tensor([n], dtype=torch.int32, device="cuda")
            with torch.no_grad():
                ref = tok_e(ids) + pos_e(torch.arange(n, n + 1, device="cuda"))
            x = ops.decode_embed(tok, pos, ids, length)
            assert x.dtype == F32 and torch.equal(x, ref), (B, n)
            out = torch.empty_like(ref)
            assert ops.decode_embed(tok, pos, ids, length, out=out) is out and torch.equal(out, ref)
    # outside either table: the row is left as it was, nothing is read
    ids = torch.tensor([5, tok_rows, -1, 7], dtype=torch.int64, device="cuda")
    out = torch.full((4, D), 3.0, device="cuda")
    ops.decode_embed(tok, pos, ids, torch.tensor([2], dtype=torch.int32, device="cuda"), out=out)
    assert torch.equal(out[0], tok[5] + pos[2]) and torch.equal(out[3], tok[7] + pos[2]) and bool((out[1:3] == 3.0).all())
    for bad in (pos_rows, -1):
        out.fill_(3.0)
        ops.decode_embed(tok, pos, ids, torch.tensor([bad], dtype=torch.int32, device="cuda"), out=out)
        assert bool((out == 3.0).all())
    with pytest.raises(lib.VitamdError):
        ops.decode_embed(tok, pos[:, :32].contiguous(), ids, length)


# ------------------------------------------------------------------------------------------------ fused QKV + append
@pytest.mark.parametrize("K", [128, 512])
@pytest.mark.parametrize("H", [2, 8])
def test_qkv_append_equals_gemm_then_kv_append(hip, K, H):
    N = 3 * H * 64
    w = _randn(10, N, K, scale=K ** -0.5)
    bias = _randn(11, N, scale=0.5, dtype=F32)
    for M in (1, 17, 64):                             # MT 1, 2 and 4
        assert (hip.vitamd_gemm_skinny_ws_bytes(M, N, K) > 0) == (K == 512)          # K = 128: unsplit main kernel; 512: split-K + reduce
        a = _randn(12 + M, M, K)
        qkv_ref = ops.gemm_skinny(a, w, ops.EPI_BIAS_BF16, bias=bias)
        for Lmax in (96, 300):
            for n in (0, 1, Lmax - 1):
                length = torch.tensor([n], dtype=torch.int32, device="cuda")
                kr = torch.full((M, H, Lmax, 64), 7.0, dtype=BF16, device="cuda")
                vr = torch.full((M, H, Lmax, 64), -7.0, dtype=BF16, device="cuda")
                ops.kv_append(qkv_ref, kr, vr, length, M, 1, H, host_len=n)
                kc = torch.full((M, H, Lmax, 64), 7.0, dtype=BF16, device="cuda")
                vc = torch.full((M, H, Lmax, 64), -7.0, dtype=BF16, device="cuda")
                qkv = ops.gemm_skinny_qkv_append(a, w, bias, kc, vc, length, H, host_len=n)
                assert torch.equal(qkv, qkv_ref), (M, Lmax, n)
                assert torch.equal(kc, kr) and torch.equal(vc, vr), (M, Lmax, n)
                assert int(length.item()) == n                                       # the kernel does not advance the length
    # the guard of kv_append_kernel: a length outside [0, Lmax) writes qkv and leaves the caches alone; the host refuses it when told
    for bad in (Lmax, -1):
        kc.fill_(7.0); vc.fill_(-7.0)
        qkv = ops.gemm_skinny_qkv_append(a, w, bias, kc, vc, torch.tensor([bad], dtype=torch.int32, device="cuda"), H)
        assert torch.equal(qkv, qkv_ref) and bool((kc == 7.0).all()) and bool((vc == -7.0).all())
    with pytest.raises(lib.VitamdError):
        ops.gemm_skinny_qkv_append(a, w, bias, kc, vc, length, H, host_len=Lmax)
    with pytest.raises(lib.VitamdError):
        ops.gemm_skinny_qkv_append(a, w, bias, kc[:, :1].contiguous(), vc[:, :1].contiguous(), length, H)
    with pytest.raises(lib.VitamdError):
        ops.gemm_skinny_qkv_append(_randn(1, 65, K), w, bias, kc, vc, length, H)


# ------------------------------------------------------------------------------------------------ captured stack against eager
@pytest.mark.parametrize("max_len", [300, 96])
def test_captured_stack_equals_eager_bit_for_bit(hip, max_len):
    import transformer as T
    seed, B, P = 7, 3, 5
    cfg = T.TransformerConfig(n_layers=2, n_heads=4, n_embd=256, block_size=300, causal=True)
    m = T.Transformer(cfg)
    m.load_state_dict(W.transformer_state(seed, "", cfg.n_layers, cfg.n_embd, causal_block=300), strict=True)
    m = m.cuda().eval()
    assert hip.vitamd_gemm_skinny_ws_bytes(B, 3 * 256, 256) > 0                        # the QKV GEMM is split-K
    assert (hip.vitamd_decode_attention_ws_bytes(B, 4, max_len) > 0) == (max_len == 300)   # 3 chunks of 128 keys + combine / one chunk
    x = W.normal(seed, "x", (B, max_len, cfg.n_embd)).cuda()
    cache = m.new_cache(B, max_len=max_len)
    eager = [m.forward_cached(x[:, :P], cache)]
    for t in range(P, max_len):
        eager.append(m.forward_cached(x[:, t:t + 1], cache))
    eager = torch.cat(eager, dim=1)

    dec = m.graphed_decoder(B, max_len=max_len)
    assert dec.captures == 1 and dec.cache.len == 0 and int(dec.cache.len_dev.item()) == 0
    outs = [dec.prefill(x[:, :P])]
    for t in range(P, max_len):
        outs.append(dec.step(x[:, t:t + 1]).clone())
    outs = torch.cat(outs, dim=1)
    assert torch.equal(outs, eager)
    assert torch.equal(dec.cache.k, cache.k) and torch.equal(dec.cache.v, cache.v)
    assert dec.cache.len == max_len == cache.len and int(dec.cache.len_dev.item()) == max_len
    with pytest.raises(ValueError):
        dec.step(x[:, :1])                                                             # full: refused without replaying
    assert int(dec.cache.len_dev.item()) == max_len
    dec.reset()
    again = [dec.prefill(x[:, :P])] + [dec.step(x[:, t:t + 1]).clone() for t in range(P, P + 10)]
    assert torch.equal(torch.cat(again, dim=1), eager[:, :P + 10])
    assert dec.captures == 1 and dec.cache.len == P + 10 == int(dec.cache.len_dev.item())


# ------------------------------------------------------------------------------------------------ VideoGPT
SAMPLED = dict(temperature=1.0, top_k=20, top_p=0.9, seed=3)


def _videogpt(seed=0):
    """preset S, 16-token frames, 256 codes, 4 frames, the head partly tied to the shifted embeddings (as tests/test_gpu_decode.py)"""
    import train_videogpt as V
    cfg = V.VideoGPTConfig(frame_size=16, codebook_size=256, transformer="S", max_frames=4, dropout=0.0)
    D, Nc = cfg.n_embd, cfg.codebook_size
    sd = {"tok_embed.weight": W.normal(seed, "tok_embed", (Nc + 1, D)), "pos_embed.weight": W.normal(seed, "pos_embed", (cfg.max_tokens, D))}
    sd.update(W.transformer_state(seed, "transformer.", cfg.trans_config.n_layers, D, causal_block=cfg.max_tokens))
    sd.update(W.linear_state(seed, "proj.", Nc, D))
    sd["proj.weight"] = sd["proj.weight"] + 0.01 * torch.roll(sd["tok_embed.weight"][:Nc], 1, 0)
    model = V.VideoGPT(cfg)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), cfg


@pytest.fixture(scope="module")
def gpt(hip):
    return _videogpt()


def _prompt(cfg, name, B=4, frames=2):
    return W.randint(0, name, (B, frames, cfg.frame_size), cfg.codebook_size).cuda()


@pytest.mark.parametrize("sampling", [{}, SAMPLED], ids=["greedy", "sampled"])
def test_generate_frames_graph_equals_eager(gpt, sampling):
    model, cfg = gpt
    video = _prompt(cfg, "prompt")
    eager = model.generate_frames(video, n=2, graph=False, **sampling)
    out = model.generate_frames(video, n=2, graph=True, **sampling)
    assert tuple(out.shape) == (4, 64) and out.dtype == eager.dtype and torch.equal(out, eager)
    dec = model._graph_decoder
    assert dec.captures == 1
    # another prompt of the same shape: the same decoder, no new capture
    video2 = _prompt(cfg, "prompt2")
    out2 = model.generate_frames(video2, n=2, graph=True, **sampling)
    assert model._graph_decoder is dec and dec.captures == 1
    assert torch.equal(out2, model.generate_frames(video2, n=2, graph=False, **sampling))
    assert not torch.equal(out2, out)
    if sampling:                                                                       # the same seed repeats its tokens (position back to 0)
        assert torch.equal(model.generate_frames(video, n=2, graph=True, **sampling), out)
        assert model._graph_decoder is dec and dec.captures == 1
    # another n: another max_len, captured again
    out1 = model.generate_frames(video, n=1, graph=True, **sampling)
    assert model._graph_decoder is not dec and model._graph_decoder.captures == 1
    assert torch.equal(out1, model.generate_frames(video, n=1, graph=False, **sampling))


def test_generate_graph_follows_a_weight_refresh(hip):
    model, cfg = _videogpt()
    video = _prompt(cfg, "prompt")
    before = model.generate_frames(video, n=2, graph=True)
    dec = model._graph_decoder
    model.proj.weight.data.mul_(1.5)
    model.transformer.layers[0].mlp[0].weight.data.mul_(1.5)
    WEIGHTS.clear()
    out = model.generate_frames(video, n=2, graph=True)
    eager = model.generate_frames(video, n=2, graph=False)
    assert torch.equal(out, eager)
    assert not torch.equal(out, before)                                                # the changed weights change the continuation
    assert model._graph_decoder is dec and dec.captures == 1                           # same buffers refreshed in place: the graph still holds
    # an operand that moves (a new parameter storage) is noticed: captured again, never a stale replay
    model.proj.weight.data = model.proj.weight.data.clone()
    out = model.generate_frames(video, n=2, graph=True)
    assert model._graph_decoder is dec and dec.captures == 2 and torch.equal(out, eager)


def test_generate_graph_batch_65(gpt):
    model, cfg = gpt
    video = _prompt(cfg, "prompt65", B=65, frames=1)                                   # head and stack in row blocks above 64
    out = model.generate_frames(video, n=3, graph=True)
    assert tuple(out.shape) == (65, 64) and torch.equal(out, model.generate_frames(video, n=3, graph=False))


def test_generate_graph_refusals(gpt):
    model, cfg = gpt
    tokens = W.randint(0, "prompt", (2, 8), cfg.codebook_size).cuda()
    with pytest.raises(ValueError):
        model.generate(tokens, n=2, graph=True, use_cache=False)
    with pytest.raises(ValueError):
        model.generate(tokens, n=cfg.max_tokens - 8 + 1, graph=True)
    assert torch.equal(model.generate(tokens, n=1, graph=True), model.generate(tokens, n=1))      # no replay at all: prefill + first pick
