"""KV-cached decoding on a real MI355X: the three decode kernels through the C ABI (K/V append, single-query attention, skinny-M GEMM),
the cached causal stack against the full-sequence path and the fp32 oracle, and VideoGPT (train_videogpt.py) generation with and
without the cache."""
import pytest
import torch

import vit_oracle as O
import weights as W
from vitamd import lib, ops

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def _randn(seed, *shape, scale=1.0, dtype=BF16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ K/V append
@pytest.mark.parametrize("T,offsets", [(1, (0, 1, 63, 511)), (197, (0, 3, 315))])
def test_kv_append_copies_the_k_and_v_slices(hip, T, offsets):
    B, H, Lmax = 3, 12, 512
    qkv = _randn(1, B * T, 3 * H * 64)
    view = qkv.view(B, T, 3, H, 64)
    for off in offsets:
        kc = torch.full((B, H, Lmax, 64), 7.0, dtype=BF16, device="cuda")
        vc = torch.full((B, H, Lmax, 64), -7.0, dtype=BF16, device="cuda")
        length = torch.tensor([off], dtype=torch.int32, device="cuda")
        ops.kv_append(qkv, kc, vc, length, B, T, H, host_len=off)
        torch.cuda.synchronize()
        assert torch.equal(kc[:, :, off:off + T], view[:, :, 1].permute(0, 2, 1, 3))
        assert torch.equal(vc[:, :, off:off + T], view[:, :, 2].permute(0, 2, 1, 3))
        rest = torch.ones(Lmax, dtype=torch.bool)
        rest[off:off + T] = False
        assert bool((kc[:, :, rest] == 7.0).all()) and bool((vc[:, :, rest] == -7.0).all())      # nothing else written
        assert int(length.item()) == off                                                          # the kernel does not advance the length


# ------------------------------------------------------------------------------------------------ decode attention
def _attention_ref(qkv, kc, vc, n, H):
    """fp32 softmax attention of each sequence's query row over cache positions 0 .. n-1 (the same bf16 cache)"""
    B = qkv.shape[0]
    q = qkv[:, :H * 64].float().view(B, H, 1, 64)
    k, v = kc[:, :, :n].float(), vc[:, :, :n].float()
    p = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, dim=-1)
    return (p @ v).view(B, H * 64)


@pytest.mark.parametrize("B,H", [(1, 8), (4, 12), (32, 12)])
def test_decode_attention_matches_fp32_softmax_attention(hip, B, H):
    Lmax = 16384
    kc, vc = _randn(2, B, H, Lmax, 64), _randn(3, B, H, Lmax, 64)
    qkv = _randn(4, B, 3 * H * 64)
    for n in (1, 31, 32, 33, 197, 1024, 4096, 16384):
        length = torch.tensor([n - 1], dtype=torch.int32, device="cuda")      # the query sits at position n-1, its K/V already appended
        ref = _attention_ref(qkv, kc, vc, n, H)
        caches = [(kc, vc)]
        if n <= 4096:
            caches.append((kc[:, :, :n].contiguous(), vc[:, :, :n].contiguous()))   # a cache exactly as long as the sequence: another split
        for k_, v_ in caches:
            o = ops.decode_attention(qkv, k_, v_, length, B, H, host_len=n - 1)
            o2 = ops.decode_attention(qkv, k_, v_, length, B, H, host_len=n - 1)
            torch.cuda.synchronize()
            assert o.dtype == BF16 and tuple(o.shape) == (B, H * 64)
            assert O.rel_l2(o.float(), ref) <= 4e-3, (n, k_.shape[2])
            assert torch.equal(o, o2), (n, k_.shape[2])                      # deterministic split + combine


# ------------------------------------------------------------------------------------------------ skinny-M GEMM
SKINNY_SHAPES = [(2304, 768), (3072, 768), (768, 3072), (1024, 768), (1536, 512), (2048, 512), (512, 2048), (3072, 1024), (1024, 4096)]


@pytest.mark.parametrize("N,K", SKINNY_SHAPES)
def test_gemm_skinny_every_epilogue(hip, N, K):
    w = _randn(10, N, K, scale=K ** -0.5)
    bias = _randn(11, N, scale=0.5, dtype=F32)
    bias_b = bias.to(BF16).float()
    for M in (1, 2, 7, 16, 32, 64):
        a = _randn(12 + M, M, K)
        acc = (a.double() @ w.double().t()).float()          # fp32-exact accumulation of the same bf16 operands
        aux = _randn(13 + M, M, N, dtype=F32)
        # fp32 output: acc + bf16(bias), no rounding
        y = ops.gemm_skinny(a, w, ops.EPI_F32, bias=bias)
        assert y.dtype == F32 and O.rel_l2(y, acc + bias_b) < 1e-5, M
        assert torch.equal(y, ops.gemm_skinny(a, w, ops.EPI_F32, bias=bias)), M                  # run to run (split-K summed in order)
        # bf16 = bf16(acc + bf16(bias))
        y = ops.gemm_skinny(a, w, ops.EPI_BIAS_BF16, bias=bias)
        assert y.dtype == BF16 and O.rel_l2(y.float(), (acc + bias_b).to(BF16).float()) < 1e-3, M
        assert torch.equal(y, ops.gemm_skinny(a, w, ops.EPI_BIAS_BF16, bias=bias)), M          # run to run
        # fp32 residual + bf16(acc + bias)
        y = ops.gemm_skinny(a, w, ops.EPI_RESID_F32, bias=bias, aux=aux)
        assert y.dtype == F32 and O.rel_l2(y, aux + (acc + bias_b).to(BF16).float()) < 1e-3, M
        # GELU: pre-activation and erf-GELU; bit-equal to gemm_nt's GELU where the two pre-activations are equal (one table)
        pre, g = ops.gemm_skinny(a, w, ops.EPI_GELU, bias=bias)
        pre_ref = (acc + bias_b).to(BF16).float()
        assert O.rel_l2(pre.float(), pre_ref) < 1e-3, M
        assert O.rel_l2(g.float(), O.gelu_erf(pre.float().cpu().double()).float().cuda()) < 4e-3, M
        pre_nt, g_nt = ops.gemm_nt(a, w, ops.EPI_GELU, bias=bias)
        same = pre == pre_nt
        assert float(same.float().mean()) > 0.95, M
        assert torch.equal(g[same], g_nt[same]), M
    torch.cuda.synchronize()


def test_decode_refusals(hip):
    w = _randn(20, 768, 768)
    with pytest.raises(lib.VitamdError):
        ops.gemm_skinny(_randn(21, 65, 768), w, ops.EPI_BIAS_BF16)                     # M > 64
    L = lib.load()
    out = torch.empty((65, 768), dtype=BF16, device="cuda")
    a65 = _randn(21, 65, 768)
    assert L.vitamd_gemm_skinny_bf16(a65.data_ptr(), w.data_ptr(), out.data_ptr(), None, None, None, 65, 768, 768, ops.EPI_BIAS_BF16,
                                     None, 0, ops._stream()) == 1                                    # VITAMD_ERR_SHAPE, nothing launched
    assert L.vitamd_gemm_skinny_ws_bytes(65, 768, 768) < 0
    B, H, Lmax = 2, 4, 64
    kc = torch.zeros((B, H, Lmax, 64), dtype=BF16, device="cuda")
    vc = torch.zeros_like(kc)
    length = torch.tensor([60], dtype=torch.int32, device="cuda")
    qkv = _randn(22, B * 5, 3 * H * 64)
    with pytest.raises(lib.VitamdError):
        ops.kv_append(qkv, kc, vc, length, B, 5, H, host_len=60)                   # len + T > Lmax
    with pytest.raises(lib.VitamdError):
        ops.decode_attention(qkv[:B], kc, vc, length, B, H, host_len=Lmax)         # len + 1 > Lmax
    assert L.vitamd_kv_append(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), length.data_ptr(), B, Lmax + 1, H, 64, Lmax, ops._stream()) == 1
    assert L.vitamd_decode_attention(qkv.data_ptr(), kc.data_ptr(), vc.data_ptr(), kc.data_ptr(), length.data_ptr(), B, H, 64, 16385, None, 0,
                                     ops._stream()) == 1
    with pytest.raises(lib.VitamdError):
        ops.gemm_skinny(w.cpu(), w, ops.EPI_BIAS_BF16)                                # CPU tensor
    with pytest.raises(lib.VitamdError):
        ops.kv_append(qkv.cpu(), kc, vc, length, B, 5, H)
    with pytest.raises(lib.VitamdError):
        ops.decode_attention(qkv[:B], kc.cpu(), vc, length, B, H)
    assert bool((kc == 0).all())                                                      # no refused call wrote anything


# ------------------------------------------------------------------------------------------------ cached causal stack
def test_cached_stack_matches_full_sequence_and_oracle(hip):
    import transformer as T
    seed, B, S, P = 5, 2, 256, 100
    cfg = T.S(block_size=S, causal=True)
    sd = W.transformer_state(seed, "", cfg.n_layers, cfg.n_embd, causal_block=S)
    m = T.Transformer(cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    x = W.normal(seed, "x", (B, S, cfg.n_embd))
    xc = x.cuda()
    with torch.no_grad():
        y_full = m(xc).cpu()
    cache = m.new_cache(B)
    assert cache.max_len == S and cache.len == 0
    outs = [m.forward_cached(xc[:, :P], cache)]                           # prefill 100 positions
    for t in range(P, S):                                                   # then one token at a time
        outs.append(m.forward_cached(xc[:, t:t + 1], cache))
    y_cached = torch.cat(outs, dim=1).cpu()
    assert cache.len == S and int(cache.len_dev.item()) == S
    with pytest.raises(ValueError):
        m.forward_cached(xc[:, :1], cache)                                    # full
    y_oracle = O.transformer(x, sd, "", cfg.n_layers, cfg.n_heads, causal=True, lowp=True)
    e_full = O.rel_l2(y_full, y_oracle)
    e_cached = O.rel_l2(y_cached, y_oracle)
    e_cached_decode = O.rel_l2(y_cached[:, P:], y_oracle[:, P:])
    print(f"rel-L2 vs oracle: full {e_full:.2e}, cached {e_cached:.2e} (decoded positions {e_cached_decode:.2e})")
    assert e_cached <= 2 * e_full + 1e-3
    assert e_cached_decode <= 2 * e_full + 1e-3
    assert torch.equal(y_cached[:, :P], m.forward_cached(xc[:, :P], _reset(cache)).cpu())       # reset() + prefill again: same bits


def _reset(cache):
    cache.reset()
    return cache


# ------------------------------------------------------------------------------------------------ VideoGPT
def _videogpt(seed=0, dropout=0.0):
    import train_videogpt as V
    cfg = V.VideoGPTConfig(frame_size=16, codebook_size=256, transformer="S", max_frames=4, dropout=dropout)
    D, Nc = cfg.n_embd, cfg.codebook_size
    sd = {"tok_embed.weight": W.normal(seed, "tok_embed", (Nc + 1, D)), "pos_embed.weight": W.normal(seed, "pos_embed", (cfg.max_tokens, D))}
    sd.update(W.transformer_state(seed, "transformer.", cfg.trans_config.n_layers, D, causal_block=cfg.max_tokens))
    sd.update(W.linear_state(seed, "proj.", Nc, D))
    # a head partly tied to the (shifted) token embeddings: greedy decisions with a clear top-1 / top-2 gap (checked below) instead of
    # the near-ties of a purely random head
    sd["proj.weight"] = sd["proj.weight"] + 0.01 * torch.roll(sd["tok_embed.weight"][:Nc], 1, 0)
    model = V.VideoGPT(cfg)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), sd, cfg


def _oracle_videogpt(x, sd, cfg):
    """fp32 restatement of reference VideoGPT.forward (train_videogpt.py:44-53) on the oracle's bf16-flow transformer"""
    B, T, N = x.shape
    y = x.reshape(B, T * N)
    inp = torch.cat([torch.full((B, 1), cfg.codebook_size, dtype=torch.long), y[:, :-1]], dim=-1)
    e = sd["tok_embed.weight"][inp] + sd["pos_embed.weight"][: T * N]
    h = O.transformer(e, sd, "transformer.", cfg.trans_config.n_layers, cfg.trans_config.n_heads, causal=True, lowp=True)
    logits = O.linear(h, sd["proj.weight"], sd["proj.bias"], lowp=True)
    return logits, O.cross_entropy(logits.reshape(B * T * N, -1), y.reshape(B * T * N))


def test_videogpt_forward_matches_oracle(hip):
    model, sd, cfg = _videogpt()
    x = W.randint(0, "video", (4, cfg.max_frames, cfg.frame_size), cfg.codebook_size)
    logits, loss = model(x.cuda())
    ologits, oloss = _oracle_videogpt(x, sd, cfg)
    assert tuple(logits.shape) == (4, cfg.max_tokens, cfg.codebook_size)
    assert O.rel_l2(logits.detach().cpu(), ologits) < 5e-3
    assert abs(float(loss.detach()) - float(oloss)) < 5e-3


def _teacher_forced_logits(model, seq, cached):
    """fp32 logits (the generate head) at every position of seq [B, S] (SOS first), through the full stack or the cache"""
    B, S = seq.shape
    with torch.no_grad():
        if not cached:
            h = model.transformer(model._embed(seq))
        else:
            cache = model.transformer.new_cache(B, max_len=S)
            P = S // 2
            hs = [model.transformer.forward_cached(model._embed(seq[:, :P]), cache)]
            for t in range(P, S):
                hs.append(model.transformer.forward_cached(model._embed(seq[:, t:t + 1], pos0=t), cache))
            h = torch.cat(hs, dim=1)
        return model._head(h.reshape(B * S, -1)).view(B, S, -1)


def test_videogpt_generate_cached_equals_uncached(hip):
    model, sd, cfg = _videogpt()
    video = W.randint(0, "prompt", (4, 2, cfg.frame_size), cfg.codebook_size).cuda()
    n_frames = 2
    out_cached = model.generate_frames(video, n=n_frames)                          # use_cache=None -> cached (dropout 0)
    out_plain = model.generate_frames(video, n=n_frames, use_cache=False)
    S0, n = 2 * cfg.frame_size, n_frames * cfg.frame_size
    assert tuple(out_cached.shape) == (4, S0 + n)
    assert torch.equal(out_cached[:, :S0], video.reshape(4, S0))                   # prefix preserved
    assert torch.equal(out_cached, out_plain)
    assert torch.equal(model.generate(video.reshape(4, S0), n=3, use_cache=True), out_plain[:, :S0 + 3])
    # margin: at every generated position the uncached top-1 / top-2 gap exceeds 4x the teacher-forced logit error of the cached path
    seq = torch.cat([torch.full((4, 1), cfg.codebook_size, dtype=torch.long, device="cuda"), out_plain[:, :-1]], dim=-1)
    lp = _teacher_forced_logits(model, seq, cached=False)[:, S0:]
    lc = _teacher_forced_logits(model, seq, cached=True)[:, S0:]
    assert torch.equal(lp.argmax(-1), out_plain[:, S0:])
    err = float((lc - lp).abs().max())
    top2 = lp.topk(2, dim=-1).values
    gap = float((top2[..., 0] - top2[..., 1]).min())
    print(f"teacher-forced logit error {err:.3e}, smallest top-1/top-2 gap {gap:.3e}")
    assert O.rel_l2(lc, lp) < 5e-3
    assert gap > 4 * err


def test_videogpt_refusals(hip):
    model, _, cfg = _videogpt(dropout=0.1)
    tokens = W.randint(0, "prompt", (2, 8), cfg.codebook_size).cuda()
    with pytest.raises(ValueError):
        model.generate(tokens, n=2, use_cache=True)                                   # dropout > 0: cache refused
    with pytest.raises(ValueError):
        model.transformer.forward_cached(torch.zeros((2, 1, cfg.n_embd), device="cuda"), None)
    out = model.generate(tokens, n=2)                                                 # None -> the uncached loop
    assert tuple(out.shape) == (2, 10) and torch.equal(out[:, :8], tokens)
    model, _, cfg = _videogpt()
    with pytest.raises(ValueError):
        model.generate(tokens, n=cfg.max_tokens - 8 + 1)                              # more than max_tokens positions
    with pytest.raises(ValueError):
        model.generate(tokens, n=cfg.max_tokens - 8 + 1, use_cache=False)
    assert tuple(model.generate(tokens, n=cfg.max_tokens - 8).shape) == (2, cfg.max_tokens)
