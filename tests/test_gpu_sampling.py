"""Sampled generation on a real MI355X: the sampling kernel through ops.sample_logits (every row's decision verified in float64 by
_sampling_ref.check_rows, see there and include/vitamd.h for the semantics), the Philox stream, the distribution of the draws, the absence
of host synchronisation, and VideoGPT.generate with temperature / top-k / top-p on the cached and the uncached loop.

Worst excess over the exact float64 boundaries measured on MI355X (printed by the kernel tests; bound: _sampling_ref.EPS = 2e-5): see
DESIGN.md section 10.1."""
import numpy as np
import pytest
import torch

import _sampling_ref as R
import weights as W
from vitamd import lib, ops
from vitamd.sampling import Sampler

pytestmark = pytest.mark.gpu
F32 = torch.float32
PARAMS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (1.3, 100, 0.95), (0.5, 0, 0.5), (1.0, "V", 1.0), (1.0, 0, 1e-6)]
VS = (2, 64, 1000, 1024, 16384, 65536)
BS = (1, 32, 257)
SPREADS = (1, 3, 8)
U_FIXED = (0.0, 0.5, 1 - 2.0 ** -24)


def _case_rows(V, B, spread, tag):
    """logits [B, V] with a block of -inf in some rows, and u: 0, 0.5, 1 - 2^-24 on the first rows (one of them when B = 1), else random"""
    x = R.logits(7, f"logits{tag}", (B, V), spread)
    for r in range(B):
        if r % 5 == 1 or (B == 1 and tag % 4 == 3):
            if V >= 4:
                x[r, V // 4:V // 2] = -np.inf
            else:
                x[r, r % V] = -np.inf
    rng = np.random.Generator(np.random.PCG64([7, tag]))
    u = rng.random(B, dtype=np.float32)
    u = np.minimum(u, np.float32(1 - 2.0 ** -24))
    if B == 1:
        if tag % 4 < 3:
            u[0] = U_FIXED[tag % 4]
    else:
        u[:3] = U_FIXED
        u[5:8] = U_FIXED            # with rows 6 (r % 5 == 1) carrying the -inf block
    return x, u


def _run_and_check(x, u, T, k, p, ld=None):
    B, V = x.shape
    xd = torch.from_numpy(x).cuda()
    if ld is not None:
        buf = torch.full((B, ld), float("nan"), dtype=F32, device="cuda")     # what lies between the rows must not matter
        buf[:, :V] = xd
        xd = buf[:, :V]
        assert xd.stride(0) == ld
    tok, info = ops.sample_logits(xd, T, k, p, u=torch.from_numpy(u).cuda(), return_info=True)
    tok2, info2 = ops.sample_logits(xd, T, k, p, u=torch.from_numpy(u).cuda(), return_info=True)
    assert tok.dtype == torch.int64 and tuple(tok.shape) == (B,) and tuple(info.shape) == (B, 4)
    assert torch.equal(tok, tok2) and torch.equal(info, info2)                  # the same bits on every call
    assert torch.equal(tok, ops.sample_logits(xd, T, k, p, u=torch.from_numpy(u).cuda()))      # with or without info
    tok, info = tok.cpu().numpy(), info.cpu().numpy()
    excess = R.check_rows(x, R.f32(T), k, R.f32(p), u, tok, info)
    zero = np.flatnonzero(u == 0)
    if zero.size:                                                                # u = 0: the lowest index of the kept set
        S = x[zero] >= info[zero, 0:1]
        assert (tok[zero] == S.argmax(1)).all()
    return excess


@pytest.mark.parametrize("V", VS)
def test_kernel_decisions_hold_in_float64(hip, V):
    worst = -1.0
    for pi, (T, k, p) in enumerate(PARAMS):
        k = V if k == "V" else k
        vi = VS.index(V)
        # every (V, parameter set) pair; batch sizes and spreads rotate so that every V meets every B and every spread
        for j in range(2 if V <= 1024 else 1):
            B, spread = BS[(vi + pi + j) % 3], SPREADS[(vi + 2 * pi + j) % 3]
            tag = (vi * 7 + pi) * 2 + j
            x, u = _case_rows(V, B, spread, tag)
            e = _run_and_check(x, u, T, k, p)
            print(f"V={V} B={B} spread={spread} T={T} top_k={k} top_p={p}: worst excess {e:.3e}")
            worst = max(worst, e)
    print(f"V={V}: worst excess over the float64 boundaries {worst:.3e} (bound {R.EPS})")


def test_kernel_every_batch_size_at_the_largest_row_and_a_padded_row_stride(hip):
    worst = -1.0
    for B, spread, (T, k, p) in ((1, 8, PARAMS[3]), (32, 1, PARAMS[4]), (257, 3, PARAMS[3]), (257, 8, PARAMS[2])):
        x, u = _case_rows(65536, B, spread, 100 + B)
        worst = max(worst, _run_and_check(x, u, T, k, p))
    for V, ld in ((1000, 1003), (16384, 16400), (65536, 65540), (2, 5)):
        x, u = _case_rows(V, 32, 3, 200 + V % 97)
        worst = max(worst, _run_and_check(x, u, 1.3, 100, 0.95, ld=ld))
    print(f"worst excess over the float64 boundaries {worst:.3e} (bound {R.EPS})")


def test_top_k_1_is_argmax(hip):
    for V in (2, 64, 1000, 16384, 65536):
        x = R.logits(8, f"argmax{V}", (64, V), 3)
        srt = np.sort(x, axis=1)
        assert (srt[:, -1] > srt[:, -2]).all()                                  # rows without a tied maximum
        xd = torch.from_numpy(x).cuda()
        for u in (0.0, 0.37, 1 - 2.0 ** -24):
            tok = ops.sample_logits(xd, 0.8, 1, 1.0, u=torch.full((64,), u, dtype=F32, device="cuda"))
            assert torch.equal(tok, torch.argmax(xd, dim=-1))
        tok = ops.sample_logits(xd, 1.0, 1, 0.3, seed=5)
        assert torch.equal(tok, torch.argmax(xd, dim=-1))


def test_ties_with_the_kth_value_are_all_kept(hip):
    V = 1000
    x = R.logits(9, "ties", (6, V), 1)
    top = x.max() + 1
    where = [3, 400, 401, 999]
    x[:, where] = top                                                           # the maximum four times
    xd = torch.from_numpy(x).cuda()
    us = np.array([0.0, 0.2499, 0.2501, 0.6, 0.7501, 1 - 2.0 ** -24], dtype=np.float32)
    tok, info = ops.sample_logits(xd, 1.0, 1, 1.0, u=torch.from_numpy(us).cuda(), return_info=True)
    tok, info = tok.cpu().numpy(), info.cpu().numpy()
    assert (info[:, 1] == 4).all() and (info[:, 0] == top).all()
    assert tok.tolist() == [3, 3, 400, 401, 999, 999]
    R.check_rows(x, 1.0, 1, 1.0, us, tok, info)
    x[:, 500] = top - 0.5                                                       # top_k = 3 lands inside the tie: still the four copies
    tok, info = ops.sample_logits(torch.from_numpy(x).cuda(), 1.0, 3, 1.0, u=torch.from_numpy(us).cuda(), return_info=True)
    assert (info[:, 1].cpu().numpy() == 4).all() and tok.cpu().tolist() == [3, 3, 400, 401, 999, 999]


def test_negative_zero_ties_with_zero(hip):
    x = -np.abs(R.logits(9, "zeros", (2, 64), 1)) - 1
    x[:, 5], x[:, 9] = -0.0, 0.0                                               # equal as numbers: one tie of two
    us = np.array([0.0, 0.9], dtype=np.float32)
    tok, info = ops.sample_logits(torch.from_numpy(x).cuda(), 1.0, 1, 1.0, u=torch.from_numpy(us).cuda(), return_info=True)
    tok, info = tok.cpu().numpy(), info.cpu().numpy()
    assert tok.tolist() == [5, 9] and (info[:, 1] == 2).all() and (info[:, 0] == 0).all()
    R.check_rows(x, 1.0, 1, 1.0, us, tok, info)


def test_philox_stream(hip):
    B, V = 257, 1024
    x = R.logits(10, "philox", (B, V), 3)
    xd = torch.from_numpy(x).cuda()
    seed = 0x1234_5678_9ABC_DEF0
    sampler = Sampler(1.3, 100, 0.95, seed=seed)
    outs = []
    for step in range(3):
        tok, info = sampler(xd, return_info=True)
        assert sampler.step == step + 1 and int(sampler.step_dev.cpu().view(torch.int64).item()) == step + 1      # advances by one per call
        u = R.philox_u(seed, B, step)
        R.check_rows(x, R.f32(1.3), 100, R.f32(0.95), u, tok.cpu().numpy(), info.cpu().numpy())
        outs.append((tok, info))
    assert not torch.equal(outs[0][0], outs[1][0]) and not torch.equal(outs[1][0], outs[2][0])          # another step, other tokens
    # the same seed and step: the same tokens, bit for bit, through the op and through a second sampler
    step1 = torch.tensor([1], dtype=torch.int64, device="cuda").view(torch.uint64)
    tok, info = ops.sample_logits(xd, 1.3, 100, 0.95, seed=seed, step=step1, return_info=True)
    assert torch.equal(tok, outs[1][0]) and torch.equal(info, outs[1][1])
    again = Sampler(1.3, 100, 0.95, seed=seed)
    assert torch.equal(again(xd), outs[0][0]) and torch.equal(again(xd), outs[1][0])
    again.reset(2)
    assert torch.equal(again(xd), outs[2][0])
    assert torch.equal(ops.sample_logits(xd, 1.3, 100, 0.95, seed=seed), outs[0][0])                        # step=None is step 0
    assert not torch.equal(Sampler(1.3, 100, 0.95, seed=seed + 1)(xd), outs[0][0])                        # another seed
    # a step beyond 2^32 uses the high counter word
    big = (1 << 32) + 5
    stepb = torch.tensor([big], dtype=torch.int64, device="cuda").view(torch.uint64)
    tok, info = ops.sample_logits(xd, 1.0, 0, 1.0, seed=seed, step=stepb, return_info=True)
    R.check_rows(x, 1.0, 0, 1.0, R.philox_u(seed, B, big), tok.cpu().numpy(), info.cpu().numpy())
    # identical rows in one batch: the row index is part of the counter
    same = xd[:1].repeat(64, 1)
    assert len(set(ops.sample_logits(same, 1.0, 0, 1.0, seed=seed).cpu().tolist())) > 16


@pytest.mark.parametrize("top_k", [0, 8])
def test_distribution_of_the_draws(hip, top_k):
    from scipy import stats
    V, B = 64, 65536
    x = R.logits(12, "dist", (1, V), 2)
    S, q, _ = R.kept_set(x[0], 1.0, top_k, 1.0)
    assert int(S.sum()) == (8 if top_k else V)
    xd = torch.from_numpy(x).cuda().repeat(B, 1)
    tok = ops.sample_logits(xd, 1.0, top_k, 1.0, seed=2024).cpu().numpy()
    counts = np.bincount(tok, minlength=V).astype(np.float64)
    assert counts[~S].sum() == 0
    order = np.argsort(q)                                           # merge the bins with an expected count < 5, smallest first
    exp_sorted, cnt_sorted = (q * B)[order], counts[order]
    keep = exp_sorted > 0
    exp_sorted, cnt_sorted = exp_sorted[keep], cnt_sorted[keep]
    bins_e, bins_c, acc_e, acc_c = [], [], 0.0, 0.0
    for e, c in zip(exp_sorted, cnt_sorted):
        acc_e, acc_c = acc_e + e, acc_c + c
        if acc_e >= 5:
            bins_e.append(acc_e); bins_c.append(acc_c)
            acc_e = acc_c = 0.0
    if acc_e > 0:
        bins_e[-1] += acc_e; bins_c[-1] += acc_c
    bins_e, bins_c = np.array(bins_e), np.array(bins_c)
    chi2 = float(((bins_c - bins_e) ** 2 / bins_e).sum())
    bound = float(stats.chi2.ppf(1 - 1e-6, len(bins_e) - 1))
    print(f"top_k={top_k}: chi-square {chi2:.2f} over {len(bins_e)} bins, bound {bound:.2f}")
    assert chi2 < bound


def test_no_host_synchronisation(hip):
    x = torch.from_numpy(R.logits(13, "nosync", (32, 1024), 3)).cuda()
    u = torch.full((32,), 0.5, dtype=F32, device="cuda")
    sampler = Sampler(0.9, 50, 0.9, seed=1)
    ops.sample_logits(x, 0.9, 50, 0.9)                                 # library loaded, code object resident
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = ops.sample_logits(x, 0.9, 50, 0.9, u=u, return_info=True)
        b = ops.sample_logits(x, 0.9, 50, 0.9, seed=1)
        c = sampler(x)
        d = sampler(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(b, c) and not torch.equal(c, d) and a[0].shape == c.shape


def test_refusals_on_the_device(hip):
    x = torch.zeros((4, 1024), device="cuda")
    with pytest.raises(ValueError):
        ops.sample_logits(x, 0.0)
    with pytest.raises(lib.VitamdError):
        ops.sample_logits(x.double())
    with pytest.raises(lib.VitamdError):
        ops.sample_logits(x.t())                                       # inner stride != 1
    with pytest.raises(lib.VitamdError):
        ops.sample_logits(x, u=torch.zeros(3, device="cuda"))
    L = lib.load()
    tok = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    assert L.vitamd_sample_logits(x.data_ptr(), tok.data_ptr(), None, None, None, 4, 1, 1, 1.0, 0, 1.0, 0, ops._stream()) == 1
    assert L.vitamd_sample_logits(x.data_ptr(), tok.data_ptr(), None, None, None, 4, 1024, 1024, 0.0, 0, 1.0, 0, ops._stream()) == 2
    torch.cuda.synchronize()
    assert bool((tok == -1).all())                                     # no refused call wrote anything


# ------------------------------------------------------------------------------------------------ VideoGPT (the preset-S fixture of test_gpu_decode.py)
def _videogpt(seed=0):
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


def test_videogpt_top_k_1_equals_greedy(hip):
    model, cfg = _videogpt()
    video = W.randint(0, "prompt", (4, 2, cfg.frame_size), cfg.codebook_size).cuda()
    greedy = model.generate_frames(video, n=2)
    S0, n = 2 * cfg.frame_size, 2 * cfg.frame_size
    for use_cache in (None, False):
        out = model.generate_frames(video, n=2, use_cache=use_cache, top_k=1, seed=9)
        assert tuple(out.shape) == (4, S0 + n) and out.dtype == greedy.dtype
        assert torch.equal(out[:, :S0], video.reshape(4, S0))                      # prefix preserved
        assert torch.equal(out, greedy), use_cache
    assert torch.equal(model.generate(video.reshape(4, S0), n=3, use_cache=True, top_k=1, temperature=0.5), greedy[:, :S0 + 3])


def test_videogpt_sampled_generation(hip):
    model, cfg = _videogpt()
    S0, n = 2 * cfg.frame_size, 2 * cfg.frame_size
    prompt = W.randint(0, "prompt", (1, 2, cfg.frame_size), cfg.codebook_size).cuda().repeat(4, 1, 1)      # four identical prompts
    kw = dict(temperature=1.0, top_k=20)
    out = model.generate_frames(prompt, n=2, seed=3, **kw)
    assert tuple(out.shape) == (4, S0 + n) and out.dtype == torch.int64
    assert torch.equal(out[:, :S0], prompt.reshape(4, S0))
    assert torch.equal(out, model.generate_frames(prompt, n=2, seed=3, **kw))                              # one seed, one continuation
    assert not torch.equal(out, model.generate_frames(prompt, n=2, seed=4, **kw))
    assert len({tuple(r) for r in out[:, S0:].cpu().tolist()}) == 4                                       # four different continuations
    plain = model.generate_frames(prompt, n=2, seed=3, use_cache=False, **kw)
    assert tuple(plain.shape) == (4, S0 + n) and torch.equal(plain[:, :S0], prompt.reshape(4, S0))
    assert torch.equal(plain, model.generate_frames(prompt, n=2, seed=3, use_cache=False, **kw))
    assert len({tuple(r) for r in plain[:, S0:].cpu().tolist()}) == 4
    nucleus = model.generate_frames(prompt, n=1, seed=3, temperature=0.8, top_p=0.9)
    assert tuple(nucleus.shape) == (4, S0 + cfg.frame_size) and int(nucleus.max()) < cfg.codebook_size and int(nucleus.min()) >= 0
    # every generated token lies in the top 20 of its teacher-forced row, up to 4x the logit difference between the two paths
    for seqs in (out, plain):
        seq = torch.cat([torch.full((4, 1), cfg.codebook_size, dtype=torch.long, device="cuda"), seqs[:, :-1]], dim=-1)
        lp = _teacher_forced_logits(model, seq, cached=False)[:, S0:]
        lc = _teacher_forced_logits(model, seq, cached=True)[:, S0:]
        err = float((lc - lp).abs().max())
        kth = lp.topk(20, dim=-1).values[..., -1]
        chosen = lp.gather(-1, seqs[:, S0:].unsqueeze(-1)).squeeze(-1)
        slack = float((kth - chosen).max())
        print(f"teacher-forced logit difference cached / uncached {err:.3e}; chosen logit below the 20th largest by at most {slack:.3e}")
        assert bool((chosen >= kth - 4 * err).all())
