"""CPU reference for attention under dropout and causal masks (torch + numpy), written from the contract in csrc/attention.hip's
header and csrc/common.h, independent of the kernel text:

    S = q k^T / 8 (+ -inf above the diagonal when causal);  P = softmax(S);  o = (P o M) v;  lse2 = log2(sum exp(S))
    M[b, h, q, k] = keep(((b*H + h)*N + q)*N + k, seed, p) / (1 - p)           (tests/_dropout_ref.py)
    dP = dO v^T;  delta = rowsum(dO o o);  dS = P o (dP o M - delta);  dq = dS k / 8;  dk = dS^T q / 8;  dv = (P o M)^T dO

ref64()    fp64 throughout, gradients by autograd with M held fixed.
restate()  the same function with bf16 roundings where the kernels round: exp(s - m) o M before the PV product (the normaliser l is the
           fp32 sum BEFORE the mask and before the rounding), o, delta from the bf16 o, P o M before the dV product, dS before the dQ / dK
           products, and the three gradient outputs.  online=True does it in fp32 with a running maximum over 32-key tiles.
The distance restate <-> ref64 is the bf16 floor the kernels are held to (bounds(), compare()); worst_tile() is the same distance per
(batch, head, 32-row tile), so that one wrong tile of a long sequence is not diluted.  MUTANTS are the deliberate mistakes
test_attention_ref_host.py proves the GPU tests would catch; the probe_* / decode_* functions make every keep decision of each of the
three dropout consumers (forward, dQ kernel, dK/dV kernel) visible in an output.  long_* are row-chunked forms for N = 16 384 that never
hold an N x N matrix.  MATRIX / PROBE_CASES / SPIKE_CASES are the cases of tests/test_gpu_attention_matrix.py, shared with the host test.
FORM_CASES (last section) are the cases of tests/test_gpu_attention_forms.py: every kernel instantiation a call can reach, at both edges of
its tile count; coverage_gaps() is the rule tests/test_attention_forms_host.py proves from the library's own vitamd_attention_form."""
import functools
import math

import numpy as np
import torch

import _dropout_ref as DR

BF16 = torch.bfloat16
SCALE = 0.125
LOG2E = 1.4426950408889634
TILE = 32
NEG_BIG = -1.0e30
SEED = (1 << 40) + 777           # bit 40 set: the high seed word is live


def r16(x):
    """round to bf16, keep the dtype"""
    return x.to(BF16).to(x.dtype)


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ------------------------------------------------------------------------------------------ layout
def split(qkv, B, N, H):
    """[B*N, 3*H*64] -> q, k, v [B, H, N, 64]"""
    t = qkv.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def heads(x, B, N, H):
    """[B*N, H*64] -> [B, H, N, 64]"""
    return x.view(B, N, H, 64).permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------------ mask
def keep_scale(idx, p, seed):
    """uint64 index array -> fp32 keep-scale (0 or 1/(1-p))"""
    if DR.thresh(p) == 0:
        return np.ones(np.shape(idx), dtype=np.float32)
    return DR.keep(idx, seed, p).astype(np.float32) * DR.scale(p)


def mask_rows(bhs, N, p, seed, q0=0, q1=None, keys=None):
    """keep-scale of (bh, query, key) for bh in bhs, q0 <= query < q1, key in keys (default all): fp32 [len(bhs), q1 - q0, len(keys)];
    built in row chunks of at most 4M decisions"""
    q1 = N if q1 is None else q1
    keys = np.arange(N, dtype=np.uint64) if keys is None else np.asarray(keys, dtype=np.uint64)
    bhs = list(bhs)
    out = torch.empty((len(bhs), q1 - q0, len(keys)), dtype=torch.float32)
    step = max(1, (1 << 22) // max(1, len(keys)))
    for i, bh in enumerate(bhs):
        for r0 in range(q0, q1, step):
            r1 = min(q1, r0 + step)
            rows = np.arange(r0, r1, dtype=np.uint64)
            idx = ((np.uint64(bh) * np.uint64(N) + rows) * np.uint64(N))[:, None] + keys[None, :]
            out[i, r0 - q0:r1 - q0] = torch.from_numpy(keep_scale(idx, p, seed))
    return out


def mask(B, H, N, p, seed):
    """[B, H, N, N] fp32: keep(((bh*N + q)*N + k), seed, p) * scale(p)"""
    return mask_rows(range(B * H), N, p, seed).view(B, H, N, N)


def allowed(N, causal):
    a = torch.ones(N, N, dtype=torch.bool)
    return torch.tril(a) if causal else a


# ------------------------------------------------------------------------------------------ fp64 reference
def ref64(q, k, v, d_o, M, causal):
    """q, k, v, d_o [B, H, N, 64] (bf16-representable), M [B, H, N, N] or None -> dict of fp64 o, lse (log2 domain), dq, dk, dv"""
    q, k, v = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    N = q.shape[-2]
    s = (q @ k.transpose(-1, -2)) * SCALE
    if causal:
        s = s.masked_fill(~allowed(N, True), float("-inf"))
    P = torch.softmax(s, -1)
    o = (P if M is None else P * M.double()) @ v
    o.backward(d_o.double())
    return {"o": o.detach(), "lse": torch.logsumexp(s.detach(), -1) * LOG2E, "dq": q.grad, "dk": k.grad, "dv": v.grad}


# ------------------------------------------------------------------------------------------ restatement with the kernels' roundings
def _masks(M, like):
    """M: None, one tensor, or {"fwd", "dq", "dkv"} (one mask per consumer) -> three tensors of like's dtype"""
    if M is None:
        one = torch.ones((), dtype=like.dtype)
        return one, one, one
    if isinstance(M, dict):
        return tuple(M[c].to(like.dtype) for c in ("fwd", "dq", "dkv"))
    M = M.to(like.dtype)
    return M, M, M


def restate(q, k, v, d_o, M, causal, online=False, flags=()):
    """Same signature and result as ref64, with bf16 roundings where the kernels round.  M may be a dict of one mask per consumer.
    flags: arithmetic mutations (see MUTANTS), plain form only."""
    if online:
        assert not flags
        return _restate_online(q, k, v, d_o, M, causal)
    q, k, v, d_o = (t.double() for t in (q, k, v, d_o))
    N = q.shape[-2]
    Mf, Mq, Mkv = _masks(M, q)
    al = allowed(N, causal)
    if "causal_lt" in flags:                            # diagonal excluded: row 0 attends to nothing and comes out as zeros
        al = torch.tril(al, -1) if causal else al
    al_q, al_kv = al, al
    if "diag_unmasked_dkv" in flags and causal:         # dK / dV only: the whole diagonal 32 x 32 tile admitted
        t = torch.arange(N) // TILE
        al_kv = al | (t[:, None] == t[None, :])
    s = (q @ k.transpose(-1, -2)) * SCALE
    # ---- forward
    vf, Mff, s_f = v, Mf, s.masked_fill(~al, float("-inf"))
    if "pad_keys" in flags and not causal and N % TILE:  # the staged copies of key N-1 that fill the last tile take part
        pad = TILE - N % TILE
        vf = torch.cat([v, v[..., -1:, :].expand(*v.shape[:-2], pad, 64)], -2)
        s_f = torch.cat([s_f, s_f[..., -1:].expand(*s.shape[:-1], pad)], -1)
        if Mf.dim():
            Mff = torch.cat([Mf, Mf[..., -1:].expand(*Mf.shape[:-1], pad)], -1)
    m = s_f.amax(-1, keepdim=True)
    e = torch.exp(s_f - m)
    l = (e * Mff).sum(-1, keepdim=True) if "l_after_mask" in flags else e.sum(-1, keepdim=True)
    o = r16((r16(e * Mff) @ vf) / l)
    lse = m + torch.log(l)
    if "causal_lt" in flags:                            # the empty row: o = 0, and lse = +inf makes its P zero in backward
        o = torch.nan_to_num(o, nan=0.0)
        lse = torch.where(torch.isnan(lse), torch.full_like(lse, float("inf")), lse)
    # ---- backward
    o_d = r16((r16(e) @ vf) / l) if "delta_pre_dropout" in flags else o
    delta = (d_o * o_d).sum(-1, keepdim=True)
    P_q = torch.exp(s.masked_fill(~al_q, float("-inf")) - lse)       # masked before the exp: a masked score may exceed the row's lse by far
    P_k = torch.exp(s.masked_fill(~al_kv, float("-inf")) - lse)
    dP = d_o @ v.transpose(-1, -2)
    dS_q = r16(P_q * ((dP if "dq_no_keep" in flags else dP * Mq) - delta))
    dS_k = r16(P_k * (dP * Mkv - delta))
    PM = r16(P_k if "dv_no_keep" in flags else P_k * Mkv)
    out = {"o": o, "lse": lse.squeeze(-1) * LOG2E, "dq": r16(dS_q @ k * SCALE), "dk": r16(dS_k.transpose(-1, -2) @ q * SCALE),
           "dv": r16(PM.transpose(-1, -2) @ d_o)}
    if "causal_lt" in flags:
        out = {n: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0) for n, t in out.items()}
    return out


def _restate_online(q, k, v, d_o, M, causal):
    """fp32, the kernels' order: per 32-key tile  m' = max(m, max(s) c);  p = exp2(s c - m');  l = l alpha + sum p;  O = O alpha + bf16(p o M) v"""
    q, k, v, d_o = (t.float() for t in (q, k, v, d_o))
    N = q.shape[-2]
    Mf, Mq, Mkv = _masks(M, q)
    al = allowed(N, causal)
    c = torch.tensor(SCALE * LOG2E, dtype=torch.float32)
    s = q @ k.transpose(-1, -2)
    m = torch.full(q.shape[:-1] + (1,), NEG_BIG, dtype=torch.float32)
    l = torch.zeros_like(m)
    acc = torch.zeros_like(q)
    for k0 in range(0, N, TILE):
        k1 = min(N, k0 + TILE)
        st = s[..., k0:k1].masked_fill(~al[:, k0:k1], NEG_BIG)
        mn = torch.maximum(m, st.amax(-1, keepdim=True) * c)
        alpha = torch.exp2(m - mn)
        pe = torch.exp2(st * c - mn)
        l = l * alpha + pe.sum(-1, keepdim=True)
        acc = acc * alpha + r16(pe * (Mf[..., k0:k1] if Mf.dim() else Mf)) @ v[..., k0:k1, :]
        m = mn
    o = r16(acc / l)
    lse2 = m + torch.log2(l)
    delta = (d_o * o).sum(-1, keepdim=True)
    P = torch.exp2((s * c).masked_fill(~al, float("-inf")) - lse2)
    dP = d_o @ v.transpose(-1, -2)
    dS_q = r16(P * (dP * Mq - delta))
    dS_k = r16(P * (dP * Mkv - delta))
    PM = r16(P * Mkv)
    return {"o": o, "lse": lse2.squeeze(-1), "dq": r16(dS_q @ k * SCALE), "dk": r16(dS_k.transpose(-1, -2) @ q * SCALE),
            "dv": r16(PM.transpose(-1, -2) @ d_o)}


# ------------------------------------------------------------------------------------------ metric and bounds
def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def worst_tile(x, ref):
    """worst rel_l2 over (batch, head, 32-row tile) of a [..., N, 64] tensor"""
    x, ref = x.double(), ref.double()
    N = ref.shape[-2]
    pad = -N % TILE
    if pad:
        z = torch.zeros(ref.shape[:-2] + (pad, ref.shape[-1]), dtype=torch.float64)
        x, ref = torch.cat([x, z], -2), torch.cat([ref, z], -2)
    d = (x - ref).reshape(*ref.shape[:-2], -1, TILE * ref.shape[-1]).norm(dim=-1)
    n = ref.reshape(*ref.shape[:-2], -1, TILE * ref.shape[-1]).norm(dim=-1)
    return float((d / n.clamp_min(1e-30)).max())


GLOBAL_MARGIN, TILE_MARGIN, LSE_TOL = 1.5, 2.0, 1.0e-6
OUTS = ("o", "dq", "dk", "dv")


def floors(ref, rs, names=OUTS):
    """{name: (global floor, worst-tile floor)} from the reference alone"""
    return {n: (rel_l2(rs[n], ref[n]), worst_tile(rs[n], ref[n])) for n in names}


def compare(got, ref, fl):
    """-> ({name: (global error / floor, worst tile / tile floor)}, [failures]); a zero floor admits only a zero error"""
    ratios, bad = {}, []
    for n, (fg, ft) in fl.items():
        eg, et = rel_l2(got[n], ref[n]), worst_tile(got[n], ref[n])
        ratios[n] = (eg / fg if fg > 0 else (0.0 if eg == 0 else math.inf), et / ft if ft > 0 else (0.0 if et == 0 else math.inf))
        if not eg <= GLOBAL_MARGIN * fg:
            bad.append(f"{n}: rel_l2 {eg:.3e} > {GLOBAL_MARGIN} x floor {fg:.3e}")
        if not et <= TILE_MARGIN * ft:
            bad.append(f"{n}: worst tile {et:.3e} > {TILE_MARGIN} x tile floor {ft:.3e}")
    if "lse" in got:
        e = rel_l2(got["lse"], ref["lse"])
        ratios["lse"] = (e, e)
        if not e <= LSE_TOL:
            bad.append(f"lse: rel_l2 {e:.3e} > {LSE_TOL}")
    return ratios, bad


def one_key_residue(got, ref_in):
    """N = 1: the fp64 dq and dk are exactly zero; what a one-ulp bf16 rounding of o leaves in delta bounds them.  -> [failures]"""
    q, k, v, d_o = ref_in
    bad = []
    lim = 2.0 ** -8 * (d_o.double() * got["o"].double()).abs().sum(-1, keepdim=True) * SCALE
    for n, other in (("dq", k), ("dk", q)):
        x = got[n].double()
        if not bool(torch.isfinite(x).all()):
            bad.append(f"{n}: not finite")
        elif not bool((x.abs() <= lim * other.double().abs().max()).all()):
            bad.append(f"{n}: |{n}| {float(x.abs().max()):.3e} above the delta residue")
    return bad


# ------------------------------------------------------------------------------------------ the cases
# (B, N, H, causal, p): the kernel family each reaches is MATRIX_FAMILIES below (asked of vitamd_attention_form by the tests)
MATRIX = [(2, 1, 2, True, 0.0), (2, 1, 2, True, 0.3), (2, 5, 1, False, 0.5), (1, 32, 2, True, 0.3),
          (2, 37, 2, True, 0.3), (2, 37, 2, False, 0.3), (1, 197, 2, True, 0.3), (1, 197, 2, False, 0.3),
          (2, 256, 1, True, 0.1), (2, 256, 1, False, 0.5),
          (1, 257, 2, True, 0.0), (1, 257, 2, True, 0.3), (1, 257, 2, False, 0.3), (1, 300, 2, True, 0.0),
          (1, 512, 1, True, 0.0), (1, 512, 1, True, 0.1),
          (1, 513, 1, True, 0.3), (1, 513, 1, False, 0.3), (1, 1056, 2, True, 0.3), (1, 1056, 2, False, 0.1)]
PROBE_CASES = [(N, causal) for N in (70, 197, 300, 600) for causal in (False, True)]
PROBE_B, PROBE_H, PROBE_P = 2, 2, 0.3
SPIKE_CASES = [(300, 290), (600, 550)]          # (N, dominating key): a late tile of attn_fwd_kernel, the second chunk of the long kernels
LONG_N = 16384
LONG_TILES = (0, 15, 16, 255, 256, 259, 260, 511)   # first, last, both sides of the 512-row chunk edges at 512 and 8192 and of the y-block edge at 8320


def case_id(c):
    B, N, H, causal, p = c
    return f"B{B}-N{N}-H{H}-{'causal' if causal else 'full'}-p{p}"


def matrix_inputs(c):
    """qkv [B*N, 3*H*64], d_o [B*N, H*64] fp32 holding bf16 values; the seed is the case's own"""
    B, N, H, causal, p = c
    seed = 5000 + 16 * N + 4 * B + 2 * int(causal) + int(p * 10) * 1000
    return r16(randn((B * N, 3 * H * 64), seed, 1.5)), r16(randn((B * N, H * 64), seed + 1))


def spike_inputs(N, key):
    """test_attention_softmax_spike's construction: `key` aligned with query 10, x 40"""
    qkv = r16(randn((N, 3 * 64), 77 + N, 0.5))
    qkv[key, 64:128] = r16(qkv[10, 0:64] * 40.0)
    return qkv, r16(randn((N, 64), 78 + N))


def _reference(qkv, d_o, B, N, H, causal, p, seed):
    q, k, v = split(qkv, B, N, H)
    g = heads(d_o, B, N, H)
    M = mask(B, H, N, p, seed) if p > 0 else None
    ref = ref64(q, k, v, g, M, causal)
    rs = restate(q, k, v, g, M, causal)
    return {"in": (q, k, v, g), "M": M, "ref": ref, "restate": rs, "floors": floors(ref, rs)}


@functools.lru_cache(maxsize=None)
def matrix_reference(c):
    """computed once per case and shared; treat as read-only"""
    B, N, H, causal, p = c
    return _reference(*matrix_inputs(c), B, N, H, causal, p, SEED)


@functools.lru_cache(maxsize=None)
def spike_reference(N, key, causal):
    return _reference(*spike_inputs(N, key), 1, N, 1, causal, 0.0, 0)


def kernel_outputs(o, lse, dqkv, B, N, H):
    """o [B*N, H*64], lse [B, H, N], dqkv [B*N, 3*H*64] (CPU) -> the dict compare() takes"""
    dq, dk, dv = split(dqkv.float(), B, N, H)
    return {"o": heads(o.float(), B, N, H), "lse": lse, "dq": dq, "dk": dk, "dv": dv}


# ------------------------------------------------------------------------------------------ mutants
def _m_swap(B, H, N, p, seed):
    return mask(B, H, N, p, seed).transpose(-1, -2).contiguous()


def _m_h_only(B, H, N, p, seed):
    return mask(1, H, N, p, seed).expand(B, H, N, N).contiguous()


def _m_last_key(B, H, N, p, seed):
    M = mask(B, H, N, p, seed)
    rows = np.arange(B * H * N, dtype=np.uint64)
    M[..., N - 1] = torch.from_numpy(keep_scale(rows * np.uint64(N) + np.uint64(N), p, seed)).view(B, H, N)
    return M


# name -> (mask builder or None, restate flag or None)
MUTANTS = {
    "mask indexed (k, q)": (_m_swap, None),
    "bh taken as h alone": (_m_h_only, None),
    "keep-scale left off dP in dQ": (None, "dq_no_keep"),
    "keep-scale left off P in dV": (None, "dv_no_keep"),
    "l summed after the mask": (None, "l_after_mask"),
    "causal diagonal excluded": (None, "causal_lt"),
    "diagonal tile unmasked in dK/dV": (None, "diag_unmasked_dkv"),
    "padded keys of the last tile admitted": (None, "pad_keys"),
    "mask of the last key taken from key N": (_m_last_key, None),
    "delta from the pre-dropout o": (None, "delta_pre_dropout"),
}


def mutant_outputs(name, c):
    """restate() of matrix case c with one mutation"""
    B, N, H, causal, p = c
    r = matrix_reference(c)
    build, flag = MUTANTS[name]
    M = r["M"]
    if build is not None and p > 0:
        M = build(B, H, N, p, SEED)
    return restate(*r["in"], M, causal, flags=(flag,) if flag else ())


# ------------------------------------------------------------------------------------------ mask probes
# q = k = 0 makes P uniform over the n_q keys a row sees, so one output element carries one keep decision.  Block j covers keys
# (forward, dQ) or queries (dK/dV) 64j .. 64j + 63; ceil(N / 64) launches recover the whole [N, N] pattern.
def n_blocks(N):
    return (N + 63) // 64


def _onehot_rows(t, j, N):
    """t [B, N, H, 64] view: t[:, 64j + c, :, c] = 1"""
    for c in range(min(64, N - 64 * j)):
        t[:, 64 * j + c, :, c] = 1.0


def probe_inputs(kind, B, N, H, j):
    """kind 'fwd' | 'dkv' | 'dq' -> (qkv [B*N, 3*H*64], d_o [B*N, H*64]) fp32"""
    qkv = torch.zeros(B * N, 3 * H * 64)
    d_o = torch.zeros(B * N, H * 64)
    t = qkv.view(B, N, 3, H, 64)
    if kind == "fwd":                        # o[q, c] = M[q, 64j + c] / n_q
        _onehot_rows(t[:, :, 2], j, N)
    elif kind == "dkv":                      # V = 0: o = 0, delta = 0;  dV[k, c] = M[64j + c, k] / n_{64j + c}
        _onehot_rows(d_o.view(B, N, H, 64), j, N)
    else:                                    # dP = 1, delta = o;  8 n_q dQ[q, c] = M[q, 64j + c] - delta[q]
        _onehot_rows(t[:, :, 1], j, N)
        t[:, :, 2] = 1.0
        d_o.fill_(2.0 ** -6)
    return qkv, d_o


def decode_fwd(o, j, N):
    """o [B, H, N, 64] -> keep [B, H, N, cols] of keys 64j .."""
    return o[..., :min(64, N - 64 * j)] != 0


def decode_dkv(dv, j, N):
    """dv [B, H, N, 64] -> keep [B, H, rows, N] of queries 64j .."""
    return (dv[..., :min(64, N - 64 * j)] != 0).transpose(-1, -2)


def dq_quantity(dq, j, N, delta_ref, causal):
    """8 n_q dQ[q, c] + delta_ref[q]: 0 or 1/(1-p).  delta_ref [B, H, N] = rowsum(P o M) from mask()"""
    n_q = (torch.arange(N) + 1 if causal else torch.full((N,), N)).double()
    return 8.0 * n_q[:, None] * dq[..., :min(64, N - 64 * j)].double() + delta_ref.double()[..., None]


def decode_dq(dq, j, N, delta_ref, causal, p):
    return dq_quantity(dq, j, N, delta_ref, causal) > 0.5 * float(DR.scale(p))


def probe_delta_ref(M, causal):
    """delta of the dQ probe = o = rowsum(P o M) with P uniform over the keys the row sees"""
    N = M.shape[-1]
    al = allowed(N, causal).double()
    return (M.double() * al).sum(-1) / al.sum(-1)


def probe_reference(N, causal):
    """-> (keep [B, H, N, N] bool, region [N, N] bool in which the kernels decide, M)"""
    M = mask(PROBE_B, PROBE_H, N, PROBE_P, SEED)
    return M != 0, allowed(N, causal), M


# ------------------------------------------------------------------------------------------ row-chunked forms, one head, no dropout
def long_inputs(N=LONG_N):
    return r16(randn((N, 3 * 64), 9000 + N, 1.5)), r16(randn((N, 64), 9001 + N))


def long_forward(q, k, v, causal, block=1024):
    """q, k, v [N, 64] -> (o fp64, lse2 fp64, restated o) in blocks of `block` query rows; no N x N matrix is held"""
    q, k, v = q.double(), k.double(), v.double()
    N = q.shape[0]
    o, o_rs, lse = torch.empty_like(q), torch.empty_like(q), torch.empty(N, dtype=torch.float64)
    for r0 in range(0, N, block):
        r1 = min(N, r0 + block)
        ke = r1 if causal else N                                   # keys past the block's last row are masked for all of it
        s = (q[r0:r1] @ k[:ke].T) * SCALE
        if causal:
            s = s.masked_fill(torch.arange(ke)[None, :] > torch.arange(r0, r1)[:, None], float("-inf"))
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        o[r0:r1] = (e @ v[:ke]) / l
        o_rs[r0:r1] = r16((r16(e) @ v[:ke]) / l)
        lse[r0:r1] = (m + torch.log(l)).squeeze(-1) * LOG2E
    return o, lse, o_rs


def long_backward(q, k, v, d_o, o, lse, causal, tiles, rounded):
    """dq of the query tiles and dk / dv of the key tiles in `tiles` -> {"dq", "dk", "dv"} each [len(tiles), 32, 64] fp64.
    o is the forward output delta is taken from (the fp64 one, or the restated one with rounded=True, which also rounds dS, P and the outputs)"""
    q, k, v, d_o, o = (t.double() for t in (q, k, v, d_o, o))
    N = q.shape[0]
    rnd = r16 if rounded else (lambda x: x)
    delta = (d_o * o).sum(-1)
    ln = lse / LOG2E
    ar = torch.arange(N)
    out = {"dq": [], "dk": [], "dv": []}
    for t in tiles:
        r = slice(TILE * t, min(N, TILE * t + TILE))
        # query tile: [32, N]
        no = (ar[None, :] > ar[r, None]) if causal else torch.zeros(1, 1, dtype=torch.bool)
        P = torch.exp(((q[r] @ k.T) * SCALE).masked_fill(no, float("-inf")) - ln[r, None])
        dS = rnd(P * (d_o[r] @ v.T - delta[r, None]))
        out["dq"].append(rnd(dS @ k * SCALE))
        # key tile: [N, 32]
        no = (ar[None, r] > ar[:, None]) if causal else torch.zeros(1, 1, dtype=torch.bool)
        P = torch.exp(((q @ k[r].T) * SCALE).masked_fill(no, float("-inf")) - ln[:, None])
        dS = rnd(P * (d_o @ v[r].T - delta[:, None]))
        out["dk"].append(rnd(dS.T @ q * SCALE))
        out["dv"].append(rnd(rnd(P).T @ d_o))
    z = torch.zeros(TILE, 64, dtype=torch.float64)                 # a ragged last tile is padded with zero rows
    return {n: torch.stack([torch.cat([t, z[t.shape[0]:]]) for t in x]) for n, x in out.items()}


def take_tiles(x, tiles):
    """[N, 64] -> [len(tiles), 32, 64]"""
    return torch.stack([x[TILE * t:TILE * t + TILE] for t in tiles])


@functools.lru_cache(maxsize=None)
def long_reference(N=LONG_N, tiles=LONG_TILES):
    """causal, p = 0, B = H = 1"""
    qkv, d_o = long_inputs(N)
    q, k, v = qkv[:, :64], qkv[:, 64:128], qkv[:, 128:]
    o, lse, o_rs = long_forward(q, k, v, True)
    ref = long_backward(q, k, v, d_o, o, lse, True, tiles, False)
    rs = long_backward(q, k, v, d_o, o_rs, lse, True, tiles, True)
    ref.update(o=o, lse=lse)
    rs.update(o=o_rs, lse=lse)
    return {"qkv": qkv, "d_o": d_o, "ref": ref, "restate": rs, "floors": floors(ref, rs)}


# ------------------------------------------------------------------------------------------ every instantiated form (test_gpu_attention_forms.py)
# The codes of include/vitamd.h vitamd_attention_form: family | key tiles << 4 | query tiles << 8 | flags
FWD_SMALL, FWD_SMALL8, FWD_LOOP, FWD_LONG, BWD_PIPE, BWD_LOOP, BWD_LONG = 1, 2, 3, 4, 5, 6, 7
F_DROP, F_CAUSAL, F_RES, F_KEEP = 0x1000, 0x2000, 0x4000, 0x8000
FAMILY_NAMES = {FWD_SMALL: "attn_fwd_small_kernel", FWD_SMALL8: "attn_fwd_small8_kernel", FWD_LOOP: "attn_fwd_kernel", FWD_LONG: "attn_fwd_long_kernel",
                BWD_PIPE: "attn_bwd_*_pipe_kernel", BWD_LOOP: "attn_bwd_*_kernel", BWD_LONG: "attn_bwd_*_long_kernel"}
TILED_FAMILIES = (FWD_SMALL, FWD_SMALL8, BWD_PIPE)          # templated on the key-tile count
FORM_B, FORM_H, FORM_P = 2, 2, 0.3                           # B*H = 4: every wave rotation on every tile count; batch stride and head offset live


def form_code(family, nt=0, nqt=0, drop=False, causal=False, res=False, keep=False):
    return family | nt << 4 | nqt << 8 | (F_DROP if drop else 0) | (F_CAUSAL if causal else 0) | (F_RES if res else 0) | (F_KEEP if keep else 0)


def code_name(code):
    fam, nt, nqt = code & 0xf, code >> 4 & 0xf, code >> 8 & 0xf
    flags = [n for n, b in (("DROP", F_DROP), ("CAUSAL", F_CAUSAL), ("RES", F_RES), ("KEEP", F_KEEP)) if code & b]
    return f"{FAMILY_NAMES.get(fam, fam)}<{', '.join(([f'{nt} tiles'] if nt else []) + ([f'{nqt} query tiles'] if nqt else []) + flags)}>"


def edges(t):
    """the two lengths of t key tiles a form is run at: one valid key in the last tile, and the tile full"""
    return (TILE * (t - 1) + 1, TILE * t)


def _form_cases():
    """-> {case: [the codes it was chosen for]}; case = (B, N, H, causal, p, resid, nq)"""
    out = {}
    # ordinary entry points, with the residual epilogue (the test also makes the call without it: both RES forms): every tile count x
    # causal x dropout at both edges.  Chosen for: forward with RES, forward without, backward.
    for t in range(1, 9):
        for causal in (False, True):
            for p in (0.0, FORM_P):
                drop = p > 0
                eight = t >= 5 and not drop and not causal
                fwd = [form_code(FWD_SMALL8, t, res=r) if eight else form_code(FWD_SMALL, t, drop=drop, causal=causal, res=r) for r in (True, False)]
                bwd = form_code(BWD_PIPE, t, t) if 2 <= t <= 7 and not drop and not causal else form_code(BWD_LOOP, drop=drop, causal=causal)
                for N in edges(t):
                    out[(FORM_B, N, FORM_H, causal, p, True, 0)] = fwd + [bwd]
    # kept-query backward: every (key tiles, query tiles) pair; nq at its ragged edge 32(q-1)+1 and at min(32q, N, 128), one with each N edge
    # (which with which alternates, so that all four combinations occur).  Chosen for: the kept backward, and the kept forward where served.
    for t in range(2, 8):
        for q in range(1, min(t, 4) + 1):
            (n_rag, n_ex), q_rag = edges(t), TILE * (q - 1) + 1
            pairs = ((n_rag, q_rag), (n_ex, None)) if (t + q) % 2 == 0 else ((n_rag, None), (n_ex, q_rag))
            for N, nq in pairs:
                nq = min(TILE * q, N, 128) if nq is None else nq
                out[(FORM_B, N, FORM_H, False, 0.0, False, nq)] = [form_code(BWD_PIPE, t, q, keep=True)] + ([form_code(FWD_SMALL8, t, keep=True)] if t >= 5 else [])
    # kept-query forward: nq in {1, 33, 128, N} over 5..8 tiles.  (129, 1), (161, 33) and (193, 128) are cases of the list above; 8 tiles
    # (no kept backward there) at both edges, with nq = N and nq = 33:
    for N, nq in ((225, 225), (256, 33)):
        out[(FORM_B, N, FORM_H, False, 0.0, False, nq)] = [form_code(FWD_SMALL8, 8, keep=True)]
    return out


FORM_EXPECT = _form_cases()
FORM_CASES = list(FORM_EXPECT)
assert all(c in FORM_EXPECT for c in ((FORM_B, 129, FORM_H, False, 0.0, False, 1), (FORM_B, 161, FORM_H, False, 0.0, False, 33),
                                      (FORM_B, 193, FORM_H, False, 0.0, False, 128)))
# tile-templated forms whose range of lengths admits only one of the two edges: {code: reason}.  None: every instantiated tile count t
# accepts 32(t-1)+1 as well as 32t, and a kept form of q = t query tiles accepts nq = N at the ragged N.
ONE_EDGE = {}
# the family (forward, backward) each MATRIX case reaches, as the docstring of tests/test_gpu_attention_matrix.py used to state in prose
MATRIX_FAMILIES = [(FWD_SMALL, BWD_LOOP) if c[1] <= 256 else (FWD_LOOP, BWD_LOOP) if c[1] <= 512 else (FWD_LONG, BWD_LONG) for c in MATRIX]


def form_case_id(c):
    B, N, H, causal, p, resid, nq = c
    return f"N{N}-{'causal' if causal else 'full'}-p{p}" + ("-resid" if resid else "") + (f"-nq{nq}" if nq else "")


def form_case_calls(c, form):
    """The (N, causal, p, resid, nq, backward) calls the GPU test of form case c makes.  form(*call) is vitamd_attention_form: it tells
    which kept forms are served (a kept case runs those, and beside them the full-size calls they are compared with)."""
    B, N, H, causal, p, resid, nq = c
    if nq == 0:
        return ([(N, causal, p, True, 0, False)] if resid else []) + [(N, causal, p, False, 0, False), (N, causal, p, False, 0, True)]
    calls = [(N, False, 0.0, False, 0, False)]
    if form(N, False, 0.0, False, nq, False) >= 0:
        calls.append((N, False, 0.0, False, nq, False))
    if form(N, False, 0.0, False, nq, True) >= 0:
        calls += [(N, False, 0.0, False, 0, True), (N, False, 0.0, False, nq, True)]
    return calls


def other_case_calls():
    """the calls of MATRIX, PROBE_CASES, SPIKE_CASES and the long-sequence case (forward and backward each)"""
    calls = [(N, causal, p) for (B, N, H, causal, p) in MATRIX]
    calls += [(N, causal, PROBE_P) for N, causal in PROBE_CASES]
    calls += [(N, causal, 0.0) for N, key in SPIKE_CASES for causal in (False, True)]
    calls += [(LONG_N, True, 0.0)]
    return [(N, causal, p, False, 0, bwd) for N, causal, p in calls for bwd in (False, True)]


def coverage_gaps(swept, form, cases=None):
    """swept: the codes the library can answer.  -> [what is unreached]: a code no case's call gets, or a tile-templated code some case
    reaches but not at both edges() of its tile count (ONE_EDGE excepted)."""
    cases = FORM_CASES if cases is None else cases
    reached = {}
    for call in [call for c in cases for call in form_case_calls(c, form)] + other_case_calls():
        reached.setdefault(form(*call), set()).add(call[0])
    gaps = []
    for code in sorted(swept):
        if code not in reached:
            gaps.append(f"{code:#x} {code_name(code)}: no case")
        elif code & 0xf in TILED_FAMILIES:
            missing = [N for N in edges(code >> 4 & 0xf) if N not in reached[code]]
            if missing and code not in ONE_EDGE:
                gaps.append(f"{code:#x} {code_name(code)}: not run at N = {missing}")
    return gaps


def form_inputs(c):
    """qkv [B*N, 3*H*64], d_o [B*N, H*64] (a kept case: COMPACT [B*nq, H*64]), x0 [B*N, H*64] fp32; qkv and d_o hold bf16 values"""
    B, N, H, causal, p, resid, nq = c
    seed = 70000 + 64 * N + 8 * nq * 1000 + 4 * int(causal) + 2 * int(p > 0)
    rows = B * (nq or N)
    return r16(randn((B * N, 3 * H * 64), seed, 1.5)), r16(randn((rows, H * 64), seed + 1)), randn((B * N, H * 64), seed + 2, 2.0)


def pad_rows(x, B, N, nq):
    """compact [B*nq, W] -> [B*N, W] with zero rows for the tokens >= nq"""
    out = torch.zeros((B, N, x.shape[-1]), dtype=x.dtype, device=x.device)
    out[:, :nq] = x.view(B, nq, -1)
    return out.view(B * N, -1)


@functools.lru_cache(maxsize=None)
def form_reference(c):
    """computed once per case and shared; treat as read-only.  A kept case: ref64 and restate on d_o zero-padded to N rows"""
    B, N, H, causal, p, resid, nq = c
    qkv, d_o, _ = form_inputs(c)
    return _reference(qkv, pad_rows(d_o, B, N, nq) if nq else d_o, B, N, H, causal, p, SEED)


def keep_slice(t, nq):
    """{name: [B, H, N, ...]} -> the kept forward's part: o and lse of the queries < nq"""
    return {"o": t["o"][..., :nq, :], "lse": t["lse"][..., :nq]}


# two mistakes a kept-query backward can make, as restatements: name -> d_o [B, H, N, 64] the mistaken kernel works from
def _keep_d_o(c, row):
    """d_o as a kernel sees it that reads row(b, t) of the compact buffer for every query t < 32 * ceil(nq / 32) (wrapping inside the buffer)"""
    B, N, H, causal, p, resid, nq = c
    compact = form_inputs(c)[1]
    t_end = min(N, TILE * ((nq + TILE - 1) // TILE))
    full = torch.zeros(B, N, H * 64)
    for b in range(B):
        for t in range(t_end):
            full[b, t] = compact[row(b, t) % (B * nq)]
    return heads(full.view(B * N, H * 64), B, N, H)


def _keep_mutant_pad_lse(c):
    """the padded queries nq .. 32*NQT-1 of the last kept tile keep their real lse (their P is not zero) and read on in the compact d_o"""
    nq = c[6]
    return _keep_d_o(c, lambda b, t: b * nq + t)


def _keep_mutant_stride(c):
    """d_o row b*nq + t read as b*N + t; the padded queries still contribute nothing"""
    B, N, H, causal, p, resid, nq = c
    g = _keep_d_o(c, lambda b, t: b * N + t).clone()
    g[..., nq:, :] = 0
    return g


KEEP_MUTANTS = {"padded queries of the last kept tile keep their lse": _keep_mutant_pad_lse,
                "compact d_o indexed with the dense batch stride": _keep_mutant_stride}


def keep_mutant_outputs(name, c):
    """restate() of kept case c as the mistaken kernel would compute it; the Q rows >= nq are written as zeros as in the real one"""
    r = form_reference(c)
    q, k, v, _ = r["in"]
    out = dict(restate(q, k, v, KEEP_MUTANTS[name](c), None, False))
    out["dq"] = out["dq"].clone()
    out["dq"][..., c[6]:, :] = 0
    return out
