"""CPU reference for KV-cached decoding (torch + numpy), written from the "KV-cached decoding" block of include/vitamd.h and
independent of the kernel text:

    o[b, h*64 + d] = sum_k softmax_k(q[b, h] . K[b, h, k] / 8) V[b, h, k, d]   over cache positions k = 0 .. n-1,  n = *len + 1
    caches bf16 [B][H][Lmax][64], q = columns h*64 .. h*64+63 of row b of qkv [B, 3*H*64], one bf16 rounding of o

ref64()    fp64 throughout; the cache is indexed as a flat buffer of rows, ((b*H + h)*Lmax + k), so that a stride or (b, h) mistake is
           expressible (MUTANTS).
restate()  the same function as a kernel is allowed to compute it: fp32, keys in groups of `group`, each group's softmax partial
           (max, sum, weighted V) taken against its own maximum, the groups of a chunk of `chunk` keys merged online with a running
           maximum, the chunks merged against their common maximum, every rescaling an exp2 of a difference of maxima (1/8 log2 e is
           folded into q), ONE bf16 rounding at the end.  Groups and chunks that saw no key carry the maximum NEG_BIG and the sum 0.

Random data.  The distance restate <-> ref64, per (b, h) row as rel-L2 over the 64 output dims, is the floor: what one bf16 rounding of
a correct fp32 result costs.  random_reference() takes the worst row of a case over the (group, chunk) pairs of GROUPS; a kernel is held,
row by row, to MARGIN = 2 x that figure (the factor _attention_ref.compare holds the training kernels' worst tile to).  The factor
covers a kernel whose fp32 result falls on the other side of a rounding boundary than the restatement's in some elements: an
element's error is at most half a bf16 ulp either way, so a row of such elements stays below twice the rounding error of the worst row.
A per-row bound is not diluted by the other (b, h): one wrong head fails it.

Spike cases.  Every element of q is 4, the key at j* equals q (score 64 * 16 / 8 = 128, 184.66 in base 2), every other visible key is
N(0, 1).  The condition the method rests on (spike_log2_margin(), asserted for every case by tests/test_decode_ref_host.py): in fp64 the
largest other weight relative to the spike's is below 2^-150.  2^-150 and everything below it rounds to zero in fp32 (the smallest
denormal is 2^-149), so in ANY grouping and merge order every other weight and every rescaling of a partial that does not hold the
spike is exactly 0, the spike's own weight and the normaliser are exactly 1, and the contract's result is o == V[j*] bit for bit.
Past the length the key at position n is 2 q (score 256: a mask that lets it in returns V[n] instead) and every later K and V row is NaN.

MUTANTS are the deliberate mistakes tests/test_decode_ref_host.py proves these checks reject; SPIKE_CASES / SPIKE_LIMIT / RANDOM_CASES
are the cases of tests/test_gpu_decode_edges.py, shared with the host test.  kv_frame() is the expected cache after vitamd_kv_append."""
import functools

import torch

import _gemm_ref as G

BF16 = torch.bfloat16
DH = 64
SCALE = 0.125
LOG2E = 1.4426950408889634
NEG_BIG = -1.0e30
MARGIN = 2.0
GROUPS = ((8, 128), (32, 1024), (128, 16384))      # (keys per group, keys per chunk): 8 and 128 are the smallest and largest unit a 4-wave walk takes
SPIKE_Q = 4.0
SPIKE_UNDERFLOW = -150.0                         # log2: at or below it fp32 holds 0


def r16(x):
    """round to bf16, keep the dtype"""
    return x.to(BF16).to(x.dtype)


def randn_bf16(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(BF16)


# ------------------------------------------------------------------------------------------ layout
def cache_rows(cache, B, H, stride, nk, swapped=False):
    """rows 0 .. nk-1 of every (b, h) of a cache held as a flat buffer of 64-element rows: row ((b*H + h)*stride + k) -> [B, H, nk, 64].
    stride is Lmax in the contract; a row past the end of the buffer reads as NaN."""
    flat = cache.reshape(-1, DH)
    b, h = torch.arange(B)[:, None, None], torch.arange(H)[None, :, None]
    bh = h * B + b if swapped else b * H + h
    idx = bh * stride + torch.arange(nk)[None, None, :]
    over = idx >= flat.shape[0]
    rows = flat[idx.clamp_max(flat.shape[0] - 1)]
    if bool(over.any()):
        rows = rows.clone()
        rows[over] = float("nan")
    return rows


def _dims(qkv, kc, H):
    B = qkv.shape[0]
    assert qkv.shape[1] == 3 * H * DH and kc.numel() % (B * H * DH) == 0
    return B, kc.numel() // (B * H * DH)


# ------------------------------------------------------------------------------------------ fp64 reference
def ref64(qkv, kc, vc, n, H):
    """qkv [B, 3*H*64], kc / vc [B][H][Lmax][64] (bf16 values) -> fp64 [B, H*64]: the query rows against cache positions 0 .. n-1"""
    B, Lmax = _dims(qkv, kc, H)
    assert 1 <= n <= Lmax
    q = qkv[:, :H * DH].double().view(B, H, DH)
    k = cache_rows(kc, B, H, Lmax, n).double()
    v = cache_rows(vc, B, H, Lmax, n).double()
    p = torch.softmax(torch.einsum("bhd,bhkd->bhk", q, k) * SCALE, -1)
    return torch.einsum("bhk,bhkd->bhd", p, v).reshape(B, H * DH)


# ------------------------------------------------------------------------------------------ restatement in fp32
def restate(qkv, kc, vc, n, H, group=8, chunk=128, flags=()):
    """Same signature and result as ref64 (fp32 holding bf16 values), computed as the module docstring says.  flags: see MUTANTS."""
    assert chunk % 128 == 0 and 128 % group == 0
    B, Lmax = _dims(qkv, kc, H)
    nk = n - 1 if "drop_own" in flags else n + 1 if "one_more" in flags else n
    if nk <= 0:                                                        # no key at all: 0 / 0
        return torch.full((B, H * DH), float("nan"))
    ex = torch.exp if "nat_exp" in flags else torch.exp2
    plain = "no_rescale" in flags                                      # partials added as they are
    stride = n if "stride_n" in flags else Lmax
    swapped = "bh_swapped" in flags
    q = (qkv[:, :H * DH].float() * torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)).view(B, H, DH)
    k = cache_rows(kc, B, H, stride, nk, swapped).float()
    v = cache_rows(kc if "v_from_k" in flags else vc, B, H, stride, nk, swapped).float()
    started = (nk + 127) // 128 * 128                                  # the four waves walk the keys 128 at a time
    chunk = min(chunk, started)
    C = (nk + chunk - 1) // chunk
    P, Gc = C * chunk, chunk // group
    s = torch.full((B, H, P), NEG_BIG)
    s[..., :nk] = torch.einsum("bhd,bhkd->bhk", q, k)
    vp = torch.zeros((B, H, P, DH))
    vp[..., :nk, :] = v
    ok = (torch.arange(P) < nk).view(C, Gc, group)
    s, vp = s.view(B, H, C, Gc, group), vp.view(B, H, C, Gc, group, DH)
    mg = s.amax(-1)                                                    # NEG_BIG where the group saw no key
    e = ex(s - mg[..., None]) * ok                                     # a masked key: p = 0
    lg = e.sum(-1)
    ag = torch.einsum("bhcgk,bhcgkd->bhcgd", e, vp)
    if "empty_p1" in flags:                                            # a started group without a key scores its zero-filled rows 0: p = 1 each
        empty = ~ok.any(-1) & (torch.arange(P).view(C, Gc, group)[..., 0] < started)
        mg = torch.where(empty, torch.zeros(()), mg)
        lg = torch.where(empty, torch.full((), float(group)), lg)
    m = torch.full((B, H, C), NEG_BIG)
    l = torch.zeros((B, H, C))
    A = torch.zeros((B, H, C, DH))
    for i in range(Gc):                                                # online, with a running maximum, over the groups of each chunk
        mn = torch.maximum(m, mg[..., i])
        a1 = torch.ones(()) if plain else ex(m - mn)
        a2 = torch.ones(()) if plain else ex(mg[..., i] - mn)
        l = l * a1 + lg[..., i] * a2
        A = A * a1[..., None] + ag[..., i, :] * a2[..., None]
        m = mn
    if "drop_last_chunk" in flags:
        if C == 1:
            return torch.full((B, H * DH), float("nan"))
        m, l, A = m[..., :-1], l[..., :-1], A[..., :-1, :]
    if "stale_chunk" in flags:                                         # what an earlier call left in the next slot: a finite partial of this row's size
        m = torch.cat([m, m[..., :1]], -1)
        l = torch.cat([l, torch.ones((B, H, 1))], -1)
        A = torch.cat([A, torch.zeros((B, H, 1, DH))], -2)
    mm = m.amax(-1, keepdim=True)
    a = torch.ones_like(m) if plain else ex(m - mm)
    L = (l * a).sum(-1)
    if "l_from_top" in flags:
        L = l.gather(-1, m.argmax(-1, keepdim=True)).squeeze(-1)
    out = (A * a[..., None]).sum(-2) / L[..., None]
    return r16(out).reshape(B, H * DH)


# ------------------------------------------------------------------------------------------ metric and checks
def row_errors(o, ref):
    """[B, H*64] each -> rel-L2 per (b, h) row over the 64 output dims, fp64 [B*H] (NaN where o holds one)"""
    o, ref = o.double().reshape(-1, DH), ref.double().reshape(-1, DH)
    return (o - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)


def check_random(o, r):
    """o [B, H*64] against random_reference()'s r -> (worst row error, [failures]); a NaN row fails"""
    e = row_errors(o, r["ref"])
    okay = e <= r["bound"]
    worst = float("nan") if bool(torch.isnan(e).any()) else float(e.max())
    if bool(okay.all()):
        return worst, []
    i = int((~okay).nonzero()[0])
    return worst, [f"{int((~okay).sum())} of {e.numel()} rows above {MARGIN} x floor = {r['bound']:.3e}; first row bh {i}: {float(e[i]):.3e}"]


def check_spike(o, v_rows):
    """o bf16 [B, H*64] against v_rows bf16 [B, H, 64] = V[:, :, j*], bit for bit -> [failures]"""
    got, want = G.bits(o.reshape(-1, DH)), G.bits(v_rows.reshape(-1, DH))
    if got.shape == want.shape and torch.equal(got, want):
        return []
    bad = (got != want).nonzero()
    nan = int(torch.isnan(o.float()).sum())
    return [f"{bad.shape[0]} of {got.numel()} elements differ from V[j*] ({nan} NaN); first at bh {int(bad[0][0])}, dim {int(bad[0][1])}"]


# ------------------------------------------------------------------------------------------ the cases
SPIKE_TABLES = [(1, 2, 640), (2, 3, 640), (1, 2, 1000), (2, 3, 1000)]       # (B, H, Lmax); 1000 is no multiple of 128: the Lmax clamp
SPIKE_LIMIT = (4369, 15, 3, 3, 2)                                             # B*H = 65535, the last grid row the contract admits


def spike_ns(Lmax):
    """every n in 1 .. 40 (slot and wave edges), every 128k - 1, 128k, 128k + 1 up to Lmax (a chunk is a multiple of 128: every chunk
    edge of every plan), and Lmax"""
    edges = {128 * k + d for k in range(1, Lmax // 128 + 2) for d in (-1, 0, 1)}
    return sorted(n for n in set(range(1, 41)) | edges | {Lmax} if 1 <= n <= Lmax)


def spike_js(n):
    """the last key, the first key, the first key of the last started 128-group"""
    return sorted({n - 1, 0, (n - 1) // 128 * 128})


SPIKE_CASES = [(B, H, Lmax, n, j) for (B, H, Lmax) in SPIKE_TABLES for n in spike_ns(Lmax) for j in spike_js(n)]
RANDOM_CASES = [(1, 1, 16384, (1, 2, 8191, 8192, 8193, 16383, 16384)), (3, 5, 1000, (1, 129, 999, 1000)), (2, 12, 4096, (127, 128, 4095, 4096)),
                (64, 12, 300, (1, 257, 300))]


def spike_id(c):
    return "B{}-H{}-Lmax{}-n{}-j{}".format(*c)


def random_id(B, H, Lmax, n):
    return f"B{B}-H{H}-Lmax{Lmax}-n{n}"


def _base(B, H, Lmax, seed, spike):
    qkv = randn_bf16((B, 3 * H * DH), seed)
    if spike:
        qkv[:, :H * DH] = SPIKE_Q
    return qkv, randn_bf16((B, H, Lmax, DH), seed + 1), randn_bf16((B, H, Lmax, DH), seed + 2)


@functools.lru_cache(maxsize=None)
def spike_base(B, H, Lmax):
    """(qkv, kc, vc) before a case's fill; treat as read-only"""
    return _base(B, H, Lmax, 7000 + 131 * B + 17 * H + Lmax, True)


@functools.lru_cache(maxsize=None)
def random_base(B, H, Lmax):
    return _base(B, H, Lmax, 8000 + 131 * B + 17 * H + Lmax, False)


def fill_past(kc, vc, n, spike_j=None):
    """in place, on either device: the spike key at j*, 2 q at position n, NaN behind it (spike cases); NaN from position n on (random cases)"""
    Lmax = kc.shape[2]
    first_nan = n
    if spike_j is not None:
        kc[:, :, spike_j] = SPIKE_Q
        if n < Lmax:
            kc[:, :, n] = 2 * SPIKE_Q
        first_nan = n + 1
    if first_nan < Lmax:
        kc[:, :, first_nan:] = float("nan")
        vc[:, :, first_nan:] = float("nan")
    return kc, vc


def spike_inputs(c):
    B, H, Lmax, n, j = c
    qkv, kc, vc = spike_base(B, H, Lmax)
    return (qkv, *fill_past(kc.clone(), vc.clone(), n, j))


def random_inputs(B, H, Lmax, n):
    qkv, kc, vc = random_base(B, H, Lmax)
    return (qkv, *fill_past(kc.clone(), vc.clone(), n))


def spike_log2_margin(c):
    """log2 of the largest non-spike weight relative to the spike's over the visible keys of every (b, h), in fp64 (-inf at n = 1)"""
    B, H, Lmax, n, j = c
    qkv, kc, _ = spike_inputs(c)
    q = qkv[:, :H * DH].double().view(B, H, DH)
    s = torch.einsum("bhd,bhkd->bhk", q, cache_rows(kc, B, H, Lmax, n).double()) * (SCALE * LOG2E)
    spike = s[..., j].clone()
    s[..., j] = float("-inf")
    return float((s.amax(-1) - spike).max())


@functools.lru_cache(maxsize=None)
def random_reference(B, H, Lmax, n):
    """computed once per case and shared; treat as read-only.  floors: worst row of restate() per (group, chunk) of GROUPS"""
    inp = random_inputs(B, H, Lmax, n)
    ref = ref64(*inp, n, H)
    floors = {g: float(row_errors(restate(*inp, n, H, *g), ref).max()) for g in GROUPS}
    floor = max(floors.values())
    return {"ref": ref, "floors": floors, "floor": floor, "bound": MARGIN * floor}


# ------------------------------------------------------------------------------------------ mutants
# name -> (restate flag, keys per group the mutation is run with).  "a wave that saw no key": taken literally - masked keys scored NEG_BIG in a
# group whose maximum is NEG_BIG too, p = exp2(0) = 1 each - the mistake is harmless in this arithmetic, because a partial whose own maximum
# is NEG_BIG is rescaled by exp2(NEG_BIG - m) = 0 in every merge.  The form that shows is the one run here: the group's zero-filled key rows
# keep their score 0 (maximum 0, p = 1 per masked key, 32 keys: one step of one wave), so its sum enters every merge with weight exp2(-m).
MUTANTS = {
    "keys 0 .. len-1: the own key dropped": ("drop_own", 8),
    "keys 0 .. len+1": ("one_more", 8),
    "natural-base exponent on the base-2 scale": ("nat_exp", 8),
    "partials merged without rescaling": ("no_rescale", 8),
    "last started chunk dropped in the combine": ("drop_last_chunk", 8),
    "one never-written chunk read in the combine": ("stale_chunk", 8),
    "a wave that saw no key counts p = 1 per masked key": ("empty_p1", 32),
    "V taken from the K cache": ("v_from_k", 8),
    "(b, h) indexed as h*B + b": ("bh_swapped", 8),
    "cache row stride n instead of Lmax": ("stride_n", 8),
    "normaliser of the chunk with the largest max only": ("l_from_top", 8),
}


def mutant_output(name, inp, n, H):
    flag, group = MUTANTS[name]
    return restate(*inp, n, H, group=group, chunk=128, flags=(flag,))


# ------------------------------------------------------------------------------------------ K/V append
def kv_frame(qkv, B, T, H, Lmax, length, guard=G.GUARD):
    """vitamd_kv_append on sentinel-filled caches framed by `guard` sentinel rows: row t of sequence b goes to position length + t, rows
    whose position is negative or reaches Lmax are dropped.  qkv bf16 [B*T, 3*H*64] -> (k, v) bit patterns [guard + B*H*Lmax + guard, 64]"""
    src = G.bits(qkv).view(B, T, 3, H, DH)
    out = []
    for which in (1, 2):
        want = G.sentinel(B * H * Lmax + 2 * guard, DH, BF16)
        body = want[guard:guard + B * H * Lmax].view(B, H, Lmax, DH)
        for t in range(T):
            if 0 <= length + t < Lmax:
                body[:, :, length + t] = src[:, t, which]
        out.append(want)
    return out
