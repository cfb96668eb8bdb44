"""Exact references for the GEMM entry points at the edges of their C-ABI contract (include/vitamd.h: vitamd_gemm_nt_bf16,
vitamd_gemm_skinny_bf16, vitamd_gemm_tn_bf16*), written from the header and independent of the kernel text.

Method: operands are small integers times a power of two, so every product and every partial sum is exact in fp32 in ANY order (MFMA
fragments, split-K, atomics).  The reference is that exact result followed by the single bf16 rounding the header documents, and the
checks are bit equality, element for element, on buffers that are larger than the logical result and pre-filled with a sentinel bit
pattern: a store outside the logical [M, N] region shows as a changed sentinel.

Everything here runs on the CPU.  tests/test_gpu_gemm_edges.py feeds the checks with what the kernels wrote; tests/test_gemm_ref_host.py
feeds them with the reference itself (and with damaged copies of it) and verifies the conditions the method rests on for every
parametrisation of the GPU file: the 2^24 exactness bounds, the share of GELU inputs inside the table, NaN padding that stays out of
the reference."""
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

torch.set_num_threads(min(torch.get_num_threads(), 16))      # the reference matmuls: at most 16 CPU threads

BF16, F32 = torch.bfloat16, torch.float32
EPI_BIAS_BF16, EPI_GELU, EPI_RESID_F32, EPI_DGELU, EPI_PATCH_F32, EPI_F32, EPI_GELU_DG, EPI_DMUL = range(8)
EPI_NAMES = ("bias", "gelu", "resid", "dgelu", "patch", "f32", "gelu_dg", "dmul")
F32_OUT = (EPI_RESID_F32, EPI_PATCH_F32, EPI_F32)
GUARD = 2                       # sentinel rows in front of and behind every output
SENT16, SENT32 = 0x7B7B, 0x7B7B7B7B
EXACT = 2 ** 24                 # integers (in units of the quantum) below this are exact in fp32, and so is every partial sum of theirs
PATCH_NP, PATCH_EXTRA = 7, 2    # EPI_PATCH_F32: patches per sequence and the rows in front of them that the GEMM must leave alone


# ---------------------------------------------------------------------------------------------- number formats
def bf16_rne_exact(v):
    """float64 array -> bf16 bit patterns, nearest-even decided on exact distances (no float32 intermediate rounding).  Domain: finite
    values whose rounding stays finite."""
    u = v.astype(np.float32).view(np.uint32).astype(np.int64)
    first = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    val = lambda b: (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    best, bd = first.copy(), np.abs(val(first) - v)
    for dl in (-1, 1):
        n = first + dl
        dd = np.abs(val(n) - v)
        take = (dd < bd) | ((dd == bd) & (n % 2 == 0) & (best % 2 == 1))
        best, bd = np.where(take, n, best), np.where(take, dd, bd)
    return best.astype(np.int64)


def bf16_val(b):
    """bf16 bit patterns (integer numpy array) -> float64"""
    return ((np.asarray(b).astype(np.int64) & 0xffff).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def r16(x):
    """one round-to-nearest-even to bf16, as fp32 (torch's cast; test_gemm_ref_host.py holds it against bf16_rne_exact)"""
    return x.to(BF16).float()


def bits(t):
    """bf16 / fp32 tensor -> its bit patterns (int16 / int32 tensor of the same shape)"""
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def u16(t):
    """int16 bit patterns -> numpy int64 in 0 .. 65535"""
    return t.numpy().astype(np.int64) & 0xffff


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def strided(x, ld, pad=float("nan")):
    """x [rows, n] -> [rows, ld] with the padding columns filled with `pad` (NaN: a read through the wrong stride poisons the result)"""
    full = torch.full((x.shape[0], ld), pad, dtype=x.dtype)
    full[:, :x.shape[1]] = x
    return full


def sentinel(rows, ld, dtype):
    return torch.full((rows, ld), SENT16 if dtype == BF16 else SENT32, dtype=torch.int16 if dtype == BF16 else torch.int32)


def gelu64(x):
    """float64 erf-GELU and its derivative: x Phi(x), Phi(x) + x phi(x) (erfc for the tail, as the library's table is built)"""
    x = x.double()
    cdf = 0.5 * torch.special.erfc(-x * 0.7071067811865476)
    return x * cdf, cdf + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


_GELU_BITS = []


def gelu_bits(pre_b):
    """bf16 bit patterns of pre-activations (int16 tensor) -> the bit patterns of bf16_rne(float64 gelu) and bf16_rne(float64 gelu'), looked
    up in a table of all 65 536 inputs (built once; non-finite inputs are left at zero: no case produces one)"""
    if not _GELU_BITS:
        pat = np.arange(65536, dtype=np.int64)
        finite = ((pat >> 7) & 0xff) != 0xff
        x = torch.from_numpy(bf16_val(np.where(finite, pat, 0)))
        _GELU_BITS.extend(torch.from_numpy(np.where(finite, bf16_rne_exact(t.numpy()), 0)).to(torch.int16) for t in gelu64(x))
    idx = pre_b.long() & 0xffff
    return _GELU_BITS[0][idx], _GELU_BITS[1][idx]


def in_table(b):
    """bf16 bit patterns whose value lies in the GELU table's range 2^-13 <= |x| < 8"""
    mag = np.asarray(b).astype(np.int64) & 0x7fff
    return (mag >= 0x3900) & (mag < 0x4100)


def gelu_shift(K):
    """the power of two the A operand of a GELU case is scaled down by: pre-activations of standard deviation 1.5 .. 3"""
    return max(0, math.ceil(math.log2(3.56 * math.sqrt(K) / 3.0)))


def plant_zero(bias, acc, shift):
    """bias[j] = -acc[0, j] at the first column j where that is bf16-exact: the pre-activation (0, j) is an exact zero, below the table"""
    j = int((acc[0].abs() * 2.0 ** shift < 256).nonzero()[0])
    bias[j] = -float(acc[0, j])
    return bias


def exact_sum_bound(rows, max_abs, quantum, what, prefill=0.0):
    """(rows x max|value| + |prefill|) / quantum < 2^24: every value is a multiple of `quantum`, so every partial sum of a column, in any
    order, is an integer below 2^24 in units of the quantum - exact in fp32"""
    n = (rows * max_abs + prefill) / quantum
    assert n < EXACT, f"{what}: ({rows} rows x {max_abs} + {prefill}) / {quantum} = {n:.3g} is not below 2^24"
    return n


# ---------------------------------------------------------------------------------------------- comparing buffers
def assert_bits_equal(name, got, want, logical=None, guard=GUARD):
    """element-for-element equality of two integer (bit pattern) tensors, with a message that says where and how many"""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    r, c = int(bad[0][0]), int(bad[0][1])
    where = ""
    if logical is not None:
        n_out = int((~logical[bad[:, 0], bad[:, 1]]).sum())
        where = f", {n_out} of them outside the logical region (sentinel overwritten)"
    raise AssertionError(f"{name}: {bad.shape[0]} of {got.numel()} elements differ{where}; first at buffer row {r} (logical {r - guard}), "
                         f"column {c}: got {int(got[r, c]) & 0xffffffff:#x}, want {int(want[r, c]) & 0xffffffff:#x}")


def frame(logical_bits, rowmask, ldo):
    """logical_bits [rows, N] (bit patterns; rows where rowmask is False are not written by the kernel) -> the whole expected buffer
    [GUARD + rows + GUARD, ldo] and the mask of its logical (written) elements"""
    rows, N = logical_bits.shape
    want = torch.full((rows + 2 * GUARD, ldo), SENT16 if logical_bits.dtype == torch.int16 else SENT32, dtype=logical_bits.dtype)
    logical = torch.zeros((rows + 2 * GUARD, ldo), dtype=torch.bool)
    if rowmask is None:
        want[GUARD:GUARD + rows, :N] = logical_bits
        logical[GUARD:GUARD + rows, :N] = True
    else:
        idx = rowmask.nonzero().flatten() + GUARD
        want[idx, :N] = logical_bits[rowmask]
        logical[idx, :N] = True
    return want, logical


def assert_untouched(name, got):
    """a refused call must leave the sentinel-filled buffer as it was"""
    s = SENT16 if got.dtype == torch.int16 else SENT32
    n = int((got != s).sum())
    assert n == 0, f"{name}: a refused call wrote {n} elements"


# ---------------------------------------------------------------------------------------------- NT GEMM
NtCase = namedtuple("NtCase", "tile epi M N K ldo")


def nt_id(c):
    return f"t{c.tile}-{EPI_NAMES[c.epi]}-M{c.M}-N{c.N}-K{c.K}-ldo{c.ldo}"


def _sparse3(M, K, seed):
    """three entries of +-1 per row at random k: |A.B^T| <= 3 for B in {-1, 0, 1}"""
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros((M, K))
    idx = torch.randint(0, K, (M, 3), generator=g)
    val = torch.randint(0, 2, (M, 3), generator=g).float() * 2 - 1
    a.scatter_(1, idx, val)
    return a


def nt_problem(c):
    """Operands, auxiliary inputs and the exact expected outputs of one vitamd_gemm_nt_bf16 call.  Asserts, on the reference alone, the
    conditions the exact checks rest on."""
    tile, epi, M, N, K, ldo = c
    seed = 100000 + M * 31 + N * 17 + K * 7 + ldo * 3 + epi
    p = SimpleNamespace(case=c, out_dtype=F32 if epi in F32_OUT else BF16, bias=None, aux=None, colsum0=None, n_patches=0, seq=0, extra=0,
                        out2_want=None, colsum_want=None, stats={})
    gelu = epi in (EPI_GELU, EPI_GELU_DG)
    if epi == EPI_DGELU and M > 4096:
        a, b = _sparse3(M, K, seed), ints((N, K), -1, 1, seed + 1)                  # |acc| <= 3: the column sums of 16k rows stay exact
    elif epi == EPI_DGELU:
        a, b = ints((M, K), -1, 1, seed) * ints((M, K), 0, 1, seed + 7), ints((N, K), -1, 2, seed + 1)
    elif gelu:
        a, b = ints((M, K), -3, 3, seed), ints((N, K), -2, 3, seed + 1)              # zero-mean products: the pre-activations stay centred at every K
    else:
        a, b = ints((M, K), -3, 2, seed), ints((N, K), -2, 3, seed + 1)              # asymmetric ranges: a transposed or swapped operand cannot pass
    acc = a @ b.t() + 0.0                                                            # integers: exact in fp32 in any order; + 0.0: no negative zero
    assert float(acc.abs().max()) < EXACT
    if gelu:
        s = 2.0 ** -gelu_shift(K)
        a, acc = a * s, acc * s                                                      # pre-activations are multiples of 2^-shift
    p.a, p.b, p.acc = a.to(BF16), b.to(BF16), acc
    assert torch.equal(p.a.float(), a) and torch.equal(p.b.float(), b)
    acc16 = r16(acc)

    if gelu:
        bias = plant_zero(ints((N,), -8, 8, seed + 2) * 0.25, acc, gelu_shift(K))    # one input below the table in every case
    elif epi in (EPI_BIAS_BF16, EPI_RESID_F32, EPI_PATCH_F32):
        bias = ints((N,), -4, 5, seed + 2)
        bias[1::2] += 2.0 ** -9                                                      # not bf16-exact beside an integer: the kernels round the bias first
    else:
        bias = None
    p.bias = bias
    lin = r16(acc + r16(bias)) if bias is not None else acc16                        # the Linear output as autocast leaves it: ONE rounding of an exact sum

    rowmask = None
    if epi == EPI_BIAS_BF16:
        want = bits(lin.to(BF16))
    elif gelu:
        pre_b = bits(lin.to(BF16))
        act_b, dg_b = gelu_bits(pre_b)
        p.inside = torch.from_numpy(in_table(u16(pre_b)))
        share = float(p.inside.float().mean())
        p.stats["gelu_inside_share"] = share
        assert share >= 0.9, f"{nt_id(c)}: only {share:.3f} of the GELU inputs lie inside the table range"
        assert not bool(p.inside.all()), f"{nt_id(c)}: no GELU input outside the table range"
        want = pre_b if epi == EPI_GELU else dg_b
        p.out2_want = act_b
    elif epi == EPI_RESID_F32:
        res = ints((M, N), -7, 8, seed + 3)
        p.aux = strided(res, ldo)
        want = bits(res + lin)
    elif epi == EPI_PATCH_F32:
        p.n_patches, p.extra, p.seq = PATCH_NP, PATCH_EXTRA, PATCH_NP + PATCH_EXTRA
        pos = ints((PATCH_NP, N), -7, 8, seed + 3)
        p.aux = strided(pos, ldo)
        m = torch.arange(M)
        bi, pi = m // PATCH_NP, m % PATCH_NP
        rows = ((M + PATCH_NP - 1) // PATCH_NP) * p.seq
        orow = bi * p.seq + p.extra + pi
        rowmask = torch.zeros(rows, dtype=torch.bool)
        rowmask[orow] = True                                                         # the `extra` rows of every sequence stay untouched
        wl = torch.zeros((rows, N))
        wl[orow] = lin + pos[pi]
        want = bits(wl)
    elif epi == EPI_F32:
        want = bits(acc)
    elif epi == EPI_DMUL:
        fac = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[ints((M, N), 0, 6, seed + 3).long()]
        p.aux = strided(fac.to(BF16), ldo)
        stored = r16(acc16 * fac)                                                    # bf16(acc) times a power of two: exact, the rounding is the identity
        want = bits(stored.to(BF16))
        p.colsum0 = ints((N,), -9, 10, seed + 5)
        p.stats["colsum_units"] = exact_sum_bound(M, float(stored.abs().max()), 0.5, nt_id(c) + " colsum", prefill=10.0)
        assert torch.equal(stored * 2, (stored * 2).round())                         # every stored value is a multiple of the quantum 0.5
        p.colsum_want = (p.colsum0.double() + stored.double().sum(0)).float()
    else:                                                                            # EPI_DGELU: the derivative by formula
        lo, n = (1.0, 8) if M > 4096 else (0.0, 12)                                  # gelu' in [1.01, 1.13] (every stored value in [1, 4) or zero) / [0.5, 1.13]
        idx = ints((M, N), 0, n, seed + 3).long()
        pre = lo + idx.float() * 0.25
        p.aux = strided(pre.to(BF16), ldo)
        dg = gelu64(lo + torch.arange(n + 1) * 0.25)[1]                               # gelu' of the n + 1 distinct inputs
        if M > 4096:                                                                 # |acc| <= 3: 7 x 9 distinct products, gathered (12.8 M elements)
            assert float(acc16.abs().max()) <= 3
            tab64 = torch.arange(-3.0, 4.0).double()[:, None] * dg[None, :]
            ai = (acc16 + 3).long()
            ref64, want_b = tab64[ai, idx], bf16_rne_exact(tab64.numpy())[ai.numpy(), idx.numpy()]
        else:
            ref64 = acc16.double() * dg[idx]
            want_b = bf16_rne_exact(ref64.numpy())
        p.dgelu_ref64 = ref64
        p.dgelu_zero = acc16 == 0                                                    # an exactly zero product must be stored as zero
        p.dgelu_half = (pre == 0) & ~p.dgelu_zero                                    # gelu'(0) = 1/2 exactly: bf16(acc) / 2, no tolerance
        want = torch.from_numpy(want_b).to(torch.int16)
        nz = torch.cat([ref64.abs()[ref64 != 0], torch.ones(1, dtype=torch.float64)])
        quantum = 2.0 ** (math.floor(math.log2(float(nz.min()))) - 8)                # one ulp below the smallest reference magnitude, binade edge included
        p.colsum0 = ints((N,), -9, 10, seed + 5)
        p.stats["colsum_units"] = exact_sum_bound(M, float(nz.max()) * (1 + 2.0 ** -7), quantum, nt_id(c) + " colsum", prefill=10.0)
    p.want_logical, p.rowmask = want, rowmask
    p.want, p.logical = frame(want, rowmask, ldo)
    if p.out2_want is not None:
        p.want2, _ = frame(p.out2_want, None, ldo)
    for w in (want, p.out2_want):                                                    # the NaN padding of aux never reaches the logical region
        assert w is None or bool(torch.isfinite(w.view(BF16 if w.dtype == torch.int16 else F32).float()).all())
    return p


def _gelu_outside_ok(got_b, want_b):
    """outside the table: one unit in the last place (same sign), or 1e-12 absolute (the contract of test_gelu_table_exact_on_every_bf16_input)"""
    ok = (np.abs((got_b & 0x7fff) - (want_b & 0x7fff)) <= 1) & ((got_b >> 15) == (want_b >> 15))
    return ok | (np.abs(bf16_val(got_b) - bf16_val(want_b)) <= 1e-12)


def nt_check(p, got):
    """got.out / got.out2: the whole buffers (bit patterns, guard rows and padding columns included) after the call; got.colsum fp32 [N].
    Returns the figures worth recording."""
    c, epi = p.case, p.case.epi
    name = nt_id(c)
    M, N = c.M, c.N
    stats = {}
    if epi in (EPI_GELU, EPI_GELU_DG):
        for label, g, w, wl in (("out", got.out, p.want, p.want_logical), ("out2", got.out2, p.want2, p.out2_want)):
            exact = label == "out" and epi == EPI_GELU                               # the pre-activation: equal everywhere
            inside = torch.ones_like(p.inside) if exact else p.inside
            mask = torch.ones_like(p.logical)
            mask[GUARD:GUARD + M, :N] = inside                                       # sentinel and in-table elements: bit for bit
            assert_bits_equal(f"{name} {label}", torch.where(mask, g, w), w, p.logical)
            if not exact:
                gl, o = u16(g[GUARD:GUARD + M, :N]), ~p.inside.numpy()
                ok = _gelu_outside_ok(gl[o], u16(wl)[o])
                assert ok.all(), f"{name} {label}: {int((~ok).sum())} inputs outside the table are off by more than one ulp"
    elif epi == EPI_DGELU:
        assert_bits_equal(f"{name} out (outside the logical region)", torch.where(p.logical, p.want, got.out), p.want, p.logical)
        gl = got.out[GUARD:GUARD + M, :N]
        gv = torch.from_numpy(bf16_val(u16(gl)))
        assert bool((gv[p.dgelu_zero] == 0).all()), f"{name}: an exactly zero product was not stored as zero"
        half = p.dgelu_half
        assert torch.equal(gv[half], (r16(p.acc).double() * 0.5)[half]), f"{name}: gelu'(0) = 1/2 must give bf16(acc) / 2 exactly"
        rest = ~p.dgelu_zero
        ref = p.dgelu_ref64[rest]
        wv = torch.from_numpy(bf16_val(u16(p.want_logical)))[rest]
        ulp = torch.pow(2.0, torch.floor(torch.log2(ref.abs())) - 7)                 # one bf16 unit in the last place AT the reference value
        d = (gv[rest] - wv).abs() / ulp
        stats["dgelu_max_ulps"] = float(d.max()) if d.numel() else 0.0
        assert stats["dgelu_max_ulps"] <= 1.0, f"{name}: {int((d > 1).sum())} elements further than one bf16 ulp from bf16(float64), worst {float(d.max()):.3g}"
        own = (p.colsum0.double() + gv.sum(0)).float()                               # the column sums of what the kernel itself stored
        assert torch.equal(got.colsum, own), f"{name}: colsum differs from the sums of the stored output in {int((got.colsum != own).sum())} columns"
    else:
        assert_bits_equal(f"{name} out", got.out, p.want, p.logical)
        if epi == EPI_DMUL and got.colsum is not None:
            assert torch.equal(got.colsum, p.colsum_want), f"{name}: colsum differs in {int((got.colsum != p.colsum_want).sum())} columns"
    return stats


def nt_reference_output(p):
    """what a correct kernel leaves behind (the host test feeds nt_check with it)"""
    colsum = p.colsum_want
    if p.case.epi == EPI_DGELU:
        colsum = (p.colsum0.double() + torch.from_numpy(bf16_val(u16(p.want_logical))).sum(0)).float()
    return SimpleNamespace(out=p.want.clone(), out2=None if p.out2_want is None else p.want2.clone(), colsum=colsum)


# ---------------------------------------------------------------------------------------------- skinny GEMM
SKINNY_EPIS = (EPI_F32, EPI_BIAS_BF16, EPI_RESID_F32, EPI_GELU)


def skinny_ks_candidates(K, splits):
    """every K range per split (a multiple of 64) that cuts K into exactly `splits` ranges; the plan's is among them"""
    return [ks for ks in range(64, K + 64, 64) if (K + ks - 1) // ks == splits]


def skinny_problem(M, N, K, epi):
    """vitamd_gemm_skinny_bf16: dense rows, fp32 bias rounded to bf16, EPI_F32 = acc + bias"""
    seed = 200000 + M * 131 + N * 17 + K * 7 + epi
    p = SimpleNamespace(M=M, N=N, K=K, epi=epi, out_dtype=F32 if epi in F32_OUT else BF16, aux=None, out2_want=None, stats={})
    a, w = ints((M, K), -3, 3 if epi == EPI_GELU else 2, seed), ints((N, K), -2, 3, seed + 1)      # GELU: zero-mean products, centred pre-activations
    acc = a @ w.t() + 0.0
    assert float(acc.abs().max()) < EXACT                                            # and so is every split-K partial sum
    if epi == EPI_GELU:
        s = 2.0 ** -gelu_shift(K)
        a, acc = a * s, acc * s
        bias = plant_zero(ints((N,), -8, 8, seed + 2) * 0.25, acc, gelu_shift(K))
    else:
        bias = ints((N,), -4, 5, seed + 2)
        bias[1::2] += 2.0 ** -9
    p.a, p.w, p.bias, p.acc = a.to(BF16), w.to(BF16), bias, acc
    assert torch.equal(p.a.float(), a)
    full = acc + r16(bias)
    lin = r16(full)
    if epi == EPI_F32:
        want = bits(full)
    elif epi == EPI_BIAS_BF16:
        want = bits(lin.to(BF16))
    elif epi == EPI_RESID_F32:
        p.aux = ints((M, N), -7, 8, seed + 3)
        want = bits(p.aux + lin)
    else:
        want = bits(lin.to(BF16))
        p.inside = torch.from_numpy(in_table(u16(want)))
        p.out2_want = gelu_bits(want)[0]
        p.want2, _ = frame(p.out2_want, None, N)
    p.want_logical = want
    p.want, p.logical = frame(want, None, N)
    assert bool(torch.isfinite(full).all())
    return p


def skinny_check(p, got):
    name = f"skinny {EPI_NAMES[p.epi]} M{p.M} N{p.N} K{p.K}"
    assert_bits_equal(name + " out", got.out, p.want, p.logical)
    if p.epi == EPI_GELU:
        mask = torch.ones_like(p.logical)
        mask[GUARD:GUARD + p.M, :] = p.inside
        assert_bits_equal(name + " out2", torch.where(mask, got.out2, p.want2), p.want2, p.logical)
        o = ~p.inside.numpy()
        ok = _gelu_outside_ok(u16(got.out2[GUARD:GUARD + p.M])[o], u16(p.out2_want)[o])
        assert ok.all(), f"{name} out2: inputs outside the table are off by more than one ulp"


def skinny_reference_output(p):
    return SimpleNamespace(out=p.want.clone(), out2=None if p.out2_want is None else p.want2.clone())


def gelu_share(problems):
    """(share of the GELU inputs of these problems inside the table range, number outside it)"""
    inside = sum(int(q.inside.sum()) for q in problems)
    total = sum(q.inside.numel() for q in problems)
    return inside / total, total - inside


# ---------------------------------------------------------------------------------------------- TN GEMM
TnCase = namedtuple("TnCase", "R P Q ldo splits accumulate")
TN_LDL, TN_LOFF, TN_ROFF = 2304, 768, 32       # L is a column slice of a [R, 2304] buffer (the packed dQKV layout); Rm sits 32 columns into its rows


def tn_id(c):
    return f"R{c.R}-P{c.P}-Q{c.Q}-ldo{c.ldo}-s{c.splits}-acc{c.accumulate}"


def tn_problem(c):
    """vitamd_gemm_tn_bf16*: out[P, Q] (+)= L^T Rm with L and Rm column slices of wider buffers whose other columns are NaN.  A leaked
    padding column can only reach outputs p >= P or q >= Q, which the kernel must mask."""
    R, P, Q, ldo, splits, accumulate = c
    seed = 300000 + R * 13 + P * 17 + Q * 7 + ldo
    p = SimpleNamespace(case=c, ldl=TN_LDL, ldr=(Q + 7) // 8 * 8 + 64)
    p.lbuf = torch.full((R, p.ldl), float("nan"), dtype=BF16)
    p.rbuf = torch.full((R, p.ldr), float("nan"), dtype=BF16)
    p.lbuf[:, TN_LOFF:TN_LOFF + P] = ints((R, P), -2, 1, seed).to(BF16)
    p.rbuf[:, TN_ROFF:TN_ROFF + Q] = ints((R, Q), -3, 2, seed + 1).to(BF16)
    assert TN_LOFF + P + 8 <= p.ldl and TN_ROFF + Q + 8 <= p.ldr                     # the 16-byte chunk past P / Q stays inside the row (and is NaN)
    assert TN_LOFF % 8 == 0 and TN_ROFF % 8 == 0 and p.ldl % 8 == 0 and p.ldr % 8 == 0
    l, r = p.lbuf[:, TN_LOFF:TN_LOFF + P].float(), p.rbuf[:, TN_ROFF:TN_ROFF + Q].float()
    prod = l.t() @ r + 0.0
    p.init = ints((P, Q), -5, 5, seed + 2)                                           # non-zero prefill of the accumulate calls
    p.colsum0 = ints((P,), -9, 10, seed + 3)
    exact_sum_bound(R, 6.0, 1.0, tn_id(c) + " out", prefill=5.0)                            # |l r| <= 6, integers: exact in every split order, atomics included
    exact_sum_bound(R, 2.0, 1.0, tn_id(c) + " colsum", prefill=10.0)
    p.want_acc, p.want_ovw = p.init + prod, prod
    p.colsum_want = p.colsum0 + l.sum(0)
    for t in (p.want_acc, p.want_ovw, p.colsum_want):
        assert bool(torch.isfinite(t).all()), "NaN padding reached the reference"
    return p


def tn_frames(p, accumulate):
    """(the [P + 2, ldo] buffer handed to the call, the buffer expected after it), bit patterns"""
    c = p.case
    before = sentinel(c.P + 2, c.ldo, F32)
    after = before.clone()
    if accumulate:
        before[:c.P, :c.Q] = bits(p.init)
    after[:c.P, :c.Q] = bits(p.want_acc if accumulate else p.want_ovw)
    return before, after


def tn_check(name, p, got, want):
    logical = torch.zeros_like(want, dtype=torch.bool)
    logical[:p.case.P, :p.case.Q] = True
    nan = torch.isnan(got.view(torch.float32))
    assert not bool(nan.any()), f"{name}: {int(nan.sum())} NaN in out ({int((nan & ~logical).sum())} of them in the padding): a padding column of L / Rm leaked"
    assert_bits_equal(name, got, want, logical, guard=0)
