"""References and checks for operands past 2^31 and 2^32 bytes (tests/test_gpu_big_operands.py; tests/test_big_ref_host.py checks this file
without a GPU).

The method is tests/_gemm_ref.py's: operands are small integers (times a power of two), every partial sum is exact in fp32 in any order, the
reference is that exact sum followed by the one bf16 rounding the header documents, and the comparison is on bit patterns of
sentinel-framed buffers.  What differs is where it runs.  A 4-GiB output cannot be referenced on the CPU in a test's time, so operands
are generated on the device, the exact sums are torch's fp32 matmul in ROW CHUNKS (integers below 2^24: exact whatever the order), and the
epilogue is restated with torch ops - the library is not used.  That reference is then itself checked: BAND-row bands (the first rows, the
last rows, and a band around every row that holds byte 2^31 or 2^32 of an operand or an output - where a 32-bit offset wraps, where a
truncated size ends, and where a store "masked" by sending it to offset 2^31 would land) are copied to the host and held, bit for bit, to
_gemm_ref's CPU arithmetic.

Every function takes the device as an argument: the host test runs the same code on small shapes on the CPU."""
from collections import namedtuple
from types import SimpleNamespace

import torch

import _gemm_ref as G
from _gemm_ref import BF16, F32, GUARD

BAND = 512
CHUNK_ELEMS = 2 ** 27            # elements of output per row chunk: 512 MiB of fp32 ("at most 1 GiB")
GIB = 2 ** 30
FORM_SMALL, FORM_PP, FORM_PP_PERSISTENT, FORM_SEAM, FORM_LOADER = 1, 2, 3, 4, 5      # include/vitamd.h VITAMD_NT_FORM_*

# ---------------------------------------------------------------------------------------------- the NT cases
# name, epilogue, M, N, K, ldo, tile codes.  M = 2^17 + 77 rows of 8200 bf16 are 2.15e9 bytes: the smallest ragged shape (rows AND columns: M % 256
# = 77, N % 256 = 8, so masked stores exist in the last tile row and the last tile column) whose bf16 output passes 2^31 bytes; twice the
# rows pass 2^32; the same rows of fp32 pass 2^32 too.  K = 4096 with 2^18 + 77 / 2^19 + 77 rows puts A past 2^31 / 2^32 bytes.
BigNt = namedtuple("BigNt", "name epi M N K ldo tiles")
ALL_TILES = (0, 4096, 2048, 1024, 256, 128)
M17, M18, M19 = 2 ** 17 + 77, 2 ** 18 + 77, 2 ** 19 + 77
NT_CASES = [
    BigNt("a-bias", G.EPI_BIAS_BF16, M17, 8200, 128, 8200, ALL_TILES),
    BigNt("a-gelu", G.EPI_GELU, M17, 8200, 128, 8200, ALL_TILES),
    BigNt("a-dmul", G.EPI_DMUL, M17, 8200, 128, 8200, (1024, 256, 128)),
    BigNt("a-dmul-n8192", G.EPI_DMUL, M17, 8192, 128, 8200, (0, 4096, 2048)),          # the seam / loader dGELU-multiply needs N % 256 == 0
    BigNt("a-bias-seam320", G.EPI_BIAS_BF16, M17, 8192, 128, 8200, (0,)),               # 408 x 32 tiles of 320 rows: >= 3 per CU, no more rounds than 256-row tiles
    BigNt("b-bias", G.EPI_BIAS_BF16, M18, 8200, 128, 8200, ALL_TILES),
    BigNt("c-bias-A2G", G.EPI_BIAS_BF16, M18, 256, 4096, 256, (0, 2048, 4096, 256, 128)),
    BigNt("c-bias-A4G", G.EPI_BIAS_BF16, M19, 256, 4096, 256, (0, 2048, 4096, 256, 128)),
    BigNt("d-resid", G.EPI_RESID_F32, M17, 8200, 128, 8200, (0, 256, 128)),
    BigNt("d-f32", G.EPI_F32, M17, 8200, 128, 8200, (0, 256, 128)),
]
DROPOUT_CASE = BigNt("d-dropout", G.EPI_RESID_F32, M17, 8200, 128, 8200, (0,))      # vitamd_linear_dropout_resid_bf16: ldo = N


def nt_id(c):
    return c.name


def form_ok(case, tile, plan):
    """the form a tile code is here for (vitamd.h: `tile`); plan = form | rows << 8"""
    form, rows = plan & 0x7f, plan >> 8
    if plan < 0:
        return False
    if case.name == "a-bias-seam320":
        return (form, rows) == (FORM_SEAM, 320)
    if tile == 0 and case.K <= 1536 and case.epi in (G.EPI_BIAS_BF16, G.EPI_GELU, G.EPI_DMUL):
        return form in (FORM_SEAM, FORM_LOADER)                                     # short K, bias, many tiles per CU
    if tile == 0 and case.epi == G.EPI_RESID_F32:
        return form in (FORM_PP, FORM_PP_PERSISTENT)                                # persistent, or a head of whole rounds + a 128x128 tail
    if tile in (0, 1024):
        return form == FORM_PP_PERSISTENT
    return (form, rows) == {4096: (FORM_SEAM, 256), 2048: (FORM_LOADER, 256), 256: (FORM_PP, 256), 128: (FORM_SMALL, 128)}[tile]


def out_esz(epi):
    return 4 if epi in G.F32_OUT else 2


def nt_spans(c):
    """{what: bytes per row} of everything a call addresses with a row index: A, and out (= out2 = the per-row aux: same ldo, no wider)"""
    return {"A": c.K * 2, "out": c.ldo * out_esz(c.epi)}


def boundary_rows(c):
    """{(what, byte): row} for the rows < M that hold byte 2^31 and byte 2^32 of A and of out.  Row 2^31 // (ldo x esz) of `out` is also where
    a store sent to offset 2^31 lands."""
    rows = {}
    for what, rb in nt_spans(c).items():
        for byte in (2 ** 31, 2 ** 32):
            if byte // rb < c.M:
                rows[(what, byte)] = byte // rb
    return rows


def bands(M, rows, band=BAND):
    """[lo, hi) row ranges: the first `band` rows, the last, and `band` rows around each of `rows`; overlapping ranges merged"""
    raw = [(0, min(band, M)), (max(0, M - band), M)]
    for r in rows:
        lo = max(0, min(r - band // 2, M - band))
        raw.append((lo, min(M, lo + band)))
    out = []
    for lo, hi in sorted(raw):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def nt_bands(c):
    return bands(c.M, sorted(set(boundary_rows(c).values())))


def row_chunks(M, N, K=0, elems=None):
    """[r0, r1) ranges whose [rows, N] output and [rows, K] operand slice both stay within `elems` (CHUNK_ELEMS) elements"""
    step = max(1, (elems or CHUNK_ELEMS) // max(N, K, 1))
    return [(r0, min(M, r0 + step)) for r0 in range(0, M, step)]


def nt_bytes_needed(c):
    """device memory a case holds at its peak, with room for the chunk temporaries: operands, aux, out (+ out2), want (+ want2)"""
    rows = c.M + 2 * GUARD
    big = rows * c.ldo * out_esz(c.epi)
    n = 2 * big                                                                      # out, want
    if c.epi in (G.EPI_GELU,):
        n += 2 * big
    if c.epi in (G.EPI_RESID_F32, G.EPI_DMUL):
        n += big
    return n + c.M * c.K * 2 + c.N * c.K * 2 + 12 * CHUNK_ELEMS * 4


# ---------------------------------------------------------------------------------------------- operands on the device
def device_ints(shape, lo, hi, seed, device, dtype=BF16):
    """_gemm_ref.ints on `device`: uniform integers lo .. hi, drawn in row chunks (no int64 image of a 2-GiB operand)"""
    g = torch.Generator(device=device).manual_seed(seed)
    out = torch.empty(shape, dtype=dtype, device=device)
    flat = out.view(shape[0], -1) if len(shape) > 1 else out.view(1, -1)
    for r0, r1 in row_chunks(flat.shape[0], flat.shape[1]):
        flat[r0:r1] = torch.randint(lo, hi + 1, (r1 - r0, flat.shape[1]), generator=g, device=device, dtype=torch.int16).to(dtype)
    return out


def device_sparse3(M, K, seed, device):
    """_gemm_ref._sparse3 on `device`: three entries of +-1 per row at random k"""
    g = torch.Generator(device=device).manual_seed(seed)
    a = torch.zeros((M, K), dtype=BF16, device=device)
    idx = torch.randint(0, K, (M, 3), generator=g, device=device)
    val = (torch.randint(0, 2, (M, 3), generator=g, device=device) * 2 - 1).to(BF16)
    a.scatter_(1, idx, val)
    return a


def sentinel(rows, ld, dtype, device):
    return torch.full((rows, ld), G.SENT16 if dtype == BF16 else G.SENT32, dtype=torch.int16 if dtype == BF16 else torch.int32, device=device)


def abs_max(t):
    return max(float(t[r0:r1].abs().max()) for r0, r1 in row_chunks(t.shape[0], t.shape[1]))


_FACTORS = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)          # _gemm_ref's EPI_DMUL factors: bf16(acc) times one of them is exact
_GELU_TAB = {}


def gelu_tables(device):
    """(bits of bf16(gelu(x)), bits of bf16(gelu'(x))) for all 65 536 bf16 inputs x, from _gemm_ref.gelu_bits, on `device` (built once)"""
    key = str(device)
    if key not in _GELU_TAB:
        pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)
        _GELU_TAB[key] = tuple(t.to(device) for t in G.gelu_bits(pat))
    return _GELU_TAB[key]


# ---------------------------------------------------------------------------------------------- the epilogue, restated
def epilogue_rows(c, acc, bias, aux_rows, gelu_tab):
    """acc fp32 [rows, N] (exact) -> (bit patterns of out, of out2 or None, the stored values as fp32 for the column sums or None) on acc's device.
    include/vitamd.h: the bias is rounded to bf16 first, the Linear output is ONE bf16 rounding of the exact sum."""
    acc = acc + 0.0                                                                  # no negative zero
    lin = G.r16(acc + G.r16(bias)) if bias is not None else G.r16(acc)
    if c.epi == G.EPI_BIAS_BF16:
        return G.bits(lin.to(BF16)), None, None
    if c.epi == G.EPI_GELU:
        pre = G.bits(lin.to(BF16))
        return pre, gelu_tab[0][pre.long() & 0xffff], None
    if c.epi == G.EPI_RESID_F32:
        return G.bits(aux_rows[:, :c.N] + lin), None, None
    if c.epi == G.EPI_F32:
        return G.bits(acc), None, None
    if c.epi == G.EPI_DMUL:
        stored = G.r16(G.r16(acc) * aux_rows[:, :c.N].float())
        return G.bits(stored.to(BF16)), None, stored
    raise ValueError(c.epi)


def nt_problem(c, device, seed=None):
    """Operands, auxiliary inputs and the expected buffers of one big vitamd_gemm_nt_bf16 call, all on `device`.  Asserts, on the reference
    alone, the bound the exact method rests on: max|a| x max|b| x K < 2^24 in units of the operands' quantum."""
    epi, M, N, K, ldo = c.epi, c.M, c.N, c.K, c.ldo
    seed = seed if seed is not None else 500000 + M * 31 + N * 17 + K * 7 + ldo * 3 + epi
    p = SimpleNamespace(case=c, out_dtype=F32 if epi in G.F32_OUT else BF16, bias=None, aux=None, colsum0=None, colsum_want=None, want2=None, scale=1.0)
    if epi == G.EPI_DMUL:
        p.a, p.b = device_sparse3(M, K, seed, device), device_ints((N, K), -1, 1, seed + 1, device)              # |acc| <= 3: the column sums stay exact
    elif epi == G.EPI_GELU:
        p.a, p.b = device_ints((M, K), -3, 3, seed, device), device_ints((N, K), -2, 3, seed + 1, device)
        p.scale = 2.0 ** -G.gelu_shift(K)
        p.a *= p.scale                                                                                         # a power of two: exact in bf16
    else:
        p.a, p.b = device_ints((M, K), -3, 2, seed, device), device_ints((N, K), -2, 3, seed + 1, device)
    p.units = abs_max(p.a) / p.scale * abs_max(p.b) * K
    assert p.units < G.EXACT, f"{c.name}: max|a| max|b| K = {p.units:.3g} quanta is not below 2^24"
    if epi == G.EPI_GELU:
        p.bias = device_ints((N,), -8, 8, seed + 2, device, F32) * 0.25
    elif epi in (G.EPI_BIAS_BF16, G.EPI_RESID_F32):
        p.bias = device_ints((N,), -4, 5, seed + 2, device, F32)
        p.bias[1::2] += 2.0 ** -9                                                    # not bf16-exact beside an integer: the kernels round the bias first
    if epi == G.EPI_RESID_F32:
        p.aux = device_ints((M, ldo), -7, 8, seed + 3, device, F32)
    elif epi == G.EPI_DMUL:
        fac = torch.tensor(_FACTORS, device=device, dtype=BF16)
        p.aux = torch.empty((M, ldo), dtype=BF16, device=device)
        for r0, r1 in row_chunks(M, ldo):
            p.aux[r0:r1] = fac[device_ints((r1 - r0, ldo), 0, 6, seed + 3 + r0, device, torch.int16).long()]
        p.colsum0 = device_ints((N,), -9, 10, seed + 5, device, F32)
    tab = gelu_tables(device) if epi == G.EPI_GELU else None
    p.want = sentinel(M + 2 * GUARD, ldo, p.out_dtype, device)
    if epi == G.EPI_GELU:
        p.want2 = sentinel(M + 2 * GUARD, ldo, BF16, device)
    bf = p.b.float()
    colsum = None if p.colsum0 is None else p.colsum0.double()
    stored_max = 0.0
    for r0, r1 in row_chunks(M, N, K):
        acc = p.a[r0:r1].float() @ bf.t()
        o, o2, stored = epilogue_rows(c, acc, p.bias, None if p.aux is None else p.aux[r0:r1], tab)
        p.want[GUARD + r0:GUARD + r1, :N] = o
        if o2 is not None:
            p.want2[GUARD + r0:GUARD + r1, :N] = o2
        if stored is not None:
            colsum += stored.double().sum(0)
            stored_max = max(stored_max, float(stored.abs().max()))
        del acc, o, o2, stored
    if colsum is not None:
        G.exact_sum_bound(M, stored_max, 0.5, c.name + " colsum", prefill=10.0)      # multiples of 0.5, exact in fp32 whatever the order of the atomics
        p.colsum_want = colsum.float()
    return p


def cpu_rows(c, a_rows, b, bias, aux_rows):
    """_gemm_ref's CPU arithmetic for some rows: (bits of out, bits of out2 or None).  GELU through _gemm_ref.gelu_bits itself."""
    acc = a_rows.float() @ b.float().t()
    tab = None
    if c.epi == G.EPI_GELU:
        pre = G.bits(G.r16(acc + 0.0 + G.r16(bias)).to(BF16))
        return pre, G.gelu_bits(pre)[0]
    o, o2, _ = epilogue_rows(c, acc, bias, aux_rows, tab)
    return o, o2


def check_reference_bands(p):
    """the device reference against the CPU on nt_bands(case): bit for bit; returns the bands"""
    c = p.case
    cpu = lambda t: None if t is None else t.cpu()
    b, bias = p.b.cpu(), cpu(p.bias)
    bs = nt_bands(c)
    for lo, hi in bs:
        o, o2 = cpu_rows(c, p.a[lo:hi].cpu(), b, bias, None if p.aux is None else p.aux[lo:hi].cpu())
        G.assert_bits_equal(f"{c.name}: device reference, rows {lo}..{hi - 1}", p.want[GUARD + lo:GUARD + hi, :c.N].cpu(), o, guard=-lo)
        if o2 is not None:
            G.assert_bits_equal(f"{c.name}: device reference of out2, rows {lo}..{hi - 1}", p.want2[GUARD + lo:GUARD + hi, :c.N].cpu(), o2, guard=-lo)
    return bs


# ---------------------------------------------------------------------------------------------- comparing whole buffers
def assert_equal_chunked(name, got, want, guard=GUARD, elems=None, settle=None):
    """bit equality of two [rows, ld] integer tensors, chunk by chunk with torch.equal; the message names the chunk, the first differing element and
    how many differ in that chunk.  settle(got_chunk, want_chunk, r0, r1) may return got_chunk with tolerated elements set to want's."""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    for k, (r0, r1) in enumerate(row_chunks(got.shape[0], got.shape[1], elems=elems)):
        g, w = got[r0:r1], want[r0:r1]
        if torch.equal(g, w):
            continue
        if settle is not None:
            g = settle(g, w, r0, r1)
            if torch.equal(g, w):
                continue
        bad = (g != w).nonzero()
        r, col = int(bad[0][0]) + r0, int(bad[0][1])
        raise AssertionError(f"{name}: chunk {k} (buffer rows {r0}..{r1 - 1}): {bad.shape[0]} elements differ; first at buffer row {r} (logical {r - guard}), "
                             f"column {col}: got {int(got[r, col]) & 0xffffffff:#x}, want {int(want[r, col]) & 0xffffffff:#x}")


def gelu_out2_settle(pre_bits_buf, M, N, guard=GUARD):
    """out2 = gelu(pre): bit-exact for inputs inside the table range; outside it (|x| < 2^-13, |x| >= 8: the formula) one unit in the last place with
    the same sign, or 1e-12 absolute - the contract of _gemm_ref._gelu_outside_ok, on the device.  pre_bits_buf: the framed buffer of the
    pre-activations' bit patterns; nothing outside its logical [M, N] region is tolerated."""
    def settle(g, w, r0, r1):
        mag = pre_bits_buf[r0:r1].int() & 0x7fff
        outside = (mag < 0x3900) | (mag >= 0x4100)
        rows = torch.arange(r0, r1, device=g.device)
        outside &= ((rows >= guard) & (rows < guard + M))[:, None]
        outside[:, N:] = False
        gi, wi = g.int() & 0xffff, w.int() & 0xffff
        near = ((gi & 0x7fff) - (wi & 0x7fff)).abs() <= 1
        near &= (gi >> 15) == (wi >> 15)
        tiny = (g.view(BF16).double() - w.view(BF16).double()).abs() <= 1e-12
        return torch.where(outside & (near | tiny), w, g)
    return settle


# ---------------------------------------------------------------------------------------------- TN GEMM at the guard
TN_BIG_LD, TN_BIG_OFF, TN_PQ, TN_BR = 4096, 768, 64, 64
TN_MAX_R = 2 ** 31 // (TN_BIG_LD * 2) - TN_BR - 1           # the largest R with (R + 64) x ld x 2 < 2^31: 262 079


def tn_guard_accepts(R, ld):
    """include/vitamd.h, vitamd_gemm_tn_bf16: (R + 64) x ld x 2 must be below 2^31"""
    return (R + TN_BR) * ld * 2 < 2 ** 31


def tn_problem(R, big, device, seed=700000):
    """L [R, 64] and Rm [R, 64] as column slices; `big` ('L' or 'R') is a slice of a [R, 4096] buffer whose other columns hold NaN (2 GiB), the other of a
    [R, 128] one.  Integers -2..1 and -3..2: |l r| <= 6, R x 6 < 2^24."""
    p = SimpleNamespace(R=R, big=big)
    p.ldl, p.ldr = (TN_BIG_LD, 128) if big == "L" else (128, TN_BIG_LD)
    p.loff, p.roff = (TN_BIG_OFF, 32) if big == "L" else (32, TN_BIG_OFF)
    p.lbuf = torch.full((R, p.ldl), float("nan"), dtype=BF16, device=device)
    p.rbuf = torch.full((R, p.ldr), float("nan"), dtype=BF16, device=device)
    p.lbuf[:, p.loff:p.loff + TN_PQ] = device_ints((R, TN_PQ), -2, 1, seed, device)
    p.rbuf[:, p.roff:p.roff + TN_PQ] = device_ints((R, TN_PQ), -3, 2, seed + 1, device)
    G.exact_sum_bound(R, 6.0, 1.0, f"tn R{R} out", prefill=5.0)
    G.exact_sum_bound(R, 2.0, 1.0, f"tn R{R} colsum", prefill=10.0)
    l, r = p.lbuf[:, p.loff:p.loff + TN_PQ].double(), p.rbuf[:, p.roff:p.roff + TN_PQ].double()
    p.init = device_ints((TN_PQ, TN_PQ), -5, 5, seed + 2, device, F32)
    p.colsum0 = device_ints((TN_PQ,), -9, 10, seed + 3, device, F32)
    prod = l.t() @ r
    p.want_ovw, p.want_acc = prod.float(), (p.init.double() + prod).float()
    p.colsum_want = (p.colsum0.double() + l.sum(0)).float()
    for t in (p.want_ovw, p.want_acc, p.colsum_want):
        assert bool(torch.isfinite(t).all()), "NaN padding reached the reference"
    return p


# ---------------------------------------------------------------------------------------------- streaming kernels past 2^31 / 2^32 elements
def flat_bands(n, marks, band=4096):
    """[lo, hi) element ranges: the first `band`, the last, and `band` around each of `marks`"""
    return bands(n, marks, band)


def ln_reference_rows(x64, eps):
    """fp64 LayerNorm without affine of some rows: (y, mean, rstd)"""
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x64 - mean) * rstd, mean[:, 0], rstd[:, 0]


def bf16_ulps(got_bf16, ref64):
    """|got - ref| in units of the bf16 spacing at the reference value (2^(floor(log2|ref|) - 7)); exact zeros of the reference count absolute differences
    in units of 2^-133 (the smallest bf16 subnormal)"""
    ref = ref64.double()
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return (got_bf16.double() - ref).abs() / torch.pow(2.0, e - 7)
