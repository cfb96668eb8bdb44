"""The three GEMM families exactly at the edges of their C-ABI contract (include/vitamd.h), on a real MI355X: ragged and N % 8 == 4 shapes,
leading dimensions wider than the logical width, every kernel form x every fused epilogue, the tail split, strided TN operands.

Every reference is exact (tests/_gemm_ref.py: integer operands, one documented bf16 rounding) and every comparison is bit equality on a
sentinel-framed buffer, so one mis-indexed column, one store past a ragged edge or one wrong stride fails a case.  The kernels are called
through the C ABI (vitamd.lib.load()): the host wrappers cannot pass a leading dimension.  The kernel form of every NT case is taken from
vitamd_gemm_nt_plan and ASSERTED, so a dispatch change cannot silently move a case onto another kernel; combinations the header refuses
must come back VITAMD_ERR_SHAPE with nothing written.  tests/test_gemm_ref_host.py imports the case lists below."""
from types import SimpleNamespace

import pytest
import torch

import _gemm_ref as G
from _gemm_ref import BF16, F32, GUARD, NtCase, TnCase

pytestmark = pytest.mark.gpu

ERR_SHAPE = 1
FORM_SMALL, FORM_PP, FORM_PP_PERSISTENT, FORM_SEAM, FORM_LOADER, FORM_TAIL_SPLIT = 1, 2, 3, 4, 5, 0x80      # include/vitamd.h VITAMD_NT_FORM_*
TALL_EPIS = (G.EPI_BIAS_BF16, G.EPI_GELU, G.EPI_RESID_F32, G.EPI_DGELU, G.EPI_GELU_DG, G.EPI_DMUL)           # "320: bias, GELU, residual and dGELU epilogues only"
SEAM_EPIS = (G.EPI_BIAS_BF16, G.EPI_GELU, G.EPI_GELU_DG, G.EPI_DMUL)                                         # "bias / GELU / dGELU-multiply epilogues"

# ---------------------------------------------------------------------------------------------- the cases
# (M, N, K, ldo).  M in {1, 255, 257, 321, 600}, K in {64, 128, 192}, N in {4, 260, 264, 512, 520}, ldo in {N, N + 8, N + 4}: every kernel form x
# epilogue meets a ragged M, a ragged N with N % 8 == 0 (264, 520), N % 8 == 4 (4, 260: the direct-store epilogue inside the 256- / 320-row
# kernels), ldo > N, and ldo % 8 == 4 with N % 8 == 0 (the direct epilogue again) - or the refusal the header states for that combination.
# The last shape is M = 1 where the loader-wave and seam forms run too (K >= 128, N % 256 == 0): one valid row in a 256-row tile.
NT_SHAPES = [(255, 264, 192, 264), (321, 520, 128, 528), (600, 260, 64, 260), (1, 4, 64, 8), (257, 512, 128, 520), (257, 264, 64, 268),
             (1, 512, 128, 520)]
NT_SHAPE_GELU_M1 = (1, 260, 64, 264)          # M = 1 for the GELU epilogues: four elements cannot be 90 % inside the table with one outside
NT_TILES = (128, 256, 320, 2048, 4096)


def _nt_small_cases():
    cases = []
    for tile in NT_TILES:
        for epi in range(8):
            for shape in NT_SHAPES:
                if shape == NT_SHAPES[3] and epi in (G.EPI_GELU, G.EPI_GELU_DG):
                    shape = NT_SHAPE_GELU_M1
                cases.append(NtCase(tile, epi, *shape))
    return cases


NT_SMALL_CASES = _nt_small_cases()

# the persistent ping-pong form: tile 0 (and 1024) on 65 x 4 = 260 big tiles, K = 64 (too short for the seam / loader forms).  N = 776: ragged last column
# tile on the row epilogue, 320-row tiles for the residual and dGELU epilogues, 256-row tiles for the patch and fp32 ones; N = 772: the direct epilogue.
BIG_M = 256 * 64 + 77
NT_BIG_CASES = [NtCase(0, epi, BIG_M, N, 64, ldo) for (N, ldo) in ((776, 784), (772, 776))
                for epi in (G.EPI_RESID_F32, G.EPI_PATCH_F32, G.EPI_DGELU, G.EPI_DMUL, G.EPI_F32)]
NT_BIG_CASES += [NtCase(1024, epi, BIG_M, 776, 64, 776) for epi in (G.EPI_RESID_F32, G.EPI_F32)]
NT_BIG_CASES += [NtCase(0, epi, BIG_M, 776, 64, 784) for epi in (G.EPI_BIAS_BF16, G.EPI_GELU, G.EPI_GELU_DG)]      # the other three selectors, 320-row tiles

# the tail split: the first M (searched through vitamd_gemm_nt_plan) at which the plan of a fused-residual launch carries VITAMD_NT_FORM_TAIL_SPLIT, and
# the same M + TAIL_EXTRA, so that the 128x128 tail has more than one tile row.  (N, K, ldo, the M a 256-CU part gives: what the host test builds.)
TAIL_EXTRA = 130
TAIL_SEARCH_BOUND = 400000
TAIL_SHAPES = [(768, 64, 776, 54401 + TAIL_EXTRA), (260, 64, 260, 65537 + TAIL_EXTRA)]
NT_REFUSED_K = 96                              # passes the first argument check (K % 32) and must be refused by every tile code
NT_ALL_TILE_CODES = (0, 128, 256, 320, 512, 1024, 2048, 4096)

SKINNY_MS = (1, 15, 16, 17, 33, 48, 49, 64)    # all four MT instantiations, each with a full and a ragged last 16-row group
SKINNY_NK = [(4, 64), (260, 64), (1000, 320), (776, 192), (68, 1088), (2304, 768)]
SKINNY_SHORT_LAST_SPLIT = [(68, 1088), (1000, 320)]
SKINNY_QKV = [(17, 2, 192), (33, 2, 192)]      # (M, H, K)

# (R, P, Q, ldo, splits, accumulate): R in {1, 63, 100, 1000}, P in {100, 260, 768}, Q in {64, 258, 264}, ldo in {Q, Q + 4, Q + 3}, splits in {0, 1, 3},
# accumulate in {0, 1}; each case runs the shared, the exclusive and the atomic form (the atomic form can only accumulate) and the colsum calls.
# The last case, ldo = Q + 2: Q % 4 != 0 with ldo % 4 == 0, where only the `q + 3 < Q` guard keeps the reduce pass's 16-byte store inside the row.
TN_CASES = [TnCase(1, 100, 64, 64, 0, 0), TnCase(63, 260, 258, 262, 1, 1), TnCase(100, 768, 264, 267, 3, 0), TnCase(1000, 260, 264, 268, 3, 1),
            TnCase(1000, 768, 64, 67, 0, 1), TnCase(100, 100, 258, 258, 1, 0), TnCase(63, 768, 64, 68, 3, 1),
            TnCase(100, 260, 258, 260, 3, 0)]


def nt_expected_plan(c):
    """vitamd_gemm_nt_plan's answer for an explicit tile code as the header states the rules; None = VITAMD_ERR_SHAPE"""
    tile, epi, M, N, K, ldo = c
    if K % 64 or N % 4 or ldo % 4:
        return None
    if tile == 128:
        return FORM_SMALL | 128 << 8
    if tile == 256:
        return FORM_PP | 256 << 8
    if tile == 320:
        return FORM_PP | 320 << 8 if epi in TALL_EPIS else None
    ok = epi in SEAM_EPIS and K >= 128 and N % 8 == 0 and ldo % 8 == 0 and (epi != G.EPI_DMUL or N % 256 == 0)
    if tile == 2048:
        return FORM_LOADER | 256 << 8 if ok and K % 128 == 0 else None
    if tile == 4096:
        return FORM_SEAM | 256 << 8 if ok else None
    raise ValueError(tile)


# ---------------------------------------------------------------------------------------------- calling the ABI
def _st():
    return torch.cuda.current_stream().cuda_stream


def _d(t):
    return None if t is None else t.cuda()


def _ptr(t, offset_bytes=0):
    return None if t is None else t.data_ptr() + offset_bytes


def _nt_device(p):
    """the inputs of a problem on the device, once per case"""
    return SimpleNamespace(a=_d(p.a), b=_d(p.b), bias=_d(p.bias), aux=_d(p.aux))


def _nt_call(hip, p, d, tile=None, colsum=True):
    """one vitamd_gemm_nt_bf16 call into fresh sentinel-framed buffers -> (return code, what it left behind, on the CPU)"""
    c = p.case
    rows = p.want.shape[0]
    esz = 4 if p.out_dtype == F32 else 2
    out = G.sentinel(rows, c.ldo, p.out_dtype).cuda()
    out2 = G.sentinel(rows, c.ldo, BF16).cuda() if c.epi in (G.EPI_GELU, G.EPI_GELU_DG) else None
    cs = _d(p.colsum0) if colsum and p.colsum0 is not None else None
    code = hip.vitamd_gemm_nt_bf16(_ptr(d.a), _ptr(d.b), _ptr(out, GUARD * c.ldo * esz), _ptr(out2, GUARD * c.ldo * 2), _ptr(d.bias), _ptr(d.aux), _ptr(cs),
                                   c.M, c.N, c.K, c.ldo, c.epi, p.n_patches, p.seq, p.extra, c.tile if tile is None else tile, _st())
    torch.cuda.synchronize()
    return code, SimpleNamespace(out=out.cpu(), out2=None if out2 is None else out2.cpu(), colsum=None if cs is None else cs.cpu())


def _nt_run_and_check(hip, p, reps, record_property):
    c = p.case
    d = _nt_device(p)
    code, first = _nt_call(hip, p, d)
    assert code == 0, (G.nt_id(c), code)
    stats = G.nt_check(p, first)
    for rep in range(1, reps):                                                    # again on the persistent forms: a race would not repeat
        code, got = _nt_call(hip, p, d)
        assert code == 0 and torch.equal(got.out, first.out), (G.nt_id(c), code, rep)
        assert got.out2 is None or torch.equal(got.out2, first.out2)
        assert got.colsum is None or torch.equal(got.colsum, first.colsum)       # exact sums: the order of the atomics does not show
    if c.epi == G.EPI_DMUL:                                                       # colsum == NULL: `out` bit-identical (the seam / loader forms compile the sums out)
        code, got = _nt_call(hip, p, d, colsum=False)
        assert code == 0
        G.nt_check(p, got)
    for k, v in stats.items():
        record_property(k, v)
        print(f"STAT {G.nt_id(c)} {k}={v:.4g}")


@pytest.fixture(scope="module")
def hip_init(hip):
    from vitamd import ops
    ops.init()                                                                   # vitamd_init: the GELU table of this device
    return hip


# ---------------------------------------------------------------------------------------------- NT GEMM
@pytest.mark.parametrize("case", NT_SMALL_CASES, ids=G.nt_id)
def test_nt_every_form_and_epilogue_at_the_shape_edges(hip_init, case, record_property):
    hip = hip_init
    plan = hip.vitamd_gemm_nt_plan(case.M, case.N, case.K, case.ldo, case.epi, case.tile)
    want_plan = nt_expected_plan(case)
    print(f"FORM nt {G.nt_id(case)} plan={plan:#x}" if plan >= 0 else f"FORM nt {G.nt_id(case)} refused={-plan}")
    p = G.nt_problem(case)
    if want_plan is None:                                                        # the header refuses this form / epilogue / shape combination
        assert plan == -ERR_SHAPE, (G.nt_id(case), plan)
        code, got = _nt_call(hip, p, _nt_device(p))
        assert code == ERR_SHAPE, (G.nt_id(case), code)
        G.assert_untouched(G.nt_id(case) + " out", got.out)
        if got.out2 is not None:
            G.assert_untouched(G.nt_id(case) + " out2", got.out2)
        if got.colsum is not None:
            assert torch.equal(got.colsum, p.colsum0)
        return
    assert plan == want_plan, (G.nt_id(case), hex(plan), hex(want_plan))
    _nt_run_and_check(hip, p, 2 if case.tile in (2048, 4096) else 1, record_property)


@pytest.mark.parametrize("case", NT_BIG_CASES, ids=G.nt_id)
def test_nt_persistent_pingpong_against_the_reference(hip_init, case, record_property):
    """Tile 0 / 1024 on 260 big tiles: one workgroup per CU walks a strided tile list (gemm_nt_pp_kernel, PERS), on 256- and 320-row tiles, row and
    direct epilogue - against the exact reference, twice."""
    hip = hip_init
    plan = hip.vitamd_gemm_nt_plan(case.M, case.N, case.K, case.ldo, case.epi, case.tile)
    print(f"FORM nt {G.nt_id(case)} plan={plan:#x}")
    tall = case.epi in TALL_EPIS and case.N % 8 == 0 and case.ldo % 8 == 0       # one round of 320-row tiles instead of two of 256-row ones
    assert plan == FORM_PP_PERSISTENT | (320 if tall else 256) << 8, hex(plan)
    _nt_run_and_check(hip, G.nt_problem(case), 2, record_property)


def find_tail_split(plan, N, K, ldo):
    """the first M whose fused-residual launch is planned with a tail split, and stays so TAIL_EXTRA rows further"""
    for M in range(1, TAIL_SEARCH_BOUND):
        if plan(M, N, K, ldo, G.EPI_RESID_F32, 0) & FORM_TAIL_SPLIT and plan(M + TAIL_EXTRA, N, K, ldo, G.EPI_RESID_F32, 0) & FORM_TAIL_SPLIT:
            return M + TAIL_EXTRA
    return None


def _head_rows(M, N):
    """rows of the head part of a tail-split launch (include/vitamd.h: whole rounds of 256-row tiles, one workgroup per CU)"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    tiles_n = (N + 255) // 256
    big = ((M + 255) // 256) * tiles_n
    return (big - big % cus) // tiles_n * 256


@pytest.mark.parametrize("N,K,ldo,_m256", TAIL_SHAPES, ids=[f"N{s[0]}-ldo{s[2]}" for s in TAIL_SHAPES])
def test_nt_tail_split_residual_exact_across_the_seam(hip_init, N, K, ldo, _m256, record_property):
    """vitamd_gemm_nt_impl cuts the launch into a head on 256-row tiles and a tail on 128x128 tiles with re-based A, out and aux pointers: the fused
    residual must be exact on both sides of the seam, with ldo > N (N = 768) and on the direct epilogue (N = 260)."""
    hip = hip_init
    M = find_tail_split(hip.vitamd_gemm_nt_plan, N, K, ldo)
    assert M is not None, f"no tail split below M = {TAIL_SEARCH_BOUND} at N = {N}"
    plan = hip.vitamd_gemm_nt_plan(M, N, K, ldo, G.EPI_RESID_F32, 0)
    head = _head_rows(M, N)
    print(f"FORM nt tail-split N{N} M={M} head_rows={head} plan={plan:#x}")
    assert plan == FORM_PP | FORM_TAIL_SPLIT | 256 << 8, hex(plan)
    assert 0 < head < M
    record_property("M", M)
    _nt_run_and_check(hip, G.nt_problem(NtCase(0, G.EPI_RESID_F32, M, N, K, ldo)), 1, record_property)


def test_nt_tail_split_dropout_mask_is_global_across_the_seam(hip):
    """vitamd_linear_dropout_resid_bf16 through the tail split: a zero GEMM with bias 2 and a zero residual shows the mask directly.  Element
    (row, col) must use index row * N + col on both sides of the seam (the tail launch carries row0 = the head's rows)."""
    import numpy as np
    import _dropout_ref as DR
    N, K, P, SEED = 768, 64, 0.25, 0x5EED1234ABCD
    M = find_tail_split(hip.vitamd_gemm_nt_plan, N, K, N)
    assert M is not None, f"no tail split below M = {TAIL_SEARCH_BOUND}"
    head = _head_rows(M, N)
    assert 0 < head < M
    a = torch.zeros((M, K), dtype=BF16, device="cuda")
    w = torch.zeros((N, K), dtype=BF16, device="cuda")
    bias = torch.full((N,), 2.0, device="cuda")
    resid = torch.zeros((M, N), device="cuda")
    out = G.sentinel(M + 2 * GUARD, N, F32).cuda()
    code = hip.vitamd_linear_dropout_resid_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr() + GUARD * N * 4, bias.data_ptr(), resid.data_ptr(),
                                                M, N, K, P, SEED, 0, _st())
    torch.cuda.synchronize()
    assert code == 0
    out = out.cpu()
    G.assert_untouched("guard rows", torch.cat([out[:GUARD], out[GUARD + M:]]))
    y = out[GUARD:GUARD + M].view(torch.float32)
    kept = G.r16(torch.tensor(2.0 * float(DR.scale(P)))).item()
    assert bool(((y == 0) | (y == kept)).all())
    # the mask itself on the first rows, 600 rows on either side of the seam, the last rows and every 61st row between
    rows = np.unique(np.concatenate([np.arange(0, 300), np.arange(head - 600, min(head + 600, M)), np.arange(M - 300, M), np.arange(0, M, 61)]))
    idx = (rows[:, None].astype(np.uint64) * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :])
    keep = torch.from_numpy(DR.keep(idx, SEED, P))
    got = y[torch.from_numpy(rows)] != 0
    bad = (got != keep).nonzero()
    assert bad.numel() == 0, f"mask differs in {bad.shape[0]} elements; first at row {int(rows[int(bad[0][0])])} (head has {head} rows), column {int(bad[0][1])}"


def test_nt_k96_is_refused_by_every_tile_code(hip_init):
    """K = 96 passes the first argument check (K % 32 == 0); the requirement is K % 64 == 0 and every tile code must refuse it with nothing written"""
    hip = hip_init
    case = NtCase(0, G.EPI_BIAS_BF16, 257, 264, 128, 272)
    p = G.nt_problem(case)
    d = _nt_device(p)
    d.a, d.b = d.a[:, :NT_REFUSED_K].contiguous(), d.b[:, :NT_REFUSED_K].contiguous()
    p.case = case._replace(K=NT_REFUSED_K)
    for tile in NT_ALL_TILE_CODES:
        assert hip.vitamd_gemm_nt_plan(case.M, case.N, NT_REFUSED_K, case.ldo, case.epi, tile) == -ERR_SHAPE, tile
        code, got = _nt_call(hip, p, d, tile=tile)
        assert code == ERR_SHAPE, (tile, code)
        G.assert_untouched(f"tile {tile}", got.out)


# ---------------------------------------------------------------------------------------------- skinny GEMM
def _skinny_call(hip, p, d, ws, ws_bytes):
    esz = 4 if p.out_dtype == F32 else 2
    out = G.sentinel(p.M + 2 * GUARD, p.N, p.out_dtype).cuda()
    out2 = G.sentinel(p.M + 2 * GUARD, p.N, BF16).cuda() if p.epi == G.EPI_GELU else None
    code = hip.vitamd_gemm_skinny_bf16(_ptr(d.a), _ptr(d.w), _ptr(out, GUARD * p.N * esz), _ptr(out2, GUARD * p.N * 2), _ptr(d.bias), _ptr(d.aux),
                                       p.M, p.N, p.K, p.epi, _ptr(ws), ws_bytes, _st())
    torch.cuda.synchronize()
    return code, SimpleNamespace(out=out.cpu(), out2=None if out2 is None else out2.cpu())


@pytest.mark.parametrize("N,K", SKINNY_NK)
def test_skinny_every_m_and_epilogue_at_the_shape_edges(hip_init, N, K):
    """M over all four MT instantiations with full and ragged last row groups; N with a ragged last 64-column workgroup, N = 4; K = 64 and K whose
    last split is shorter than the others.  Split-K sums of integers are exact: equality through the reduce pass, and run to run."""
    hip = hip_init
    for M in SKINNY_MS:
        ws_bytes = hip.vitamd_gemm_skinny_ws_bytes(M, N, K)
        assert ws_bytes >= 0
        splits = ws_bytes // (M * N * 4) if ws_bytes else 1
        assert ws_bytes == (splits * M * N * 4 if splits > 1 else 0)
        ks = G.skinny_ks_candidates(K, splits)
        assert ks, (M, N, K, splits)
        if M == SKINNY_MS[0]:
            print(f"FORM skinny N{N} K{K} splits={splits} ks={ks} last={[K - (splits - 1) * k for k in ks]}")
        if (N, K) in SKINNY_SHORT_LAST_SPLIT:                                     # the plan this case is here for
            assert splits > 1 and all(K - (splits - 1) * k < k for k in ks), (splits, ks)
        ws = torch.full((max(ws_bytes // 4, 1),), float("nan"), device="cuda")
        for epi in G.SKINNY_EPIS:
            p = G.skinny_problem(M, N, K, epi)
            d = SimpleNamespace(a=_d(p.a), w=_d(p.w), bias=_d(p.bias), aux=_d(p.aux))
            outs = []
            for rep in range(2):                                                 # run to run
                code, got = _skinny_call(hip, p, d, ws if ws_bytes else None, ws_bytes)
                assert code == 0, (M, N, K, epi, code)
                G.skinny_check(p, got)
                outs.append(got)
            assert torch.equal(outs[0].out, outs[1].out) and (outs[0].out2 is None or torch.equal(outs[0].out2, outs[1].out2))
        print(f"FORM skinny M{M} N{N} K{K} MT={(M + 15) // 16} splits={splits}")


@pytest.mark.parametrize("M,H,K", SKINNY_QKV)
def test_skinny_qkv_append_equals_gemm_plus_kv_append(hip, M, H, K):
    """qkv bit-equal to vitamd_gemm_skinny_bf16(BIAS_BF16) and to the exact reference, the caches bit-equal to vitamd_kv_append(T = 1), and a
    sentinel-filled cache untouched everywhere except row *len - at M with a ragged last row group (17: MT = 2, 33: MT = 3)."""
    N, Lmax, pos = 3 * H * 64, 8, 5
    p = G.skinny_problem(M, N, K, G.EPI_BIAS_BF16)
    d = SimpleNamespace(a=_d(p.a), w=_d(p.w), bias=_d(p.bias), aux=None)
    ws_bytes = hip.vitamd_gemm_skinny_ws_bytes(M, N, K)
    ws = torch.full((max(ws_bytes // 4, 1),), float("nan"), device="cuda")
    code, plain = _skinny_call(hip, p, d, ws if ws_bytes else None, ws_bytes)
    assert code == 0
    G.skinny_check(p, plain)
    length = torch.tensor([pos], dtype=torch.int32, device="cuda")
    qkv = G.sentinel(M + 2 * GUARD, N, BF16).cuda()
    caches = [G.sentinel(M * H * Lmax, 64, BF16).cuda() for _ in range(4)]         # k, v of the fused call; k, v of vitamd_kv_append
    code = hip.vitamd_gemm_skinny_qkv_append(_ptr(d.a), _ptr(d.w), _ptr(qkv, GUARD * N * 2), _ptr(d.bias), _ptr(caches[0]), _ptr(caches[1]), _ptr(length),
                                             M, H, K, 64, Lmax, _ptr(ws) if ws_bytes else None, ws_bytes, _st())
    assert code == 0
    code = hip.vitamd_kv_append(_ptr(qkv, GUARD * N * 2), _ptr(caches[2]), _ptr(caches[3]), _ptr(length), M, 1, H, 64, Lmax, _st())
    assert code == 0
    torch.cuda.synchronize()
    assert torch.equal(qkv.cpu(), plain.out)
    kc, vc, kc2, vc2 = (c.cpu().view(M, H, Lmax, 64) for c in caches)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)
    logical = p.want_logical.view(M, 3, H, 64)
    for cache, which in ((kc, 1), (vc, 2)):
        assert torch.equal(cache[:, :, pos], logical[:, which])
        rest = torch.ones(Lmax, dtype=torch.bool)
        rest[pos] = False
        G.assert_untouched("cache rows other than *len", cache[:, :, rest].reshape(-1, 64))


# ---------------------------------------------------------------------------------------------- TN GEMM
@pytest.mark.parametrize("case", TN_CASES, ids=G.tn_id)
def test_tn_strided_operands_and_dimension_edges(hip, case):
    """L and Rm are column slices of wider buffers whose other columns are NaN (ldl, ldr > the logical width, P % 8 != 0: the last 16-byte chunk
    of a row reaches into the NaN); out is a [P + 2, ldo] sentinel buffer with ldo % 4 != 0 and Q % 4 != 0 among the cases (the scalar path
    of the reduce pass).  Integer operands: equality in every split order and with atomics; exclusive == shared; the colsum call's out == the plain
    call's, its colsum exact."""
    R, P, Q, ldo, splits, accumulate = case
    p = G.tn_problem(case)
    lbuf, rbuf = p.lbuf.cuda(), p.rbuf.cuda()
    lp, rp = lbuf.data_ptr() + G.TN_LOFF * 2, rbuf.data_ptr() + G.TN_ROFF * 2
    ws_bytes = hip.vitamd_gemm_tn_ws_bytes(R, P, Q, splits)
    ws = torch.full((ws_bytes // 4,), float("nan"), device="cuda")
    print(f"FORM tn {G.tn_id(case)} ws_bytes={ws_bytes} splits_planned={ws_bytes // ((((P + 255) // 256) * ((Q + 255) // 256) * 65536 + (P + 255) // 256 * 256) * 4)}")
    results = {}
    for form, name in ((0, "shared"), (1, "exclusive")):
        before, want = G.tn_frames(p, accumulate)
        out = before.cuda()
        assert hip.vitamd_gemm_tn_bf16_ws(lp, rp, out.data_ptr(), R, P, Q, p.ldl, p.ldr, ldo, splits, ws.data_ptr(), ws_bytes, accumulate, form, _st()) == 0
        torch.cuda.synchronize()
        results[name] = out.cpu()
        G.tn_check(f"tn {name} {G.tn_id(case)}", p, results[name], want)
        out = before.cuda()
        cs = p.colsum0.cuda()
        assert hip.vitamd_gemm_tn_bf16_ws_colsum(lp, rp, out.data_ptr(), cs.data_ptr(), R, P, Q, p.ldl, p.ldr, ldo, splits, ws.data_ptr(), ws_bytes,
                                                 accumulate, form, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), results[name]), f"{name}: out of the colsum call differs from the plain call's"
        cs = cs.cpu()
        assert not bool(torch.isnan(cs).any()), f"{name}: NaN in colsum: a padding column of L leaked"
        assert torch.equal(cs, p.colsum_want), f"{name}: colsum differs in {int((cs != p.colsum_want).sum())} columns"
    assert torch.equal(results["shared"], results["exclusive"])
    before, want = G.tn_frames(p, 1)                                             # the atomic form adds into `out`
    out = before.cuda()
    assert hip.vitamd_gemm_tn_bf16(lp, rp, out.data_ptr(), R, P, Q, p.ldl, p.ldr, ldo, splits, _st()) == 0
    torch.cuda.synchronize()
    G.tn_check(f"tn atomic {G.tn_id(case)}", p, out.cpu(), want)
