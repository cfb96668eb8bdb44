"""Return codes of the LayerNorm and weight-gradient (TN) GEMM entry points for calls that are refused before any launch (no GPU): which check
answers, and which answers first.  The pointers are dummies that no such call dereferences."""
import ctypes

import pytest

SHAPE, ARG = 1, 2            # VITAMD_ERR_SHAPE, VITAMD_ERR_ARG
NAN = float("nan")
INT_MAX = 2**31 - 1
WIDTHS = (256, 512, 768, 1024)

_buf = (ctypes.c_float * 64)()
P = ctypes.addressof(_buf)


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


def _nulls(call, args, checked):
    """one null pointer at a time at each of the `checked` positions"""
    return [call(*[None if i == k else a for i, a in enumerate(args)]) for k in checked]


@pytest.mark.parametrize("M,D", [(0, 256), (-1, 256), (4, 0), (4, -4), (4, 258), (4, 770)])
def test_layernorm_shape_is_refused_first(L, M, D):
    # ... also with null pointers and a bad p: the shape answers before them
    assert L.vitamd_layernorm_fwd(P, P, P, P, P, P, M, D, 1e-5, None) == SHAPE
    assert L.vitamd_layernorm_fwd(None, None, None, None, None, None, M, D, 1e-5, None) == SHAPE
    assert L.vitamd_layernorm_bwd(P, P, P, P, P, P, P, P, M, D, None) == SHAPE
    assert L.vitamd_layernorm_bwd(None, None, None, None, None, None, None, None, M, D, None) == SHAPE
    assert L.vitamd_layernorm_bwd_dropout(P, P, P, P, P, P, P, P, M, D, 0.1, 7, None) == SHAPE
    assert L.vitamd_layernorm_bwd_dropout(None, None, None, None, None, None, None, None, M, D, NAN, 7, None) == SHAPE


@pytest.mark.parametrize("D", [256, 768, 200])
def test_layernorm_null_pointers(L, D):
    # forward: x_in, y, mean, rstd; x_out only with an addend
    assert _nulls(L.vitamd_layernorm_fwd, (P, P, P, P, P, P, 4, D, 1e-5, None), (0, 3, 4, 5)) == [ARG] * 4
    assert L.vitamd_layernorm_fwd(P, P, None, P, P, P, 4, D, 1e-5, None) == ARG
    # backward: dy, x, mean, rstd, g_out (g_res, g_bf16 and colsum are optional)
    assert _nulls(L.vitamd_layernorm_bwd, (P, P, P, P, P, P, P, P, 4, D, None), (0, 1, 2, 3, 5)) == [ARG] * 5
    assert _nulls(L.vitamd_layernorm_bwd_dropout, (P, P, P, P, P, P, P, P, 4, D, 0.1, 7, None), (0, 1, 2, 3, 5)) == [ARG] * 5


@pytest.mark.parametrize("p", [-0.1, 1.0, NAN])
def test_layernorm_bwd_dropout_probability(L, p):
    for D in (256, 200):
        assert L.vitamd_layernorm_bwd_dropout(P, P, P, P, P, P, P, P, 4, D, p, 7, None) == ARG
        assert L.vitamd_layernorm_bwd_dropout(P, P, P, P, None, P, None, None, 4, D, p, 7, None) == ARG
    assert L.vitamd_layernorm_bwd_xhat(P, P, P, P, P, P, P, 4, 256, p, 7, None) == ARG
    assert L.vitamd_layernorm_bwd_keep(P, P, P, P, P, P, P, P, 2, 5, 2, 256, 0, p, 7, None) == ARG
    assert L.vitamd_layernorm_bwd_keep(P, P, None, P, P, P, P, P, 2, 5, 2, 256, 1, p, 7, None) == ARG
    # the shape still answers before p
    assert L.vitamd_layernorm_bwd_dropout(P, P, P, P, P, P, P, P, 4, 258, p, 7, None) == SHAPE
    assert L.vitamd_layernorm_bwd_xhat(P, P, P, P, P, P, P, 4, 200, p, 7, None) == SHAPE


@pytest.mark.parametrize("D", [0, 4, 200, 128, 1280, 2048, 260])
def test_layernorm_bwd_xhat_width_before_any_pointer(L, D):
    assert L.vitamd_layernorm_bwd_xhat(P, P, P, P, P, P, P, 4, D, 0.0, 0, None) == SHAPE
    assert L.vitamd_layernorm_bwd_xhat(None, None, None, None, None, None, None, 4, D, 0.0, 0, None) == SHAPE


@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_bwd_xhat_pointers(L, D):
    assert L.vitamd_layernorm_bwd_xhat(P, P, P, P, P, P, P, 0, D, 0.0, 0, None) == SHAPE
    assert _nulls(L.vitamd_layernorm_bwd_xhat, (P, P, P, P, P, P, P, 4, D, 0.0, 0, None), (0, 1, 2, 4)) == [ARG] * 4
    assert _nulls(L.vitamd_layernorm_bwd_xhat, (P, P, P, P, P, P, P, 4, D, NAN, 0, None), (0, 1, 2, 4)) == [ARG] * 4


@pytest.mark.parametrize("B,seq,keep", [(3, 5, 6), (3, 5, 0), (3, 5, -1), (0, 5, 2), (3, 0, 0), (INT_MAX // 197 + 1, 197, 1), (2**30, 4, 1)])
def test_keep_forms_shape(L, B, seq, keep):
    for D in (256, 200):
        assert L.vitamd_layernorm_fwd_keep(P, P, P, P, P, P, B, seq, keep, D, 1e-5, None) == SHAPE
        assert L.vitamd_layernorm_fwd_keep(None, None, None, None, None, None, B, seq, keep, D, 1e-5, None) == SHAPE
        assert L.vitamd_layernorm_bwd_keep(P, P, P, P, P, P, P, P, B, seq, keep, D, 0, 0.0, 0, None) == SHAPE
        assert L.vitamd_layernorm_bwd_keep(None, None, None, None, None, None, None, None, B, seq, keep, D, 0, NAN, 0, None) == SHAPE


def test_keep_forms_width_and_pointers(L):
    for D in (0, 258):
        assert L.vitamd_layernorm_fwd_keep(P, P, P, P, P, P, 3, 5, 2, D, 1e-5, None) == SHAPE
        assert L.vitamd_layernorm_bwd_keep(P, P, P, P, P, P, P, P, 3, 5, 2, D, 0, 0.0, 0, None) == SHAPE
    # the forward needs every pointer, the addend and x_out included
    assert _nulls(L.vitamd_layernorm_fwd_keep, (P, P, P, P, P, P, 3, 5, 2, 200, 1e-5, None), range(6)) == [ARG] * 6
    # xhat form: the four register-resident widths only, asked before the pointers
    for D in (200, 128, 1280):
        assert L.vitamd_layernorm_bwd_keep(P, P, P, P, P, P, P, P, 3, 5, 2, D, 1, 0.0, 0, None) == SHAPE
        assert L.vitamd_layernorm_bwd_keep(None, None, None, None, None, None, None, None, 3, 5, 2, D, 1, 0.0, 0, None) == SHAPE
    # g_res is required (and dy, x_or_y, rstd, g_out); mean only without xhat
    for D in (256, 200):
        assert _nulls(L.vitamd_layernorm_bwd_keep, (P, P, P, P, P, P, P, P, 3, 5, 2, D, 0, 0.0, 0, None), (0, 1, 2, 3, 4, 5)) == [ARG] * 6
    assert _nulls(L.vitamd_layernorm_bwd_keep, (P, P, P, P, P, P, P, P, 3, 5, 2, 768, 1, 0.0, 0, None), (0, 1, 3, 4, 5)) == [ARG] * 5


def _tn(L, colsum, *, R=64, P_=256, Q=256, ldl=256, ldr=256, ldo=256, splits=1, ws=P, ws_bytes=1 << 30, accumulate=1, form=0, ptrs=(P, P, P)):
    if colsum is False:
        return L.vitamd_gemm_tn_bf16_ws(*ptrs, R, P_, Q, ldl, ldr, ldo, splits, ws, ws_bytes, accumulate, form, None)
    return L.vitamd_gemm_tn_bf16_ws_colsum(*ptrs, colsum, R, P_, Q, ldl, ldr, ldo, splits, ws, ws_bytes, accumulate, form, None)


@pytest.mark.parametrize("colsum", [False, None, P], ids=["False", "None", "buffer"])      # (P is an address: as an id it changes from run to run)
def test_tn_refusals(L, colsum):
    for form in (-1, 2, 7):          # before anything else: with a bad shape and null operands the answer is still the form's
        assert _tn(L, colsum, form=form) == ARG
        assert _tn(L, colsum, form=form, ldl=257, ptrs=(None, None, None)) == ARG
        assert _tn(L, colsum, form=form, R=0) == ARG
    for form in (0, 1):
        for bad in (dict(ldl=260), dict(ldr=260), dict(P_=264, ldl=256), dict(Q=264, ldr=256, ldo=264), dict(Q=264, ldr=264, ldo=256),
                    dict(R=0), dict(P_=0), dict(Q=-1)):
            assert _tn(L, colsum, form=form, **bad) == SHAPE, bad
            assert _tn(L, colsum, form=form, ptrs=(None, None, None), **bad) == SHAPE, bad      # shape before pointers
        for k in range(3):
            assert _tn(L, colsum, form=form, ptrs=tuple(None if i == k else P for i in range(3))) == ARG
        # overwrite mode needs a workspace that holds splits x tiles partial tiles (+ the column-sum partials): absent, or one byte short
        need = L.vitamd_gemm_tn_ws_bytes(64, 256, 256, 1)
        assert need == (256 * 256 + 256) * 4
        short = need - 256 * 4 - 1 if colsum is not P else need - 1
        assert _tn(L, colsum, form=form, accumulate=0, ws=None, ws_bytes=0) == ARG
        assert _tn(L, colsum, form=form, accumulate=0, ws_bytes=short) == ARG
        assert _tn(L, colsum, form=form, accumulate=0, ws_bytes=-1) == ARG


def test_tn_colsum_needs_the_workspace(L):
    need = L.vitamd_gemm_tn_ws_bytes(64, 256, 256, 1)
    for form in (0, 1):
        for accumulate in (0, 1):
            assert _tn(L, P, form=form, accumulate=accumulate, ws=None, ws_bytes=0) == ARG
            assert _tn(L, P, form=form, accumulate=accumulate, ws=None, ws_bytes=need) == ARG
            assert _tn(L, P, form=form, accumulate=accumulate, ws_bytes=need - 1) == ARG           # room for the tiles but not for the column sums
            assert _tn(L, P, form=form, accumulate=accumulate, ws=None, ws_bytes=need, ldl=260) == ARG   # asked before the shape


# ---- operand sizes (include/vitamd.h, "Sizes"): every refusal below is answered before a launch
G31 = 2**31
EPI_BIAS, EPI_PATCH = 0, 4
NT_TILE_CODES = (0, 128, 256, 320, 512, 1024, 2048, 4096)


def _nt(L, M, N, K, ldo, epi, tile, n_patches=0, seq=0, extra=0):
    return L.vitamd_gemm_nt_bf16(P, P, P, P, None, P, None, M, N, K, ldo, epi, n_patches, seq, extra, tile, None)


def test_nt_refuses_a_weight_of_2g_bytes():
    from vitamd import lib
    L = lib.load()
    K = 1024
    n_at, n_under = G31 // (K * 2), G31 // (K * 2) - 8                # N x K x 2 = 2^31 exactly / 16 KiB less (N % 8 == 0: every form applies)
    assert n_at * K * 2 == G31 and n_at % 4 == 0
    for tile in NT_TILE_CODES:
        assert L.vitamd_gemm_nt_plan(1, n_at, K, n_at, EPI_BIAS, tile) == -SHAPE, tile
        assert _nt(L, 1, n_at, K, n_at, EPI_BIAS, tile) == SHAPE, tile
        assert L.vitamd_gemm_nt_plan(300, n_at + 4, K, n_at + 4, EPI_BIAS, tile) == -SHAPE, tile
    # just under: accepted (the plan answers a form; 320-row tiles, the seam and the loader form apply to this shape too)
    for tile in NT_TILE_CODES:
        assert L.vitamd_gemm_nt_plan(300, n_under, K, n_under, EPI_BIAS, tile) > 0, tile
    # the argument checks still answer first
    assert L.vitamd_gemm_nt_bf16(None, P, P, P, None, P, None, 1, n_at, K, n_at, EPI_BIAS, 0, 0, 0, 0, None) == ARG
    assert _nt(L, 1, n_at, K + 16, n_at, EPI_BIAS, 0) == SHAPE


def test_nt_patch_epilogue_is_refused_past_the_limit_and_other_epilogues_are_split():
    from vitamd import lib
    L = lib.load()
    K, N = 1024, 64
    m_at = G31 // (K * 2)                                              # M x K x 2 = 2^31
    for tile in (0, 128, 256, 512, 1024):
        assert L.vitamd_gemm_nt_plan(m_at, N, K, N, EPI_PATCH, tile) == -SHAPE, tile
        assert _nt(L, m_at, N, K, N, EPI_PATCH, tile, n_patches=196, seq=197, extra=1) == SHAPE, tile
        assert L.vitamd_gemm_nt_plan(m_at - 1, N, K, N, EPI_PATCH, tile) > 0, tile
        assert L.vitamd_gemm_nt_plan(m_at, N, K, N, EPI_BIAS, tile) > 0, tile              # the same shape in row panels
    # ... and through the fp32 output: M x ldo x 4 = 2^31 with a small A
    m_out = G31 // (4096 * 4)
    assert L.vitamd_gemm_nt_plan(m_out, 4096, 64, 4096, EPI_PATCH, 0) == -SHAPE
    assert _nt(L, m_out, 4096, 64, 4096, EPI_PATCH, 0, n_patches=196, seq=197, extra=1) == SHAPE
    assert L.vitamd_gemm_nt_plan(m_out - 1, 4096, 64, 4096, EPI_PATCH, 0) > 0
    # a row so wide that a 1280-row panel cannot stay below 2^31 bytes
    wide = G31 // (1280 * 2) // 8 * 8 + 8
    assert L.vitamd_gemm_nt_plan(1281, 8, 64, wide, EPI_BIAS, 0) == -SHAPE and _nt(L, 1281, 8, 64, wide, EPI_BIAS, 0) == SHAPE
    assert L.vitamd_gemm_nt_plan(1280, 8, 64, wide - 8, EPI_BIAS, 0) > 0


def test_nt_plan_of_a_split_call_is_the_plan_of_its_panels():
    """explicit tile codes (their plans do not depend on the CU count): a call past 2^31 bytes of out answers what a 1280-row multiple below it does"""
    from vitamd import lib
    L = lib.load()
    N, K = 8200, 128
    rows = (G31 - 1) // (N * 2) // 1280 * 1280
    assert rows * N * 2 < G31 <= (rows + 1280) * N * 2
    for tile, form in ((4096, 4 | 256 << 8), (2048, 5 | 256 << 8), (256, 2 | 256 << 8), (320, 2 | 320 << 8), (128, 1 | 128 << 8)):
        for M in (rows, rows + 1, 2 * rows + 77, 2**18 + 77):
            assert L.vitamd_gemm_nt_plan(M, N, K, N, EPI_BIAS, tile) == form, (tile, M)
    # the seam / loader forms' own rules still refuse through a split: N % 8 != 0
    assert L.vitamd_gemm_nt_plan(2**18, 8204, K, 8204, EPI_BIAS, 4096) == -SHAPE and _nt(L, 2**18, 8204, K, 8204, EPI_BIAS, 4096) == SHAPE


def test_tn_size_guard_at_its_exact_edge():
    """(R + 64) x ld x 2 < 2^31 for both operands, all three entry points.  The accepted side is shown without a launch: a null operand is asked for
    only after the shape has passed."""
    from vitamd import lib
    L = lib.load()
    for ld in (4096, 2304, 8):
        r_max = (G31 - 1) // (ld * 2) - 64
        assert (r_max + 64) * ld * 2 < G31 <= (r_max + 65) * ld * 2
        for big in ("L", "R"):
            pq = min(64, ld)                                            # the other operand: the narrowest stride that holds it
            ldl, ldr = (ld, pq) if big == "L" else (pq, ld)
            for R, want in ((r_max + 1, SHAPE), (r_max, ARG)):
                for form in (0, 1):
                    assert L.vitamd_gemm_tn_bf16_ws(None, None, None, R, pq, pq, ldl, ldr, 64, 1, P, 1 << 30, 1, form, None) == want, (ld, big, R)
                    assert L.vitamd_gemm_tn_bf16_ws_colsum(None, None, None, P, R, pq, pq, ldl, ldr, 64, 1, P, 1 << 30, 1, form, None) == want, (ld, big, R)
                assert L.vitamd_gemm_tn_bf16(None, None, None, R, pq, pq, ldl, ldr, 64, 1, None) == want, (ld, big, R)
            assert L.vitamd_gemm_tn_bf16(P, P, P, r_max + 1, pq, pq, ldl, ldr, 64, 1, None) == SHAPE
