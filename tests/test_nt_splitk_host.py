"""Host side of the split-K form of the 128x128 NT GEMM (no GPU): the three new C-ABI names, the split rule as vitamd_gemm_nt_ws_plan and
vitamd_gemm_nt_ws_bytes report it (256 CUs are assumed where no device answers), what keeps a launch unsplit, and that vitamd_gemm_nt_plan -
the description of vitamd_gemm_nt_bf16, which has no workspace - answers what it answered."""
import ctypes

import pytest

import _abi

SHAPE, ARG = 1, 2
FORM_SMALL, FORM_SPLITK, TILE_BYTES = 1, 6, 128 * 128 * 4
CUS = 256


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


def test_new_symbols_are_declared_and_bound_and_the_abi_version_stays(L):
    from vitamd import lib, ops
    header = _abi.header()
    declared, _ = _abi.declared()
    for name, n, restype in (("vitamd_gemm_nt_bf16_ws", 20, ctypes.c_int), ("vitamd_gemm_nt_ws_bytes", 7, ctypes.c_long),
                             ("vitamd_gemm_nt_ws_plan", 7, ctypes.c_int)):
        assert declared[name] == n == len(lib.SIGNATURES[name]), name
        fn = getattr(L, name)
        assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is restype
    assert declared["vitamd_gemm_nt_bf16_ws"] == declared["vitamd_gemm_nt_bf16"] + 3
    assert f"#define VITAMD_NT_FORM_SPLITK {FORM_SPLITK}" in header and ops.NT_FORM_SPLITK == FORM_SPLITK and ops.NT_SPLITS == 0
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION          # additive: no existing signature changed


# the six small NT launches of a ViT-B step at batch 256 (kept-row layer, classifier head and its input gradient): M = 256
STEP = [(768, 3072, 2), (3072, 768, 6), (3072, 768, 7), (768, 3072, 0), (1024, 768, 0), (768, 1024, 0)]


@pytest.mark.parametrize("N,K,epi", STEP)
def test_the_rule_on_the_launches_of_the_step(L, N, K, epi):
    M = 256
    tiles = 2 * (N // 128)
    splits = min(CUS // tiles, K // 128)
    assert splits >= 2 and tiles * splits <= CUS and K // 64 // splits >= 2
    assert L.vitamd_gemm_nt_ws_plan(M, N, K, N, epi, 0, 0) == FORM_SPLITK | 128 << 8 | splits << 16
    assert L.vitamd_gemm_nt_ws_bytes(M, N, K, N, epi, 0, 0) == splits * tiles * TILE_BYTES
    # the split count is a function of N and K: fewer rows, the same K ranges (a sample's result does not depend on the batch it is in)
    for rows in (1, 32, 128, 129):
        assert L.vitamd_gemm_nt_ws_plan(rows, N, K, N, epi, 0, 0) == FORM_SPLITK | 128 << 8 | splits << 16
        assert L.vitamd_gemm_nt_ws_bytes(rows, N, K, N, epi, 0, 0) == splits * (tiles // 2 if rows <= 128 else tiles) * TILE_BYTES
    assert L.vitamd_gemm_nt_ws_bytes(257, N, K, N, epi, 0, 0) == 0 and L.vitamd_gemm_nt_ws_plan(257, N, K, N, epi, 0, 2) >> 16 == 2
    assert L.vitamd_gemm_nt_plan(M, N, K, N, epi, 0) == FORM_SMALL | 128 << 8          # the entry point without a workspace: as before


@pytest.mark.parametrize("tile", [0, 512, 1024])
def test_forced_and_capped_split_counts(L, tile):
    for K, want, got in ((128, 2, 1), (192, 2, 1), (256, 2, 2), (768, 2, 2), (768, 7, 6), (768, 1, 1), (3072, 100, 24)):
        plan = L.vitamd_gemm_nt_ws_plan(256, 768, K, 768, 0, tile, want)
        assert plan == (FORM_SPLITK | 128 << 8 | got << 16 if got > 1 else FORM_SMALL | 128 << 8), (K, want)
        assert L.vitamd_gemm_nt_ws_bytes(256, 768, K, 768, 0, tile, want) == (got * 12 * TILE_BYTES if got > 1 else 0)


def test_what_stays_unsplit(L):
    plain = lambda *a: L.vitamd_gemm_nt_plan(*a)
    # an explicit tile code, the patch epilogue, more than two tile rows, two tile rows of 128 tiles each, the large forms
    for M, N, K, epi, tile in ((256, 768, 768, 0, 128), (256, 768, 768, 4, 0), (384, 768, 768, 0, 0), (128, 128 * 128, 768, 0, 0),
                               (50432, 768, 768, 0, 0), (50432, 3072, 768, 1, 0)):
        assert L.vitamd_gemm_nt_ws_plan(M, N, K, N, epi, tile, 0) == plain(M, N, K, N, epi, tile), (M, N, K, epi, tile)
        assert L.vitamd_gemm_nt_ws_bytes(M, N, K, N, epi, tile, 0) == 0
    # refusals: the shape first, then the arguments
    assert L.vitamd_gemm_nt_ws_bytes(0, 768, 768, 768, 0, 0, 0) == -SHAPE and L.vitamd_gemm_nt_ws_plan(256, 768, 100, 768, 0, 0, 0) == -SHAPE
    assert L.vitamd_gemm_nt_ws_bytes(256, 768, 768, 768, 0, 7, 0) == -ARG and L.vitamd_gemm_nt_ws_plan(256, 768, 768, 768, 0, 0, -1) == -ARG
    assert L.vitamd_gemm_nt_bf16_ws(None, None, None, None, None, None, None, 0, 768, 768, 768, 0, 0, 0, 0, 0, 0, None, 0, None) == SHAPE
    assert L.vitamd_gemm_nt_bf16_ws(None, None, None, None, None, None, None, 256, 768, 768, 768, 0, 0, 0, 0, 0, 0, None, 0, None) == ARG
