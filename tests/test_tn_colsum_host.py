"""Host-side checks of the weight-gradient GEMM's column-sum entry (no GPU): the binding, the workspace size, the refusals that need no launch."""
import ctypes

import pytest


def _auto_splits(R, P, Q, requested):
    ntile = ((P + 255) // 256) * ((Q + 255) // 256)
    splits = requested if requested > 0 else (1 if ntile >= 256 else 256 // ntile)
    return min(splits, (R + 63) // 64)


def test_the_colsum_entry_is_bound_with_sixteen_arguments_and_the_abi_version_stays():
    from vitamd import lib
    L = lib.load()
    sig = lib.SIGNATURES["vitamd_gemm_tn_bf16_ws_colsum"]
    assert len(sig) == 16 == len(lib.SIGNATURES["vitamd_gemm_tn_bf16_ws"]) + 1           # vitamd_gemm_tn_bf16_ws + colsum
    assert sig[3] is ctypes.c_void_p and list(L.vitamd_gemm_tn_bf16_ws_colsum.argtypes) == sig
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION                                 # additive: the version does not move


@pytest.mark.parametrize("R,P,Q,splits", [(64, 256, 256, 1), (1000, 264, 768, 3), (1000, 768, 256, 0), (100, 768, 768, 0), (50432, 3072, 768, 7),
                                          (50432, 768, 3072, 5)])
def test_ws_bytes_counts_the_column_sum_partials_behind_the_tiles(R, P, Q, splits):
    """256 floats per (split, row tile) behind the split-K partial tiles"""
    from vitamd import lib
    tiles_p, tiles_q = (P + 255) // 256, (Q + 255) // 256
    s = _auto_splits(R, P, Q, splits)
    tiles = s * tiles_p * tiles_q * 256 * 256 * 4
    assert lib.load().vitamd_gemm_tn_ws_bytes(R, P, Q, splits) == tiles + s * tiles_p * 256 * 4


def test_colsum_without_a_workspace_is_refused_before_any_launch():
    from vitamd import lib
    L = lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert L.vitamd_gemm_tn_bf16_ws_colsum(p, p, p, p, 64, 256, 256, 256, 256, 256, 1, None, 0, 1, 0, None) == 2        # VITAMD_ERR_ARG
    assert L.vitamd_gemm_tn_bf16_ws_colsum(p, p, p, p, 64, 256, 256, 256, 256, 256, 1, None, 0, 1, 2, None) == 2        # unknown form


def test_ops_gemm_tn_takes_colsum_and_the_step_has_its_switch():
    import inspect
    from vitamd import functions as F, ops
    assert inspect.signature(ops.gemm_tn).parameters["colsum"].default is None
    assert F.BIAS_FROM_WGRAD is True and isinstance(F.BIAS_QKV_FROM_WGRAD, bool)
