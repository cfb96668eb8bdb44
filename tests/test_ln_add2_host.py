"""Host side of the two-addend LayerNorm forward (no GPU): the two new C-ABI names, their refusals before any launch and the order of those
refusals, and what the poison test demands of vitamd/ (no new uninitialised allocation in the wrappers)."""
import ctypes
import os

import pytest

import _abi
import _poison as P

SHAPE, ARG = 1, 2            # VITAMD_ERR_SHAPE, VITAMD_ERR_ARG
_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


def test_new_symbols_are_declared_and_bound_and_the_abi_version_stays(L):
    from vitamd import lib
    declared, _ = _abi.declared()
    for name, n in (("vitamd_layernorm_fwd_add2", 11), ("vitamd_layernorm_fwd_keep_add2", 13)):
        assert declared[name] == n == len(lib.SIGNATURES[name]), name
        fn = getattr(L, name)
        assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION          # additive: no existing signature changed


@pytest.mark.parametrize("M,D", [(0, 256), (-1, 256), (4, 0), (4, -4), (4, 258)])
def test_add2_shape_is_refused_first(L, M, D):
    assert L.vitamd_layernorm_fwd_add2(PTR, PTR, PTR, PTR, PTR, PTR, PTR, M, D, 1e-5, None) == SHAPE
    assert L.vitamd_layernorm_fwd_add2(None, None, None, None, None, None, None, M, D, 1e-5, None) == SHAPE


@pytest.mark.parametrize("D", [256, 768, 200])
def test_add2_null_pointers(L, D):
    # x_in, addend1, y, mean, rstd are required; addend2 and x_out are optional (no launch without a GPU: only the refusals are asked for)
    args = (PTR, PTR, PTR, PTR, PTR, PTR, PTR, 4, D, 1e-5, None)
    for k in (0, 1, 4, 5, 6):
        assert L.vitamd_layernorm_fwd_add2(*[None if i == k else a for i, a in enumerate(args)]) == ARG


@pytest.mark.parametrize("B,seq,keep,D", [(0, 5, 2, 256), (3, 0, 1, 256), (3, 5, 0, 256), (3, 5, 6, 256), (3, 5, 2, 0), (3, 5, 2, 258),
                                          (2 ** 20, 2 ** 11, 1, 256)])
def test_keep_add2_shape_is_refused_first(L, B, seq, keep, D):
    assert L.vitamd_layernorm_fwd_keep_add2(PTR, PTR, PTR, PTR, PTR, PTR, PTR, B, seq, keep, D, 1e-5, None) == SHAPE
    assert L.vitamd_layernorm_fwd_keep_add2(None, None, None, None, None, None, None, B, seq, keep, D, 1e-5, None) == SHAPE


def test_keep_add2_null_pointers(L):
    # everything but x_out is required
    args = (PTR, PTR, PTR, PTR, PTR, PTR, PTR, 3, 5, 2, 200, 1e-5, None)
    for k in (0, 1, 2, 4, 5, 6):
        assert L.vitamd_layernorm_fwd_keep_add2(*[None if i == k else a for i, a in enumerate(args)]) == ARG


def test_the_wrappers_add_no_uninitialised_allocation():
    """The new forms ride in ops.layernorm_fwd / layernorm_fwd_keep and use their output allocations: the poisoned workloads of
    test_gpu_poison.py reach every torch.empty of those two functions already."""
    src = open(os.path.join(P.PKG_DIR, "ops.py")).read()
    for fn, nxt, n in (("def layernorm_fwd(", "def layernorm_fwd_keep(", 4), ("def layernorm_fwd_keep(", "XHAT_WIDTHS", 4)):
        body = src[src.index(fn):src.index(nxt)]
        assert body.count("torch.empty") == n, fn
    from vitamd import functions as F, ops
    assert F.STREAM_ONCE is True and ops.XHAT_WIDTHS == (256, 512, 768, 1024)
