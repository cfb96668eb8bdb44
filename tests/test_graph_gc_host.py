"""vitamd.graph.quiet_collector, without a GPU: what every capture of the package is wrapped in.  A dead reference cycle is collected
BEFORE the body runs (so a torch.cuda.CUDAGraph held by one is destroyed outside the capture), the automatic collector is off inside the
body and back afterwards, also when the body raises, and a collector that was off stays off."""
import gc
import weakref

import pytest


class _Node:
    pass


def _dead_cycle():
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    return weakref.ref(a)


def test_collects_before_the_body_and_holds_the_collector_inside():
    from vitamd import graph
    assert gc.isenabled()
    gc.disable()                                  # so that only quiet_collector's own collect can have freed the cycle
    try:
        ref = _dead_cycle()
        assert ref() is not None
        gc.enable()
        with graph.quiet_collector():
            assert ref() is None and not gc.isenabled()
            inner = _dead_cycle()
            junk = [[] for _ in range(5000)]      # far past the generation-0 threshold: an enabled collector would have run
            del junk
            assert inner() is not None
        assert gc.isenabled()
    finally:
        gc.enable()


def test_restores_the_collector_when_the_body_raises_and_leaves_a_disabled_one_alone():
    from vitamd import graph
    with pytest.raises(RuntimeError):
        with graph.quiet_collector():
            raise RuntimeError("capture failed")
    assert gc.isenabled()
    gc.disable()
    try:
        with graph.quiet_collector():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()


def test_every_capture_of_the_package_is_wrapped():
    import inspect
    from vitamd import graph
    src = inspect.getsource(graph)
    assert src.count("torch.cuda.graph(") == src.count("with quiet_collector(), torch.cuda.graph(") == 3
