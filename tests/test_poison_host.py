"""The poison harness (tests/_poison.py) has teeth: planted mistakes are reported, correct code passes, the context manager restores
what it patched, and empty_sites() finds the call sites.  No GPU."""
import glob
import os
import re
import types

import pytest
import torch

import _poison as P

F32 = torch.float32


def _both(fn):
    """fn() clean and poisoned -> (clean dict, poisoned dict)"""
    clean = fn()
    with P.poisoned():
        dirty = fn()
    return clean, dirty


# ------------------------------------------------------------------------------------------ planted mistakes are reported
def test_sum_over_a_half_written_empty_is_reported():
    def fn():
        buf = torch.empty(8, dtype=F32)
        if not P._active:
            buf.zero_()                                            # the clean run: what a zero-filled fresh allocation holds
        buf[:4] = torch.arange(4.0)
        return {"sum": buf.sum().reshape(1)}
    clean, dirty = _both(fn)
    assert float(clean["sum"]) == 6.0
    fails = P.compare(clean, dirty, exact={"sum"})
    assert len(fails) == 1 and fails[0].startswith("sum:") and "(0,)" in fails[0]
    assert P.compare(clean, dirty, exact=set()) and "non-finite" in P.compare(clean, dirty, exact=set())[0]


def test_empty_like_followed_by_accumulate_is_reported():
    g = torch.arange(6.0).reshape(2, 3)

    def fn():
        acc = torch.empty_like(g)
        if not P._active:
            acc.zero_()                                            # the lucky allocation
        acc += g
        return {"acc": acc}
    clean, dirty = _both(fn)
    assert torch.equal(clean["acc"], g)
    fails = P.compare(clean, dirty, exact={"acc"})
    assert len(fails) == 1 and "acc" in fails[0] and "(0, 0)" in fails[0] and "6 of 6" in fails[0]


def test_new_empty_index_under_a_range_guard_is_reported():
    """A stale integer is -1: outside every table, so guarded code skips the row (the result changes) instead of reading an address."""
    table = torch.arange(12.0).reshape(4, 3)
    base = torch.tensor([2, 0, 3])

    def fn():
        idx = base.new_empty(3)
        idx[:2] = base[:2]                                         # the last entry is never written
        if not P._active:
            idx[2] = 0
        ok = (idx >= 0) & (idx < table.shape[0])                   # the kernels' range guard
        rows = torch.index_select(table, 0, idx.clamp(0, table.shape[0] - 1)) * ok[:, None]
        return {"rows": rows, "idx": idx}
    clean, dirty = _both(fn)
    assert int(dirty["idx"][2]) == -1
    fails = P.compare(clean, dirty, exact={"rows", "idx"})
    assert len(fails) == 2 and any(f.startswith("rows:") and "(2, 1)" in f for f in fails) and any(f.startswith("idx:") and "(2,)" in f for f in fails)


def test_empty_strided_read_through_maximum_is_reported():
    """torch.maximum propagates NaN, so the stale read shows as a NaN.  Code in the style of C's fmax (or a kernel's v_max_f32) returns the
    OTHER operand when one is NaN: there the stale value silently vanishes whenever the live operand happens to win, the result stays
    finite, and only a bit comparison of a case where the stale value matters can see the read - the reason compare() has `exact` keys
    beside the finiteness rule."""
    x = torch.tensor([[1.0, -2.0], [3.0, -4.0]])

    def fn(maximum):
        stale = torch.empty_strided((2, 2), (1, 2), dtype=F32)     # column-major
        if not P._active:
            stale.zero_()
        return {"relu": maximum(x, stale)}
    clean = fn(torch.maximum)
    with P.poisoned():
        dirty, dropped = fn(torch.maximum), fn(torch.fmax)
    assert bool(torch.isnan(dirty["relu"]).all())
    assert P.compare(clean, dirty, exact=set()) and P.compare(clean, dirty, exact={"relu"})
    assert bool(torch.isfinite(dropped["relu"]).all())             # fmax dropped the NaN ...
    assert P.compare(clean, dropped, exact=set()) == []            # ... the finiteness rule is blind to it ...
    assert P.compare(clean, dropped, exact={"relu"})               # ... the bit comparison is not (max(x, 0) != x where x < 0)


def test_compare_sees_minus_zero_and_nan_payloads():
    a = {"z": torch.tensor([0.0, float("nan")])}
    b = {"z": torch.tensor([-0.0, float("nan")])}
    assert torch.equal(a["z"][:1], b["z"][:1])                     # == cannot see it
    fails = P.compare(a, b, exact={"z"})
    assert len(fails) == 1 and "1 of 2" in fails[0] and "(0,)" in fails[0]
    c = {"z": a["z"].view(torch.int32).clone().view(F32)}
    assert P.compare(a, c, exact={"z"}) == []                      # the same NaN bits are equal
    c["z"].view(torch.int32)[1] |= 1                               # another payload
    assert len(P.compare(a, c, exact={"z"})) == 1
    assert P.compare(a, {"y": a["z"]}, exact=set())                # key sets differ
    assert P.compare(a, a, exact={"nope"})                         # an exact key that does not exist


# ------------------------------------------------------------------------------------------ correct code passes
def test_a_fully_overwritten_buffer_passes():
    x = torch.arange(10.0)

    def fn():
        out = torch.empty_like(x)
        torch.mul(x, 2.0, out=out)
        idx = torch.empty(3, dtype=torch.int64)
        idx.copy_(torch.tensor([4, 1, 0]))
        return {"out": out, "picked": out[idx]}
    clean, dirty = _both(fn)
    assert P.compare(clean, dirty, exact={"out", "picked"}) == []


def test_a_linear_constructed_inside_the_context_passes():
    def fn():
        torch.manual_seed(5)
        lin = torch.nn.Linear(7, 3)                                # torch.empty, then an initialiser that overwrites all of it
        return {"w": lin.weight.detach(), "b": lin.bias.detach(), "y": lin(torch.ones(2, 7)).detach()}
    clean, dirty = _both(fn)
    assert P.compare(clean, dirty, exact={"w", "b", "y"}) == []
    assert bool(torch.isfinite(dirty["w"]).all())


# ------------------------------------------------------------------------------------------ the context manager
def _all_ff(t):
    return bool((t.contiguous().view(torch.uint8) == 255).all())


def test_the_poison_is_all_ff_bytes():
    with P.poisoned():
        for dtype in (torch.float64, F32, torch.bfloat16, torch.float16, torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            t = torch.empty((3, 5), dtype=dtype)
            assert _all_ff(t), dtype
            if dtype.is_floating_point:
                assert bool(torch.isnan(t).all()), dtype
            elif dtype != torch.uint8:
                assert bool((t == -1).all()), dtype
            else:
                assert bool((t == 255).all())
        assert bool(torch.empty(4, dtype=torch.bool).all())
        assert bool(torch.isnan(torch.view_as_real(torch.empty(2, dtype=torch.complex64))).all())
        assert bool(torch.isnan(torch.empty_strided((2, 3), (1, 2))).all())


def test_the_patched_names_take_every_calling_form():
    like = torch.zeros((2, 3), dtype=torch.float64)
    with P.poisoned():
        for t in (torch.empty(2, 3), torch.empty((2, 3)), torch.empty(size=(2, 3)), torch.empty([2, 3], dtype=F32),
                  torch.empty(2, 3, pin_memory=False), torch.empty((2, 3), memory_format=torch.contiguous_format),
                  torch.empty_like(like, dtype=F32), torch.empty_like(like, memory_format=torch.preserve_format).float(),
                  torch.empty_strided((2, 3), (3, 1), dtype=F32), like.new_empty((2, 3), dtype=F32), like.new_empty(2, 3).float(),
                  like.new_empty_strided((2, 3), (3, 1)).float()):
            assert tuple(t.shape) == (2, 3) and bool(torch.isnan(t).all())
        cl = torch.empty((1, 2, 3, 3), memory_format=torch.channels_last)
        assert cl.is_contiguous(memory_format=torch.channels_last) and bool(torch.isnan(cl).all())
        meta = torch.empty((2, 3), device="meta")
        assert meta.is_meta and tuple(meta.shape) == (2, 3)
        assert torch.empty_like(meta).is_meta and meta.new_empty((4,)).is_meta
        assert torch.empty(0).numel() == 0 and torch.empty((0, 3)).shape == (0, 3)
        out = torch.zeros(2, 3)
        assert torch.empty((2, 3), out=out) is out


def _attrs():
    return [getattr(owner, name) for owner, name in P.PATCHED]


def test_the_originals_are_back_after_exit_and_after_an_exception():
    before = _attrs()
    with P.poisoned():
        assert all(a is not b for a, b in zip(_attrs(), before))
    assert all(a is b for a, b in zip(_attrs(), before))
    with pytest.raises(KeyError):
        with P.poisoned():
            raise KeyError("boom")
    assert all(a is b for a, b in zip(_attrs(), before))
    assert "new_empty" not in vars(torch.Tensor) and not P._active
    assert not bool(torch.isnan(torch.zeros(3).new_empty(0).sum()))
    with P.poisoned():                                             # usable again
        assert bool(torch.isnan(torch.empty(1)).all())


def test_nesting_raises_and_leaves_the_outer_context_intact():
    before = _attrs()
    with P.poisoned():
        with pytest.raises(RuntimeError):
            with P.poisoned():
                pass
        assert bool(torch.isnan(torch.empty(2)).all())             # the outer one is still active
    assert all(a is b for a, b in zip(_attrs(), before))


def test_the_log_holds_the_package_call_site_and_not_the_tests_own(tmp_path):
    pkg = tmp_path / "vitamd"
    pkg.mkdir()
    src = ("import torch\n"
           "def make(x):\n"
           "    a = torch.empty((2, 3), dtype=torch.float32)\n"
           "    b = torch.empty_like(x)\n"
           "    c = x.new_empty(\n"
           "        (5,))\n"
           "    m = torch.empty((7,), device='meta')\n"
           "    z = torch.empty((0,))\n"
           "    return a, b, c\n")
    path = pkg / "fake_ops.py"
    path.write_text(src)
    mod = types.ModuleType("fake_ops")
    exec(compile(src, str(path), "exec"), mod.__dict__)
    log = []
    with P.poisoned(log):
        torch.empty(4)                                             # the test's own: not logged
        mod.make(torch.zeros(4, dtype=torch.int32))
    assert [e[:2] for e in log] == [("fake_ops.py", 3), ("fake_ops.py", 4), ("fake_ops.py", 5)]
    assert log[0][2:] == ((2, 3), F32) and log[1][2:] == ((4,), torch.int32) and log[2][2:] == ((5,), torch.int32)
    spans = P.site_spans(src)
    assert {("fake_ops.py", n) for _, n in P.sites_hit([("<string>",) + e[1:] for e in log], spans)} == {("fake_ops.py", 3), ("fake_ops.py", 4), ("fake_ops.py", 5)}
    assert ("<string>", 7) in spans and ("<string>", 7) not in P.sites_hit([("<string>",) + e[1:] for e in log], spans)


def test_dirty_scratch_poisons_what_it_is_given_and_nothing_else():
    table = types.SimpleNamespace(partials=torch.zeros(5), norm_coef=torch.zeros(2), dev_rows=torch.zeros(8, dtype=torch.uint8))
    optim = types.SimpleNamespace(_table=table)
    prep = {"scratch": {96: torch.zeros(2, 96), 192: torch.zeros(2, 192)}, "mean": torch.zeros(3)}
    n = P.dirty_scratch(optim, prep, None)
    assert n >= 4
    assert bool(torch.isnan(table.partials).all()) and bool(torch.isnan(table.norm_coef).all())
    assert all(bool(torch.isnan(t).all()) for t in prep["scratch"].values())
    assert not bool(table.dev_rows.any()) and not bool(prep["mean"].any())      # values: left alone


# ------------------------------------------------------------------------------------------ empty_sites()
def test_empty_sites_finds_the_calls_of_a_source_string():
    src = ("import torch\n"
           "x = torch.empty(3)\n"
           "y = torch.empty_like(x); z = torch.empty_strided((1,), (1,))\n"
           "def f(t):\n"
           "    return t.new_empty(\n"
           "        (2,)), t.new_empty_strided((1,), (1,))\n"
           "w = torch.zeros(3)  # torch.empty( in a comment is no call\n"
           "s = 'torch.empty(1)'\n")
    assert P.empty_sites(src) == {("<string>", 2), ("<string>", 3), ("<string>", 5), ("<string>", 6)}
    assert P.site_spans(src)[("<string>", 5)] == 6


def test_empty_sites_covers_the_package_at_least_as_well_as_a_text_count():
    sites = P.empty_sites()
    pattern = re.compile(r"torch\.empty(_like|_strided)?\(|\.new_empty(_strided)?\(")
    per_file = {}
    for path in glob.glob(os.path.join(P.PKG_DIR, "*.py")):
        with open(path) as f:
            lines = [i + 1 for i, line in enumerate(f) if pattern.search(line.split("#")[0])]
        per_file[os.path.basename(path)] = lines
    text = {(name, n) for name, lines in per_file.items() for n in lines}
    assert len(text) > 100 and "ops.py" in per_file                # the package was found
    assert text <= sites, sorted(text - sites)
    assert len(sites) >= sum(len(v) for v in per_file.values())
