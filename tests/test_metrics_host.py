"""Host-side checks of the evaluation path (vitamd/metrics.py, csrc/loss.hip vitamd_classify_metrics): the float64 reference of
tests/_metrics_ref.py against torch's argmax and topk, the comparison of the GPU tests against planted mistakes, the C ABI's symbol and
refusals, the Python surface's refusals, the allocation rule of tests/_poison.py and the scripts' flags.  No GPU is needed."""
import ast
import ctypes
import os

import pytest
import torch

import _abi
import _metrics_ref as MR
import _poison as P

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ERR_SHAPE, ERR_ARG = 1, 2


def _ties_case(M, V, seed, special=False):
    """logits from five small integers (ties everywhere), targets that include 0 and V - 1, rows 2 and M - 1 ignored; special: row 3
    has a NaN at its target, row 4 a NaN elsewhere, row 5 a target outside [0, V)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (M, V), generator=g).to(F32)
    t = torch.randint(0, V, (M,), generator=g)
    t[0], t[1], t[2], t[M - 1] = 0, V - 1, -100, -100
    if special:
        x[3, t[3]] = float("nan")
        x[4, (int(t[4]) + 1) % V] = float("nan")
        t[5] = V + 3
    return x, t


@pytest.mark.parametrize("V", [2, 7, 40])
def test_rank_zero_is_argmax_and_rank_below_k_is_topk(V):
    x, t = _ties_case(64, V, seed=V)
    t = torch.where(t == -100, torch.zeros_like(t), t)
    ref = MR.metrics_ref(x, t, topk=min(3, V))
    assert torch.equal(ref["rank"] == 0, x.argmax(-1) == t)                  # torch returns the first maximal index
    assert ref["counts"][0] == 64 and ref["counts"][1] == int((x.argmax(-1) == t).sum())
    y = torch.randn(64, V, generator=torch.Generator().manual_seed(V), dtype=F64)         # no ties at all: top-k is unambiguous
    for k in {1, min(2, V), min(5, V), V}:
        r = MR.metrics_ref(y, t, topk=k)
        member = (torch.topk(y, k, dim=-1).indices == t[:, None]).any(-1)
        assert torch.equal(r["rank"] < k, member), k
        assert r["counts"][2] == int(member.sum())
    sorted_rank = (torch.argsort(torch.argsort(y, dim=-1, descending=True), dim=-1)).gather(1, t[:, None])[:, 0]
    assert torch.equal(MR.metrics_ref(y, t, topk=1)["rank"], sorted_rank)


def test_reference_loss_is_torch_float64_and_special_rows_follow_the_definition():
    x, t = _ties_case(32, 9, seed=5, special=True)
    ref = MR.metrics_ref(x, t, topk=2)
    assert int(ref["rank"][2]) == -1 == int(ref["rank"][31]) and float(ref["loss_row"][2]) == 0.0
    assert int(ref["rank"][3]) == 8                      # a NaN target ranks below every column
    assert int(ref["rank"][4]) >= 1                      # a NaN elsewhere ranks above the target
    assert int(ref["rank"][5]) == 9                      # out of range: wrong for every k, V included
    assert ref["counts"][0] == 30 and ref["loss_sum"] != ref["loss_sum"]
    assert MR.metrics_ref(x, t, topk=9)["counts"][2] == 29               # k = V: every in-range target, never the out-of-range one
    x, t = _ties_case(32, 9, seed=6)
    ref = MR.metrics_ref(x, t, topk=2)
    rows = torch.nn.functional.cross_entropy(x.to(F64), t, ignore_index=-100, reduction="none")
    assert torch.allclose(ref["loss_row"], rows, rtol=1e-13, atol=1e-13)
    assert abs(ref["loss_sum"] - float(rows.sum())) < 1e-11


def test_comparison_catches_every_planted_mistake():
    """Each mistake is applied to the reference and handed, as `got`, to the comparison the GPU tests use: it must be reported.  The
    unchanged reference must pass."""
    finite = _ties_case(48, 6, seed=11)
    special = _ties_case(48, 6, seed=12, special=True)
    k = 2
    for bug in MR.BUGS:
        x, t = special if bug in ("oor_skipped", "nan_target_correct") else finite
        ref = MR.metrics_ref(x, t, k)
        allow = MR.sum_allowance(ref, MR.row_bound(*finite))
        assert MR.check_metrics(ref, ref, allow, "reference") == []
        bad = MR.metrics_ref(x, t, k, bug=bug)
        assert MR.check_metrics(bad, ref, allow, bug), bug
    calls = [MR.metrics_ref(*_ties_case(M, 6, seed=20 + M), k) for M in (9, 17, 30)]
    total = MR.accumulate(calls)
    allow = sum(MR.sum_allowance(c, MR.row_bound(*_ties_case(M, 6, seed=20 + M))) for c, M in zip(calls, (9, 17, 30)))
    assert total["counts"][0] == sum(c["counts"][0] for c in calls)
    assert MR.check_metrics(total, total, allow, "accumulated") == []
    for bug in MR.ACC_BUGS:
        assert MR.check_metrics(MR.accumulate(calls, bug=bug), total, allow, bug), bug


# ------------------------------------------------------------------------------------------------ the library
def test_symbol_is_declared_bound_and_the_abi_stays_9():
    from vitamd import lib
    L = lib.load()
    name = "vitamd_classify_metrics"
    fn = getattr(L, name)
    assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    assert _abi.declared()[1][name] == "int" and len(_abi.declaration(name).split(",")) == len(lib.SIGNATURES[name]) == 13


def test_entry_point_refuses_before_any_launch():
    """null pointers everywhere: a shape error is reported first, valid numbers then give the argument error; with real host
    addresses in every pointer a bad topk is still refused; nothing is launched (no device is needed)"""
    from vitamd import lib
    L = lib.load()
    null = lambda M, V, ld, topk: L.vitamd_classify_metrics(None, 0, None, None, None, None, None, M, V, ld, topk, -100, None)
    for M, V, ld in ((4, 1, 1), (4, 65537, 65537), (4, 10, 9), (0, 10, 10), (1 << 31, 10, 10), (4, 10, 1 << 31)):
        assert null(M, V, ld, 1) == ERR_SHAPE, (M, V, ld)
    assert null(4, 10, 10, 1) == ERR_ARG and null(1, 2, 2, 2) == ERR_ARG and null(4, 65536, 65536, 5) == ERR_ARG
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    full = lambda V, topk, bf16=0: L.vitamd_classify_metrics(p, bf16, p, p, p, p, p, 4, V, V, topk, -100, None)
    assert full(10, 0) == ERR_ARG and full(10, 11) == ERR_ARG and full(10, -1) == ERR_ARG and full(2, 3, 1) == ERR_ARG
    for missing in range(6):                                                  # each pointer alone
        ptrs = [p] * 6
        ptrs[missing] = None
        assert L.vitamd_classify_metrics(ptrs[0], 0, *ptrs[1:], 4, 10, 10, 5, -100, None) == ERR_ARG, missing


def test_python_surface_refuses_before_any_launch():
    from vitamd import metrics, mix, ops
    from vitamd.lib import VitamdError
    refuse = (ValueError, VitamdError)
    x, t = torch.randn(4, 10), torch.randint(0, 10, (4,))
    acc = (torch.zeros(1, dtype=F64), torch.zeros(3, dtype=torch.int64))
    for topk in (0, 11, -1, 2.0, True):
        with pytest.raises(ValueError):
            ops.classify_metrics(x, t, *acc, topk=topk)                       # also on CPU tensors: nothing has looked at a device yet
    with pytest.raises(ValueError):
        ops.classify_metrics(torch.randn(4, 1), t, *acc, topk=1)
    with pytest.raises(VitamdError):
        ops.classify_metrics(x, t, *acc)                                      # a CPU tensor
    with pytest.raises(refuse):
        ops.classify_metrics(x, t[:3], *acc)
    with pytest.raises(ValueError):
        metrics.ClassifyMetrics(topk=0)
    m = metrics.ClassifyMetrics(topk=5, device="cpu")                        # the accumulators exist; every update is refused
    assert m.loss_sum.dtype == F64 and tuple(m.loss_sum.shape) == (1,) and m.counts.dtype == torch.int64 and tuple(m.counts.shape) == (3,)
    with pytest.raises(VitamdError):
        m.update(x, t)
    with pytest.raises(VitamdError):
        m.update(x.reshape(2, 2, 10), t.reshape(2, 2))
    with pytest.raises(refuse):
        m.update(x, t[:3])
    with pytest.raises(refuse):
        m.update(x, t.int())
    with pytest.raises(ValueError):
        m.update(torch.randn(4, 3), torch.randint(0, 3, (4,)))               # topk = 5 of 3 classes
    with pytest.raises(TypeError, match="hard labels"):
        m.update(x, mix.MixedLabels(t, t, torch.ones(4)))
    with pytest.raises(RuntimeError):
        m.rows()
    assert float(m.loss_sum) == 0.0 and m.counts.tolist() == [0, 0, 0]
    r = m.result()
    assert r["count"] == 0 and r["loss"] != r["loss"] and set(r) == {"loss", "top1", "topk", "count", "perplexity"}


def test_no_uninitialised_allocation_was_added():
    """tests/test_gpu_poison.py demands that its workloads reach every torch.empty-family call of the package and names the ones they
    cannot by line: the evaluation path adds none, and the lines that test names still hold such calls"""
    spans = P.site_spans()
    assert not [k for k in spans if k[0] == "metrics.py"]
    import test_gpu_poison as TP
    for name, line in TP.NOT_REACHED:
        assert (name, line) in spans, (name, line)
    src = open(os.path.join(P.PKG_DIR, "ops.py")).read()
    fn = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "classify_metrics")
    assert not [k for k in spans if k[0] == "ops.py" and fn.lineno <= k[1] <= fn.end_lineno]
    lm_src = open(os.path.join(P.PKG_DIR, "lm.py")).read()
    fn = next(n for n in ast.walk(ast.parse(lm_src)) if isinstance(n, ast.FunctionDef) and n.name == "head_logits")
    assert not [k for k in spans if k[0] == "lm.py" and fn.lineno <= k[1] <= fn.end_lineno]


def test_scripts_accept_the_flags_and_default_to_off():
    import train_videogpt as VG
    import train_vit as TV
    for mod in (TV, VG):
        a = mod.parse_args([])
        assert a.eval_every == 0 and a.eval_batches >= 1
        b = mod.parse_args(["--eval_every", "10", "--eval_batches", "3"])
        assert (b.eval_every, b.eval_batches) == (10, 3)
        assert {k: v for k, v in vars(a).items() if not k.startswith("eval_")} == {k: v for k, v in vars(b).items() if not k.startswith("eval_")}
        assert callable(mod.evaluate)
        main_src = ast.get_source_segment(open(mod.__file__).read(), next(
            n for n in ast.walk(ast.parse(open(mod.__file__).read())) if isinstance(n, ast.FunctionDef) and n.name == "main"))
        assert "if val is not None and" in main_src and "args.eval_every > 0" in main_src       # the default route builds no validation set and prints nothing new
    assert callable(VG.VideoGPT.eval_logits)
