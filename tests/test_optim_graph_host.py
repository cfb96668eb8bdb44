"""Host side of the device-resident optimiser table (no GPU): the two new C-ABI symbols, the schedule entry's layout, the Python model of
the advance kernel against optim.hyper_row and utils.lr_factor on every step the GPU test runs, the refusals that need no device, and
what capturable=True adds to (and keeps out of) the param groups."""
import ctypes
import re

import numpy as np
import pytest
import torch

import _abi
import _optim_graph_ref as R


def test_symbols_are_declared_bound_and_sized():
    from vitamd import lib, optim
    header = _abi.header()
    L = lib.load()
    for name, nargs, restype in (("vitamd_sched_row_bytes", 0, ctypes.c_long), ("vitamd_sched_advance", 4, ctypes.c_int)):
        assert name in _abi.declared()[0], name
        fn = getattr(L, name)
        assert len(lib.SIGNATURES[name]) == nargs and fn.argtypes == lib.SIGNATURES[name] and fn.restype is restype
    assert lib.ABI_VERSION == 9 and L.vitamd_abi_version() == 9                     # additive: no existing signature changed
    assert optim.SCHED_DTYPE.itemsize == L.vitamd_sched_row_bytes() == 64
    assert optim.ROW_DTYPE.itemsize == L.vitamd_mt_row_bytes() == 80
    fields = re.search(r"typedef\s+struct\s+vitamd_sched_row\s*\{(.*?)\}\s*vitamd_sched_row\s*;", header, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    declared = [n.strip().split()[-1] for decl in fields.split(";") if decl.strip() for n in decl.split(",")]
    assert declared == list(optim.SCHED_DTYPE.names), declared
    assert [optim.SCHED_DTYPE.fields[n][1] for n in optim.SCHED_DTYPE.names] == [0, 8, 16, 24, 32, 40, 48, 56]
    assert list(R.entry(1e-3, (0.9, 0.999), None)) == list(optim.SCHED_DTYPE.names)


def test_advance_refuses_before_any_launch():
    """On a machine without a GPU an attempted launch would be VITAMD_ERR_LAUNCH (3): each of these is refused first."""
    from vitamd import lib
    L = lib.load()
    SHAPE, ARG = 1, 2
    assert L.vitamd_sched_advance(4096, 8192, 0, None) == SHAPE
    assert L.vitamd_sched_advance(4096, 8192, -1, None) == SHAPE
    assert L.vitamd_sched_advance(None, 8192, 1, None) == ARG
    assert L.vitamd_sched_advance(4096, None, 1, None) == ARG
    assert L.vitamd_sched_advance(4096 + 4, 8192, 1, None) == ARG
    assert L.vitamd_sched_advance(4096, 8192 + 4, 1, None) == ARG


def _walk(group, start, launches):
    """the model's outputs for `launches` consecutive launches from counters `start`, beside hyper_row / lr_factor for the same steps"""
    import utils as U
    from vitamd import optim
    base, betas, schedule = group
    e = R.entry(base, betas, schedule, step=start, sched_t=start)
    for i in range(launches):
        k, t = start + i + 1, start + i
        got = R.advance(e)
        assert (e["step"], e["sched_t"]) == (k, t + 1)
        row = optim.hyper_row(base, betas, 1e-8, 0.0, k)
        f = 1.0 if schedule is None else U.lr_factor(t, *schedule)
        want = (np.float32(base * f), row[7], row[8])
        assert all(type(x) is np.float32 for x in got)
        assert got == want, (group, k, got, want)
        if schedule is not None:
            assert optim.lr_factor(t, *schedule) == f                               # the package's copy of utils.lr_factor
    return e


def test_model_of_the_advance_equals_hyper_row_and_lr_factor():
    for group in R.GROUPS:
        _walk(group, 0, R.LAUNCHES)
        for preset in R.PRESETS:
            _walk(group, preset, 1)
    # what the cases are there to cross
    assert R.factor(2, 3, 8, 0.1) == 2 / 3 and R.factor(3, 3, 8, 0.1) == 1.0 and R.factor(7, 3, 8, 0.1) < 0.6 and R.factor(8, 3, 8, 0.1) == 1.0
    e = R.entry(1e-3, (0.9, 0.999), None, step=R.PRESETS[-1])
    assert R.advance(e)[1:] == (np.float32(1.0), np.float32(1.0)) and 0.999 ** 10 ** 7 == 0.0


def test_constructor_refusals_and_groups():
    from vitamd.optim import AdamW
    w = [torch.nn.Parameter(torch.zeros(4))]
    for bad in ((1, 2), (1, 2, 3, 4), 5, (1.5, 8, 0.0), (-1, 8, 0.0), (2, 0, 0.0), (2, 8, -1e-5), (2, 8, float("nan")), (2, 8, float("inf")),
                (True, 8, 0.0), ("2", 8, 0.0)):
        with pytest.raises(ValueError):
            AdamW(w, capturable=True, schedule=bad)
    with pytest.raises(ValueError):
        AdamW(w, schedule=(2, 8, 1e-5))                                             # the schedule runs on the device: capturable only
    with pytest.raises(TypeError):
        AdamW(w, 1e-3, (0.9, 0.999), 1e-8, 1e-2, False, None, True)                 # keyword-only, like the other two
    plain = AdamW(w)
    assert plain.capturable is False and plain.schedule is None and plain.multi_tensor is False
    assert set(plain.param_groups[0]) == {"params", "lr", "betas", "eps", "weight_decay"}          # the default path's groups are untouched
    cap = AdamW(w, lr=2e-3, capturable=True)
    assert cap.capturable and cap.multi_tensor and cap.max_grad_norm is None        # capturable implies the multi-tensor path
    assert cap.param_groups[0]["sched_t"] == 0 and cap.param_groups[0]["lr"] == 2e-3 and "initial_lr" not in cap.param_groups[0]
    assert AdamW(w, capturable=True, max_grad_norm=1).max_grad_norm == 1.0
    sch = AdamW([{"params": w, "lr": 4e-3}, {"params": [torch.nn.Parameter(torch.zeros(3))], "lr": 0.0}], lr=1e-3, capturable=True,
                schedule=(2, 8, 1e-4))
    g0, g1 = sch.param_groups
    assert g0["initial_lr"] == 4e-3 and g0["sched_t"] == 0 and g0["lr"] == 0.0       # what a LambdaLR leaves at t = 0 of a warm-up
    assert sch._sched_fields(g0) == (2, 8, 1e-4 / 4e-3) and sch._sched_fields(g1) == (2, 8, 0.0)   # min_ratio 0 for a zero base
    assert sch.schedule == (2, 8, 1e-4) and set(sch.defaults) == {"lr", "betas", "eps", "weight_decay"}


def test_torch_scheduler_on_a_scheduled_optimiser_is_refused():
    import utils as U
    from vitamd.optim import AdamW
    w = [torch.nn.Parameter(torch.zeros(4))]
    opt = AdamW(w, lr=1e-3, capturable=True, schedule=(2, 8, 1e-4))
    with pytest.raises(ValueError, match="torch LR scheduler"):
        U.get_lr_scheduler(opt, 2, 8, 1e-4)
    with pytest.raises(ValueError, match="torch LR scheduler"):
        torch.optim.lr_scheduler.StepLR(opt, 3)
    opt.param_groups[0]["lr"] = 5e-4                                                # ... and a rate written from outside, at the next step
    with pytest.raises(ValueError, match="changed from outside"):
        opt.step()
    # without a schedule the rate is the caller's: a torch scheduler may drive it (the table is rebuilt when it moves)
    free = AdamW(w, lr=1e-3, capturable=True)
    U.get_lr_scheduler(free, 2, 8, 1e-4)
    assert free.param_groups[0]["lr"] == 0.0


def test_state_dict_moves_between_the_paths_and_torch():
    """torch.optim.AdamW (+ LambdaLR) -> capturable with a schedule -> the host-built path and torch.optim.AdamW: steps, moments, the base
    rate and the schedule position travel; no device is needed to load."""
    import utils as U
    from vitamd.optim import AdamW

    def params():
        g = torch.Generator().manual_seed(5)
        return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((6, 4), (7,))]

    src_p = params()
    src = torch.optim.AdamW([{"params": src_p[:1], "lr": 2e-3}, {"params": src_p[1:]}], lr=1e-3, betas=(0.9, 0.95))
    sched = U.get_lr_scheduler(src, 2, 8, 1e-4)
    for k in range(3):
        for i, p in enumerate(src_p):
            p.grad = torch.full_like(p, 0.1 * (k + 1) + i)
        src.step()
        sched.step()
    cap_p = params()
    cap = AdamW([{"params": cap_p[:1]}, {"params": cap_p[1:]}], capturable=True, schedule=(2, 8, 1e-4))
    cap.load_state_dict(src.state_dict())
    for g, s in zip(cap.param_groups, src.param_groups):
        assert g["sched_t"] == 3 and g["initial_lr"] == s["initial_lr"]            # the position: where the step counts are
        assert g["lr"] == pytest.approx(s["lr"], rel=1e-12)                         # the rate LambdaLR left there
    for p, q in zip(cap_p, src_p):
        assert set(cap.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and int(cap.state[p]["step"]) == 3
        assert torch.equal(cap.state[p]["exp_avg_sq"], src.state[q]["exp_avg_sq"])
    out = cap.state_dict()
    assert all({"sched_t", "initial_lr"} <= set(g) for g in out["param_groups"])
    for make in (lambda ps: AdamW(ps), lambda ps: AdamW(ps, multi_tensor=True), lambda ps: torch.optim.AdamW(ps),
                 lambda ps: AdamW(ps, capturable=True, schedule=(2, 8, 1e-4))):
        dst_p = params()
        dst = make([{"params": dst_p[:1]}, {"params": dst_p[1:]}])
        dst.load_state_dict(out)
        for p, q in zip(dst_p, src_p):
            assert int(dst.state[p]["step"]) == 3 and torch.equal(dst.state[p]["exp_avg"], src.state[q]["exp_avg"])
        assert dst.param_groups[0]["betas"] == (0.9, 0.95) and dst.param_groups[0]["sched_t"] == 3


def test_nothing_with_a_gradient_means_no_launch_and_no_step():
    from vitamd.optim import AdamW
    from vitamd.lib import VitamdError
    w = [torch.nn.Parameter(torch.zeros(4))]
    opt = AdamW(w, lr=1e-3, capturable=True, schedule=(2, 8, 1e-4), max_grad_norm=1.0)
    opt.step()
    assert opt.state_dict()["state"] == {} and opt.param_groups[0]["sched_t"] == 0 and opt.grad_norm is None and opt._table is None
    w[0].grad = torch.ones(4)                                                        # a host tensor: refused, nothing advanced
    with pytest.raises(VitamdError):
        opt.step()
    assert opt.param_groups[0]["sched_t"] == 0 and torch.equal(w[0].detach(), torch.zeros(4))


def test_training_scripts_take_graph():
    import train_videogpt
    import train_vit
    from vitamd.optim import AdamW
    for mod in (train_vit, train_videogpt):
        assert mod.parse_args([]).graph is False and mod.parse_args([]).dropout == 0.0
        args = mod.parse_args(["--graph", "--max_grad_norm", "0.5", "--warmup_steps", "3", "--train_steps", "9", "--lr", "1e-3"])
        opt = mod.make_optim(torch.nn.Linear(4, 4), args)
        assert type(opt) is AdamW and opt.capturable and opt.max_grad_norm == 0.5 and opt.schedule == (3, 9, 1e-4)
        assert mod.make_optim(torch.nn.Linear(4, 4), mod.parse_args(["--graph"])).max_grad_norm is None
        assert type(mod.make_optim(torch.nn.Linear(4, 4), mod.parse_args([]))) is torch.optim.AdamW
    with pytest.raises(SystemExit, match="--u8"):                                    # refused before any device is touched
        train_vit.main(["--graph", "--u8"])


def test_graphed_train_step_refusals_without_a_device():
    from vitamd.graph import GraphedTrainStep
    from vitamd.lib import VitamdError
    from vitamd.optim import AdamW
    model = torch.nn.Linear(4, 4)
    with pytest.raises(VitamdError):
        GraphedTrainStep(model, lambda x: model(x).sum(), (torch.zeros(2, 4),), AdamW(model.parameters(), capturable=True))
