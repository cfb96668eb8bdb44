"""Host side of the multi-tensor optimiser step (no GPU): the C ABI surface, the row layout, the chunk planner, the constructor's
validation, the refusals the entry points make before any launch, and the state_dict exchange with torch.optim.AdamW."""
import math
import re

import numpy as np
import pytest
import torch

import _abi

MT_NAMES = ["vitamd_mt_row_bytes", "vitamd_mt_chunk_elems", "vitamd_mt_grid_cap", "vitamd_mt_sumsq", "vitamd_mt_adamw", "vitamd_mt_scale"]


def test_mt_entry_points_are_declared_and_bound():
    from vitamd import lib, optim
    header = _abi.header()
    for name in MT_NAMES:
        assert name in _abi.declared()[0], name
        assert name in lib.SIGNATURES, name
    assert sorted(n for n in lib.SIGNATURES if n.startswith("vitamd_mt_")) == sorted(MT_NAMES)
    assert re.search(r"typedef\s+struct\s+vitamd_mt_row\s*\{", header)
    L = lib.load()
    assert lib.ABI_VERSION == 9 and L.vitamd_abi_version() == 9
    assert optim.ROW_DTYPE.itemsize == L.vitamd_mt_row_bytes() == 80
    chunk = L.vitamd_mt_chunk_elems()
    assert chunk > 0 and chunk % 4 == 0 and L.vitamd_mt_grid_cap() > 0
    # the fields in the header's order, the pointers and the count on their natural boundaries
    fields = re.search(r"typedef\s+struct\s+vitamd_mt_row\s*\{(.*?)\}\s*vitamd_mt_row\s*;", header, flags=re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    declared = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in decl.split(",")]
    declared = [d.split()[-1].lstrip("*") for d in declared]
    assert declared == list(optim.ROW_DTYPE.names), declared
    assert [optim.ROW_DTYPE.fields[n][1] for n in ("p", "g", "m", "v", "n", "first_chunk", "lr")] == [0, 8, 16, 24, 32, 40, 44]


def test_chunk_planner():
    from vitamd import lib, optim
    chunk = lib.load().vitamd_mt_chunk_elems()
    sizes = [1, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 1027]
    first, total = optim.plan_chunks(sizes, chunk)
    assert first == [0, 1, 2, 3, 4, 6] and total == 9
    assert optim.plan_chunks([], chunk) == ([], 0)
    assert optim.plan_chunks([5] * 7, 4) == ([0, 2, 4, 6, 8, 10, 12], 14)
    assert optim.plan_chunks([2 ** 33 + 1], 8192) == ([0], 2 ** 20 + 1)           # counts past 2^31 elements
    with pytest.raises(ValueError):
        optim.plan_chunks([4, 0], chunk)


def test_hyper_row_rounds_each_coefficient_once_from_the_doubles():
    from vitamd import optim
    b1, b2, k = 0.9, 0.999, 7
    row = optim.hyper_row(3e-4, (b1, b2), 1e-8, 0.05, k)
    want = (3e-4, 0.05, b1, 1.0 - b1, b2, 1.0 - b2, 1e-8, 1.0 / (1.0 - b1 ** k), 1.0 / math.sqrt(1.0 - b2 ** k))
    assert all(type(x) is np.float32 for x in row)
    assert row == tuple(np.float32(x) for x in want)
    assert row[5] != np.float32(1.0) - np.float32(b2)                              # 1 - beta2 is NOT formed from the rounded beta2


def test_constructor_validation():
    from vitamd.optim import AdamW
    w = [torch.nn.Parameter(torch.zeros(4))]
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            AdamW(w, max_grad_norm=bad)
    with pytest.raises(ValueError):
        AdamW(w, lr=-1.0, multi_tensor=True)
    with pytest.raises(TypeError):
        AdamW(w, 1e-3, (0.9, 0.999), 1e-8, 1e-2, True)                            # the new arguments are keyword-only
    plain = AdamW(w)
    assert plain.multi_tensor is False and plain.max_grad_norm is None
    assert AdamW(w, multi_tensor=True).multi_tensor is True and AdamW(w, multi_tensor=True).max_grad_norm is None
    clipped = AdamW(w, max_grad_norm=1)
    assert clipped.multi_tensor is True and clipped.max_grad_norm == 1.0           # max_grad_norm implies the multi-tensor path
    assert clipped.grad_norm is None and clipped.clip_coef is None
    assert set(clipped.defaults) == {"lr", "betas", "eps", "weight_decay"}         # nothing new reaches param_groups or a state_dict
    from vitamd import optim
    with pytest.raises(ValueError):
        optim.clip_grad_norm_(w, 0.0)


def test_nothing_with_a_gradient_means_no_launch():
    """Without a gradient neither the optimiser nor the free functions reach the device (this machine has none: a launch would raise)."""
    from vitamd import optim
    w = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(3))]
    opt = optim.AdamW(w, max_grad_norm=1.0)
    opt.step()
    assert opt.state_dict()["state"] == {} and opt.grad_norm is None and opt.clip_coef is None
    assert float(optim.grad_norm(w)) == 0.0 and float(optim.clip_grad_norm_(w, 1.0)) == 0.0


def test_host_tensors_are_refused():
    from vitamd import optim
    from vitamd.lib import VitamdError
    w = torch.nn.Parameter(torch.ones(8))
    w.grad = torch.ones(8)
    for call in (lambda: optim.AdamW([w], multi_tensor=True).step(), lambda: optim.grad_norm([w]), lambda: optim.clip_grad_norm_([w], 1.0)):
        with pytest.raises(VitamdError):
            call()
    assert torch.equal(w.detach(), torch.ones(8)) and torch.equal(w.grad, torch.ones(8))


def test_entry_points_refuse_before_any_launch():
    """The table is checked on the host's copy: a wrong plan is a shape error, a missing or misaligned pointer an argument error, and each
    is returned before a launch is attempted (on a machine without a GPU an attempted launch would be VITAMD_ERR_LAUNCH instead)."""
    from vitamd import lib, optim
    L = lib.load()
    chunk = L.vitamd_mt_chunk_elems()
    SHAPE, ARG = 1, 2

    def table(ptrs=(4096, 8192), sizes=None):
        sizes = sizes or [5, chunk + 1]
        rows = np.zeros(2, optim.ROW_DTYPE)
        rows["first_chunk"], total = optim.plan_chunks(sizes, chunk)
        rows["n"] = sizes
        for k in ("p", "g", "m", "v"):
            rows[k] = ptrs
        return rows, total

    dev, buf = 4096, 4096                                                          # never dereferenced: every call below is refused first
    rows, total = table()
    assert L.vitamd_mt_sumsq(rows.ctypes.data, dev, 2, total + 1, buf, buf, 1.0, None) == SHAPE
    assert L.vitamd_mt_adamw(rows.ctypes.data, dev, 2, total - 1, None, None) == SHAPE
    assert L.vitamd_mt_adamw(rows.ctypes.data, dev, 0, total, None, None) == SHAPE
    bad = rows.copy()
    bad["first_chunk"][1] = 2
    assert L.vitamd_mt_scale(bad.ctypes.data, dev, 2, total, buf, None) == SHAPE
    bad = rows.copy()
    bad["n"][0] = 0
    assert L.vitamd_mt_sumsq(bad.ctypes.data, dev, 2, total, buf, buf, 1.0, None) == SHAPE
    for key in ("p", "g", "m", "v"):
        for value in (0, 8192 + 4):
            bad = rows.copy()
            bad[key][1] = value
            assert L.vitamd_mt_adamw(bad.ctypes.data, dev, 2, total, None, None) == ARG, (key, value)
    for value in (0, 8192 + 4):
        bad = rows.copy()
        bad["g"][1] = value
        assert L.vitamd_mt_sumsq(bad.ctypes.data, dev, 2, total, buf, buf, 1.0, None) == ARG
        assert L.vitamd_mt_scale(bad.ctypes.data, dev, 2, total, buf, None) == ARG
    assert L.vitamd_mt_sumsq(None, dev, 2, total, buf, buf, 1.0, None) == ARG
    assert L.vitamd_mt_sumsq(rows.ctypes.data, None, 2, total, buf, buf, 1.0, None) == ARG
    assert L.vitamd_mt_sumsq(rows.ctypes.data, dev, 2, total, None, buf, 1.0, None) == ARG
    assert L.vitamd_mt_sumsq(rows.ctypes.data, dev, 2, total, buf, None, 1.0, None) == ARG
    assert L.vitamd_mt_adamw(rows.ctypes.data, None, 2, total, None, None) == ARG
    assert L.vitamd_mt_scale(rows.ctypes.data, dev, 2, total, None, None) == ARG


def test_state_dict_round_trips_from_torch_adamw():
    """torch.optim.AdamW -> vitamd AdamW (either path) -> torch.optim.AdamW: same keys, same values, nothing else in the groups."""
    from vitamd.optim import AdamW

    def params():
        g = torch.Generator().manual_seed(5)
        return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((6, 4), (7,))]

    src_p = params()
    src = torch.optim.AdamW([{"params": src_p[:1], "weight_decay": 0.0}, {"params": src_p[1:]}], lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
    for k in range(3):
        for i, p in enumerate(src_p):
            p.grad = torch.full_like(p, 0.1 * (k + 1) + i)
        src.step()
    sd = src.state_dict()
    for kwargs in ({}, {"multi_tensor": True}, {"max_grad_norm": 1.0}):
        mid_p = params()
        mid = AdamW([{"params": mid_p[:1]}, {"params": mid_p[1:]}], **kwargs)
        mid.load_state_dict(sd)
        for p, q in zip(mid_p, src_p):
            assert set(mid.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
            assert int(mid.state[p]["step"]) == 3
            assert torch.equal(mid.state[p]["exp_avg"], src.state[q]["exp_avg"])
        assert mid.param_groups[0]["weight_decay"] == 0.0 and mid.param_groups[1]["betas"] == (0.9, 0.95)
        out = mid.state_dict()
        assert [set(g) for g in out["param_groups"]] == [set(g) for g in sd["param_groups"]]
        dst_p = params()
        dst = torch.optim.AdamW([{"params": dst_p[:1]}, {"params": dst_p[1:]}])
        dst.load_state_dict(out)
        for p, q in zip(dst_p, src_p):
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(torch.as_tensor(dst.state[p][key]), torch.as_tensor(src.state[q][key])), key
        assert dst.param_groups[0]["weight_decay"] == 0.0 and dst.param_groups[1]["lr"] == 1e-3


def test_training_scripts_take_max_grad_norm():
    import train_videogpt
    import train_vit
    for mod in (train_vit, train_videogpt):
        args = mod.parse_args([])
        assert args.max_grad_norm is None
        assert mod.parse_args(["--max_grad_norm", "1.0"]).max_grad_norm == 1.0
        model = torch.nn.Linear(4, 4)
        assert type(mod.make_optim(model, args)) is torch.optim.AdamW
        clipped = mod.make_optim(model, mod.parse_args(["--max_grad_norm", "0.5"]))
        from vitamd.optim import AdamW
        assert type(clipped) is AdamW and clipped.max_grad_norm == 0.5 and clipped.multi_tensor
