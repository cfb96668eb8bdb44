"""The device-resident optimiser table and the captured training iteration on the GPU: the advance kernel against
its Python model, AdamW(capturable=True) against the host-built multi-tensor path and float64 torch, GraphedTrainStep against the eager
loop on a deterministic toy and on the real models, construction without side effects, checkpoints and stale graphs, refusals.

The float64 references, the fp32 floor runs and the bounds are those of test_gpu_optim_multi.py::test_clipped_steps_match_float64
(4 x the distance of torch's own fp32 CPU run from float64, + 1e-6), computed once per case and shared.  The toy's loss is made of
elementwise torch ops and full reductions only, so its gradients are the same bits on every run and a graph replay can be compared with
an eager step bit for bit where the arithmetic is the same."""
import copy
import functools

import numpy as np
import pytest
import torch

import _optim_graph_ref as R
import vit_oracle as O
import weights as W
from test_gpu_optim_multi import _coef32, _norm64
from test_gpu_streaming import Bounds, dev, randn

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
FIELDS = ("lr", "inv_bc1", "inv_sqrt_bc2")

# test 5, the real model: what is allowed on top of 4 x the eager-against-eager floor.  The first GPU run
# (profiles/graph_train/gpu_visit.md) measured the floor AND the graph-against-eager distances as exactly 0 at this shape: the step is
# deterministic run to run there and a replay computes the eager step's bits.  The constants therefore only have to cover what may
# legitimately differ when the floor happens to be 0: a learning rate one fp32 ulp apart at a rounding tie (6e-8 relative on one step's
# update) and the last bits of a loss near 11.5 (fp32 spacing 9.5e-7).  Reordered atomics, where they occur, show in the floor too.
UPDATE_CONST = 1e-5          # rel-L2 of the four-step parameter update p_4 - p_0, all parameters as one vector
LOSS_CONST = 1e-5            # absolute, on each of the four losses


# ------------------------------------------------------------------------------------------------ 1. the advance kernel alone
def _advance_case(n_rows, start):
    """rows of random bytes (the kernel must leave all but three floats of each alone), schedule entries of the three groups in rotation"""
    from vitamd import optim
    rows = np.frombuffer(np.random.default_rng(7 + n_rows).bytes(n_rows * optim.ROW_DTYPE.itemsize), dtype=optim.ROW_DTYPE).copy()
    sched = np.zeros(n_rows, optim.SCHED_DTYPE)
    entries = [R.entry(*R.GROUPS[r % len(R.GROUPS)], step=start, sched_t=start) for r in range(n_rows)]
    for name in optim.SCHED_DTYPE.names:
        sched[name] = [e[name] for e in entries]
    return rows, sched, entries


def _blank(rows):
    out = rows.copy()
    for name in FIELDS:
        out[name] = 0
    return out.tobytes()


def _launch_and_check(hip, n_rows, start, launches):
    from vitamd import optim
    rows, sched, entries = _advance_case(n_rows, start)
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(dev())
    d_sched = torch.from_numpy(sched.view(np.uint8).copy()).to(dev())
    worst = dict.fromkeys(FIELDS, 0.0)
    for i in range(launches):
        assert hip.vitamd_sched_advance(d_rows.data_ptr(), d_sched.data_ptr(), n_rows, torch.cuda.current_stream().cuda_stream) == 0
        got = d_rows.cpu().numpy().view(optim.ROW_DTYPE)
        got_sched = d_sched.cpu().numpy().view(optim.SCHED_DTYPE)
        want = [R.advance(e) for e in entries]
        for j, name in enumerate(FIELDS):
            w = np.array([x[j] for x in want], np.float32)
            ulps = np.abs(got[name].astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
            assert np.isfinite(got[name]).all() and ulps.max() <= 1.0, (name, start + i + 1, int(ulps.argmax()), got[name][ulps.argmax()], w[ulps.argmax()])
            worst[name] = max(worst[name], float(ulps.max()))
        assert _blank(got) == _blank(rows), f"launch {i + 1}: a byte outside lr / inv_bc1 / inv_sqrt_bc2 changed"
        assert (got_sched["step"] == start + i + 1).all() and (got_sched["sched_t"] == start + i + 1).all()
        for name in optim.SCHED_DTYPE.names[2:]:
            assert got_sched[name].tobytes() == sched[name].tobytes(), name
    print(f"  n_rows {n_rows} from {start}, {launches} launches: worst ulps {worst}")
    return got


@pytest.mark.parametrize("n_rows", [3, 300])
def test_advance_twelve_launches(hip, n_rows):
    """Three groups (a scheduled one, a constant one, a scheduled one at rate 0) over 12 launches: through the warm-up milestone, the cosine
    phase and train_steps into the constant phase.  300 rows: more than one workgroup has lanes."""
    got = _launch_and_check(hip, n_rows, 0, R.LAUNCHES)
    assert got["lr"][0] == np.float32(1e-3) and got["lr"][1] == np.float32(3e-4) and got["lr"][2] == 0.0       # past train_steps: the base rates


@pytest.mark.parametrize("n_rows", [1, 300])
def test_advance_from_preset_counters(hip, n_rows):
    for start in R.PRESETS:
        got = _launch_and_check(hip, n_rows, start, 1)
    assert (got["inv_bc1"] == 1.0).all() and (got["inv_sqrt_bc2"] == 1.0).all()      # k = 10^7: beta^k underflows, the corrections are exactly 1


# ------------------------------------------------------------------------------------------------ shared: references and bounds
def _reference_runs(p0, grads_of, groups_of, schedule, max_norm, steps):
    """(float64 run, fp32 floor run, float64 norm of every step, param_groups[0]["lr"] after every step): [clip_grad_norm_ +]
    torch.optim.AdamW + the schedule on the CPU; the floor run is fp32 with each step's clip coefficient taken from the float64 norm.
    grads_of(k, params, dtype) -> the gradients of step k."""
    import utils as U
    out, norms, lrs = [], [], []
    for dtype in (F64, F32):
        params = [torch.nn.Parameter(p.to(dtype).clone()) for p in p0]
        opt = torch.optim.AdamW(groups_of(params), eps=1e-8)
        sched = U.get_lr_scheduler(opt, *schedule)
        for k in range(steps):
            for p, g in zip(params, grads_of(k, params, dtype)):
                p.grad = g.clone()
            if dtype is F64:
                norms.append(_norm64([p.grad for p in params]))
                if max_norm is not None:
                    torch.nn.utils.clip_grad_norm_(params, max_norm)
            elif max_norm is not None:
                c = _coef32(norms[k], max_norm)
                for p in params:
                    p.grad.mul_(c)
            opt.step()
            sched.step()
            if dtype is F64:
                lrs.append(opt.param_groups[0]["lr"])
        out.append([(p.detach().double(), opt.state[p]["exp_avg"].double(), opt.state[p]["exp_avg_sq"].double()) for p in params])
    return out[0], out[1], norms, lrs


def _collect(params, opt):
    torch.cuda.synchronize()
    return [(p.detach().cpu().double(), opt.state[p]["exp_avg"].cpu().double(), opt.state[p]["exp_avg_sq"].cpu().double()) for p in params]


def _check_against_float64(b, tag, got, ref, f32, p0):
    """the bounds of test_gpu_optim_multi.py::test_clipped_steps_match_float64"""
    for i, start in enumerate(p0):
        start = start.double()
        for name, j in (("p", 0), ("exp_avg", 1), ("exp_avg_sq", 2)):
            bound = 4 * O.rel_l2(f32[i][j], ref[i][j]) + 1e-6
            b.lt(f"{tag} {name}[{i}]", O.rel_l2(got[i][j], ref[i][j]), min(bound, 1e-6) if name == "p" else bound)
        b.lt(f"{tag} update[{i}]", O.rel_l2(got[i][0] - start, ref[i][0] - start), 4 * O.rel_l2(f32[i][0] - start, ref[i][0] - start) + 1e-6)


# ------------------------------------------------------------------------------------------------ 2. capturable eager against the host-built path
STEPS2, SCHEDULE2 = 5, (2, 4, 1e-4)              # warm-up at t = 0, 1; cosine at 2, 3; back at the base rate at 4


def _groups2(params):
    return [{"params": params[0::2], "lr": 1e-3, "weight_decay": 0.05, "betas": (0.9, 0.999)},
            {"params": params[1::2], "lr": 3e-4, "weight_decay": 0.0, "betas": (0.9, 0.95)}]


@functools.lru_cache(maxsize=None)
def _inputs2(chunk):
    sizes = [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]
    p0 = [randn((n,), 800 + i) for i, n in enumerate(sizes)]
    gs = [[randn((n,), 900 + 10 * k + i) for i, n in enumerate(sizes)] for k in range(STEPS2)]
    return p0, gs


@functools.lru_cache(maxsize=None)
def _references2(chunk, max_norm):
    p0, gs = _inputs2(chunk)
    return _reference_runs(p0, lambda k, params, dtype: [g.to(dtype) for g in gs[k]], _groups2, SCHEDULE2, max_norm, STEPS2)


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_capturable_eager_matches_the_host_built_path(hip, max_norm):
    """Eight tensors around the chunk size in two groups under a schedule, five steps, the same gradients on both paths; with
    max_grad_norm = 1.0 the clip is active on every step (randn gradients: a norm of about 200).  The capturable path's gradients are
    static tensors, so its table is built once - and once more when one gradient is re-allocated between steps 2 and 3."""
    import utils as U
    from vitamd.optim import AdamW
    chunk = hip.vitamd_mt_chunk_elems()
    p0, gs = _inputs2(chunk)
    ref, f32, norms, ref_lrs = _references2(chunk, max_norm)
    b = Bounds()

    host_p = [torch.nn.Parameter(p.clone().to(dev())) for p in p0]
    host = AdamW(_groups2(host_p), eps=1e-8, multi_tensor=True, max_grad_norm=max_norm)
    host_sched = U.get_lr_scheduler(host, *SCHEDULE2)
    cap_p = [torch.nn.Parameter(p.clone().to(dev())) for p in p0]
    cap = AdamW(_groups2(cap_p), eps=1e-8, capturable=True, schedule=SCHEDULE2, max_grad_norm=max_norm)
    for p in cap_p:
        p.grad = torch.empty_like(p)
    tables = []
    for k in range(STEPS2):
        if k == 2:
            cap_p[4].grad = torch.empty_like(cap_p[4])           # a pointer moves: the table is built and uploaded again
        for hp, cp, g in zip(host_p, cap_p, gs[k]):
            hp.grad = g.to(dev())
            cp.grad.copy_(hp.grad)
        host.step()
        host_sched.step()
        cap.step()
        if not any(cap._table is t for t in tables):
            tables.append(cap._table)
        assert all(cap.state[p]["step"] == k + 1 and type(cap.state[p]["step"]) is int for p in cap_p)
        assert cap.param_groups[0]["sched_t"] == k + 1
        for g_cap, g_host in zip(cap.param_groups, host.param_groups):
            assert abs(g_cap["lr"] - g_host["lr"]) <= 1e-12 * abs(g_host["lr"]), (k, g_cap["lr"], g_host["lr"])
        assert abs(cap.param_groups[0]["lr"] - ref_lrs[k]) <= 1e-12 * abs(ref_lrs[k])
        if max_norm is None:
            assert cap.grad_norm is None and cap.clip_coef is None and host.grad_norm is None
        else:
            assert cap.grad_norm.dim() == 0 and cap.grad_norm.is_cuda and cap.clip_coef.dim() == 0
            gn, cc = float(cap.grad_norm), float(cap.clip_coef)
            assert gn == float(host.grad_norm) and cc == float(host.clip_coef), (k, gn, float(host.grad_norm))    # the norm does not depend on the hypers
            assert cc < 1.0
            b.lt(f"norm[{k}]", abs(gn - norms[k]) / norms[k], 1e-6)
    assert len(tables) == 2, len(tables)
    _check_against_float64(b, "host-built", _collect(host_p, host), ref, f32, p0)
    _check_against_float64(b, "capturable", _collect(cap_p, cap), ref, f32, p0)
    b.check()


# ------------------------------------------------------------------------------------------------ 3. the graph on a deterministic toy
TOY_C = (65, 33)                                  # 2145 elements: a scalar tail of one
TOY_STEPS, TOY_SCHEDULE, TOY_MAX_NORM = 6, (2, 5, 1e-4), 0.05


def _toy_loss(a, b, c, x):
    n = TOY_C[0] * TOY_C[1]
    return (a * x[:5]).sum() * 0.1 + (b * x).pow(2).mean() + (c * x[:n].view(TOY_C)).tanh().sum() * 1e-3


class Toy(torch.nn.Module):
    """a: five elements; b: one chunk and a tail of three; c: a matrix.  `extra` adds a parameter the loss never reads."""

    def __init__(self, p0, extra=False):
        super().__init__()
        self.a, self.b, self.c = (torch.nn.Parameter(p.clone()) for p in p0)
        if extra:
            self.d = torch.nn.Parameter(torch.ones(4))

    def forward(self, x):
        return _toy_loss(self.a, self.b, self.c, x)


def _toy_groups(params):
    a, b, c = params[:3]
    return [{"params": [a, c], "lr": 1e-3, "weight_decay": 0.05, "betas": (0.9, 0.999)},
            {"params": [b] + list(params[3:]), "lr": 3e-4, "weight_decay": 0.0, "betas": (0.9, 0.95)}]


@functools.lru_cache(maxsize=None)
def _toy_inputs(chunk):
    p0 = [randn((5,), 1000), randn((chunk + 3,), 1001), randn(TOY_C, 1002)]
    xs = [randn((chunk + 3,), 1010 + k) for k in range(TOY_STEPS)]
    return p0, xs


@functools.lru_cache(maxsize=None)
def _toy_references(chunk):
    p0, xs = _toy_inputs(chunk)

    def grads_of(k, params, dtype):
        return torch.autograd.grad(_toy_loss(*params, xs[k].to(dtype)), params)

    return _reference_runs(p0, grads_of, _toy_groups, TOY_SCHEDULE, TOY_MAX_NORM, TOY_STEPS)


def _toy(chunk, extra=False, **kwargs):
    from vitamd.optim import AdamW
    p0, xs = _toy_inputs(chunk)
    toy = Toy(p0, extra).to(dev())
    opt = AdamW(_toy_groups(list(toy.parameters())), eps=1e-8, max_grad_norm=TOY_MAX_NORM, **kwargs)
    return toy, opt, [x.to(dev()) for x in xs]


def _graphed_toy(chunk):
    from vitamd.graph import GraphedTrainStep
    toy, opt, xs = _toy(chunk, capturable=True, schedule=TOY_SCHEDULE)
    return toy, opt, xs, GraphedTrainStep(toy, lambda x: toy(x), (xs[0],), opt)


def _snapshot(params, opt):
    """every bit a construction could disturb: parameters, moments where present, the host mirrors"""
    torch.cuda.synchronize()
    tensors = [p.detach().clone() for p in params]
    for p in params:
        st = opt.state[p] if p in opt.state else {}
        tensors += [st[k].clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
    mirrors = [(g["lr"], g["sched_t"], g.get("initial_lr")) for g in opt.param_groups]
    mirrors += [opt.state[p]["step"] for p in params if p in opt.state]
    return tensors, mirrors


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]


def test_graphed_toy_matches_the_eager_loop(hip):
    import utils as U
    chunk = hip.vitamd_mt_chunk_elems()
    p0, _ = _toy_inputs(chunk)
    ref, f32, norms, ref_lrs = _toy_references(chunk)
    b = Bounds()
    toy_e, opt_e, xs = _toy(chunk, multi_tensor=True)
    sched_e = U.get_lr_scheduler(opt_e, *TOY_SCHEDULE)
    toy_g, opt_g, _, step = _graphed_toy(chunk)
    assert step.captures == 1
    for k in range(TOY_STEPS):
        opt_e.zero_grad(set_to_none=True)
        loss_e = toy_e(xs[k])
        loss_e.backward()
        opt_e.step()
        sched_e.step()
        loss_g = step(xs[k])
        assert loss_g.dim() == 0 and float(loss_g) == float(loss_e.detach()), (k, float(loss_g), float(loss_e.detach()))
        gn_g, gn_e = float(opt_g.grad_norm), float(opt_e.grad_norm)
        assert gn_g == gn_e and float(opt_g.clip_coef) == float(opt_e.clip_coef) < 1.0, (k, gn_g, gn_e)
        b.lt(f"norm[{k}]", abs(gn_g - norms[k]) / norms[k], 1e-6)
        assert all(opt_g.state[p]["step"] == k + 1 for p in toy_g.parameters())
        for g_g, g_e in zip(opt_g.param_groups, opt_e.param_groups):
            assert abs(g_g["lr"] - g_e["lr"]) <= 1e-12 * abs(g_e["lr"]), (k, g_g["lr"], g_e["lr"])
        assert abs(opt_g.param_groups[0]["lr"] - ref_lrs[k]) <= 1e-12 * abs(ref_lrs[k])
        assert all(p.grad is g for p, g in zip(step.params, step.grads))             # the static gradients are attached again
    assert step.captures == 1
    _check_against_float64(b, "eager", _collect(list(toy_e.parameters()), opt_e), ref, f32, p0)
    _check_against_float64(b, "graph", _collect(list(toy_g.parameters()), opt_g), ref, f32, p0)
    b.check()


# ------------------------------------------------------------------------------------------------ 4. construction is free of side effects
@pytest.mark.parametrize("stepped", [False, True])
def test_construction_leaves_the_toy_alone(hip, stepped):
    """fresh (no moments yet: construction creates them as zeros) and after one eager capturable step (moments present, counters at 1)"""
    from vitamd.graph import GraphedTrainStep
    chunk = hip.vitamd_mt_chunk_elems()
    toy, opt, xs = _toy(chunk, capturable=True, schedule=TOY_SCHEDULE)
    params = list(toy.parameters())
    if stepped:
        toy(xs[0]).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
    before = _snapshot(params, opt)
    step = GraphedTrainStep(toy, lambda x: toy(x), (xs[0],), opt)
    after = _snapshot(params, opt)
    if stepped:
        assert _same(before, after)
    else:                                                                           # the moments exist now, as zeros; no step count moved
        assert all(torch.equal(x, y) for x, y in zip(before[0], after[0][:3])) and before[1] == after[1][:2]
        assert all(not t.any() for t in after[0][3:]) and after[1][2:] == [0, 0, 0]
    step(xs[1])
    assert all(opt.state[p]["step"] == (2 if stepped else 1) for p in params)
    assert opt.param_groups[0]["sched_t"] == (2 if stepped else 1)


# ------------------------------------------------------------------------------------------------ 5. the real models
VIT_LR, VIT_SCHEDULE, VIT_STEPS = 1e-3, (2, 6, 1e-4), 4


@functools.lru_cache(maxsize=None)
def _vit_case():
    import train_vit as TV
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    sd = W.classifier_state(11, 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, 10)
    xs = [W.normal(120 + i, "x", (64, 3, 32, 32)) for i in range(VIT_STEPS)]
    ys = [W.randint(120 + i, "y", (64,), 10) for i in range(VIT_STEPS)]
    return cfg, sd, xs, ys


def _vit(**kwargs):
    import train_vit as TV
    from vitamd.optim import AdamW
    cfg, sd, xs, ys = _vit_case()
    m = TV.ViTClassifier(cfg, num_classes=10)
    m.load_state_dict(sd)
    m = m.cuda()
    opt = AdamW(m.parameters(), lr=VIT_LR, weight_decay=0.05, max_grad_norm=1.0, **kwargs)
    return m, opt, [x.cuda() for x in xs], [y.cuda() for y in ys]


def _flat_update(m, sd):
    return torch.cat([(p.detach().cpu().double() - sd[k].double()).reshape(-1) for k, p in m.named_parameters()])


def test_graphed_vit_matches_the_eager_loop(hip):
    """BASELINE configs[0] (ViT-S at 32x32, batch 64), lm.cross_entropy, clip at 1.0, schedule (2, 6, lr / 10), four iterations on new
    inputs.  The model's gradients differ from run to run by reordered atomics, and Adam's normalisation amplifies that where a gradient
    is near zero, so the yardstick is the eager loop against a second eager run: the graph may be 4 x that floor + a constant away.
    Measured on an MI355X (profiles/graph_train/gpu_visit.md): see the figures printed below against UPDATE_CONST / LOSS_CONST."""
    import train_vit as TV
    import utils as U
    from vitamd import lm
    from vitamd.graph import GraphedTrainStep
    from vitamd.lib import VitamdError
    _, sd, _, _ = _vit_case()

    def eager():
        m, opt, xs, ys = _vit()
        sched = U.get_lr_scheduler(opt, *VIT_SCHEDULE)
        losses = [float(TV.train_step(m, x, y, opt, sched, loss_fn=lm.cross_entropy).detach()) for x, y in zip(xs, ys)]
        return losses, _flat_update(m, sd), [g["lr"] for g in opt.param_groups]

    losses_a, upd_a, lr_a = eager()
    losses_b, upd_b, _ = eager()
    m, opt, xs, ys = _vit(capturable=True, schedule=VIT_SCHEDULE)
    params = list(m.parameters())
    before = _snapshot(params, opt)
    step = GraphedTrainStep(m, lambda x, y: lm.cross_entropy(m(x), y), (xs[0], ys[0]), opt)
    after = _snapshot(params, opt)
    n = len(params)
    assert all(torch.equal(x, y) for x, y in zip(before[0], after[0][:n])) and before[1] == after[1][:1]       # test 4 on the real model
    assert all(not t.any() for t in after[0][n:]) and after[1][1:] == [0] * n
    losses_g = []
    for k, (x, y) in enumerate(zip(xs, ys)):
        losses_g.append(float(step(x, y)))
        assert all(opt.state[p]["step"] == k + 1 for p in params)
    upd_g = _flat_update(m, sd)
    assert step.captures == 1 and abs(opt.param_groups[0]["lr"] - lr_a[0]) <= 1e-12 * lr_a[0]
    floor_u, dist_u = O.rel_l2(upd_b, upd_a), O.rel_l2(upd_g, upd_a)
    floor_l = max(abs(a - c) for a, c in zip(losses_a, losses_b))
    dist_l = max(abs(a - c) for a, c in zip(losses_a, losses_g))
    print(f"  losses eager {losses_a}\n  losses eager again {losses_b}\n  losses graph {losses_g}")
    print(f"  update p_4 - p_0, rel-L2: eager against eager (floor) {floor_u:.3e}, graph against eager {dist_u:.3e}")
    print(f"  losses, worst absolute difference: floor {floor_l:.3e}, graph against eager {dist_l:.3e}")
    assert all(np.isfinite(v) for v in losses_g)
    assert abs(losses_g[0] - losses_a[0]) < 1e-6                                     # step 1: before any update
    b = Bounds()
    b.lt("update", dist_u, 4 * floor_u + UPDATE_CONST)
    b.lt("losses", dist_l, 4 * floor_l + LOSS_CONST)
    b.check()
    with pytest.raises(VitamdError):
        step(xs[0][:32], ys[0][:32])                                                 # another batch size
    with pytest.raises(VitamdError):
        step(xs[0], ys[0].int())                                                     # another dtype
    assert all(opt.state[p]["step"] == VIT_STEPS for p in params)


def test_graphed_videogpt_step(hip):
    """A two-layer causal VideoGPT on model.loss(tokens), the stack's smallest shapes of test_gpu_lm.py (frame_size 16, 4 frames, S width):
    the loss of step 1 against the eager route on the same weights, and the step counts."""
    import train_videogpt as V
    from vitamd.graph import GraphedTrainStep
    from vitamd.optim import AdamW
    cfg = V.VideoGPTConfig(frame_size=16, codebook_size=256, transformer="S", max_frames=4, dropout=0.0)
    cfg.trans_config.n_layers = 2
    D, Nc = cfg.n_embd, cfg.codebook_size
    sd = {"tok_embed.weight": W.normal(3, "tok_embed", (Nc + 1, D)), "pos_embed.weight": W.normal(3, "pos_embed", (cfg.max_tokens, D))}
    sd.update(W.transformer_state(3, "transformer.", 2, D, causal_block=cfg.max_tokens))
    sd.update(W.linear_state(3, "proj.", Nc, D))
    model = V.VideoGPT(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    tokens = [W.randint(130 + i, "tokens", (2, 4, 16), Nc).cuda() for i in range(2)]
    want = float(model.loss(tokens[0]).detach())
    opt = AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0, capturable=True, schedule=(1, 4, 1e-5))
    step = GraphedTrainStep(model, lambda tok: model.loss(tok), (tokens[0],), opt)
    got = float(step(tokens[0]))
    print(f"  VideoGPT step-1 loss: graph {got:.7f}, eager {want:.7f}")
    assert np.isfinite(got) and abs(got - want) < 1e-6
    second = float(step(tokens[1]))
    assert np.isfinite(second) and all(opt.state[p]["step"] == 2 for p in model.parameters())
    assert opt.param_groups[0]["sched_t"] == 2 and step.captures == 1


# ------------------------------------------------------------------------------------------------ 6. staleness and checkpoints
def test_checkpoint_and_stale_graph(hip):
    chunk = hip.vitamd_mt_chunk_elems()

    def state(toy, opt):
        return [t for row in _collect(list(toy.parameters()), opt) for t in row]

    toy, opt, xs, step = _graphed_toy(chunk)
    for k in range(4):
        step(xs[k])
    straight = state(toy, opt)

    # a. two replays, a checkpoint, fresh objects, two more
    toy, opt, xs, step = _graphed_toy(chunk)
    step(xs[0]), step(xs[1])
    torch.cuda.synchronize()
    saved_model = {k: v.clone() for k, v in toy.state_dict().items()}
    # deep copies, as a checkpoint read back from a file holds: load_state_dict keeps a tensor that already has the parameter's dtype and
    # device, so a second optimiser loaded from the live state_dict() would share its moments with the first
    saved_optim = copy.deepcopy(opt.state_dict())
    toy2, opt2, _ = _toy(chunk, capturable=True, schedule=TOY_SCHEDULE)
    toy2.load_state_dict(saved_model)
    opt2.load_state_dict(copy.deepcopy(saved_optim))
    from vitamd.graph import GraphedTrainStep
    step2 = GraphedTrainStep(toy2, lambda x: toy2(x), (xs[0],), opt2)
    assert opt2.param_groups[0]["sched_t"] == 2 and all(opt2.state[p]["step"] == 2 for p in toy2.parameters())
    step2(xs[2]), step2(xs[3])
    resumed = state(toy2, opt2)
    assert all(torch.equal(x, y) for x, y in zip(resumed, straight))
    assert all(opt2.state[p]["step"] == 4 for p in toy2.parameters()) and opt2.param_groups[0]["sched_t"] == 4

    # b. load_state_dict on a live step: the moments are new tensors, so the next replay captures again - and gives the same result
    assert step.captures == 1
    opt.load_state_dict(copy.deepcopy(saved_optim))
    step(xs[2])
    assert step.captures == 2
    step(xs[3])
    assert step.captures == 2
    assert all(torch.equal(x, y) for x, y in zip(state(toy, opt), straight))
    assert all(opt.state[p]["step"] == 4 for p in toy.parameters()) and opt.param_groups[0]["sched_t"] == 4

    # c. the saved optimiser state loads into torch.optim.AdamW
    plain = torch.optim.AdamW(_toy_groups(list(Toy(_toy_inputs(chunk)[0]).parameters())))
    plain.load_state_dict(saved_optim)
    assert all(int(st["step"]) == 2 for st in plain.state.values()) and len(plain.state) == 3


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(hip):
    import train_vit as TV
    from vitamd.graph import GraphedTrainStep
    from vitamd.lib import VitamdError
    from vitamd.optim import AdamW
    chunk = hip.vitamd_mt_chunk_elems()
    toy, opt, xs = _toy(chunk, multi_tensor=True)
    with pytest.raises(ValueError):
        GraphedTrainStep(toy, lambda x: toy(x), (xs[0],), opt)                       # not capturable
    with pytest.raises(ValueError):
        GraphedTrainStep(toy, lambda x: toy(x), (xs[0],), torch.optim.AdamW(toy.parameters()))
    m = TV.ViTClassifier(TV.ViTConfig(32, 3, 16, "S", 1, 0.1), num_classes=10).cuda()
    with pytest.raises(NotImplementedError):
        GraphedTrainStep(m, lambda x: m(x).sum(), (torch.zeros(2, 3, 32, 32, device=dev()),), AdamW(m.parameters(), capturable=True))
    toy, opt, xs, step = _graphed_toy(chunk)
    with pytest.raises(VitamdError):
        step(xs[0][:-1])                                                             # another shape at replay
    with pytest.raises(VitamdError):
        step(xs[0], xs[0])
    assert all(opt.state[p]["step"] == 0 for p in toy.parameters())
    # a parameter the loss never reads: no gradient after the warm-up -> refused at construction, nothing touched, no state created
    toy, opt, xs = _toy(chunk, extra=True, capturable=True, schedule=TOY_SCHEDULE)
    params = list(toy.parameters())
    before = _snapshot(params, opt)
    with pytest.raises(VitamdError):
        GraphedTrainStep(toy, lambda x: toy(x), (xs[0],), opt)
    assert _same(before, _snapshot(params, opt)) and len(opt.state) == 0
