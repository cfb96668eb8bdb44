"""The multi-tensor optimiser step on the GPU: bit-identity with the per-tensor path, clipped steps and the in-place
clip against float64 torch, the deterministic norm, refusal before any launch, and a training loop in which the clip is active.

The chunk size and the grid cap are read from the library, so the shapes follow the constants: tensors of chunk - 0 / + 1 elements, one of
two chunks and a ragged third with a scalar tail, and cap + 3 five-element tensors, which alone make more chunks than the grid has
workgroups.  References are float64 torch on the CPU.  Where a bound is a multiple of a floor, the floor is torch's own fp32 CPU evaluation
of the same sequence given the clip coefficient of the float64 norm (torch's fp32 CPU norm itself is 4e-5 off float64 at these sizes and
is no yardstick; the chunked fp32-partials / fp64-finish scheme is 2e-9 off): the 1e-6 added to 4 x floor is what the norm is allowed."""
import functools

import pytest
import torch

import vit_oracle as O
from test_gpu_streaming import ADAMW_LRS, Bounds, dev, randn

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SMALL = 5                                                          # elements of each of the cap + 3 small tensors


def _consts(hip):
    return hip.vitamd_mt_chunk_elems(), hip.vitamd_mt_grid_cap()


def _listed(chunk):
    return [(3072, 768), (2 * chunk + 1027,), (chunk,), (chunk + 1,), (5, 7, 3), (3,), (1,)]


def _device_set(big, small):
    """Device copies of the CPU tensors: the listed ones one by one, the small ones as rows of ONE padded buffer (row stride 32 bytes, so
    each is a contiguous, 16-byte aligned view) - a single copy instead of thousands."""
    out = [t.clone().to(dev()) for t in big]
    if small is not None:
        buf = torch.zeros(small.shape[0], 8)
        buf[:, :SMALL] = small
        buf = buf.to(dev())
        out += [buf[i, :SMALL] for i in range(small.shape[0])]
    return out


@functools.lru_cache(maxsize=None)
def _wide_inputs(chunk, cap):
    """Test 1 / 3: initial values and five steps of gradients for the seven listed shapes and cap + 3 small tensors (CPU, never modified)."""
    shapes = _listed(chunk)
    p0 = ([randn(s, 300 + i) for i, s in enumerate(shapes)], randn((cap + 3, SMALL), 299))
    gs = [([randn(s, 400 + 10 * k + i) for i, s in enumerate(shapes)], randn((cap + 3, SMALL), 390 + k)) for k in range(len(ADAMW_LRS))]
    return p0, gs


def test_multi_tensor_is_bit_identical_to_the_per_tensor_path(hip):
    """Two parameter groups (lr, weight decay and betas all differ), five steps under changing learning rates, one parameter without a
    gradient on step 2 (its bias correction lags from then on): p, exp_avg, exp_avg_sq and step of every tensor are torch.equal."""
    from vitamd.optim import AdamW
    chunk, cap = _consts(hip)
    (big0, small0), gs = _wide_inputs(chunk, cap)
    lag = 3                                                        # the (chunk + 1,) tensor

    def run(**kwargs):
        params = [torch.nn.Parameter(t) for t in _device_set(big0, small0)]
        groups = [{"params": params[0::2], "weight_decay": 0.05, "betas": (0.9, 0.999)},
                  {"params": params[1::2], "weight_decay": 0.0, "betas": (0.9, 0.95)}]
        opt = AdamW(groups, lr=ADAMW_LRS[0], eps=1e-8, **kwargs)
        for k, (lr, (gbig, gsmall)) in enumerate(zip(ADAMW_LRS, gs)):
            opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = lr, 0.5 * lr
            for i, (p, g) in enumerate(zip(params, _device_set(gbig, gsmall))):
                p.grad = None if (k == 1 and i == lag) else g
            opt.step()
        torch.cuda.synchronize()
        return params, opt

    pa, oa = run()
    pb, ob = run(multi_tensor=True)
    assert oa.multi_tensor is False and ob.multi_tensor is True and len(pa) == 7 + cap + 3
    bad = []
    for i, (a, b) in enumerate(zip(pa, pb)):
        sa, sb = oa.state[a], ob.state[b]
        assert int(sa["step"]) == int(sb["step"]) == (4 if i == lag else 5), i
        for name, x, y in (("p", a, b), ("exp_avg", sa["exp_avg"], sb["exp_avg"]), ("exp_avg_sq", sa["exp_avg_sq"], sb["exp_avg_sq"])):
            if not torch.equal(x.detach(), y.detach()):
                bad.append((i, name, int((x.detach() != y.detach()).sum())))
    assert not bad, bad[:20]
    assert not torch.equal(pa[0].detach().cpu(), big0[0])          # and the steps did move the parameters


# ------------------------------------------------------------------------------------------------ clipped steps, in-place clip
def _clip_shapes(chunk):
    return [(3072, 768), (2 * chunk + 1027,), (5, 7, 3), (1,)]


@functools.lru_cache(maxsize=None)
def _clip_inputs(chunk):
    """Test 2 / 4: steps 1-3 are randn gradients (norm about 1.5e3: clipped at 1.0), steps 4-5 the same kind scaled by 1e-4 (about 0.15:
    not clipped).  Flat elements 100..199 of the first tensor never get a gradient."""
    shapes = _clip_shapes(chunk)
    ps = [randn(s, 500 + i) for i, s in enumerate(shapes)]
    gs = []
    for k in range(len(ADAMW_LRS)):
        row = [randn(s, 600 + 10 * k + i, 1.0 if k < 3 else 1e-4) for i, s in enumerate(shapes)]
        row[0].view(-1)[100:200] = 0.0
        gs.append(row)
    return ps, gs


def _norm64(tensors):
    return float(torch.sqrt(sum((t.double() ** 2).sum() for t in tensors)))


def _coef32(norm64, max_norm):
    """The clip coefficient of the float64 norm, rounded to fp32."""
    return float(torch.tensor(min(1.0, max_norm / (norm64 + 1e-6)), dtype=F64).to(F32))


@functools.lru_cache(maxsize=None)
def _clipped_references(chunk):
    """(float64 run, fp32 floor run, float64 norm of every step): clip_grad_norm_(1.0) + torch.optim.AdamW on the CPU; the floor run is
    fp32 with each step's coefficient taken from the float64 norm."""
    ps, gs = _clip_inputs(chunk)
    out, norms = [], []
    for dtype in (F64, F32):
        params = [torch.nn.Parameter(p.to(dtype).clone()) for p in ps]
        opt = torch.optim.AdamW(params, lr=ADAMW_LRS[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
        for k, (lr, row) in enumerate(zip(ADAMW_LRS, gs)):
            opt.param_groups[0]["lr"] = lr
            for p, g in zip(params, row):
                p.grad = g.to(dtype).clone()
            if dtype is F64:
                norms.append(float(torch.nn.utils.clip_grad_norm_(params, 1.0)))
            else:
                c = _coef32(norms[k], 1.0)
                for p in params:
                    p.grad.mul_(c)
            opt.step()
        out.append([(p.detach().double(), opt.state[p]["exp_avg"].double(), opt.state[p]["exp_avg_sq"].double()) for p in params])
    return out[0], out[1], norms


def test_clipped_steps_match_float64(hip):
    from vitamd.optim import AdamW
    chunk, _ = _consts(hip)
    ps, gs = _clip_inputs(chunk)
    ref, f32, norms = _clipped_references(chunk)
    b = Bounds()
    params = [torch.nn.Parameter(p.clone().to(dev())) for p in ps]
    opt = AdamW(params, lr=ADAMW_LRS[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, max_grad_norm=1.0)
    kept = [[g.clone().to(dev()) for g in row] for row in gs]
    seen = []
    for k, (lr, row) in enumerate(zip(ADAMW_LRS, kept)):
        opt.param_groups[0]["lr"] = lr
        for p, g in zip(params, row):
            p.grad = g
        opt.step()
        assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda and opt.clip_coef.dim() == 0 and opt.clip_coef.is_cuda
        seen.append((opt.grad_norm, opt.clip_coef))                # of that step: a later step must not overwrite them
    torch.cuda.synchronize()
    for k, (gn, cc) in enumerate(seen):
        gn, cc = float(gn), float(cc)
        print(f"  step {k + 1}: norm {gn:.9g} (float64 {norms[k]:.12g}) coef {cc:.9g}")
        b.lt(f"norm[{k}]", abs(gn - norms[k]) / norms[k], 1e-6)
        if k < 3:
            assert cc < 1.0 and abs(cc - _coef32(norms[k], 1.0)) <= 2e-6 * cc, (k, cc)
        else:
            assert cc == 1.0, (k, cc)
    for row_dev, row in zip(kept, gs):                             # p.grad is not rewritten
        assert all(torch.equal(g.cpu(), g0) for g, g0 in zip(row_dev, row))
    got = [(p.detach().cpu().double(), opt.state[p]["exp_avg"].cpu().double(), opt.state[p]["exp_avg_sq"].cpu().double()) for p in params]
    for i, p0 in enumerate(ps):
        p0 = p0.double()
        for name, j in (("p", 0), ("exp_avg", 1), ("exp_avg_sq", 2)):
            bound = 4 * O.rel_l2(f32[i][j], ref[i][j]) + 1e-6
            b.lt(f"{name}[{i}]", O.rel_l2(got[i][j], ref[i][j]), min(bound, 1e-6) if name == "p" else bound)
        b.lt(f"update[{i}]", O.rel_l2(got[i][0] - p0, ref[i][0] - p0), 4 * O.rel_l2(f32[i][0] - p0, ref[i][0] - p0) + 1e-6)
    never = got[0][2].view(-1)[100:200]
    assert torch.equal(never, torch.zeros_like(never)) and torch.isfinite(got[0][0].view(-1)[100:200]).all()
    b.check()


def test_clip_grad_norm_in_place(hip):
    from vitamd import optim
    chunk, _ = _consts(hip)
    _, gs = _clip_inputs(chunk)
    g0 = gs[0]
    norm = _norm64(g0)
    b = Bounds()

    def params():
        out = [torch.nn.Parameter(torch.zeros(g.shape, device=dev())) for g in g0]
        for p, g in zip(out, g0):
            p.grad = g.clone().to(dev())
        return out

    ref = [torch.nn.Parameter(g.double()) for g in g0]
    for p, g in zip(ref, g0):
        p.grad = g.double().clone()
    ref_norm = float(torch.nn.utils.clip_grad_norm_(ref, 1.0))
    c = _coef32(norm, 1.0)
    ps = params()
    got = optim.clip_grad_norm_(ps, 1.0)
    assert got.dim() == 0 and got.is_cuda
    b.lt("norm", abs(float(got) - ref_norm) / ref_norm, 1e-6)
    for i, (p, r, g) in enumerate(zip(ps, ref, g0)):
        floor = O.rel_l2(g * c, r.grad)
        b.lt(f"grad[{i}]", O.rel_l2(p.grad.cpu(), r.grad), 4 * floor + 1e-6)
    ps = params()
    got = optim.clip_grad_norm_(ps, 1e9)
    torch.cuda.synchronize()
    b.lt("norm, not clipped", abs(float(got) - norm) / norm, 1e-6)
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(ps, g0))
    b.check()
    from vitamd.lib import VitamdError
    p = torch.nn.Parameter(torch.zeros(6, 4, device=dev()))
    p.grad = torch.ones(4, 6, device=dev()).t()                    # not contiguous: a scaled copy would not be written back
    with pytest.raises(VitamdError):
        optim.clip_grad_norm_([p], 1.0)
    assert torch.equal(p.grad, torch.ones(6, 4, device=dev()))
    b.lt("norm of a non-contiguous gradient", abs(float(optim.grad_norm([p])) - 24 ** 0.5) / 24 ** 0.5, 1e-6)
    b.check()


# ------------------------------------------------------------------------------------------------ the norm
def test_grad_norm_whole_per_tensor_and_reproducible(hip):
    """Tensors scaled by 1e3, 1, 1e-3 in rotation.  The whole set, each listed tensor alone, and each listed tensor with one five-element
    tensor after it (a chunk dropped or counted twice at a row boundary shows): within 1e-6 of float64; a second call gives the same bits."""
    from vitamd import optim
    chunk, cap = _consts(hip)
    _, gs = _wide_inputs(chunk, cap)
    gbig, gsmall = gs[0]
    scales = [1e3, 1.0, 1e-3]
    big = [g * scales[i % 3] for i, g in enumerate(gbig)]
    small = gsmall * torch.tensor([scales[(7 + i) % 3] for i in range(gsmall.shape[0])]).unsqueeze(1)
    cpu = big + list(small)
    params = []
    for g in _device_set(big, small):
        p = torch.nn.Parameter(g)                                  # the norm never looks at the parameter itself
        p.grad = g
        params.append(p)
    b = Bounds()

    def check(name, idx):
        want = _norm64([cpu[i] for i in idx])
        first, second = optim.grad_norm([params[i] for i in idx]), optim.grad_norm([params[i] for i in idx])
        assert first.dim() == 0 and first.is_cuda and torch.equal(first, second), name
        b.lt(name, abs(float(first) - want) / want, 1e-6)

    check("whole set", range(len(params)))
    for i in range(7):
        check(f"tensor {i} alone", [i])
        check(f"tensor {i} + a small one", [i, 7])
    check("a small one + tensor 1", [7, 1])
    assert float(optim.grad_norm(params[5])) > 0                   # a single tensor is accepted as torch's function accepts it
    for g, g0 in zip((params[0].grad, params[1].grad, params[-1].grad), (cpu[0], cpu[1], cpu[-1])):
        assert torch.equal(g.cpu(), g0)                            # the norm reads only
    b.check()


# ------------------------------------------------------------------------------------------------ refusal
def test_refusal_leaves_memory_alone(hip):
    """One parameter (then one gradient) 4 bytes off the 16-byte boundary among aligned ones: VitamdError before any launch, every buffer
    as it was, no step count advanced."""
    from vitamd import optim
    from vitamd.lib import VitamdError
    buf = randn((1040,), 700).to(dev())
    gbuf = randn((1040,), 701).to(dev())
    others = [torch.nn.Parameter(randn(s, 702 + i).to(dev())) for i, s in enumerate([(1024,), (33, 7)])]
    off = torch.nn.Parameter(buf[1:1025])                          # a view: storage starts 4 bytes off the boundary
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    params = [others[0], off, others[1]]
    for i, p in enumerate(params):
        p.grad = randn(tuple(p.shape), 710 + i).to(dev())
    watched = [buf, gbuf] + [p.detach() for p in others] + [p.grad for p in params]
    before = [t.clone() for t in watched]
    for kwargs in ({"multi_tensor": True}, {"max_grad_norm": 1.0}):
        opt = optim.AdamW(params, lr=1e-3, **kwargs)
        with pytest.raises(VitamdError):
            opt.step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(watched, before))
        assert all(int(opt.state[p].get("step", 0)) == 0 for p in params)
    off.grad = None
    others[0].grad = gbuf[1:1025]                                  # now a gradient is off the boundary
    assert others[0].grad.data_ptr() % 16 == 4
    for call in (lambda: optim.AdamW(params, lr=1e-3, max_grad_norm=1.0).step(), lambda: optim.clip_grad_norm_(params, 1.0),
                 lambda: optim.grad_norm(params)):
        with pytest.raises(VitamdError):
            call()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(watched, before))


# ------------------------------------------------------------------------------------------------ a training loop
def test_training_loop_with_active_clipping(hip):
    """ViTClassifier S/16 at 32x32 on the weights and batch of train_steps_s32.pt.  max_grad_norm is half the step-1 gradient norm of the
    CPU oracle (fp32), so the clip is active by construction.  Four steps of oracle forward/backward + clip_grad_norm_ + torch.optim.AdamW
    + the schedule on the CPU against four of train_vit.train_step with the new optimiser: losses at the tolerances of
    test_training_steps_match_reference_loop."""
    import train_vit as TV
    import utils as U
    import weights as W
    from conftest import load_golden
    from vitamd.optim import AdamW
    c = load_golden("train_steps_s32.pt")["cfg"]
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    sd = W.classifier_state(c["seed"], 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, c["num_classes"])
    images = W.normal(c["seed"], "images", (c["batch"], 3, 32, 32))
    labels = W.randint(c["seed"], "labels", (c["batch"],), c["num_classes"])
    ocfg = O.OracleViTConfig.preset(32, 3, 16, "S", 1)

    _, _, g1 = O.classifier_loss_and_grads(images, labels, sd, ocfg)
    norm1 = _norm64(list(g1.values()))
    max_norm = 0.5 * norm1

    cpu = {k: torch.nn.Parameter(v.clone()) for k, v in sd.items()}
    opt = torch.optim.AdamW(cpu.values(), lr=c["lr"], weight_decay=c["weight_decay"])
    sched = U.get_lr_scheduler(opt, c["warmup"], c["train_steps"], c["min_lr"])
    ref = []
    for _ in range(c["steps"]):
        _, loss, grads = O.classifier_loss_and_grads(images, labels, {k: p.detach() for k, p in cpu.items()}, ocfg)
        for k, p in cpu.items():
            p.grad = grads[k].clone()
        torch.nn.utils.clip_grad_norm_(cpu.values(), max_norm)
        opt.step()
        sched.step()
        ref.append(float(loss))

    m = TV.ViTClassifier(cfg, num_classes=c["num_classes"])
    m.load_state_dict(sd)
    m = m.cuda()
    optim = AdamW(m.parameters(), lr=c["lr"], weight_decay=c["weight_decay"], max_grad_norm=max_norm)
    sched = U.get_lr_scheduler(optim, c["warmup"], c["train_steps"], c["min_lr"])
    images, labels = images.cuda(), labels.cuda()
    losses, coefs = [], []
    for _ in range(c["steps"]):
        losses.append(float(TV.train_step(m, images, labels, optim, sched).detach()))
        coefs.append((float(optim.grad_norm), float(optim.clip_coef)))
    print(f"  oracle step-1 norm {norm1:.6g}, max_grad_norm {max_norm:.6g}; (norm, coef) per step {coefs}\n  losses {losses}\n  ref    {ref}")
    assert coefs[0][1] < 1.0
    assert abs(losses[0] - ref[0]) < 5e-3
    for a, r in zip(losses, ref):
        assert abs(a - r) < 3e-2 * max(1.0, abs(r)), (losses, ref)
