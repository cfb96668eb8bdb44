"""The perceptual loss on the MI355X (vitamd/perceptual.py, csrc/perceptual.hip) against the float64 references of tests/_perceptual_ref.py:
the depthwise 7x7 convolution and the resize + normalise kernels, forward and backward, at the shapes where the kernels can go wrong; the
whole loss and its gradient on a small network; one ConvNeXt-S stage-1 block at real width (C = 96: the K-padding path); train_step with
the term switched on.  Bounds: _perceptual_ref's docstring."""
import functools
import warnings

import pytest
import torch

import _perceptual_ref as R
import vit_oracle as O

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16

# (H, W, C), B = 2: every tap meets padding; the same at ConvNeXt's width; the real stage-4 map; non-square with a width that is no
# multiple of 64; one pixel past the kernel's pixel tile (1 row x 8 columns) in each direction and one vector group past its 64-channel tile
DW_SHAPES = [(2, 2, 8), (3, 5, 96), (7, 7, 128), (14, 9, 96), (2, 9, 68)]
# (h_in, w_in) -> size: 5 taps; 5 and 3 taps, rectangular; upsample; identity; the training shape
RESIZE_CASES = [((20, 20), 16), ((40, 24), 16), ((12, 12), 16), ((16, 16), 16), ((256, 256), 224)]
SMALL = dict(depths=(1, 1, 2, 1), dims=(32, 64, 96, 128), num_classes=40, size=64)


def _check(name, got, ref, t32, bf16_out=False):
    e, e32 = R.dist(got.cpu(), ref), R.dist(t32, ref)
    print(f"{name}: {e:.3e} (torch fp32 {e32:.3e}, bound {R.bound(e32, bf16_out):.3e})")
    return [] if e <= R.bound(e32, bf16_out) else [f"{name}: {e:.3e} > {R.bound(e32, bf16_out):.3e}"]


@pytest.mark.parametrize("in_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv7_matches_float64(hip, shape, in_bf16):
    from vitamd import ops
    H, W, C = shape
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C)
    x, dy = torch.randn((2, H, W, C), generator=g), torch.randn((2, H, W, C), generator=g)
    w, b, add = torch.randn((C, 7, 7), generator=g) / 7, torch.randn((C,), generator=g), torch.randn((2, H, W, C), generator=g)
    if in_bf16:                                     # bf16 rows are read exactly: the reference sees the same rounded values
        x, dy = x.to(BF16).float(), dy.to(BF16).float()
    dt = BF16 if in_bf16 else F32
    y = ops.dwconv7_fwd(x.cuda().to(dt), w.cuda(), b.cuda())
    dx = ops.dwconv7_bwd(dy.cuda().to(dt), w.cuda())
    dxa = ops.dwconv7_bwd(dy.cuda().to(dt), w.cuda(), add=add.cuda())
    y0 = ops.dwconv7_fwd(x.cuda().to(dt), w.cuda())
    torch.cuda.synchronize()
    assert y.dtype == F32 and dx.dtype == F32 and tuple(y.shape) == tuple(dx.shape) == (2, H, W, C)
    t_y, t_dx = R.dwconv_torch(x, w, b, dy, F32)
    ref_dx = R.dwconv_bwd_ref(dy, w)
    fails = _check("fwd", y, R.dwconv_ref(x, w, b), t_y) + _check("bwd", dx, ref_dx, t_dx)
    fails += _check("bwd+add", dxa, ref_dx + add.double(), t_dx + add)
    # the input gradient as the adjoint: <conv(x), dy> = <x, conv^T(dy)>.  Each of the two fp32 results carries at most 50 * 2^-24 of the sum of
    # its absolute products (49 multiply-adds), so the two sides differ by at most 100 * 2^-24 * <|dy|, conv(|x|, |w|)>
    lhs, rhs = float((y0.cpu().double() * dy.double()).sum()), float((x.double() * dx.cpu().double()).sum())
    scale = float((dy.double().abs() * R.dwconv_ref(x.abs(), w.abs())).sum())
    print(f"adjoint: {lhs:.9e} vs {rhs:.9e}, |diff| / scale {abs(lhs - rhs) / scale:.3e}")
    assert abs(lhs - rhs) <= 100 * 2.0 ** -24 * scale
    assert not fails, fails


@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1]}")
def test_resize_norm_matches_float64(hip, case):
    from vitamd import ops, perceptual as P
    (h, w), size = case
    B = 2
    g = torch.Generator().manual_seed(h * 100 + w)
    img, gout = torch.rand((B, 3, h, w), generator=g), torch.randn((B, 3, size, size), generator=g)
    dev = torch.device("cuda")
    th, tw = P.band_tables(h, size, dev), P.band_tables(w, size, dev)
    mean, std = torch.tensor(R.MEAN, device=dev), torch.tensor(R.STD, device=dev)
    rows, nchw = ops.resize_norm_fwd(img.cuda(), th[0], tw[0], mean, std, size, want_rows=True, want_nchw=True)
    grows = R.nchw_to_rows(gout)
    grows[:, 48:] = float("nan")                    # the pad columns of the gradient rows are never read
    dimg = ops.resize_norm_bwd(grows.cuda(), th[1], tw[1], std, B, h, w, size)
    torch.cuda.synchronize()
    ref = R.resize_norm_ref(img, size)
    t_out, t_dimg = R.resize_norm_torch(img, size, F32, gout)
    assert tuple(rows.shape) == (B * (size // 4) ** 2, 64) and rows.dtype == BF16
    assert not bool(rows[:, 48:].float().abs().max() > 0)
    assert torch.equal(R.rows_to_nchw(rows.cpu(), B, size), nchw.cpu().to(BF16))          # one value, stored twice
    fails = _check("fwd fp32", nchw, ref, t_out) + _check("fwd bf16 rows", R.rows_to_nchw(rows.cpu().float(), B, size), ref, t_out, True)
    fails += _check("bwd", dimg, R.resize_norm_bwd_ref(gout, h, w), t_dimg)
    assert not fails, fails


@functools.lru_cache(maxsize=None)
def _small_case(seed):
    """weights, images, the float64 loss and gradient, and torch's bf16-autocast distances from them, computed once per seed"""
    sd = R.random_state(SMALL["depths"], SMALL["dims"], SMALL["num_classes"], seed)
    inp, tgt = R.images(2, 72, 72, 100 + seed)
    loss, grad = R.loss_and_grad(sd, inp, tgt, SMALL["depths"], SMALL["size"])
    l16, g16 = R.loss_and_grad(sd, inp, tgt, SMALL["depths"], SMALL["size"], how="torch", dtype=F32, autocast=True)
    return sd, inp, tgt, loss, grad, R.rel(l16, loss), float((g16.double() - grad).norm() / grad.norm())


def _floors(case):
    cases = [case(s) for s in range(3)]
    return max(c[-2] for c in cases), max(c[-1] for c in cases)


def _small_module(sd):
    from vitamd.perceptual import PerceptualLoss
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        m = PerceptualLoss(weights=sd, **SMALL).cuda()
    assert not [w for w in seen if "stand-in" in str(w.message)]           # weights are given: nothing to warn about
    return m


def test_whole_loss_and_input_gradient_match_float64(hip):
    sd, inp, tgt, loss_ref, grad_ref, _, _ = _small_case(0)
    f_loss, f_grad = _floors(_small_case)
    m = _small_module(sd)
    assert not m.training and all(not p.requires_grad for p in m.parameters())
    x, t = inp.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
    loss = m(x, t)
    assert loss.dim() == 0 and loss.dtype == F32
    loss.backward()
    torch.cuda.synchronize()
    e_loss, e_grad = R.rel(loss.detach().cpu(), loss_ref), O.rel_l2(x.grad.cpu(), grad_ref)
    print(f"loss {float(loss.detach()):.6f} (float64 {float(loss_ref):.6f}) rel {e_loss:.3e} floor {f_loss:.3e}; gradient rel-L2 {e_grad:.3e} floor {f_grad:.3e}")
    assert t.grad is None and all(p.grad is None for p in m.parameters())
    assert tuple(x.grad.shape) == tuple(inp.shape) and x.grad.dtype == F32
    # the same bits on a second call, loss and gradient
    x2 = inp.cuda().requires_grad_(True)
    loss2 = m(x2, tgt.cuda())
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(x2.grad, x.grad)
    with torch.no_grad():                           # no gradient wanted: the same loss, nothing saved
        assert torch.equal(m(inp.cuda(), tgt.cuda()), loss.detach())
    assert e_loss <= 2 * f_loss + 1e-3 and e_grad <= 2 * f_grad + 1e-3


@functools.lru_cache(maxsize=None)
def _block_case(seed):
    """one stage-1 block at ConvNeXt-S's real width: C = 96 on an 8 x 8 map, B = 2"""
    C = 96
    sd = {k: v for k, v in R.random_state((1, 1, 1, 1), (C, 128, 128, 128), 8, 10 + seed).items() if k.startswith("features.1.0.")}
    g = torch.Generator().manual_seed(20 + seed)
    x, gy = torch.randn((2, 8, 8, C), generator=g), torch.randn((2, 8, 8, C), generator=g)

    def run(dtype, how, autocast=False):
        xx = x.to(dtype).requires_grad_(True)
        with torch.autocast("cpu", dtype=BF16, enabled=autocast):
            y = R.block_ref(xx, {k: v.to(dtype) for k, v in sd.items()}, "features.1.0.", dtype, how).float() if autocast else \
                R.block_ref(xx, {k: v.to(dtype) for k, v in sd.items()}, "features.1.0.", dtype, how)
        y.backward(gy.to(y.dtype))
        return y.detach(), xx.grad
    y, dx = run(F64, "restated")
    y16, dx16 = run(F32, "torch", True)
    return sd, x, gy, y, dx, float((y16.double() - y).norm() / y.norm()), float((dx16.double() - dx).norm() / dx.norm())


def test_stage1_block_at_real_width(hip):
    from vitamd import perceptual as P
    sd, x, gy, y_ref, dx_ref, _, _ = _block_case(0)
    f_y, f_dx = _floors(_block_case)
    full = R.random_state((1, 1, 1, 1), (96, 128, 128, 128), 8, 10)
    assert all(torch.equal(full[k], v) for k, v in sd.items())
    m = P.PerceptualLoss(weights=full, depths=(1, 1, 1, 1), dims=(96, 128, 128, 128), num_classes=8, size=32).cuda()
    prep = m.prepared()
    p = prep["stages"][0][0]
    assert tuple(p["w1"].shape) == (384, 128) and tuple(p["w2t"].shape) == (384, 128)       # K = 96 carried at 128 with zero columns
    saved = []
    y = P.block_fwd(x.cuda().view(-1, 96), p, 2, 8, 8, saved)
    dx = P.block_bwd(gy.cuda().view(-1, 96), p, 2, 8, 8, saved.pop(), prep["scratch"][96])
    torch.cuda.synchronize()
    e_y, e_dx = O.rel_l2(y.cpu().view(2, 8, 8, 96), y_ref), O.rel_l2(dx.cpu().view(2, 8, 8, 96), dx_ref)
    print(f"block output rel-L2 {e_y:.3e} floor {f_y:.3e}; input gradient rel-L2 {e_dx:.3e} floor {f_dx:.3e}")
    assert e_y <= 2 * f_y + 1e-3 and e_dx <= 2 * f_dx + 1e-3


def test_train_step_with_the_perceptual_term(hip):
    """train_titok.train_step with a PerceptualLoss: the loss is mse + 0.5 * perceptual + quantiser loss on the same weights, and the
    tokenizer's encoder and decoder receive gradients"""
    import train_titok as TT
    from test_gpu_parity import _tokenizer_model
    _, model, _, images = _tokenizer_model("titok_s256.pt")
    perc = _small_module(R.random_state(SMALL["depths"], SMALL["dims"], SMALL["num_classes"], 0))
    optim = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    with torch.no_grad():
        recon, _, qloss = model(images)
        parts = (float(torch.nn.functional.mse_loss(recon, images)), float(perc(recon, images)), float(qloss))
    loss = float(TT.train_step(model, images, optim, perceptual=perc, perceptual_weight=0.5))
    expect = parts[0] + 0.5 * parts[1] + parts[2]
    print(f"train_step loss {loss:.6f}; mse {parts[0]:.6f} + 0.5 * perceptual {parts[1]:.6f} + quantiser {parts[2]:.6f} = {expect:.6f}")
    assert loss == loss and abs(loss) < float("inf") and parts[1] > 0
    assert abs(loss - expect) <= 1e-5 * max(1.0, abs(expect))       # the same kernels on the same weights and images: fp32 summation noise only
    for part in (model.enc, model.dec):
        grads = [p.grad for p in part.parameters()]
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    assert all(p.grad is None for p in perc.parameters())
