"""The memory-bound kernels past their grid caps, against float64 references.

Every streaming kernel outside the GEMMs and attention caps its grid and walks the rest of its data in a grid-stride loop (casts, dropout,
im2col, column sums, LayerNorm, the 3x3 convolution, fused AdamW).  Each shape here is the smallest that crosses a cap with a ragged
remainder: a partially filled last pass and a tail.  A wrong stride, a wrong tail owner or a per-workgroup partial folded too early passes
every smaller shape of the suite and corrupts exactly the sizes the models train at.

References are float64 torch on the CPU of the same formula, or torch's own bit-exact rounding where the operation is a rounding or a gather.
Where a bound is not one the suite already holds the same quantity to, it is 4 x the distance of torch's own fp32 CPU evaluation from the
float64 reference at that shape, computed inside the test (the factor allows for the different summation order); never the kernel's output."""
import functools

import numpy as np
import pytest
import torch

import _dropout_ref as R
import vit_oracle as O

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def dev():
    return torch.device("cuda")


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def r16(x):
    return x.to(BF16).float()


class Bounds:
    """Collects (name, measured, bound) so that one run reports every figure of a test; check() asserts them all (NaN fails)."""

    def __init__(self):
        self.rows = []

    def lt(self, name, value, bound):
        self.rows.append((name, float(value), float(bound)))
        print(f"  {name}: {float(value):.3e} (bound {float(bound):.2e})")

    def check(self):
        bad = [r for r in self.rows if not r[1] < r[2]]
        assert not bad, bad


# ------------------------------------------------------------------------------------------ casts, im2col, column sums, embed backward
def test_cast_bf16_past_the_grid_cap(hip):
    """4096 workgroups x 256 lanes x 8 elements = 8 388 608 before the loop starts: three more partial passes and a 5-element tail."""
    from vitamd import ops
    n = 8388608 + 3 * 2048 + 5
    x = randn((n,), 42)
    assert torch.equal(ops.cast_bf16(x.to(dev())).cpu(), x.to(BF16))


def test_cast_bf16_rounds_to_nearest_even_on_every_upper_half(hip):
    """For each of the 65 536 upper halves h: the fp32 patterns h<<16 | 0x7fff (just below the tie), | 0x8000 (the tie), | 0x8001 (just
    above) must round as torch rounds them, bit for bit; a NaN input must give a NaN."""
    from vitamd import ops
    h = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    bits = np.stack([h | np.uint32(0x7fff), h | np.uint32(0x8000), h | np.uint32(0x8001)], axis=1).reshape(-1)
    x = torch.from_numpy(bits.view(np.int32).copy()).view(F32)
    got = ops.cast_bf16(x.to(dev())).cpu()
    want = x.to(BF16)
    nan = torch.isnan(x)
    assert int(nan.sum()) == 2 * 128 * 3                         # exponent 0xff, either sign, any upper mantissa: the low half is never zero
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])
    assert torch.isnan(got[nan]).all()


@pytest.mark.parametrize("B,C,H,W,p", [(57, 3, 224, 224, 16), (8, 3, 300, 300, 6)])
def test_im2col_past_the_grid_cap(hip, B, C, H, W, p):
    """16-B path: 8192 x 256 lanes x 4 = 8 388 608 output elements per pass (8 580 096 here); scalar path (p % 4 != 0): 2 097 152 (2 160 000)."""
    from vitamd import ops
    img = randn((B, C, H, W), 43)
    got = ops.im2col(img.to(dev()), p)
    assert got.numel() > (8388608 if p % 4 == 0 else 2097152)
    assert torch.equal(got.float().cpu(), r16(O.patchify(img, p)).reshape(-1, C * p * p))


@pytest.mark.parametrize("M,N,prefill", [(5000, 768, 0.0), (70, 264, 0.0), (1, 8, 0.0), (140001, 256, 0.0), (5000, 768, 7.0), (5000, 770, 0.0), (5000, 770, -3.0)])
def test_colsum_exact_on_integers(hip, M, N, prefill):
    """N % 8 == 0 takes the 16-byte kernel (every real bias gradient), 770 the scalar one.  Integer-valued inputs in [-3, 3]: every partial
    sum is exact in fp32, so the result equals the float64 sum bit for bit whatever the order of the atomics.  (70, 264): the last
    256-column block is partly outside N; (140 001, 256): row slabs of 69 rows, not a multiple of the 8 row groups; `out` is accumulated into."""
    from vitamd import ops
    m = ints((M, N), -3, 3, 44)
    out = torch.full((N,), prefill, device=dev())
    ops.colsum(m.to(dev(), BF16), out=out)
    assert torch.equal(out.cpu().double(), m.double().sum(0) + prefill)


@pytest.mark.parametrize("B,seq,extra,D", [(3, 5, 1, 1280), (65, 9, 2, 256)])
def test_embed_bwd_exact_on_integers(hip, B, seq, extra, D):
    """D = 1280: the second pass of the 1024-column loop; B = 65: three batch chunks of 32, the last of one sample.  Integer-valued g:
    dpos, dextra and dbias are exact, dyp is the bf16 copy bit for bit."""
    from vitamd import ops
    g = ints((B * seq, D), -4, 4, 45)
    dpos, dextra, dyp, dbias = ops.embed_bwd(g.to(dev()), B, seq, extra, D)
    g3 = g.view(B, seq, D).double()
    assert torch.equal(dpos.cpu().double(), g3[:, extra:].sum(0))
    assert torch.equal(dextra.cpu().double(), g3[:, :extra].sum(0))
    assert torch.equal(dyp.cpu(), g.view(B, seq, D)[:, extra:].reshape(-1, D).to(BF16))
    assert torch.equal(dbias.cpu().double(), g3[:, extra:].sum((0, 1)))


# ------------------------------------------------------------------------------------------ the dropout contract
DROP_P, DROP_SEED = 0.3, (0x5bd1e995 << 32) | 0x2545f491          # a seed with a non-zero high word
DROP_N = 2097152 + 777                                           # 8192 workgroups x 256 lanes, + a ragged second pass


def _keepscale(n, group=1):
    """fp32 tensor: scale where tests/_dropout_ref.py keeps flat index i // group, 0 elsewhere"""
    k = torch.from_numpy(R.mask(n, DROP_SEED, DROP_P, group=group))
    return k, k.float() * float(R.scale(DROP_P))


def _nonzero_randn(shape, seed):
    x = randn(shape, seed)
    x[x == 0] = 1.0                                               # a zero input would hide its mask bit
    return x


def test_dropout_kernels_follow_the_documented_mask(hip):
    """ops.dropout (fp32, bf16) and ops.cast_bf16_dropout against the numpy restatement of csrc/common.h: the mask element for element,
    kept values = x * fp32(1 / (1 - p)) rounded as the kernel's type says, past the 2 097 152-element grid cap."""
    from vitamd import ops
    x = _nonzero_randn((DROP_N,), 51)
    keep, ks = _keepscale(DROP_N)
    y = ops.dropout(x.to(dev()), DROP_P, DROP_SEED).cpu()
    assert torch.equal(y != 0, keep)
    assert torch.equal(y, x * ks)
    xb = x.to(BF16)
    yb = ops.dropout(xb.to(dev()), DROP_P, DROP_SEED).cpu()
    assert torch.equal(yb != 0, keep)
    assert torch.equal(yb, (xb.float() * ks).to(BF16))
    yc = ops.cast_bf16_dropout(x.to(dev()), (DROP_P, DROP_SEED)).cpu()
    assert torch.equal(yc != 0, keep)
    assert torch.equal(yc, (r16(x) * ks).to(BF16))


def test_drop_path_mask_is_one_decision_per_group(hip):
    from vitamd import ops
    group = 50 * 128
    x = _nonzero_randn((DROP_N,), 52)
    keep, ks = _keepscale(DROP_N, group=group)
    assert 0 < int(keep[::group].sum()) < keep[::group].numel()
    y = ops.dropout(x.to(dev()), DROP_P, DROP_SEED, group=group).cpu()
    assert torch.equal(y != 0, keep)
    assert torch.equal(y, x * ks)


def test_layernorm_bwd_dropout_mask_is_row_major(hip):
    """The bf16 copy of LayerNorm backward is the gradient of a dropped-out [M, D] Linear output: gb = bf16(bf16(g) * keep(row * D + col)
    * scale), at M = 4101 > the 4096 rows of the column-sum form's first pass."""
    from vitamd import ops
    M, D = 4101, 256
    x = (randn((M, D), 53, 2.0) + 0.5).to(dev())
    dy = r16(randn((M, D), 54)).to(dev(), BF16)
    gres = randn((M, D), 55).to(dev())
    _, _, mean, rstd = ops.layernorm_fwd(x)
    cs = torch.zeros(D, device=dev())
    g, gb = ops.layernorm_bwd(dy, x, mean, rstd, g_res=gres, want_bf16=True, colsum=cs, dropout=(DROP_P, DROP_SEED))
    keep, ks = _keepscale(M * D)
    g, gb = g.cpu(), gb.cpu()
    assert int((r16(g) == 0).sum()) == 0
    assert torch.equal(gb != 0, keep.view(M, D))
    assert torch.equal(gb, (r16(g) * ks.view(M, D)).to(BF16))
    g0, _ = ops.layernorm_bwd(dy, x, mean, rstd, g_res=gres)
    assert torch.equal(g, g0.cpu())                               # the fp32 gradient carries no mask


def test_linear_dropout_resid_mask_is_row_major(hip):
    """A zero GEMM with bias 2 and a zero residual shows the epilogue's mask directly: element (row, col) of the [M, N] output uses index
    row * N + col."""
    from vitamd import ops
    M, N, K = 1000, 768, 256
    a = torch.zeros(M, K, device=dev(), dtype=BF16)
    w = torch.zeros(N, K, device=dev(), dtype=BF16)
    bias = torch.full((N,), 2.0, device=dev())
    resid = torch.zeros(M, N, device=dev())
    y = ops.linear_dropout_resid(a, w, bias, resid, (DROP_P, DROP_SEED)).cpu()
    keep, ks = _keepscale(M * N)
    assert torch.equal(y != 0, keep.view(M, N))
    assert torch.equal(y, r16(2.0 * ks).view(M, N))


# ------------------------------------------------------------------------------------------ non-affine LayerNorm
def _ln_case(M, D, colsums):
    """The assertions and bounds of test_gpu_kernels.py::test_layernorm_fwd_bwd, against float64."""
    from vitamd import ops
    b = Bounds()
    x = randn((M, D), 21, 2.0) + 0.5
    add = r16(randn((M, D), 22))
    xs, y, mean, rstd = ops.layernorm_fwd(x.to(dev()), addend=add.to(dev(), BF16))
    xr = (x.double() + add.double()).requires_grad_(True)
    yr = O.layer_norm(xr)
    b.lt("x_sum", O.rel_l2(xs.cpu(), xr), 1e-6)
    b.lt("y", O.rel_l2(y.float().cpu(), r16(yr)), 2.9e-5)
    b.lt("mean", O.rel_l2(mean.cpu(), xr.mean(-1)), 1.0e-6)
    _, y2, _, _ = ops.layernorm_fwd(x.to(dev()))
    b.lt("y no addend", O.rel_l2(y2.float().cpu(), r16(O.layer_norm(x.double()))), 3.0e-5)
    dy = r16(randn((M, D), 23))
    yr.backward(dy.double())
    if colsums:
        gres = randn((M, D), 24)
        cs = torch.zeros(D, device=dev())
        g, gb = ops.layernorm_bwd(dy.to(dev(), BF16), xs, mean, rstd, g_res=gres.to(dev()), want_bf16=True, colsum=cs)
        b.lt("g", O.rel_l2(g.cpu(), gres.double() + xr.grad), 1.0e-6)
        assert torch.equal(gb.float().cpu(), r16(g.cpu()))
        b.lt("colsum", O.rel_l2(cs.cpu(), gb.cpu().double().sum(0)), 1.0e-6)
    g2, none = ops.layernorm_bwd(dy.to(dev(), BF16), xs, mean, rstd)
    assert none is None
    b.lt("g plain", O.rel_l2(g2.cpu(), xr.grad), 1.0e-6)
    b.check()


@pytest.mark.parametrize("M,D", [(65541, 256), (65541, 128)])
def test_layernorm_past_the_row_cap(hip, M, D):
    """16384 workgroups x 4 rows = 65 536 rows before the loop starts (forward with and without addend, backward without column sums);
    D = 128 takes the generic kernels."""
    _ln_case(M, D, False)


@pytest.mark.parametrize("M,D", [(4101, 256), (12289, 768), (4101, 200)])
def test_layernorm_bwd_colsum_past_the_row_cap(hip, M, D):
    """The column-sum form (the one every layer uses) caps at 1024 workgroups x 4 rows: its register partials live across loop passes and
    are folded once after the loop.  (12 289, 768): four passes, the last with one row; D = 200: the generic kernel's atomics."""
    _ln_case(M, D, True)


@pytest.mark.parametrize("M,D", [(4101, 256), (12289, 768)])
def test_layernorm_bwd_xhat_past_the_row_cap(hip, M, D):
    """The assertions and bounds of test_gpu_kernels.py::test_layernorm_bwd_xhat_mode past the cap of the column-sum form."""
    from vitamd import ops
    b = Bounds()
    x = (randn((M, D), 71, 2.0) + 0.3).to(dev())
    dy = r16(randn((M, D), 72)).to(dev(), BF16)
    gres = randn((M, D), 73).to(dev())
    _, y, mean, rstd = ops.layernorm_fwd(x)
    c1, c2 = torch.zeros(D, device=dev()), torch.zeros(D, device=dev())
    g_ref, gb_ref = ops.layernorm_bwd(dy, x, mean, rstd, g_res=gres, want_bf16=True, colsum=c1)
    g, gb = ops.layernorm_bwd(dy, x, mean, rstd, g_res=gres, want_bf16=True, colsum=c2, xhat=y)
    b.lt("g vs recomputing kernel", O.rel_l2(g.cpu(), g_ref.cpu()), 7.2e-5)
    b.lt("gb vs recomputing kernel", O.rel_l2(gb.float().cpu(), gb_ref.float().cpu()), 5.3e-4)
    b.lt("colsum", O.rel_l2(c2.cpu(), gb.cpu().double().sum(0)), 1.0e-6)
    xr = x.cpu().double().requires_grad_(True)
    O.layer_norm(xr).backward(dy.cpu().double())
    b.lt("g vs float64", O.rel_l2(g.cpu(), xr.grad + gres.cpu().double()), 7.2e-5)
    b.check()


def test_layernorm_bwd_keep_form_past_the_row_cap(hip):
    """Compact g_res (the first k tokens of every sequence) at 21 x 197 = 4137 rows, against the float64 formula with a zero-expanded g_res
    (not against the full kernel): the recomputing form at the bounds of test_layernorm_fwd_bwd, the xhat form at those of the xhat test."""
    from vitamd import ops
    b = Bounds()
    B, seq, k, D = 21, 197, 5, 256
    M = B * seq
    x = (randn((M, D), 81, 2.0) + 0.5).to(dev())
    dy = r16(randn((M, D), 82)).to(dev(), BF16)
    gres_c = randn((B * k, D), 83)
    _, y, mean, rstd = ops.layernorm_fwd(x)
    xr = x.cpu().double().requires_grad_(True)
    O.layer_norm(xr).backward(dy.cpu().double())
    full = torch.zeros((B, seq, D), dtype=F64)
    full[:, :k] = gres_c.double().view(B, k, D)
    want = xr.grad + full.view(M, D)
    # xhat form: the contract stated by test_layernorm_bwd_xhat_mode is 1e-3 of the fp32 formula; its 7.2e-5 is relative to a dense g_res of
    # twice the norm of LN'(dy), which is absent from 192 of every 197 rows here
    for name, xhat, bound in (("recompute", None, 1.0e-6), ("xhat", y, 1.0e-3)):
        cs = torch.zeros(D, device=dev())
        g, gb = ops.layernorm_bwd(dy, x, mean, rstd, g_res=gres_c.to(dev()), want_bf16=True, colsum=cs, xhat=xhat, keep=(seq, k))
        b.lt(f"g {name}", O.rel_l2(g.cpu(), want), bound)
        assert torch.equal(gb.float().cpu(), r16(g.cpu()))
        b.lt(f"colsum {name}", O.rel_l2(cs.cpu(), gb.cpu().double().sum(0)), 1.0e-6)
    b.check()


# ------------------------------------------------------------------------------------------ fused AdamW
ADAMW_SHAPES = [(3072, 768), (2097152 + 1024 + 3,)]               # fc1 / fc2 of ViT-B (2 359 296 > 2048 x 256 x 4), and a ragged one with a scalar tail
ADAMW_LRS = [1e-4, 3e-4, 1e-3, 7e-4, 2e-4]                        # the scheduler changes lr between steps


@functools.lru_cache(maxsize=None)
def _adamw_inputs():
    ps = [randn(s, 90 + i) for i, s in enumerate(ADAMW_SHAPES)]
    gs = []
    for step in range(len(ADAMW_LRS)):
        row = [randn(s, 100 + 10 * step + i) for i, s in enumerate(ADAMW_SHAPES)]
        row[0][100:200] = 0.0                                     # never a gradient: v stays 0 and eps alone is the denominator
        row[1][5000:9000] = 0.0
        gs.append(row)
    return ps, gs


def _adamw_run(make, opt_cls, wd, betas):
    ps, gs = _adamw_inputs()
    params = [torch.nn.Parameter(make(p)) for p in ps]
    opt = opt_cls(params, lr=ADAMW_LRS[0], betas=betas, eps=1e-8, weight_decay=wd)
    for lr, row in zip(ADAMW_LRS, gs):
        for grp in opt.param_groups:
            grp["lr"] = lr
        for p, g in zip(params, row):
            p.grad = make(g)
        opt.step()
    return [(p.detach().cpu().double(), opt.state[p]["exp_avg"].cpu().double(), opt.state[p]["exp_avg_sq"].cpu().double()) for p in params]


@pytest.mark.parametrize("wd,betas", [(0.05, (0.9, 0.999)), (0.0, (0.9, 0.95))])       # the training scripts' defaults; the betas of test_adamw_kernel_matches_torch
def test_adamw_past_the_grid_cap(hip, wd, betas):
    """Five steps against float64 torch.optim.AdamW: p, exp_avg, exp_avg_sq and the update p - p0 each within 4 x the distance of torch's
    fp32 CPU optimiser from float64 (p never above the suite's 1e-6; p is stored in fp32, so the update inherits its rounding)."""
    from vitamd.optim import AdamW
    b = Bounds()
    ps, _ = _adamw_inputs()
    ref = _adamw_run(lambda t: t.double().clone(), torch.optim.AdamW, wd, betas)
    f32 = _adamw_run(lambda t: t.clone(), torch.optim.AdamW, wd, betas)
    got = _adamw_run(lambda t: t.clone().to(dev()), AdamW, wd, betas)
    for i, p0 in enumerate(ps):
        p0 = p0.double()
        for name, j in (("p", 0), ("exp_avg", 1), ("exp_avg_sq", 2)):
            floor = O.rel_l2(f32[i][j], ref[i][j])
            bound = min(4 * floor, 1e-6) if name == "p" else 4 * floor
            b.lt(f"{name}[{i}]", O.rel_l2(got[i][j], ref[i][j]), bound)
        floor = O.rel_l2(f32[i][0] - p0, ref[i][0] - p0)
        b.lt(f"update[{i}]", O.rel_l2(got[i][0] - p0, ref[i][0] - p0), 4 * floor)
        z = (slice(100, 200),) if i == 0 else (slice(5000, 9000),)
        assert torch.equal(got[i][2][z], torch.zeros_like(got[i][2][z])) and torch.isfinite(got[i][0][z]).all()
    b.check()


def test_adamw_refuses_a_parameter_off_the_16_byte_boundary(hip):
    from vitamd.optim import AdamW
    from vitamd.lib import VitamdError
    buf = randn((1040,), 95).to(dev())
    p = torch.nn.Parameter(buf[1:1025])                            # a view: storage starts 4 bytes off the boundary
    assert p.data_ptr() % 16 == 4 and p.is_contiguous()
    before = buf.clone()
    p.grad = randn((1024,), 96).to(dev())
    opt = AdamW([p], lr=1e-3)
    with pytest.raises(VitamdError):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# ------------------------------------------------------------------------------------------ conv3x3
@pytest.mark.parametrize("B,H,W", [(17, 256, 256), (5, 459, 457), (65, 256, 256)])
def test_conv3x3_past_the_grid_caps(hip, B, H, W):
    """Forward and input gradient cap at 4096 x 256 = 1 048 576 pixels ((17, 256, 256); (5, 459, 457) with ragged rows), the weight
    gradient at 1024 x 256 x 16 = 4 194 304 ((65, 256, 256)).  y and dx at the suite's 1e-6; dw and db at max(the suite's 2.4e-6 / 2e-5,
    4 x torch's fp32 distance from float64 at this shape)."""
    import torch.nn.functional as F
    from vitamd import ops
    b = Bounds()
    x, w, bias = randn((B, 3, H, W), 61), randn((3, 3, 3, 3), 62, 0.3), randn((3,), 63)
    dy = randn((B, 3, H, W), 64)

    def grads(dt):
        xr, wr, br = (t.to(dt).requires_grad_(True) for t in (x, w, bias))
        yr = F.conv2d(xr, wr, br, padding=1)
        return (yr.detach(),) + torch.autograd.grad((yr * dy.to(dt)).sum(), [xr, wr, br])

    yr, gx, gw, gb = grads(F64)
    _, _, gw32, gb32 = grads(F32)
    y = ops.conv3x3_fwd(x.to(dev()), w.to(dev()), bias.to(dev()))
    dx, dw, db = ops.conv3x3_bwd(x.to(dev()), w.to(dev()), dy.to(dev()))
    b.lt("y", O.rel_l2(y.cpu(), yr), 1e-6)
    b.lt("dx", O.rel_l2(dx.cpu(), gx), 1e-6)
    b.lt("dw", O.rel_l2(dw.cpu(), gw), max(2.4e-6, 4 * O.rel_l2(gw32, gw)))
    b.lt("db", O.rel_l2(db.cpu(), gb), max(2e-5, 4 * O.rel_l2(gb32, gb)))
    b.check()
