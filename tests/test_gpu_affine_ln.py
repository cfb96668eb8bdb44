"""Affine LayerNorm (csrc/layernorm_affine.hip), all four entry points against torch.nn.functional.layer_norm in float64.

The kernels are reached by the models only through the blocks.py goldens at small M; here they run past their grid caps (forward 2048
workgroups x 4 rows = 8192 rows, backward 1024 x 4 = 4096), at widths below one wave pass (D = 1, 4), ragged against the 64-lane stride
(72), equal to the non-affine kernels' (768) and at the backward's limit (4096: 3 x D floats of LDS partials), with both eps values the
models use.  dgamma / dbeta / colsum are LDS atomics folded into global atomics after the loop: they are accumulated into, so the buffers
are pre-filled.

Bounds: the ones the suite holds the same quantities of the non-affine kernel to - 1e-6 for fp32 outputs and reductions, 3e-5 for the bf16
y.  Beside every reduction the test records the distance of torch's own fp32 CPU evaluation from float64 at the same shape."""
import pytest
import torch
import torch.nn.functional as F

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

    def note(self, name, value):
        print(f"  {name}: {float(value):.3e} (for the record)")

    def check(self):
        bad = [r for r in self.rows if not r[1] < r[2]]
        assert not bad, bad


def _inputs(M, D):
    x = randn((M, D), 31, 2.0) + 0.5
    gamma = 1.0 + randn((D,), 32, 0.3)
    beta = randn((D,), 33, 0.2)
    dy = r16(randn((M, D), 34))
    return x, gamma, beta, dy


def _reference(x, gamma, beta, dy, eps, dt):
    """F.layer_norm in `dt` on the CPU -> y, mean, rstd, dx, dgamma, dbeta"""
    D = x.shape[1]
    xr, gr, br = (t.to(dt).clone().requires_grad_(True) for t in (x, gamma, beta))
    yr = F.layer_norm(xr, (D,), gr, br, eps)
    yr.backward(dy.to(dt))
    xd = xr.detach()
    mean = xd.mean(-1)
    rstd = (xd.var(-1, unbiased=False) + eps).rsqrt()
    return yr.detach(), mean, rstd, xr.grad, gr.grad, br.grad


CASES = [(1, 72), (3, 72), (4101, 72), (8197, 72), (3, 1), (3, 4), (3, 768), (3, 4096), (4101, 768)]
PRE_G, PRE_B = 0.75, -1.25                                        # dgamma / dbeta are accumulated into


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("M,D", CASES)
def test_affine_layernorm_against_float64(hip, M, D, eps):
    from vitamd import ops
    b = Bounds()
    x, gamma, beta, dy = _inputs(M, D)
    yr, mean_r, rstd_r, dx_r, dgamma_r, dbeta_r = _reference(x, gamma, beta, dy, eps, F64)
    _, _, _, _, dgamma_32, dbeta_32 = _reference(x, gamma, beta, dy, eps, F32)
    b.note("torch fp32 dgamma", O.rel_l2(dgamma_32 + PRE_G, dgamma_r + PRE_G))         # recorded beside the kernel's, not a check of the kernel
    b.note("torch fp32 dbeta", O.rel_l2(dbeta_32 + PRE_B, dbeta_r + PRE_B))
    # D = 1: xhat = 0 and dxhat equals its own mean, so the gradient is exactly zero and a relative distance from zero (float64 leaves
    # 1e-17 there) says nothing; g is then measured on top of the term that cancels in it, rstd * dy * gamma
    T = rstd_r[:, None] * dy.double() * gamma.double() if D == 1 else torch.zeros((M, D), dtype=F64)
    xd, gd, bd = x.to(dev()), gamma.to(dev()), beta.to(dev())
    # forward, bf16 and fp32 outputs
    y, mean, rstd = ops.layernorm_affine_fwd(xd, gd, bd, eps)
    b.lt("y bf16", O.rel_l2(y.float().cpu(), r16(yr)), 3e-5)
    b.lt("mean", O.rel_l2(mean.cpu(), mean_r), 1e-6)
    b.lt("rstd", O.rel_l2(rstd.cpu(), rstd_r), 1e-6)
    yf, mean_f, rstd_f = ops.layernorm_affine_fwd_f32(xd, gd, bd, eps)
    b.lt("y fp32", O.rel_l2(yf.cpu(), yr), 1e-6)
    b.lt("mean (fp32 form)", O.rel_l2(mean_f.cpu(), mean_r), 1e-6)
    b.lt("rstd (fp32 form)", O.rel_l2(rstd_f.cpu(), rstd_r), 1e-6)
    # backward from bf16 dy, no residual gradient
    dyd = dy.to(dev(), BF16)
    dgamma, dbeta = torch.full((D,), PRE_G, device=dev()), torch.full((D,), PRE_B, device=dev())
    g, none = ops.layernorm_affine_bwd(dyd, xd, mean, rstd, gd, dgamma, dbeta)
    assert none is None
    b.lt("g", O.rel_l2(g.cpu().double() + T, dx_r + T), 1e-6)
    b.lt("dgamma", O.rel_l2(dgamma.cpu(), dgamma_r + PRE_G), 1e-6)
    b.lt("dbeta", O.rel_l2(dbeta.cpu(), dbeta_r + PRE_B), 1e-6)
    # ... with the residual gradient, the bf16 copy and its column sums
    gres = randn((M, D), 35)
    dgamma, dbeta = torch.full((D,), PRE_G, device=dev()), torch.full((D,), PRE_B, device=dev())
    cs = torch.zeros(D, device=dev())
    g, gb = ops.layernorm_affine_bwd(dyd, xd, mean, rstd, gd, dgamma, dbeta, g_res=gres.to(dev()), want_bf16=True, colsum=cs)
    b.lt("g + g_res", O.rel_l2(g.cpu(), dx_r + gres.double()), 1e-6)
    assert torch.equal(gb.float().cpu(), r16(g.cpu()))
    gb64 = gb.cpu().double()
    b.note("torch fp32 colsum", O.rel_l2(gb.float().cpu().sum(0), gb64.sum(0)))
    b.lt("colsum", O.rel_l2(cs.cpu(), gb64.sum(0)), 1e-6)
    b.lt("dgamma (g_res form)", O.rel_l2(dgamma.cpu(), dgamma_r + PRE_G), 1e-6)
    b.lt("dbeta (g_res form)", O.rel_l2(dbeta.cpu(), dbeta_r + PRE_B), 1e-6)
    # backward from fp32 dy
    dgamma, dbeta = torch.full((D,), PRE_G, device=dev()), torch.full((D,), PRE_B, device=dev())
    g = ops.layernorm_affine_bwd_f32(dy.to(dev()), xd, mean_f, rstd_f, gd, dgamma, dbeta)
    b.lt("g (fp32 form)", O.rel_l2(g.cpu().double() + T, dx_r + T), 1e-6)
    b.lt("dgamma (fp32 form)", O.rel_l2(dgamma.cpu(), dgamma_r + PRE_G), 1e-6)
    b.lt("dbeta (fp32 form)", O.rel_l2(dbeta.cpu(), dbeta_r + PRE_B), 1e-6)
    b.check()


def test_affine_layernorm_dbeta_exact_on_integer_dy(hip):
    """Integer-valued dy in [-3, 3] and an integer pre-fill: every partial of dbeta is exact in fp32, so the LDS atomics of the four waves,
    the fold after the grid-stride loop and the global atomics of 1024 workgroups must give the float64 sum bit for bit."""
    from vitamd import ops
    M, D = 4101, 72
    x, gamma, beta, _ = _inputs(M, D)
    dy = ints((M, D), -3, 3, 36)
    xd, gd = x.to(dev()), gamma.to(dev())
    _, mean, rstd = ops.layernorm_affine_fwd(xd, gd, beta.to(dev()))
    want = dy.double().sum(0) + 3.0
    dgamma, dbeta = torch.zeros(D, device=dev()), torch.full((D,), 3.0, device=dev())
    ops.layernorm_affine_bwd(dy.to(dev(), BF16), xd, mean, rstd, gd, dgamma, dbeta)
    assert torch.equal(dbeta.cpu().double(), want)
    dgamma, dbeta = torch.zeros(D, device=dev()), torch.full((D,), 3.0, device=dev())
    ops.layernorm_affine_bwd_f32(dy.to(dev()), xd, mean, rstd, gd, dgamma, dbeta)
    assert torch.equal(dbeta.cpu().double(), want)


def test_affine_layernorm_width_limit(hip):
    """D = 4097: the forward has no width limit; both backward forms (3 x D floats of LDS partials, D <= 4096) refuse it and write nothing."""
    from vitamd import ops
    from vitamd.lib import VitamdError
    b = Bounds()
    M, D = 3, 4097
    x, gamma, beta, dy = _inputs(M, D)
    yr, mean_r, rstd_r, _, _, _ = _reference(x, gamma, beta, dy, 1e-5, F64)
    xd, gd, bd = x.to(dev()), gamma.to(dev()), beta.to(dev())
    y, mean, rstd = ops.layernorm_affine_fwd(xd, gd, bd)
    yf, _, _ = ops.layernorm_affine_fwd_f32(xd, gd, bd)
    b.lt("y bf16", O.rel_l2(y.float().cpu(), r16(yr)), 3e-5)
    b.lt("y fp32", O.rel_l2(yf.cpu(), yr), 1e-6)
    b.lt("mean", O.rel_l2(mean.cpu(), mean_r), 1e-6)
    b.lt("rstd", O.rel_l2(rstd.cpu(), rstd_r), 1e-6)
    b.check()
    dgamma, dbeta, cs = (torch.full((D,), v, device=dev()) for v in (PRE_G, PRE_B, 2.0))
    with pytest.raises(VitamdError):
        ops.layernorm_affine_bwd(dy.to(dev(), BF16), xd, mean, rstd, gd, dgamma, dbeta, g_res=xd, want_bf16=True, colsum=cs)
    with pytest.raises(VitamdError):
        ops.layernorm_affine_bwd_f32(dy.to(dev()), xd, mean, rstd, gd, dgamma, dbeta)
    # the C ABI with the caller's own output buffers: refused before any launch
    g = torch.full((M, D), 9.0, device=dev())
    gb = torch.full((M, D), 9.0, device=dev(), dtype=BF16)
    dyb, dyf = dy.to(dev(), BF16), dy.to(dev())
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    assert hip.vitamd_layernorm_affine_bwd(p(dyb), p(xd), p(mean), p(rstd), p(gd), p(xd), p(g), p(gb), p(cs), p(dgamma), p(dbeta), M, D, st) == 1
    assert hip.vitamd_layernorm_affine_bwd_f32(p(dyf), p(xd), p(mean), p(rstd), p(gd), p(g), p(dgamma), p(dbeta), M, D, st) == 1
    torch.cuda.synchronize()
    assert torch.all(g == 9.0) and torch.all(gb == 9.0) and torch.all(cs == 2.0)
    assert torch.all(dgamma == PRE_G) and torch.all(dbeta == PRE_B)
