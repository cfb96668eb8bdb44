"""Host-side checks of the perceptual loss (vitamd/perceptual.py, csrc/perceptual.hip): the float64 restatement of tests/_perceptual_ref.py
against torch's own float64 evaluation, the module's state-dict contract and argument handling, the C ABI's new symbols and refusals, and the
bounds of the GPU tests against planted mistakes.  No GPU is needed."""
import ctypes
import warnings

import pytest
import torch

import _abi
import _perceptual_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ERR_SHAPE, ERR_ARG = 1, 2
NEW_SYMBOLS = {"vitamd_dwconv7_fwd": 10, "vitamd_dwconv7_bwd": 10, "vitamd_resize_norm_fwd": 17, "vitamd_resize_norm_bwd": 16}
RESIZES = [(256, 224), (128, 224), (64, 224), (300, 224), (224, 224), (40, 16), (20, 16), (1, 32), (5, 32)]
SMALL = dict(depths=(1, 1, 2, 1), dims=(32, 64, 96, 128), num_classes=40, size=64)


def _quiet(**kw):
    from vitamd.perceptual import PerceptualLoss
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return PerceptualLoss(**kw)


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n_in,n_out", RESIZES)
def test_tap_tables_equal_interpolate(n_in, n_out):
    """the closed-form taps - the reference's and the module's - against F.interpolate in float64, forward and (transposed) backward; the
    band tables the kernels read hold every non-zero of the matrix and stay inside it"""
    from vitamd import perceptual as P
    g = torch.Generator().manual_seed(n_in)
    img, gout = torch.rand((1, 3, n_in, n_in), generator=g, dtype=F64), torch.randn((1, 3, n_out, n_out), generator=g, dtype=F64)
    out, dimg = R.resize_norm_torch(img, n_out, F64, gout)
    # 1e-14 where an output sums a few taps; the two extreme upsamplings sum up to 32 x 32 gradient values per pixel, in another order
    tol = 1e-14 if n_in >= 20 else 1e-12
    assert R.dist(R.resize_norm_ref(img, n_out), out) <= tol
    assert R.dist(R.resize_norm_bwd_ref(gout, n_in, n_in), dimg) <= tol
    m = P.resize_matrix(n_in, n_out)
    assert torch.equal(m, R.taps(n_in, n_out))
    for mat in (m, m.t().contiguous()):
        start, taps = P.band(mat)
        T = taps.shape[1]
        assert start.dtype == torch.int32 and taps.dtype == F32 and int(start.min()) >= 0 and int((start + T).max()) <= mat.shape[1]
        dense = torch.zeros_like(mat)
        for r in range(mat.shape[0]):
            dense[r, int(start[r]):int(start[r]) + T] = taps[r].double()
        assert float((dense - mat).abs().max()) <= 2.0 ** -24
    expect = {(256, 224): 3, (128, 224): 2, (40, 16): 5}
    if (n_in, n_out) in expect:
        assert P.band(m)[1].shape[1] == expect[(n_in, n_out)]


@pytest.mark.parametrize("shape", [(2, 2, 8), (3, 5, 96), (9, 17, 68)])
def test_dwconv_restatement_equals_torch(shape):
    H, W, C = shape
    g = torch.Generator().manual_seed(C)
    x, dy = torch.randn((2, H, W, C), generator=g, dtype=F64), torch.randn((2, H, W, C), generator=g, dtype=F64)
    w, b = torch.randn((C, 7, 7), generator=g, dtype=F64), torch.randn((C,), generator=g, dtype=F64)
    y, dx = R.dwconv_torch(x, w, b, dy)
    assert R.dist(R.dwconv_ref(x, w, b), y) <= 1e-13 and R.dist(R.dwconv_bwd_ref(dy, w), dx) <= 1e-13


@pytest.fixture(scope="module")
def small():
    sd = R.random_state(SMALL["depths"], SMALL["dims"], SMALL["num_classes"], 0)
    inp, tgt = R.images(2, 72, 72, 100)
    loss, grad = R.loss_and_grad(sd, inp, tgt, SMALL["depths"], SMALL["size"])
    return sd, inp, tgt, loss, grad


def test_network_restatement_equals_torch(small):
    sd, inp, tgt, loss, grad = small
    l_t, g_t = R.loss_and_grad(sd, inp, tgt, SMALL["depths"], SMALL["size"], how="torch")
    assert R.rel(l_t, loss) <= 1e-12 and float((g_t - grad).norm() / grad.norm()) <= 1e-12
    assert float(grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------ the module
def test_default_module_has_torchvisions_layout():
    from vitamd.perceptual import PerceptualLoss
    with pytest.warns(UserWarning, match="stand-in") as rec:
        m = PerceptualLoss()
    assert len([w for w in rec if "stand-in" in str(w.message)]) == 1
    sd = m.state_dict()
    expect = R.keys((3, 3, 27, 3), (96, 192, 384, 768), 1000)
    assert len(expect) == 344 and len(sd) == 344 + 2
    assert {k: tuple(v.shape) for k, v in sd.items() if k.startswith("convnext.")} == {"convnext." + k: v for k, v in expect.items()}
    assert tuple(sd["imagenet_mean"].shape) == tuple(sd["imagenet_std"].shape) == (1, 3, 1, 1)
    assert torch.allclose(sd["imagenet_mean"].flatten(), torch.tensor(R.MEAN)) and torch.allclose(sd["imagenet_std"].flatten(), torch.tensor(R.STD))
    assert sum(p.numel() for p in m.parameters()) == 50_223_688
    assert all(not p.requires_grad for p in m.parameters()) and not m.training
    assert not m.train().training                                  # always in eval mode
    # torchvision's initialisation
    assert float(sd["convnext.features.1.0.layer_scale"].max()) == pytest.approx(1e-6) and float(sd["convnext.features.1.0.block.3.bias"].abs().max()) == 0
    w = sd["convnext.features.5.3.block.3.weight"]
    assert float(w.abs().max()) <= 2.0 and 0.018 < float(w.std()) < 0.022
    assert torch.equal(sd["convnext.classifier.0.weight"], torch.ones(768))


def test_weights_and_arguments(tmp_path):
    from vitamd.perceptual import PerceptualLoss
    sd = R.random_state(SMALL["depths"], SMALL["dims"], SMALL["num_classes"], 3)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        a = PerceptualLoss(weights=sd, **SMALL)                    # torchvision's own keys, no prefix
        b = PerceptualLoss(weights={"convnext." + k: v for k, v in sd.items()}, **SMALL)
        path = str(tmp_path / "w.pt")
        torch.save(b.state_dict(), path)
        c = PerceptualLoss("convnext_s_anything", weights=path, **SMALL)
    assert not [w for w in seen if "stand-in" in str(w.message)]
    for m in (a, b, c):
        got = m.state_dict()
        assert all(torch.equal(got["convnext." + k], v) for k, v in sd.items()) and all(not p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError):
        PerceptualLoss("vgg16")
    with pytest.raises(ValueError):
        _quiet(size=100)
    with pytest.raises(RuntimeError):
        _quiet(weights={k: v for k, v in sd.items() if "layer_scale" not in k}, **SMALL)


# ------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_bound_with_the_headers_arity():
    from vitamd import lib
    L = lib.load()
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    for name, nargs in NEW_SYMBOLS.items():
        fn = getattr(L, name)
        assert len(lib.SIGNATURES[name]) == nargs and fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
        assert _abi.declared()[1][name] == "int" and len(_abi.declaration(name).split(",")) == nargs, name


def test_entry_points_refuse_before_any_launch():
    """null pointers everywhere: a shape error is reported first, valid numbers then give the argument error; nothing is launched"""
    from vitamd import lib
    L = lib.load()
    for fn in (L.vitamd_dwconv7_fwd, L.vitamd_dwconv7_bwd):
        for B, H, W, C in ((0, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 6), (1, 4, 4, 0)):
            assert fn(None, 0, None, None, None, B, H, W, C, None) == ERR_SHAPE
        assert fn(None, 0, None, None, None, 2, 4, 4, 8, None) == ERR_ARG
    rf = lambda B, C, H, W, S, Th=1, Tw=1: L.vitamd_resize_norm_fwd(None, None, None, Th, None, None, Tw, None, None, None, None, B, C, H, W, S, None)
    rb = lambda B, C, H, W, S, Th=1, Tw=1, ld=64: L.vitamd_resize_norm_bwd(None, ld, None, None, Th, None, None, Tw, None, None, B, C, H, W, S, None)
    for f in (rf, rb):
        assert f(0, 3, 8, 8, 16) == ERR_SHAPE and f(1, 4, 8, 8, 16) == ERR_SHAPE and f(1, 3, 8, 8, 18) == ERR_SHAPE and f(1, 3, 0, 8, 16) == ERR_SHAPE
        assert f(1, 3, 8, 8, 16, Th=0) == ERR_SHAPE and f(1, 3, 8, 8, 16) == ERR_ARG
    assert rf(1, 3, 8, 8, 16, Th=9) == ERR_SHAPE and rb(1, 3, 8, 8, 16, Tw=17) == ERR_SHAPE         # a band longer than the axis it reads
    assert rb(1, 3, 8, 8, 16, ld=40) == ERR_SHAPE


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    from vitamd import ops
    from vitamd.lib import VitamdError
    x, w = torch.randn(2, 4, 4, 8), torch.randn(8, 7, 7)
    img = torch.rand(2, 3, 8, 8)
    tab = (torch.zeros(16, dtype=torch.int32), torch.ones(16, 1))
    with pytest.raises(ValueError):
        ops.dwconv7_fwd(torch.randn(2, 4, 4, 6), torch.randn(6, 7, 7))       # C % 4: before any device is looked at
    with pytest.raises(ValueError):
        ops.dwconv7_bwd(x, torch.randn(8, 3, 3))
    with pytest.raises(ValueError):
        ops.resize_norm_fwd(torch.rand(2, 4, 8, 8), tab, tab, torch.zeros(3), torch.ones(3), 16)
    with pytest.raises(ValueError):
        ops.resize_norm_fwd(img, tab, tab, torch.zeros(3), torch.ones(3), 18)
    with pytest.raises(ValueError):
        ops.resize_norm_bwd(torch.randn(30, 64), tab, tab, torch.ones(3), 2, 8, 8, 16)
    for call in (lambda: ops.dwconv7_fwd(x, w),
                 lambda: ops.dwconv7_fwd(x.double(), w),
                 lambda: ops.dwconv7_fwd(x.permute(0, 2, 1, 3), w),
                 lambda: ops.dwconv7_bwd(x, w, add=x),
                 lambda: ops.resize_norm_fwd(img, tab, tab, torch.zeros(3), torch.ones(3), 16),
                 lambda: ops.resize_norm_bwd(torch.randn(32, 64), tab, tab, torch.ones(3), 2, 8, 8, 16),
                 lambda: _quiet(**SMALL)(img, img)):
        with pytest.raises(VitamdError):
            call()


# ------------------------------------------------------------------------------------------ planted mistakes
def test_kernel_bounds_catch_planted_mistakes():
    """every mistake's float64 distance from the reference exceeds the bound the GPU test applies (4 x torch's fp32 figure, floor 8 * 2^-24;
    + half a bf16 ulp for the bf16 rows of the resize)"""
    g = torch.Generator().manual_seed(0)
    H, W, C = 9, 12, 8
    x, dy = torch.randn((2, H, W, C), generator=g), torch.randn((2, H, W, C), generator=g)
    w, b = torch.randn((C, 7, 7), generator=g) / 7, torch.randn((C,), generator=g)
    t_y, t_dx = R.dwconv_torch(x, w, b, dy, F32)
    ref_y, ref_dx = R.dwconv_ref(x, w, b), R.dwconv_bwd_ref(dy, w)
    b_y, b_dx = R.bound(R.dist(t_y, ref_y)), R.bound(R.dist(t_dx, ref_dx))
    assert b_y < 1e-5 and b_dx < 1e-5
    for bug in ("clamp_border", "no_bias", "shift"):
        assert R.dist(R.dwconv_ref(x, w, b, bug), ref_y) > b_y, bug
    for bug in ("no_flip", "clamp_border", "shift"):
        assert R.dist(R.dwconv_bwd_ref(dy, w, bug), ref_dx) > b_dx, bug
    # resize: the downscale 40 -> 16 for the forward mistakes; 16 -> 16 lets the untransposed tables fit a square matrix, so take 20 -> 16
    # transposed by hand for that one
    img, gout = torch.rand((2, 3, 40, 40), generator=g), torch.randn((2, 3, 16, 16), generator=g)
    t_out, t_dimg = R.resize_norm_torch(img, 16, F32, gout)
    ref, ref_d = R.resize_norm_ref(img, 16), R.resize_norm_bwd_ref(gout, 40, 40)
    b_f, b_b = R.bound(R.dist(t_out, ref), bf16_out=True), R.bound(R.dist(t_dimg, ref_d))
    assert b_f < 5e-3 and b_b < 1e-5
    for bug in ("no_antialias", "align_corners", "no_renorm"):
        assert R.dist(R.resize_norm_ref(img, 16, bug), ref) > b_f, bug
    assert R.dist(R.resize_norm_bwd_ref(gout, 40, 40, "no_std"), ref_d) > b_b
    sq = torch.randn((2, 3, 16, 16), generator=g)                   # a non-symmetric square matrix: 16 -> 16 is the identity, so use the
    m = R.taps(20, 16)[:, :16]                                      # 16 x 16 corner of the 20 -> 16 matrix
    right, wrong = torch.einsum("oh,bcop,pw->bchw", m, sq.double(), m), torch.einsum("ho,bcop,wp->bchw", m, sq.double(), m)
    assert R.dist(wrong, right) > b_b


def test_network_bounds_catch_planted_mistakes(small):
    """each mistake moves loss AND gradient beyond the fp32 bound (4 x torch's fp32 figure, floor 8 * 2^-24), and fails the GPU test, which
    asserts both figures against 2 x floor + 1e-3 with the floor of torch's bf16-autocast evaluation at the same weights and inputs"""
    sd, inp, tgt, loss, grad = small
    rel_l2 = lambda g: float((g.double() - grad).norm() / grad.norm())
    l32, g32 = R.loss_and_grad(sd, inp, tgt, SMALL["depths"], SMALL["size"], how="torch", dtype=F32)
    l16, g16 = R.loss_and_grad(sd, inp, tgt, SMALL["depths"], SMALL["size"], how="torch", dtype=F32, autocast=True)
    b32_loss, b32_grad = R.bound(R.rel(l32, loss)), R.bound(rel_l2(g32))
    f_loss, f_grad = R.rel(l16, loss), rel_l2(g16)
    print(f"fp32 bounds: loss {b32_loss:.3e} gradient {b32_grad:.3e}; bf16 floors: loss {f_loss:.3e} gradient {f_grad:.3e}")
    assert b32_loss < 1e-4 and b32_grad < 1e-4
    assert 1e-5 < f_loss < 5e-2 and 1e-3 < f_grad < 1e-1            # a bf16 flow: neither exact nor broken
    for bug in R.NET_BUGS:
        l, g = R.loss_and_grad(sd, inp, tgt, SMALL["depths"], SMALL["size"], bug=bug)
        e_loss, e_grad = R.rel(l, loss), rel_l2(g)
        print(f"{bug}: loss {e_loss:.3e} gradient {e_grad:.3e}")
        assert e_loss > b32_loss and e_grad > b32_grad, bug
        assert e_loss > 2 * f_loss + 1e-3 or e_grad > 2 * f_grad + 1e-3, bug


# ------------------------------------------------------------------------------------------ the training scripts
def test_training_scripts_take_the_perceptual_arguments():
    import inspect
    import train_titok as TT
    import train_vit_vqgan as TQ
    for mod in (TT, TQ):
        args = mod.parse_args([])
        assert args.perceptual_weight == 0.0 and args.perceptual_weights is None
        args = mod.parse_args(["--perceptual_weight", "0.5", "--perceptual_weights", "w.pt"])
        assert args.perceptual_weight == 0.5 and args.perceptual_weights == "w.pt"
        assert list(inspect.signature(mod.train_step).parameters) == ["model", "images", "optim", "lr_sched", "perceptual", "perceptual_weight"]
    assert TT.make_perceptual(TT.parse_args([])) is None
