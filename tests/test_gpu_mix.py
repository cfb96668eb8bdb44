"""Mixup / CutMix / label smoothing on the GPU (csrc/input.hip vitamd_frames_prep_mix, csrc/loss.hip vitamd_soft_cross_entropy_*,
vitamd/mix.py) against tests/_mix_ref.py.

The prep comparisons are exact: a mixed pixel is a table lookup, three rounded fp32 operations or a select, and its patch row is the bf16
ops.im2col makes of it.  The loss is held to _lm_ref.bound (max(4 x torch fp32's own distance from float64 at the shape, the floor)),
bf16 gradients to _lm_ref.check_bf16_grad's rule, and at smoothing 0 without lam to the bits of the hard-label kernels.

Shapes: the geometry family of test_gpu_data.py (39-byte source rows; C = 3 p = 4 fast, C = 1 p = 2 / C = 3 p = 2 / C = 4 p = 4 generic,
37 x 41 -> 32 x 32 at p = 16) with B = 3 (the middle sample is its own partner) and B = 4 (repeated, out-of-order frames), one sample of
each pair flipped; V in {2, 1001, 4104} (the element tail, one wave per row, four waves per row) with M in {1, 5} and one M past the
grid cap; one prep case past the grid cap."""
import functools
import time

import pytest
import torch

import _data_ref as D
import _mix_ref as R
import _poison as P
import weights as Wt
from test_gpu_data import GUARD, _Alarm, _guarded, _same, _table

pytestmark = pytest.mark.gpu
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
G_UP = 0.5


# ---------------------------------------------------------------------------------------------- prep
@functools.lru_cache(maxsize=None)
def _prep_case(geom_name, B, rec_name):
    """(src, index, geom, rec, lam, the CPU reference image); computed once, never written to"""
    Nsrc, Hs, Ws, C, H, W, p = R.GEOMS[geom_name]
    src, index, geom = R.frames_case(geom_name, B)
    rec, lam = R.record(rec_name, B, H, W)
    return src, index, geom, rec, lam, R.mixed_frames_ref(src, (H, W), index, geom, rec, lam, R.MEAN[:C], R.STD[:C])


def _run_raw(hip, src, table, index, geom, rec, lam, B, H, W, p, want_patches=True, want_image=True):
    """the C entry on guarded outputs (rec None: vitamd_frames_prep) -> (patches or None, image or None), with the guards checked"""
    from vitamd import lib
    Nsrc, Hs, Ws, C = src.shape
    pw = iw = pm = im = None
    if want_patches:
        pw, pm = _guarded(B * C * H * W, BF16)
    if want_image:
        iw, im = _guarded(B * C * H * W, F32)
    ptr = lambda t: None if t is None else t.data_ptr()
    args = (src.data_ptr(), ptr(index), ptr(geom), table.data_ptr(), ptr(pm), ptr(im), B, Nsrc, Hs, Ws, C, H, W, p)
    stream = torch.cuda.current_stream().cuda_stream
    if rec is None:
        lib.check(hip.vitamd_frames_prep(*args, stream), "frames_prep")
    else:
        lib.check(hip.vitamd_frames_prep_mix(*args, rec.data_ptr(), ptr(lam), stream), "frames_prep_mix")
    torch.cuda.synchronize()
    for whole in (pw, iw):
        if whole is not None:
            assert bool((whole[:GUARD] == 7).all()) and bool((whole[-GUARD:] == 7).all()), "a guard was written"
    return (pm.view(B * (H // p) * (W // p), C * p * p).clone() if want_patches else None, im.view(B, C, H, W).clone() if want_image else None)


def _dev_case(geom_name, B, rec_name):
    src, index, geom, rec, lam, ref = _prep_case(geom_name, B, rec_name)
    return src.cuda(), torch.tensor(index, device="cuda"), geom.cuda(), rec.cuda(), lam.cuda(), ref


@pytest.mark.parametrize("rec_name", R.RECORDS)
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("geom_name", list(R.GEOMS))
def test_prep_mix_equals_the_cpu_reference_and_im2col(hip, geom_name, B, rec_name):
    from vitamd import ops
    Nsrc, Hs, Ws, C, H, W, p = R.GEOMS[geom_name]
    src, index, geom, rec, lam, ref = _dev_case(geom_name, B, rec_name)
    patches, image = _run_raw(hip, src, _table(C), index, geom, rec, lam, B, H, W, p)
    assert _same(image, ref)
    assert _same(patches, ops.im2col(ref.cuda(), p))                  # the rows the unfused route makes of the mixed image
    assert _same(patches, D.patch_rows(ref, p).to(BF16))
    plain_p, plain_i = _run_raw(hip, src, _table(C), index, geom, None, None, B, H, W, p)
    if rec_name == "none":                                            # all mode 0: the bits of vitamd_frames_prep
        assert _same(image, plain_i) and _same(patches, plain_p)
    if B == 3:                                                        # its own partner: the plain prep, whatever the mode
        assert _same(image[1], plain_i[1])
    if rec_name == "mixup":                                           # NULL lam is l = 1 ...
        _, one = _run_raw(hip, src, _table(C), index, geom, rec, None, B, H, W, p, want_patches=False)
        ones = R.mixed_frames_ref(_prep_case(geom_name, B, rec_name)[0], (H, W), index.tolist(), geom.cpu(), rec.cpu(), torch.ones(B),
                                  R.MEAN[:C], R.STD[:C])
        assert _same(one, ones)
    if rec_name in ("cut_a", "cut_b"):                                # ... and mode 2 does not read it
        _, cut = _run_raw(hip, src, _table(C), index, geom, rec, None, B, H, W, p, want_patches=False)
        assert _same(cut, ref)


@pytest.mark.parametrize("outputs", ["image", "patches"])
@pytest.mark.parametrize("geom_name", ["fast_p4", "generic_c3_p2", "fast_p16"])
def test_prep_mix_with_one_output(hip, geom_name, outputs):
    Nsrc, Hs, Ws, C, H, W, p = R.GEOMS[geom_name]
    src, index, geom, rec, lam, ref = _dev_case(geom_name, 4, "mixed")
    patches, image = _run_raw(hip, src, _table(C), index, geom, rec, lam, 4, H, W, p, outputs == "patches", outputs == "image")
    if outputs == "image":
        assert patches is None and _same(image, ref)
    else:
        assert image is None and _same(patches, D.patch_rows(ref, p).to(BF16))


@pytest.mark.parametrize("rec_name", ["mixup", "cut_a", "mixed"])
def test_prep_mix_from_an_odd_base_address(hip, rec_name):
    """a source that starts at an odd address takes the byte-load path of the fast form for both samples of a pair"""
    Nsrc, Hs, Ws, C, H, W, p = R.GEOMS["fast_p4"]
    src, index, geom, rec, lam, ref = _dev_case("fast_p4", 4, rec_name)
    store = torch.empty(src.numel() + 1, dtype=U8, device="cuda")
    shifted = store[1:].view(src.shape)
    shifted.copy_(src)
    assert shifted.data_ptr() % 2 == 1
    patches, image = _run_raw(hip, shifted, _table(C), index, geom, rec, lam, 4, H, W, p)
    assert _same(image, ref) and _same(patches, D.patch_rows(ref, p).to(BF16))


@pytest.mark.parametrize("geom_name", ["fast_p4", "generic_c3_p2", "fast_p16"])
def test_a_wild_record_gives_what_the_tame_record_it_clamps_to_gives(hip, geom_name):
    Nsrc, Hs, Ws, C, H, W, p = R.GEOMS[geom_name]
    B = 4
    src, index, geom = R.frames_case(geom_name, B)
    lo, hi = R.I32_MIN, R.I32_MAX
    wild = torch.tensor([[B + 5, 1, lo, hi, hi, lo], [-3, 2, lo, hi, lo, hi], [1, 7, 0, H, 0, W], [0, 2, 2, hi, lo, 5]], dtype=torch.int32)
    tame = torch.tensor([[B - 1, 1, 0, H, W, 0], [0, 2, 0, H, 0, W], [1, 0, 0, H, 0, W], [0, 2, 2, H, 0, 5]], dtype=torch.int32)
    lam = torch.tensor([0.3, 0.5, 0.25, 0.75])
    assert R.clamp_rec(wild, B, H, W) == R.clamp_rec(tame, B, H, W) == [tuple(r) for r in tame.tolist()]
    ref = R.mixed_frames_ref(src, (H, W), index, geom, tame, lam, R.MEAN[:C], R.STD[:C])
    it = torch.tensor(index, device="cuda")
    got_w = _run_raw(hip, src.cuda(), _table(C), it, geom.cuda(), wild.cuda(), lam.cuda(), B, H, W, p)
    got_t = _run_raw(hip, src.cuda(), _table(C), it, geom.cuda(), tame.cuda(), lam.cuda(), B, H, W, p)
    assert _same(got_w[1], ref) and _same(got_t[1], ref)
    assert _same(got_w[0], got_t[0]) and _same(got_w[0], D.patch_rows(ref, p).to(BF16))
    # own partner after the clamp: partner -3 and B + 5 at the two ends
    ends = torch.tensor([[-3, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0], [B + 5, 2, 0, H, 0, W]], dtype=torch.int32)
    _, image = _run_raw(hip, src.cuda(), _table(C), it, geom.cuda(), ends.cuda(), lam.cuda(), B, H, W, p, want_patches=False)
    assert _same(image, D.frames_ref(src, (H, W), index, geom, R.MEAN[:C], R.STD[:C]))


def test_prep_mix_past_the_grid_cap(hip):
    """more 4-pixel groups than cap * 256 lanes cover in one pass: 40 samples of 232 x 232 from 5 frames of 233 x 235, mixed per sample
    by the host draw; the generic form (p = 2) then has twelve times the items"""
    from vitamd import mix, ops
    B, H, W, p = 40, 232, 232, 8
    assert B * H * (W // 4) > ops.frames_prep_grid_cap() * 256
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, 256, (5, 233, 235, 3), generator=g, dtype=U8)
    index = torch.randint(0, 5, (B,), generator=g)
    geom = torch.stack([torch.randint(0, 2, (B,), generator=g), torch.randint(0, 4, (B,), generator=g), torch.randint(0, 2, (B,), generator=g)], 1).int()
    rec, lam = mix.Mix(per_sample=True, prob=0.9, seed=3).draw(B, (H, W), 0)
    assert {0, 1, 2} == set(rec[:, 1].tolist())
    base = D.frames_ref_tv(src, (H, W), index.tolist(), geom, R.MEAN[:3], R.STD[:3])
    ref = R.mixed_frames_ref(src, (H, W), index.tolist(), geom, rec, lam, R.MEAN[:3], R.STD[:3], base=base)
    f = mix.MixedFrames(src.cuda(), (H, W), index=index.cuda(), geom=geom.cuda(), table=_table(3), mix=(rec.cuda(), lam.cuda()))
    f.materialise(p, image=True)
    assert _same(f.images(), ref)
    assert _same(f.patches(p), ops.im2col(ref.cuda(), p))
    assert _same(f.patches(2), ops.im2col(ref.cuda(), 2))


# ---------------------------------------------------------------------------------------------- soft-target cross-entropy
def _grid_rows(V):
    from vitamd import ops
    return ops.cross_entropy_grid_rows(V)


# (M, V, ld, dtype); M = None: one row more than a sweep of the capped grid covers at V = 2, plus a ragged remainder
CE_SHAPES = [(1, 2, 2, F32), (5, 2, 2, BF16), (1, 1001, 1001, F32), (5, 1001, 1008, F32), (5, 1001, 1008, BF16), (1, 4104, 4104, BF16),
             (5, 4104, 4104, F32), (5, 4104, 4112, BF16), (None, 2, 2, F32)]
SOFTS = ["plain", "smooth", "pair", "pair_smooth"]


@functools.lru_cache(maxsize=None)
def _ce_case(idx, soft):
    """inputs (a view of a buffer whose other columns hold NaN), the float64 reference and torch's fp32 CPU evaluation; computed once"""
    M, V, ld, dtype = CE_SHAPES[idx]
    M = _grid_rows(2) + 3 if M is None else M
    x, ya, yb, lam = R.ce_case(M, V, seed=idx, bf16=dtype == BF16)
    buf = torch.full((M, ld), float("nan"), dtype=dtype)
    buf[:, :V] = x
    kw = dict(smoothing=0.1 if "smooth" in soft else 0.0, grad_out=G_UP)
    if "pair" in soft:
        kw.update(yb=yb, lam=lam)
    return {"buf": buf, "ya": ya, "yb": yb, "lam": lam, "kw": kw, "ref": R.soft_ce_ref(buf[:, :V], ya, **kw),
            "t32": R.soft_ce_torch32(buf[:, :V], ya, **kw), "shape": (M, V, ld, dtype)}


def _soft_arg(c):
    """the `soft` argument of ops.cross_entropy_fwd / _bwd for a case, on the device"""
    kw = c["kw"]
    return (c["yb"].cuda(), c["lam"].cuda(), kw["smoothing"]) if "lam" in kw else (None, None, kw["smoothing"])


@pytest.mark.parametrize("soft", SOFTS)
@pytest.mark.parametrize("idx", range(len(CE_SHAPES)))
def test_soft_cross_entropy_kernels_match_float64(hip, idx, soft):
    from vitamd import ops
    c = _ce_case(idx, soft)
    M, V, ld, dtype = c["shape"]
    buf = c["buf"].cuda()
    x, ya, sa = buf[:, :V], c["ya"].cuda(), _soft_arg(c)
    loss_row, lse, stats = ops.cross_entropy_fwd(x, ya, soft=sa)
    gup = torch.tensor(G_UP, device="cuda")
    SENT = 7.0
    outs = {}
    for od in (F32, BF16):
        obuf = torch.full((M, ld), SENT, dtype=od, device="cuda")
        ops.cross_entropy_bwd(x, ya, lse, stats, gup, out=obuf[:, :V], soft=sa)
        outs[od] = obuf.cpu()
    torch.cuda.synchronize()
    assert abs(float(stats[1]) * M - 1) < 1e-6
    got = {"loss_row": loss_row.cpu(), "lse": lse.cpu(), "mean": stats[0].cpu(), "grad": outs[F32][:, :V]}
    fails = R.check_cross_entropy(got, c["ref"], c["t32"], f"case {c['shape']} {soft}")
    fails += R.check_bf16_grad(outs[BF16][:, :V], c["ref"], c["t32"], f"case {c['shape']} {soft}")
    assert not fails, fails
    if ld > V:                                                        # the pad columns: NaN still on the input, the sentinel on both outputs
        assert bool(torch.isnan(buf.cpu()[:, V:]).all())
        assert bool((outs[F32][:, V:] == SENT).all()) and bool((outs[BF16][:, V:] == SENT).all())
    # twice the same bits, and the backward in place
    again = ops.cross_entropy_fwd(x, ya, soft=sa)
    for u, v in zip((loss_row, lse, stats), again):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    d1 = ops.cross_entropy_bwd(x, ya, lse, stats, gup, soft=sa)
    assert d1.dtype == dtype and _same(d1, outs[dtype][:, :V].contiguous())
    buf2 = buf.clone()
    x2 = buf2[:, :V]
    d2 = ops.cross_entropy_bwd(x2, ya, lse, stats, gup, out=x2, soft=sa)
    assert d2.data_ptr() == x2.data_ptr() and _same(x2.contiguous(), d1)
    if ld > V:
        assert bool(torch.isnan(buf2.cpu()[:, V:]).all())


@pytest.mark.parametrize("idx", range(len(CE_SHAPES)))
def test_smoothing_zero_without_lam_has_the_bits_of_the_hard_label_kernels(hip, idx):
    from vitamd import ops
    c = _ce_case(idx, "plain")
    M, V, ld, dtype = c["shape"]
    buf = c["buf"].cuda()
    x, ya = buf[:, :V], c["ya"].cuda()
    gup = torch.tensor(G_UP, device="cuda")
    hard = ops.cross_entropy_fwd(x, ya)                               # no target is the ignore_index: no row ignored
    soft = ops.cross_entropy_fwd(x, ya, soft=(None, None, 0.0))
    for h, s in zip(hard, soft):
        assert _same(h, s)
    for od in (F32, BF16):
        dh = ops.cross_entropy_bwd(x, ya, hard[1], hard[2], gup, out_dtype=od)
        ds = ops.cross_entropy_bwd(x, ya, soft[1], soft[2], gup, out_dtype=od, soft=(None, None, 0.0))
        assert _same(dh, ds)
    # lam = 1 with any target_b, and ya == yb with any lam, fold to the same target: the loss within the bound of the hard reference
    ones = ops.cross_entropy_fwd(x, ya, soft=(c["yb"].cuda(), torch.ones(M, device="cuda"), 0.0))
    same = ops.cross_entropy_fwd(x, ya, soft=(ya, c["lam"].cuda(), 0.0))
    for got in (ones, same):
        fails = R.check_cross_entropy({"loss_row": got[0].cpu(), "lse": got[1].cpu(), "mean": got[2][0].cpu()}, c["ref"], c["t32"], "folded")
        assert not fails, fails


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_minus_infinity_logits_are_legal_without_smoothing(hip, dtype):
    from vitamd import ops
    M, V = 5, 1001
    x, ya, yb, lam = R.ce_case(M, V, seed=77, bf16=dtype == BF16)
    x = x.clone()
    x[:, 200:500] = float("-inf")
    x[torch.arange(M), ya] = 1.0                                      # the targets that carry weight stay finite
    live = lam != 1
    x[torch.arange(M)[live], yb[live]] = -1.0
    x[3, yb[3]] = float("-inf")                                       # row 3: lam = 1, so yb's term is not formed
    assert float(lam[3]) == 1.0 and int(ya[3]) != int(yb[3])
    kw = dict(yb=yb, lam=lam, smoothing=0.0, grad_out=G_UP)
    ref, t32 = R.soft_ce_ref(x, ya, **kw), R.soft_ce_torch32(x, ya, **kw)
    assert all(bool(torch.isfinite(ref[k]).all()) for k in ("loss_row", "lse", "mean", "grad"))
    xd = x.cuda()
    sa = (yb.cuda(), lam.cuda(), 0.0)
    loss_row, lse, stats = ops.cross_entropy_fwd(xd, ya.cuda(), soft=sa)
    d = ops.cross_entropy_bwd(xd, ya.cuda(), lse, stats, torch.tensor(G_UP, device="cuda"), out_dtype=F32, soft=sa)
    got = {"loss_row": loss_row.cpu(), "lse": lse.cpu(), "mean": stats[0].cpu(), "grad": d.cpu()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert not R.check_cross_entropy(got, ref, t32, f"-inf {dtype}")
    assert bool((got["grad"][:, 200:500] == 0).all())


def test_out_of_range_targets_give_nan_rows_zero_gradients_and_a_nan_mean(hip):
    from vitamd import ops
    M, V = 5, 1001
    x, ya, yb, lam = R.ce_case(M, V, seed=78)
    bad_a, bad_b = ya.clone(), yb.clone()
    bad_a[1], bad_b[3], bad_b[4] = V, -1, 1 << 40
    xd, gup = x.cuda(), torch.tensor(G_UP, device="cuda")
    sa = (bad_b.cuda(), lam.cuda(), 0.1)
    loss_row, lse, stats = ops.cross_entropy_fwd(xd, bad_a.cuda(), soft=sa)
    d = ops.cross_entropy_bwd(xd, bad_a.cuda(), lse, stats, gup, soft=sa)
    for r in (1, 3, 4):
        assert bool(torch.isnan(loss_row[r])) and bool((d[r] == 0).all())
    assert bool(torch.isnan(stats[0])) and abs(float(stats[1]) * M - 1) < 1e-6
    ref, t32 = R.soft_ce_ref(x, ya, yb, lam, 0.1, G_UP), R.soft_ce_torch32(x, ya, yb, lam, 0.1, G_UP)
    keep = torch.tensor([0, 2])
    sub = lambda dct: {k: (v[keep] if k in ("loss_row", "lse", "grad") else v) for k, v in dct.items() if k != "mean"}
    got = {"loss_row": loss_row.cpu()[keep], "lse": lse.cpu()[keep], "grad": d.cpu()[keep]}
    assert not R.check_cross_entropy(got, sub(ref), sub(t32), "bad targets")
    # without lam target_b is not looked at: the same wild yb, and None
    for tb in (bad_b.cuda(), None):
        lr = ops.cross_entropy_fwd(xd, ya.cuda(), soft=(tb, None, 0.1))[0]
        assert bool(torch.isfinite(lr).all())


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_lm_soft_cross_entropy_matches_the_torch_expression(hip, dtype):
    from vitamd import lm
    M, V = 64, 1000
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(4, 16, V, generator=g) * 3).to(dtype)
    ya, yb = torch.randint(0, V, (4, 16), generator=g), torch.randint(0, V, (4, 16), generator=g)
    lam = torch.rand(4, 16, generator=g)
    ref = R.soft_ce_ref(x.reshape(M, V), ya.reshape(M), yb.reshape(M), lam.reshape(M), 0.1, G_UP)
    t32 = R.soft_ce_torch32(x.reshape(M, V), ya.reshape(M), yb.reshape(M), lam.reshape(M), 0.1, G_UP)
    xd = x.cuda().requires_grad_(True)
    loss = lm.soft_cross_entropy(xd, ya.cuda(), yb.cuda(), lam.cuda(), 0.1)
    assert loss.dim() == 0 and loss.dtype == F32
    (loss * G_UP).backward()
    assert xd.grad.dtype == dtype and xd.grad.shape == x.shape
    got = {"mean": loss.detach().cpu()}
    if dtype == F32:
        got["grad"] = xd.grad.cpu().reshape(M, V)
    fails = R.check_cross_entropy(got, ref, t32, f"lm.soft_cross_entropy {dtype}")
    if dtype == BF16:
        fails += R.check_bf16_grad(xd.grad.cpu().reshape(M, V), ref, t32, "lm.soft_cross_entropy")
    assert not fails, fails
    # the expression a user would write, on the device: each fp32 evaluation may be bound() from float64, so twice that apart
    t = R.soft_target(V, ya.reshape(M), yb.reshape(M), lam.reshape(M), 0.1, F32).cuda()
    loss_t = (-t * torch.log_softmax(x.cuda().float().reshape(M, V), dim=-1)).sum(-1).mean()
    e32 = R.cross_entropy_errors(t32, ref)
    assert abs(float(loss.detach()) - float(loss_t)) <= 2 * R.bound(e32["mean"]) * max(1.0, abs(float(ref["mean"])))
    # labels alone: smoothing on an int64 tensor
    plain = lm.soft_cross_entropy(x.cuda(), ya.cuda(), smoothing=0.1)
    ref_p, t32_p = R.soft_ce_ref(x.reshape(M, V), ya.reshape(M), smoothing=0.1), R.soft_ce_torch32(x.reshape(M, V), ya.reshape(M), smoothing=0.1)
    assert not R.check_cross_entropy({"mean": plain.detach().cpu()}, ref_p, t32_p, "smoothing only")


# ---------------------------------------------------------------------------------------------- through the stack
def _model():
    import train_vit as TV
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    model = TV.ViTClassifier(cfg, num_classes=10)
    model.load_state_dict(Wt.classifier_state(3, 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, 10))
    return TV, model.cuda()


def test_classifier_on_mixed_frames_equals_classifier_on_the_mixed_images(hip):
    """the pattern of test_gpu_data.test_classifier_on_frames_equals_classifier_on_their_images: MixedFrames against the fp32
    mixed_frames_ref batch"""
    import vit_oracle as O
    from vitamd import mix
    TV, model = _model()
    labels = Wt.randint(3, "labels", (4,), 10).cuda()
    src, index, geom, rec, lam, ref = _prep_case("fast_p16", 4, "mixed")
    table = _table(3)

    def run(x):
        model.zero_grad(set_to_none=True)
        logits = model(x)
        torch.nn.functional.cross_entropy(logits, labels).backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    images = ref.cuda()
    l1, g1 = run(images)
    l2, g2 = run(images)
    make = lambda: mix.MixedFrames(src.cuda(), 32, index=torch.tensor(index, device="cuda"), geom=geom.cuda(), table=table,
                                   mix=(rec.cuda(), lam.cuda()))
    assert _same(make().images(), ref)
    lf, gf = run(make())
    assert _same(lf, l1) and _same(l1, l2)
    for k in g1:
        if _same(g1[k], g2[k]):
            assert _same(gf[k], g1[k]), k
        else:                                        # atomics in its reduction: the bound test_gpu_data.py puts on these gradients
            assert O.rel_l2(gf[k].cpu(), g1[k].cpu()) < 5e-3, k


def test_soft_target_loss_as_loss_fn_of_the_training_step(hip):
    from vitamd import mix
    from vitamd.optim import AdamW
    TV, model = _model()
    src, index, geom, rec, lam, ref = _prep_case("fast_p16", 4, "mixed")
    a = Wt.randint(3, "labels", (4,), 10)
    b = a[rec[:, 0].long()]
    with torch.no_grad():
        logits = model(ref.cuda()).float().cpu()
    want, t32 = R.soft_ce_ref(logits, a, b, lam, 0.1), R.soft_ce_torch32(logits, a, b, lam, 0.1)
    optim = AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    frames = mix.MixedFrames(src.cuda(), 32, index=torch.tensor(index, device="cuda"), geom=geom.cuda(), table=_table(3), mix=(rec.cuda(), lam.cuda()))
    before = model.head.bias.detach().clone()
    loss = TV.train_step(model, frames, mix.MixedLabels(a.cuda(), b.cuda(), lam.cuda()), optim, loss_fn=mix.SoftTargetLoss(0.1))
    assert loss.dim() == 0 and not torch.equal(model.head.bias.detach(), before)
    assert not R.check_cross_entropy({"mean": loss.detach().cpu()}, want, t32, "train_step")
    # and on an int64 label tensor with the fp32 batch: smoothing alone
    TV, model = _model()
    with torch.no_grad():
        logits = model(ref.cuda()).float().cpu()
    want, t32 = R.soft_ce_ref(logits, a, smoothing=0.1), R.soft_ce_torch32(logits, a, smoothing=0.1)
    optim = AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    loss = TV.train_step(model, ref.cuda(), a.cuda(), optim, loss_fn=mix.SoftTargetLoss(0.1))
    assert not R.check_cross_entropy({"mean": loss.detach().cpu()}, want, t32, "train_step, labels alone")


# ---------------------------------------------------------------------------------------------- the loader
def _host_batches(n_batches, B):
    g = torch.Generator().manual_seed(21)
    originals = [torch.randint(0, 256, (B, 11, 13, 3), generator=g, dtype=U8) for _ in range(n_batches)]
    labels = [torch.arange(B) + 10 * i for i in range(n_batches)]
    return originals, labels


def _drain(loader, handed):
    seen = []
    with _Alarm(60):
        for frames, lab in loader:
            for u8, l in handed:                     # everything the loader has taken so far is overwritten at once
                u8.fill_(0)
                l.fill_(-1)
            seen.append((frames, lab, frames.geom))
        done = torch.cuda.Event()
        done.record()
        deadline = time.monotonic() + 30
        while not done.query():                      # polled, not waited on
            assert time.monotonic() < deadline, "the loader's work did not finish"
    return seen


def _host(originals, labels, handed):
    for u8, lab in zip(originals, labels):
        pair = (u8.clone(), lab.clone())
        handed.append(pair)
        yield pair


def test_mix_loader_yields_the_reference_and_reuses_slots_behind_their_events(hip):
    from vitamd import mix
    n_batches, B = 3, 4
    originals, labels = _host_batches(n_batches, B)
    handed = []
    m = mix.Mix(per_sample=True, seed=13)
    loader = mix.MixLoader(_host(originals, labels, handed), "cuda", 8, m, patch=4, image=True, mean=R.MEAN[:3], std=R.STD[:3], train=True,
                           seed=77, depth=2)
    seen = _drain(loader, handed)
    assert len(seen) == n_batches and loader.step == n_batches
    modes = set()
    for i, (frames, lab, geom) in enumerate(seen):
        want_geom = D.draw_ref(B, (11, 13), (8, 8), 77, i)
        rec, lam = m.draw(B, (8, 8), i)
        modes |= set(rec[:, 1].tolist())
        assert isinstance(frames, mix.MixedFrames) and isinstance(lab, mix.MixedLabels)
        assert torch.equal(geom.cpu(), want_geom)
        assert torch.equal(frames.mix[0].cpu(), rec) and torch.equal(frames.mix[1].cpu(), lam)
        ref = R.mixed_frames_ref(originals[i], (8, 8), None, want_geom, rec, lam, R.MEAN[:3], R.STD[:3])
        assert _same(frames.images(), ref), i
        assert _same(frames.patches(4), D.patch_rows(ref, 4).to(BF16)), i
        assert lab.a.is_cuda and torch.equal(lab.a.cpu(), labels[i]) and torch.equal(lab.b.cpu(), labels[i].flip(0))
        assert lab.lam.dtype == F32 and torch.equal(lab.lam.cpu(), lam)
    assert modes == {1, 2}


def test_mix_loader_in_evaluation_is_the_device_loader(hip):
    from vitamd import data, mix
    n_batches, B = 3, 4
    originals, labels = _host_batches(n_batches, B)
    kw = dict(patch=4, image=True, mean=R.MEAN[:3], std=R.STD[:3], train=False, seed=77, depth=2)
    h1, h2 = [], []
    got = _drain(mix.MixLoader(_host(originals, labels, h1), "cuda", 8, mix.Mix(), **kw), h1)
    want = _drain(data.DeviceLoader(_host(originals, labels, h2), "cuda", 8, **kw), h2)
    assert len(got) == len(want) == n_batches
    for (f1, l1, g1), (f2, l2, g2) in zip(got, want):
        assert type(f1) is data.Frames and isinstance(l1, torch.Tensor)
        assert torch.equal(g1, g2) and torch.equal(l1, l2)
        assert _same(f1.images(), f2.images()) and _same(f1.patches(4), f2.patches(4))


# ---------------------------------------------------------------------------------------------- poison
def test_prep_mix_and_soft_cross_entropy_clean_against_poisoned(hip):
    """the workload of tests/test_gpu_poison.py's rule: prep + mix, then the loss forward and backward on fixed logits, run clean, clean
    again and inside poisoned() with dirty_scratch before it; every output must have equal bits"""
    from vitamd import lm, mix
    src, index, geom, rec, lam, _ = _prep_case("fast_p16", 4, "mixed")
    x, ya, yb, cl = R.ce_case(5, 1001, seed=9)

    def workload():
        f = mix.MixedFrames(src.cuda(), 32, index=torch.tensor(index, device="cuda"), geom=geom.cuda(), table=_table(3), mix=(rec.cuda(), lam.cuda()))
        f.materialise(16, image=True)
        out = {"image": f.images().cpu(), "patches": f.patches(16).cpu(), "patches_p4": f.patches(4).cpu()}
        for dtype in (F32, BF16):
            xd = x.to(dtype).cuda().requires_grad_(True)
            loss = lm.soft_cross_entropy(xd, ya.cuda(), yb.cuda(), cl.cuda(), 0.1)
            (loss * G_UP).backward()
            out[f"loss/{dtype}"], out[f"grad/{dtype}"] = loss.detach().cpu().reshape(1), xd.grad.cpu()
            plain = lm.soft_cross_entropy(xd.detach(), ya.cuda(), smoothing=0.1)
            out[f"plain/{dtype}"] = plain.detach().cpu().reshape(1)
        torch.cuda.synchronize()
        return out

    clean, again = workload(), workload()
    log = []
    with P.poisoned(log):
        P.dirty_scratch()
        dirty = workload()
    torch.cuda.synchronize()
    assert log, "nothing was poisoned"
    assert not P.compare(clean, again, set(clean))
    assert not P.compare(clean, dirty, set(clean))
