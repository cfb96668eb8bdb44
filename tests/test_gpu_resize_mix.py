"""Mixing resized samples in one launch on the GPU (csrc/resize.hip vitamd_frames_prep_resize_mix, vitamd.mix.MixedResizedFrames /
ResizeMixLoader) against tests/_resize_mix_ref.py.

The contract: with R the fp32 image a STAND-ALONE vitamd_frames_prep_resize launch gives for the same (index, box, mean, std), the
mixing entry's image is bit-equal to the composition of R by the record (torch's CPU a.mul(l).add(p.mul(1 - l)) and torch.where) -
both passes of a tile add in the plain kernel's order - and lies within _resize_mix_ref.bounds of the float64 reference (derived
there).  The bf16 rows are the round-to-nearest-even im2col of the entry's own image.  Every output is filled with 0xFF bytes (NaN in
both formats) before its launch and lies between guards (test_gpu_resize's helpers).

Cases (_resize_mix_ref): a16_p4 one tile; b16_p4 exactly 8x, two strip chunks per pass (the second pass must not disturb the first);
b40x36_p4 2 x 2 partial tiles, with a CutMix box that covers tile (0, 0) and one that touches tile (1, 1) by a single pixel; c4_p4 and
w14_p7 the generic form.  B = 5: sample 2 is its own partner.  Every name of _mix_ref.RECORDS, with and without mean / std."""
import functools

import pytest
import torch

import _mix_ref as M
import _poison as P
import _resize_mix_ref as RM
import _resize_ref as R
import test_gpu_resize as T
import weights as Wt
from test_gpu_data import _same, _table
from test_gpu_mix import _run_raw as _run_prep_mix
from test_gpu_resize import GUARD, _dev, _filled

pytestmark = pytest.mark.gpu
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
B = RM.B


def _run_mix(hip, src, index, box, mean, std, rec, lam, H, W, p, want_patches=True, want_image=True, expect=0, override=None):
    """the mixing C entry on filled, guarded outputs (test_gpu_resize._run_raw with the two further arguments) -> (patches or None,
    image or None) on the CPU.  expect != 0: the call must return that code and leave every byte of both outputs as it was"""
    Nsrc, Hs, Ws, C = src.shape
    n = box.shape[0]
    pw = iw = pm = im = None
    if want_patches:
        pw, pm = _filled(n * C * H * W, BF16)
    if want_image:
        iw, im = _filled(n * C * H * W, F32)
    ptr = lambda t: None if t is None else t.data_ptr()
    a = dict(src=ptr(src), index=ptr(index), box=ptr(box), mean=ptr(mean), std=ptr(std), patches=ptr(pm), image=ptr(im), B=n, Nsrc=Nsrc, Hs=Hs,
             Ws=Ws, C=C, H=H, W=W, p=p, rec=ptr(rec), lam=ptr(lam))
    a.update(override or {})
    code = hip.vitamd_frames_prep_resize_mix(a["src"], a["index"], a["box"], a["mean"], a["std"], a["patches"], a["image"], a["B"], a["Nsrc"],
                                             a["Hs"], a["Ws"], a["C"], a["H"], a["W"], a["p"], a["rec"], a["lam"],
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == expect, (code, expect, override)
    for whole in (pw, iw):
        if whole is not None:
            assert bool((whole[:GUARD] == -1).all()) and bool((whole[-GUARD:] == -1).all()), "a guard was written"
            if expect != 0:
                assert bool((whole == -1).all()), "a refused call wrote to an output"
    if expect != 0:
        return None, None
    return (pm.view(n * (H // p) * (W // p), C * p * p).cpu() if want_patches else None, im.view(n, C, H, W).cpu() if want_image else None)


@functools.lru_cache(maxsize=None)
def _case(name, norm):
    """(src, index, box, mean, std, the float64 images of every sample, _resize_ref.bounds); computed once, never written to"""
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index, box = RM.case(name)
    mean, std = (R.MEAN[:C], R.STD[:C]) if norm else (None, None)
    return src, index, box, mean, std, R.resize_ref(src, (H, W), index, box, mean, std), R.bounds(src.shape, (H, W), box, std)


@functools.lru_cache(maxsize=None)
def _alone(name, norm):
    """the stand-alone launch of vitamd_frames_prep_resize of a case -> (patches, image) on the CPU; launched once per case"""
    from vitamd import lib
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index, box, mean, std = _case(name, norm)[:5]
    return T._run_raw(lib.load(), src.cuda(), _dev(index, torch.int64), box.cuda(), _dev(mean, F32), _dev(std, F32), H, W, p)


def _on_device(name, norm):
    src, index, box, mean, std = _case(name, norm)[:5]
    return src.cuda(), _dev(index, torch.int64), box.cuda(), _dev(mean, F32), _dev(std, F32)


# ---------------------------------------------------------------------------------------------- the kernel against the composition
@pytest.mark.parametrize("norm", [False, True], ids=["unit", "norm"])
@pytest.mark.parametrize("name,rname", [(c, r) for c in RM.CASE_NAMES for r in RM.record_names(c)])
def test_image_is_the_composition_within_the_bound_rows_round_to_nearest_even_outputs_independent(hip, name, rname, norm):
    from vitamd import ops
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src_c, index_c, box_c, mean_c, std_c, ref_images, bnd_alone = _case(name, norm)
    rec, lam = RM.record(rname, H, W)
    alone_p, alone_i = _alone(name, norm)
    dev = _on_device(name, norm)
    patches, image = _run_mix(hip, *dev, rec.cuda(), lam.cuda(), H, W, p)
    assert bool(torch.isfinite(image).all())
    want = RM.mixed_resized_ref(src_c, (H, W), index_c, box_c, rec, lam, mean_c, std_c, images=alone_i)
    assert not RM.check_bits(image, want, f"{name} {rname}")
    ref = RM.compose(ref_images, rec, lam)
    bnd = RM.bounds(src_c.shape, (H, W), box_c, rec, lam, ref_images, std_c, bnd=bnd_alone)
    err = (image.double() - ref).abs()
    print(f"{name} {rname} norm={norm}: worst error / bound {float((err / bnd).max()):.3f}, worst error {float(err.max()):.3e}")
    assert not R.check_image(image, ref, bnd, f"{name} {rname}")
    assert not R.check_rows(patches, image, p, name)
    assert _same(patches, ops.im2col(image.cuda(), p).cpu())               # the rows the unfused route makes of the same image
    assert _same(image[2], alone_i[2])                                     # its own partner: the plain resize, whatever the mode
    only_p, none_i = _run_mix(hip, *dev, rec.cuda(), lam.cuda(), H, W, p, want_image=False)
    none_p, only_i = _run_mix(hip, *dev, rec.cuda(), lam.cuda(), H, W, p, want_patches=False)
    assert none_i is None and none_p is None and _same(only_p, patches) and _same(only_i, image)
    again_p, again_i = _run_mix(hip, *dev, rec.cuda(), lam.cuda(), H, W, p)
    assert _same(again_p, patches) and _same(again_i, image)               # no atomics: the same bits on every call
    if rname == "none":                                                    # all mode 0: the bits of vitamd_frames_prep_resize
        assert _same(image, alone_i) and _same(patches, alone_p)
    if rname == "mixup":                                                   # NULL lam is l = 1 ...
        _, one = _run_mix(hip, *dev, rec.cuda(), None, H, W, p, want_patches=False)
        assert not RM.check_bits(one, RM.compose(alone_i, rec, torch.ones(B)), "NULL lam")
    if rname.startswith("cut"):                                            # ... and mode 2 does not read it
        _, cut = _run_mix(hip, *dev, rec.cuda(), None, H, W, p, want_patches=False)
        assert _same(cut, image)


@pytest.mark.parametrize("rname", ["mixup", "mixed"])
@pytest.mark.parametrize("name", ["a16_p4", "c4_p4", "w14_p7"])
def test_an_identity_box_record_under_mixing_has_the_bits_of_the_plain_mixing_prep(hip, name, rname):
    """h = Hv = H and w = Wv = W: one tap of weight 1 per value, so the entry is vitamd_frames_prep_mix with geom (y0, x0, flip) and the
    table of the same mean and std"""
    from vitamd import data
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index = R.case(name)[:2]
    geom = torch.tensor([[3, 5, 1], [0, 0, 0], [Hs - H, Ws - W, 1], [7, 2, 0], [Hs - H - 1, Ws - W - 1, 0]], dtype=torch.int32)
    box = torch.tensor([[y, H, H, 0, x, W, W, 0, f, 0] for y, x, f in geom.tolist()], dtype=torch.int32)
    rec, lam = RM.record(rname, H, W)
    it = _dev(index, torch.int64)
    for mean, std in ((None, None), (R.MEAN[:C], R.STD[:C])):
        table = data.norm_table(mean, std, channels=C).cuda()
        want_p, want_i = _run_prep_mix(hip, src.cuda(), table, it, geom.cuda(), rec.cuda(), lam.cuda(), B, H, W, p)
        got_p, got_i = _run_mix(hip, src.cuda(), it, box.cuda(), _dev(mean, F32), _dev(std, F32), rec.cuda(), lam.cuda(), H, W, p)
        assert _same(got_i, want_i.cpu()) and _same(got_p, want_p.cpu())


@pytest.mark.parametrize("name", ["a16_p4", "w14_p7"])
def test_a_wild_record_gives_what_the_record_it_clamps_to_gives(hip, name):
    """test_gpu_resize's wild boxes and index, and on top of them partner, mode and mix box out of range"""
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src = R.case(name)[0]
    lo, hi = R.I32_MIN, R.I32_MAX
    index, tame_index = [-3, 77, 1, 1 << 40, 2], [0, Nsrc - 1, 1, Nsrc - 1, 2]
    wild = torch.tensor([[lo, hi, lo, hi, hi, lo, hi, lo, 7, 99], [-5, 0, 3, -1, 60, 0, 0, 5, -1, 0], [hi, hi, hi, hi, lo, lo, lo, lo, -7, 0],
                         [5, 1000, 2, 1000, 3, 1000, 2, -4, 0, 0], [30, 100, 1, 0, 50, 100, 1, 0, 1 << 20, -1]], dtype=torch.int32)
    tame = torch.tensor([[*R.clamp_box(r, Hs, Ws, H, W), 0] for r in wild.tolist()], dtype=torch.int32)
    assert tame[:, :8].tolist() != wild[:, :8].tolist()
    wild_rec = torch.tensor([[B + 5, 1, lo, hi, hi, lo], [-3, 2, lo, hi, lo, hi], [1, 7, 0, H, 0, W], [0, 2, 2, hi, lo, 5], [hi, 2, -1, 3, -2, W + 9]],
                            dtype=torch.int32)
    tame_rec = torch.tensor([[B - 1, 1, 0, H, W, 0], [0, 2, 0, H, 0, W], [1, 0, 0, H, 0, W], [0, 2, 2, H, 0, 5], [B - 1, 0, 0, 3, 0, W]],
                            dtype=torch.int32)
    assert M.clamp_rec(wild_rec, B, H, W) == M.clamp_rec(tame_rec, B, H, W) == [tuple(r) for r in tame_rec.tolist()]
    lam = torch.tensor([0.3, 0.5, 0.25, 0.75, 0.625])
    mean, std = R.MEAN[:C], R.STD[:C]
    norm = (_dev(mean, F32), _dev(std, F32))
    _, alone = T._run_raw(hip, src.cuda(), _dev(tame_index, torch.int64), tame.cuda(), *norm, H, W, p)
    want = RM.compose(alone, tame_rec, lam)
    got_w = _run_mix(hip, src.cuda(), _dev(index, torch.int64), wild.cuda(), *norm, wild_rec.cuda(), lam.cuda(), H, W, p)
    got_t = _run_mix(hip, src.cuda(), _dev(tame_index, torch.int64), tame.cuda(), *norm, tame_rec.cuda(), lam.cuda(), H, W, p)
    assert bool(torch.isfinite(got_w[1]).all()) and bool(torch.isfinite(got_w[0].float()).all())
    assert not RM.check_bits(got_w[1], want, "wild") and not RM.check_bits(got_t[1], want, "tame")
    assert _same(got_w[0], got_t[0]) and not R.check_rows(got_w[0], got_w[1], p, name)
    ref_images = R.resize_ref(src, (H, W), tame_index, tame, mean, std)
    bnd = RM.bounds(src.shape, (H, W), tame, tame_rec, lam, ref_images, std)
    assert not R.check_image(got_w[1], RM.compose(ref_images, tame_rec, lam), bnd, name)


@pytest.mark.parametrize("rname", ["mixup", "mixed"])
def test_the_end_of_src_and_an_odd_base_address_take_byte_loads_with_the_same_bits(hip, rname):
    """test_gpu_resize's boxes in the bottom-right corner of the LAST frame (2, 4, 6 and 16 taps per column), for both passes of a
    tile; and a source that starts at an odd address takes byte loads throughout"""
    Nsrc, Hs, Ws, C, H, W, p = R.CASES["b16_p4"]
    src = R.case("b16_p4")[0]
    box = torch.tensor([[Hs - h, h, H, 0, Ws - w, w, W, 0, f, 0] for h, w, f in ((7, 9, 0), (16, 16, 1), (30, 28, 1), (50, 47, 0), (128, 128, 1))],
                       dtype=torch.int32)
    index = [Nsrc - 1] * 5
    rec, lam = RM.record(rname, H, W)
    args = (_dev(index, torch.int64), box.cuda(), _dev(R.MEAN[:3], F32), _dev(R.STD[:3], F32))
    _, alone = T._run_raw(hip, src.cuda(), *args, H, W, p)
    patches, image = _run_mix(hip, src.cuda(), *args, rec.cuda(), lam.cuda(), H, W, p)
    assert not RM.check_bits(image, RM.compose(alone, rec, lam), "end of src") and not R.check_rows(patches, image, p, "end of src")
    store = torch.empty(src.numel() + 1, dtype=U8, device="cuda")
    shifted = store[1:].view(src.shape)
    shifted.copy_(src)
    assert shifted.data_ptr() % 2 == 1
    odd_p, odd_i = _run_mix(hip, shifted, *args, rec.cuda(), lam.cuda(), H, W, p)
    assert _same(odd_i, image) and _same(odd_p, patches)


def test_every_refusal_returns_its_code_and_writes_nothing(hip):
    SHAPE, ARG = 1, 2
    Nsrc, Hs, Ws, C, H, W, p = R.CASES["a16_p4"]
    dev = _on_device("a16_p4", True)
    rec, lam = RM.record("mixed", H, W)
    run = lambda code, **o: _run_mix(hip, *dev, rec.cuda(), lam.cuda(), H, W, p, expect=code, override=o)
    for bad in (dict(B=0), dict(Nsrc=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(C=0), dict(C=5), dict(Hs=8193), dict(Ws=8193),
                dict(H=8193), dict(W=8193), dict(p=0), dict(p=3), dict(p=32), dict(index=None, B=Nsrc + 1),
                dict(Nsrc=1 << 20, Hs=8192, Ws=8192), dict(B=1 << 20, H=8192, W=8192, p=4)):
        run(SHAPE, **bad)
        run(SHAPE, src=None, box=None, rec=None, **bad)                      # the shape answers first
    for bad in (dict(src=None), dict(box=None), dict(mean=None), dict(std=None), dict(rec=None), dict(rec=None, lam=None)):
        run(ARG, **bad)
    _run_mix(hip, *dev, rec.cuda(), lam.cuda(), H, W, p, want_patches=False, want_image=False, expect=ARG)


@pytest.mark.parametrize("p", [8, 2], ids=["fast", "generic"])
def test_past_the_grid_cap(hip, p):
    """test_gpu_resize's case past the cap (2 x 2 tiles of 64 x 64 outputs, a quarter of the cap + 1 samples), mixed per sample by the
    host draw"""
    from vitamd import mix, ops
    cap = ops.frames_prep_resize_grid_cap()
    src, rec15, combos, ref15, bnd15 = T._cap_case()
    n = cap // 4 + 1
    assert n * 4 > cap and n * 3 * 64 * 64 > cap * 256
    pick = [(7 * b) % 15 for b in range(n)]
    index = torch.tensor([combos[k][0] for k in pick])
    box = rec15[[combos[k][1] for k in pick]]
    rec, lam = mix.Mix(per_sample=True, prob=0.9, seed=3).draw(n, (64, 64), 0)
    assert {0, 1, 2} == set(rec[:, 1].tolist())
    norm = (_dev(R.MEAN[:3], F32), _dev(R.STD[:3], F32))
    _, alone = T._run_raw(hip, src.cuda(), index.cuda(), box.cuda(), *norm, 64, 64, p)
    patches, image = _run_mix(hip, src.cuda(), index.cuda(), box.cuda(), *norm, rec.cuda(), lam.cuda(), 64, 64, p)
    assert not RM.check_bits(image, RM.compose(alone, rec, lam), f"cap p={p}")
    bnd = RM.bounds(src.shape, (64, 64), box, rec, lam, ref15[pick], R.STD[:3], bnd=bnd15[pick])
    assert not R.check_image(image, RM.compose(ref15[pick], rec, lam), bnd, f"cap p={p}")
    assert not R.check_rows(patches, image, p, f"cap p={p}")


# ---------------------------------------------------------------------------------------------- the Python objects
def test_mixed_resized_frames_hand_out_what_the_entry_point_computes(hip):
    from vitamd import data, mix, resize
    name = "b40x36_p4"
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index, box, mean, std = _case(name, True)[:5]
    rec, lam = RM.record("cut_cover", H, W)
    want_p, want_i = _run_mix(hip, *_on_device(name, True), rec.cuda(), lam.cuda(), H, W, p)
    f = mix.MixedResizedFrames(src.cuda(), (H, W), box, index=torch.tensor(index), mean=mean, std=std, mix=(rec, lam))
    assert isinstance(f, resize.ResizedFrames) and isinstance(f, data.Frames) and tuple(f.shape) == (5, C, H, W) and f.geom is None
    assert torch.equal(f.box.cpu(), box) and torch.equal(f.mix[0].cpu(), rec) and torch.equal(f.mix[1].cpu(), lam) and f.mix[0].is_cuda
    assert _same(f.patches(p).cpu(), want_p) and _same(f.images().cpu(), want_i)
    f.release_source()
    assert _same(f.patches(p).cpu(), want_p)
    with pytest.raises(Exception, match="source slot is reused"):
        f.patches(2)


def _model():
    import train_vit as TV
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    model = TV.ViTClassifier(cfg, num_classes=10)
    model.load_state_dict(Wt.classifier_state(3, 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, 10))
    return TV, model.cuda()


def test_classifier_takes_mixed_resized_frames_where_it_takes_frames_with_the_soft_target_loss(hip):
    from vitamd import mix, resize
    from vitamd.optim import AdamW
    TV, model = _model()
    src = R.case("a16_p4")[0]
    box = resize.rrc_boxes(5, (37, 53), 32, seed=3, step=0)
    rec, lam = RM.record("mixed", 32, 32)
    make = lambda: mix.MixedResizedFrames(src.cuda(), 32, box, index=torch.tensor([3, 1, 1, 0, 2]), mean=R.MEAN[:3], std=R.STD[:3], mix=(rec, lam))
    with torch.no_grad():
        images = make().images()
        want = model(images)
        got = model(make())
    assert images.dtype == F32 and want.shape == (5, 10) and torch.equal(got, want)
    a = Wt.randint(3, "labels", (5,), 10)
    b = a[rec[:, 0].long()]
    logits = want.float().cpu()
    ref, t32 = M.soft_ce_ref(logits, a, b, lam, 0.1), M.soft_ce_torch32(logits, a, b, lam, 0.1)
    optim = AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)
    before = model.head.bias.detach().clone()
    loss = TV.train_step(model, make(), mix.MixedLabels(a.cuda(), b.cuda(), lam.cuda()), optim, loss_fn=mix.SoftTargetLoss(0.1))
    assert loss.dim() == 0 and not torch.equal(model.head.bias.detach(), before)
    assert not M.check_cross_entropy({"mean": loss.detach().cpu()}, ref, t32, "train_step")


# ---------------------------------------------------------------------------------------------- the loader
@pytest.mark.parametrize("mode,with_extents", [("rrc", True), ("resize_crop", False)])
def test_resize_mix_loader_yields_what_the_draws_and_the_reference_predict(hip, mode, with_extents):
    """three batches through two slots (the last one smaller): the boxes of ResizeLoader.boxes and the record of Mix.draw under the
    loader's (seed, step), the image the composition of a stand-alone resize of the same boxes, the labels paired by the record"""
    from vitamd import mix, resize
    n_batches, n = 3, 4
    originals, labels, extents = T._host_batches(n_batches, n)
    handed = []
    m = mix.Mix(per_sample=True, seed=13)
    loader = mix.ResizeMixLoader(T._host(originals, labels, extents if with_extents else None, handed), "cuda", 16, m, mode=mode, resize_to=18,
                                 patch=4, image=True, mean=R.MEAN[:3], std=R.STD[:3], train=True, seed=77, depth=2)
    seen = T._drain(loader, handed)
    assert len(seen) == n_batches and loader.step == n_batches
    modes = set()
    for i, (frames, lab) in enumerate(seen):
        k = originals[i].shape[0]
        ext = extents[i] if with_extents else None
        box = loader.boxes(k, (37, 53), i, ext)
        if mode == "rrc":
            assert torch.equal(box, resize.rrc_boxes(k, (37, 53), 16, seed=77, step=i, extents=ext))
        else:
            assert torch.equal(box, resize.resize_crop_boxes(k, (37, 53), 18, 16, seed=77, step=i, extents=ext))
        rec, lam = m.draw(k, (16, 16), i)
        modes |= set(rec[:, 1].tolist())
        assert isinstance(frames, mix.MixedResizedFrames) and isinstance(lab, mix.MixedLabels) and tuple(frames.shape) == (k, 3, 16, 16)
        assert torch.equal(frames.box.cpu(), box) and torch.equal(frames.mix[0].cpu(), rec) and torch.equal(frames.mix[1].cpu(), lam)
        alone = resize.ResizedFrames(originals[i].cuda(), 16, box, mean=R.MEAN[:3], std=R.STD[:3]).images().cpu()
        image = frames.images().cpu()
        assert not RM.check_bits(image, RM.compose(alone, rec, lam), f"batch {i}")
        ref_images = R.resize_ref(originals[i], (16, 16), None, box, R.MEAN[:3], R.STD[:3])
        bnd = RM.bounds(originals[i].shape, (16, 16), box, rec, lam, ref_images, R.STD[:3])
        assert not R.check_image(image, RM.compose(ref_images, rec, lam), bnd, f"batch {i}")
        assert not R.check_rows(frames.patches(4).cpu(), image, 4, f"batch {i}")
        assert lab.a.is_cuda and torch.equal(lab.a.cpu(), labels[i]) and torch.equal(lab.b.cpu(), labels[i].flip(0))
        assert lab.lam.dtype == F32 and torch.equal(lab.lam.cpu(), lam)
    assert modes == {1, 2}


def test_resize_mix_loader_in_evaluation_is_the_centre_form_with_plain_labels(hip):
    from vitamd import mix, resize
    n_batches, n = 3, 4
    originals, labels, extents = T._host_batches(n_batches, n)
    handed = []
    loader = mix.ResizeMixLoader(T._host(originals, labels, extents, handed), "cuda", 16, mix.Mix(), mode="rrc", resize_to=18, patch=4,
                                 image=True, train=False, depth=2)
    seen = T._drain(loader, handed)
    assert len(seen) == n_batches
    for i, (frames, lab) in enumerate(seen):
        k = originals[i].shape[0]
        box = resize.resize_center_boxes(k, (37, 53), 18, 16, extents=extents[i])
        assert type(frames) is resize.ResizedFrames and isinstance(lab, torch.Tensor) and torch.equal(lab.cpu(), labels[i])
        assert torch.equal(frames.box.cpu(), box) and set(box[:, 8].tolist()) == {0}
        ref = R.resize_ref(originals[i], (16, 16), None, box)
        assert not R.check_image(frames.images().cpu(), ref, R.bounds(originals[i].shape, (16, 16), box), f"batch {i}")


# ---------------------------------------------------------------------------------------------- poison
def test_the_new_route_clean_against_poisoned(hip):
    """the rule of tests/test_gpu_poison.py (its three_runs): the workload clean, clean again, and inside poisoned() with
    dirty_scratch before it; every output must have equal bits, and the route's allocations must have been poisoned"""
    from test_gpu_poison import three_runs
    from vitamd import lm, mix
    name = "b40x36_p4"
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index, box, mean, std = _case(name, True)[:5]
    rec, lam = RM.record("mixed", H, W)
    x, ya, yb, cl = M.ce_case(5, 1001, seed=9)

    def workload(dirty):
        dirty()
        f = mix.MixedResizedFrames(src.cuda(), (H, W), box, index=torch.tensor(index), mean=mean, std=std, mix=(rec, lam))
        f.materialise(p, image=True)
        out = {"image": f.images().cpu(), "patches": f.patches(p).cpu(), "patches_p2": f.patches(2).cpu()}
        xd = x.cuda().requires_grad_(True)
        loss = lm.soft_cross_entropy(xd, ya.cuda(), yb.cuda(), cl.cuda(), 0.1)
        loss.backward()
        out["loss"], out["grad"] = loss.detach().cpu().reshape(1), xd.grad.cpu()
        torch.cuda.synchronize()
        return out

    clean, dirty, exact = three_runs("resize-mix", workload)
    assert exact == set(clean) and not P.compare(clean, dirty, exact)
    assert bool(torch.isfinite(dirty["image"]).all())
