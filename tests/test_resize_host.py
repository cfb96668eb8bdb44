"""The resizing input feed without a GPU: the float64 reference of tests/_resize_ref.py against torch's own antialiased bilinear
interpolation, the fp32 restatements against the derived bound, proof that the checks of test_gpu_resize.py bite (every planted
mistake of _resize_ref.standin is reported at that file's shapes), the host-side draws of vitamd.resize, the binding of the new entry
points and their refusals, and the conditions tests/test_gpu_poison.py puts on new code in vitamd/."""
import ctypes
import os

import pytest
import torch

import _abi
import _poison as P
import _resize_ref as R

SHAPE, ARG = 1, 2
NEW_SYMBOLS = {"vitamd_frames_prep_resize": 16, "vitamd_frames_prep_resize_grid_cap": 0}
PINNED_SITES = {("ops.py", 137), ("functions.py", 182), ("data.py", 229), ("data.py", 230), ("data.py", 243)}

_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", list(R.CASES))
def test_the_reference_is_torchs_antialiased_bilinear_of_the_cropped_box(name):
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index, box = R.case(name)
    ref = R.resize_ref(src, (H, W), index, box) * 255.0                  # no mean / std: r / 255
    tv = R.interpolate_ref(src, (H, W), index, box)
    assert float((ref - tv).abs().max()) < 1e-9


def test_the_reference_on_further_box_forms():
    """1-pixel boxes, 8x down-scaling of a whole axis, up-scaling by 16, a window in the middle of a virtual image"""
    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 256, (2, 64, 96, 3), generator=g, dtype=torch.uint8)
    box = torch.tensor([[5, 1, 8, 0, 7, 1, 8, 0, 0, 0], [0, 64, 8, 0, 0, 64, 8, 0, 1, 0], [10, 2, 32, 12, 20, 3, 48, 20, 1, 0],
                        [3, 50, 19, 6, 1, 90, 31, 11, 0, 0]], dtype=torch.int32)
    ref = R.resize_ref(src, (8, 8), [1, 0, 1, 0], box) * 255.0
    assert float((ref - R.interpolate_ref(src, (8, 8), [1, 0, 1, 0], box)).abs().max()) < 1e-9


def test_weights_are_integer_ratios_with_at_most_sixteen_taps():
    for O, off, n, nv in [(16, 0, 128, 16), (16, 0, 23, 16), (16, 0, 3, 16), (16, 4, 37, 20), (8, 0, 1, 8), (2, 1022, 8192, 1024)]:
        num = R.numerators(O, off, n, nv)
        assert all(sum(r) > 0 and sum(v > 0 for v in r) <= 16 for r in num)
        assert max(max(r) for r in num) <= 2 * max(n, nv) and 16 * 2 * max(n, nv) < 1 << 24
        w = R.weights(O, off, n, nv)
        assert torch.allclose(w.sum(1), torch.ones(O, dtype=torch.float64), rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_fp32_restatements_stay_within_the_bound(name):
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index, box = R.case(name)
    for mean, std in ((None, None), (R.MEAN[:C], R.STD[:C])):
        ref = R.resize_ref(src, (H, W), index, box, mean, std)
        bnd = R.bounds(src.shape, (H, W), box, std)
        for order in ("xy", "yx"):
            got = R.resize_f32(src, (H, W), index, box, mean, std, order=order)
            assert not R.check_image(got, ref, bnd, f"{name} {order}")
        image, rows = R.standin(src, (H, W), index, box, mean, std, p=p)         # the clean stand-in passes both checks
        assert not R.check_image(image, ref, bnd, name) and not R.check_rows(rows, image, p, name)


def test_the_identity_record_is_the_plain_prep():
    import _data_ref as D
    src, index, _ = R.case("a16_p4")
    geom = torch.tensor([[3, 5, 1], [0, 0, 0], [21, 37, 1], [7, 2, 0], [20, 36, 0]], dtype=torch.int32)
    plain = D.frames_ref(src, (16, 16), index, geom, R.MEAN[:3], R.STD[:3])
    # h = Hv = H: one tap of weight 1 per value (oy is clamped into [0, Hv - H] = [0, 0]: the offset of such a record lives in y0)
    box = torch.tensor([[y, 16, 16, 0, x, 16, 16, 0, f, 0] for y, x, f in geom.tolist()], dtype=torch.int32)
    for order in ("xy", "yx"):
        got = R.resize_f32(src, (16, 16), index, box, R.MEAN[:3], R.STD[:3], order=order)
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32))
    assert all(sum(v > 0 for v in r) == 1 for r in R.numerators(16, 0, 16, 16))


# ---------------------------------------------------------------------------------------------- the checks bite
BUG_CASES = {                                        # bug -> the cases (and the normalisation) in which it is exercised
    "no_half_pixel": list(R.CASES), "support_one": list(R.CASES), "no_clip": list(R.CASES), "no_renorm": list(R.CASES),
    "flip_virtual": list(R.CASES), "no_offset": list(R.CASES), "swap_scales": list(R.CASES), "no_index": list(R.CASES),
    "swap_norm": ["a16_p4", "a12x20_p4", "b16_p4", "b40x36_p4", "c4_p4", "w14_p7"], "short_taps": list(R.CASES), "bf16_trunc": list(R.CASES),
}


@pytest.mark.parametrize("bug", R.BUGS)
def test_every_planted_mistake_is_reported(bug):
    for name in BUG_CASES[bug]:
        Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
        src, index, box = R.case(name)
        mean, std = R.MEAN[:C], R.STD[:C]
        ref = R.resize_ref(src, (H, W), index, box, mean, std)
        bnd = R.bounds(src.shape, (H, W), box, std)
        image, rows = R.standin(src, (H, W), index, box, mean, std, p=p, bug=bug)
        fails = R.check_image(image, ref, bnd, name) + R.check_rows(rows, image, p, name)
        assert fails, (bug, name)
        if bug == "bf16_trunc":
            assert not R.check_image(image, ref, bnd, name)              # the image is right: the rows alone are reported


def test_a_one_pixel_shift_is_orders_above_the_bound():
    src, index, box = R.case("a16_p4")
    shifted = box.clone()
    shifted[:, 4] += 1
    a, b = R.resize_ref(src, (16, 16), index, box[:2]), R.resize_ref(src, (16, 16), index, shifted[:2])
    assert float((a - b).abs().max()) > 1e4 * R.bound(16, 16)


def test_wild_records_clamp_to_tame_ones():
    lo, hi = R.I32_MIN, R.I32_MAX
    assert R.clamp_box([lo, hi, lo, hi, hi, lo, hi, lo, 7, 99], 37, 53, 16, 16) == (0, 37, 16, 0, 52, 1, 8192, 0, 1)
    assert R.clamp_box([-5, 0, 3, -1, 60, 0, 0, 5, -1, 0], 37, 53, 16, 16) == (0, 1, 16, 0, 52, 1, 16, 0, 1)
    assert R.clamp_box([2, 35, 1, 9, 0, 53, 1, 9, 0, 0], 131, 140, 4, 4) == (2, 35, 5, 1, 0, 53, 7, 3, 0)      # Hv up to ceil(h / 8)


# ---------------------------------------------------------------------------------------------- the draws
def test_draws_are_a_function_of_seed_and_step():
    from vitamd import resize
    a = resize.rrc_boxes(16, (37, 53), 16, seed=5, step=3)
    assert a.dtype == torch.int32 and tuple(a.shape) == (16, 10) and not a.is_cuda
    assert torch.equal(a, resize.rrc_boxes(16, (37, 53), 16, seed=5, step=3))
    for other in (resize.rrc_boxes(16, (37, 53), 16, seed=5, step=4), resize.rrc_boxes(16, (37, 53), 16, seed=6, step=3),
                  resize.rrc_boxes(16, (37, 53), 16, seed=5, step=(1 << 32) + 3)):
        assert not torch.equal(a, other)
    b = resize.resize_crop_boxes(16, (37, 53), 20, 16, seed=5, step=3)
    assert torch.equal(b, resize.resize_crop_boxes(16, (37, 53), 20, 16, seed=5, step=3))
    assert not torch.equal(b, resize.resize_crop_boxes(16, (37, 53), 20, 16, seed=5, step=4))
    assert set(a[:, 8].tolist()) == {0, 1} and set(resize.rrc_boxes(16, (37, 53), 16, seed=5, step=3, flip=False)[:, 8].tolist()) == {0}


@pytest.mark.parametrize("scale,ratio", [((0.08, 1.0), (3 / 4, 4 / 3)), ((0.3, 0.6), (0.5, 2.0))])
def test_rrc_boxes_lie_inside_their_extents_with_the_asked_area_and_aspect(scale, ratio):
    from vitamd import resize
    Hs, Ws, B = 120, 160, 8
    ext = torch.tensor([[120, 160], [90, 160], [120, 100], [64, 64], [120, 160], [100, 30], [33, 150], [120, 159]], dtype=torch.int32)
    for extents in (None, ext):
        for step in range(12):
            box = resize.rrc_boxes(B, (Hs, Ws), (24, 32), scale=scale, ratio=ratio, seed=1, step=step, extents=extents)
            for b, (y0, h, Hv, oy, x0, w, Wv, ox, flip, pad) in enumerate(box.tolist()):
                hs, ws = (Hs, Ws) if extents is None else ext[b].tolist()
                assert (Hv, oy, Wv, ox, pad) == (24, 0, 32, 0, 0) and flip in (0, 1)
                assert 0 <= y0 and 1 <= h and y0 + h <= hs and 0 <= x0 and 1 <= w and x0 + w <= ws
                central = (y0, x0) == ((hs - h) // 2, (ws - w) // 2) and (h == hs or w == ws)
                if not central:
                    # w = round(sqrt(A r)), h = round(sqrt(A / r)): each within 1/2 of its real value
                    lo = (max(w - 0.5, 0) * max(h - 0.5, 0)) / (hs * ws)
                    hi = (w + 0.5) * (h + 0.5) / (hs * ws)
                    assert hi >= scale[0] and lo <= scale[1]
                    assert (w + 0.5) / max(h - 0.5, 1e-9) >= ratio[0] and (w - 0.5) / (h + 0.5) <= ratio[1]


def test_an_impossible_range_takes_the_central_fallback():
    from vitamd import resize
    box = resize.rrc_boxes(4, (60, 100), 16, scale=(4.0, 5.0), seed=2, step=0)
    for y0, h, Hv, oy, x0, w, Wv, ox, flip, _ in box.tolist():       # in_ratio 100 / 60 > 4 / 3: h = 60, w = round(60 * 4 / 3) = 80, centred
        assert (y0, h, x0, w) == (0, 60, 10, 80)
    box = resize.rrc_boxes(4, (100, 60), 16, scale=(4.0, 5.0), seed=2, step=0)
    for y0, h, Hv, oy, x0, w, Wv, ox, flip, _ in box.tolist():       # in_ratio 0.6 < 3 / 4: w = 60, h = round(60 / 0.75) = 80
        assert (y0, h, x0, w) == (10, 80, 0, 60)
    box = resize.rrc_boxes(2, (60, 60), 16, scale=(4.0, 5.0), seed=2, step=0)
    assert all(r[:2] == [0, 60] and r[4:6] == [0, 60] for r in box.tolist())


def test_resize_sizes_are_torchvisions_and_centre_offsets_center_geoms():
    from vitamd import data, resize
    assert resize.resized_size(375, 500, 224) == (224, 298)
    assert resize.resized_size(500, 375, 224) == (298, 224)
    assert resize.resized_size(64, 64, 256) == (256, 256)
    box = resize.resize_crop_boxes(32, (375, 500), 224, 224, seed=0, step=0)
    assert set(box[:, 2].tolist()) == {224} and set(box[:, 6].tolist()) == {298}
    assert set(box[:, 3].tolist()) == {0} and 0 <= int(box[:, 7].min()) and int(box[:, 7].max()) <= 74 and len(set(box[:, 7].tolist())) > 8
    assert torch.equal(box[:, [0, 1, 4, 5]], torch.tensor([[0, 375, 0, 500]], dtype=torch.int32).repeat(32, 1))
    for src_hw, S, out_hw in (((375, 500), 224, (224, 224)), ((500, 375), 231, (224, 224)), ((64, 64), 256, (255, 250)), ((24, 40), 16, (16, 16))):
        box = resize.resize_center_boxes(3, src_hw, S, out_hw)
        Hv, Wv = resize.resized_size(*src_hw, S)
        geom = data.center_geom(3, (Hv, Wv), out_hw)
        assert torch.equal(box[:, [3, 7, 8]], geom) and box[0].tolist() == [0, src_hw[0], Hv, int(geom[0, 0]), 0, src_hw[1], Wv, int(geom[0, 1]), 0, 0]
    ext = torch.tensor([[375, 500], [500, 375], [300, 300]], dtype=torch.int32)
    box = resize.resize_center_boxes(3, (500, 500), 224, 224, extents=ext)
    assert box[:, [1, 2, 5, 6]].tolist() == [[375, 224, 500, 298], [500, 298, 375, 224], [300, 224, 300, 224]]


def test_arguments_are_refused_before_any_device_is_looked_at():
    from vitamd import lib, mix, ops, resize
    for call in (lambda: resize.rrc_boxes(0, (37, 53), 16), lambda: resize.rrc_boxes(4, (37, 53), 16, seed=-1),
                 lambda: resize.rrc_boxes(4, (37, 53), 16, step=1 << 64), lambda: resize.rrc_boxes(4, (37, 53), 16, scale=(1.0, 0.5)),
                 lambda: resize.rrc_boxes(4, (37, 53), 16, ratio=(0.0, 1.0)), lambda: resize.rrc_boxes(4, (200, 53), 16),      # beyond 8x
                 lambda: resize.rrc_boxes(4, (37, 53), 16, extents=torch.tensor([[38, 53]] * 4, dtype=torch.int32)),
                 lambda: resize.rrc_boxes(4, (37, 53), 16, extents=torch.zeros((4, 2), dtype=torch.int64)),
                 lambda: resize.rrc_boxes(4, (9000, 53), 16), lambda: resize.resize_crop_boxes(4, (37, 53), 12, 16, 0, 0),      # smaller than the crop
                 lambda: resize.resize_crop_boxes(4, (37, 53), 0, 16, 0, 0), lambda: resize.resize_center_boxes(4, (200, 200), 16, 16),
                 lambda: resize.ResizeLoader(iter([]), "cuda", 16, mode="bicubic"), lambda: resize.ResizeLoader(iter([]), "cpu", 16),
                 lambda: mix.MixLoader(iter([]), "cuda", 16, mix.Mix(), mode="rrc")):
        with pytest.raises(ValueError):
            call()
    u8 = torch.zeros((4, 11, 13, 3), dtype=torch.uint8)
    box = resize.resize_center_boxes(4, (11, 13), 16, 16)
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        resize.ResizedFrames(u8, 16, box)
    with pytest.raises(ValueError, match="box"):
        resize.ResizedFrames(u8, 16, box[:3])
    with pytest.raises(ValueError, match="mean and std"):
        resize.ResizedFrames(u8, 16, box, mean=(0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="not both"):
        ops.frames_prep(u8, (16, 16), None, 4, True, mix=(box, None), resize=(box, None, None))
    with pytest.raises(ValueError, match="table and geom"):
        ops.frames_prep(u8, (16, 16), torch.zeros((3, 256)), 4, True, resize=(box, None, None))
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        ops.frames_prep(u8, (16, 16), None, 4, True, resize=(box, None, None))
    # the default of check_frames is unchanged, message included; resize=True lifts the refusal and caps the sizes
    with pytest.raises(ValueError, match=r"does not fit the source \(11, 13\) \(resizing stays with the host loader\)"):
        ops.check_frames(u8.shape, (16, 16))
    assert ops.check_frames(u8.shape, (16, 16), 4, resize=True) == (4, 4, 11, 13, 3, 16, 16)
    with pytest.raises(ValueError, match="8192"):
        ops.check_frames((1, 8193, 8, 3), (16, 16), resize=True)
    loader = resize.ResizeLoader(iter([(u8, None, torch.tensor([[12, 13]] * 4, dtype=torch.int32))]), "cuda", 16)
    with pytest.raises(ValueError, match="extent"):
        next(loader)                                                      # refused by _check, before the copy stream exists
    assert loader._copy_stream is None


def test_frames_to_tokens_refuses_size_on_a_float_batch():
    import train_videogpt as TG
    with pytest.raises(ValueError, match="uint8"):
        TG.frames_to_tokens(None, torch.zeros((1, 2, 3, 8, 8)), size=16)


# ---------------------------------------------------------------------------------------------- the binding and the refusals
def test_new_symbols_are_bound_with_the_headers_argument_counts(L):
    from vitamd import lib, ops
    declared, _ = _abi.declared()
    for name, n in NEW_SYMBOLS.items():
        assert declared[name] == n == len(lib.SIGNATURES[name]), name
        fn = getattr(L, name)
        assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    assert ops.frames_prep_resize_grid_cap() == L.vitamd_frames_prep_resize_grid_cap() >= 256


def _resize(L, src=PTR, index=PTR, box=PTR, mean=PTR, std=PTR, patches=PTR, image=PTR, B=3, Nsrc=5, Hs=11, Ws=13, C=3, H=16, W=16, p=4):
    return L.vitamd_frames_prep_resize(src, index, box, mean, std, patches, image, B, Nsrc, Hs, Ws, C, H, W, p, None)


REFUSED_SHAPES = [dict(B=0), dict(Nsrc=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(C=0), dict(C=5), dict(Hs=8193), dict(Ws=8193),
                  dict(H=8193, p=1), dict(W=8193, p=1), dict(p=0), dict(p=3), dict(H=12, p=8), dict(index=None, B=6),
                  dict(Nsrc=1 << 20, Hs=8192, Ws=8192), dict(B=1 << 20, H=8192, W=8192)]
REFUSED_ARGS = [dict(src=None), dict(box=None), dict(mean=None), dict(std=None), dict(patches=None, image=None)]


@pytest.mark.parametrize("bad", REFUSED_SHAPES, ids=str)
def test_shape_refusals_come_first(L, bad):
    assert _resize(L, **bad) == SHAPE
    assert _resize(L, src=None, box=None, **bad) == SHAPE


def test_argument_refusals_and_what_is_legal(L):
    for bad in REFUSED_ARGS:
        assert _resize(L, **bad) == ARG, bad
    assert _resize(L, patches=None, p=3, src=None) == ARG                # p is not looked at without patch rows: the NULL src answers
    assert _resize(L, H=64, W=40, src=None) == ARG                       # an output larger than the source is a legal shape


# ---------------------------------------------------------------------------------------------- what the poison test demands of vitamd/
def test_no_new_empty_site_and_the_pinned_sites_stand():
    sites = P.empty_sites()
    assert not [s for s in sites if s[0] == "resize.py"]
    assert PINNED_SITES <= sites
    with open(os.path.join(P.PKG_DIR, "ops.py")) as f:
        lines = f.read().splitlines()
    prep = [n for n in range(len(lines)) if lines[n].startswith("def frames_prep(")][0]
    end = [n for n in range(prep + 1, len(lines)) if lines[n].startswith("def ")][0]
    inside = sorted(s[1] for s in sites if s[0] == "ops.py" and prep < s[1] <= end)
    assert len(inside) == 2                                              # the two output allocations frames_prep had: the resize form adds none


def test_the_loader_hook_follows_next_and_resized_frames_is_a_frames():
    import inspect
    from vitamd import data, resize
    lines = {name: inspect.getsourcelines(getattr(data.DeviceLoader, name))[1] for name in ("__next__", "_frames", "_labels", "_geom", "_feed")}
    assert lines["_feed"] < lines["__next__"] < lines["_frames"] < lines["_labels"] < lines["_geom"]
    assert resize.ResizeLoader._geom is not data.DeviceLoader._geom and resize.ResizeLoader._check is not data.DeviceLoader._check
    assert issubclass(resize.ResizedFrames, data.Frames)
    # the subclass takes its own route through the kernels, and the bookkeeping around it is the one of Frames
    assert resize.ResizedFrames.materialise is data.Frames.materialise and resize.ResizedFrames._launch is not data.Frames._launch
