"""Mixing resized samples in one launch (vitamd_frames_prep_resize_mix, vitamd.mix.MixedResizedFrames / ResizeMixLoader) without a GPU:
the binding of the new entry point and its refusals, the refusals of the new op, class and loader before any device is looked at, the
two refusals the earlier routes keep, proof that the checks of test_gpu_resize_mix.py bite (every planted mistake of
_resize_mix_ref.standin is reported at that file's cases, the clean stand-in is not), and the conditions tests/test_gpu_poison.py
puts on new code in vitamd/."""
import ctypes
import functools
import os

import pytest
import torch

import _abi
import _poison as P
import _resize_mix_ref as RM
import _resize_ref as R
from test_gpu_poison import NOT_REACHED             # imports without a device: only its tests need one

SHAPE, ARG = 1, 2
PARENT_SITES = 119                                   # len(_poison.site_spans()) on the commit this route was added to

_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


# ---------------------------------------------------------------------------------------------- the binding and the C refusals
def test_the_symbol_is_bound_with_the_headers_argument_count(L):
    from vitamd import lib
    declared, _ = _abi.declared()
    name = "vitamd_frames_prep_resize_mix"
    assert declared[name] == 18 == len(lib.SIGNATURES[name]) == declared["vitamd_frames_prep_resize"] + 2
    fn = getattr(L, name)
    assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION          # additive: the ABI number stands


def _entry(L, src=PTR, index=PTR, box=PTR, mean=PTR, std=PTR, patches=PTR, image=PTR, B=3, Nsrc=5, Hs=11, Ws=13, C=3, H=16, W=16, p=4, rec=PTR,
           lam=PTR):
    return L.vitamd_frames_prep_resize_mix(src, index, box, mean, std, patches, image, B, Nsrc, Hs, Ws, C, H, W, p, rec, lam, None)


def test_the_refusals_are_those_of_the_resizing_entry_and_a_null_rec(L):
    """nothing is launched on a refusal: every pointer here is host memory or NULL"""
    from test_resize_host import REFUSED_ARGS, REFUSED_SHAPES
    for bad in REFUSED_SHAPES:
        assert _entry(L, **bad) == SHAPE, bad
        assert _entry(L, src=None, box=None, rec=None, **bad) == SHAPE, bad      # the shape answers first
    for bad in REFUSED_ARGS + [dict(rec=None), dict(rec=None, lam=None)]:
        assert _entry(L, **bad) == ARG, bad
    assert _entry(L, lam=None, src=None) == ARG                          # a NULL lam is legal: the NULL src answers
    assert _entry(L, H=64, W=40, src=None) == ARG                        # an output larger than the source is a legal shape


# ---------------------------------------------------------------------------------------------- the Python refusals
def test_arguments_are_refused_before_any_device_is_looked_at():
    from vitamd import lib, mix, ops, resize
    u8 = torch.zeros((4, 11, 13, 3), dtype=torch.uint8)
    box = resize.resize_center_boxes(4, (11, 13), 16, 16)
    rec, lam = mix.Mix().draw(4, 16, 0)
    op = lambda **kw: ops.frames_prep_resize_mix(**{**dict(src=u8, out_hw=(16, 16), patch=4, image=True, index=None, box=box, mean=None,
                                                           std=None, rec=rec, lam=lam), **kw})
    for bad, match in ((dict(src=u8.float()), "uint8"), (dict(patch=None, image=False), "nothing to write"), (dict(index=torch.zeros((2, 2))), "index"),
                       (dict(mean=torch.zeros(3)), "mean and std"), (dict(patch=5), "patch"), (dict(src=u8[:, :, :, :0]), "C in"),
                       (dict(out_hw=(9000, 16), patch=None), "8192"), (dict(box=None), "box"), (dict(rec=None), "rec"),
                       (dict(index=torch.zeros(5, dtype=torch.int64), src=u8[:0]), ">= 1")):
        with pytest.raises(ValueError, match=match):
            op(**bad)
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        op()                                                              # legal arguments: only now is a device asked for
    frames = lambda **kw: mix.MixedResizedFrames(**{**dict(src_u8=u8, size=16, box=box, mix=(rec, lam)), **kw})
    for bad in (dict(mix=rec), dict(mix=(rec[:3], lam)), dict(mix=(rec.long(), lam)), dict(mix=(rec, lam.double())), dict(mix=(rec, lam[:3])),
                dict(mix=(rec, None)), dict(box=box[:3]), dict(mean=(0.5, 0.5, 0.5)), dict(src_u8=u8.float())):
        with pytest.raises(ValueError):
            frames(**bad)
    with pytest.raises(TypeError):
        mix.MixedResizedFrames(u8, 16, box)                               # mix is required
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        frames()
    loader = lambda *a, **kw: mix.ResizeMixLoader(iter([]), *a, **kw)
    for call in (lambda: loader("cuda", 16, object()), lambda: loader("cuda", 16, mix.Mix(), mode="bicubic"), lambda: loader("cpu", 16, mix.Mix()),
                 lambda: loader("cuda", 16, mix.Mix(), resize_to=0), lambda: loader("cuda", 16, mix.Mix(), patch=5),
                 lambda: loader("cuda", 16, mix.Mix(), depth=1)):
        with pytest.raises(ValueError):
            call()
    for labels in (None, torch.zeros(4, dtype=torch.int32), torch.zeros((4, 1), dtype=torch.int64), [0, 1, 2, 3]):
        ld = mix.ResizeMixLoader(iter([(u8, labels)]), "cuda", 16, mix.Mix())
        with pytest.raises(ValueError, match="int64 labels"):
            next(ld)                                                      # refused by _check, before the copy stream exists
        assert ld._copy_stream is None
    ld = mix.ResizeMixLoader(iter([(u8, torch.zeros(4, dtype=torch.int64), torch.tensor([[12, 13]] * 4, dtype=torch.int32))]), "cuda", 16, mix.Mix())
    with pytest.raises(ValueError, match="extent"):
        next(ld)
    assert ld._copy_stream is None


def test_the_two_refusals_of_the_earlier_routes_still_hold():
    from vitamd import mix, ops, resize
    u8 = torch.zeros((4, 11, 13, 3), dtype=torch.uint8)
    box = resize.resize_center_boxes(4, (11, 13), 16, 16)
    with pytest.raises(ValueError, match="not both"):
        ops.frames_prep(u8, (16, 16), None, 4, True, mix=(box, None), resize=(box, None, None))
    for kw in (dict(mode="rrc"), dict(scale=(0.5, 1.0)), dict(ratio=(1.0, 1.0)), dict(resize_to=18)):
        with pytest.raises(ValueError, match="ResizeMixLoader"):
            mix.MixLoader(iter([]), "cuda", 16, mix.Mix(), **kw)


def test_the_loader_overrides_the_hooks_it_must_and_the_classes_stand_where_their_bases_stand():
    from vitamd import data, mix, resize
    RL, ML = resize.ResizeLoader, mix.ResizeMixLoader
    assert issubclass(ML, RL) and issubclass(mix.MixedResizedFrames, resize.ResizedFrames) and issubclass(mix.MixedResizedFrames, data.Frames)
    assert ML._frames is not RL._frames and ML._labels is not RL._labels and ML._check is not RL._check
    assert ML._staged is RL._staged and ML.boxes is RL.boxes and ML._geom is RL._geom and ML.__next__ is data.DeviceLoader.__next__
    # the subclass takes its own route through the kernels, and the bookkeeping around it is the one of Frames
    assert mix.MixedResizedFrames.materialise is data.Frames.materialise
    assert mix.MixedResizedFrames._launch is not resize.ResizedFrames._launch and mix.MixedResizedFrames._launch is not mix.MixedFrames._launch
    ld = ML(iter([]), "cuda", 16, mix.Mix(), depth=3)
    assert ld._mix_stage is not ld._stage and len(ld._mix_stage) == len(ld._stage) == 3      # a staging list of its own
    assert isinstance(mix.MixedResizedFrames.mix, property)


# ---------------------------------------------------------------------------------------------- what the poison test demands of vitamd/
def test_no_new_empty_site_and_the_not_reached_sites_stand():
    spans = P.site_spans()
    assert len(spans) <= PARENT_SITES
    assert len(NOT_REACHED) == 5 and set(NOT_REACHED) <= set(spans)
    assert not [s for s in spans if s[0] in ("mix.py", "resize.py")]
    src = open(os.path.join(P.PKG_DIR, "ops.py")).read()
    body = src[src.index("def frames_prep_resize_mix("):src.index("def crop_flip_draw(")]
    assert "torch.empty" not in body and "frames_prep(" in body           # the outputs are those of frames_prep, whose sites the workloads reach


# ---------------------------------------------------------------------------------------------- the checks bite
CASES = [(c, r) for c in RM.CASE_NAMES for r in RM.record_names(c)]


@functools.lru_cache(maxsize=None)
def _clean(case, norm):
    """per case: the stand-alone fp32 images of the clean stand-in, the float64 images; computed once, never written to"""
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[case]
    src, index, box = RM.case(case)
    mean, std = (R.MEAN[:C], R.STD[:C]) if norm else (None, None)
    return R.standin(src, (H, W), index, box, mean, std)[0], R.resize_ref(src, (H, W), index, box, mean, std)


def _findings(case, rname, norm, bug):
    """the GPU test's two checks of the image on the stand-in's output -> (bit failures, bound failures)"""
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[case]
    src, index, box = RM.case(case)
    rec, lam = RM.record(rname, H, W)
    mean, std = (R.MEAN[:C], R.STD[:C]) if norm else (None, None)
    alone, ref_images = _clean(case, norm)
    got, rows = RM.standin(src, (H, W), index, box, rec, lam, mean, std, p=p, bug=bug)
    want = RM.mixed_resized_ref(src, (H, W), index, box, rec, lam, mean, std, images=alone)
    ref = RM.mixed_resized_ref(src, (H, W), index, box, rec, lam, mean, std)
    bnd = RM.bounds(src.shape, (H, W), box, rec, lam, ref_images, std)
    assert not R.check_rows(rows, got, p, case)
    return RM.check_bits(got, want, case), R.check_image(got, ref, bnd, case)


@pytest.mark.parametrize("norm", [False, True], ids=["unit", "norm"])
@pytest.mark.parametrize("case,rname", CASES)
def test_the_clean_standin_passes_both_checks(case, rname, norm):
    bits, bound = _findings(case, rname, norm, None)
    assert not bits and not bound


def test_the_float64_reference_is_the_composition_and_the_record_cases_are_what_they_claim():
    for case in RM.CASE_NAMES:
        src, index, box = RM.case(case)
        assert box[:, 8].tolist() != R.case(case)[2][:, 8].tolist()
        assert all(box[b, 8] != box[4 - b, 8] for b in (0, 1))              # of every pair one sample is flipped
    H, W = R.CASES["b40x36_p4"][4:6]
    yl, yh, xl, xh = RM.EXTRA_BOXES["cut_cover"]
    assert yl == 0 and xl == 0 and yh >= 32 and xh >= 32 and 32 < yh < H and 32 < xh < W      # tile (0, 0) wholly, the others cut
    yl, yh, xl, xh = RM.EXTRA_BOXES["cut_touch"]
    assert (yh, xh) == (33, 33) and yl < 32 and xl < 32                     # tile (1, 1) by the single pixel (32, 32)
    rec, lam = RM.record("mixed", 16, 16)
    assert rec[:, 0].tolist() == [4, 3, 2, 1, 0] and set(rec[:, 1].tolist()) == {0, 1, 2}
    src, index, box = RM.case("a16_p4")
    a = RM.mixed_resized_ref(src, (16, 16), index, box, rec, lam)
    images = R.resize_ref(src, (16, 16), index, box)
    assert a.dtype == torch.float64 and torch.equal(a[2], images[2])       # its own partner
    l = float(lam[0])
    assert torch.allclose(a[0], l * images[0] + (1 - l) * images[4], rtol=0, atol=1e-15)
    assert torch.equal(a[1, :, :, 1:6], images[3][:, :, 1:6]) and torch.equal(a[1, :, :, 6:], images[1][:, :, 6:])


# bug -> the (case, record) on which it must show
WHERE = {"partner_receiver_box": ("a16_p4", "mixup"), "partner_receiver_flip": ("a16_p4", "cut_b"), "box_inclusive": ("w14_p7", "mixed"),
         "lam_swapped": ("b16_p4", "mixup"), "fma": ("a16_p4", "mixup"), "blend_before_norm": ("c4_p4", "mixup"),
         "skip_touching_tile": ("b40x36_p4", "cut_touch")}


@pytest.mark.parametrize("bug", RM.BUGS)
def test_every_planted_mistake_is_caught_by_the_bit_check_or_the_bound(bug):
    assert set(WHERE) == set(RM.BUGS)
    case, rname = WHERE[bug]
    bits, bound = _findings(case, rname, True, bug)
    print(bug, "bits:", bits, "bound:", bound)
    assert bits or bound
    if bug in ("partner_receiver_box", "partner_receiver_flip", "box_inclusive", "lam_swapped", "skip_touching_tile"):
        assert bits and bound                        # a wrong pixel, not a rounding: both see it
