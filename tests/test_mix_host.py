"""Mixup / CutMix / label smoothing without a GPU: the host-side draw (vitamd.mix.Mix), the binding of the new entry points and their
refusals, proof that the checks of test_gpu_mix.py bite (every planted mistake of _mix_ref.standin fails at the shapes that file
uses), and the conditions tests/test_gpu_poison.py puts on new code in vitamd/."""
import ctypes
import os

import pytest
import torch

import _abi
import _mix_ref as R
import _poison as P

SHAPE, ARG = 1, 2
NEW_SYMBOLS = {"vitamd_frames_prep_mix": 17, "vitamd_soft_cross_entropy_fwd": 13, "vitamd_soft_cross_entropy_bwd": 16}
PINNED_SITES = {("ops.py", 137), ("functions.py", 182), ("data.py", 229), ("data.py", 230), ("data.py", 243)}

_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


# ---------------------------------------------------------------------------------------------- the draw
def _mix(**kw):
    from vitamd import mix
    return mix.Mix(**kw)


@pytest.mark.parametrize("per_sample", [False, True])
def test_draw_is_a_function_of_seed_and_step(per_sample):
    m = _mix(per_sample=per_sample, seed=5)
    rec, lam = m.draw(16, (8, 12), 3)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (16, 6) and lam.dtype == torch.float32 and tuple(lam.shape) == (16,)
    again = m.draw(16, (8, 12), 3)
    assert torch.equal(rec, again[0]) and torch.equal(lam, again[1])
    same_seed = _mix(per_sample=per_sample, seed=5).draw(16, (8, 12), 3)
    assert torch.equal(rec, same_seed[0]) and torch.equal(lam, same_seed[1])
    others = [m.draw(16, (8, 12), s) for s in (4, 5, (1 << 32) + 3)] + [_mix(per_sample=per_sample, seed=6).draw(16, (8, 12), 3)]
    assert all(not (torch.equal(rec, r) and torch.equal(lam, l)) for r, l in others)
    assert rec[:, 0].tolist() == list(range(15, -1, -1))                 # the partner is the reversal


@pytest.mark.parametrize("hw", [(8, 8), (7, 13), (224, 224)], ids=str)
def test_boxes_lie_inside_the_image_and_lam_is_the_kept_area(hw):
    H, W = hw
    m = _mix(per_sample=True, seed=1)
    seen = set()
    for step in range(40):
        rec, lam = m.draw(8, hw, step)
        for (q, mode, yl, yh, xl, xh), l in zip(rec.tolist(), lam):
            seen.add(mode)
            assert mode in (1, 2)                                        # prob = 1 with both alphas: every row is mixed
            if mode == 1:
                assert (yl, yh, xl, xh) == (0, 0, 0, 0) and 0.0 <= float(l) <= 1.0
            else:
                assert 0 <= yl <= yh <= H and 0 <= xl <= xh <= W
                want = torch.tensor(1.0 - (yh - yl) * (xh - xl) / (H * W), dtype=torch.float64).to(torch.float32)
                assert torch.equal(l, want)
    assert seen == {1, 2}


def test_draw_modes_follow_the_switches():
    rec, lam = _mix(prob=0.0).draw(6, 8, 0)
    assert rec[:, 1].tolist() == [0] * 6 and lam.tolist() == [1.0] * 6 and rec[:, 2:].abs().sum() == 0
    rec, lam = _mix(mixup_alpha=0.0, cutmix_alpha=0.0).draw(6, 8, 0)
    assert rec[:, 1].tolist() == [0] * 6 and lam.tolist() == [1.0] * 6
    for step in range(8):
        assert set(_mix(cutmix_alpha=0.0, per_sample=True).draw(8, 8, step)[0][:, 1].tolist()) == {1}
        assert set(_mix(mixup_alpha=0.0, per_sample=True).draw(8, 8, step)[0][:, 1].tolist()) == {2}
        assert set(_mix(switch_prob=1.0, per_sample=True).draw(8, 8, step)[0][:, 1].tolist()) == {2}
        assert set(_mix(switch_prob=0.0, per_sample=True).draw(8, 8, step)[0][:, 1].tolist()) == {1}
    modes = torch.cat([_mix(prob=0.5, per_sample=True, seed=2).draw(64, 8, s)[0][:, 1] for s in range(4)])
    assert {0, 1, 2} == set(modes.tolist()) and 64 < int((modes == 0).sum()) < 192          # about half of 256 rows stay unmixed


def test_one_decision_per_batch_is_replicated_to_every_row():
    for step in range(6):
        rec, lam = _mix(per_sample=False, seed=9).draw(7, (8, 8), step)
        assert all(torch.equal(rec[b, 1:], rec[0, 1:]) for b in range(7)) and bool((lam == lam[0]).all())
    rec, lam = _mix(per_sample=True, seed=9).draw(64, (8, 8), 0)
    assert len({tuple(r) for r in rec[:, 1:].tolist()}) > 8


def test_mix_refuses_bad_arguments():
    from vitamd import mix
    for kw in (dict(mixup_alpha=-1.0), dict(cutmix_alpha=float("nan")), dict(prob=1.5), dict(switch_prob=-0.1), dict(label_smoothing=2.0),
               dict(seed=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            mix.Mix(**kw)
    with pytest.raises(ValueError):
        mix.Mix().draw(0, 8, 0)
    with pytest.raises(ValueError):
        mix.Mix().draw(4, 8, -1)
    with pytest.raises(ValueError):
        mix.SoftTargetLoss(1.5)
    with pytest.raises(ValueError, match="vitamd.mix.Mix"):
        mix.MixLoader(iter([]), "cuda", 8, object())


# ---------------------------------------------------------------------------------------------- the binding and the refusals
def test_new_symbols_are_bound_with_the_headers_argument_counts(L):
    from vitamd import lib
    declared, _ = _abi.declared()
    for name, n in NEW_SYMBOLS.items():
        assert declared[name] == n == len(lib.SIGNATURES[name]), name
        fn = getattr(L, name)
        assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION


def _prep_mix(L, src=PTR, table=PTR, patches=PTR, image=PTR, rec=PTR, lam=PTR, B=3, Nsrc=5, Hs=11, Ws=13, C=3, H=8, W=8, p=4):
    return L.vitamd_frames_prep_mix(src, PTR, PTR, table, patches, image, B, Nsrc, Hs, Ws, C, H, W, p, rec, lam, None)


def test_prep_mix_refusals_are_those_of_frames_prep_plus_the_record(L):
    for bad in (dict(B=0), dict(C=5), dict(H=12), dict(p=3), dict(Hs=0)):
        assert _prep_mix(L, **bad) == SHAPE
        assert _prep_mix(L, rec=None, src=None, **bad) == SHAPE                # the shape answers first
    assert _prep_mix(L, rec=None) == ARG
    assert _prep_mix(L, src=None) == ARG and _prep_mix(L, table=None) == ARG and _prep_mix(L, patches=None, image=None) == ARG


def _soft_fwd(L, logits=PTR, ya=PTR, yb=PTR, lam=PTR, e=0.1, loss_row=PTR, lse=PTR, stats=PTR, M=4, V=10, ld=10):
    return L.vitamd_soft_cross_entropy_fwd(logits, 0, ya, yb, lam, e, loss_row, lse, stats, M, V, ld, None)


def _soft_bwd(L, logits=PTR, ya=PTR, yb=PTR, lam=PTR, e=0.1, lse=PTR, stats=PTR, out=PTR + 64, out_bf16=0, M=4, V=10, ld=10, ldo=10):
    return L.vitamd_soft_cross_entropy_bwd(logits, 0, ya, yb, lam, e, lse, stats, None, out, out_bf16, M, V, ld, ldo, None)


def test_soft_cross_entropy_refusals(L):
    for bad in (dict(M=0), dict(V=1), dict(V=65537, ld=65537), dict(ld=9)):
        assert _soft_fwd(L, **bad) == SHAPE and _soft_fwd(L, logits=None, **bad) == SHAPE
        assert _soft_bwd(L, **bad) == SHAPE
    assert _soft_bwd(L, ldo=9) == SHAPE
    for bad in (dict(logits=None), dict(ya=None), dict(loss_row=None), dict(lse=None), dict(stats=None), dict(yb=None),      # lam without target_b
                dict(e=-0.1), dict(e=1.5), dict(e=float("nan"))):
        assert _soft_fwd(L, **bad) == ARG, bad
    for bad in (dict(logits=None), dict(ya=None), dict(lse=None), dict(stats=None), dict(out=None), dict(yb=None), dict(e=2.0),
                dict(out=PTR, out_bf16=1), dict(out=PTR, ldo=12)):                                                          # in place: same type and stride
        assert _soft_bwd(L, **bad) == ARG, bad


def test_python_wrappers_refuse_before_any_device_work():
    from vitamd import lib, lm, mix, ops
    x, y = torch.zeros((4, 10)), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        lm.soft_cross_entropy(x, y, smoothing=0.1)
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        mix.SoftTargetLoss(0.1)(x, mix.MixedLabels(y, y, torch.ones(4)))
    with pytest.raises(ValueError, match="soft"):
        ops._need_soft((None, None), 4)
    with pytest.raises(ValueError, match="smoothing"):
        ops._need_soft((None, None, 1.5), 4)
    u8 = torch.zeros((4, 11, 13, 3), dtype=torch.uint8)
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        mix.MixedFrames(u8, 8, mix=mix.Mix().draw(4, 8, 0))


# ---------------------------------------------------------------------------------------------- the checks bite
def _frames(geom_name, B, rec_name, bug=None):
    Nsrc, Hs, Ws, C, H, W, p = R.GEOMS[geom_name]
    src, index, geom = R.frames_case(geom_name, B)
    rec, lam = R.record(rec_name, B, H, W)
    return R.standin("frames", src, (H, W), index, geom, rec, lam, R.MEAN[:C], R.STD[:C], bug=bug)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("bug,rec_names", [("partner_receiver_geom", ("mixup", "cut_a", "mixed")), ("box_inclusive", ("cut_a", "cut_b", "mixed")),
                                           ("lam_swapped", ("mixup", "mixed")), ("fma", ("mixup", "mixed"))])
@pytest.mark.parametrize("geom_name", list(R.GEOMS))
def test_every_planted_prep_mistake_changes_the_bits(geom_name, bug, rec_names):
    """the comparison test_gpu_mix.py makes (equal bits with mixed_frames_ref) fails for each mistake at every geometry of that file, in
    every record that exercises the mistaken step, at B = 4 (and B = 3 wherever a mixed pair exists there)"""
    for rec_name in rec_names:
        clean, broken = _frames(geom_name, 4, rec_name), _frames(geom_name, 4, rec_name, bug)
        assert not torch.equal(_bits(clean), _bits(broken)), (rec_name, bug)
    assert not torch.equal(_bits(_frames(geom_name, 3, rec_names[0])), _bits(_frames(geom_name, 3, rec_names[0], bug)))
    assert torch.equal(_bits(_frames(geom_name, 4, "none")), _bits(_frames(geom_name, 4, "none", bug)))        # nothing mixed, nothing to get wrong


def test_unmixed_rows_and_own_partners_are_the_plain_frames():
    import _data_ref as D
    for geom_name in R.GEOMS:
        Nsrc, Hs, Ws, C, H, W, p = R.GEOMS[geom_name]
        src, index, geom = R.frames_case(geom_name, 3)
        plain = D.frames_ref(src, (H, W), index, geom, R.MEAN[:C], R.STD[:C])
        assert torch.equal(_bits(_frames(geom_name, 3, "none")), _bits(plain))
        for rec_name in R.RECORDS:
            assert torch.equal(_bits(_frames(geom_name, 3, rec_name)[1]), _bits(plain[1]))       # the middle sample is its own partner
        whole = _frames(geom_name, 4, "cut_a")                                                    # row 1 of cut_a: the whole image is the partner's
        src4, index4, geom4 = R.frames_case(geom_name, 4)
        assert torch.equal(_bits(whole[1]), _bits(D.frames_ref(src4, (H, W), index4, geom4, R.MEAN[:C], R.STD[:C])[2]))


def test_wild_records_clamp_to_tame_ones():
    B, H, W = 4, 8, 8
    wild = torch.tensor([[-3, 2, R.I32_MIN, R.I32_MAX, R.I32_MIN, R.I32_MAX], [B + 5, 1, 0, 0, 0, 0], [1, 7, 0, 8, 0, 8],
                         [0, 2, 2, R.I32_MAX, R.I32_MIN, 5]], dtype=torch.int32)
    assert R.clamp_rec(wild, B, H, W) == [(0, 0, 0, 8, 0, 8), (3, 1, 0, 0, 0, 0), (1, 0, 0, 8, 0, 8), (0, 2, 2, 8, 0, 5)]


CE_SHAPES = [(5, 2), (5, 1001), (5, 4104), (1, 1001)]


@pytest.mark.parametrize("M,V", CE_SHAPES)
def test_the_clean_loss_standin_is_within_the_bound(M, V):
    x, ya, yb, lam = R.ce_case(M, V)
    for kw in (dict(yb=yb, lam=lam, smoothing=0.1), dict(yb=yb, lam=lam, smoothing=0.0), dict(smoothing=0.1), dict()):
        ref, t32 = R.soft_ce_ref(x, ya, grad_out=0.5, **kw), R.soft_ce_torch32(x, ya, grad_out=0.5, **kw)
        assert not R.check_cross_entropy(R.standin("ce", x, ya, grad_out=0.5, **kw), ref, t32, f"M={M} V={V} {sorted(kw)}")


@pytest.mark.parametrize("bug", R.CE_BUGS)
@pytest.mark.parametrize("M,V", CE_SHAPES)
def test_every_planted_loss_mistake_fails_the_bound(M, V, bug):
    x, ya, yb, lam = R.ce_case(M, V)
    kw = dict(yb=yb, lam=lam, smoothing=0.1, grad_out=0.5)
    ref, t32 = R.soft_ce_ref(x, ya, **kw), R.soft_ce_torch32(x, ya, **kw)
    fails = R.check_cross_entropy(R.standin("ce", x, ya, bug=bug, **kw), ref, t32, f"M={M} V={V} {bug}")
    assert fails, bug
    hit = {f.split(":")[0].split()[-1] for f in fails}
    assert {"smooth_ya_only": "loss_row", "no_sum_x": "loss_row", "grad_no_yb": "grad", "mean_wrong_count": "mean"}[bug] in hit


def test_the_soft_reference_at_its_anchor_is_the_hard_reference():
    """smoothing 0 and no lam: the float64 soft reference equals _lm_ref.cross_entropy_ref, and lam = 1 / ya == yb fold as the header says"""
    import _lm_ref as LR
    x, ya, yb, lam = R.ce_case(5, 1001)
    soft, hard = R.soft_ce_ref(x, ya), LR.cross_entropy_ref(x, ya)
    for k in ("loss_row", "lse", "mean", "grad"):
        assert torch.equal(soft[k], hard[k]), k
    ones = R.soft_ce_ref(x, ya, yb, torch.ones(5), 0.0)
    assert torch.allclose(ones["loss_row"], hard["loss_row"], rtol=0, atol=1e-12)
    same = R.soft_ce_ref(x, ya, ya, lam, 0.0)                                 # ya == yb adds the two weights
    assert torch.allclose(same["loss_row"], hard["loss_row"], rtol=0, atol=1e-12)
    t = R.soft_target(1001, ya, yb, lam, 0.1)
    assert torch.allclose(t.sum(-1), torch.ones(5, dtype=torch.float64), rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------- what the poison test demands of vitamd/
def test_no_new_empty_site_and_the_pinned_sites_stand():
    sites = P.empty_sites()
    assert not [s for s in sites if s[0] == "mix.py"]
    # lm.py keeps the one allocation it had (the fused head's weight gradient, reached by the poison workloads); the new autograd
    # function adds none
    lm_sites = [s for s in sites if s[0] == "lm.py"]
    assert len(lm_sites) == 1
    with open(os.path.join(P.PKG_DIR, "lm.py")) as f:
        assert "dW = torch.empty(tuple(weight.shape)" in f.read().splitlines()[lm_sites[0][1] - 1]
    assert PINNED_SITES <= sites


def test_device_loader_hooks_follow_next():
    """DeviceLoader.__next__ takes its Frames and labels from two methods defined after it, so that nothing above it moved"""
    import inspect
    from vitamd import data, mix
    lines = {name: inspect.getsourcelines(getattr(data.DeviceLoader, name))[1] for name in ("__next__", "_frames", "_labels", "_feed")}
    assert lines["_feed"] < lines["__next__"] < lines["_frames"] < lines["_labels"]
    assert mix.MixLoader._frames is not data.DeviceLoader._frames and mix.MixLoader._labels is not data.DeviceLoader._labels
    assert issubclass(mix.MixedFrames, data.Frames)
    # the subclass takes its own route through the kernels, and the bookkeeping around it is the one of Frames
    assert mix.MixedFrames.materialise is data.Frames.materialise and mix.MixedFrames._launch is not data.Frames._launch
