"""Random Erasing without a GPU: the binding of the two new entry points and their refusals, the host-side draw (vitamd.erase.Erase)
against its restatement and its expectation, the reference noise against the caps the GPU test applies to the kernel, proof that the
checks of test_gpu_erase.py bite (every planted mistake of _erase_ref fails them), and the two mixins on stub classes."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _abi
import _erase_ref as R
import _poison as P

SHAPE, ARG = 1, 2
NEW_SYMBOLS = {"vitamd_frames_erase": 13, "vitamd_frames_erase_grid_cap": 0}

_buf = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_buf)


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


def _erase(**kw):
    from vitamd import erase
    return erase.Erase(**kw)


# ---------------------------------------------------------------------------------------------- the binding and the refusals
def test_new_symbols_are_declared_exported_and_bound_with_the_headers_argument_counts(L):
    from vitamd import lib
    declared, _ = _abi.declared()
    for name, n in NEW_SYMBOLS.items():
        assert declared[name] == n == len(lib.SIGNATURES[name]), name
        fn = getattr(L, name)
        assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    assert L.vitamd_frames_erase_grid_cap() >= 1


def _call(L, patches=PTR, image=PTR, B=3, C=3, H=8, W=8, p=4, rec=PTR, fill=PTR, K=1):
    return L.vitamd_frames_erase(patches, image, B, C, H, W, p, rec, fill, K, 0, 0, None)


def test_frames_erase_refusals_come_before_any_launch(L):
    """the host pointers here would fault a launch: every call must be answered before one"""
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=5), dict(K=0), dict(K=9), dict(p=0), dict(p=3), dict(H=12, W=8, p=8),
                dict(B=1 << 20, H=1 << 11, W=1 << 11, p=1), dict(B=1 << 30, C=1, H=1, W=1, p=1), dict(B=1, C=4, H=(1 << 30) + 4, W=4, p=4)):
        assert _call(L, **bad) == SHAPE, bad
        assert _call(L, rec=None, **bad) == SHAPE, bad                       # the shape answers first
    assert _call(L, patches=None, p=0, B=0) == SHAPE
    assert _call(L, rec=None) == ARG and _call(L, patches=None, image=None) == ARG
    assert _call(L, patches=None, image=None, p=3) == ARG                    # p is only looked at with patch rows


def test_ops_frames_erase_refuses_before_any_device_work():
    from vitamd import lib, ops
    rec, fill = torch.zeros((2, 1, 5), dtype=torch.int32), torch.zeros((2, 1, 4))
    img, rows = torch.zeros((2, 3, 8, 8)), torch.zeros((2 * 4, 3 * 16), dtype=torch.bfloat16)
    for bad in (dict(patches=None, image=None), dict(rec=rec.long()), dict(rec=rec[:, 0]), dict(rec=torch.zeros((2, 9, 5), dtype=torch.int32)),
                dict(rec=torch.zeros((2, 1, 6), dtype=torch.int32)), dict(fill=fill[:1]), dict(fill=fill.double()), dict(seed=-1), dict(step=1 << 64),
                dict(seed=True), dict(patch=3), dict(patch=None), dict(image=img[:1]), dict(image=torch.zeros((2, 5, 8, 8))), dict(image=None),
                dict(image=None, hw=(8, 0)), dict(hw=(8, 4)), dict(patches=rows[:4]), dict(patches=torch.zeros((8, 40), dtype=torch.bfloat16)),
                dict(patches=torch.zeros((8, 16), dtype=torch.bfloat16))):
        kw = dict(patches=rows, image=img, patch=4, rec=rec, fill=fill, seed=0, step=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.frames_erase(**kw)
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        ops.frames_erase(rows, img, 4, rec, fill, 0, 0)
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        ops.frames_erase(None, img, None, rec, None, 0, 0)


def test_erase_refuses_bad_arguments():
    from vitamd import erase
    for kw in (dict(probability=-0.1), dict(probability=1.5), dict(probability=float("nan")), dict(probability=True), dict(min_area=0.0),
               dict(min_area=0.5, max_area=0.4), dict(max_area=1.5), dict(min_aspect=0.0), dict(min_aspect=-1.0), dict(min_aspect=2.0, max_aspect=1.0),
               dict(max_aspect=float("inf")), dict(mode="noise"), dict(mode=None), dict(min_count=0), dict(max_count=9), dict(min_count=3, max_count=2),
               dict(min_count=1.0), dict(seed=-1), dict(seed=1 << 64), dict(seed=0.0)):
        with pytest.raises(ValueError):
            erase.Erase(**kw)
    e = erase.Erase()
    assert (e.probability, e.min_area, e.max_area, e.min_aspect, e.mode, e.min_count, e.max_count) == (0.25, 0.02, 1 / 3, 0.3, "pixel", 1, 1)
    assert e.max_aspect == 1 / 0.3 and e.enabled and not erase.Erase(probability=0).enabled
    for bad in ((0, 8, 0), (4, 8, -1), (4, 0, 0), (True, 8, 0), (4, 8, 1 << 64)):
        with pytest.raises(ValueError):
            e.draw(*bad)
    for cls, args in ((erase.EraseLoader, ()), (erase.EraseResizeLoader, ()), (erase.EraseMixLoader, (object(),)), (erase.EraseResizeMixLoader, (object(),))):
        with pytest.raises(ValueError, match="vitamd.erase.Erase"):
            cls(iter([]), "cuda", 8, *args, erase=object())
        with pytest.raises(TypeError):
            cls(iter([]), "cuda", 8, *args)                                 # erase= is keyword-only and has no default


# ---------------------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("mode,counts", [("pixel", (1, 1)), ("rand", (1, 3)), ("const", (2, 2))])
def test_draw_is_a_function_of_seed_and_step_and_equals_its_restatement(mode, counts):
    kw = dict(probability=0.6, mode=mode, min_count=counts[0], max_count=counts[1])
    e = _erase(seed=5, **kw)
    rec, fill = e.draw(16, (24, 40), 3)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (16, counts[1], 5) and fill.dtype == torch.float32 and tuple(fill.shape) == (16, counts[1], 4)
    again = _erase(seed=5, **kw).draw(16, (24, 40), 3)
    assert torch.equal(rec, again[0]) and torch.equal(fill, again[1])
    others = [e.draw(16, (24, 40), s) for s in (4, (1 << 32) + 3)] + [_erase(seed=6, **kw).draw(16, (24, 40), 3)]
    assert all(not torch.equal(rec, r) for r, _ in others)
    ref_rec, ref_fill = R.draw_ref(16, (24, 40), 3, seed=5, **kw)
    assert rec.tolist() == ref_rec and torch.equal(fill, torch.tensor(ref_fill, dtype=torch.float64).to(torch.float32))
    want_mode = 2 if mode == "pixel" else 1
    assert set(rec[:, :, 0].reshape(-1).tolist()) == {0, want_mode}
    assert bool((fill != 0).any()) == (mode == "rand")
    per_sample = (rec[:, :, 0] != 0).sum(1)
    assert set(per_sample.tolist()) <= {0, *range(counts[0], counts[1] + 1)} and (counts[0] == counts[1] or len(set(per_sample.tolist())) > 2)


@pytest.mark.parametrize("hw", [(8, 8), (7, 13), (32, 32), (224, 224)], ids=str)
def test_boxes_lie_strictly_inside_the_image(hw):
    H, W = hw
    e = _erase(probability=1.0, max_count=2, seed=1)
    n = 0
    for step in range(20):
        for rows in e.draw(8, hw, step)[0].tolist():
            for mode, yl, yh, xl, xh in rows:
                if mode:
                    n += 1
                    assert mode == 2 and 0 <= yl < yh <= H and 0 <= xl < xh <= W and yh - yl < H and xh - xl < W
                else:
                    assert (yl, yh, xl, xh) == (0, 0, 0, 0)
    assert n > 100


def test_probability_switches_the_draw():
    rec, fill = _erase(probability=0.0).draw(64, 32, 0)
    assert int(rec.abs().sum()) == 0 and float(fill.abs().sum()) == 0
    for step in range(4):
        rec, _ = _erase(probability=1.0).draw(64, (32, 32), step)
        assert rec[:, 0, 0].tolist() == [2] * 64                              # a box per sample


def test_erased_share_and_mean_area_follow_the_restated_rule():
    """4 000 samples at probability 0.25, 224 x 224: the share of erased samples and the mean box area within 5 standard errors of what
    the restated rule gives (the reference draw first, then Erase.draw, which must also be the reference draw)"""
    hw, p, n = (224, 224), 0.25, 4000
    q, area_mean, area_std, n_mc = R.expected_box(hw)
    share = p * (1 - (1 - q) ** 10)
    rec_ref = [row for step in range(4) for row in R.draw_ref(n // 4, hw, step, seed=3)[0]]
    rec_got = [row for step in range(4) for row in _erase(seed=3).draw(n // 4, hw, step)[0].tolist()]
    for rec in (rec_ref, rec_got):
        boxes = [rows[0] for rows in rec if rows[0][0]]
        got_share = len(boxes) / n
        assert abs(got_share - share) < 5 * math.sqrt(share * (1 - share) / n), (got_share, share)
        areas = np.array([(yh - yl) * (xh - xl) for _, yl, yh, xl, xh in boxes], dtype=np.float64)
        se = area_std * math.sqrt(1 / len(boxes) + 1 / n_mc)
        assert abs(areas.mean() - area_mean) < 5 * se, (areas.mean(), area_mean, se)
    assert rec_got == rec_ref


def test_the_draw_is_apart_from_mix_draw_under_the_same_seed_and_step():
    """the two host generators: the same key, counters (0, 0, 0, 0) and (0, 0, 0, 2) - different first uniforms, so an erase decision
    never repeats the mix decision of its step"""
    for seed, step in ((0, 0), (7, 3), (1 << 40, 1 << 33)):
        key = np.array([seed, step], dtype=np.uint64)
        u_mix = np.random.Generator(np.random.Philox(key=key)).random()
        u_erase = np.random.Generator(np.random.Philox(key=key, counter=np.array([0, 0, 0, 2], dtype=np.uint64))).random()
        assert u_mix != u_erase
    # and Erase.draw is on the second stream: probability = that first uniform's successor decides sample 0
    from vitamd import mix
    u = np.random.Generator(np.random.Philox(key=np.array([9, 4], dtype=np.uint64), counter=np.array([0, 0, 0, 2], dtype=np.uint64))).random()
    assert _erase(probability=min(u + 1e-9, 1.0), seed=9).draw(1, 32, 4)[0][0, 0, 0] == 2
    assert _erase(probability=u, seed=9).draw(1, 32, 4)[0][0, 0, 0] == 0
    assert mix.Mix(seed=9).draw(1, 32, 4)[0].shape == (1, 6)


# ---------------------------------------------------------------------------------------------- the reference noise
def test_reference_noise_is_standard_normal_within_the_caps():
    z, r = R.noise_ref(0, 0, 0, 3, 64, 64)
    assert z.shape == (3, 64, 64) and R.moments_ok(z)
    assert np.abs(z).max() <= R.Z_MAX and (r >= 0).all() and (np.abs(z) <= r + 1e-12).all()
    assert not R.moments_ok(z * 1.1) and not R.moments_ok(z + 0.05)         # the caps bite
    # a function of (seed, step, b, c, y, x): another of any of them gives other values, and W only sets the row pitch of the counter
    for other in (R.noise_ref(1, 0, 0, 3, 64, 64), R.noise_ref(0, 1, 0, 3, 64, 64), R.noise_ref(0, 0, 1, 3, 64, 64), R.noise_ref(0, 1 << 32, 0, 3, 64, 64)):
        assert not np.array_equal(z, other[0])
    assert np.array_equal(R.noise_ref(0, 0, 0, 3, 64, 62)[0], R.noise_ref(0, 0, 0, 3, 64, 64)[0][:, :, :62])
    assert np.array_equal(R.noise_ref(0, 0, 0, 1, 64, 64)[0], z[:1])


# ---------------------------------------------------------------------------------------------- the checks bite
def _case():
    """the record of test_gpu_erase.py's fast form (B = 5, H = W = 32, K = 2)"""
    B, C, H, W = 5, 3, 32, 32
    g = torch.Generator().manual_seed(11)
    before = torch.randn((B, C, H, W), generator=g)
    rec = torch.tensor(R.FAST_RECORD, dtype=torch.int32)
    fill = torch.randn((B, 2, 4), generator=g)
    return before, rec, fill


def test_the_clean_reference_passes_its_own_check_and_every_planted_mistake_fails():
    before, rec, fill = _case()
    ref = R.erase_ref(before, rec, fill, 3, 9)
    clean = torch.from_numpy(ref["want"].astype(np.float32))
    fails, ratio = R.check_erased(clean, before, ref)
    assert not fails and ratio <= 1 / 6                  # fp32 rounding of the float64 value alone: half an ulp <= 2^-23 |z| <= 2^-23 r
    assert torch.equal(R.bits(clean[4]), R.bits(before[4])) and (ref["kind"][4] == 0).all()
    assert {0, 1, 2} == set(np.unique(ref["kind"]).tolist())
    for bug in R.BUGS:
        broken = torch.from_numpy(R.erase_ref(before, rec, fill, 3, 9, bug=bug)["want"].astype(np.float32))
        assert R.check_erased(broken, before, ref)[0], bug
    # a touched pixel outside, a wrong fill, noise one fp32 ulp-of-8 off: each is caught
    for kind, delta in ((0, 1e-3), (1, 1e-6), (2, 2e-5)):
        broken = clean.clone()
        idx = tuple(int(v[0]) for v in np.nonzero(ref["kind"] == kind))
        broken[idx] += delta
        assert R.check_erased(broken, before, ref)[0], kind


def test_winners_are_the_latest_box_per_pixel():
    rec = torch.tensor(R.FAST_RECORD, dtype=torch.int32)
    win = R.winners(rec, 32, 32)
    assert win[0, 12, 5] == 1 and win[0, 4, 5] == 0 and win[0, 12, 2] == 0 and win[0, 12, 7] == 1 and win[0, 0, 0] == -1
    assert win[1, 25, 20] == 1 and win[1, 25, 5] == 0 and win[1, 31, 31] == 1 and win[1, 30, 31] == 1 and win[1, 1, 1] == -1
    assert (win[2, :, 9:14] == 0).all() and (win[2] == 1).sum() == 0
    assert (win[3, :9, 25:] == 1).all() and (win[3] == 0).sum() == 0 and (win[4] == -1).all()
    assert R.clamp_rec(rec, 32, 32)[3] == [(0, 0, 32, 0, 32), (2, 0, 9, 25, 32)]


# ---------------------------------------------------------------------------------------------- the mixins, on stubs
def test_erased_runs_the_base_launch_first_then_the_erasing_launch(monkeypatch):
    from vitamd import data, erase, ops
    calls = []

    class Stub(data.Frames):
        def __init__(self, B):
            self.shape, self.device = torch.Size((B, 3, 8, 8)), torch.device("cpu")
            self._patches, self._image, self._src = {}, None, object()

        def _launch(self, patch, image):
            calls.append(("base", patch, image))
            return "rows", "img"

    monkeypatch.setattr(ops, "frames_erase", lambda *a, **k: calls.append(("erase", a, k)))
    rec, fill = erase.Erase(probability=1.0).draw(2, 8, 0)
    f = Stub(2)
    out = erase.erased(f, (rec, fill), 5, 6)
    assert out is f and isinstance(f, Stub) and isinstance(f, data.Frames) and type(f).__name__ == "ErasedStub"
    assert type(f).materialise is data.Frames.materialise
    assert f.patches(4) == "rows" and calls[0] == ("base", 4, False)
    name, a, k = calls[1]
    assert name == "erase" and a[:3] == ("rows", "img", 4) and torch.equal(a[3], rec) and torch.equal(a[4], fill) and a[5:] == (5, 6) and k == {"hw": (8, 8)}
    assert torch.equal(f.erase[0], rec)
    assert f.images() == "img" and [c[0] for c in calls] == ["base", "erase", "base", "erase"] and calls[2] == ("base", None, True)
    assert type(erase.erased(Stub(2), (rec, None), 0, 0)) is type(f)              # one erased class per frames class
    for bad in (lambda: erase.erased(f, (rec, fill), 0, 0), lambda: erase.erased(object(), (rec, fill), 0, 0),
                lambda: erase.erased(Stub(3), (rec, fill), 0, 0), lambda: erase.erased(Stub(2), (rec, fill[:, :, :3]), 0, 0),
                lambda: erase.erased(Stub(2), rec, 0, 0), lambda: erase.erased(Stub(2), (rec, fill), -1, 0),
                lambda: erase.erased(Stub(2), (rec, fill), 0, 1 << 64)):
        with pytest.raises(ValueError):
            bad()
    done = Stub(2)
    done._image = "img"
    with pytest.raises(ValueError, match="materialised"):
        erase.erased(done, (rec, fill), 0, 0)


def test_the_loader_mixin_calls_the_base_frames_first_and_train_false_bypasses_it(monkeypatch):
    from vitamd import erase
    calls = []

    class Base:
        def __init__(self, train, depth=2):
            self.train, self.depth, self.step, self.out_hw = train, depth, 4, (8, 8)

        def _frames(self, src, geom, table):
            calls.append(("base", src.shape[0]))
            return "frames"

        def _stage_over(self, stage, **host):
            calls.append(("stage", stage, {k: v.clone() for k, v in host.items()}))
            return tuple(host.values())

    class Feed(erase._EraseFeed, Base):
        pass

    monkeypatch.setattr(erase, "erased", lambda frames, pair, seed, step: calls.append(("erased", frames, pair, seed, step)) or "erased frames")
    e = erase.Erase(probability=1.0, mode="rand", seed=7)
    src = torch.zeros((3, 9, 9, 3), dtype=torch.uint8)
    feed = Feed(True, depth=3, erase=e)
    assert feed._erase_stage == [None] * 3
    assert feed._frames(src, None, None) == "erased frames"
    rec, fill = e.draw(3, (8, 8), 4)
    assert calls[0] == ("base", 3) and calls[1][0] == "stage" and calls[1][1] is feed._erase_stage
    assert list(calls[1][2]) == ["erase_rec", "erase_fill"] and torch.equal(calls[1][2]["erase_rec"], rec) and torch.equal(calls[1][2]["erase_fill"], fill)
    assert calls[2][:2] == ("erased", "frames") and torch.equal(calls[2][2][0], rec) and calls[2][3:] == (7, 4)
    del calls[:]
    assert Feed(False, erase=e)._frames(src, None, None) == "frames" and calls == [("base", 3)]
    del calls[:]
    assert Feed(True, erase=erase.Erase(probability=0.0))._frames(src, None, None) == "frames" and calls == [("base", 3)]


def test_the_four_loaders_are_the_mixin_over_their_parents():
    from vitamd import data, erase, mix, resize
    for cls, parent in ((erase.EraseLoader, data.DeviceLoader), (erase.EraseResizeLoader, resize.ResizeLoader), (erase.EraseMixLoader, mix.MixLoader),
                        (erase.EraseResizeMixLoader, mix.ResizeMixLoader)):
        assert cls.__mro__[1:3] == (erase._EraseFeed, parent) and cls._frames is erase._EraseFeed._frames
        assert cls.__next__ is data.DeviceLoader.__next__ and cls._labels is parent._labels
    feed = erase.EraseResizeMixLoader(iter([]), "cuda", 8, mix.Mix(), erase=erase.Erase(), patch=4, image=False, depth=3)
    assert feed._erase_stage == [None] * 3 and feed._mix_stage == [None] * 3 and feed.erase.enabled


def test_train_vit_takes_the_flags_and_refuses_them_without_u8():
    import train_vit as TV
    a = TV.parse_args([])
    assert (a.reprob, a.remode, a.recount) == (0.0, "pixel", 1)
    a = TV.parse_args(["--u8", "--reprob", "0.25", "--remode", "rand", "--recount", "2"])
    assert (a.reprob, a.remode, a.recount) == (0.25, "rand", 2)
    with pytest.raises(SystemExit):
        TV.parse_args(["--remode", "noise"])
    for argv in (["--reprob", "0.25"], ["--remode", "const"], ["--recount", "2"]):
        with pytest.raises(SystemExit, match="need --u8"):
            TV.main(argv + ["--train_steps", "0"])


# ---------------------------------------------------------------------------------------------- what the poison test demands of vitamd/
def test_no_new_empty_site():
    sites = P.empty_sites()
    assert not [s for s in sites if s[0] == "erase.py"]
    with open(os.path.join(P.PKG_DIR, "ops.py")) as f:
        lines = f.read().splitlines()
    tail = next(i for i, line in enumerate(lines) if "Random Erasing on the finished batch" in line) + 1
    assert not [s for s in sites if s[0] == "ops.py" and s[1] >= tail]
    assert {("ops.py", 137), ("functions.py", 182), ("data.py", 229), ("data.py", 230), ("data.py", 243)} <= sites
