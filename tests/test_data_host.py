"""The device input pipeline without a GPU: the binding of its entry points, every refusal the C entries make before a launch (dummy
pointers that no such call dereferences, as in test_launch_args_host.py), the CPU restatements of its semantics against each other and
against the lookup table, the crop geometry, and the argument checks of vitamd.data."""
import ctypes
import os

import pytest
import torch

import _abi
import _data_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, ARG = 1, 2            # VITAMD_ERR_SHAPE, VITAMD_ERR_ARG
INT_MAX = 2**31 - 1
NEW_SYMBOLS = {"vitamd_frames_prep": 15, "vitamd_frames_prep_grid_cap": 0, "vitamd_crop_flip_draw": 10, "vitamd_frames_to_u8": 7}

_buf = (ctypes.c_float * 64)()
P = ctypes.addressof(_buf)


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


def test_new_symbols_are_bound_with_the_headers_argument_counts(L):
    from vitamd import lib, ops
    declared, _ = _abi.declared()
    for name, n in NEW_SYMBOLS.items():
        assert declared[name] == n == len(lib.SIGNATURES[name]), name
        assert hasattr(L, name)
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    assert ops.frames_prep_grid_cap() == L.vitamd_frames_prep_grid_cap() >= 256


def _prep(L, src=P, index=P, geom=P, table=P, patches=P, image=P, B=3, Nsrc=5, Hs=11, Ws=13, C=3, H=8, W=8, p=4):
    return L.vitamd_frames_prep(src, index, geom, table, patches, image, B, Nsrc, Hs, Ws, C, H, W, p, None)


BAD_SHAPES = [dict(B=0), dict(B=-1), dict(Nsrc=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(H=-8), dict(C=0), dict(C=5), dict(H=12), dict(W=14),
              dict(p=0), dict(p=-4), dict(p=3), dict(H=8, W=6, p=4), dict(H=6, W=8, p=4),
              dict(index=None, B=6),                                                      # identity needs Nsrc >= B
              dict(Nsrc=INT_MAX, Hs=INT_MAX, Ws=INT_MAX, C=4, H=8, W=8),                  # source element count
              dict(B=INT_MAX, index=P, Hs=INT_MAX, Ws=INT_MAX, H=INT_MAX - 7, W=INT_MAX - 7, p=8, C=4)]   # output element count


def _shape_id(bad):
    """str(bad) with the dummy pointer spelled "P" (it is an address: as an id it would change from run to run)"""
    return str({k: "P" if v == P else v for k, v in bad.items()})


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=_shape_id)
def test_frames_prep_shape_is_refused_first(L, bad):
    assert _prep(L, **bad) == SHAPE
    # ... also with the required pointers null: the shape answers before them
    assert _prep(L, **{**dict(src=None, table=None, geom=None), **bad}) == SHAPE
    if not ({"p"} & set(bad) or 6 in (bad.get("H"), bad.get("W"))):     # (the patch rules hold only where patch rows are asked for)
        assert _prep(L, **{**dict(src=None, table=None, patches=None, image=None), **bad}) == SHAPE


def test_frames_prep_patch_rules_only_with_patch_rows(L):
    # without patch rows p is not looked at: the call gets as far as the pointer check
    assert _prep(L, patches=None, image=None, p=0) == ARG
    assert _prep(L, patches=None, image=None, p=3, H=7, W=5) == ARG


def test_frames_prep_null_pointers(L):
    assert _prep(L, src=None) == ARG
    assert _prep(L, table=None) == ARG
    assert _prep(L, patches=None, image=None) == ARG
    assert _prep(L, src=None, table=None, patches=None, image=None) == ARG


@pytest.mark.parametrize("bad", [dict(B=0), dict(Hs=0), dict(Ws=-1), dict(H=0), dict(W=0), dict(H=12), dict(W=14)], ids=str)
def test_crop_flip_draw_refusals(L, bad):
    a = dict(B=3, Hs=11, Ws=13, H=8, W=8)
    a.update(bad)
    for geom in (P, None):
        assert L.vitamd_crop_flip_draw(geom, a["B"], a["Hs"], a["Ws"], a["H"], a["W"], 1, 7, 1 << 40, None) == SHAPE
    assert L.vitamd_crop_flip_draw(None, 3, 11, 13, 8, 8, 1, 7, 0, None) == ARG


@pytest.mark.parametrize("bad", [dict(B=0), dict(C=0), dict(C=5), dict(H=0), dict(W=-2), dict(B=INT_MAX, C=4, H=INT_MAX, W=INT_MAX)], ids=str)
def test_frames_to_u8_refusals(L, bad):
    a = dict(B=2, C=3, H=4, W=4)
    a.update(bad)
    for img, out in ((P, P), (None, None)):
        assert L.vitamd_frames_to_u8(img, out, a["B"], a["C"], a["H"], a["W"], None) == SHAPE
    assert L.vitamd_frames_to_u8(None, P, 2, 3, 4, 4, None) == ARG
    assert L.vitamd_frames_to_u8(P, None, 2, 3, 4, 4, None) == ARG


# ---------------------------------------------------------------------------------------------- the semantics, on the CPU
def _case(seed=0, Nsrc=5, Hs=11, Ws=13, C=3):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (Nsrc, Hs, Ws, C), generator=g, dtype=torch.uint8)
    src.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    return src


def test_the_two_cpu_statements_and_the_table_agree_bit_for_bit():
    from vitamd import data
    src = _case()
    index = [4, 0, 4]
    geom = torch.tensor([[0, 3, 0], [3, 5, 1], [1, 0, 0]], dtype=torch.int32)
    for mean, std in ((data.IMAGENET_MEAN, data.IMAGENET_STD), (None, None)):
        a = R.frames_ref(src, (8, 8), index, geom, mean, std)
        b = R.frames_ref_tv(src, (8, 8), index, geom, mean, std)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        table = data.norm_table(mean, std)
        assert table.shape == (3, 256) and table.dtype == torch.float32
        for c in range(3):
            assert torch.equal(table[c].view(torch.int32), R.value(torch.arange(256, dtype=torch.uint8), c, mean, std).view(torch.int32))
        # the table trick itself: looking the source bytes up gives the same image
        idx, g = R.clamp_geom(index, geom, 3, *src.shape[:3], 8, 8)
        for b_, (y0, x0, flip) in enumerate(g):
            crop = src[idx[b_], y0:y0 + 8, x0:x0 + 8].long()
            crop = crop.flip(1) if flip else crop
            looked = torch.stack([table[c][crop[..., c]] for c in range(3)])
            assert torch.equal(looked.view(torch.int32), a[b_].view(torch.int32))
    assert data.norm_table(data.IMAGENET_MEAN, data.IMAGENET_STD) is data.norm_table(data.IMAGENET_MEAN, data.IMAGENET_STD)
    assert data.IMAGENET_MEAN == (0.485, 0.456, 0.406) and data.IMAGENET_STD == (0.229, 0.224, 0.225)


def test_reference_clamps_and_patch_rows():
    src = _case(1)
    wild = torch.tensor([[-5, 99, 7], [99, -1, 0], [2, 2, 0]], dtype=torch.int32)
    tame = torch.tensor([[0, 5, 1], [3, 0, 0], [2, 2, 0]], dtype=torch.int32)
    assert torch.equal(R.frames_ref(src, (8, 8), [-3, 77, 1], wild), R.frames_ref(src, (8, 8), [0, 4, 1], tame))
    img = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).view(2, 3, 4, 6)
    rows = R.patch_rows(img, 2)
    assert rows.shape == (2 * 2 * 3, 12)
    b, ph, pw, c, kh, kw = 1, 1, 2, 2, 1, 0
    assert rows[(b * 2 + ph) * 3 + pw, (c * 2 + kh) * 2 + kw] == img[b, c, ph * 2 + kh, pw * 2 + kw]


@pytest.mark.parametrize("d", range(6))
def test_center_geom_is_torchvisions_center_crop(d):
    from vitamd import data
    g = data.center_geom(3, (8 + d, 8 + 5 - d), (8, 8))
    assert g.dtype == torch.int32 and g.shape == (3, 3)
    assert g.tolist() == [[int(round(d / 2.0)), int(round((5 - d) / 2.0)), 0]] * 3
    assert g[0, 0] == [0, 0, 1, 2, 2, 2][d]                  # ties go to the even offset, as Python's round does inside CenterCrop
    assert 0 <= g[0, 0] <= d and 0 <= g[0, 1] <= 5 - d


@pytest.mark.parametrize("n", [1, 2, 7])
def test_draw_reference_stays_in_bounds_and_reaches_both_ends(n):
    H = W = 8
    g = R.draw_ref(4096, (H + n - 1, W + n - 1), (H, W), seed=0x1234_5678_9ABC_DEF0, step=(1 << 32) + 5)
    assert g.dtype == torch.int32 and g.shape == (4096, 3)
    for col in (0, 1):
        assert int(g[:, col].min()) == 0 and int(g[:, col].max()) == n - 1
    assert set(g[:, 2].tolist()) == {0, 1}
    assert set(R.draw_ref(64, (9, 9), (8, 8), 3, 0, flip=False)[:, 2].tolist()) == {0}
    # another step, another draw; the same step, the same draw
    assert not torch.equal(g, R.draw_ref(4096, (H + n - 1, W + n - 1), (H, W), 0x1234_5678_9ABC_DEF0, 5)) or n == 1
    assert torch.equal(g, R.draw_ref(4096, (H + n - 1, W + n - 1), (H, W), 0x1234_5678_9ABC_DEF0, (1 << 32) + 5))


def test_to_u8_reference_ties_and_specials():
    x = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255, -1.0, 2.0, float("inf"), -float("inf"), float("nan")]).view(1, 1, 2, 4)
    assert R.to_u8_ref(x).view(-1).tolist() == [0, 2, 2, 0, 255, 255, 0, 0]


# ---------------------------------------------------------------------------------------------- vitamd.data refuses before any device work
def test_frames_refuses_wrong_input_before_any_device_work():
    from vitamd import data, lib
    u8 = torch.zeros((5, 11, 13, 3), dtype=torch.uint8)
    bad = {
        "uint8": lambda: data.Frames(u8.float(), 8),
        "channels last": lambda: data.Frames(u8[0], 8),
        "does not fit": lambda: data.Frames(u8, 12),
        "C in 1..4": lambda: data.Frames(torch.zeros((2, 8, 8, 5), dtype=torch.uint8), 8),
        "size must be": lambda: data.Frames(u8, 0),
        "index must be": lambda: data.Frames(u8, 8, index=torch.zeros(3, dtype=torch.int32)),
        "geom must be int32": lambda: data.Frames(u8, 8, geom=torch.zeros((4, 3), dtype=torch.int32)),
        "table must be fp32": lambda: data.Frames(u8, 8, table=torch.zeros((3, 255))),
    }
    for msg, call in bad.items():
        with pytest.raises(ValueError, match=msg):
            call()
    with pytest.raises(lib.VitamdError, match="ROCm device"):            # everything right but the place: still no device touched
        data.Frames(u8, 8)
    with pytest.raises(lib.VitamdError, match="ROCm device"):
        data.Frames(u8.view(1, 5, 11, 13, 3), (8, 8), index=torch.tensor([4, 0, 4]))
    with pytest.raises(ValueError):
        data.to_u8(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="together"):
        data.norm_table(mean=data.IMAGENET_MEAN)


def test_device_loader_refuses_wrong_input_before_any_device_work():
    from vitamd import data
    ok = torch.zeros((4, 11, 13, 3), dtype=torch.uint8)
    for kw, msg in ((dict(size=0), "size must be"), (dict(size=8, patch=3), "does not tile"), (dict(size=8, depth=1), "depth"),
                    (dict(size=8, image=False), "nothing to produce"), (dict(size=8, seed=-1), "seed"),
                    (dict(size=8, mean=data.IMAGENET_MEAN), "together")):
        with pytest.raises(ValueError, match=msg):
            data.DeviceLoader(iter([(ok, None)]), "cuda", **kw)
    with pytest.raises(ValueError, match="ROCm device"):
        data.DeviceLoader(iter([(ok, None)]), "cpu", 8)
    batches = {
        "uint8 CPU tensor": (ok.float(), None),
        r"\[B, Hs, Ws, C\]": (ok[0], None),
        "does not fit": (torch.zeros((4, 7, 13, 3), dtype=torch.uint8), None),
        "C in 1..4": (torch.zeros((4, 11, 13, 6), dtype=torch.uint8), None),
        "one row per frame": (ok, torch.zeros(3, dtype=torch.int64)),
        "must yield": ok,
    }
    for msg, batch in batches.items():
        loader = data.DeviceLoader(iter([batch]), "cuda", 8, patch=4)
        with pytest.raises(ValueError, match=msg):
            next(loader)
        assert loader._copy_stream is None and loader._slots is None        # refused before a stream, a pinned buffer or a device slot exists
    empty = data.DeviceLoader(iter([]), "cuda", 8)
    with pytest.raises(StopIteration):
        next(empty)


# ---------------------------------------------------------------------------------------------- one home for what the four routes share
def test_one_materialise_and_one_launch_hook_per_frames_class():
    from vitamd import data, mix, resize
    classes = (data.Frames, resize.ResizedFrames, mix.MixedFrames, mix.MixedResizedFrames)
    assert [c for c in classes if "materialise" in vars(c)] == [data.Frames]        # the bookkeeping is stated once
    assert all("_launch" in vars(c) for c in classes)                               # and every class says only which kernel it takes
    assert len({c._launch for c in classes}) == 4 and all(c.materialise is data.Frames.materialise for c in classes)
    pkg = os.path.join(ROOT, "vit-is-all-you-need_amd", "vitamd")
    src = {n: open(os.path.join(pkg, n)).read() for n in sorted(os.listdir(pkg)) if n.endswith(".py")}
    assert sum(s.count("self._src is None") for s in src.values()) == 1             # the released-source refusal
    assert "pin_memory(" not in src["mix.py"] and "pin_memory(" not in src["resize.py"]      # the record staging has one home
    assert src["data.py"].count("def _stage_over(") == 1 and src["data.py"].count("pin_memory(") == 3     # _feed's two and this one
    assert all(n not in s for n in ("torch.cuda.Event", "non_blocking=") for s in (src["mix.py"], src["resize.py"]))


def test_record_staging_keeps_its_order_of_steps(monkeypatch):
    """DeviceLoader._stage_over with stand-ins for the pinned allocation and the event: entry step % depth, allocated on first use
    and again when too short; the host waits for the entry's event BEFORE the buffers are rewritten and records it AFTER the copies
    to the device were issued; the device tensors come back in the order given."""
    from vitamd import data
    log = []

    class Event:
        def synchronize(self):
            log.append(("sync", {k: v.clone() for k, v in (stage[slot] or {}).items() if k != "done"}))

        def record(self, stream):
            log.append(("record", stream, {k: v.clone() for k, v in stage[slot].items() if k != "done"}))

    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: ("stream of", device))
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: log.append(("pin", tuple(self.shape), self.dtype, int(self.abs().sum()))) or self)
    ld = data.DeviceLoader(iter([]), "cuda", 8, depth=3)
    ld.device = "cpu"                                   # where the stand-in copies go
    stage = [None] * 3
    rec1, lam1 = torch.arange(12, dtype=torch.int32).reshape(2, 6) + 1, torch.tensor([0.25, 0.5])
    ld.step, slot = 4, 1
    out = ld._stage_over(stage, rec=rec1, lam=lam1)
    assert [e[0] for e in log] == ["pin", "pin", "sync", "record"] and log[0][1:] == ((2, 6), torch.int32, 0) and log[1][1:] == ((2,), torch.float32, 0)
    assert stage[0] is None and stage[2] is None and list(stage[1]) == ["rec", "lam", "done"]
    assert not log[2][1]["rec"].any() and torch.equal(log[3][2]["rec"], rec1) and log[3][1] == ("stream of", "cpu")
    assert isinstance(out, tuple) and torch.equal(out[0], rec1) and torch.equal(out[1], lam1)
    del log[:]
    rec2, lam2 = rec1[:1] * 3, lam1[:1] * 3                # a shorter batch, `depth` steps later: the same entry, no allocation
    ld.step = 7
    first = stage[1]
    out = ld._stage_over(stage, rec=rec2, lam=lam2)
    assert stage[1] is first and [e[0] for e in log] == ["sync", "record"]
    assert torch.equal(log[0][1]["rec"], rec1) and torch.equal(log[0][1]["lam"], lam1)          # still the earlier record when the host waits
    assert torch.equal(log[1][2]["rec"][:1], rec2) and torch.equal(log[1][2]["lam"][:1], lam2)
    assert tuple(out[0].shape) == (1, 6) and torch.equal(out[0], rec2) and torch.equal(out[1], lam2)
    del log[:]
    box = torch.ones((5, 10), dtype=torch.int32)            # a record of its own list, and a longer batch: allocated again
    ld.step, slot = 10, 1
    stage[1] = {"box": torch.zeros((2, 10), dtype=torch.int32), "done": Event()}
    (out,) = ld._stage_over(stage, box=box)
    assert [e[0] for e in log] == ["pin", "sync", "record"] and tuple(stage[1]["box"].shape) == (5, 10) and torch.equal(out, box)
