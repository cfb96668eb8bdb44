"""The resizing input feed on the GPU (csrc/resize.hip vitamd_frames_prep_resize, vitamd/resize.py) against tests/_resize_ref.py.

The image is held, element by element, to _resize_ref.bound of the float64 reference (derived there: 2 (Tx + Ty + 6) 2^-24 / std);
the bf16 rows to the bits of the round-to-nearest-even im2col of the kernel's own image; an identity record to the bits of
vitamd_frames_prep.  Every output is filled with 0xFF bytes (NaN in both formats) before its launch and lies between guards.

Shapes (_resize_ref.CASES): sources of 37 x 53 and 131 x 140 (rows of 159 and 420 bytes), outputs 16 x 16 at p = 4 and 8, 12 x 20 and
40 x 36 (2 x 2 partial tiles) at p = 4, B = 5 with an index that repeats and reverses frames; C = 3 in the fast form, C = 1, C = 4 and
W = 14 / p = 7 in the generic one.  The five records of a case: an interior down-scale with different x and y scales, a 3 x 1 box scaled
up from the bottom-left corner, the largest box the 8x cap admits from the top-right corner (exactly 8x from the larger source: two strip
chunks), and Resize(S) + crop at offset 0 and at (Hv - H, Wv - W); flips on and off in one batch.  One case past the grid cap."""
import functools
import time

import pytest
import torch

import _resize_ref as R
import weights as Wt
from test_gpu_data import _Alarm, _same

pytestmark = pytest.mark.gpu
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
GUARD = 64


@functools.lru_cache(maxsize=None)
def _case(name, norm):
    """(src, index, box, mean, std, the float64 reference, the bound per sample and channel); computed once, never written to"""
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index, box = R.case(name)
    mean, std = (R.MEAN[:C], R.STD[:C]) if norm else (None, None)
    return src, index, box, mean, std, R.resize_ref(src, (H, W), index, box, mean, std), R.bounds(src.shape, (H, W), box, std)


def _dev(v, dtype):
    return None if v is None else torch.tensor(v, dtype=dtype, device="cuda")


def _filled(n, dtype):
    """a device buffer of n elements between two guards, every byte 0xFF (NaN) -> (whole buffer as integers, the middle)"""
    whole = torch.full((n + 2 * GUARD,), -1, dtype={F32: torch.int32, BF16: torch.int16}[dtype], device="cuda")
    return whole, whole.view(dtype)[GUARD:GUARD + n]


def _run_raw(hip, src, index, box, mean, std, H, W, p, want_patches=True, want_image=True, expect=0, override=None):
    """the C entry on filled, guarded outputs -> (patches or None, image or None) on the CPU.  expect != 0: the call must return that
    code and leave every byte of both outputs as it was"""
    Nsrc, Hs, Ws, C = src.shape
    B = box.shape[0]
    pw = iw = pm = im = None
    if want_patches:
        pw, pm = _filled(B * C * H * W, BF16)
    if want_image:
        iw, im = _filled(B * C * H * W, F32)
    ptr = lambda t: None if t is None else t.data_ptr()
    a = dict(src=ptr(src), index=ptr(index), box=ptr(box), mean=ptr(mean), std=ptr(std), patches=ptr(pm), image=ptr(im), B=B, Nsrc=Nsrc, Hs=Hs,
             Ws=Ws, C=C, H=H, W=W, p=p)
    a.update(override or {})
    code = hip.vitamd_frames_prep_resize(a["src"], a["index"], a["box"], a["mean"], a["std"], a["patches"], a["image"], a["B"], a["Nsrc"], a["Hs"],
                                         a["Ws"], a["C"], a["H"], a["W"], a["p"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == expect, (code, expect, override)
    for whole in (pw, iw):
        if whole is not None:
            assert bool((whole[:GUARD] == -1).all()) and bool((whole[-GUARD:] == -1).all()), "a guard was written"
            if expect != 0:
                assert bool((whole == -1).all()), "a refused call wrote to an output"
    if expect != 0:
        return None, None
    return (pm.view(B * (H // p) * (W // p), C * p * p).cpu() if want_patches else None, im.view(B, C, H, W).cpu() if want_image else None)


def _on_device(name, norm):
    src, index, box, mean, std, ref, bnd = _case(name, norm)
    return src.cuda(), _dev(index, torch.int64), box.cuda(), _dev(mean, F32), _dev(std, F32)


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("norm", [False, True], ids=["unit", "norm"])
@pytest.mark.parametrize("name", list(R.CASES))
def test_image_within_the_bound_rows_round_to_nearest_even_outputs_independent(hip, name, norm):
    from vitamd import ops
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    ref, bnd = _case(name, norm)[5:]
    src, index, box, mean, std = _on_device(name, norm)
    patches, image = _run_raw(hip, src, index, box, mean, std, H, W, p)
    err = (image.double() - ref).abs()
    print(f"{name} norm={norm}: worst error / bound {float((err / bnd).max()):.3f}, worst error {float(err.max()):.3e}")
    assert bool(torch.isfinite(image).all())
    assert not R.check_image(image, ref, bnd, name)
    assert not R.check_rows(patches, image, p, name)
    assert _same(patches, ops.im2col(image.cuda(), p))                    # the rows the unfused route makes of the same image
    only_p, none_i = _run_raw(hip, src, index, box, mean, std, H, W, p, want_image=False)
    none_p, only_i = _run_raw(hip, src, index, box, mean, std, H, W, p, want_patches=False)
    assert none_i is None and none_p is None and _same(only_p, patches) and _same(only_i, image)
    again_p, again_i = _run_raw(hip, src, index, box, mean, std, H, W, p)
    assert _same(again_p, patches) and _same(again_i, image)             # no atomics: the same bits on every call


@pytest.mark.parametrize("name", ["a16_p4", "a16_p8", "c1_p4", "c4_p4", "w14_p7"])
def test_an_identity_record_has_the_bits_of_the_plain_prep(hip, name):
    """h = Hv = H and w = Wv = W: one tap of weight 1 per value"""
    from vitamd import data, ops
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src, index = R.case(name)[:2]
    geom = torch.tensor([[3, 5, 1], [0, 0, 0], [Hs - H, Ws - W, 1], [7, 2, 0], [Hs - H - 1, Ws - W - 1, 0]], dtype=torch.int32)
    box = torch.tensor([[y, H, H, 0, x, W, W, 0, f, 0] for y, x, f in geom.tolist()], dtype=torch.int32)
    it = _dev(index, torch.int64)
    for mean, std in ((None, None), (R.MEAN[:C], R.STD[:C])):
        table = data.norm_table(mean, std, channels=C).cuda()
        want_p, want_i = ops.frames_prep(src.cuda(), (H, W), table, p, True, it, geom.cuda())
        got_p, got_i = _run_raw(hip, src.cuda(), it, box.cuda(), _dev(mean, F32), _dev(std, F32), H, W, p)
        assert _same(got_i, want_i.cpu()) and _same(got_p, want_p.cpu())


@pytest.mark.parametrize("name", ["a16_p4", "w14_p7"])
def test_a_wild_record_gives_what_the_record_it_clamps_to_gives(hip, name):
    Nsrc, Hs, Ws, C, H, W, p = R.CASES[name]
    src = R.case(name)[0]
    lo, hi = R.I32_MIN, R.I32_MAX
    index = [-3, 77, 1, 1 << 40, 2]
    wild = torch.tensor([[lo, hi, lo, hi, hi, lo, hi, lo, 7, 99], [-5, 0, 3, -1, 60, 0, 0, 5, -1, 0], [hi, hi, hi, hi, lo, lo, lo, lo, -7, 0],
                         [5, 1000, 2, 1000, 3, 1000, 2, -4, 0, 0], [30, 100, 1, 0, 50, 100, 1, 0, 1 << 20, -1]], dtype=torch.int32)
    tame = torch.tensor([[*R.clamp_box(r, Hs, Ws, H, W), 0] for r in wild.tolist()], dtype=torch.int32)
    assert tame[:, :8].tolist() != wild[:, :8].tolist() and tame[:, 8].tolist() == [1, 1, 1, 0, 1]
    assert [R.clamp_box(r, Hs, Ws, H, W) for r in tame.tolist()] == [tuple(r[:9]) for r in tame.tolist()]
    mean, std = R.MEAN[:C], R.STD[:C]
    ref = R.resize_ref(src, (H, W), [0, Nsrc - 1, 1, Nsrc - 1, 2], tame, mean, std)
    bnd = R.bounds(src.shape, (H, W), tame, std)
    args = (_dev(mean, F32), _dev(std, F32), H, W, p)
    got_w = _run_raw(hip, src.cuda(), _dev(index, torch.int64), wild.cuda(), *args)
    got_t = _run_raw(hip, src.cuda(), _dev([0, Nsrc - 1, 1, Nsrc - 1, 2], torch.int64), tame.cuda(), *args)
    assert bool(torch.isfinite(got_w[1]).all()) and bool(torch.isfinite(got_w[0].float()).all())
    assert not R.check_image(got_w[1], ref, bnd, name) and not R.check_rows(got_w[0], got_w[1], p, name)
    assert _same(got_w[1], got_t[1]) and _same(got_w[0], got_t[0])


def test_the_end_of_src_and_an_odd_base_address_take_byte_loads_with_the_same_bits(hip):
    """the fast form's aligned-dword window must lie inside src: boxes in the bottom-right corner of the LAST frame end where src ends
    (2, 4, 6 and 16 taps per column), and a source that starts at an odd address takes byte loads throughout"""
    Nsrc, Hs, Ws, C, H, W, p = R.CASES["b16_p4"]
    src = R.case("b16_p4")[0]
    box = torch.tensor([[Hs - h, h, H, 0, Ws - w, w, W, 0, f, 0] for h, w, f in ((7, 9, 0), (16, 16, 1), (30, 28, 1), (50, 47, 0), (128, 128, 1))],
                       dtype=torch.int32)
    index = [Nsrc - 1] * 5
    mean, std = R.MEAN[:3], R.STD[:3]
    ref, bnd = R.resize_ref(src, (H, W), index, box, mean, std), R.bounds(src.shape, (H, W), box, std)
    args = (_dev(index, torch.int64), box.cuda(), _dev(mean, F32), _dev(std, F32), H, W, p)
    patches, image = _run_raw(hip, src.cuda(), *args)
    assert not R.check_image(image, ref, bnd, "end of src") and not R.check_rows(patches, image, p, "end of src")
    store = torch.empty(src.numel() + 1, dtype=U8, device="cuda")
    shifted = store[1:].view(src.shape)
    shifted.copy_(src)
    assert shifted.data_ptr() % 2 == 1
    odd_p, odd_i = _run_raw(hip, shifted, *args)
    assert _same(odd_i, image) and _same(odd_p, patches)


def test_every_refusal_returns_its_code_and_writes_nothing(hip):
    SHAPE, ARG = 1, 2
    Nsrc, Hs, Ws, C, H, W, p = R.CASES["a16_p4"]
    src, index, box, mean, std = _on_device("a16_p4", True)
    run = lambda code, **o: _run_raw(hip, src, index, box, mean, std, H, W, p, expect=code, override=o)
    for bad in (dict(B=0), dict(Nsrc=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(C=0), dict(C=5), dict(Hs=8193), dict(Ws=8193),
                dict(H=8193), dict(W=8193), dict(p=0), dict(p=3), dict(p=32), dict(index=None, B=Nsrc + 1),
                dict(Nsrc=1 << 20, Hs=8192, Ws=8192), dict(B=1 << 20, H=8192, W=8192, p=4)):
        run(SHAPE, **bad)
        run(SHAPE, src=None, box=None, **bad)                                # the shape answers first
    for bad in (dict(src=None), dict(box=None), dict(mean=None), dict(std=None)):
        run(ARG, **bad)
    _run_raw(hip, src, index, box, mean, std, H, W, p, want_patches=False, want_image=False, expect=ARG)


@functools.lru_cache(maxsize=None)
def _cap_case():
    """more tiles than the grid cap: 64 x 64 outputs (2 x 2 tiles) from 3 frames of 131 x 140, the five records of that shape and the
    three frames in every combination, one sample more than a quarter of the cap"""
    g = torch.Generator().manual_seed(11)
    src = torch.randint(0, 256, (3, 131, 140, 3), generator=g, dtype=U8)
    rec = R.records(131, 140, 64, 64)
    combos = [(f, r) for f in range(3) for r in range(5)]
    ref = R.resize_ref(src, (64, 64), [f for f, _ in combos], rec[[r for _, r in combos]], R.MEAN[:3], R.STD[:3])
    bnd = R.bounds(src.shape, (64, 64), rec[[r for _, r in combos]], R.STD[:3])
    return src, rec, combos, ref, bnd


@pytest.mark.parametrize("p", [8, 2], ids=["fast", "generic"])
def test_past_the_grid_cap(hip, p):
    from vitamd import ops
    cap = ops.frames_prep_resize_grid_cap()
    src, rec, combos, ref15, bnd15 = _cap_case()
    B = cap // 4 + 1
    assert B * 4 > cap and B * 3 * 64 * 64 > cap * 256                      # tiles of the fast form, elements of the generic one
    pick = [(7 * b) % 15 for b in range(B)]
    index = torch.tensor([combos[k][0] for k in pick])
    box = rec[[combos[k][1] for k in pick]]
    patches, image = _run_raw(hip, src.cuda(), index.cuda(), box.cuda(), _dev(R.MEAN[:3], F32), _dev(R.STD[:3], F32), 64, 64, p)
    assert not R.check_image(image, ref15[pick], bnd15[pick], f"cap p={p}")
    assert not R.check_rows(patches, image, p, f"cap p={p}")


# ---------------------------------------------------------------------------------------------- the Python objects
def test_resized_frames_hand_out_what_the_entry_point_computes(hip):
    from vitamd import data, resize
    Nsrc, Hs, Ws, C, H, W, p = R.CASES["a12x20_p4"]
    src, index, box, mean, std, ref, bnd = _case("a12x20_p4", True)
    want_p, want_i = _run_raw(hip, *_on_device("a12x20_p4", True), H, W, p)
    f = resize.ResizedFrames(src.cuda(), (H, W), box, index=torch.tensor(index), mean=mean, std=std)
    assert isinstance(f, data.Frames) and tuple(f.shape) == (5, C, H, W) and f.device.type == "cuda" and f.geom is None
    assert torch.equal(f.box.cpu(), box)
    assert _same(f.patches(p), want_p) and _same(f.images(), want_i)
    f2 = resize.ResizedFrames(src.cuda().reshape(2, 2, Hs, Ws, C), (H, W), box, index=torch.tensor(index)).materialise(p, image=True)
    unit = R.resize_ref(src, (H, W), index, box)
    assert not R.check_image(f2.images().cpu(), unit, R.bounds(src.shape, (H, W), box), "5-d source, no normalisation")
    f2.release_source()
    assert _same(f2.patches(p), R.bf16_rows(f2.images().cpu(), p))
    with pytest.raises(Exception, match="source slot is reused"):
        f2.patches(2)


def _model():
    import train_vit as TV
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    model = TV.ViTClassifier(cfg, num_classes=10)
    model.load_state_dict(Wt.classifier_state(3, 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, 10))
    return model.cuda()


def test_classifier_takes_resized_frames_where_it_takes_frames(hip):
    from vitamd import resize
    model = _model()
    src = R.case("a16_p4")[0]
    box = resize.rrc_boxes(5, (37, 53), 32, seed=3, step=0)
    make = lambda: resize.ResizedFrames(src.cuda(), 32, box, index=torch.tensor([3, 1, 1, 0, 2]), mean=R.MEAN[:3], std=R.STD[:3])
    with torch.no_grad():
        images = make().images()
        want = model(images)
        got = model(make())
    assert images.dtype == F32 and want.shape == (5, 10) and torch.equal(got, want)


def test_frames_to_tokens_resizes_raw_videos_to_the_tokenizers_size(hip):
    import train_tatitok as TA
    import train_videogpt as VG
    from vitamd import resize
    torch.manual_seed(0)
    tok = TA.TiTok(TA.TiTokConfig(32, 8, 8, 64, 12, "small")).cuda().eval()
    g = torch.Generator().manual_seed(6)
    videos = torch.randint(0, 256, (2, 3, 24, 40, 3), generator=g, dtype=U8)
    box = resize.resize_center_boxes(6, (24, 40), 32, 32)
    assert box[0].tolist() == [0, 24, 32, 0, 0, 40, 53, 10, 0, 0]            # the short side to 32, the centre 32 of int(32 * 40 / 24) = 53
    ref = R.resize_ref(videos.reshape(6, 24, 40, 3), (32, 32), None, box)
    got = VG.frames_to_tokens(tok, videos.cuda(), size=32)
    assert got.dtype == torch.int64 and got.shape == (2, 3, 8)
    kernel = resize.ResizedFrames(videos.cuda(), 32, box).images()
    assert not R.check_image(kernel.cpu(), ref, R.bounds((6, 24, 40, 3), (32, 32), box), "videos")
    assert torch.equal(got, VG.frames_to_tokens(tok, kernel.reshape(2, 3, 3, 32, 32)))
    assert torch.equal(got, VG.frames_to_tokens(tok, ref.to(F32).cuda().reshape(2, 3, 3, 32, 32)))      # the reference-resized frames
    window = torch.tensor([[1, 2], [4, 5]], device="cuda")
    assert torch.equal(VG.frames_to_tokens(tok, videos.cuda(), index=window, size=32), got[:, 1:3])
    same = torch.randint(0, 256, (1, 2, 32, 32, 3), generator=g, dtype=U8).cuda()
    assert torch.equal(VG.frames_to_tokens(tok, same, size=32), VG.frames_to_tokens(tok, same))          # already at size: today's route


# ---------------------------------------------------------------------------------------------- the loader
def _host_batches(n_batches, B):
    g = torch.Generator().manual_seed(21)
    originals = [torch.randint(0, 256, (B if i < n_batches - 1 else B - 1, 37, 53, 3), generator=g, dtype=U8) for i in range(n_batches)]
    labels = [torch.arange(o.shape[0]) + 10 * i for i, o in enumerate(originals)]
    extents = [torch.tensor([[37, 53], [30, 53], [37, 41], [19, 23]][:o.shape[0]], dtype=torch.int32) for o in originals]
    return originals, labels, extents


def _host(originals, labels, extents, handed):
    for i, (u8, lab) in enumerate(zip(originals, labels)):
        item = (u8.clone(), lab.clone()) if extents is None else (u8.clone(), lab.clone(), extents[i].clone())
        handed.append(item)
        yield item


def _drain(loader, handed):
    seen = []
    with _Alarm(60):
        for frames, lab in loader:
            for item in handed:                      # everything the loader has taken so far is overwritten at once
                item[0].fill_(0)
                item[1].fill_(-1)
                if len(item) == 3:
                    item[2].fill_(1)
            seen.append((frames, lab))
        done = torch.cuda.Event()
        done.record()
        deadline = time.monotonic() + 30
        while not done.query():                      # polled, not waited on
            assert time.monotonic() < deadline, "the loader's work did not finish"
    return seen


@pytest.mark.parametrize("mode,with_extents", [("rrc", True), ("rrc", False), ("resize_crop", True)])
def test_resize_loader_yields_what_the_draw_and_the_reference_predict(hip, mode, with_extents):
    from vitamd import resize
    n_batches, B = 3, 4
    originals, labels, extents = _host_batches(n_batches, B)
    handed = []
    loader = resize.ResizeLoader(_host(originals, labels, extents if with_extents else None, handed), "cuda", 16, mode=mode, resize_to=18,
                                 patch=4, image=True, mean=R.MEAN[:3], std=R.STD[:3], train=True, seed=77, depth=2)
    seen = _drain(loader, handed)
    assert len(seen) == n_batches and loader.step == n_batches
    flips = set()
    for i, (frames, lab) in enumerate(seen):
        n = originals[i].shape[0]
        ext = extents[i] if with_extents else None
        if mode == "rrc":
            box = resize.rrc_boxes(n, (37, 53), 16, seed=77, step=i, extents=ext)
        else:
            box = resize.resize_crop_boxes(n, (37, 53), 18, 16, seed=77, step=i, extents=ext)
        flips |= set(box[:, 8].tolist())
        assert isinstance(frames, resize.ResizedFrames) and tuple(frames.shape) == (n, 3, 16, 16)
        assert torch.equal(frames.box.cpu(), box)
        ref = R.resize_ref(originals[i], (16, 16), None, box, R.MEAN[:3], R.STD[:3])
        image = frames.images().cpu()
        assert not R.check_image(image, ref, R.bounds(originals[i].shape, (16, 16), box, R.STD[:3]), f"batch {i}")
        assert not R.check_rows(frames.patches(4).cpu(), image, 4, f"batch {i}")
        assert lab.is_cuda and torch.equal(lab.cpu(), labels[i])
    assert flips == {0, 1}


def test_resize_loader_in_evaluation_is_the_centre_form(hip):
    from vitamd import resize
    n_batches, B = 3, 4
    originals, labels, extents = _host_batches(n_batches, B)
    handed = []
    loader = resize.ResizeLoader(_host(originals, labels, extents, handed), "cuda", 16, mode="rrc", resize_to=18, patch=4, image=True,
                                 train=False, depth=2)
    seen = _drain(loader, handed)
    assert len(seen) == n_batches
    for i, (frames, lab) in enumerate(seen):
        n = originals[i].shape[0]
        box = resize.resize_center_boxes(n, (37, 53), 18, 16, extents=extents[i])
        assert torch.equal(frames.box.cpu(), box) and set(box[:, 8].tolist()) == {0}
        ref = R.resize_ref(originals[i], (16, 16), None, box)
        assert not R.check_image(frames.images().cpu(), ref, R.bounds(originals[i].shape, (16, 16), box), f"batch {i}")
