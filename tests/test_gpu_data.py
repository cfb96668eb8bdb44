"""The device input pipeline on the GPU (csrc/input.hip, vitamd/data.py) against tests/_data_ref.py.  Every comparison is exact: the
kernel's image is a table lookup of torch's own CPU arithmetic, its patch rows are the bits ops.im2col makes of that image, the draw is
integer arithmetic, and the way back to uint8 is one correctly rounded product.

Shapes: the smallest at which each form can go wrong - source rows of 13 * 3 = 39 bytes, so that rows, crops and flips start at odd
addresses; frames out of order and repeated; crops at both ends of their range; every generic-form reason (C != 3, p % 4 != 0); the fast
form at p = 16 over more than one patch; and one case past the grid cap."""
import functools
import signal
import time

import pytest
import torch

import _data_ref as R
import vit_oracle as O
import weights as Wt

pytestmark = pytest.mark.gpu
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
GUARD = 64            # guard elements on either side of an output


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({BF16: torch.int16, F32: torch.int32}.get(t.dtype, t.dtype))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# name -> (Nsrc, Hs, Ws, C, H, W, p, index, geom)
CASES = {
    "smallest":      (5, 11, 13, 3, 8, 8, 4, [4, 0, 4], [[0, 3, 0], [3, 5, 1], [1, 0, 0]]),       # odd x0; x0 = Ws-W with a flip; y0 = 0 and Hs-H
    "generic_c1_p2": (5, 11, 13, 1, 8, 8, 2, [4, 0, 4], [[0, 3, 0], [3, 5, 1], [1, 0, 0]]),
    "generic_c3_p2": (5, 11, 13, 3, 8, 8, 2, [4, 0, 4], [[0, 3, 0], [3, 5, 1], [1, 0, 0]]),
    "generic_c4_p4": (5, 11, 13, 4, 8, 8, 4, [4, 0, 4], [[0, 3, 0], [3, 5, 1], [1, 0, 0]]),
    "fast_p16":      (4, 37, 41, 3, 32, 32, 16, [3, 1, 1, 0], [[5, 9, 1], [0, 0, 0], [2, 7, 0], [5, 8, 1]]),
    "identity":      (5, 11, 13, 3, 8, 8, 4, None, None),
    "identity_geom": (3, 11, 13, 3, 8, 8, 4, None, [[3, 1, 1], [0, 5, 0], [2, 2, 1]]),
    "index_only":    (5, 11, 13, 3, 8, 8, 4, [2, 2, 0, 4], None),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(src uint8 on the CPU, the CPU reference image); computed once, never written to"""
    Nsrc, Hs, Ws, C, H, W, p, index, geom = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    src = torch.randint(0, 256, (Nsrc, Hs, Ws, C), generator=g, dtype=U8)
    gt = None if geom is None else torch.tensor(geom, dtype=torch.int32)
    ref = R.frames_ref(src, (H, W), index, gt, MEAN[:C], STD[:C])
    return src, ref


def _table(C):
    from vitamd import data
    return data.norm_table(MEAN[:C], STD[:C], channels=C).cuda()


def _guarded(n, dtype):
    """a device buffer of n elements between two guards, all set to a sentinel -> (whole buffer, the middle)"""
    whole = torch.full((n + 2 * GUARD,), 7.0, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def _run_raw(hip, src, table, index, geom, B, H, W, p, want_patches, want_image):
    """the C entry on guarded outputs -> (patches or None, image or None), with the guards checked"""
    from vitamd import lib
    Nsrc, Hs, Ws, C = src.shape
    pw = iw = None
    if want_patches:
        pw, pm = _guarded(B * C * H * W, BF16)
    if want_image:
        iw, im = _guarded(B * C * H * W, F32)
    lib.check(hip.vitamd_frames_prep(src.data_ptr(), None if index is None else index.data_ptr(), None if geom is None else geom.data_ptr(),
                                     table.data_ptr(), pm.data_ptr() if want_patches else None, im.data_ptr() if want_image else None,
                                     B, Nsrc, Hs, Ws, C, H, W, p, torch.cuda.current_stream().cuda_stream), "frames_prep")
    torch.cuda.synchronize()
    for whole in (pw, iw):
        if whole is not None:
            assert bool((whole[:GUARD] == 7).all()) and bool((whole[-GUARD:] == 7).all()), "a guard was written"
    return (pm.view(B * (H // p) * (W // p), C * p * p).clone() if want_patches else None, im.view(B, C, H, W).clone() if want_image else None)


@pytest.mark.parametrize("outputs", ["both", "image", "patches"])
@pytest.mark.parametrize("name", list(CASES))
def test_prep_equals_the_cpu_reference_and_im2col(hip, name, outputs):
    from vitamd import ops
    Nsrc, Hs, Ws, C, H, W, p, index, geom = CASES[name]
    src, ref = _case(name)
    B = Nsrc if index is None else len(index)
    assert (Ws * C) % 2 == 1 or C % 2 == 0                       # rows start at odd addresses wherever the channel count allows it
    it = None if index is None else torch.tensor(index, dtype=torch.int64, device="cuda")
    gt = None if geom is None else torch.tensor(geom, dtype=torch.int32, device="cuda")
    patches, image = _run_raw(hip, src.cuda(), _table(C), it, gt, B, H, W, p, outputs != "image", outputs != "patches")
    if image is not None:
        assert _same(image, ref)
    if patches is not None:
        want = ops.im2col(ref.cuda(), p)                          # the rows the present route makes of the same image
        assert _same(patches, want)
        assert _same(patches, R.patch_rows(ref, p).to(BF16))      # and the permutation, restated


def test_prep_from_an_odd_base_address(hip):
    """a source that starts at an odd address takes the byte-load path of the fast form throughout"""
    Nsrc, Hs, Ws, C, H, W, p, index, geom = CASES["smallest"]
    src, ref = _case("smallest")
    store = torch.empty(src.numel() + 1, dtype=U8, device="cuda")
    shifted = store[1:].view(src.shape)
    shifted.copy_(src)
    assert shifted.data_ptr() % 2 == 1
    it, gt = torch.tensor(index, device="cuda"), torch.tensor(geom, dtype=torch.int32, device="cuda")
    patches, image = _run_raw(hip, shifted, _table(C), it, gt, len(index), H, W, p, True, True)
    assert _same(image, ref) and _same(patches, R.patch_rows(ref, p).to(BF16))


@pytest.mark.parametrize("name", ["smallest", "generic_c3_p2"])
def test_out_of_range_index_and_geom_give_the_clamped_frames_values(hip, name):
    Nsrc, Hs, Ws, C, H, W, p, _, _ = CASES[name]
    src, _ = _case(name)
    index = [-3, 77, 1, 1 << 40]
    wild = torch.tensor([[-5, 99, 7], [99, -1, 0], [2, 2, -1], [-(1 << 31), (1 << 31) - 1, 0]], dtype=torch.int32)
    ref = R.frames_ref(src, (H, W), index, wild, MEAN[:C], STD[:C])
    tame = torch.tensor([[0, Ws - W, 1], [Hs - H, 0, 0], [2, 2, 1], [0, Ws - W, 0]], dtype=torch.int32)
    assert torch.equal(ref, R.frames_ref(src, (H, W), [0, Nsrc - 1, 1, Nsrc - 1], tame, MEAN[:C], STD[:C]))     # what the clamps mean
    patches, image = _run_raw(hip, src.cuda(), _table(C), torch.tensor(index, device="cuda"), wild.cuda(), 4, H, W, p, True, True)
    assert _same(image, ref) and _same(patches, R.patch_rows(ref, p).to(BF16))


def test_prep_past_the_grid_cap(hip):
    """more 4-pixel groups than cap * 256 lanes cover in one pass: 40 samples of 232 x 232 from 5 frames of 233 x 235; the generic form
    (p = 2) then has twelve times the items"""
    from vitamd import data, ops
    B, H, W, p = 40, 232, 232, 8
    assert B * H * (W // 4) > ops.frames_prep_grid_cap() * 256
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, 256, (5, 233, 235, 3), generator=g, dtype=U8)
    index = torch.randint(0, 5, (B,), generator=g)
    geom = torch.stack([torch.randint(0, 2, (B,), generator=g), torch.randint(0, 4, (B,), generator=g), torch.randint(0, 2, (B,), generator=g)], 1).int()
    ref = R.frames_ref_tv(src, (H, W), index.tolist(), geom, MEAN[:3], STD[:3])
    f = data.Frames(src.cuda(), (H, W), index=index.cuda(), geom=geom.cuda(), table=_table(3)).materialise(p, image=True)
    assert _same(f.images(), ref)
    assert _same(f.patches(p), ops.im2col(ref.cuda(), p))
    assert _same(f.patches(2), ops.im2col(ref.cuda(), 2))


def test_frames_object_caches_and_flattens_videos(hip):
    from vitamd import data, lib
    src, _ = _case("smallest")
    video = torch.stack([src[:4], src[1:5]])                      # [2, 4, 11, 13, 3]
    index = torch.tensor([1, 2, 5, 6])                            # the window [:, 1:3] of the flattened frames
    f = data.Frames(video.cuda(), (8, 12), index=index.cuda())
    assert tuple(f.shape) == (4, 3, 8, 12) and f.device.type == "cuda"
    want = video[:, 1:3].reshape(4, 11, 13, 3).permute(0, 3, 1, 2)[:, :, :8, :12].float().div(255)
    assert _same(f.images(), want)
    assert f.images() is f.images() and f.patches(2) is f.patches(2)
    assert _same(f.patches(2), R.patch_rows(want, 2).to(BF16))
    f.release_source()
    assert f.patches(2) is not None
    with pytest.raises(lib.VitamdError, match="source slot"):
        f.patches(4)


@pytest.mark.parametrize("seed", [0, 0xFEDC_BA98_7654_3210])
def test_draw_equals_the_philox_reference(hip, seed):
    from vitamd import data
    step = (1 << 32) + 3
    for B, src_hw, out_hw, flip in ((300, (11, 13), (8, 8), True), (5, (8, 14), (8, 8), True), (7, (37, 41), (32, 32), False)):
        got = data.random_geom(B, src_hw, out_hw, seed, step, flip=flip)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), R.draw_ref(B, src_hw, out_hw, seed, step, flip))
    a = data.random_geom(300, (11, 13), (8, 8), seed, 3)
    assert not torch.equal(a.cpu(), R.draw_ref(300, (11, 13), (8, 8), seed, step))            # the high half of the step counts
    assert torch.equal(a.cpu(), R.draw_ref(300, (11, 13), (8, 8), seed, 3))


@pytest.mark.parametrize("shape", [(2, 3, 4, 6), (3, 3, 5, 7), (2, 1, 4, 4), (1, 4, 8, 8), (2, 2, 3, 3)], ids=str)
def test_frames_to_u8_equals_the_torch_expression(hip, shape):
    from vitamd import data
    g = torch.Generator().manual_seed(shape[-1])
    x = torch.rand(shape, generator=g) * 1.5 - 0.25                                           # negatives and values above 1 among them
    flat = x.view(-1)
    ties = (torch.arange(0, 16, dtype=F32) + 0.5) / 255                                       # k + 0.5 after the product wherever it is exact
    flat[:16] = ties
    flat[16:20] = torch.tensor([float("inf"), -float("inf"), -0.0, 1.0])
    want = (x.clamp(0, 1) * 255).round().to(U8).permute(0, 2, 3, 1).contiguous()              # the expression of the issue, finite and infinite input
    got = data.to_u8(x.cuda())
    assert got.dtype == U8 and got.shape == want.shape and torch.equal(got.cpu(), want)
    flat[20] = float("nan")
    got = data.to_u8(x.cuda()).cpu()
    assert torch.equal(got, R.to_u8_ref(x)) and int(got.permute(0, 3, 1, 2).reshape(-1)[20]) == 0
    video = data.to_u8(x.cuda().unsqueeze(0))                                                 # leading dimensions are kept
    assert video.shape == (1, *want.shape)


# ---------------------------------------------------------------------------------------------- model level
def _frames32(B=4, seed=11, geom=True):
    from vitamd import data
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (B, 37, 41, 3), generator=g, dtype=U8).cuda()
    gt = torch.tensor([[5, 9, 1], [0, 0, 0], [2, 7, 0], [5, 8, 1]], dtype=torch.int32)[:B].cuda() if geom else None
    return lambda table: data.Frames(src, 32, geom=gt, table=table)


def test_classifier_on_frames_equals_classifier_on_their_images(hip):
    import train_vit as TV
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    model = TV.ViTClassifier(cfg, num_classes=10)
    model.load_state_dict(Wt.classifier_state(3, 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, 10))
    model = model.cuda()
    labels = Wt.randint(3, "labels", (4,), 10).cuda()
    make = _frames32()
    table = _table(3)

    def run(x):
        model.zero_grad(set_to_none=True)
        logits = model(x)
        torch.nn.functional.cross_entropy(logits, labels).backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    images = make(table).images()
    l1, g1 = run(images)
    l2, g2 = run(images)
    lf, gf = run(make(table))
    assert _same(lf, l1) and _same(l1, l2)
    for k in g1:
        if _same(g1[k], g2[k]):                      # the tensor route reproduces this gradient: the Frames route must give its bits
            assert _same(gf[k], g1[k]), k
        else:                                        # atomics in its reduction: the additive bound test_gpu_parity.py puts on these gradients
            assert O.rel_l2(gf[k].cpu(), g1[k].cpu()) < 5e-3, k


def test_titok_loss_on_frames_equals_loss_on_their_images(hip):
    import train_titok as TT
    torch.manual_seed(0)
    model = TT.TiTok(TT.TiTokConfig(32, 8, 8, 64, 12, "S")).cuda()
    make = _frames32(B=3)
    table = None                                      # pixels in [0, 1], as the tokenizers take them
    images = make(table).images()
    with torch.no_grad():
        want = model.loss(images)
        got = model.loss(make(table))
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- the loader
class _Alarm:
    """a time limit of this test's own: a wait on an event that nothing will record must fail the test, not hold the session"""

    def __init__(self, seconds):
        self.seconds = seconds

    def _fire(self, *_):
        raise TimeoutError(f"DeviceLoader test exceeded {self.seconds} s")

    def __enter__(self):
        self.old = signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)
        signal.signal(signal.SIGALRM, self.old)


@pytest.mark.parametrize("train", [True, False])
def test_device_loader_yields_the_reference_and_reuses_slots_behind_their_events(hip, train):
    from vitamd import data
    n_batches, B = 8, 4
    g = torch.Generator().manual_seed(21)
    originals = [torch.randint(0, 256, (B, 11, 13, 3), generator=g, dtype=U8) for _ in range(n_batches)]
    labels = [torch.arange(B) + 10 * i for i in range(n_batches)]
    handed = []

    def host():
        for u8, lab in zip(originals, labels):
            pair = (u8.clone(), lab.clone())
            handed.append(pair)
            yield pair

    with _Alarm(60):
        loader = data.DeviceLoader(host(), "cuda", 8, patch=4, image=True, mean=MEAN[:3], std=STD[:3], train=train, seed=77, depth=2)
        seen = []
        for i, (frames, lab) in enumerate(loader):
            for u8, l in handed:                     # everything the loader has taken so far is overwritten at once
                u8.fill_(0)
                l.fill_(-1)
            seen.append((frames, lab, frames.geom))
        done = torch.cuda.Event()
        done.record()
        deadline = time.monotonic() + 30
        while not done.query():                      # polled, not waited on: a wait that never ends would hold the session past the alarm
            assert time.monotonic() < deadline, "the loader's work did not finish"
    assert len(seen) == n_batches and loader.step == n_batches
    for i, (frames, lab, geom) in enumerate(seen):
        want_geom = R.draw_ref(B, (11, 13), (8, 8), 77, i) if train else data.center_geom(B, (11, 13), (8, 8))
        assert torch.equal(geom.cpu(), want_geom)
        ref = R.frames_ref(originals[i], (8, 8), None, want_geom, MEAN[:3], STD[:3])
        assert _same(frames.images(), ref), i
        assert _same(frames.patches(4), R.patch_rows(ref, 4).to(BF16)), i
        assert lab.is_cuda and torch.equal(lab.cpu(), labels[i])


def test_video_bridge_takes_uint8_videos_and_returns_uint8_frames(hip):
    import train_tatitok as TA
    import train_videogpt as VG
    torch.manual_seed(0)
    tok = TA.TiTok(TA.TiTokConfig(32, 8, 8, 64, 12, "small")).cuda().eval()
    g = torch.Generator().manual_seed(4)
    videos = torch.randint(0, 256, (2, 3, 32, 32, 3), generator=g, dtype=U8).cuda()
    as_float = videos.permute(0, 1, 4, 2, 3).float().cpu().div(255).cuda()              # the CPU's division: the values the table holds
    want = VG.frames_to_tokens(tok, as_float)
    got = VG.frames_to_tokens(tok, videos)
    assert got.dtype == torch.int64 and got.shape == want.shape == (2, 3, 8) and torch.equal(got, want)
    window = torch.tensor([[1, 2], [4, 5]], device="cuda")                              # videos[:, 1:3] of the flattened frames
    assert torch.equal(VG.frames_to_tokens(tok, videos, index=window), want[:, 1:3])
    with pytest.raises(ValueError, match="uint8 videos"):
        VG.frames_to_tokens(tok, as_float, index=window)
    flat = want.reshape(2, -1)
    frames = VG.tokens_to_frames(tok, flat, 3)
    u8 = VG.tokens_to_frames(tok, flat, 3, as_u8=True)
    assert u8.dtype == U8 and u8.shape == (2, 3, 32, 32, 3)
    assert torch.equal(u8.cpu(), (frames.cpu() * 255).round().to(U8).permute(0, 1, 3, 4, 2))
