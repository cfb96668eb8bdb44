"""Random Erasing on the GPU (csrc/erase.hip vitamd_frames_erase, vitamd.ops.frames_erase, vitamd.erase) against tests/_erase_ref.py.

The contract (include/vitamd.h): outside every box the bits of the prep output stay; a mode-1 pixel holds fill[b, k, c] exactly; a
mode-2 pixel lies within 6 * 2^-23 * max(r, 1) of the float64 Box-Muller value of (seed, step, b, c, y, x) (r = sqrt(-2 ln u1): three
1-ulp operations give 3 * 2^-23 * r, doubled); under several boxes the largest k writes; the bf16 rows are the round-to-nearest-even
im2col of the image, whether they were erased in the same launch or in one of their own.  Every output is a copy of a real prep
output between two guards of 0xFF bytes.  The largest measured ratio to the noise bound is printed by every case."""
import functools

import numpy as np
import pytest
import torch

import _erase_ref as R

pytestmark = pytest.mark.gpu
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
GUARD = 64
SEED, STEP = (1 << 40) + 3, (1 << 33) + 9            # both words of both counters in use

# name -> (B, C, H, W, p, offset of the image in fp32 elements)
CASES = {
    "fast":   (5, 3, 32, 32, 8, 0),
    "c1":     (5, 1, 32, 32, 8, 0),
    "c4":     (5, 4, 32, 32, 8, 0),
    "w30_p5": (5, 3, 30, 30, 5, 0),                  # W % 4 != 0: the boxes that reach 32 are clamped to 30
    "p6":     (5, 3, 36, 36, 6, 0),                  # p % 4 != 0: one element at a time with patch rows, groups of 4 with the image alone
    "off4":   (5, 3, 32, 32, 8, 1),                  # the image 4 bytes off its 16-byte alignment
}


def _same(a, b):
    it = {F32: torch.int32, BF16: torch.int16}
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().contiguous().view(it[a.dtype]), b.cpu().contiguous().view(it[b.dtype]))


@functools.lru_cache(maxsize=None)
def _before(B, C, H, W, p, seed=0):
    """the prep output of seeded frames -> (patch rows, image) on the device; launched once per shape, never written to"""
    from vitamd import data
    g = torch.Generator().manual_seed(100 + seed)
    src = torch.randint(0, 256, (B, H + 3, W + 5, C), generator=g, dtype=U8).cuda()
    mean, std = (0.485, 0.456, 0.406, 0.5)[:C], (0.229, 0.224, 0.225, 0.25)[:C]
    f = data.Frames(src, (H, W), geom=torch.tensor([[b % 4, (2 * b) % 6, b & 1] for b in range(B)], dtype=torch.int32),
                    table=data.norm_table(mean, std, channels=C))
    return f.patches(p), f.images()


def _guarded(t, off=0):
    """a copy of device tensor t between two guards of 0xFF bytes, `off` elements further in -> (the whole buffer as integers, the copy)"""
    n = t.numel()
    whole = torch.full((n + 2 * GUARD + off,), -1, dtype={F32: torch.int32, BF16: torch.int16}[t.dtype], device="cuda")
    mid = whole.view(t.dtype)[GUARD + off:GUARD + off + n].view(t.shape)
    mid.copy_(t)
    return whole, mid


def _erase(rows0, img0, p, rec, fill, want_patches=True, want_image=True, off=0, seed=SEED, step=STEP):
    """ops.frames_erase on guarded copies of the prep output -> (rows or None, image or None) on the CPU, the guards checked"""
    from vitamd import ops
    pw = iw = rows = img = None
    if want_patches:
        pw, rows = _guarded(rows0)
    if want_image:
        iw, img = _guarded(img0, off)
        assert img.data_ptr() % 16 == (4 * off) % 16
    assert ops.frames_erase(rows, img, p if want_patches else None, rec.cuda(), None if fill is None else fill.cuda(), seed, step,
                            hw=tuple(img0.shape[2:])) is None
    torch.cuda.synchronize()
    for whole, o, t in ((pw, 0, rows), (iw, off, img)):
        if whole is not None:
            assert bool((whole[:GUARD + o] == -1).all()) and bool((whole[GUARD + o + t.numel():] == -1).all()), "a guard was written"
    return None if rows is None else rows.cpu(), None if img is None else img.cpu()


def _hold(name, rows0, img0, p, rec, fill, off=0, seed=SEED, step=STEP):
    """every check of the contract on one record -> the erased (rows, image)"""
    from vitamd import ops
    assert _same(rows0, ops.im2col(img0, p))                                # the before state is a prep output
    ref = R.erase_ref(img0.cpu(), rec, fill, seed, step)
    rows, img = _erase(rows0, img0, p, rec, fill, off=off, seed=seed, step=step)
    fails, ratio = R.check_erased(img, img0.cpu(), ref)
    print(f"{name}: {int((ref['kind'] == 2).sum())} noise and {int((ref['kind'] == 1).sum())} fill elements, worst noise error / bound {ratio:.4f}")
    assert not fails, fails
    assert _same(rows, ops.im2col(img.cuda(), p).cpu())                     # the rows the unfused route makes of the erased image
    only_rows, none_i = _erase(rows0, img0, p, rec, fill, want_image=False, seed=seed, step=step)
    none_r, only_img = _erase(rows0, img0, p, rec, fill, want_patches=False, off=off, seed=seed, step=step)
    assert none_i is None and none_r is None and _same(only_rows, rows) and _same(only_img, img)     # separate launches agree
    again = _erase(rows0, img0, p, rec, fill, off=off, seed=seed, step=step)
    assert _same(again[0], rows) and _same(again[1], img)                   # the same bits on every call
    return rows, img, ref


def _fill(B, K, seed=5):
    return torch.randn((B, K, 4), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("name", list(CASES))
def test_boxes_are_rewritten_and_nothing_else_in_every_form(name):
    B, C, H, W, p, off = CASES[name]
    rows0, img0 = _before(B, C, H, W, p)
    rec, fill = torch.tensor(R.FAST_RECORD, dtype=torch.int32), _fill(B, 2)
    rows, img, ref = _hold(name, rows0, img0, p, rec, fill, off=off)
    assert {0, 1, 2} == set(np.unique(ref["kind"]).tolist())
    assert _same(img[4], img0[4].cpu())                                     # the sample without a box
    win = R.winners(rec, H, W)
    assert (win[0, 12, 4:min(28, W)] == 1).all() and win[0, 12, 2] == 0 and win[1, 25, 20] == 1 and win[1, 25, 5] == 0       # both overlaps are in the case
    # NULL fill is zeros
    _, zero = _erase(rows0, img0, p, rec, None, want_patches=False)
    kind = torch.from_numpy(ref["kind"])
    assert bool((zero[kind == 1] == 0).all()) and _same(zero[kind != 1], img[kind != 1])


def test_device_noise_is_standard_normal_within_the_caps_of_the_reference():
    """seed 0, step 0, one 3 x 64 x 64 box: the caps test_erase_host.py holds the reference noise to"""
    rows0, img0 = _before(1, 3, 64, 64, 16)
    rec = torch.tensor([[[2, 0, 64, 0, 64]]], dtype=torch.int32)
    rows, img, ref = _hold("moments", rows0, img0, 16, rec, None, seed=0, step=0)
    assert (ref["kind"] == 2).all() and R.moments_ok(img.numpy())


def test_noise_does_not_depend_on_patch_size_output_batch_size_or_box():
    from vitamd import data, erase, ops
    B, C, H, W = 7, 3, 32, 32
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, 256, (B, H, W, C), generator=g, dtype=U8).cuda()
    e = erase.Erase(probability=1.0, max_count=2, seed=4)
    pair = e.draw(B, (H, W), 11)
    # patches(8), patches(16) and images() of one erased batch: three launches of the prep kernel, three of the erasing kernel
    f = erase.erased(data.Frames(src, (H, W)), pair, SEED, STEP)
    rows8, rows16, img = f.patches(8), f.patches(16), f.images()
    assert isinstance(f, data.Frames) and _same(rows8, ops.im2col(img, 8)) and _same(rows16, ops.im2col(img, 16))
    plain = data.Frames(src, (H, W)).images()
    fails, ratio = R.check_erased(img.cpu(), plain.cpu(), R.erase_ref(plain.cpu(), pair[0], pair[1], SEED, STEP))
    assert not fails, fails
    # sample b at B = 3 and at B = 7
    f3 = erase.erased(data.Frames(src[:3], (H, W)), (pair[0][:3], pair[1][:3]), SEED, STEP)
    assert _same(f3.images(), img[:3])
    # another box over the same pixels: the same values where both cover
    whole = torch.tensor([[[2, 0, H, 0, W]]] * B, dtype=torch.int32)
    full = erase.erased(data.Frames(src, (H, W)), (whole, None), SEED, STEP).images().cpu()
    noise = torch.from_numpy(R.erase_ref(plain.cpu(), pair[0], pair[1], SEED, STEP)["kind"] == 2)
    assert bool(noise.any()) and _same(full[noise], img.cpu()[noise])
    # another step, another seed: other values
    for seed, step in ((SEED, STEP + 1), (SEED + 1, STEP), (SEED, STEP + (1 << 32)), (SEED + (1 << 32), STEP)):
        other = erase.erased(data.Frames(src, (H, W)), (whole, None), seed, step).images().cpu()
        assert float((other == full).float().mean()) < 0.01


def test_more_units_than_the_grid_cap(hip):
    """many 8 x 8 samples, each with a box: (sample, box, strip) units beyond vitamd_frames_erase_grid_cap() are reached by the stride loop"""
    from vitamd import ops
    cap = ops.frames_erase_grid_cap()
    assert cap == hip.vitamd_frames_erase_grid_cap()
    B = cap // 32 + 37                                                      # 32 strips per box (include/vitamd.h)
    rows0, img0 = _before(B, 3, 8, 8, 4)
    rec = torch.tensor([[[1 + (b & 1), b % 3, 4 + b % 5, b % 4, 3 + b % 6]] for b in range(B)], dtype=torch.int32)
    assert B * 32 > cap
    rows, img, ref = _hold("grid cap", rows0, img0, 4, rec, _fill(B, 1))
    assert all((ref["kind"][b] != 0).any() for b in range(B))


# ---------------------------------------------------------------------------------------------- the loaders
def _host(n_batches, B=6, classes=10):
    g = torch.Generator().manual_seed(21)
    batches = [(torch.randint(0, 256, (B, 40, 48, 3), generator=g, dtype=U8), torch.randint(0, classes, (B,), generator=g)) for _ in range(n_batches)]
    return iter(batches)


@pytest.mark.parametrize("which", ["mix", "resize_mix"])
def test_erasing_loaders_are_their_parents_outside_the_boxes(which):
    from vitamd import data, erase, mix
    e = erase.Erase(probability=0.7, max_count=2, seed=3)
    m = mix.Mix(seed=2, per_sample=True)
    kw = dict(patch=8, image=True, mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, seed=5)
    parent_cls, child_cls = (mix.MixLoader, erase.EraseMixLoader) if which == "mix" else (mix.ResizeMixLoader, erase.EraseResizeMixLoader)
    for train in (True, False):
        parent = parent_cls(_host(2), "cuda", 32, m, train=train, **kw)
        child = child_cls(_host(2), "cuda", 32, m, erase=e, train=train, **kw)
        seen = 0
        for step, ((pf, pl), (cf, cl)) in enumerate(zip(parent, child)):
            assert isinstance(cf, type(pf)) and isinstance(cf, erase._Erased) == train
            p_img, c_img, p_rows, c_rows = pf.images().cpu(), cf.images().cpu(), pf.patches(8), cf.patches(8)
            if train:
                rec, fill = e.draw(6, (32, 32), step)
                assert torch.equal(cf.erase[0].cpu(), rec)
                ref = R.erase_ref(p_img, rec, fill, e.seed, step)
                fails, ratio = R.check_erased(c_img, p_img, ref)
                assert not fails, fails
                seen += int((ref["kind"] == 2).sum())
                from vitamd import ops
                assert _same(c_rows, ops.im2col(cf.images(), 8))
                assert all(torch.equal(a, b) for a, b in zip(pl, cl))       # MixedLabels: a, b, lam
            else:
                assert _same(c_img, p_img) and _same(c_rows, p_rows) and torch.equal(pl, cl)
        assert step == 1 and (seen > 0) == train


def test_an_erased_batch_feeds_a_training_step():
    import train_vit as TV
    from vitamd import data, erase
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (8, 32, 32, 3), generator=g, dtype=U8).cuda()
    labels = torch.randint(0, 10, (8,), generator=g).cuda()
    model = TV.ViTClassifier(TV.ViTConfig(32, 3, 16, "S", 1, 0.0), num_classes=10).cuda()
    optim = torch.optim.AdamW(model.parameters(), lr=1e-4)
    e = erase.Erase(probability=1.0)
    frames = erase.erased(data.Frames(u8, 32, table=data.norm_table(data.IMAGENET_MEAN, data.IMAGENET_STD)), e.draw(8, 32, 0), 0, 0)
    loss = TV.train_step(model, frames, labels, optim)
    assert bool(torch.isfinite(loss)) and 16 in frames._patches
    plain = data.Frames(u8, 32, table=data.norm_table(data.IMAGENET_MEAN, data.IMAGENET_STD)).patches(16)
    assert not _same(frames.patches(16), plain)


# ---------------------------------------------------------------------------------------------- the refusals
def test_every_refusal_is_answered_with_nothing_written(hip):
    B, C, H, W, p = 3, 3, 8, 8, 4
    rows0, img0 = _before(B, C, H, W, p)
    rec = torch.tensor([[[2, 0, 8, 0, 8]]] * B, dtype=torch.int32).cuda()
    fill = _fill(B, 1).cuda()
    SHAPE, ARG = 1, 2
    cases = [(SHAPE, bad) for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=5), dict(K=0), dict(K=9), dict(p=0), dict(p=3),
                                      dict(H=12, p=8), dict(B=1 << 20, H=1 << 11, W=1 << 11, p=1), dict(B=1 << 30, C=1, H=1, W=1, p=1),
                                      dict(B=1, C=4, H=(1 << 30) + 4, W=4, p=4))]
    cases += [(ARG, dict(rec=None)), (ARG, dict(patches=None, image=None))]
    for expect, bad in cases:
        pw, rows = _guarded(rows0)
        iw, img = _guarded(img0)
        a = dict(patches=rows.data_ptr(), image=img.data_ptr(), B=B, C=C, H=H, W=W, p=p, rec=rec.data_ptr(), fill=fill.data_ptr(), K=1)
        a.update(bad)
        code = hip.vitamd_frames_erase(a["patches"], a["image"], a["B"], a["C"], a["H"], a["W"], a["p"], a["rec"], a["fill"], a["K"], SEED, STEP,
                                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert code == expect, (code, expect, bad)
        assert _same(rows, rows0) and _same(img, img0), bad
        assert bool((pw[:GUARD] == -1).all()) and bool((pw[-GUARD:] == -1).all()) and bool((iw[:GUARD] == -1).all()) and bool((iw[-GUARD:] == -1).all())
