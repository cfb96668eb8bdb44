"""Mixup / CutMix on resized samples in the launch that resizes (csrc/resize.hip vitamd_frames_prep_resize_mix, vitamd/mix.py
MixedResizedFrames / ResizeMixLoader) against the route that existed before it, on one MI355X, at ViT-B/16 224
batch 256 from 256 x 320 uint8 frames cut by rrc_boxes.  Device-event timings, warmed, the routes alternated round by round in one
process, median of --rounds rounds with the spread (min .. max); prints one JSON line and writes it to --out when given.  Before
anything is timed routes (a) and (b) must give the same patch rows, bit for bit.

  prep   - device time, uint8 frames on the device -> the bf16 patch rows of the MIXED batch (every record is on the device):
             a_mixup / a_cutmix:  ResizedFrames.images() (the resizing kernel, fp32 image out), then torch on the fp32 batch - mul / add
                                  with the reversed batch, or the slice copy of the box from the reversed batch - then ops.im2col
             b_mixup / b_cutmix:  the one launch, every row mode 1 (one lam) or mode 2 (one box), as Mix's batch-wise draw gives it
             b_none:              the one launch with an all-mode-0 record
             c_resize:            plain vitamd_frames_prep_resize of the same boxes: the floor
  step   - a whole train_step, data included, host clock around --reps steps ending in a synchronise:
             resize_loader:       ResizeLoader mode rrc -> train_step with the hard-label loss
             resize_mix_loader:   ResizeMixLoader mode rrc, Mix(0.8, 1.0) -> train_step with SoftTargetLoss(0.1)
usage: bench_resize_mix.py [--rounds N] [--reps N] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_input import _alternate, _device_ms, _host_ms  # noqa: E402

BATCH, SRC_HW, SIZE, PATCH, CLASSES = 256, (256, 320), 224, 16, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_resize_mix: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize_mix: needs a GPU (no timing is taken without one)")
    import train_vit as TV
    from vitamd import data, mix, ops, resize
    from vitamd.functions import claim_streams
    dev = torch.device("cuda", 0)
    claim_streams(dev)
    gen = torch.Generator().manual_seed(0)
    Hs, Ws = SRC_HW
    out = {"rounds": args.rounds, "reps": args.reps, "batch": BATCH, "src": [BATCH, Hs, Ws, 3], "out": [BATCH, 3, SIZE, SIZE], "patch": PATCH}
    u8_host = torch.randint(0, 256, (BATCH, Hs, Ws, 3), generator=gen, dtype=torch.uint8)
    labels_host = torch.randint(0, CLASSES, (BATCH,), generator=gen)
    u8 = u8_host.to(dev)
    mean_t = torch.tensor(data.IMAGENET_MEAN, device=dev)
    std_t = torch.tensor(data.IMAGENET_STD, device=dev)

    # ---- (1) the prep routes
    box = resize.rrc_boxes(BATCH, SRC_HW, SIZE, seed=1, step=0).to(dev)
    rec_m, lam_m = mix.Mix(0.8, 0.0, seed=1).draw(BATCH, SIZE, 0)                # every row Mixup with one lam
    rec_c, lam_c = mix.Mix(0.0, 1.0, seed=3).draw(BATCH, SIZE, 0)                # every row CutMix with one box (169 x 182: 61 % of the image)
    rec_0 = rec_m.clone()
    rec_0[:, 1] = 0
    assert set(rec_m[:, 1].tolist()) == {1} and set(rec_c[:, 1].tolist()) == {2}
    l = float(lam_m[0])
    m = float(1 - lam_m[0])                                                      # fl32(1 - l), as the kernel forms it
    yl, yh, xl, xh = rec_c[0, 2:].tolist()
    dm, dc, d0 = (rec_m.to(dev), lam_m.to(dev)), (rec_c.to(dev), lam_c.to(dev)), (rec_0.to(dev), lam_m.to(dev))

    def images():
        return resize.ResizedFrames(u8, SIZE, box, mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD).images()

    def a_mixup():
        x = images()
        return ops.im2col(x.mul(l).add_(x.flip(0).mul_(m)), PATCH)

    def a_cutmix():
        x = images()
        x[:, :, yl:yh, xl:xh] = x[:, :, yl:yh, xl:xh].flip(0)                # the box alone is mirrored along the batch, not the whole batch
        return ops.im2col(x, PATCH)

    one = lambda pair: ops.frames_prep_resize_mix(u8, (SIZE, SIZE), PATCH, False, None, box, mean_t, std_t, *pair)[0]
    b_mixup, b_cutmix, b_none = (lambda: one(dm)), (lambda: one(dc)), (lambda: one(d0))
    c_resize = lambda: ops.frames_prep(u8, (SIZE, SIZE), None, PATCH, False, None, resize=(box, mean_t, std_t))[0]

    for name, fa, fb in (("mixup", a_mixup, b_mixup), ("cutmix", a_cutmix, b_cutmix), ("none", c_resize, b_none)):
        ra, rb = fa(), fb()
        if not torch.equal(ra.view(torch.int16), rb.view(torch.int16)):
            share = float((ra.view(torch.int16) == rb.view(torch.int16)).float().mean())
            raise SystemExit(f"bench_resize_mix: the two routes disagree for {name} (bit-equal share of the patch rows {share:.6f})")
        del ra, rb
    k = _alternate({"a_mixup": a_mixup, "b_mixup": b_mixup, "a_cutmix": a_cutmix, "b_cutmix": b_cutmix, "b_none": b_none, "c_resize": c_resize},
                   args.rounds, args.reps, _device_ms)
    k["lam_mixup"], k["cutmix_box"], k["cutmix_box_share"] = l, [yl, yh, xl, xh], round((yh - yl) * (xh - xl) / (SIZE * SIZE), 4)
    for r in ("mixup", "cutmix"):
        k[f"speedup_b_over_a_{r}"] = round(k[f"a_{r}"]["median"] / k[f"b_{r}"]["median"], 2)
        k[f"b_{r}_over_c"] = round(k[f"b_{r}"]["median"] / k["c_resize"]["median"], 2)
    k["b_none_over_c"] = round(k["b_none"]["median"] / k["c_resize"]["median"], 3)
    out["prep"] = k

    # ---- (2) whole training steps, data included
    if not args.skip_step:
        torch.manual_seed(0)
        model = TV.ViTClassifier(TV.ViTConfig(SIZE, 3, PATCH, "B", 1, 0.0), CLASSES).to(dev)
        optim = torch.optim.AdamW(model.parameters(), lr=1e-4)
        u8_pinned = u8_host.pin_memory()

        def forever():
            while True:
                yield u8_pinned, labels_host

        kw = dict(patch=PATCH, image=False, mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, train=True, seed=1)
        resized = resize.ResizeLoader(forever(), dev, SIZE, mode="rrc", **kw)
        mixed = mix.ResizeMixLoader(forever(), dev, SIZE, mix.Mix(0.8, 1.0, label_smoothing=0.1, seed=1), mode="rrc", **kw)
        soft = mix.SoftTargetLoss(0.1)

        def resize_loader():
            x, y = next(resized)
            TV.train_step(model, x, y, optim)

        def resize_mix_loader():
            x, y = next(mixed)
            TV.train_step(model, x, y, optim, loss_fn=soft)

        out["step"] = _alternate({"resize_loader": resize_loader, "resize_mix_loader": resize_mix_loader}, args.rounds, args.reps, _host_ms)
        out["step"]["images_per_s"] = {r: round(BATCH / (out["step"][r]["median"] * 1e-3), 1) for r in ("resize_loader", "resize_mix_loader")}
        out["step"]["mix_over_plain"] = round(out["step"]["resize_mix_loader"]["median"] / out["step"]["resize_loader"]["median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
