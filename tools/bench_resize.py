"""Resizing in the device input feed (csrc/resize.hip vitamd_frames_prep_resize, vitamd/resize.py) against the
route a user writes today, on one MI355X, at ViT-B/16 224 batch 256 from 256 x 320 uint8 frames.  Device-event timings, warmed, the
routes alternated round by round in one process, median of --rounds rounds with the spread (min .. max); prints one JSON line and
writes it to --out when given.  Before anything is timed routes (a) and (b) must agree.

  prep   - device time, uint8 frames on the device -> the bf16 patch rows of the batch (the records are on the device for all):
             a_torch:        the reference's transform with torch device ops: u8 -> float -> ONE batched
                             F.interpolate(antialias=True) of the whole frames to Resize(224)'s 224 x 280 -> per-sample crop and flip
                             (one gather) -> normalise -> ops.im2col
             b_resize_crop:  resize_crop_boxes (the same transform) through the one kernel
             c_rrc:          rrc_boxes (RandomResizedCrop, scale 0.08 - 1) through the one kernel.  No batched torch route exists for
                             per-sample boxes: F.interpolate takes one size ratio per call, so (c) has no torch column
             d_plain:        vitamd_frames_prep, a 224 x 224 crop of the same frames without resizing: the floor
  step   - a whole train_step, data included, host clock around --reps steps ending in a synchronise:
             device_loader:  DeviceLoader (random crop of the 256 x 320 frames) -> train_step
             resize_loader:  ResizeLoader mode rrc (host draw, staging copy, resizing prep) -> train_step
usage: bench_resize.py [--rounds N] [--reps N] [--skip-step] [--out FILE]"""
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
        raise SystemExit("bench_resize: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize: needs a GPU (no timing is taken without one)")
    import train_vit as TV
    from vitamd import data, ops, resize
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
    table = data.norm_table(data.IMAGENET_MEAN, data.IMAGENET_STD, device=dev)

    # ---- (1) the four prep routes
    box_b = resize.resize_crop_boxes(BATCH, SRC_HW, SIZE, SIZE, seed=1, step=0)
    box_c = resize.rrc_boxes(BATCH, SRC_HW, SIZE, seed=1, step=0)
    Hv, Wv = resize.resized_size(Hs, Ws, SIZE)
    bb, bc = box_b.to(dev), box_c.to(dev)
    geom = data.random_geom(BATCH, SRC_HW, (SIZE, SIZE), seed=1, step=0, device=dev)
    # (a)'s crop and flip as ONE advanced-indexing gather; its index grids are built outside the window
    ar = torch.arange(SIZE, device=dev)
    ys = (bb[:, 3:4].long() + ar[None, :])[:, None, :, None]
    xs = (bb[:, 7:8].long() + torch.where(bb[:, 8:9] != 0, SIZE - 1 - ar[None, :], ar[None, :]))[:, None, None, :]
    bs = torch.arange(BATCH, device=dev)[:, None, None, None]
    cs = torch.arange(3, device=dev)[None, :, None, None]

    def a_torch(want_image=False):
        x = u8.permute(0, 3, 1, 2).to(torch.float32)
        x = torch.nn.functional.interpolate(x, size=(Hv, Wv), mode="bilinear", antialias=True, align_corners=False)
        x = x[bs, cs, ys, xs].div(255).sub(mean_t[None, :, None, None]).div(std_t[None, :, None, None]).contiguous()
        return x if want_image else ops.im2col(x, PATCH)

    b_resize_crop = lambda: ops.frames_prep(u8, (SIZE, SIZE), None, PATCH, False, None, resize=(bb, mean_t, std_t))[0]
    c_rrc = lambda: ops.frames_prep(u8, (SIZE, SIZE), None, PATCH, False, None, resize=(bc, mean_t, std_t))[0]
    d_plain = lambda: ops.frames_prep(u8, (SIZE, SIZE), table, PATCH, False, None, geom)[0]

    img_a = a_torch(want_image=True)
    img_b = ops.frames_prep(u8, (SIZE, SIZE), None, None, True, None, resize=(bb, mean_t, std_t))[1]
    diff = float((img_a - img_b).abs().max())
    if not diff <= 1e-3:                             # torch's fp32 antialias kernel and this one each sit near 1e-6 of float64
        raise SystemExit(f"bench_resize: the torch route and the kernel disagree (max abs diff {diff})")
    rows_a, rows_b = a_torch(), b_resize_crop()
    share = float((rows_a.view(torch.int16) == rows_b.view(torch.int16)).float().mean())
    del img_a, img_b, rows_a, rows_b
    k = _alternate({"a_torch": a_torch, "b_resize_crop": b_resize_crop, "c_rrc": c_rrc, "d_plain": d_plain}, args.rounds, args.reps, _device_ms)
    k["a_b_image_max_abs_diff"] = diff
    k["a_b_patch_rows_bit_equal_share"] = round(share, 6)
    k["speedup_b_over_a"] = round(k["a_torch"]["median"] / k["b_resize_crop"]["median"], 2)
    k["b_over_d"] = round(k["b_resize_crop"]["median"] / k["d_plain"]["median"], 2)
    k["c_over_d"] = round(k["c_rrc"]["median"] / k["d_plain"]["median"], 2)
    rows_bytes = BATCH * 3 * SIZE * SIZE * 2
    area_c = int((box_c[:, 1].long() * box_c[:, 5].long()).sum())
    k["bytes"] = {"b_resize_crop": BATCH * Hs * Ws * 3 + rows_bytes, "c_rrc": area_c * 3 + rows_bytes, "d_plain": BATCH * SIZE * SIZE * 3 + rows_bytes}
    k["GBps"] = {r: round(k["bytes"][r] / (k[r]["median"] * 1e-3) / 1e9, 1) for r in k["bytes"]}
    k["rrc_mean_box"] = [round(float(box_c[:, 1].float().mean()), 1), round(float(box_c[:, 5].float().mean()), 1)]
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
        plain = data.DeviceLoader(forever(), dev, SIZE, **kw)
        resized = resize.ResizeLoader(forever(), dev, SIZE, mode="rrc", **kw)

        def device_loader():
            x, y = next(plain)
            TV.train_step(model, x, y, optim)

        def resize_loader():
            x, y = next(resized)
            TV.train_step(model, x, y, optim)

        out["step"] = _alternate({"device_loader": device_loader, "resize_loader": resize_loader}, args.rounds, args.reps, _host_ms)
        out["step"]["images_per_s"] = {r: round(BATCH / (out["step"][r]["median"] * 1e-3), 1) for r in ("device_loader", "resize_loader")}
        out["step"]["resize_over_plain"] = round(out["step"]["resize_loader"]["median"] / out["step"]["device_loader"]["median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
