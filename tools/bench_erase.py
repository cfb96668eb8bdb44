"""Random Erasing as a post-pass of the device input feed (csrc/erase.hip vitamd_frames_erase, vitamd/erase.py)
against the route a user of the fused feed writes without it, on one MI355X, at ViT-B/16 224 batch 256 from 256 x 256 uint8 frames,
Erase() defaults (probability 0.25, per-pixel noise).  Device-event timings, warmed, the routes alternated round by round in one
process, median of --rounds rounds with the spread (min .. max); prints one JSON line and writes it to --out when given.  Before
anything is timed the routes must agree outside the boxes, bit for bit (inside, each draws its own noise).

  prep   - device time, uint8 frames on the device -> the bf16 patch rows:
             plain:  the prep launch alone (nothing erased: what the feed costs today)
             erase:  the prep launch, then vitamd_frames_erase on its patch rows (the record is on the device)
             torch:  Frames.images() (the prep kernel, fp32 batch out), a slice assignment of torch.randn per erased sample, ops.im2col
  step   - a whole train_step, data included, host clock around --reps steps ending in a synchronise:
             resize_mix_loader:        ResizeMixLoader mode rrc, Mix(0.8, 1.0) -> train_step with SoftTargetLoss(0.1)
             erase_resize_mix_loader:  EraseResizeMixLoader, the same with Erase() behind it
usage: bench_erase.py [--rounds N] [--reps N] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_input import _alternate, _device_ms, _host_ms  # noqa: E402

BATCH, SRC, SIZE, PATCH, CLASSES, SMOOTHING = 256, 256, 224, 16, 1000, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_erase: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_erase: needs a GPU (no timing is taken without one)")
    import train_vit as TV
    from vitamd import data, erase, mix, ops
    from vitamd.functions import claim_streams
    dev = torch.device("cuda", 0)
    claim_streams(dev)
    gen = torch.Generator().manual_seed(0)
    out = {"rounds": args.rounds, "reps": args.reps, "batch": BATCH, "src": [BATCH, SRC, SRC, 3], "out": [BATCH, 3, SIZE, SIZE], "patch": PATCH}
    u8_host = torch.randint(0, 256, (BATCH, SRC, SRC, 3), generator=gen, dtype=torch.uint8)
    labels_host = torch.randint(0, CLASSES, (BATCH,), generator=gen)
    u8 = u8_host.to(dev)
    table = data.norm_table(data.IMAGENET_MEAN, data.IMAGENET_STD, device=dev)
    geom = data.random_geom(BATCH, (SRC, SRC), (SIZE, SIZE), seed=1, step=0, device=dev)

    # ---- (1) prep, prep + erase, and the torch route
    er = erase.Erase(seed=1)
    rec_h, fill_h = er.draw(BATCH, (SIZE, SIZE), 0)
    rec, fill = rec_h.to(dev), fill_h.to(dev)
    boxes = [(b, *row[0][1:]) for b, row in enumerate(rec_h.tolist()) if row[0][0]]
    erased_px = sum((yh - yl) * (xh - xl) for _, yl, yh, xl, xh in boxes)
    out["record"] = {"erased_samples": len(boxes), "erased_share_of_pixels": round(erased_px / (BATCH * SIZE * SIZE), 4),
                     "bytes_written_bf16": erased_px * 3 * 2}

    def plain():
        return ops.frames_prep(u8, (SIZE, SIZE), table, PATCH, False, None, geom)[0]

    def fused():
        rows = plain()
        ops.frames_erase(rows, None, PATCH, rec, fill, 1, 0, hw=(SIZE, SIZE))
        return rows

    def torch_route():
        x = data.Frames(u8, SIZE, geom=geom, table=table).images()
        for b, yl, yh, xl, xh in boxes:
            x[b, :, yl:yh, xl:xh] = torch.randn((3, yh - yl, xh - xl), device=dev)
        return ops.im2col(x, PATCH)

    mask = torch.zeros((BATCH, 3, SIZE, SIZE), device=dev)
    for b, yl, yh, xl, xh in boxes:
        mask[b, :, yl:yh, xl:xh] = 1
    inside = ops.im2col(mask, PATCH) != 0
    base, got, want = plain(), fused(), torch_route()
    for name, rows in (("fused", got), ("torch", want)):
        same = rows.view(torch.int16) == base.view(torch.int16)
        if not bool(same[~inside].all()) or not bool(torch.isfinite(rows.float()).all()) or float(same[inside].float().mean()) > 0.01:
            raise SystemExit(f"bench_erase: the {name} route does not leave the plain rows outside the boxes and new values inside")
    out["prep"] = _alternate({"plain": plain, "erase": fused, "torch": torch_route}, args.rounds, args.reps, _device_ms)
    out["prep"]["erase_minus_plain_ms"] = round(out["prep"]["erase"]["median"] - out["prep"]["plain"]["median"], 4)
    out["prep"]["torch_over_erase"] = round(out["prep"]["torch"]["median"] / out["prep"]["erase"]["median"], 2)
    del base, got, want, mask, inside

    # ---- (2) whole training steps, data included
    if not args.skip_step:
        torch.manual_seed(0)
        model = TV.ViTClassifier(TV.ViTConfig(SIZE, 3, PATCH, "B", 1, 0.0), CLASSES).to(dev)
        optim = torch.optim.AdamW(model.parameters(), lr=1e-4)
        u8_pinned = u8_host.pin_memory()

        def forever():
            while True:
                yield u8_pinned, labels_host

        kw = dict(mode="rrc", patch=PATCH, image=False, mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, train=True, seed=1)
        m = mix.Mix(0.8, 1.0, label_smoothing=SMOOTHING, seed=1)
        mixed = mix.ResizeMixLoader(forever(), dev, SIZE, m, **kw)
        erasing = erase.EraseResizeMixLoader(forever(), dev, SIZE, m, erase=erase.Erase(seed=1), **kw)
        soft = mix.SoftTargetLoss(SMOOTHING)

        def resize_mix_loader():
            x, y = next(mixed)
            TV.train_step(model, x, y, optim, loss_fn=soft)

        def erase_resize_mix_loader():
            x, y = next(erasing)
            TV.train_step(model, x, y, optim, loss_fn=soft)

        routes = {"resize_mix_loader": resize_mix_loader, "erase_resize_mix_loader": erase_resize_mix_loader}
        out["step"] = _alternate(routes, args.rounds, args.reps, _host_ms)
        out["step"]["images_per_s"] = {r: round(BATCH / (out["step"][r]["median"] * 1e-3), 1) for r in routes}
        out["step"]["erase_over_plain"] = round(out["step"]["erase_resize_mix_loader"]["median"] / out["step"]["resize_mix_loader"]["median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
