"""The device input pipeline (csrc/input.hip, vitamd/data.py) against the route a user writes today, on one MI355X,
at ViT-B/16 224 batch 256 (random crop + flip from 256 x 256 frames, ImageNet normalisation) and at TiTok-S 256 batch 256 (frames scaled
to [0, 1]).  Device-event timings, warmed, the routes alternated round by round in one process, median of --rounds rounds with the
spread (min .. max); prints one JSON line and writes it to --out when given.  Before anything is timed the routes must agree (to an fp32 ulp;
the share of bit-equal values is reported).

  kernel - device time, uint8 frames on the device -> bf16 patch rows (+ the fp32 image where the model's loss needs one):
             torch:  one gather for crop + flip, permute, to(float).div(255).sub(mean).div(std) with torch ops, then ops.im2col
             prep:   vitamd_frames_prep, one launch (the crop geometry is drawn once, outside the window, for both)
           with the kernel's algorithmic bytes (1 in, 4 fp32 out, 2 bf16 out per pixel and channel) over its time
  h2d    - the copy alone: the fp32 NCHW batch against the uint8 frames, both from pinned memory
  step   - a whole train_step, data included, host clock around --reps steps ending in a synchronise:
             fp32_h2d: per step, the normalised fp32 batch is copied from pinned memory and handed to train_step (the present route;
                       its CPU-side transform is NOT in the window, which favours it)
             u8_loader: per step, the uint8 frames go through DeviceLoader (pinned staging copy on the host included) to train_step
             resident: the fp32 batch already on the device - what bench.py times - as the floor
usage: bench_input.py [--rounds N] [--reps N] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))

BATCH = 256


def _stats(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def _device_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def _host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _alternate(routes, rounds, reps, timer):
    for fn in routes.values():
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(timer(fn, reps))
    return {k: dict(_stats(v), unit="ms") for k, v in times.items()}


def torch_route(u8, geom, mean, std, size, patch, ops):
    """the same frames -> (patch rows, fp32 image) with torch device ops and ops.im2col: what a user writes today on the device"""
    H = W = size
    if geom is not None:          # crop and flip as ONE advanced-indexing gather on the uint8 frames; its index grids are built outside the window
        g = geom.long()
        ar_h, ar_w = torch.arange(H, device=u8.device), torch.arange(W, device=u8.device)
        ys = (g[:, 0:1] + ar_h[None, :])[:, :, None]
        xs = (g[:, 1:2] + torch.where(g[:, 2:3] != 0, W - 1 - ar_w[None, :], ar_w[None, :]))[:, None, :]
        bs = torch.arange(u8.shape[0], device=u8.device)[:, None, None]

    def run():
        x = u8[bs, ys, xs] if geom is not None else u8
        x = x.permute(0, 3, 1, 2).to(torch.float32).div(255)
        if mean is not None:
            x = x.sub(mean).div(std)
        x = x.contiguous()
        return ops.im2col(x, patch), x
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_input: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_input: needs a GPU (no timing is taken without one)")
    import train_titok as TT
    import train_vit as TV
    from vitamd import data, ops
    from vitamd.functions import claim_streams
    dev = torch.device("cuda", 0)
    claim_streams(dev)
    gen = torch.Generator().manual_seed(0)
    out = {"rounds": args.rounds, "reps": args.reps, "batch": BATCH}

    shapes = {
        "vit_b16_224": dict(src=256, size=224, patch=16, mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, image=False, train=True),
        "titok_s_256": dict(src=256, size=256, patch=16, mean=None, std=None, image=True, train=False),
    }
    for name, c in shapes.items():
        size, patch = c["size"], c["patch"]
        u8_host = torch.randint(0, 256, (BATCH, c["src"], c["src"], 3), generator=gen, dtype=torch.uint8)
        labels_host = torch.randint(0, 1000, (BATCH,), generator=gen)
        u8 = u8_host.to(dev)
        table = data.norm_table(c["mean"], c["std"], device=dev)
        geom = data.random_geom(BATCH, (c["src"],) * 2, (size,) * 2, seed=1, step=0, device=dev) if c["train"] else None
        mean = None if c["mean"] is None else torch.tensor(c["mean"], device=dev)[None, :, None, None]
        std = None if c["std"] is None else torch.tensor(c["std"], device=dev)[None, :, None, None]
        res = out[name] = {"src": [BATCH, c["src"], c["src"], 3], "out": [BATCH, 3, size, size], "patch": patch, "image_output": c["image"]}

        # ---- (1) the kernel against the torch-op route, same frames, same geometry; bit-equal first
        tr = torch_route(u8, geom, mean, std, size, patch, ops)
        want_p, want_i = tr()
        got_p, got_i = ops.frames_prep(u8, (size, size), table, patch, True, None, geom)
        # the kernel's values are the CPU's (tests/test_gpu_data.py holds it to them bit for bit); torch's DEVICE ops may round a division
        # by a scalar differently, so the two device routes are held to an fp32 ulp here and the exact share is reported
        diff = float((got_i - want_i).abs().max())
        if not diff <= 2.0 ** -21 * float(want_i.abs().max()):
            raise SystemExit(f"bench_input: {name}: the kernel and the torch route disagree by {diff}")
        res["agreement"] = {"image_max_abs_diff": diff, "image_bit_equal_share": round(float((got_i == want_i).float().mean()), 6),
                            "patch_rows_bit_equal_share": round(float((got_p.view(torch.int16) == want_p.view(torch.int16)).float().mean()), 6)}
        px = BATCH * 3 * size * size
        nbytes = px * (1 + 2 + (4 if c["image"] else 0))
        k = _alternate({"torch": tr, "prep": lambda: ops.frames_prep(u8, (size, size), table, patch, c["image"], None, geom)},
                       args.rounds, args.reps, _device_ms)
        k["prep"]["algorithmic_MB"] = round(nbytes / 1e6, 1)
        k["prep"]["GB_per_s"] = round(nbytes / (k["prep"]["median"] * 1e-3) / 1e9, 1)
        res["kernel"] = k
        del want_p, want_i, got_p, got_i

        # ---- (2) the copies alone
        f32_pinned = tr()[1].cpu().pin_memory()
        u8_pinned = u8_host.pin_memory()
        f32_dev, u8_dev = torch.empty_like(f32_pinned, device=dev), torch.empty_like(u8_pinned, device=dev)
        h = _alternate({"fp32": lambda: f32_dev.copy_(f32_pinned, non_blocking=True), "u8": lambda: u8_dev.copy_(u8_pinned, non_blocking=True)},
                       args.rounds, args.reps, _device_ms)
        h["fp32"]["MB"], h["u8"]["MB"] = round(f32_pinned.numel() * 4 / 1e6, 1), round(u8_pinned.numel() / 1e6, 1)
        res["h2d"] = h
        del u8_dev
        if args.skip_step:
            continue

        # ---- (3) whole training steps, data included
        torch.manual_seed(0)
        if name.startswith("vit"):
            model = TV.ViTClassifier(TV.ViTConfig(size, 3, patch, "B", 1, 0.0), 1000).to(dev)
            optim = torch.optim.AdamW(model.parameters(), lr=1e-4)
            labels_dev = labels_host.to(dev)
            step = lambda x, y: TV.train_step(model, x, y, optim)
        else:
            model = TT.TiTok(TT.TiTokConfig(size, patch, 32, 2048, 12, "S")).to(dev)
            optim = torch.optim.AdamW(model.parameters(), lr=1e-4)
            labels_dev = None
            step = lambda x, y: TT.train_step(model, x, optim)
        labels_pinned = labels_host.pin_memory()

        def forever():
            while True:
                yield u8_pinned, (labels_host if labels_dev is not None else None)

        loader = data.DeviceLoader(forever(), dev, size, patch=patch, image=c["image"], mean=c["mean"], std=c["std"], train=c["train"], seed=1)

        def fp32_h2d():
            x = f32_pinned.to(dev, non_blocking=True)
            y = labels_pinned.to(dev, non_blocking=True) if labels_dev is not None else None
            step(x, y)

        def u8_loader():
            x, y = next(loader)
            step(x, y)

        res["step"] = _alternate({"fp32_h2d": fp32_h2d, "u8_loader": u8_loader, "resident": lambda: step(f32_dev, labels_dev)},
                                 args.rounds, args.reps, _host_ms)
        res["step"]["images_per_s"] = {r: round(BATCH / (res["step"][r]["median"] * 1e-3), 1) for r in ("fp32_h2d", "u8_loader", "resident")}
        del model, optim, loader, f32_dev
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
