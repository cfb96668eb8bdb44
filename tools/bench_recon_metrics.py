"""One validation batch of a tokenizer through vitamd.metrics.ReconMetrics.update + CodebookMetrics.update (csrc/recon_metrics.hip;
DESIGN.md section 25) against the same numbers written with torch ops, on one MI355X, with both images and the ids on the device:

  titok_s        256 x 3 x 256 x 256 bf16 reconstruction, fp32 target, 256 x 32 ids, 2 048 codes
  reference      32 x 3 x 128 x 128 fp32 reconstruction (the reference loops' default batch), 32 x 64 ids, 2 048 codes

  update          ReconMetrics.update + CodebookMetrics.update: three launches, the counters stay on the device
  update_read     the same, followed by both result() calls (the two host reads of one evaluation)
  torch_no_items  per-image mse_loss / l1_loss / PSNR, SSIM by grouped conv2d in fp32 (the 11 x 11 window on x, y, x^2, y^2, xy) and the
                  reference loops' usage[ids] = 1, summed into device tensors
  torch_items     the same, with the .item() per number the reference loops make

Every route is timed with the host clock around --reps batches ending in one synchronise (what a validation loop sees), and the two
that never stall also with device events (the kernels alone).  Warmed, the routes alternated round by round in one process, median
of --rounds rounds with the spread (min .. max); prints one JSON line and writes it to --out when given.  Before anything is timed the
routes must agree (fp32 torch against the kernels: 1e-4 relative, the usage exactly).  The TB/s figure is the algorithmic traffic -
both images read once - over the device time of `update`.
usage: bench_recon_metrics.py [--rounds N] [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_input import _alternate, _device_ms, _host_ms  # noqa: E402

SHAPES = (("titok_s", 256, 256, torch.bfloat16, 32, 2048), ("reference", 32, 128, torch.float32, 64, 2048))


def _window(C, dev):
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-k * k / 4.5)
    g = (g / g.sum()).float()
    return torch.outer(g, g).expand(C, 1, 11, 11).contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_recon_metrics: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_recon_metrics: needs a GPU (no timing is taken without one)")
    from vitamd.metrics import CodebookMetrics, ReconMetrics
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    out = {"rounds": args.rounds, "reps": args.reps}
    for name, B, size, dtype, n_ids, K in SHAPES:
        target = torch.rand(B, 3, size, size, generator=gen).to(dev)
        recon = (target + 0.05 * torch.randn(B, 3, size, size, generator=gen).to(dev)).to(dtype)
        ids = torch.randint(0, K // 2, (B, n_ids), generator=gen).to(dev)
        win = _window(3, dev)
        m, c = ReconMetrics(device=dev), CodebookMetrics(K, device=dev)
        sink, usage = torch.zeros(4, device=dev), torch.zeros(K, device=dev)

        def update():
            m.update(recon, target)
            c.update(ids)

        def update_read():
            update()
            return m.result(), c.result()

        def torch_ops():
            x, y = recon.float(), target
            mse = F.mse_loss(x, y, reduction="none").mean(dim=(1, 2, 3))
            mae = F.l1_loss(x, y, reduction="none").mean(dim=(1, 2, 3))
            psnr = 10.0 * torch.log10(1.0 / mse)
            blur = lambda z: F.conv2d(z, win, groups=3)
            mx, my = blur(x), blur(y)
            vx, vy, vxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
            ssim = (((2 * mx * my + 1e-4) * (2 * vxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))).mean(dim=(1, 2, 3))
            usage[ids] = 1
            return mse.mean(), mae.mean(), psnr.mean(), ssim.mean(), usage.sum() / K

        def torch_items():
            return [v.item() for v in torch_ops()]

        def torch_no_items():
            vals = torch_ops()
            for k in range(4):
                sink[k] += vals[k]

        m.reset(), c.reset()
        r, u = update_read()
        t = torch_items()
        for k, key in enumerate(("mse", "mae", "psnr", "ssim")):
            if abs(t[k] - r[key]) > 1e-4 * max(1.0, abs(r[key])):
                raise SystemExit(f"bench_recon_metrics: the routes disagree at {name} {key}: update {r[key]}, torch {t[k]}")
        if t[4] != u["usage"]:
            raise SystemExit(f"bench_recon_metrics: the routes disagree at {name} usage: update {u['usage']}, torch {t[4]}")
        routes = {"update": update, "update_read": update_read, "torch_no_items": torch_no_items, "torch_items": torch_items}
        image_bytes = recon.numel() * recon.element_size() + target.numel() * 4
        res = {"shape": [B, 3, size, size], "recon_dtype": str(dtype).replace("torch.", ""), "ids": [B, n_ids], "codes": K,
               "image_bytes": image_bytes, "result": {**{k: r[k] for k in ("mse", "mae", "psnr", "ssim", "count")}, "usage": u["usage"]},
               "host_clock": _alternate(routes, args.rounds, args.reps, _host_ms),
               "device_events": _alternate({k: routes[k] for k in ("update", "torch_no_items")}, args.rounds, args.reps, _device_ms)}
        h, d = res["host_clock"], res["device_events"]
        res["torch_items_over_update_read_host"] = round(h["torch_items"]["median"] / h["update_read"]["median"], 2)
        res["torch_no_items_over_update_device"] = round(d["torch_no_items"]["median"] / d["update"]["median"], 2)
        res["update_tb_per_s_device"] = round(image_bytes / (d["update"]["median"] * 1e-3) / 1e12, 3)
        out[name] = res
        del target, recon, ids, m, c
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
