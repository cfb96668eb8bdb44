"""One validation batch through vitamd.metrics.ClassifyMetrics.update (csrc/loss.hip vitamd_classify_metrics)
against the route the reference's validation loop takes (train_vit.py:114-128), on one MI355X, with the logits already on the device:

  [256, 1000] fp32      the ViT head's logits
  [32768, 1024] bf16    VideoGPT-B's logits as the fused head writes them

  update          ClassifyMetrics.update: the row walk + the single-workgroup sum, counters stay on the device
  torch_items     F.cross_entropy(logits.float(), y).item(), (argmax == y).float().mean().item(), the topk(5) hit rate .item():
                  the reference's three reads per batch
  torch_no_items  the same torch ops without the .item()s (what the stalls cost, apart from the kernels)

Every route is timed with the host clock around --reps batches ending in one synchronise (what a validation loop sees), and the two
that never stall also with device events (the kernels alone).  Warmed, the routes alternated round by round in one process, median
of --rounds rounds with the spread (min .. max); prints one JSON line and writes it to --out when given.  Before anything is timed the
routes must agree: equal counts, the mean loss within 1e-5 relative.
usage: bench_metrics.py [--rounds N] [--reps N] [--out FILE]"""
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

SHAPES = (("vit_head_fp32", 256, 1000, torch.float32), ("videogpt_b_bf16", 32768, 1024, torch.bfloat16))
TOPK = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_metrics: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: needs a GPU (no timing is taken without one)")
    from vitamd.metrics import ClassifyMetrics
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    out = {"rounds": args.rounds, "reps": args.reps, "topk": TOPK}
    for name, M, V, dtype in SHAPES:
        logits = (torch.randn(M, V, generator=gen) * 2.0).to(dtype).to(dev)
        y = torch.randint(0, V, (M,), generator=gen).to(dev)
        y[::3] = logits[::3].float().argmax(-1)                 # a third of the rows are hits, so the counts say something
        m = ClassifyMetrics(topk=TOPK, device=dev)
        sink = torch.zeros(3, device=dev)

        def update():
            m.update(logits, y)

        def torch_ops():
            x = logits.float()
            loss = F.cross_entropy(x, y)
            top1 = (x.argmax(-1) == y).float().mean()
            topk = (x.topk(TOPK, dim=-1).indices == y[:, None]).any(-1).float().mean()
            return loss, top1, topk

        def torch_items():
            loss, top1, topk = torch_ops()
            return loss.item(), top1.item(), topk.item()

        def torch_no_items():
            loss, top1, topk = torch_ops()
            sink[0] += loss; sink[1] += top1; sink[2] += topk     # the running sums a stall-free torch loop would keep

        r = m.reset().update(logits, y).result()
        loss, top1, topk = torch_items()
        if round(top1 * M) != round(r["top1"] * M) or round(topk * M) != round(r["topk"] * M) or abs(loss - r["loss"]) > 1e-5 * abs(loss):
            raise SystemExit(f"bench_metrics: the routes disagree at {name}: update {r}, torch {(loss, top1, topk)}")
        routes = {"update": update, "torch_items": torch_items, "torch_no_items": torch_no_items}
        res = {"shape": [M, V], "dtype": str(dtype).replace("torch.", ""), "logits_bytes": M * V * logits.element_size(),
               "result": {k: r[k] for k in ("loss", "top1", "topk", "count")},
               "host_clock": _alternate(routes, args.rounds, args.reps, _host_ms),
               "device_events": _alternate({k: routes[k] for k in ("update", "torch_no_items")}, args.rounds, args.reps, _device_ms)}
        h, d = res["host_clock"], res["device_events"]
        res["torch_items_over_update_host"] = round(h["torch_items"]["median"] / h["update"]["median"], 2)
        res["torch_no_items_over_update_device"] = round(d["torch_no_items"]["median"] / d["update"]["median"], 2)
        res["update_gb_per_s_device"] = round(res["logits_bytes"] / (d["update"]["median"] * 1e-3) / 1e9, 1)
        out[name] = res
        del logits, y, m
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
