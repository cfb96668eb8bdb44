"""The optimiser step after backward(): the per-tensor AdamW (one launch per parameter tensor) against the multi-tensor path
(vitamd/optim.py, csrc/optim.hip), on the parameter sets of ViT-B/16 (224 px, 1000 classes) and VideoGPT-B
(train_videogpt.py:73-79) with random gradients.  Two comparisons, the routes of each alternated round by round in one process:

  a  per_tensor   vitamd.optim.AdamW(...)                                 against   multi     AdamW(..., multi_tensor=True)
  b  torch_clip   torch.nn.utils.clip_grad_norm_(1.0) + the per-tensor    against   clipped   AdamW(..., max_grad_norm=1.0)

and three times per route, each the median over --rounds rounds with the spread (min .. max):

  device_ms   the step's kernels with the queue kept full: a plug of large GEMMs is enqueued first, the host issues the step while the
              plug runs, and device events bracket the step alone - what the step costs a GPU that never waits for the host
  stream_ms   --reps steps issued back to back from an empty stream, per step: max(host, device), what a training loop sees when the
              optimiser step is all there is
  host_ms     wall time of step() alone, the stream drained before and left to drain after (the enqueue cost)

Achieved GB/s = parameters x 28 B (a: p, g, m, v read, p, m, v written) or x 32 B (b: one more read of g for the norm) over device_ms.
Before anything is timed the multi-tensor step must leave the bits of the per-tensor step.  Prints one JSON line.
usage: bench_optim.py [--rounds N] [--reps N] [--models vit,videogpt]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))


def param_shapes(name):
    if name == "vit":
        import train_vit as TV
        model = TV.ViTClassifier(TV.ViTConfig(224, 3, 16, "B", 1, 0.0), 1000)
    else:
        import train_videogpt as V
        model = V.VideoGPT(V.VideoGPTConfig(64, 1024, "B", 16, 0.0))
    return [tuple(p.shape) for p in model.parameters()]


def _stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


class Plug:
    """Enough GEMM work to keep the GPU busy while the host issues one optimiser step."""

    def __init__(self, dev, n=8192, count=12):
        self.a = torch.randn(n, n, device=dev, dtype=torch.bfloat16)
        self.b = torch.randn(n, n, device=dev, dtype=torch.bfloat16)
        self.c = torch.empty(n, n, device=dev, dtype=torch.bfloat16)
        self.count = count

    def __call__(self):
        for _ in range(self.count):
            torch.mm(self.a, self.b, out=self.c)


def measure(routes, rounds, reps, plug):
    for fn in routes.values():
        fn(); fn()
    torch.cuda.synchronize()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    dev_t, str_t, host_t, plug_t = ({k: [] for k in routes} for _ in range(4))
    for _ in range(rounds):
        for k, fn in routes.items():
            # device: plug, then the step, all enqueued before the plug has run
            torch.cuda.synchronize()
            p0, s, e = ev(), ev(), ev()
            p0.record(); plug(); s.record()
            t0 = time.perf_counter()
            fn()
            enqueue = time.perf_counter() - t0
            e.record(); e.synchronize()
            plug_ms = p0.elapsed_time(s)
            if enqueue * 1e3 < 0.8 * plug_ms:                   # else the host was not ahead and the figure is not the device's
                dev_t[k].append(s.elapsed_time(e))
            plug_t[k].append(plug_ms)
            # stream: reps steps back to back from an empty stream
            torch.cuda.synchronize()
            s, e = ev(), ev()
            s.record()
            for _ in range(reps):
                fn()
            e.record(); e.synchronize()
            str_t[k].append(s.elapsed_time(e) / reps)
            # host: step() alone
            h = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                h.append((time.perf_counter() - t0) * 1e3)
            host_t[k].append(statistics.median(h))
    out = {}
    for k in routes:
        out[k] = {"device": _stats(dev_t[k]) if len(dev_t[k]) >= max(3, rounds // 2) else "host never ahead of the plug: not measured",
                  "device_samples": len(dev_t[k]), "stream": _stats(str_t[k]), "host": _stats(host_t[k]),
                  "plug_ms": round(statistics.median(plug_t[k]), 3)}
    return out


def run_model(name, rounds, reps, plug):
    from vitamd.functions import WEIGHTS  # noqa: F401  (the optimiser clears it)
    from vitamd.optim import AdamW
    dev = torch.device("cuda")
    shapes = param_shapes(name)
    gen = torch.Generator(device="cpu").manual_seed(0)
    params = [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.02).to(dev)) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device=dev)
    n = sum(p.numel() for p in params)
    kw = dict(lr=1e-4, weight_decay=1e-2)

    # the same bits first: one step of each path on copies
    def copies():
        out = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for q, p in zip(out, params):
            q.grad = p.grad
        return out
    pa, pb = copies(), copies()
    oa, ob = AdamW(pa, **kw), AdamW(pb, multi_tensor=True, **kw)
    for _ in range(2):
        oa.step(); ob.step()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]) for a, b in zip(pa, pb))
    if not same:
        raise SystemExit(f"bench_optim: {name}: the multi-tensor step does not leave the bits of the per-tensor step")
    del pa, pb, oa, ob

    per_tensor, multi = AdamW(params, **kw), AdamW(params, multi_tensor=True, **kw)
    base_b, clipped = AdamW(params, **kw), AdamW(params, max_grad_norm=1.0, **kw)

    def torch_clip():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        base_b.step()

    res = {"tensors": len(params), "parameters": n, "same_bits": same}
    res["a"] = measure({"per_tensor": per_tensor.step, "multi": multi.step}, rounds, reps, plug)
    res["b"] = measure({"torch_clip": torch_clip, "clipped": clipped.step}, rounds, reps, plug)
    res["clip_coef"] = float(clipped.clip_coef)
    for cmp_, bytes_per in (("a", 28), ("b", 32)):
        for k, r in res[cmp_].items():
            if isinstance(r["device"], dict):
                r["GBps_device"] = round(n * bytes_per / (r["device"]["median_ms"] * 1e-3) / 1e9, 1)
            r["GBps_stream"] = round(n * bytes_per / (r["stream"]["median_ms"] * 1e-3) / 1e9, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--models", type=str, default="vit,videogpt")
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_optim: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs a GPU (no timing is taken on a CPU)")
    plug = Plug(torch.device("cuda"))
    out = {"rounds": args.rounds, "reps": args.reps}
    for name in args.models.split(","):
        out[name] = run_model(name, args.rounds, args.reps, plug)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
