"""One training iteration by three routes, alternated in one process:

  (a) eager       train_step: forward, loss, backward, multi-tensor AdamW (host-built table), the LambdaLR scheduler
  (b) graph+eager vitamd.graph.GraphedStep (forward + loss + backward replayed), then the same eager optimiser and scheduler
  (c) graph       vitamd.graph.GraphedTrainStep: the whole iteration, AdamW(capturable=True, schedule=...) included, as one graph launch

Routes (a) and (b) run code paths that exist without the capturable optimiser; they are the baseline of every claim about (c).  Each
route has its own copy of the model (the same initial weights) and its own optimiser.  A round times `iters` iterations of every route,
one route after the other; the rounds alternate the routes, so drift of the box hits all three.  Per route: ms per iteration (host clock
around the loop, ending in a device synchronise) and host ms per iteration (the same clock stopped when the last call has returned,
before the synchronise: what the host spends enqueueing).  Reported: the median over the rounds and the round-to-round spread (max - min).

    python tools/bench_graph_train.py [--shapes s32 b224 gpt] [--rounds 7] [--max_grad_norm 1.0] [--out bench_graph_train.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))

SCHEDULE = (10, 10 ** 6, 1e-5)                   # warm-up, then a cosine far longer than any run here: the rate moves on every step
LR, WD = 1e-4, 1e-2


def vit_shape(image, size, batch, classes):
    import train_vit as TV
    from vitamd import lm
    cfg = TV.ViTConfig(image, 3, 16, size, 1, 0.0)
    g = torch.Generator().manual_seed(0)
    inputs = (torch.randn(batch, 3, image, image, generator=g).cuda(), torch.randint(0, classes, (batch,), generator=g).cuda())

    def make():
        torch.manual_seed(0)
        model = TV.ViTClassifier(cfg, num_classes=classes).cuda()
        return model, model, lm.cross_entropy           # (what owns the parameters, module for GraphedStep, its loss_fn)

    return make, inputs, (lambda model: (lambda x, y: lm.cross_entropy(model(x), y)))


class _LossModule(torch.nn.Module):
    """VideoGPT behind GraphedStep's (model, loss_fn, x, y) form: forward is model.loss, the loss_fn passes it through"""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, tokens):
        return self.model.loss(tokens)


def gpt_shape(batch):
    import train_videogpt as V
    cfg = V.VideoGPTConfig(frame_size=64, codebook_size=1024, transformer="B", max_frames=16, dropout=0.0)
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(0, cfg.codebook_size, (batch, cfg.max_frames, cfg.frame_size), generator=g).cuda()
    inputs = (tokens, torch.zeros((), device="cuda"))   # GraphedStep wants a y; nothing reads it

    def make():
        torch.manual_seed(0)
        model = V.VideoGPT(cfg).cuda()
        return model, _LossModule(model), (lambda out, y: out)

    return make, inputs, (lambda model: (lambda tok, y: model.loss(tok)))


SHAPES = {"s32": ("ViT-S/16 32x32 batch 64 (BASELINE configs[0])", lambda: vit_shape(32, "S", 64, 10), 200),
          "b224": ("ViT-B/16 224x224 batch 256", lambda: vit_shape(224, "B", 256, 1000), 10),
          "gpt": ("VideoGPT-B batch 32 x 1024 tokens", lambda: gpt_shape(32), 10)}


def build_routes(make, inputs, step_fn_of, max_grad_norm):
    import utils as U
    from vitamd.graph import GraphedStep, GraphedTrainStep
    from vitamd.optim import AdamW
    routes = {}

    model, module, loss_fn = make()
    opt = AdamW(model.parameters(), lr=LR, weight_decay=WD, multi_tensor=True, max_grad_norm=max_grad_norm)
    sched = U.get_lr_scheduler(opt, *SCHEDULE)

    def eager(model=model, module=module, loss_fn=loss_fn, opt=opt, sched=sched):
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(module(inputs[0]), inputs[1])
        loss.backward()
        opt.step()
        sched.step()
        return loss
    routes["a eager"] = eager

    model, module, loss_fn = make()
    opt = AdamW(model.parameters(), lr=LR, weight_decay=WD, multi_tensor=True, max_grad_norm=max_grad_norm)
    sched = U.get_lr_scheduler(opt, *SCHEDULE)
    fb = GraphedStep(module, loss_fn, inputs[0], inputs[1])

    def graph_eager(fb=fb, opt=opt, sched=sched):
        loss = fb(inputs[0], inputs[1])
        opt.step()
        sched.step()
        return loss
    routes["b graph + eager optimiser"] = graph_eager

    model, module, loss_fn = make()
    opt = AdamW(model.parameters(), lr=LR, weight_decay=WD, max_grad_norm=max_grad_norm, capturable=True, schedule=SCHEDULE)
    whole = GraphedTrainStep(model, step_fn_of(model), inputs, opt)
    routes["c one graph"] = lambda whole=whole: whole(*inputs)
    return routes


def time_route(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        loss = fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / iters * 1e3, (t1 - t0) / iters * 1e3, float(loss.detach())


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=None, help="iterations per route and round (default: per shape)")
    p.add_argument("--max_grad_norm", type=float, default=None)
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph_train: no GPU (there is no CPU path and no timing without one)")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds, "max_grad_norm": args.max_grad_norm,
              "schedule": SCHEDULE, "shapes": {}}
    for key in args.shapes:
        title, shape, iters = SHAPES[key]
        iters = args.iters or iters
        make, inputs, step_fn_of = shape()
        routes = build_routes(make, inputs, step_fn_of, args.max_grad_norm)
        for fn in routes.values():                      # warm every route at this shape before any timed window
            time_route(fn, max(3, iters // 10))
        rows = {name: {"ms": [], "host_ms": []} for name in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                ms, host, loss = time_route(fn, iters)
                rows[name]["ms"].append(ms)
                rows[name]["host_ms"].append(host)
                rows[name]["last_loss"] = loss
        print(f"{title}: {args.rounds} rounds x {iters} iterations")
        out = {}
        for name, r in rows.items():
            out[name] = {"ms_median": statistics.median(r["ms"]), "ms_spread": max(r["ms"]) - min(r["ms"]),
                         "host_ms_median": statistics.median(r["host_ms"]), "host_ms_spread": max(r["host_ms"]) - min(r["host_ms"]),
                         "ms": r["ms"], "host_ms": r["host_ms"], "last_loss": r["last_loss"]}
            print(f"  {name:28s} {out[name]['ms_median']:9.3f} ms/iteration (spread {out[name]['ms_spread']:.3f})   "
                  f"host {out[name]['host_ms_median']:8.3f} ms (spread {out[name]['host_ms_spread']:.3f})")
        result["shapes"][key] = {"title": title, "iters": iters, "routes": out}
        del routes, rows
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
