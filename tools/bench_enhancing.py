"""The Enhancing ViT-VQGAN tokenizer's own kernels (vitamd.enhancing, csrc/enhancing.hip) against the same work
written with functions.linear and torch device ops on the same GEMMs, at the reference's configuration: 128 px, patch 16 (64 tokens an
image), 768 / 12 / 12 / 3072 stacks, 2 048 codes x 12, batch 32 (the reference's) and batch 256.  Device-event timings, warmed, the two
routes alternated in one process on the same seeded inputs, median of --rounds rounds with the spread (min .. max); prints one JSON line and
writes it to --out when given.  Before anything is timed each pair of routes must agree on its result.

  mlp     - (a) forward + backward of one FeedForward: functions.linear + torch.tanh + functions.linear against enhancing.tanh_mlp
  tail    - (b) ConvTranspose2d head + L1 pixel term, forward + backward, from the decoder's output rows: functions.linear on the transposed
            weight + permute copy + abs().mean() against enhancing.linear_recon_l1
  step    - (c) the whole train_step (forward, backward, torch.optim.AdamW) on either route (train_enhancing_vitvqgan.FUSED_ROUTE)
  kernels - (d) the two tanh kernels alone on the [rows, 3072] bf16 activations of one MLP, and vitamd_cast_f32_bf16 on as many elements
            beside them: launches recorded into a graph (the entry points only enqueue) and replayed, so the host's launch cost is outside
            the figure; bytes per second against the algorithmic bytes (4 B an element forward in place, 6 B backward, 6 B the cast).  The
            buffers of one launch are re-used by the next, so whatever of them the last-level cache holds is served from there - for all
            three kernels alike.  The two tanh figures are the price of NOT fusing the tanh into the fc1 GEMM's epilogue.
usage: bench_enhancing.py [--rounds N] [--reps N] [--batches 32,256] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_lm_loss import _ab  # noqa: E402  (the same timing)
from bench_tokenizer_loss import _agree, _verdict  # noqa: E402

IMG, PATCH, CODES, LATENT, DIM, HID = 128, 16, 2048, 12, 768, 3072


def kernel_rates(rows, rounds, calls=20):
    """-> {kernel: {us: median per launch, min_us, max_us, MB: algorithmic bytes, GB_per_s}} at n = rows * HID elements"""
    from vitamd import ops
    dev = torch.device("cuda")
    n = rows * HID
    pre = (torch.randn(n, device=dev) * 1.5).bfloat16()
    t = torch.tanh(pre.float()).bfloat16()
    dh, dpre = torch.randn(n, device=dev).bfloat16(), torch.empty(n, dtype=torch.bfloat16, device=dev)
    x32 = torch.randn(n, device=dev)
    kernels = {"tanh_fwd_in_place": (lambda: ops.tanh_bf16(pre, out=pre), 4 * n),
               "tanh_bwd": (lambda: ops.tanh_bwd_bf16(dh, t, out=dpre), 6 * n),
               "cast_f32_bf16": (lambda: ops._lib.check(ops._L().vitamd_cast_f32_bf16(x32.data_ptr(), dpre.data_ptr(), n, ops._stream()), "cast"), 6 * n)}
    out = {}
    for name, (fn, nbytes) in kernels.items():
        fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(calls):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            graph.replay()
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e) * 1e3 / calls)
        med = statistics.median(ts)
        out[name] = {"us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2), "MB": round(nbytes / 1e6, 1),
                     "GB_per_s": round(nbytes / med / 1e3, 1)}
        del graph
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=str, default="32,256")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 7:
        raise SystemExit("bench_enhancing: at least 7 rounds")
    import train_enhancing_vitvqgan as EV
    from vitamd import enhancing
    from vitamd.functions import WEIGHTS, linear
    dev = torch.device("cuda")
    G = IMG // PATCH
    props = torch.cuda.get_device_properties(0)
    out = {"box": {"host": socket.gethostname(), "device": props.name, "arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
                   "torch": torch.__version__, "hip": torch.version.hip},
           "rounds": args.rounds, "reps": args.reps,
           "config": {"image": IMG, "patch": PATCH, "codes": CODES, "latent_dim": LATENT, "dim": DIM, "mlp_dim": HID, "depth": 12, "heads": 12}}
    for B in [int(b) for b in args.batches.split(",")]:
        res = {}
        M = B * G * G
        torch.manual_seed(0)

        # ---- (a) one MLP
        ff = EV.FeedForward(DIM, HID).to(dev)
        fc1, fc2 = ff.net[0], ff.net[2]
        x = torch.randn(B, G * G, DIM, device=dev, requires_grad=True)
        gy = torch.randn(B, G * G, DIM, device=dev)

        def mlp(route):
            x.grad = None
            ff.zero_grad(set_to_none=True)
            WEIGHTS.clear()
            if route == "present":
                y = linear(torch.tanh(linear(x, fc1.weight, fc1.bias)), fc2.weight, fc2.bias)
            else:
                y = enhancing.tanh_mlp(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
            y.backward(gy)
            return y.detach()

        y_new, y_present = mlp("new"), mlp("present")
        rel = float((y_new - y_present).double().norm() / y_present.double().norm())
        if not rel <= 2.0 ** -7:                 # each route rounds the hidden activations to bf16 once
            raise SystemExit(f"bench_enhancing: the two MLP routes disagree: relative L2 {rel}")
        res["mlp"] = {"rows": M, "dim": DIM, "mlp_dim": HID, "output_rel_l2_new_vs_present": round(rel, 6)}
        del y_new, y_present
        res["mlp"].update(_ab({"present": lambda: mlp("present"), "new": lambda: mlp("new")}, args.rounds, args.reps))
        res["mlp"]["verdict"] = _verdict(res["mlp"])
        del ff, x, gy

        # ---- (b) the pixel tail from the decoder's output rows
        convt = torch.nn.ConvTranspose2d(DIM, 3, kernel_size=PATCH, stride=PATCH).to(dev)
        F_ = 3 * PATCH * PATCH
        h = torch.randn(B, G * G, DIM, device=dev, requires_grad=True)
        img = torch.rand(B, 3, IMG, IMG, device=dev)

        def tail(route):
            h.grad = None
            convt.zero_grad(set_to_none=True)
            WEIGHTS.clear()
            if route == "present":
                y = linear(h, convt.weight.reshape(DIM, F_).t(), convt.bias.repeat_interleave(PATCH * PATCH))
                loss = torch.nn.functional.l1_loss(enhancing.conv_shuffle_tokens(y, G, PATCH), img)
            else:
                loss = enhancing.linear_recon_l1(h, convt.weight, convt.bias, img, G, PATCH)
            loss.backward()
            return loss.detach()

        res["tail"] = {"rows": M, "D": DIM, "F": F_, "loss_check": _agree(tail("new"), tail("present"), "tail loss")}
        res["tail"].update(_ab({"present": lambda: tail("present"), "new": lambda: tail("new")}, args.rounds, args.reps))
        res["tail"]["verdict"] = _verdict(res["tail"])
        del convt, h, img

        # ---- (d) the streaming kernels alone
        res["kernels"] = kernel_rates(M, args.rounds)

        # ---- (c) the whole train_step
        if not args.skip_step:
            torch.manual_seed(0)
            model = EV.ViTVQGAN(EV.ViTVQGANConfig(IMG, PATCH, CODES, LATENT, "B")).to(dev)
            optim = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-5, weight_decay=1e-4)
            xs = torch.rand(B, 3, IMG, IMG, device=dev)

            def step(route):
                EV.FUSED_ROUTE = route == "new"
                try:
                    return EV.train_step(model, xs, optim)
                finally:
                    EV.FUSED_ROUTE = True

            rl, ql, _ = model.loss(xs)
            EV.FUSED_ROUTE = False
            try:
                with torch.no_grad():
                    recon, _, q0 = model(xs)
            finally:
                EV.FUSED_ROUTE = True
            res["step"] = {"batch": B, "loss_check": _agree(rl.detach() + ql.detach(), (recon - xs).abs().mean() + q0, "step loss", tol=2e-2)}
            del rl, ql, recon, q0
            res["step"].update(_ab({"present": lambda: step("present"), "new": lambda: step("new")}, args.rounds, max(1, args.reps // 2)))
            res["step"]["verdict"] = _verdict(res["step"])
            res["step"]["img_per_s"] = {k: round(B / (res["step"][k]["median_ms"] * 1e-3), 1) for k in ("present", "new")}
            del model, optim, xs
        out[f"batch_{B}"] = res
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
