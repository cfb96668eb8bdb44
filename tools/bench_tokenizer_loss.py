"""The training route of the two image tokenizers (vitamd/tokenizer.py, csrc/tokenizer.hip) against the present route, at the shapes of
bench.py's `also` block (TiTok-S at batch 256: 8 192 latents x 2 048 codes x 12; ViT-VQGAN-B at batch 128: 32 768 latents; 256 px,
patch 16).  Device-event timings, warmed, the two routes alternated in one process, median of --rounds rounds with the spread
(min .. max); prints one JSON line and writes it to --out when given.  Before anything is timed each pair of routes must agree on the
loss and the ids.

  quantiser  - forward + backward alone: train_titok.Quantizer.forward against tokenizer.vq_quantize, at both latent counts
  head       - pixel head + reconstruction loss, forward + backward alone: HipConv1x1 + pixel_shuffle_tokens + mse_loss against
               tokenizer.linear_recon_mse (TiTok-S: 65 536 rows, D = 384, F = 768)
  step       - whole forward + backward of TiTok-S (batch 256) and ViT-VQGAN-B (batch 128): model(x) + mse_loss against model.loss(x)
  launches   - what the host issues per call on each route: C-ABI calls of the library plus torch device ops (views and allocations
               left out), counted, not timed
usage: bench_tokenizer_loss.py [--rounds N] [--reps N] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_lm_loss import _ab, _count  # noqa: E402  (the same timing and counting)

IMG, PATCH, CODES, DIM = 256, 16, 2048, 12


def _agree(a, b, what, tol=2e-3):
    a, b = float(a), float(b)
    if not abs(a - b) <= tol * max(1.0, abs(b)):
        raise SystemExit(f"bench_tokenizer_loss: the two routes disagree on the {what}: {a} vs {b}")
    return {"present": round(b, 6), "new": round(a, 6)}


def _ids_agree(a, b, what):
    frac = float((a == b).float().mean())
    if frac < 0.999:
        raise SystemExit(f"bench_tokenizer_loss: the two routes disagree on the {what} ids: {frac:.5f} equal")
    return round(frac, 6)


def _verdict(r):
    """whether the two medians differ by more than the rounds scatter: the ranges [min, max] do not overlap"""
    p, n = r["present"], r["new"]
    apart = n["max_ms"] < p["min_ms"] or p["max_ms"] < n["min_ms"]
    return {"new_over_present": round(n["median_ms"] / p["median_ms"], 4), "outside_spread": apart,
            "faster": "new" if n["median_ms"] < p["median_ms"] else "present"}


def head_bytes(B):
    """HBM bytes between the head GEMM's bf16 output and its two gradient GEMMs' bf16 input, counted from shapes"""
    E = B * 3 * IMG * IMG
    bf, f32 = 2 * E, 4 * E
    present = {"upcast (read bf16, write fp32)": bf + f32, "pixel shuffle copy": 2 * f32, "mse_loss (read 2, write 1)": 3 * f32,
               "sum": f32, "mse backward (read 2, write 1)": 3 * f32, "pad: zero fill": f32, "pad: permuted copy (read, write)": 2 * f32,
               "cast (read fp32, write bf16)": f32 + bf}
    new = {"loss forward (read bf16 tokens, fp32 image)": bf + f32, "loss backward (read both, write bf16 in place)": 2 * bf + f32}
    return {"present": sum(present.values()), "new": sum(new.values()), "present_parts": present, "new_parts": new}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_tokenizer_loss: at least 5 rounds")
    import train_titok as TT
    import train_vit_vqgan as TQ
    from vitamd import tokenizer
    from vitamd.functions import WEIGHTS
    dev = torch.device("cuda")
    torch.manual_seed(0)
    out = {"rounds": args.rounds, "reps": args.reps}

    # ---- (a) the quantiser alone
    for key, M in (("quantiser_titok_s_b256", 256 * 32), ("quantiser_vitvqgan_b_b128", 128 * 256)):
        quant = TT.Quantizer(TT.TiTokConfig(IMG, PATCH, 32, CODES, DIM, "S")).to(dev)
        x = torch.randn(M // 32, 32, DIM, device=dev, requires_grad=True)
        gq = torch.randn(M // 32, 32, DIM, device=dev)

        def run(route):
            x.grad = quant.codebook.weight.grad = None
            q, ids, loss = quant(x) if route == "present" else tokenizer.vq_quantize(x, quant.codebook.weight)
            ((q * gq).sum() + loss).backward()
            return ids, loss.detach()

        (i1, l1), (i0, l0) = run("new"), run("present")
        out[key] = {"rows": M, "loss_check": _agree(l1, l0, f"{key} loss"), "ids_equal": _ids_agree(i1, i0, key)}
        out[key].update(_ab({"present": lambda: run("present"), "new": lambda: run("new")}, args.rounds, args.reps))
        out[key]["launches"] = {"present": _count(lambda: run("present")), "new": _count(lambda: run("new"))}
        out[key]["verdict"] = _verdict(out[key])
        del quant, x, gq

    # ---- (b) head + reconstruction loss (TiTok-S, batch 256)
    B, G, D = 256, IMG // PATCH, 384
    conv = TT.HipConv1x1(D, 3 * PATCH * PATCH, kernel_size=1).to(dev)
    h = torch.randn(B, G * G, D, device=dev, requires_grad=True)
    img = torch.rand(B, 3, IMG, IMG, device=dev)

    def head(route):
        h.grad = None
        conv.zero_grad(set_to_none=True)
        WEIGHTS.clear()
        if route == "present":
            loss = F.mse_loss(TT.pixel_shuffle_tokens(conv(h), G, PATCH), img)
        else:
            loss = tokenizer.linear_recon_mse(h, conv.weight, conv.bias, img, G, PATCH)
        loss.backward()
        return loss.detach()

    out["head"] = {"rows": B * G * G, "D": D, "F": 3 * PATCH * PATCH, "loss_check": _agree(head("new"), head("present"), "head loss")}
    out["head"].update(_ab({"present": lambda: head("present"), "new": lambda: head("new")}, args.rounds, args.reps))
    out["head"]["launches"] = {"present": _count(lambda: head("present")), "new": _count(lambda: head("new"))}
    out["head"]["bytes"] = head_bytes(B)
    out["head"]["verdict"] = _verdict(out["head"])
    del conv, h, img

    # ---- (c) whole forward + backward
    if not args.skip_step:
        for key, make, bs in (("step_titok_s_b256", lambda: TT.TiTok(TT.TiTokConfig(IMG, PATCH, 32, CODES, DIM, "S")), 256),
                              ("step_vitvqgan_b_b128", lambda: TQ.ViTVQGAN(TQ.ViTVQGANConfig(IMG, PATCH, CODES, DIM, "B")), 128)):
            torch.manual_seed(0)
            model = make().to(dev)
            x = torch.rand(bs, 3, IMG, IMG, device=dev)

            def step(route):
                model.zero_grad(set_to_none=True)
                WEIGHTS.clear()
                if route == "present":
                    recon, ids, ql = model(x)
                    loss = F.mse_loss(recon, x) + ql
                else:
                    rl, ql, ids = model.loss(x)
                    loss = rl + ql
                loss.backward()
                return ids, loss.detach()

            (i1, l1), (i0, l0) = step("new"), step("present")
            out[key] = {"batch": bs, "loss_check": _agree(l1, l0, f"{key} loss"), "ids_equal": _ids_agree(i1, i0, key)}
            out[key].update(_ab({"present": lambda: step("present"), "new": lambda: step("new")}, args.rounds, max(1, args.reps // 2)))
            out[key]["launches"] = {"present": _count(lambda: step("present")), "new": _count(lambda: step("new"))}
            out[key]["verdict"] = _verdict(out[key])
            out[key]["img_per_s"] = {k: round(bs / (out[key][k]["median_ms"] * 1e-3), 1) for k in ("present", "new")}
            del model, x
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
