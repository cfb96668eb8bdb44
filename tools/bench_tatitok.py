"""The training route of the 1D TiTok tokenizer (train_tatitok.TiTok.loss: the unit-code quantiser kernels and the fused pixel tail,
DESIGN.md section 15) against the present route (forward() on the blocks.py wrappers), at the reference's configuration: preset
`small`, 256 px, patch 16, 256 latent tokens, 16 384 codes x 12, batch 32 (the reference's) and batch 128.  Device-event timings, warmed,
the two routes alternated in one process on the same seeded inputs, median of --rounds rounds with the spread (min .. max); prints one JSON
line and writes it to --out when given.  Before anything is timed each pair of routes must agree on the loss and the ids.

  quantiser  - forward + backward alone: blocks.VectorQuantizer(use_l2_norm=True) against tokenizer.vq_quantize(unit_codes=True)
  tail       - pixel head + conv_out + mean squared error, forward + backward alone, from the ln_post rows: functions.linear + pixel-shuffle
               copy + Conv3x3Fn + mse_loss against tokenizer.linear_conv_recon_mse (the head GEMMs are the same work on both routes)
  step       - the whole train_step (forward, backward, clipped multi-tensor AdamW) on either route
  bytes      - what each tail route moves between the head GEMM's output and its gradient GEMMs' input, counted from shapes (expectations,
               not measurements)
usage: bench_tatitok.py [--rounds N] [--reps N] [--batches 32,128] [--skip-step] [--out FILE]"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_lm_loss import _ab  # noqa: E402  (the same timing)
from bench_tokenizer_loss import _agree, _ids_agree, _verdict  # noqa: E402

IMG, PATCH, LATENTS, CODES, DIM, PRESET, WIDTH = 256, 16, 256, 16384, 12, "small", 512


def tail_bytes(B):
    """HBM bytes of the pixel tail between the head GEMM's output and the gradient GEMMs' bf16 input, counted from shapes.  E = elements
    of the image tensor; halo re-reads (a 36/32 or 34/32 share of the tile) and the 84 floats a tile of weight-gradient partials are left out"""
    E = B * 3 * IMG * IMG
    bf, f32 = 2 * E, 4 * E
    present = {"linear output (write fp32 tokens)": f32, "pixel shuffle copy (read, write)": 2 * f32, "conv forward (read, write)": 2 * f32,
               "mse_loss (read 2, write 1)": 3 * f32, "sum": f32, "mse backward (read 2, write 1)": 3 * f32,
               "conv backward (read x, dy; write dx)": 3 * f32, "un-shuffle copy (read, write)": 2 * f32, "cast (read fp32, write bf16)": f32 + bf}
    new = {"head GEMM output (write bf16 tokens)": bf, "tail forward (read bf16 tokens, fp32 image)": bf + f32,
           "tail backward (read both, write bf16 gradient)": 2 * bf + f32}
    return {"present": sum(present.values()), "new": sum(new.values()), "present_parts": present, "new_parts": new}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=str, default="32,128")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("bench_tatitok: at least 3 rounds")
    import blocks as BK
    import train_tatitok as TA
    from vitamd import tokenizer
    from vitamd.block_functions import Conv3x3Fn
    from vitamd.functions import WEIGHTS, linear
    dev = torch.device("cuda")
    G = IMG // PATCH
    out = {"rounds": args.rounds, "reps": args.reps, "config": {"image": IMG, "patch": PATCH, "latent_tokens": LATENTS, "codes": CODES,
                                                                 "latent_dim": DIM, "preset": PRESET}}
    for B in [int(b) for b in args.batches.split(",")]:
        res = {}
        torch.manual_seed(0)

        # ---- (a) the quantiser alone
        vq = BK.VectorQuantizer(codebook_size=CODES, token_size=DIM, commitment_cost=0.25, use_l2_norm=True).to(dev)
        z = torch.randn(B, DIM, 1, LATENTS, device=dev, requires_grad=True)
        gz = torch.randn(B, DIM, 1, LATENTS, device=dev)

        def quant(route):
            z.grad = vq.embedding.weight.grad = None
            if route == "present":
                zq, info = vq(z)
                ids, loss = info["min_encoding_indices"], info["quantizer_loss"]
            else:
                q, ids, loss = tokenizer.vq_quantize(z.permute(0, 2, 3, 1), vq.embedding.weight, unit_codes=True)
                zq = q.permute(0, 3, 1, 2)
            ((zq * gz).sum() + loss).backward()
            return ids, loss.detach()

        (i1, l1), (i0, l0) = quant("new"), quant("present")
        res["quantiser"] = {"rows": B * LATENTS, "loss_check": _agree(l1, l0, "quantiser loss"), "ids_equal": _ids_agree(i1, i0, "quantiser")}
        res["quantiser"].update(_ab({"present": lambda: quant("present"), "new": lambda: quant("new")}, args.rounds, args.reps))
        res["quantiser"]["verdict"] = _verdict(res["quantiser"])
        del vq, z, gz

        # ---- (b) the pixel tail from the ln_post rows
        ffn = torch.nn.Conv2d(WIDTH, 3 * PATCH * PATCH, 1).to(dev)
        conv = torch.nn.Conv2d(3, 3, 3, padding=1).to(dev)
        h = torch.randn(B, G * G, WIDTH, device=dev, requires_grad=True)
        img = torch.rand(B, 3, IMG, IMG, device=dev)

        def tail(route):
            h.grad = None
            ffn.zero_grad(set_to_none=True)
            conv.zero_grad(set_to_none=True)
            WEIGHTS.clear()
            if route == "present":
                y = linear(h, ffn.weight.view(ffn.weight.shape[0], -1), ffn.bias)
                loss = F.mse_loss(Conv3x3Fn.apply(tokenizer.pixel_shuffle_tokens(y, G, PATCH), conv.weight, conv.bias), img)
            else:
                loss = tokenizer.linear_conv_recon_mse(h, ffn.weight, ffn.bias, conv.weight, conv.bias, img, G, PATCH)
            loss.backward()
            return loss.detach()

        res["tail"] = {"rows": B * G * G, "D": WIDTH, "F": 3 * PATCH * PATCH, "loss_check": _agree(tail("new"), tail("present"), "tail loss")}
        res["tail"].update(_ab({"present": lambda: tail("present"), "new": lambda: tail("new")}, args.rounds, args.reps))
        res["tail"]["bytes"] = tail_bytes(B)
        res["tail"]["verdict"] = _verdict(res["tail"])
        del ffn, conv, h, img

        # ---- (c) the whole train_step
        if not args.skip_step:
            torch.manual_seed(0)
            model = TA.TiTok(TA.TiTokConfig(IMG, PATCH, LATENTS, CODES, DIM, PRESET)).to(dev)
            optim = TA.make_optim(model, NS(lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0))
            x = torch.rand(B, 3, IMG, IMG, device=dev)
            with torch.no_grad():
                ids0 = model(x)[1]["min_encoding_indices"]
            rl, ql, ids1 = model.loss(x)
            with torch.no_grad():
                recon, info = model(x)
            res["step"] = {"batch": B, "loss_check": _agree(rl.detach() + ql.detach(), F.mse_loss(recon, x) + info["quantizer_loss"], "step loss"),
                           "ids_equal": _ids_agree(ids1, ids0, "step")}
            del rl, ql, recon, info

            def step(route):
                TA.FUSED_ROUTE = route == "new"
                try:
                    return TA.train_step(model, x, optim)
                finally:
                    TA.FUSED_ROUTE = True

            res["step"].update(_ab({"present": lambda: step("present"), "new": lambda: step("new")}, args.rounds, max(1, args.reps // 2)))
            res["step"]["verdict"] = _verdict(res["step"])
            res["step"]["img_per_s"] = {k: round(B / (res["step"][k]["median_ms"] * 1e-3), 1) for k in ("present", "new")}
            del model, optim, x
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
