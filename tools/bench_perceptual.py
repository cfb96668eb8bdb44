"""The perceptual loss (vitamd/perceptual.py, csrc/perceptual.hip) against the route a user has without it: the same ConvNeXt-S written with
torch operators (F.interpolate, F.conv2d, F.layer_norm, F.gelu, F.linear) under bf16 autocast, on the same GPU, in the same process, the
same random weights.  Forward + backward of PerceptualLoss at batch --batch (256) from 256 x 256 images.  Device-event timings, warmed, the
two routes alternated round by round, median of --rounds rounds with the spread (min .. max); prints one JSON line and writes it to --out.
Before anything is timed the two routes must agree on the loss.

  loss      - forward (both images) + backward (to the reconstruction) of the whole loss on both routes, and the peak memory of one call
  families  - device time of each kernel family alone at the network's shapes, forward + input gradient, summed over the network with the
              counts of one loss call (forward on 2B images, backward on B): depthwise conv, LayerNorm, the MLP GEMMs, resize; with the
              bytes / FLOPs each needs from its shapes and the time those take at --hbm-tbs / --bf16-tflops (the family's floor)
  step      - train_step's forward + backward of TiTok-S (batch 256) and ViT-VQGAN-B (batch 128) with perceptual_weight = 1 on both routes
usage: bench_perceptual.py [--batch N] [--rounds N] [--reps N] [--skip-step] [--skip-families] [--out FILE]"""
import argparse
import json
import os
import sys
import warnings

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-is-all-you-need_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_lm_loss import _ab  # noqa: E402  (the same timing)

BF16, F32 = torch.bfloat16, torch.float32
IMG, EPS = 256, 1e-6


def torch_logits(sd, img, depths, size, mean, std):
    """torchvision's convnext forward written out with torch operators (NCHW, two permutes per block), on the module's state dict"""
    g = lambda k: sd["convnext." + k]
    x = (F.interpolate(img, size=size, mode="bilinear", align_corners=False, antialias=True) - mean) / std
    ln2d = lambda t, k: F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), g(k + ".weight"), g(k + ".bias"), EPS).permute(0, 3, 1, 2)
    x = ln2d(F.conv2d(x, g("features.0.0.weight"), g("features.0.0.bias"), stride=4), "features.0.1")
    for s in range(4):
        f = 2 * s + 1
        for i in range(depths[s]):
            p = f"features.{f}.{i}."
            y = F.conv2d(x, g(p + "block.0.weight"), g(p + "block.0.bias"), padding=3, groups=x.shape[1]).permute(0, 2, 3, 1)
            y = F.layer_norm(y, (y.shape[-1],), g(p + "block.2.weight"), g(p + "block.2.bias"), EPS)
            y = F.linear(F.gelu(F.linear(y, g(p + "block.3.weight"), g(p + "block.3.bias"))), g(p + "block.5.weight"), g(p + "block.5.bias"))
            x = x + g(p + "layer_scale") * y.permute(0, 3, 1, 2)
        if s < 3:
            x = F.conv2d(ln2d(x, f"features.{f + 1}.0"), g(f"features.{f + 1}.1.weight"), g(f"features.{f + 1}.1.bias"), stride=2)
    x = F.layer_norm(x.mean(dim=(2, 3)), (x.shape[1],), g("classifier.0.weight"), g("classifier.0.bias"), EPS)
    return F.linear(x, g("classifier.2.weight"), g("classifier.2.bias"))


class TorchRoute(torch.nn.Module):
    """the reference's PerceptualLoss.forward on torch operators under bf16 autocast"""

    def __init__(self, module):
        super().__init__()
        self.m = module

    def forward(self, inp, tgt):
        m = self.m
        sd = dict(m.named_parameters())
        with torch.autocast("cuda", dtype=BF16):
            li = torch_logits(sd, inp, m.depths, m.size, m.imagenet_mean, m.imagenet_std)
            with torch.no_grad():
                lt = torch_logits(sd, tgt, m.depths, m.size, m.imagenet_mean, m.imagenet_std)
        return F.mse_loss(li.float(), lt.float())


def _verdict(r):
    t, h = r["torch"], r["hip"]
    return {"hip_over_torch": round(h["median_ms"] / t["median_ms"], 4), "outside_spread": h["max_ms"] < t["min_ms"] or t["max_ms"] < h["min_ms"],
            "faster": "hip" if h["median_ms"] < t["median_ms"] else "torch"}


def families(module, B, rounds, reps, hbm_tbs, tflops):
    """each kernel family alone at every stage's shape, both routes; the network total weighs forward x 2B images and backward x B"""
    from vitamd import ops, perceptual as P
    dev = module.imagenet_mean.device
    prep = module.prepared()
    out, size = {}, module.size
    total = {f: {"torch": 0.0, "hip": 0.0, "floor_ms": 0.0} for f in ("dwconv", "layernorm", "mlp_gemms")}
    for s, (depth, C) in enumerate(zip(module.depths, module.dims)):
        H = size // 4 >> s
        M = B * H * H
        p = prep["stages"][s][0]
        blk = module.convnext.features[2 * s + 1][0].block
        x = torch.randn(M, C, device=dev)
        xn = x.view(B, H, H, C).permute(0, 3, 1, 2).contiguous().to(BF16).requires_grad_(True)        # the torch route's NCHW bf16 activation
        xr = x.to(BF16).requires_grad_(True)
        gr = torch.randn(M, C, device=dev)
        sc = prep["scratch"][C]
        w7 = blk[0].weight.to(BF16)

        def t_dw():
            xn.grad = None
            F.conv2d(xn, w7, blk[0].bias.to(BF16), padding=3, groups=C).backward(xn)

        def h_dw():
            ops.dwconv7_fwd(x.view(B, H, H, C), p["wd"], p["bd"])
            ops.dwconv7_bwd(gr.view(B, H, H, C), p["wd"], add=x.view(B, H, H, C))

        def t_ln():
            xr.grad = None
            F.layer_norm(xr.float(), (C,), blk[2].weight, blk[2].bias, EPS).to(BF16).backward(xr)

        y_, mean_, rstd_ = ops.layernorm_affine_fwd(x, p["g"], p["be"], EPS)

        def h_ln():
            ops.layernorm_affine_fwd(x, p["g"], p["be"], EPS)
            ops.layernorm_affine_bwd(y_, x, mean_, rstd_, p["g"], sc[0], sc[1])

        def t_mlp():
            xr.grad = None
            with torch.autocast("cuda", dtype=BF16):
                F.linear(F.gelu(F.linear(xr, blk[3].weight, blk[3].bias)), blk[5].weight, blk[5].bias).backward(xr)

        yp = P._pad_k(y_)
        dg_, h_ = ops.gemm_nt(yp, p["w1"], ops.EPI_GELU_DG, bias=p["b1"])
        gb = P._pad_k(ops.cast_bf16(gr))

        def h_mlp():
            _, h = ops.gemm_nt(yp, p["w1"], ops.EPI_GELU_DG, bias=p["b1"])
            ops.gemm_nt(h, p["w2"], ops.EPI_RESID_F32, bias=p["b2"], aux=x)
            ops.gemm_nt(ops.gemm_nt(gb, p["w2t"], ops.EPI_DMUL, aux=dg_), p["w1t"], ops.EPI_BIAS_BF16)

        # what the hip route's kernels must move / compute per forward + backward of one block at this shape
        floors = {"dwconv": (4 * M * C * 2 + 4 * M * C * 3) / (hbm_tbs * 1e12) * 1e3,                      # fwd: read + write fp32; bwd: read 2, write 1
                  "layernorm": ((4 + 2) * M * C + (2 + 4 + 4) * M * C) / (hbm_tbs * 1e12) * 1e3,
                  "mlp_gemms": 4 * 2 * M * C * 4 * C / (tflops * 1e12) * 1e3}
        for fam, t_fn, h_fn in (("dwconv", t_dw, h_dw), ("layernorm", t_ln, h_ln), ("mlp_gemms", t_mlp, h_mlp)):
            r = _ab({"torch": t_fn, "hip": h_fn}, rounds, reps)
            r["floor_ms"] = round(floors[fam], 4)
            r["verdict"] = _verdict(r)
            out[f"{fam}_stage{s + 1}_C{C}_M{M}"] = r
            # a loss call runs the forward on 2B images and the backward on B: 1.5 x (forward + backward at B) to first order
            for k in ("torch", "hip"):
                total[fam][k] += 1.5 * depth * r[k]["median_ms"]
            total[fam]["floor_ms"] += 1.5 * depth * floors[fam]
        del x, xn, xr, gr, y_, yp, dg_, h_, gb
    img = torch.rand(B, 3, IMG, IMG, device=dev)
    imr = img.clone().requires_grad_(True)
    th, tw = P.band_tables(IMG, size, dev), P.band_tables(IMG, size, dev)
    grow = torch.randn(B * (size // 4) ** 2, 64, device=dev)

    def t_rs():
        imr.grad = None
        o = (F.interpolate(imr, size=size, mode="bilinear", align_corners=False, antialias=True) - module.imagenet_mean) / module.imagenet_std
        o.backward(o.detach())

    def h_rs():
        ops.resize_norm_fwd(img, th[0], tw[0], prep["mean"], prep["std"], size)
        ops.resize_norm_bwd(grow, th[1], tw[1], prep["std"], B, IMG, IMG, size)

    r = _ab({"torch": t_rs, "hip": h_rs}, rounds, reps)
    r["floor_ms"] = round((4 * img.numel() * 2 + 2 * grow.numel() + 4 * grow.numel()) / (hbm_tbs * 1e12) * 1e3, 4)
    r["verdict"] = _verdict(r)
    out["resize_norm"] = r
    out["network_totals_ms"] = {f: {k: round(v, 3) for k, v in t.items()} for f, t in total.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-families", action="store_true")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate for the byte floors, TB/s")
    ap.add_argument("--bf16-tflops", type=float, default=2500.0, help="dense bf16 MFMA rate for the FLOP floors, TFLOP/s")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("bench_perceptual: at least 5 rounds")
    from vitamd.perceptual import PerceptualLoss
    dev = torch.device("cuda")
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hip = PerceptualLoss().to(dev)
    # torchvision's layer_scale of 1e-6 hides the blocks from the loss check: spread it so both routes are compared on a live network
    for name, p in hip.named_parameters():
        if name.endswith("layer_scale"):
            p.data.normal_(0, 0.1)
    hip._prep = None
    ref = TorchRoute(hip)
    B = args.batch
    out = {"batch": B, "image": IMG, "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    tgt = torch.rand(B, 3, IMG, IMG, device=dev)
    inp = (tgt + 0.1 * torch.randn_like(tgt)).clamp(0, 1).requires_grad_(True)

    def loss(route):
        inp.grad = None
        l = (hip if route == "hip" else ref)(inp, tgt)
        l.backward()
        return l.detach()

    a, b = float(loss("hip")), float(loss("torch"))
    if not abs(a - b) <= 5e-2 * max(abs(b), 1e-6):
        raise SystemExit(f"bench_perceptual: the two routes disagree on the loss: {a} vs {b}")
    out["loss_check"] = {"torch": b, "hip": a}
    peaks = {}
    for route in ("torch", "hip"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss(route)
        torch.cuda.synchronize()
        peaks[route] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)
    out["loss"] = _ab({"torch": lambda: loss("torch"), "hip": lambda: loss("hip")}, args.rounds, args.reps)
    out["loss"]["peak_GiB_above_resident"] = peaks
    out["loss"]["verdict"] = _verdict(out["loss"])
    out["loss"]["img_per_s"] = {k: round(B / (out["loss"][k]["median_ms"] * 1e-3), 1) for k in ("torch", "hip")}
    del inp, tgt
    if not args.skip_families:
        out["families"] = families(hip, B, args.rounds, args.reps, args.hbm_tbs, args.bf16_tflops)
    if not args.skip_step:
        import train_titok as TT
        import train_vit_vqgan as TQ
        from vitamd.functions import WEIGHTS
        for key, make, bs in (("step_titok_s_b256", lambda: TT.TiTok(TT.TiTokConfig(IMG, 16, 32, 2048, 12, "S")), 256),
                              ("step_vitvqgan_b_b128", lambda: TQ.ViTVQGAN(TQ.ViTVQGANConfig(IMG, 16, 2048, 12, "B")), 128)):
            torch.manual_seed(0)
            model = make().to(dev)
            x = torch.rand(bs, 3, IMG, IMG, device=dev)

            def step(route):
                model.zero_grad(set_to_none=True)
                WEIGHTS.clear()
                recon, _, ql = model(x)
                l = F.mse_loss(recon, x) + (hip if route == "hip" else ref)(recon, x) + ql
                l.backward()
                return l.detach()

            out[key] = {"batch": bs, "loss_check": {"hip": float(step("hip")), "torch": float(step("torch"))}}
            out[key].update(_ab({"torch": lambda: step("torch"), "hip": lambda: step("hip")}, args.rounds, 1))
            out[key]["verdict"] = _verdict(out[key])
            out[key]["img_per_s"] = {k: round(bs / (out[key][k]["median_ms"] * 1e-3), 1) for k in ("torch", "hip")}
            del model, x
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
