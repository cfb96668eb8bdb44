"""Mixup / CutMix / label smoothing fused into the device input feed and the loss (csrc/input.hip vitamd_frames_prep_mix, csrc/loss.hip
vitamd_soft_cross_entropy_*, vitamd/mix.py) against the route a user writes today, on one MI355X, at ViT-B/16 224
batch 256 from 256 x 256 uint8 frames.  Device-event timings, warmed, the routes alternated round by round in one process, median of
--rounds rounds with the spread (min .. max); prints one JSON line and writes it to --out when given.  Before anything is timed the
routes of a comparison must agree.

  prep   - device time, uint8 frames on the device -> the bf16 patch rows of the MIXED batch, for a Mixup batch and a CutMix batch:
             torch:  Frames.images() (the plain prep kernel, fp32 batch out), then flip(0) / mul / mul / add (Mixup) or a slice copy
                     from the flipped batch (CutMix, one box per batch as timm's batch mode), then ops.im2col
             fused:  vitamd_frames_prep_mix, one launch (the record is on the device for both)
  loss   - device time, forward + backward on bf16 logits [256, 1000]:
             torch:  (-one_hot_mix * log_softmax(x.float())).sum(-1).mean() and its autograd backward, the [B, classes] target built
                     inside the window (two scatters and the smoothing)
             fused:  lm.soft_cross_entropy
  step   - a whole train_step, data included, host clock around --reps steps ending in a synchronise:
             device_loader: DeviceLoader -> train_step with the hard-label loss (no mixing: the step as it is today)
             mix_loader:    MixLoader (host draw, staging copy, mixing prep) -> train_step with SoftTargetLoss(0.1)
usage: bench_mix.py [--rounds N] [--reps N] [--skip-step] [--out FILE]"""
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
        raise SystemExit("bench_mix: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix: needs a GPU (no timing is taken without one)")
    import train_vit as TV
    from vitamd import data, lm, mix, ops
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

    # ---- (1) prep + mix: one record per mode (one decision per batch, as timm's default)
    out["prep"] = {}
    for name, m in (("mixup", mix.Mix(0.8, 0.0, seed=1)), ("cutmix", mix.Mix(0.0, 1.0, seed=1))):
        rec_h, lam_h = m.draw(BATCH, (SIZE, SIZE), 0)
        rec, lam = rec_h.to(dev), lam_h.to(dev)
        mode, yl, yh, xl, xh = rec_h[0, 1:].tolist()
        l = lam[0]

        def torch_route():
            x = data.Frames(u8, SIZE, geom=geom, table=table).images()
            if mode == 1:
                x = x.mul(l).add(x.flip(0).mul(1 - l))
            else:
                x = x.clone()
                x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
            return ops.im2col(x, PATCH)

        fused = lambda: ops.frames_prep(u8, (SIZE, SIZE), table, PATCH, False, None, geom, mix=(rec, lam))[0]
        want, got = torch_route(), fused()
        share = float((got.view(torch.int16) == want.view(torch.int16)).float().mean())
        # CutMix is a select: equal bits.  Mixup: torch's device kernels may fuse the blend's product into its sum, so the two device
        # routes are held to a bf16 ulp here (tests/test_gpu_mix.py holds the kernel to the CPU's bits) and the exact share is reported
        diff = float((got.float() - want.float()).abs().max())
        if not (share == 1.0 if mode == 2 else diff <= 2.0 ** -7 * float(want.float().abs().max())):
            raise SystemExit(f"bench_mix: {name}: the fused and the torch route disagree (max abs diff {diff}, bit-equal share {share})")
        k = _alternate({"torch": torch_route, "fused": fused}, args.rounds, args.reps, _device_ms)
        k["record"] = {"mode": mode, "lam": round(float(l), 4), "box": [yl, yh, xl, xh]}
        k["patch_rows_bit_equal_share"] = round(share, 6)
        k["speedup"] = round(k["torch"]["median"] / k["fused"]["median"], 2)
        out["prep"][name] = k
        del want, got

    # ---- (2) the loss, forward + backward on bf16 logits
    logits = (torch.randn(BATCH, CLASSES, generator=gen) * 3).to(torch.bfloat16).to(dev)
    ya = labels_host.to(dev)
    yb = ya.flip(0)
    lam = torch.rand(BATCH, generator=gen).to(dev)

    def torch_loss():
        x = logits.detach().requires_grad_(True)
        t = torch.zeros((BATCH, CLASSES), device=dev)
        t.scatter_add_(1, ya[:, None], lam[:, None]).scatter_add_(1, yb[:, None], (1 - lam)[:, None])
        t = t * (1 - SMOOTHING) + SMOOTHING / CLASSES
        loss = (-t * torch.log_softmax(x.float(), dim=-1)).sum(-1).mean()
        loss.backward()
        return loss.detach(), x.grad

    def fused_loss():
        x = logits.detach().requires_grad_(True)
        loss = lm.soft_cross_entropy(x, ya, yb, lam, SMOOTHING)
        loss.backward()
        return loss.detach(), x.grad

    (lt, gt), (lf, gf) = torch_loss(), fused_loss()
    if not abs(float(lt) - float(lf)) <= 1e-5 * max(1.0, abs(float(lt))) or not float((gt.float() - gf.float()).abs().max()) <= 2.0 ** -7 / BATCH:
        raise SystemExit(f"bench_mix: the two losses disagree: {float(lt)} against {float(lf)}")
    out["loss"] = _alternate({"torch": torch_loss, "fused": fused_loss}, args.rounds, args.reps, _device_ms)
    out["loss"]["speedup"] = round(out["loss"]["torch"]["median"] / out["loss"]["fused"]["median"], 2)

    # ---- (3) whole training steps, data included
    if not args.skip_step:
        torch.manual_seed(0)
        model = TV.ViTClassifier(TV.ViTConfig(SIZE, 3, PATCH, "B", 1, 0.0), CLASSES).to(dev)
        optim = torch.optim.AdamW(model.parameters(), lr=1e-4)
        u8_pinned = u8_host.pin_memory()

        def forever():
            while True:
                yield u8_pinned, labels_host

        kw = dict(patch=PATCH, image=False, mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, train=True, seed=1)
        plain = data.DeviceLoader(forever(), dev, SIZE, **kw)
        mixed = mix.MixLoader(forever(), dev, SIZE, mix.Mix(0.8, 1.0, label_smoothing=SMOOTHING, seed=1), **kw)
        soft = mix.SoftTargetLoss(SMOOTHING)

        def device_loader():
            x, y = next(plain)
            TV.train_step(model, x, y, optim)

        def mix_loader():
            x, y = next(mixed)
            TV.train_step(model, x, y, optim, loss_fn=soft)

        out["step"] = _alternate({"device_loader": device_loader, "mix_loader": mix_loader}, args.rounds, args.reps, _host_ms)
        out["step"]["images_per_s"] = {r: round(BATCH / (out["step"][r]["median"] * 1e-3), 1) for r in ("device_loader", "mix_loader")}
        out["step"]["mix_over_plain"] = round(out["step"]["mix_loader"]["median"] / out["step"]["device_loader"]["median"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
