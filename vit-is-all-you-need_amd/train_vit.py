"""MI355X-native drop-in for the model half of the reference's `train_vit` module
(reference train_vit.py:16-53): ViTConfig, ViT, ViTClassifier with identical constructor
signatures, attributes (.config, .patch_proj, .pos_emb, .extra_emb, .transformer, .vit, .head) and
state_dict keys, so `from train_vit import ViTConfig, ViT` (train_titok.py:8, train_vit_vqgan.py:8)
resolves here.  The training loop of the reference (train_vit.py:55-129) is re-stated in
`train_step` / `main` without wandb / torchvision / fp16 GradScaler: bf16 needs no loss scaling.
"""
import argparse
import time
from dataclasses import dataclass

import torch
import torch.nn as nn

from transformer import Transformer, transformer_configs
from utils import get_lr_scheduler
from vitamd.functions import PatchEmbedFn, linear


@dataclass
class ViTConfig:
    image_size: int
    in_channels: int
    patch_size: int
    transformer: str
    extra_tokens: int
    dropout: float

    def __post_init__(self):
        self.n_patches = (self.image_size // self.patch_size) ** 2
        self.patch_dim = 3 * self.patch_size ** 2  # hard-coded 3 as in the reference (train_vit.py:27); unused
        self.trans_config = transformer_configs[self.transformer](block_size=self.n_patches + self.extra_tokens,
                                                                  dropout=self.dropout)


class ViT(nn.Module):
    def __init__(self, args: ViTConfig):
        super().__init__()
        self.config = args
        D = args.trans_config.n_embd
        self.patch_proj = nn.Conv2d(in_channels=args.in_channels, out_channels=D, kernel_size=args.patch_size,
                                    stride=args.patch_size)
        self.pos_emb = nn.Embedding(args.n_patches, D)
        self.extra_emb = nn.Embedding(args.extra_tokens, D)
        self.transformer = Transformer(args.trans_config)

    def forward(self, x, keep=None):
        """keep=k: only the first k tokens are wanted -> [B, k, D] = forward(x)[:, :k] (Transformer.forward, keep=)"""
        # conv patchify + (h w) flatten + pos_emb + prepended extra tokens in one GEMM epilogue
        emb = PatchEmbedFn.apply(x, self.patch_proj.weight, self.patch_proj.bias, self.pos_emb.weight,
                                 self.extra_emb.weight, self.config.patch_size, self.config.n_patches)
        return self.transformer(emb, keep=keep)


class ViTClassifier(nn.Module):
    def __init__(self, vit_config: ViTConfig, num_classes=1000):
        super().__init__()
        self.vit = ViT(vit_config)
        self.head = nn.Linear(vit_config.trans_config.n_embd, num_classes)

    def forward(self, x):
        # the head reads the class token alone (train_vit.py:53): the stack's last layer runs its MLP on that row only
        return linear(self.vit(x, keep=1)[:, 0], self.head.weight, self.head.bias)


def train_step(model, images, labels, optim, lr_sched=None, loss_fn=None):
    """One iteration of the reference hot loop (train_vit.py:99-107) without the fp16 scaler."""
    loss_fn = loss_fn or nn.functional.cross_entropy
    optim.zero_grad(set_to_none=True)
    loss = loss_fn(model(images), labels)
    loss.backward()
    optim.step()
    if lr_sched is not None:
        lr_sched.step()
    return loss


def evaluate(model, batches, topk=5, metrics=None):
    """The validation half of the reference loop (train_vit.py:114-128) without its per-batch .item()s: the model in eval mode under
    torch.no_grad() over `batches` of (images fp32 [B, C, H, W] or vitamd.data.Frames, int64 labels on the device), every batch added to
    a vitamd.metrics.ClassifyMetrics on the device (metrics: one to continue; None: a fresh one).  The host reads nothing before the
    final result() -> {"loss", "top1", "topk", "count", "perplexity"}.  model.training is put back, also when a batch raises."""
    from vitamd.metrics import ClassifyMetrics
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for images, labels in batches:
                if metrics is None:
                    metrics = ClassifyMetrics(topk=topk, device=labels.device)
                metrics.update(model(images), labels)
    finally:
        model.train(was_training)
    if metrics is None:
        raise ValueError("evaluate: no batches")
    return metrics.result()


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="ViT classifier training on synthetic data (MI355X-native path)")
    p.add_argument("--image_size", type=int, default=224)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--extra_tokens", type=int, default=1)
    p.add_argument("--transformer", type=str, default="B")
    p.add_argument("--num_classes", type=int, default=1000)
    p.add_argument("--bs", type=int, default=256)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-2)
    p.add_argument("--warmup_steps", type=int, default=10)
    p.add_argument("--train_steps", type=int, default=50)
    p.add_argument("--u8", action="store_true",
                   help="feed seeded random uint8 frames through vitamd.data.DeviceLoader (the device input pipeline: random crop and flip, ImageNet normalisation) instead of one fp32 batch")
    p.add_argument("--rrc", action="store_true",
                   help="with --u8: RandomResizedCrop on the device (vitamd.resize.ResizeLoader, mode rrc) from frames of --src_size")
    p.add_argument("--rrc_scale", type=float, nargs=2, default=(0.08, 1.0), metavar=("LO", "HI"), help="the area range of --rrc")
    p.add_argument("--resize", type=int, default=None, metavar="S",
                   help="with --u8 and without --rrc: the reference's transform Resize(S) -> RandomCrop(image_size) -> flip on the device "
                        "(vitamd.resize.ResizeLoader, mode resize_crop) from frames of --src_size")
    p.add_argument("--src_size", type=int, nargs=2, default=None, metavar=("H", "W"),
                   help="the size of the seeded random source frames of --rrc / --resize (default: a non-square 8 : 7 frame, 320 x 280 at 224)")
    p.add_argument("--max_grad_norm", type=float, default=None,
                   help="clip the global gradient norm on the device (vitamd.optim.AdamW, multi-tensor path); default: no clipping")
    p.add_argument("--dropout", type=float, default=0.0)
    p.add_argument("--mixup", type=float, default=0.0, help="Mixup: the alpha of its Beta draw (0 = off); needs --u8 (vitamd.mix.MixLoader; with --rrc / --resize vitamd.mix.ResizeMixLoader)")
    p.add_argument("--cutmix", type=float, default=0.0, help="CutMix: the alpha of its Beta draw (0 = off); needs --u8")
    p.add_argument("--mix_prob", type=float, default=1.0, help="the chance that a batch is mixed at all")
    p.add_argument("--mix_switch_prob", type=float, default=0.5, help="the chance of CutMix when both --mixup and --cutmix are on")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="label smoothing of the soft-target loss (vitamd.lm.soft_cross_entropy); also works on the fp32 batch")
    p.add_argument("--reprob", type=float, default=0.0,
                   help="Random Erasing: the chance that a sample is erased (0 = off; the DeiT / timm recipe takes 0.25); needs --u8 "
                        "(vitamd.erase: the batch is erased after the mix, behind the prep launch)")
    p.add_argument("--remode", type=str, default="pixel", choices=("const", "rand", "pixel"),
                   help="what an erased box is filled with: zeros, one N(0, 1) value per channel, or one per pixel and channel")
    p.add_argument("--recount", type=int, default=1, help="the most boxes an erased sample gets (their number is drawn from 1 .. this)")
    p.add_argument("--graph", action="store_true",
                   help="one graph launch per iteration (vitamd.graph.GraphedTrainStep): forward, loss, backward, the clip, the LR schedule "
                        "and the AdamW update, all replayed from the device; needs --dropout 0 (and not --u8)")
    p.add_argument("--eval_every", type=int, default=0,
                   help="evaluate every N training steps on seeded held-out random data (evaluate / vitamd.metrics.ClassifyMetrics: loss, "
                        "top-1 and top-k from counters on the device, one host read per evaluation); 0 = never")
    p.add_argument("--eval_batches", type=int, default=2, help="the batches of one evaluation (--eval_every)")
    return p.parse_args(argv)


def make_val_batches(args, dev):
    """-> a function whose every call yields the same args.eval_batches held-out batches (their own seed): fp32 images, or with --u8 uint8
    frames through the training feed's loader with train=False (the centre crop; after --rrc / --resize, Resize + CenterCrop)"""
    g = torch.Generator(device="cpu").manual_seed(1)
    n, size = args.eval_batches, args.image_size
    labels = [torch.randint(0, args.num_classes, (args.bs,), generator=g) for _ in range(n)]
    if not args.u8:
        images = [torch.randn(args.bs, 3, size, size, generator=g) for _ in range(n)]
        return lambda: ((x.to(dev), y.to(dev)) for x, y in zip(images, labels))
    from vitamd.data import IMAGENET_MEAN, IMAGENET_STD, DeviceLoader
    resizing = args.rrc or args.resize is not None
    src_hw = (size + size // 7,) * 2
    if resizing:
        src_hw = tuple(args.src_size) if args.src_size is not None else (size * 10 // 7, size * 5 // 4)
    u8 = [torch.randint(0, 256, (args.bs, *src_hw, 3), generator=g, dtype=torch.uint8) for _ in range(n)]
    kw = dict(patch=args.patch_size, image=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, train=False)
    if resizing:
        from vitamd.resize import ResizeLoader
        return lambda: ResizeLoader(zip(u8, labels), dev, size, mode="rrc" if args.rrc else "resize_crop", resize_to=args.resize, **kw)
    return lambda: DeviceLoader(zip(u8, labels), dev, size, **kw)


def make_optim(model, args):
    from vitamd.optim import AdamW
    if getattr(args, "graph", False):
        return AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm, capturable=True,
                     schedule=(args.warmup_steps, args.train_steps, args.lr / 10))
    if args.max_grad_norm is None:
        return torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    return AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm)


def main(argv=None):
    args = parse_args(argv)
    if args.graph and args.u8:
        raise SystemExit("--graph with --u8: the device loader hands over vitamd.data.Frames (patch rows in buffers of its own), not tensors "
                         "to copy into a graph's static inputs; a graph-fed loader is not built - use one or the other")
    if args.eval_every < 0 or (args.eval_every > 0 and args.eval_batches < 1):
        raise SystemExit("--eval_every needs N >= 0 and --eval_batches >= 1")
    topk = min(5, args.num_classes)                                 # of the evaluations: top-5, or all the classes of a smaller head
    mixing = args.mixup > 0 or args.cutmix > 0
    if mixing and not args.u8:
        raise SystemExit("--mixup / --cutmix mix inside the device input feed (vitamd.mix.MixLoader): they need --u8")
    erasing = args.reprob > 0
    if (erasing or args.remode != "pixel" or args.recount != 1) and not args.u8:
        raise SystemExit("--reprob / --remode / --recount erase the batch of the device input feed (vitamd.erase): they need --u8")
    if args.graph and args.label_smoothing > 0:
        raise SystemExit("--graph with --label_smoothing: the graphed step is built on the hard-label loss - use one or the other")
    resizing = args.rrc or args.resize is not None
    if resizing and not args.u8:
        raise SystemExit("--rrc / --resize resize inside the device input feed (vitamd.resize.ResizeLoader): they need --u8")
    if args.src_size is not None and not resizing:
        raise SystemExit("--src_size goes with --rrc or --resize")
    dev = torch.device("cuda")
    cfg = ViTConfig(args.image_size, 3, args.patch_size, args.transformer, args.extra_tokens, args.dropout)
    model = ViTClassifier(cfg, args.num_classes).to(dev)
    optim = make_optim(model, args)
    sched = None if args.graph else get_lr_scheduler(optim, args.warmup_steps, args.train_steps, args.lr / 10)
    g = torch.Generator(device="cpu").manual_seed(0)
    images = torch.randn(args.bs, 3, args.image_size, args.image_size, generator=g).to(dev)
    labels = torch.randint(0, args.num_classes, (args.bs,), generator=g).to(dev)
    feed = None
    if args.u8:
        from vitamd.data import IMAGENET_MEAN, IMAGENET_STD, DeviceLoader
        side = args.image_size + args.image_size // 7           # 256 for 224: the frame the random crop is taken from
        src_hw = (side, side)
        if resizing:                                            # a non-square frame of another size: 320 x 280 for 224
            src_hw = tuple(args.src_size) if args.src_size is not None else (args.image_size * 10 // 7, args.image_size * 5 // 4)
        u8 = torch.randint(0, 256, (args.bs, *src_hw, 3), generator=g, dtype=torch.uint8)
        host_labels = labels.cpu()
        host = ((u8, host_labels) for _ in range(args.train_steps))
        if erasing:                                             # the loader chosen below, with the erasing launch behind its prep launch
            from vitamd import erase as E
            from vitamd.mix import Mix
            er = dict(erase=E.Erase(args.reprob, mode=args.remode, max_count=args.recount, seed=0))
            kw = dict(patch=args.patch_size, image=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0, **er)
            rs = dict(mode="rrc" if args.rrc else "resize_crop", scale=tuple(args.rrc_scale), resize_to=args.resize)
            mix = Mix(args.mixup, args.cutmix, args.mix_prob, args.mix_switch_prob, label_smoothing=args.label_smoothing, seed=0)
            if resizing and mixing:
                feed = E.EraseResizeMixLoader(host, dev, args.image_size, mix, **rs, **kw)
            elif resizing:
                feed = E.EraseResizeLoader(host, dev, args.image_size, **rs, **kw)
            elif mixing:
                feed = E.EraseMixLoader(host, dev, args.image_size, mix, **kw)
            else:
                feed = E.EraseLoader(host, dev, args.image_size, **kw)
        elif resizing and mixing:                                 # the DeiT recipe: RandomResizedCrop and the mix in one launch
            from vitamd.mix import Mix, ResizeMixLoader
            mix = Mix(args.mixup, args.cutmix, args.mix_prob, args.mix_switch_prob, label_smoothing=args.label_smoothing, seed=0)
            feed = ResizeMixLoader(host, dev, args.image_size, mix, mode="rrc" if args.rrc else "resize_crop", scale=tuple(args.rrc_scale),
                                   resize_to=args.resize, patch=args.patch_size, image=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0)
        elif resizing:
            from vitamd.resize import ResizeLoader
            feed = ResizeLoader(host, dev, args.image_size, mode="rrc" if args.rrc else "resize_crop", scale=tuple(args.rrc_scale),
                                resize_to=args.resize, patch=args.patch_size, image=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0)
        elif mixing:
            from vitamd.mix import Mix, MixLoader
            mix = Mix(args.mixup, args.cutmix, args.mix_prob, args.mix_switch_prob, label_smoothing=args.label_smoothing, seed=0)
            feed = MixLoader(host, dev, args.image_size, mix, patch=args.patch_size, image=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0)
        else:
            feed = DeviceLoader(host, dev, args.image_size, patch=args.patch_size, image=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0)
    loss_fn = None                                              # train_step's default: the route a run without these flags takes today
    if mixing or args.label_smoothing > 0:
        from vitamd.mix import SoftTargetLoss
        loss_fn = SoftTargetLoss(args.label_smoothing)
    graphed = None
    if args.graph:
        from vitamd.graph import GraphedTrainStep
        hard_loss = nn.functional.cross_entropy
        graphed = GraphedTrainStep(model, lambda x, y: hard_loss(model(x), y), (images, labels), optim)      # refuses dropout > 0
    val = make_val_batches(args, dev) if args.eval_every > 0 else None
    for step in range(args.train_steps):
        t0 = time.time()
        if feed is not None:
            images, labels = next(feed)
        loss = graphed(images, labels) if graphed is not None else train_step(model, images, labels, optim, sched, loss_fn)
        torch.cuda.synchronize()
        print(f"step {step} loss {loss.item():.4f} {args.bs / (time.time() - t0):.0f} img/s")
        if val is not None and (step + 1) % args.eval_every == 0:
            r = evaluate(model, val(), topk=topk)
            print(f"step {step} val loss {r['loss']:.4f} top1 {r['top1']:.4f} top{topk} {r['topk']:.4f} over {r['count']} samples")


if __name__ == "__main__":
    main()
