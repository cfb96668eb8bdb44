"""MI355X-native drop-in for the model half of the reference's `train_titok` module
(reference train_titok.py:18-93): TiTokConfig, TiTokEncoder, Quantizer, TiTokDecoder, TiTok with
the same constructor signatures, attributes and state_dict keys (`enc.vit.*`, `enc.proj.*`,
`quant.codebook.weight`, `dec.vit.*`, `dec.quant_proj.*`, `dec.embd_proj.*`).  Both ViTs, the three
projections and the nearest-code search run on libvitamd kernels; the O(tokens x latent_dim)
elementwise glue of the quantiser (L2 normalise, the two MSE terms, the straight-through add) and the
pure data movement (token slicing, pixel shuffle) are torch device ops."""
import argparse
import time
from dataclasses import dataclass

import torch
import torch.nn as nn

from train_vit import ViT, ViTConfig
from utils import get_lr_scheduler
from vitamd import ops, tokenizer
from vitamd.data import Frames
from vitamd.functions import linear


@dataclass
class TiTokConfig:
    image_size: int
    patch_size: int
    latent_tokens: int
    codebook_size: int
    latent_dim: int
    transformer: str

    def __post_init__(self):
        self.patch_dim = self.image_size // self.patch_size
        self.n_patches = self.patch_dim ** 2
        self.enc_vit_config = ViTConfig(self.image_size, 3, self.patch_size, self.transformer, self.latent_tokens, 0.0)
        self.n_embd = self.enc_vit_config.trans_config.n_embd
        # decoder: 1x1 "patches" over the latent tokens, one learned mask token per image patch as extra tokens
        self.dec_vit_config = ViTConfig(self.latent_tokens, self.n_embd, 1, self.transformer, self.n_patches, 0.0)
        self.dec_vit_config.n_patches = self.latent_tokens


class HipLinear(nn.Linear):
    """nn.Linear parameters (same state_dict keys), forward/backward on the MFMA GEMMs."""

    def forward(self, x):
        return linear(x, self.weight, self.bias)


class HipConv1x1(nn.Conv2d):
    """nn.Conv2d(kernel_size=1) parameters, applied to TOKEN-major input [B, T, C] -> [B, T, out]."""

    def forward(self, tokens):
        return linear(tokens, self.weight, self.bias)


def pixel_shuffle_tokens(y, grid, p):
    """[B, grid*grid, p*p*c] -> [B, c, grid*p, grid*p]; the two rearranges of reference
    train_titok.py:73-75 composed ('b (h w) (p1 p2 c) -> b c (h p1) (w p2)')."""
    B, _, F = y.shape
    c = F // (p * p)
    return y.view(B, grid, grid, p, p, c).permute(0, 5, 1, 3, 2, 4).reshape(B, c, grid * p, grid * p)


class TiTokEncoder(nn.Module):
    def __init__(self, titok_config: TiTokConfig):
        super().__init__()
        self.latent_tokens = titok_config.latent_tokens
        self.vit = ViT(titok_config.enc_vit_config)
        self.proj = HipLinear(titok_config.n_embd, titok_config.latent_dim)

    def forward(self, x):
        return self.proj(self.vit(x, keep=self.latent_tokens))   # latent tokens are the PREPENDED extra tokens: [:, :latent_tokens]


class Quantizer(nn.Module):
    def __init__(self, titok_config):
        super().__init__()
        self.codebook = nn.Embedding(titok_config.codebook_size, titok_config.latent_dim)
        self.codebook.weight.data.uniform_(-1.0 / titok_config.codebook_size, 1.0 / titok_config.codebook_size)

    def forward(self, x):
        """cosine-similarity VQ (behaviour of reference train_titok.py:50-59): tokens and codes are compared on the unit sphere,
        the RAW code rows are what comes out; loss = |codes - sg(tokens)|^2 + 0.25 |sg(codes) - tokens|^2 (means); straight-through"""
        unit = torch.nn.functional.normalize(x, dim=-1)
        with torch.no_grad():
            codes_unit = torch.nn.functional.normalize(self.codebook.weight, dim=-1).float().contiguous()
            ids = ops.vq_nearest(unit.reshape(-1, unit.shape[-1]).float().contiguous(), codes_unit).view(unit.shape[:-1])
        picked = self.codebook(ids)
        sq = lambda t: t.pow(2).mean()
        loss = sq(picked - unit.detach()) + 0.25 * sq(picked.detach() - unit)
        return unit + (picked - unit).detach(), ids, loss


class TiTokDecoder(nn.Module):
    def __init__(self, titok_config: TiTokConfig):
        super().__init__()
        self.config = titok_config
        self.vit = ViT(titok_config.dec_vit_config)
        self.quant_proj = HipLinear(titok_config.latent_dim, titok_config.n_embd)
        self.embd_proj = HipConv1x1(titok_config.n_embd, 3 * titok_config.patch_size ** 2, kernel_size=1)

    def features(self, z):
        """quantised latents -> the decoder ViT's output at the image patches [b, n_patches, n_embd], before the pixel head"""
        z = self.quant_proj(z)                                   # [b, latents, n_embd]
        z = z.transpose(1, 2).unsqueeze(-1)                      # 'b h c -> b c h 1'
        return self.vit(z, keep=self.config.n_patches)           # mask tokens come first (extra tokens): [:, :n_patches]

    def forward(self, z):
        return pixel_shuffle_tokens(self.embd_proj(self.features(z)), self.config.patch_dim, self.config.patch_size)


class TiTok(nn.Module):
    def __init__(self, titok_config: TiTokConfig):
        super().__init__()
        self.config = titok_config
        self.enc = TiTokEncoder(titok_config)
        self.quant = Quantizer(titok_config)
        self.dec = TiTokDecoder(titok_config)

    def encode(self, z):
        """image -> code ids [b, latent_tokens]"""
        _, ids, _ = self.quant(self.enc(z))
        return ids

    def decode(self, z_quant):
        return self.dec(z_quant)

    def decode_indices(self, indices):
        return self.dec(self.quant.codebook(indices))

    def forward(self, x):
        """-> (reconstruction [b, 3, H, W], code ids, quantiser loss)"""
        tokens, ids, qloss = self.quant(self.enc(x))
        return self.dec(tokens), ids, qloss

    def loss(self, x):
        """-> (reconstruction loss mse(recon, x), quantiser loss, code ids) on the fused route (vitamd.tokenizer):
        encoder -> vq_quantize -> quant_proj -> decoder ViT -> linear_recon_mse on embd_proj's parameters.  No reconstruction image is
        formed; forward() stays the route that yields one."""
        return tokenizer_loss(self.enc, self.quant, self.dec, x)


def tokenizer_loss(enc, quant, dec, x):
    """the loss route shared by TiTok and ViTVQGAN (their decoders both have features(), embd_proj and config).  x: fp32 images, or
    uint8 vitamd.data.Frames - one launch then makes the encoder's patch rows and the fp32 target together"""
    target = x.materialise(enc.vit.config.patch_size, image=True).images() if isinstance(x, Frames) else x
    tokens, ids, qloss = tokenizer.vq_quantize(enc(x), quant.codebook.weight)
    recon = tokenizer.linear_recon_mse(dec.features(tokens), dec.embd_proj.weight, dec.embd_proj.bias, target, dec.config.patch_dim, dec.config.patch_size)
    return recon, qloss, ids


def train_step(model, images, optim, lr_sched=None, perceptual=None, perceptual_weight=1.0):
    """One iteration of the reference hot loop (train_titok.py:151-163) without the fp16 scaler, on model.loss: the pixel term is the mean
    squared error.  perceptual: a callable (recon, images) -> a loss or per-image values - vitamd.perceptual.PerceptualLoss, the reference's
    frozen ConvNeXt-S on this library's kernels, fits as it is: the step then runs model(images), which yields the image, and adds
    perceptual_weight * perceptual(recon, images).mean().
    The reference clips the gradients AFTER the optimiser step, where the clip changes no update; this step does not clip.
    -> the detached device loss"""
    optim.zero_grad(set_to_none=True)
    if perceptual is None:
        recon_loss, qloss, _ = model.loss(images)
    else:
        target = images.materialise(model.config.patch_size, image=True).images() if isinstance(images, Frames) else images
        recon, _, qloss = model(images)
        recon_loss = torch.nn.functional.mse_loss(recon, target) + perceptual_weight * perceptual(recon, target).mean()
    loss = recon_loss + qloss
    loss.backward()
    optim.step()
    if lr_sched is not None:
        lr_sched.step()
    return loss.detach()


def evaluate(model, batches, recon=None, codes=None):
    """The validation half of the loop: vitamd.metrics.evaluate_tokenizer on model(x) = (reconstruction, code ids, quantiser loss) ->
    {"mse", "mae", "psnr", "ssim", "count", "usage", "used", "dead", "perplexity", "entropy", "codes", "bad"}, one host read at the end"""
    from vitamd.metrics import evaluate_tokenizer
    return evaluate_tokenizer(model, batches, recon=recon, codes=codes, patch=model.config.patch_size)


def make_val_batches(args, dev):
    """the args.eval_batches held-out batches of one evaluation (their own seed): fp32 images in [0, 1] on the device"""
    g = torch.Generator(device="cpu").manual_seed(1)
    return [torch.rand((args.bs, 3, args.image_size, args.image_size), generator=g).to(dev) for _ in range(args.eval_batches)]


def report(step, r):
    print(f"step {step} val mse {r['mse']:.5f} mae {r['mae']:.5f} psnr {r['psnr']:.2f} ssim {r['ssim']:.4f} codebook_usage {r['usage']:.3f} "
          f"perplexity {r['perplexity']:.1f} over {r['count']} images")


def add_common_args(p):
    p.add_argument("--image_size", type=int, default=128)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--codebook_size", type=int, default=2048)
    p.add_argument("--latent_dim", type=int, default=12)
    p.add_argument("--transformer", type=str, default="B")
    p.add_argument("--bs", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--warmup_steps", type=int, default=5000)
    p.add_argument("--train_steps", type=int, default=50)
    p.add_argument("--max_grad_norm", type=float, default=None,
                   help="clip the global gradient norm on the device (vitamd.optim.AdamW, multi-tensor path); default: no clipping")
    p.add_argument("--u8", action="store_true",
                   help="feed seeded random uint8 frames through vitamd.data.DeviceLoader (the device input pipeline) instead of one fp32 batch")
    p.add_argument("--resize", type=int, default=None, metavar="S",
                   help="with --u8: the frames come at 3/2 by 2 times the image size (192 x 256 for 128) and are resized on the device, shorter "
                        "side to S, then centre-cropped (vitamd.resize.ResizeLoader)")
    p.add_argument("--perceptual_weight", type=float, default=0.0,
                   help="weight of the ConvNeXt-S perceptual term (reference train_titok.py:155-158); 0 = no perceptual term")
    p.add_argument("--perceptual_weights", type=str, default=None,
                   help="path of a torchvision convnext_small state dict for the perceptual network; without it the network is untrained "
                        "(a throughput stand-in).  Nothing is ever downloaded")
    p.add_argument("--eval_every", type=int, default=0,
                   help="evaluate every N training steps on seeded held-out random data (evaluate / vitamd.metrics: MSE, MAE, PSNR, SSIM and codebook usage "
                        "from counters on the device, one host read per evaluation); 0 = never")
    p.add_argument("--eval_batches", type=int, default=2, help="the batches of one evaluation (--eval_every)")
    return p


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="TiTok training on synthetic images (MI355X-native path)")
    p.add_argument("--latent_tokens", type=int, default=256)
    return add_common_args(p).parse_args(argv)


def make_optim(model, args):
    if args.max_grad_norm is None:
        return torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    from vitamd.optim import AdamW
    return AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm)


def make_perceptual(args):
    """the perceptual network the arguments ask for, or None (weight 0: the step stays on the fused model.loss route)"""
    if args.perceptual_weight <= 0:
        return None
    from vitamd.perceptual import PerceptualLoss
    return PerceptualLoss("convnext_s", weights=args.perceptual_weights)


def run(model, args, codebook_size):
    """the training loop of both tokenizers on one seeded batch of random images in [0, 1], with the reference's codebook-usage counter"""
    dev = torch.device("cuda")
    model = model.to(dev)
    optim = make_optim(model, args)
    sched = get_lr_scheduler(optim, args.warmup_steps, args.train_steps, args.lr / 10)
    perceptual = make_perceptual(args)
    if perceptual is not None:
        perceptual = perceptual.to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    images = torch.rand((args.bs, 3, args.image_size, args.image_size), generator=g).to(dev)
    usage = torch.zeros([codebook_size], device=dev)
    feed = None
    if getattr(args, "u8", False):
        from vitamd.data import DeviceLoader
        if getattr(args, "resize", None) is not None:
            from vitamd.resize import ResizeLoader
            u8 = torch.randint(0, 256, (args.bs, args.image_size * 3 // 2, args.image_size * 2, 3), generator=g, dtype=torch.uint8)
            feed = ResizeLoader(((u8, None) for _ in range(args.train_steps)), dev, args.image_size, mode="resize_crop", resize_to=args.resize,
                                patch=args.patch_size, train=False)
        else:
            u8 = torch.randint(0, 256, (args.bs, args.image_size, args.image_size, 3), generator=g, dtype=torch.uint8)
            feed = DeviceLoader(((u8, None) for _ in range(args.train_steps)), dev, args.image_size, patch=args.patch_size, train=False)
    if args.eval_every < 0 or (args.eval_every > 0 and args.eval_batches < 1):
        raise SystemExit("--eval_every needs N >= 0 and --eval_batches >= 1")
    val = make_val_batches(args, dev) if args.eval_every > 0 else None
    for step in range(args.train_steps):
        t0 = time.time()
        if feed is not None:
            images, _ = next(feed)
        loss = train_step(model, images, optim, sched, perceptual=perceptual, perceptual_weight=args.perceptual_weight)
        with torch.no_grad():
            usage[model.encode(images)] = 1
        torch.cuda.synchronize()
        print(f"step {step} loss {loss.item():.4f} codebook_usage {usage.sum().item() / codebook_size:.3f} "
              f"{args.bs / (time.time() - t0):.1f} images/s")
        if val is not None and (step + 1) % args.eval_every == 0:
            report(step, evaluate(model, val))


def main():
    args = parse_args()
    if args.resize is not None and not args.u8:
        raise SystemExit("--resize resizes inside the device input feed (vitamd.resize.ResizeLoader): it needs --u8")
    cfg = TiTokConfig(args.image_size, args.patch_size, args.latent_tokens, args.codebook_size, args.latent_dim, args.transformer)
    run(TiTok(cfg), args, cfg.codebook_size)


if __name__ == "__main__":
    main()
