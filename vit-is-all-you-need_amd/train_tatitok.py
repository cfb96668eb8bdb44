"""MI355X-native drop-in for the model half of the reference's `train_tatitok` module (reference train_tatitok.py:21-111): the 1D TiTok
tokenizer that train_videogpt.py trains on - TiTokConfig, TiTok and make_optim with the same constructor signatures, attributes and
state_dict keys (`latent_tokens`, `encoder.*`, `decoder.*`, `quantize.embedding.weight`), so reference checkpoints load.

The model composes the wrappers of blocks.py (TiTokEncoder, TiTokDecoder, VectorQuantizer(use_l2_norm=True)).  `forward`, `encode`,
`decode` and `decode_tokens` are the reference's methods on those wrappers.  `loss` is the training route (vitamd/tokenizer.py,
DESIGN.md section 15): encoder -> the unit-code quantiser kernels -> decoder stack -> one head GEMM that writes bf16 tokens -> the fused
pixel tail (conv_out and the mean squared error in one kernel, forward and backward), with the reconstruction as an optional second
output for a perceptual term.  `train_step` is one iteration of the reference loop (train_tatitok.py:185-202) on that route, without
the fp16 scaler, and `main()` runs it on seeded random images.  Gradient accumulation (`micro_steps`), data loading and logging are
not part of this module."""
import argparse
import time
from dataclasses import dataclass
from types import SimpleNamespace

import torch
import torch.nn as nn

from blocks import TiTokDecoder, TiTokEncoder, VectorQuantizer
from train_titok import make_val_batches, report
from utils import get_lr_scheduler
from vitamd import ops, tokenizer
from vitamd.data import Frames


@dataclass
class TiTokConfig:
    image_size: int
    patch_size: int
    latent_tokens: int
    codebook_size: int
    latent_dim: int
    transformer: str
    use_l2_norm: bool = True


class TiTok(nn.Module):
    def __init__(self, config):
        if isinstance(config, dict):
            config = SimpleNamespace(**config)           # the reference wraps a dict in OmegaConf; attribute access is all that is used
        super().__init__()
        self.config = config
        self.encoder = TiTokEncoder(config)
        self.decoder = TiTokDecoder(config)
        self.num_latent_tokens = config.latent_tokens
        scale = self.encoder.width ** -0.5
        self.latent_tokens = nn.Parameter(scale * torch.randn(self.num_latent_tokens, self.encoder.width))
        self.apply(self._init_weights)
        # created AFTER the initialisation pass, as in the reference (train_tatitok.py:48-54): the codebook keeps its uniform init
        self.quantize = VectorQuantizer(codebook_size=config.codebook_size, token_size=config.latent_dim, commitment_cost=0.25,
                                        use_l2_norm=config.use_l2_norm)

    def _init_weights(self, module):
        """truncated normal (std 0.02) for Linear / Conv / Embedding weights, zero biases, unit LayerNorms (train_tatitok.py:56-69)"""
        if isinstance(module, (nn.Linear, nn.Conv1d, nn.Conv2d)):
            nn.init.trunc_normal_(module.weight.data, mean=0.0, std=0.02)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            nn.init.trunc_normal_(module.weight.data, mean=0.0, std=0.02)
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    def encode(self, x):
        """images [B, 3, H, W] -> (z_quantized [B, C, 1, N], {"min_encoding_indices" [B, 1, N], "quantizer_loss", ...})"""
        z = self.encoder(pixel_values=x, latent_tokens=self.latent_tokens)
        return self.quantize(z)

    def decode(self, z_quantized):
        return self.decoder(z_quantized)

    def decode_tokens(self, tokens):
        """code ids [B, 1, N] or [B, N] -> frames [B, 3, H, W]"""
        tokens = tokens.squeeze(1)
        batch, seq_len = tokens.shape
        z_quantized = self.quantize.get_codebook_entry(tokens.reshape(-1)).reshape(batch, 1, seq_len, -1)
        return self.decode(z_quantized.permute(0, 3, 1, 2).contiguous())          # 'b h w c -> b c h w'

    def forward(self, x):
        """-> (decoded [B, 3, H, W], result_dict)"""
        z_quantized, result_dict = self.encode(x)
        return self.decode(z_quantized), result_dict

    def _fused_quantiser(self):
        q = self.quantize
        return q.use_l2_norm and q.commitment_cost == 0.25 and not q.clustering_vq and q.token_size <= ops.VQ_MAX_D

    def loss(self, x, return_recon=False):
        """-> (reconstruction loss mse(decoded, x), quantiser loss, code ids [B, 1, N][, decoded]) on the fused route: encoder ->
        tokenizer.vq_quantize(unit_codes=True) -> decoder.features -> tokenizer.linear_conv_recon_mse on the parameters of `ffn` and
        `conv_out`.  return_recon: the decoded image as a differentiable fourth result (a perceptual term's gradient joins the pixel
        loss's inside the backward kernel).  A quantiser the kernels do not cover (use_l2_norm=False) runs as in forward()."""
        target = x
        if isinstance(x, Frames):      # uint8 frames: the encoder's patch rows and the fp32 target come out of one launch
            target = x.materialise(self.encoder.patch_size, image=True).images()
        z = self.encoder(pixel_values=x, latent_tokens=self.latent_tokens)                 # [B, C, 1, N]
        if self._fused_quantiser():
            q, ids, qloss = tokenizer.vq_quantize(z.float().permute(0, 2, 3, 1), self.quantize.embedding.weight, unit_codes=True)
            z_quantized = q.permute(0, 3, 1, 2).contiguous()
        else:
            z_quantized, info = self.quantize(z)
            ids, qloss = info["min_encoding_indices"], info["quantizer_loss"]
        dec = self.decoder
        out = tokenizer.linear_conv_recon_mse(dec.features(z_quantized), dec.ffn[0].weight, dec.ffn[0].bias, dec.conv_out.weight,
                                              dec.conv_out.bias, target, dec.grid_size, dec.patch_size, return_recon=return_recon)
        if return_recon:
            return out[0], qloss, ids, out[1]
        return out, qloss, ids


NO_DECAY_NAMES = ("ln", "bias", "latent_tokens", "mask_token", "embedding", "norm", "gamma", "embed")


def param_groups(model, weight_decay):
    """the reference's two groups (train_tatitok.py:95-107): vectors and every parameter whose name contains one of NO_DECAY_NAMES get
    no weight decay"""
    no_decay = lambda n, p: p.ndim < 2 or any(t in n for t in NO_DECAY_NAMES)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    return [{"params": [p for n, p in named if no_decay(n, p)], "weight_decay": 0.0},
            {"params": [p for n, p in named if not no_decay(n, p)], "weight_decay": weight_decay}]


def make_optim(model, args):
    """AdamW over the reference's two parameter groups.  With max_grad_norm (default 1.0, the reference's clip_grad_norm_ BEFORE the
    step, train_tatitok.py:198): vitamd.optim.AdamW, which clips on the device inside the step; without: torch.optim.AdamW."""
    groups = param_groups(model, args.weight_decay)
    max_grad_norm = getattr(args, "max_grad_norm", 1.0)
    if max_grad_norm is None or max_grad_norm <= 0:
        return torch.optim.AdamW(groups, lr=args.lr, betas=(0.9, 0.999))
    from vitamd.optim import AdamW
    return AdamW(groups, lr=args.lr, betas=(0.9, 0.999), max_grad_norm=max_grad_norm)


FUSED_ROUTE = True          # train_step's route: model.loss (the fused quantiser and pixel tail); False = model.forward on the present operators


def train_step(model, images, optim, lr_sched=None, perceptual=None, perceptual_weight=1.1):
    """One iteration of the reference hot loop (train_tatitok.py:185-202) without the fp16 scaler: loss = mse(decoded, images)
    [+ perceptual_weight * perceptual(decoded, images).mean()] + quantiser loss.  perceptual: a callable (recon, images) -> a loss or
    per-image values (vitamd.perceptual.PerceptualLoss fits); with one the step calls model.loss(images, return_recon=True) and stays
    on the fused tail.  Gradient clipping is the optimiser's (make_optim).  -> the detached device loss"""
    optim.zero_grad(set_to_none=True)
    target = images.images() if isinstance(images, Frames) and (perceptual is not None or not FUSED_ROUTE) else images
    if not FUSED_ROUTE:
        recon, info = model(images)
        recon_loss, qloss = torch.nn.functional.mse_loss(recon, target), info["quantizer_loss"]
    elif perceptual is None:
        recon_loss, qloss, _ = model.loss(images)
        recon = None
    else:
        recon_loss, qloss, _, recon = model.loss(images, return_recon=True)
    if perceptual is not None:
        recon_loss = recon_loss + perceptual_weight * perceptual(recon, target).mean()
    loss = recon_loss + qloss
    loss.backward()
    optim.step()
    if lr_sched is not None:
        lr_sched.step()
    return loss.detach()


def evaluate(model, batches, recon=None, codes=None):
    """The validation half of the loop: vitamd.metrics.evaluate_tokenizer on model(x) = (decoded, result_dict), ids = result_dict["min_encoding_indices"] ->
    {"mse", "mae", "psnr", "ssim", "count", "usage", "used", "dead", "perplexity", "entropy", "codes", "bad"}, one host read at the end"""
    from vitamd.metrics import evaluate_tokenizer
    return evaluate_tokenizer(model, batches, recon=recon, codes=codes, patch=model.encoder.patch_size)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="1D TiTok (train_tatitok) training on synthetic images (MI355X-native path)")
    p.add_argument("--image_size", type=int, default=256)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--latent_tokens", type=int, default=256)
    p.add_argument("--codebook_size", type=int, default=16384)
    p.add_argument("--latent_dim", type=int, default=12)
    p.add_argument("--transformer", type=str, default="small")
    p.add_argument("--bs", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--warmup_steps", type=int, default=10000)
    p.add_argument("--train_steps", type=int, default=50)
    p.add_argument("--max_grad_norm", type=float, default=1.0,
                   help="clip the global gradient norm on the device before the update (vitamd.optim.AdamW); 0 = no clipping, torch.optim.AdamW")
    p.add_argument("--perceptual_weight", type=float, default=0.0,
                   help="weight of the ConvNeXt-S perceptual term (the reference uses 1.1); 0 = no perceptual term")
    p.add_argument("--perceptual_weights", type=str, default=None,
                   help="path of a torchvision convnext_small state dict for the perceptual network; without it the network is untrained "
                        "(a throughput stand-in).  Nothing is ever downloaded")
    p.add_argument("--eval_every", type=int, default=0,
                   help="evaluate every N training steps on seeded held-out random data (evaluate / vitamd.metrics: MSE, MAE, PSNR, SSIM and codebook usage "
                        "from counters on the device, one host read per evaluation); 0 = never")
    p.add_argument("--eval_batches", type=int, default=2, help="the batches of one evaluation (--eval_every)")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.eval_every < 0 or (args.eval_every > 0 and args.eval_batches < 1):
        raise SystemExit("--eval_every needs N >= 0 and --eval_batches >= 1")
    dev = torch.device("cuda")
    cfg = TiTokConfig(args.image_size, args.patch_size, args.latent_tokens, args.codebook_size, args.latent_dim, args.transformer)
    model = TiTok(cfg).to(dev)
    optim = make_optim(model, args)
    sched = get_lr_scheduler(optim, args.warmup_steps, args.train_steps, args.lr / 10)
    perceptual = None
    if args.perceptual_weight > 0:
        from vitamd.perceptual import PerceptualLoss
        perceptual = PerceptualLoss("convnext_s", weights=args.perceptual_weights).to(dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    images = torch.rand((args.bs, 3, args.image_size, args.image_size), generator=g).to(dev)
    usage = torch.zeros([cfg.codebook_size], device=dev)
    val = make_val_batches(args, dev) if args.eval_every > 0 else None
    for step in range(args.train_steps):
        t0 = time.time()
        loss = train_step(model, images, optim, sched, perceptual=perceptual, perceptual_weight=args.perceptual_weight)
        with torch.no_grad():
            usage[model.encode(images)[1]["min_encoding_indices"].flatten()] = 1
        torch.cuda.synchronize()
        print(f"step {step} loss {loss.item():.4f} codebook_usage {usage.sum().item() / cfg.codebook_size:.3f} "
              f"{args.bs / (time.time() - t0):.1f} images/s")
        if val is not None and (step + 1) % args.eval_every == 0:
            report(step, evaluate(model, val))


if __name__ == "__main__":
    main()
