"""MI355X-native drop-in for the model half of the reference's `train_enhancing_vitvqgan` module (reference
train_enhancing_vitvqgan.py:20-272): ViTVQGANConfig, get_2d_sincos_pos_embed, init_weights, PreNorm, FeedForward, Attention, Transformer,
ViTEncoder, ViTDecoder, Quantizer, ViTVQGAN with the same constructor signatures and defaults, state_dict keys (`to_patch_embedding.0`,
`layers.{i}.0.fn.to_qkv`, `layers.{i}.1.fn.net.0` / `net.2`, `to_pixel.1`, ...), initialisation rule and fixed sincos position tables
(`requires_grad=False` parameters).  The modules are parameter containers; forward and backward run on libvitamd kernels (DESIGN.md
section 19): patch-embed GEMM with the position table in its epilogue, affine LayerNorm, fused-QKV attention with its out-projection
(block_functions.AttnProjFn, no QKV bias), the tanh MLP (vitamd.enhancing.tanh_mlp), padded-Linear GEMMs for the two narrow projections,
tokenizer.vq_quantize, and the ConvTranspose2d head as a Linear followed by the (c p1 p2) depatchify - in loss() fused with the L1 pixel
term (vitamd.enhancing.linear_recon_l1).

Differences from the reference, stated:
  - dim_head must be 64 and heads * dim_head must equal dim (the attention kernels and AttnProjFn are built for that): anything else,
    the `heads == 1 and dim_head == dim` form without an out-projection included, raises NotImplementedError;
  - image and patch sizes may be given as pairs, but the grid and the patch must be square (NotImplementedError otherwise);
  - ViTVQGAN ignores `config.transformer` as the reference does (always 768 / 12 / 12 / 3072) and accepts keyword-only
    `dim, depth, heads, mlp_dim` to build another size;
  - the reference's loop calls clip_grad_norm_ AFTER optim.step() (train_enhancing_vitvqgan.py:338-340), where the clip changes no
    update; train_step does not clip;
  - uint8 vitamd.data.Frames are accepted by forward() / loss() / train_step where the sibling tokenizers accept them (the same helper
    calls).
"""
import argparse
import time
from dataclasses import dataclass
from typing import Tuple, Union

import numpy as np
import torch
import torch.nn as nn
from einops.layers.torch import Rearrange

from train_vit import ViTConfig
from train_titok import make_val_batches, report
from utils import get_lr_scheduler
from vitamd import enhancing, tokenizer
from vitamd.block_functions import AttnProjFn, LayerNormAffineFn
from vitamd.data import Frames
from vitamd.functions import PatchEmbedFn, linear


@dataclass
class ViTVQGANConfig:
    image_size: int
    patch_size: int
    codebook_size: int
    latent_dim: int
    transformer: str

    def __post_init__(self):
        self.patch_dim = self.image_size // self.patch_size
        self.n_patches = self.patch_dim ** 2
        self.latent_tokens = self.n_patches
        self.enc_vit_config = ViTConfig(self.image_size, 3, self.patch_size, self.transformer, 0, 0.0)
        self.n_embd = self.enc_vit_config.trans_config.n_embd
        self.dec_vit_config = ViTConfig(self.latent_tokens, self.n_embd, 1, self.transformer, 0, 0.0)
        self.dec_vit_config.n_patches = self.latent_tokens


# ------------------------------------------------------------------------------------------------ position tables, initialisation
def get_1d_sincos_pos_embed_from_grid(embed_dim, pos):
    """positions (any shape, flattened to M) -> [M, embed_dim] float64: sin of pos / 10000^(2i/embed_dim) in the first half, cos in the second"""
    if embed_dim % 2:
        raise ValueError("embed_dim must be even")
    omega = 1.0 / 10000 ** (np.arange(embed_dim // 2, dtype=float) / (embed_dim / 2.0))
    angle = np.einsum("m,d->md", np.asarray(pos).reshape(-1), omega)
    return np.concatenate([np.sin(angle), np.cos(angle)], axis=1)


def get_2d_sincos_pos_embed_from_grid(embed_dim, grid):
    """grid [2, 1, H, W] (plane 0 = column index, plane 1 = row index) -> [H*W, embed_dim]: each plane takes half of the channels"""
    if embed_dim % 2:
        raise ValueError("embed_dim must be even")
    return np.concatenate([get_1d_sincos_pos_embed_from_grid(embed_dim // 2, grid[0]),
                           get_1d_sincos_pos_embed_from_grid(embed_dim // 2, grid[1])], axis=1)


def get_2d_sincos_pos_embed(embed_dim, grid_size):
    """grid_size: int or (height, width) -> numpy [height*width, embed_dim], rows in (h w) order; the column index is encoded first"""
    gh, gw = grid_size if isinstance(grid_size, tuple) else (grid_size, grid_size)
    cols, rows = np.meshgrid(np.arange(gw, dtype=np.float32), np.arange(gh, dtype=np.float32))
    return get_2d_sincos_pos_embed_from_grid(embed_dim, np.stack([cols, rows], axis=0).reshape(2, 1, gh, gw))


def init_weights(m):
    """Linear: Xavier-uniform weight, zero bias; LayerNorm: unit weight, zero bias; Conv2d / ConvTranspose2d: Xavier-uniform on the weight
    viewed [out, -1] (the bias keeps torch's default)"""
    if isinstance(m, nn.Linear):
        nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)
    elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
        w = m.weight.data
        nn.init.xavier_uniform_(w.view([w.shape[0], -1]))


FUSED_ROUTE = True          # the tanh MLP and train_step's pixel term on vitamd.enhancing; False = functions.linear + torch.tanh and forward() + abs().mean()
                            # on the same GEMMs (the comparison route of tools/bench_enhancing.py)


def _ln(mod, x):
    return LayerNormAffineFn.apply(x.contiguous(), mod.weight, mod.bias, mod.eps)


def _pair(v):
    return v if isinstance(v, tuple) else (v, v)


# ------------------------------------------------------------------------------------------------ layers
class PreNorm(nn.Module):
    def __init__(self, dim: int, fn: nn.Module) -> None:
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn

    def forward(self, x, **kwargs):
        return self.fn(_ln(self.norm, x), **kwargs)


class FeedForward(nn.Module):
    """Linear -> Tanh -> Linear; `net` holds the parameters under the reference's indices 0 and 2"""

    def __init__(self, dim: int, hidden_dim: int) -> None:
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.Tanh(), nn.Linear(hidden_dim, dim))

    def forward(self, x):
        fc1, fc2 = self.net[0], self.net[2]
        if not FUSED_ROUTE:
            return linear(torch.tanh(linear(x, fc1.weight, fc1.bias)), fc2.weight, fc2.bias)
        return enhancing.tanh_mlp(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias)


class Attention(nn.Module):
    """to_qkv (no bias) -> softmax(q k^T / sqrt(dim_head)) v -> to_out (bias).  dim_head must be 64 and heads * dim_head == dim; the
    reference's `heads == 1 and dim_head == dim` form (no out-projection) is refused with the rest: NotImplementedError."""

    def __init__(self, dim: int, heads: int = 8, dim_head: int = 64) -> None:
        super().__init__()
        if dim_head != 64:
            raise NotImplementedError("the attention kernels are built for head_dim 64")
        if heads * dim_head != dim:
            raise NotImplementedError(f"heads * dim_head must equal dim ({heads} * {dim_head} != {dim}): the fused attention block has no other form")
        inner_dim = dim_head * heads
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.attend = nn.Softmax(dim=-1)
        self.to_qkv = nn.Linear(dim, inner_dim * 3, bias=False)
        self.to_out = nn.Linear(inner_dim, dim)

    def forward(self, x):
        return AttnProjFn.apply(x, self.to_qkv.weight, None, self.to_out.weight, self.to_out.bias, self.heads)


class Transformer(nn.Module):
    def __init__(self, dim: int, depth: int, heads: int, dim_head: int, mlp_dim: int) -> None:
        super().__init__()
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head)),
                                              PreNorm(dim, FeedForward(dim, mlp_dim))]))
        self.norm = nn.LayerNorm(dim)

    def forward(self, x):
        for attn, ff in self.layers:
            x = attn(x) + x
            x = ff(x) + x
        return _ln(self.norm, x)


def _square_grid(image_size, patch_size):
    (ih, iw), (ph, pw) = _pair(image_size), _pair(patch_size)
    assert ih % ph == 0 and iw % pw == 0, "Image dimensions must be divisible by the patch size."
    if ph != pw or ih != iw:
        raise NotImplementedError("the patch-embed and pixel-tail kernels are built for square patches on a square grid")
    return ih // ph, ph


class ViTEncoder(nn.Module):
    def __init__(self, image_size: Union[Tuple[int, int], int], patch_size: Union[Tuple[int, int], int],
                 dim: int = 768, depth: int = 12, heads: int = 12, mlp_dim: int = 3072, channels: int = 3, dim_head: int = 64) -> None:
        super().__init__()
        self.grid, self.patch = _square_grid(image_size, patch_size)
        self.num_patches = self.grid * self.grid
        self.patch_dim = channels * self.patch * self.patch
        self.to_patch_embedding = nn.Sequential(
            nn.Conv2d(channels, dim, kernel_size=patch_size, stride=patch_size),
            Rearrange("b c h w -> b (h w) c"),
        )
        table = get_2d_sincos_pos_embed(dim, (self.grid, self.grid))
        self.en_pos_embedding = nn.Parameter(torch.from_numpy(table).float().unsqueeze(0), requires_grad=False)
        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim)
        self.apply(init_weights)

    def forward(self, img):
        conv = self.to_patch_embedding[0]
        pos = self.en_pos_embedding[0]
        x = PatchEmbedFn.apply(img, conv.weight, conv.bias, pos, pos.new_zeros((0, pos.shape[1])), self.patch, self.num_patches)
        return self.transformer(x)


class ViTDecoder(nn.Module):
    def __init__(self, image_size: Union[Tuple[int, int], int], patch_size: Union[Tuple[int, int], int],
                 dim: int = 768, depth: int = 12, heads: int = 12, mlp_dim: int = 3072, channels: int = 3, dim_head: int = 64) -> None:
        super().__init__()
        self.grid, self.patch = _square_grid(image_size, patch_size)
        self.num_patches = self.grid * self.grid
        self.patch_dim = channels * self.patch * self.patch
        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim)
        table = get_2d_sincos_pos_embed(dim, (self.grid, self.grid))
        self.de_pos_embedding = nn.Parameter(torch.from_numpy(table).float().unsqueeze(0), requires_grad=False)
        self.to_pixel = nn.Sequential(
            Rearrange("b (h w) c -> b c h w", h=self.grid),
            nn.ConvTranspose2d(dim, channels, kernel_size=patch_size, stride=patch_size),
        )
        self.apply(init_weights)

    def features(self, token):
        """tokens [B, grid*grid, dim] -> the stack's output rows, what the pixel head (`to_pixel.1`) is applied to"""
        return self.transformer(token + self.de_pos_embedding)

    def forward(self, token):
        convt = self.to_pixel[1]
        dim, pp = convt.weight.shape[0], self.patch * self.patch
        # ConvTranspose2d(kernel = stride): a Linear whose [out, in] weight is the layer's [dim, c*p*p] transposed, then the (c p1 p2) depatchify
        y = linear(self.features(token), convt.weight.reshape(dim, -1).t(), None if convt.bias is None else convt.bias.repeat_interleave(pp))
        return enhancing.conv_shuffle_tokens(y, self.grid, self.patch)

    def get_last_layer(self) -> nn.Parameter:
        return self.to_pixel[-1].weight


class Quantizer(nn.Module):
    def __init__(self, config: ViTVQGANConfig):
        super().__init__()
        self.codebook = nn.Embedding(config.codebook_size, config.latent_dim)
        self.codebook.weight.data.uniform_(-1.0 / config.codebook_size, 1.0 / config.codebook_size)

    def forward(self, x):
        """-> (quantized, indices, quantize_loss): the search on normalised rows, the RAW codebook rows picked, both loss terms against the
        normalised latents, straight-through - tokenizer.vq_quantize expression for expression"""
        return tokenizer.vq_quantize(x.float(), self.codebook.weight)


class ViTVQGAN(nn.Module):
    def __init__(self, config: ViTVQGANConfig, *, dim: int = 768, depth: int = 12, heads: int = 12, mlp_dim: int = 3072):
        super().__init__()
        self.config = config
        kw = dict(dim=dim, depth=depth, heads=heads, mlp_dim=mlp_dim)
        self.encoder = ViTEncoder(config.image_size, config.patch_size, **kw)
        self.pre_quant_proj = nn.Linear(dim, config.latent_dim)
        self.quant = Quantizer(config)
        self.quant_proj = nn.Linear(config.latent_dim, dim)
        self.decoder = ViTDecoder(config.image_size, config.patch_size, **kw)

    def _latents(self, x):
        return linear(self.encoder(x), self.pre_quant_proj.weight, self.pre_quant_proj.bias)

    def _features(self, x):
        quantized, indices, quantize_loss = self.quant(self._latents(x))
        h = self.decoder.features(linear(quantized, self.quant_proj.weight, self.quant_proj.bias))
        return h, indices, quantize_loss

    def encode(self, z):
        return self.quant(self._latents(z))[1]

    def decode(self, z_quant):
        return self.decoder(z_quant)

    def decode_indices(self, indices):
        return self.decoder(self.quant.codebook(indices))

    def forward(self, x):
        """-> (image_recon [B, 3, H, W], indices [B, n_patches], quantize_loss).  As the reference's forward, the decoder sees the quantised
        latents through quant_proj; decode() / decode_indices() hand their argument to the decoder as it is, as the reference does."""
        quantized, indices, quantize_loss = self.quant(self._latents(x))
        return self.decoder(linear(quantized, self.quant_proj.weight, self.quant_proj.bias)), indices, quantize_loss

    def loss(self, x, return_recon=False):
        """-> (recon_loss = mean |recon - x|, quantize_loss, indices[, recon]) on the fused tail: the head GEMM writes bf16 tokens once, the
        L1 kernel reads them (and with return_recon hands out the image, differentiable, for a perceptual term), the backward overwrites
        them with their gradient.  x: fp32 images or uint8 vitamd.data.Frames."""
        target = x.materialise(self.encoder.patch, image=True).images() if isinstance(x, Frames) else x
        h, indices, quantize_loss = self._features(x)
        convt = self.decoder.to_pixel[1]
        out = enhancing.linear_recon_l1(h, convt.weight, convt.bias, target, self.decoder.grid, self.decoder.patch, return_recon=return_recon)
        if return_recon:
            return out[0], quantize_loss, indices, out[1]
        return out, quantize_loss, indices

    def get_last_layer(self) -> nn.Parameter:
        return self.decoder.get_last_layer()


# ------------------------------------------------------------------------------------------------ the loop
def train_step(model, images, optim, lr_sched=None, perceptual=None, perceptual_weight=1.0):
    """One iteration of the reference hot loop (train_enhancing_vitvqgan.py:330-341) without the fp16 scaler: loss = mean |recon - images|
    [+ perceptual_weight * perceptual(recon, images).mean()] + quantize_loss, on model.loss.  perceptual: a callable (recon, images) -> a
    loss or per-image values (vitamd.perceptual.PerceptualLoss fits); with one the step asks model.loss for the image and stays on the
    fused tail.  No gradient clipping (see the module docstring).  -> the detached device loss"""
    optim.zero_grad(set_to_none=True)
    target = images.images() if isinstance(images, Frames) and (perceptual is not None or not FUSED_ROUTE) else images
    if not FUSED_ROUTE:
        recon, _, qloss = model(images)
        recon_loss = (recon - target).abs().mean()
    elif perceptual is None:
        recon_loss, qloss, _ = model.loss(images)
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
    """The validation half of the loop: vitamd.metrics.evaluate_tokenizer on model(x) = (image_recon, indices, quantize_loss) ->
    {"mse", "mae", "psnr", "ssim", "count", "usage", "used", "dead", "perplexity", "entropy", "codes", "bad"}, one host read at the end"""
    from vitamd.metrics import evaluate_tokenizer
    return evaluate_tokenizer(model, batches, recon=recon, codes=codes, patch=model.encoder.patch)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Enhancing ViT-VQGAN training on synthetic images (MI355X-native path)")
    p.add_argument("--image_size", type=int, default=128)
    p.add_argument("--patch_size", type=int, default=16)
    p.add_argument("--latent_tokens", type=int, default=256)
    p.add_argument("--codebook_size", type=int, default=2048)
    p.add_argument("--latent_dim", type=int, default=12)
    p.add_argument("--transformer", type=str, default="B")
    p.add_argument("--bs", type=int, default=32)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=1e-4)
    p.add_argument("--warmup_steps", type=int, default=10000)
    p.add_argument("--train_steps", type=int, default=20, help="seeded steps to run (the reference's default is 500 000 on ImageNet)")
    p.add_argument("--perceptual_weight", type=float, default=0.0,
                   help="weight of the ConvNeXt-S perceptual term (the reference adds it with weight 1); 0 = no perceptual term")
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
    cfg = ViTVQGANConfig(args.image_size, args.patch_size, args.codebook_size, args.latent_dim, args.transformer)
    torch.manual_seed(0)
    model = ViTVQGAN(cfg).to(dev)
    optim = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
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
            usage[model.encode(images)] = 1
        torch.cuda.synchronize()
        print(f"step {step} loss {loss.item():.4f} codebook_usage {usage.sum().item() / cfg.codebook_size:.3f} "
              f"{args.bs / (time.time() - t0):.1f} images/s")
        if val is not None and (step + 1) % args.eval_every == 0:
            report(step, evaluate(model, val))


if __name__ == "__main__":
    main()
