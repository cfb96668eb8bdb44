"""The perceptual term of the tokenizers' objective (reference perceptual_loss.py, used at train_titok.py:155-158 and the same lines of
train_vit_vqgan.py): mse_loss between the ImageNet logits a frozen ConvNeXt-S gives the reconstruction and the target image, on this
library's kernels.

The network is restated from its published structure (torchvision.models.convnext_small; torchvision is not a dependency): the state
dict keeps torchvision's keys under the prefix `convnext.`, so a `convnext_small` checkpoint loads.  No weights are shipped and none are
ever fetched: `weights=None` gives torchvision's initialisation, a throughput stand-in and not a perceptual metric.

The network is frozen, so one autograd node with a hand-written backward carries the whole thing: forward of both images, backward to the
reconstruction only, no weight gradients.  Activations are channels-last rows [B*H*W, C] - the layout the GEMMs and the row LayerNorm
want - so torchvision's two Permutes per block vanish."""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

from . import ops
from .functions import _amp_fwd, _amp_bwd

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
LN_EPS = 1e-6            # every LayerNorm of ConvNeXt
PREFIX = "convnext."


# ------------------------------------------------------------------------------------------ the resize tables
def resize_matrix(n_in, n_out):
    """float64 [n_out, n_in]: one axis of F.interpolate(mode="bilinear", align_corners=False, antialias=True) as a matrix.  scale =
    n_in / n_out, support = max(scale, 1), centre = (o + 0.5) scale; taps j in [max(int(centre - support + 0.5), 0), min(int(centre +
    support + 0.5), n_in)) weigh max(0, 1 - |(j - centre + 0.5) / support|), normalised to sum 1 per output."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    m = torch.zeros((n_out, n_in), dtype=F64)
    for o in range(n_out):
        centre = (o + 0.5) * scale
        lo, hi = max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n_in)
        j = torch.arange(lo, hi, dtype=F64)
        w = (1.0 - ((j - centre + 0.5) / support).abs()).clamp_min(0.0)
        m[o, lo:hi] = w / w.sum()
    return m


def band(m):
    """a matrix whose rows hold one run of non-zeros -> (start int32 [rows], taps fp32 [rows, T]): T = the longest run, taps[r] =
    m[r, start[r] : start[r] + T] with start[r] + T <= columns (runs near the end are shifted back and keep their zeros in front)"""
    rows, cols = m.shape
    nz = m != 0
    any_nz = nz.any(dim=1)
    idx = torch.arange(cols)
    lo = torch.where(nz, idx, torch.full_like(idx, cols)).min(dim=1).values
    hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).max(dim=1).values
    lo = torch.where(any_nz, lo, torch.zeros_like(lo))
    T = max(int((hi - lo).max()), 1)
    start = torch.minimum(lo, torch.full_like(lo, cols - T))
    taps = torch.gather(m, 1, start[:, None] + torch.arange(T)[None, :])
    assert float((taps.sum(1) - m.sum(1)).abs().max()) < 1e-12            # the band holds every non-zero of its row
    return start.to(torch.int32), taps.to(F32)


_TABLES = {}


def band_tables(n_in, n_out, device):
    """-> ((start, taps) of the resize matrix [n_out, n_in], (start, taps) of its transpose), on `device`; built once per key"""
    key = (n_in, n_out, str(device))
    t = _TABLES.get(key)
    if t is None:
        m = resize_matrix(n_in, n_out)
        t = _TABLES[key] = tuple(tuple(x.to(device).contiguous() for x in band(mm)) for mm in (m, m.t().contiguous()))
    return t


# ------------------------------------------------------------------------------------------ the module (torchvision's key layout)
class _Affine(nn.Module):
    """a parameter holder with torchvision's names: weight (and bias)"""

    def __init__(self, wshape, bshape):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(wshape), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(bshape), requires_grad=False)


class _CNBlock(nn.Module):
    """block.0 depthwise 7x7, block.2 LayerNorm, block.3 Linear(d, 4d) + GELU, block.5 Linear(4d, d), layer_scale [d,1,1]"""

    def __init__(self, d):
        super().__init__()
        self.block = nn.ModuleList([_Affine((d, 1, 7, 7), (d,)), nn.Identity(), _Affine((d,), (d,)), _Affine((4 * d, d), (4 * d,)),
                                    nn.Identity(), _Affine((d, 4 * d), (d,))])
        self.layer_scale = nn.Parameter(torch.empty((d, 1, 1)), requires_grad=False)


def _pad_k(t):
    """bf16 [M, K] -> [M, K rounded up to 64] with zero columns: the GEMM contract K % 64 == 0 (only ConvNeXt's 96 and the test widths
    break it; a copy, as functions.LinearFn makes)"""
    pad = -t.shape[1] % 64
    return t if pad == 0 else torch.nn.functional.pad(t, (0, pad))


class PerceptualLoss(nn.Module):
    """Drop-in for the reference's perceptual_loss.PerceptualLoss: forward(input, target) -> 0-dim fp32 mse_loss(logits(input),
    logits(target)), images [B, 3, H, W] fp32 in [0, 1].  Always in eval mode, every parameter frozen; the gradient flows to `input` only.

    weights: None (torchvision's initialisation; warns), a path for torch.load(..., weights_only=True), or a state dict with or without
    the `convnext.` prefix.  depths / dims / num_classes / size exist so tests can build a small network."""

    def __init__(self, model_name="convnext_s", weights=None, *, depths=(3, 3, 27, 3), dims=(96, 192, 384, 768), num_classes=1000, size=224):
        super().__init__()
        if "convnext_s" not in model_name:
            raise ValueError(f"Unsupported Perceptual Loss model name {model_name}")
        if size < 32 or size % 32 != 0:
            raise ValueError(f"PerceptualLoss: size must be a positive multiple of 32 (the network strides by 32), got {size}")
        if len(depths) != 4 or len(dims) != 4 or any(d % 4 for d in dims) or num_classes % 4:
            raise ValueError("PerceptualLoss: four stages, widths and class count multiples of 4")
        self.depths, self.dims, self.num_classes, self.size = tuple(depths), tuple(dims), num_classes, size
        feats = [nn.ModuleList([_Affine((dims[0], 3, 4, 4), (dims[0],)), _Affine((dims[0],), (dims[0],))])]
        for s in range(4):
            feats.append(nn.ModuleList([_CNBlock(dims[s]) for _ in range(depths[s])]))
            if s < 3:
                feats.append(nn.ModuleList([_Affine((dims[s],), (dims[s],)), _Affine((dims[s + 1], dims[s], 2, 2), (dims[s + 1],))]))
        self.convnext = nn.Module()
        self.convnext.features = nn.ModuleList(feats)
        self.convnext.classifier = nn.ModuleList([_Affine((dims[3],), (dims[3],)), nn.Identity(), _Affine((num_classes, dims[3]), (num_classes,))])
        self.register_buffer("imagenet_mean", torch.tensor(IMAGENET_MEAN)[None, :, None, None])
        self.register_buffer("imagenet_std", torch.tensor(IMAGENET_STD)[None, :, None, None])
        self._prep = None
        self._init_weights()
        if weights is None:
            warnings.warn("PerceptualLoss: no weights given - an untrained ConvNeXt-S is a throughput stand-in, not a perceptual metric "
                          "(pass weights=<a torchvision convnext_small state dict or its path>)")
        else:
            sd = torch.load(weights, map_location="cpu", weights_only=True) if not isinstance(weights, dict) else weights
            self.load_state_dict(sd)
        self.eval()

    def _init_weights(self):
        """torchvision: trunc-normal std 0.02 on conv and Linear weights, zero biases, layer_scale 1e-6, LayerNorm 1 / 0"""
        for name, p in self.named_parameters():
            if name.endswith("layer_scale"):
                nn.init.constant_(p, 1e-6)
            elif name.endswith("bias"):
                nn.init.zeros_(p)
            elif p.dim() == 1:
                nn.init.ones_(p)
            else:
                nn.init.trunc_normal_(p, std=0.02)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """accepts torchvision's own keys (`features.0.0.weight`) as well as the reference module's (`convnext.features.0.0.weight`)"""
        if not any(k.startswith(PREFIX) for k in state_dict):
            state_dict = {(k if k.startswith("imagenet_") else PREFIX + k): v for k, v in state_dict.items()}
        state_dict = dict(state_dict)
        for k in ("imagenet_mean", "imagenet_std"):                # constants: a bare network checkpoint does not carry them
            state_dict.setdefault(k, getattr(self, k))
        self._prep = None
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _apply(self, fn, recurse=True):
        self._prep = None
        return super()._apply(fn, recurse)

    def train(self, mode=True):
        return super().train(False)               # always in eval mode (perceptual_loss.py:59)

    # -------------------------------------------------------------------------------------- the frozen operands, built once
    def prepared(self):
        """The operands of the kernels, derived from the parameters ONCE (not per step, and not through functions.WEIGHTS, whose copies
        follow the optimiser's epoch): bf16 weights, their transposes for the input-gradient GEMMs, both zero-padded along K to a multiple
        of 64; layer_scale folded into fc2 in fp32 before the cast (W2' = diag(ls) W2, b2' = ls b2: the residual add is then the stock
        EPI_RESID_F32 epilogue and the backward needs no extra multiply); the 2x2 weights with their columns in (kh, kw, c) order, the
        order of the 2x2 gather on channels-last rows.  Rebuilt after load_state_dict / .to()."""
        dev = self.imagenet_mean.device
        if self._prep is not None and self._prep["device"] == dev:
            return self._prep
        f = self.convnext.features

        def lin(w):                                # fp32 [N, K] -> (bf16 [N, K64], bf16 [K, N64]): forward operand, input-gradient operand
            w = w.detach().to(F32)
            return _pad_k(w.to(BF16)).contiguous(), _pad_k(w.t().to(BF16)).contiguous()

        def vec(p):
            return p.detach().to(F32).contiguous()

        def zrow(n):                               # the zero "position" row of the EPI_PATCH_F32 epilogue (fp32 out = bf16(acc + bias) + 0)
            return torch.zeros((1, n), dtype=F32, device=dev)

        d = self.dims
        w, wt = lin(f[0][0].weight.reshape(d[0], 48))
        prep = {"device": dev, "mean": vec(self.imagenet_mean).view(3), "std": vec(self.imagenet_std).view(3),
                "stem": {"w": w, "wt": wt, "b": vec(f[0][0].bias), "z": zrow(d[0]), "g": vec(f[0][1].weight), "be": vec(f[0][1].bias)},
                "stages": [], "down": [], "scratch": {}}
        for s in range(4):
            blocks = []
            for blk in f[2 * s + 1]:
                b = blk.block
                ls = blk.layer_scale.detach().to(F32).view(-1)
                w1, w1t = lin(b[3].weight)
                w2, w2t = lin(ls[:, None] * b[5].weight.detach().to(F32))
                blocks.append({"wd": vec(b[0].weight).view(d[s], 7, 7), "bd": vec(b[0].bias), "g": vec(b[2].weight), "be": vec(b[2].bias),
                               "w1": w1, "w1t": w1t, "b1": vec(b[3].bias), "w2": w2, "w2t": w2t, "b2": (ls * b[5].bias.detach().to(F32)).contiguous()})
            prep["stages"].append(blocks)
            if s < 3:
                ds = f[2 * s + 2]
                w, wt = lin(ds[1].weight.detach().permute(0, 2, 3, 1).reshape(d[s + 1], 4 * d[s]))
                prep["down"].append({"g": vec(ds[0].weight), "be": vec(ds[0].bias), "w": w, "wt": wt, "b": vec(ds[1].bias), "z": zrow(d[s + 1])})
        c = self.convnext.classifier
        w, wt = lin(c[2].weight)
        prep["head"] = {"g": vec(c[0].weight), "be": vec(c[0].bias), "w": w, "wt": wt, "b": vec(c[2].bias), "z": zrow(self.num_classes)}
        for n in set(d):                           # where the LayerNorm backward kernels add the (unused) affine gradients: never read
            prep["scratch"][n] = torch.zeros((2, n), dtype=F32, device=dev)
        self._prep = prep
        return prep

    def forward(self, input, target):
        return _PerceptualFn.apply(input, target, self)


# ------------------------------------------------------------------------------------------ the network on rows
def _linear_f32(a, p):
    """fp32 [M, N] = bf16(a . w^T + b): the strided convolutions and the classifier (EPI_PATCH_F32 with one all-zero position row)"""
    return ops.gemm_nt(a, p["w"], ops.EPI_PATCH_F32, bias=p["b"], aux=p["z"], n_patches=1, seq=1, extra=0)


def _gather2x2(y, B, H, W, C):
    """rows [B*H*W, C] -> [B*(H/2)*(W/2), 4C] with columns (kh, kw, c): the operand of the 2x2 stride-2 convolution, a pure permutation"""
    return y.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // 2) * (W // 2), 4 * C)


def _scatter2x2(dy, B, H, W, C):
    """its inverse: [B*(H/2)*(W/2), 4C] -> rows [B*H*W, C]"""
    return dy.view(B, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, C)


def block_fwd(x, p, B, H, W, saved=None):
    """one CNBlock on fp32 rows x [B*H*W, C] -> fp32 rows; saved (a list) receives what the backward needs: the LayerNorm input with its
    mean / rstd and the stored gelu' (bf16 [M, 4C])"""
    C = x.shape[1]
    d = ops.dwconv7_fwd(x.view(B, H, W, C), p["wd"], p["bd"]).view(-1, C)
    y, mean, rstd = ops.layernorm_affine_fwd(d, p["g"], p["be"], LN_EPS)
    dg, h = ops.gemm_nt(_pad_k(y), p["w1"], ops.EPI_GELU_DG, bias=p["b1"])
    out = ops.gemm_nt(h, p["w2"], ops.EPI_RESID_F32, bias=p["b2"], aux=x)
    if saved is not None:
        saved.append((d, mean, rstd, dg))
    return out


def block_bwd(g, p, B, H, W, saved, scratch):
    """gradient of the block output (fp32 rows) -> gradient of its input.  As block_functions.MlpFn's backward without its two weight-
    gradient GEMMs and column sums, then the LayerNorm backward and the transposed depthwise convolution, which adds the residual branch."""
    d, mean, rstd, dg = saved
    C = g.shape[1]
    dh = ops.gemm_nt(_pad_k(ops.cast_bf16(g)), p["w2t"], ops.EPI_DMUL, aux=dg)
    dy = ops.gemm_nt(dh, p["w1t"], ops.EPI_BIAS_BF16)
    gd, _ = ops.layernorm_affine_bwd(dy, d, mean, rstd, p["g"], scratch[0], scratch[1])
    return ops.dwconv7_bwd(gd.view(B, H, W, C), p["wd"], add=g.view(B, H, W, C)).view(-1, C)


def _trunk(prep, rows, B, size, saved=None):
    """bf16 patch rows [B*(size/4)^2, 64] -> fp32 logits [B, classes]"""
    H = W = size // 4
    pre = _linear_f32(rows, prep["stem"])
    x, mean, rstd = ops.layernorm_affine_fwd_f32(pre, prep["stem"]["g"], prep["stem"]["be"], LN_EPS)
    if saved is not None:
        saved.append((pre, mean, rstd))
    for s, blocks in enumerate(prep["stages"]):
        for p in blocks:
            x = block_fwd(x, p, B, H, W, saved)
        if s < 3:
            p = prep["down"][s]
            y, mean, rstd = ops.layernorm_affine_fwd(x, p["g"], p["be"], LN_EPS)
            if saved is not None:
                saved.append((x, mean, rstd))
            x = _linear_f32(_gather2x2(y, B, H, W, x.shape[1]), p)
            H, W = H // 2, W // 2
    pooled = x.view(B, H * W, x.shape[1]).mean(dim=1)              # B x C values: torch device op, like the other O(B) glue
    p = prep["head"]
    y, mean, rstd = ops.layernorm_affine_fwd(pooled, p["g"], p["be"], LN_EPS)
    if saved is not None:
        saved.append((pooled, mean, rstd, H * W))
    return _linear_f32(_pad_k(y), p)


def _trunk_bwd(prep, dlogits, B, size, saved):
    """fp32 dlogits [B, classes] -> fp32 gradient of the patch rows [B*(size/4)^2, 64]; frees each saved entry as it is used"""
    sc = prep["scratch"]
    p = prep["head"]
    pooled, mean, rstd, hw = saved.pop()
    C = pooled.shape[1]
    dy = ops.gemm_nt(_pad_k(ops.cast_bf16(dlogits)), p["wt"], ops.EPI_BIAS_BF16)
    gp, _ = ops.layernorm_affine_bwd(dy, pooled, mean, rstd, p["g"], sc[C][0], sc[C][1])
    g = (gp / hw)[:, None, :].expand(B, hw, C).reshape(B * hw, C)
    H = W = size // 32
    for s in (3, 2, 1, 0):
        if s < 3:
            p = prep["down"][s]
            x, mean, rstd = saved.pop()
            C = x.shape[1]
            da = ops.gemm_nt(_pad_k(ops.cast_bf16(g)), p["wt"], ops.EPI_BIAS_BF16)
            H, W = H * 2, W * 2
            g, _ = ops.layernorm_affine_bwd(_scatter2x2(da, B, H, W, C).contiguous(), x, mean, rstd, p["g"], sc[C][0], sc[C][1])
        for p in reversed(prep["stages"][s]):
            g = block_bwd(g, p, B, H, W, saved.pop(), sc[C])
    pre, mean, rstd = saved.pop()
    p = prep["stem"]
    gpre = ops.layernorm_affine_bwd_f32(g, pre, mean, rstd, p["g"], sc[C][0], sc[C][1])
    return ops.gemm_nt(_pad_k(ops.cast_bf16(gpre)), p["wt"], ops.EPI_F32)


class _PerceptualFn(torch.autograd.Function):
    """the whole loss as one node: forward of both images, backward to `input` only"""

    @staticmethod
    @_amp_fwd
    def forward(ctx, input, target, module):
        if input.dim() != 4 or input.shape[1] != 3 or input.shape != target.shape:
            raise ValueError(f"PerceptualLoss: expected input and target [B, 3, H, W] of one shape, got {tuple(input.shape)} and {tuple(target.shape)}")
        prep = module.prepared()
        size = module.size
        B, _, H, W = input.shape
        th, tw = band_tables(H, size, input.device), band_tables(W, size, input.device)
        need_grad = ctx.needs_input_grad[0]
        saved = [] if need_grad else None
        rows, _ = ops.resize_norm_fwd(input.detach().to(F32).contiguous(), th[0], tw[0], prep["mean"], prep["std"], size)
        li = _trunk(prep, rows, B, size, saved)
        rows, _ = ops.resize_norm_fwd(target.detach().to(F32).contiguous(), th[0], tw[0], prep["mean"], prep["std"], size)
        lt = _trunk(prep, rows, B, size, None)
        del rows
        diff = li - lt
        ctx.state = (prep, saved, diff, (B, H, W, size), (th[1], tw[1]), input.dtype)
        ctx.set_materialize_grads(False)
        return (diff * diff).mean()

    @staticmethod
    @_amp_bwd
    def backward(ctx, gout):
        prep, saved, diff, (B, H, W, size), (th_t, tw_t), dtype = ctx.state
        if gout is None or saved is None:
            return None, None, None
        if not saved:
            raise RuntimeError("PerceptualLoss: backward through the same forward a second time (its saved activations were freed)")
        dlogits = diff * (gout.to(F32) * (2.0 / diff.numel()))
        grows = _trunk_bwd(prep, dlogits, B, size, saved)
        return ops.resize_norm_bwd(grows, th_t, tw_t, prep["std"], B, H, W, size).to(dtype), None, None
