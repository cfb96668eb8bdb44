"""The Enhancing ViT-VQGAN tokenizer on the HIP kernels (train_enhancing_vitvqgan.py, csrc/enhancing.hip): the tanh MLP
of its transformer and the L1 pixel tail of its ConvTranspose2d head.  Attention, LayerNorm and the quantiser of that model are
block_functions.AttnProjFn, block_functions.LayerNormAffineFn and tokenizer.vq_quantize as they are.

    y = enhancing.tanh_mlp(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias)                  # fc1 GEMM -> tanh in place -> fc2 GEMM
    loss = enhancing.recon_l1(tokens, images, grid, patch)                                 # mean |conv_shuffle_tokens(tokens) - images|
    loss, recon = enhancing.linear_recon_l1(h, convt.weight, convt.bias, images, grid, patch, return_recon=True)

The tanh is NOT an epilogue of the fc1 GEMM: it re-reads and re-writes the [M, mlp_dim] bf16 activations once per MLP and direction, and
no GEMM source changes for it (tools/bench_enhancing.py measures that price).
"""
from __future__ import annotations

import torch

from . import ops
from .functions import WEIGHTS, _amp_bwd, _amp_fwd, _f32c, linear
from .lm import _scalar
from .tokenizer import _rows, _zero_scalar, fused_head_applies

BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ the MLP
class TanhMlpFn(torch.autograd.Function):
    """fc2(tanh(fc1(x))) - FeedForward of the reference's train_enhancing_vitvqgan.py.  Saved: bf16(x) and t = tanh(pre); the
    pre-activation is overwritten by t.  The backward is block_functions.MlpFn's with the tanh kernel in place of the stored-derivative
    multiply, and both bias gradients as column sums inside their weight-gradient GEMMs."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x, w1, b1, w2, b2):
        lead, K = x.shape[:-1], x.shape[-1]
        xb = ops.cast_bf16(_f32c(x).reshape(-1, K))
        w1_b, _ = WEIGHTS.get(w1, True)
        w2_b, _ = WEIGHTS.get(w2, True)
        t = ops.gemm_nt(xb, w1_b, ops.EPI_BIAS_BF16, bias=None if b1 is None else _f32c(b1))
        ops.tanh_bf16(t, out=t)
        y = ops.gemm_nt(t, w2_b, ops.EPI_BIAS_BF16, bias=None if b2 is None else _f32c(b2))
        ctx.save_for_backward(xb, t)
        ctx.params = (w1, w2)
        ctx.meta = (lead, K, x.dtype, b1 is not None, b2 is not None)
        return y.view(*lead, w2.shape[0]).to(x.dtype)

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        lead, K, xdtype, has_b1, has_b2 = ctx.meta
        w1, w2 = ctx.params
        xb, t = ctx.saved_tensors
        dev = g.device
        Dh, Dout = t.shape[1], w2.shape[0]
        dy = ops.cast_bf16(_f32c(g).reshape(-1, Dout))
        _, w1_t = WEIGHTS.get(w1, True)
        _, w2_t = WEIGHTS.get(w2, True)
        db2 = torch.zeros((Dout,), dtype=F32, device=dev) if has_b2 else None
        dW2 = torch.empty((Dout, Dh), dtype=F32, device=dev)
        ops.gemm_tn(dy, t, dW2, accumulate=False, colsum=db2)
        dpre = ops.gemm_nt(dy, w2_t, ops.EPI_BIAS_BF16)
        ops.tanh_bwd_bf16(dpre, t, out=dpre)
        db1 = torch.zeros((Dh,), dtype=F32, device=dev) if has_b1 else None
        dW1 = torch.empty((Dh, K), dtype=F32, device=dev)
        ops.gemm_tn(dpre, xb, dW1, accumulate=False, colsum=db1)
        dx = ops.gemm_nt(dpre, w1_t, ops.EPI_BIAS_BF16).view(*lead, K).to(xdtype) if ctx.needs_input_grad[0] else None
        return dx, dW1, db1, dW2, db2


def tanh_mlp(x, w1, b1, w2, b2):
    """nn.Sequential(nn.Linear(dim, hidden), nn.Tanh(), nn.Linear(hidden, dim)) on x [..., dim]: bf16 GEMM operands, fp32 accumulation,
    the result in x's dtype.  dim and hidden must be multiples of 64 (the GEMMs' reduction dims).  The residual add stays with the caller."""
    for name, v in (("x", x), ("w1", w1), ("w2", w2)):
        if not isinstance(v, torch.Tensor):
            raise ops._lib.VitamdError(f"tanh_mlp: {name} must be a tensor")
    if x.dim() < 1 or w1.dim() != 2 or w2.dim() != 2 or w1.shape[1] != x.shape[-1] or w2.shape[1] != w1.shape[0]:
        raise ops._lib.VitamdError(f"tanh_mlp: x {tuple(x.shape)}, w1 {tuple(w1.shape)} and w2 {tuple(w2.shape)} do not chain")
    if x.shape[-1] % 64 or w1.shape[0] % 64 or w2.shape[0] % 4:
        raise ops._lib.VitamdError(f"tanh_mlp: dim {x.shape[-1]} and hidden {w1.shape[0]} must be multiples of 64, the output width {w2.shape[0]} of 4")
    if not x.is_cuda or not w1.is_cuda or not w2.is_cuda:
        raise ops._lib.VitamdError("tanh_mlp: expected ROCm device tensors (the HIP kernels are the only implementation)")
    return TanhMlpFn.apply(x, w1, b1, w2, b2)


# ------------------------------------------------------------------------------------------------ the pixel tail
def conv_shuffle_tokens(y, grid, p):
    """[B, grid*grid, c*p*p] -> [B, c, grid*p, grid*p] ('b (h w) (c p1 p2) -> b c (h p1) (w p2)'): what nn.ConvTranspose2d(dim, c, kernel_size
    = stride = p) does to the output of the Linear that its weight [dim, c*p*p] is"""
    B, _, F = y.shape
    c = F // (p * p)
    return y.view(B, grid, grid, c, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, c, grid * p, grid * p)


def _recon_l1_torch(tokens3, images, grid, patch, return_recon):
    """the torch expressions: token rows that are not whole 16-byte pieces"""
    recon = conv_shuffle_tokens(tokens3.float(), grid, patch)
    loss = (recon - images).abs().mean()
    return (loss, recon) if return_recon else loss


class ReconL1Fn(torch.autograd.Function):
    """(loss, recon or None) on tokens that exist already; the backward takes the gradients of both outputs at once"""

    @staticmethod
    def forward(ctx, tokens, images, grid, patch, want_recon):
        t = _rows(tokens)
        img = _f32c(images)
        loss, recon = ops.recon_l1_fwd(t, img, grid, patch, want_recon)
        ctx.save_for_backward(t, img)
        ctx.meta = (tuple(tokens.shape), grid, patch)
        ctx.set_materialize_grads(False)
        return loss, recon

    @staticmethod
    def backward(ctx, g_loss, g_recon):
        t, img = ctx.saved_tensors
        shape, grid, patch = ctx.meta
        gl = _zero_scalar(t) if g_loss is None else _scalar(g_loss)
        dt = ops.recon_l1_bwd(t, img, grid, patch, gl, None if g_recon is None else _f32c(g_recon))
        return dt.view(shape), None, None, None, None


def _check_tail(what, rows, F, images, grid, patch):
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ops._lib.VitamdError(f"{what}: expected images [B, c, H, W]")
    B, c, H, Wd = images.shape
    if grid < 1 or patch < 1 or H != grid * patch or Wd != grid * patch or F != patch * patch * c or rows != B * grid * grid:
        raise ValueError(f"{what}: {rows} token rows of width {F} and images {tuple(images.shape)} do not fit grid {grid}, patch {patch}")
    return B, c


def recon_l1(tokens, images, grid, patch, return_recon=False):
    """mean |conv_shuffle_tokens(tokens) - images| for tokens fp32 or bf16 [B, grid*grid, c*patch*patch] (or [B*grid*grid, ...]) and images
    fp32 [B, c, grid*patch, grid*patch]: the 0-dim fp32 loss, computed in fp32 on the tokens as stored; its gradient g sign(.) / N
    (sign(0) = 0) comes back in the tokens' dtype.  return_recon: -> (loss, recon fp32 [B, c, H, W]), the image as a second differentiable
    output; a gradient arriving on it joins the loss's own inside the backward kernel.  Token widths outside the kernels' 16-byte path
    (patch 2 in bf16: 12 features) take the torch expressions."""
    if not isinstance(tokens, torch.Tensor) or tokens.dim() not in (2, 3):
        raise ops._lib.VitamdError("recon_l1: expected tokens [B, grid*grid, F]")
    F = tokens.shape[-1]
    B, _ = _check_tail("recon_l1", tokens.numel() // max(F, 1), F, images, grid, patch)
    if not tokens.is_cuda or not images.is_cuda:
        raise ops._lib.VitamdError("recon_l1: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if not ops.recon_l1_applies(_rows(tokens)):
        return _recon_l1_torch(tokens.reshape(B, grid * grid, F), images, grid, patch, return_recon)
    loss, recon = ReconL1Fn.apply(tokens, images, grid, patch, bool(return_recon))
    return (loss, recon) if return_recon else loss


class LinearReconL1Fn(torch.autograd.Function):
    """(loss, recon or None) = recon_l1(h W + b, images) for the parameters of nn.ConvTranspose2d(dim, c, p, p): W = weight viewed
    [dim, c*p*p], b = bias repeated p*p times.  The bf16 tokens exist once: written by the head GEMM, read by the loss kernel, overwritten
    in place by their own gradient in the backward, which then feeds the two gradient GEMMs and the bias column sum (the structure of
    tokenizer.LinearReconMSEFn).  The layer's weight is the TRANSPOSE of a Linear's [out, in], so the bf16 copies WEIGHTS keeps of it serve
    with their roles swapped - the transposed copy in the forward, the plain one in the input gradient - and the weight gradient h^T dy
    comes out of the TN GEMM in the layer's own layout: no transpose is ever formed."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, h, weight, bias, images, grid, patch, want_recon):
        hb = ops.cast_bf16(_f32c(h))
        _, w_out_in = WEIGHTS.get(weight, True)                                      # [c*p*p, dim]
        pp = patch * patch
        bias_f = None if bias is None else _f32c(bias).repeat_interleave(pp)
        tokens = ops.gemm_nt(hb, w_out_in, ops.EPI_BIAS_BF16, bias=bias_f)
        img = _f32c(images)
        loss, recon = ops.recon_l1_fwd(tokens, img, grid, patch, want_recon)
        ctx.save_for_backward(hb, tokens, img)
        ctx.weight = weight
        ctx.meta = (h.dtype, bias is not None, grid, patch)
        ctx.consumed = False
        ctx.set_materialize_grads(False)
        return loss, recon

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_loss, g_recon):
        if ctx.consumed:
            raise RuntimeError("linear_recon_l1: the tokens were overwritten by their gradient in the first backward; "
                               "a second backward through the same loss needs a new forward")
        ctx.consumed = True
        hb, tokens, img = ctx.saved_tensors
        hdtype, has_bias, grid, patch = ctx.meta
        weight = ctx.weight
        w_in_out, _ = WEIGHTS.get(weight, True)                                      # [dim, c*p*p]
        gl = _zero_scalar(tokens) if g_loss is None else _scalar(g_loss)
        dy = ops.recon_l1_bwd(tokens, img, grid, patch, gl, None if g_recon is None else _f32c(g_recon), out=tokens)      # in place
        dx = ops.gemm_nt(dy, w_in_out, ops.EPI_BIAS_BF16).to(hdtype) if ctx.needs_input_grad[0] else None
        dW = torch.empty((weight.shape[0], weight.numel() // weight.shape[0]), dtype=F32, device=dy.device)
        ops.gemm_tn(hb, dy, dW, accumulate=False)
        db = ops.colsum(dy).view(-1, patch * patch).sum(dim=1) if has_bias else None
        return dx, dW.view(weight.shape), db, None, None, None, None


def linear_recon_l1(h, convt_weight, convt_bias, images, grid, patch, return_recon=False):
    """recon_l1(nn.ConvTranspose2d(dim, c, kernel_size=patch, stride=patch) on the token grid of h, images) for h [..., dim] (B*grid*grid
    rows), convt_weight fp32 [dim, c, patch, patch], convt_bias fp32 [c] or None: the 0-dim fp32 loss, and with return_recon the image
    fp32 [B, c, H, W] as a second differentiable output (so that a perceptual term stays on this route).  dim % 64 == 0 and
    c*patch*patch % 64 == 0: the fused head (LinearReconL1Fn; its backward consumes the tokens, so a second backward through the same
    loss raises RuntimeError).  Other shapes: the weight transposed and the bias repeated by torch ops inside the autograd graph,
    functions.linear, then recon_l1."""
    if not isinstance(h, torch.Tensor) or not isinstance(convt_weight, torch.Tensor) or h.dim() < 1 or convt_weight.dim() != 4 \
            or convt_weight.shape[0] != h.shape[-1] or convt_weight.shape[2] != patch or convt_weight.shape[3] != patch:
        raise ops._lib.VitamdError("linear_recon_l1: expected h [..., dim] and a ConvTranspose2d weight [dim, c, patch, patch]")
    D = h.shape[-1]
    F = convt_weight.numel() // D
    B, c = _check_tail("linear_recon_l1", h.numel() // max(D, 1), F, images, grid, patch)
    if convt_bias is not None and (not isinstance(convt_bias, torch.Tensor) or tuple(convt_bias.shape) != (c,)):
        raise ValueError(f"linear_recon_l1: bias must be [{c}]")
    if not h.is_cuda or not convt_weight.is_cuda or not images.is_cuda:
        raise ops._lib.VitamdError("linear_recon_l1: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if not fused_head_applies(F, D):
        w = convt_weight.reshape(D, F).t()
        b = None if convt_bias is None else convt_bias.repeat_interleave(patch * patch)
        return recon_l1(linear(h, w, b).reshape(B, grid * grid, F), images, grid, patch, return_recon)
    loss, recon = LinearReconL1Fn.apply(h.reshape(-1, D), convt_weight, convt_bias, images, grid, patch, bool(return_recon))
    return (loss, recon) if return_recon else loss
