"""Training the image tokenizers on the HIP kernels: the cosine-similarity VQ quantiser and the reconstruction loss fused with the pixel
head (csrc/tokenizer.hip).

    q, ids, qloss = tokenizer.vq_quantize(latents, quant.codebook.weight)        # train_titok.Quantizer.forward: four launches, one more backward
    loss = tokenizer.recon_mse(tokens, images, grid, patch)                      # mse_loss(pixel_shuffle_tokens(tokens), images)
    loss = tokenizer.linear_recon_mse(h, embd_proj.weight, embd_proj.bias, images, grid, patch)   # head GEMM -> bf16 tokens -> loss

and the 1D TiTok of train_tatitok (blocks.TiTokDecoder's tail, blocks.VectorQuantizer(use_l2_norm=True)):

    q, ids, qloss = tokenizer.vq_quantize(latents, quantize.embedding.weight, unit_codes=True)    # normalised codes out, gradient through the norm
    loss = tokenizer.conv_recon_mse(tokens, conv_out.weight, conv_out.bias, images, grid, patch)  # mse(conv3x3(pixel_shuffle(tokens)), images)
    loss, recon = tokenizer.linear_conv_recon_mse(h, ffn0.weight, ffn0.bias, conv_out.weight, conv_out.bias, images, grid, patch, return_recon=True)

Every value the backward needs stays on the device (upstream gradients are read by the kernels).
"""
from __future__ import annotations

import torch

from . import ops
from .functions import WEIGHTS, _amp_bwd, _amp_fwd, _f32c, linear
from .lm import _scalar

BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ quantiser
def vq_quantize_torch(x, codebook_weight):
    """the present route (train_titok.Quantizer.forward): torch device ops around the nearest-code kernel; wide codes stay here"""
    unit = torch.nn.functional.normalize(x, dim=-1)
    with torch.no_grad():
        codes_unit = torch.nn.functional.normalize(codebook_weight, dim=-1).float().contiguous()
        ids = ops.vq_nearest(unit.reshape(-1, unit.shape[-1]).float().contiguous(), codes_unit).view(unit.shape[:-1])
    picked = torch.nn.functional.embedding(ids, codebook_weight)
    sq = lambda t: t.pow(2).mean()
    loss = sq(picked - unit.detach()) + 0.25 * sq(picked.detach() - unit)
    return unit + (picked - unit).detach(), ids, loss


class VQQuantizeFn(torch.autograd.Function):
    """the quantiser kernels, forward and backward; unit_codes: q and the loss on the normalised code rows, the codebook gradient through
    the normalisation"""

    @staticmethod
    def forward(ctx, x, codebook, unit_codes):
        lead, d = x.shape[:-1], x.shape[-1]
        x2 = x.detach().reshape(-1, d).contiguous()
        cb = codebook.detach().contiguous()
        unit, rnorm, q, idx, loss = (ops.vq_quantize_unit_fwd if unit_codes else ops.vq_quantize_fwd)(x2, cb)
        ctx.save_for_backward(unit, rnorm, idx, cb)
        ctx.lead, ctx.unit_codes = tuple(lead), unit_codes
        ids = idx.view(lead)
        ctx.mark_non_differentiable(ids)
        return q.view(*lead, d), ids, loss

    @staticmethod
    def backward(ctx, g_q, _g_ids, g_loss):
        unit, rnorm, idx, cb = ctx.saved_tensors
        gq = None if g_q is None else g_q.detach().to(F32).reshape(unit.shape).contiguous()
        gl = None if g_loss is None else _scalar(g_loss)
        dx, dcb = (ops.vq_quantize_unit_bwd if ctx.unit_codes else ops.vq_quantize_bwd)(gq, gl, unit, rnorm, idx, cb)
        return dx.view(*ctx.lead, unit.shape[1]), dcb, None


def vq_quantize_unit_torch(x, codebook_weight):
    """blocks.VectorQuantizer(use_l2_norm=True, commitment_cost=0.25).forward on [..., d] rows, as torch device ops around the nearest-code
    kernel: the route of wide codes"""
    normalize = torch.nn.functional.normalize
    unit = normalize(x, dim=-1)
    with torch.no_grad():
        ids = ops.vq_nearest(unit.reshape(-1, unit.shape[-1]).float().contiguous(),
                             normalize(codebook_weight, dim=-1).float().contiguous()).view(unit.shape[:-1])
    picked = normalize(torch.nn.functional.embedding(ids, codebook_weight), dim=-1)
    sq = lambda t: t.pow(2).mean()
    loss = 0.25 * sq(picked.detach() - unit) + sq(picked - unit.detach())
    return unit + (picked - unit).detach(), ids, loss


def vq_quantize(x, codebook_weight, unit_codes=False):
    """train_titok.Quantizer.forward on x fp32 [..., d] and the codebook fp32 [K, d] -> (q [..., d], ids int64 [...], loss 0-dim):
    q = unit + (picked - unit) with the straight-through gradient, loss = |picked - sg(unit)|^2 + 0.25 |sg(picked) - unit|^2 (means).
    unit_codes: picked = normalize(codebook[ids]) instead of the raw rows, the codebook gradient taken through the normalisation -
    blocks.VectorQuantizer(use_l2_norm=True, commitment_cost=0.25).forward on channels-last rows.
    d <= 64: the two quantiser kernels; wider codes: the present torch expressions around ops.vq_nearest."""
    if not isinstance(x, torch.Tensor) or not isinstance(codebook_weight, torch.Tensor) or x.dim() < 1 or codebook_weight.dim() != 2 \
            or x.shape[-1] != codebook_weight.shape[1]:
        raise ops._lib.VitamdError("vq_quantize: expected x [..., d] and codebook [K, d]")
    if x.dtype != F32 or codebook_weight.dtype != F32:
        raise ops._lib.VitamdError(f"vq_quantize: expected fp32 inputs, got {x.dtype} and {codebook_weight.dtype}")
    if not x.is_cuda or not codebook_weight.is_cuda:
        raise ops._lib.VitamdError("vq_quantize: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if x.shape[-1] > ops.VQ_MAX_D:
        return vq_quantize_unit_torch(x, codebook_weight) if unit_codes else vq_quantize_torch(x, codebook_weight)
    return VQQuantizeFn.apply(x, codebook_weight, bool(unit_codes))


# ------------------------------------------------------------------------------------------------ reconstruction loss
def pixel_shuffle_tokens(y, grid, p):
    """[B, grid*grid, p*p*c] -> [B, c, grid*p, grid*p] ('b (h w) (p1 p2 c) -> b c (h p1) (w p2)'): train_titok.pixel_shuffle_tokens"""
    B, _, F = y.shape
    c = F // (p * p)
    return y.view(B, grid, grid, p, p, c).permute(0, 5, 1, 3, 2, 4).reshape(B, c, grid * p, grid * p)


def _rows(tokens):
    """tokens of any leading shape as [M, F] with unit inner stride (a copy only when the layout demands one)"""
    t = tokens.detach()
    t = t.reshape(-1, t.shape[-1])
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


class ReconMSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, images, grid, patch):
        t = _rows(tokens)
        img = images.detach().to(F32).contiguous()
        loss = ops.recon_mse_fwd(t, img, grid, patch)
        ctx.save_for_backward(t, img)
        ctx.meta = (tuple(tokens.shape), grid, patch)
        return loss

    @staticmethod
    def backward(ctx, g):
        t, img = ctx.saved_tensors
        shape, grid, patch = ctx.meta
        return ops.recon_mse_bwd(t, img, grid, patch, _scalar(g)).view(shape), None, None, None


def recon_mse(tokens, images, grid, patch):
    """mse_loss(pixel_shuffle_tokens(tokens), images) for tokens fp32 or bf16 [B, grid*grid, patch*patch*c] (or [B*grid*grid, ...]) and
    images fp32 [B, c, grid*patch, grid*patch]: the 0-dim fp32 loss, computed in fp32 on the tokens as stored; its gradient comes back in
    the tokens' dtype.  Token widths outside the kernels' 16-byte path take the torch expressions."""
    if not isinstance(tokens, torch.Tensor) or not isinstance(images, torch.Tensor) or tokens.dim() not in (2, 3) or images.dim() != 4:
        raise ops._lib.VitamdError("recon_mse: expected tokens [B, grid*grid, F] and images [B, c, H, W]")
    B, c, H, Wd = images.shape
    F = patch * patch * c
    if H != grid * patch or Wd != grid * patch or tokens.shape[-1] != F or tokens.numel() != B * grid * grid * F:
        raise ValueError(f"recon_mse: tokens {tuple(tokens.shape)} and images {tuple(images.shape)} do not fit grid {grid}, patch {patch}")
    if not tokens.is_cuda or not images.is_cuda:
        raise ops._lib.VitamdError("recon_mse: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if not ops.recon_mse_applies(_rows(tokens)):
        return torch.nn.functional.mse_loss(pixel_shuffle_tokens(tokens.reshape(B, grid * grid, F).float(), grid, patch), images)
    return ReconMSEFn.apply(tokens, images, grid, patch)


def fused_head_applies(F, D):
    """the shapes linear_recon_mse runs unpadded on the MFMA GEMMs; others take functions.linear + recon_mse"""
    return F % 64 == 0 and D % 64 == 0


class LinearReconMSEFn(torch.autograd.Function):
    """loss = recon_mse(h W^T + b, images) with bf16 tokens that exist once: written by the head GEMM, read by the loss, overwritten in
    place by their own gradient in the backward, which then feeds the two gradient GEMMs and the bias column sum."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, h, weight, bias, images, grid, patch):
        hb = ops.cast_bf16(_f32c(h))
        wb, _ = WEIGHTS.get(weight, True)
        tokens = ops.gemm_nt(hb, wb, ops.EPI_BIAS_BF16, bias=None if bias is None else _f32c(bias))
        img = _f32c(images)
        loss = ops.recon_mse_fwd(tokens, img, grid, patch)
        ctx.save_for_backward(hb, tokens, img)
        ctx.weight = weight
        ctx.meta = (h.dtype, bias is not None, grid, patch)
        ctx.consumed = False
        return loss

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        if ctx.consumed:
            raise RuntimeError("linear_recon_mse: the tokens were overwritten by their gradient in the first backward; "
                               "a second backward through the same loss needs a new forward")
        ctx.consumed = True
        hb, tokens, img = ctx.saved_tensors
        hdtype, has_bias, grid, patch = ctx.meta
        weight = ctx.weight
        _, wbt = WEIGHTS.get(weight, True)
        dy = ops.recon_mse_bwd(tokens, img, grid, patch, _scalar(g), out=tokens)                    # in place
        dx = ops.gemm_nt(dy, wbt, ops.EPI_BIAS_BF16).to(hdtype) if ctx.needs_input_grad[0] else None
        dW = torch.empty((weight.shape[0], weight.numel() // weight.shape[0]), dtype=F32, device=dy.device)
        ops.gemm_tn(dy, hb, dW, accumulate=False)
        db = ops.colsum(dy) if has_bias else None
        return dx, dW.view(weight.shape), db, None, None, None


def linear_recon_mse(h, weight, bias, images, grid, patch):
    """recon_mse(nn.Linear(h), images) for h [..., D] (B*grid*grid rows), weight fp32 [F, D] (or a 1x1 conv's [F, D, 1, 1]), bias fp32 [F]
    or None: the 0-dim fp32 loss.  F % 64 == 0 and D % 64 == 0: the fused head (LinearReconMSEFn; its backward consumes the tokens, so a
    second backward through the same loss raises RuntimeError).  Other shapes: functions.linear followed by recon_mse."""
    if not isinstance(h, torch.Tensor) or not isinstance(weight, torch.Tensor) or h.dim() < 1 or weight.dim() < 2 \
            or weight.numel() != weight.shape[0] * h.shape[-1]:
        raise ops._lib.VitamdError("linear_recon_mse: expected h [..., D] and weight [F, D]")
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ops._lib.VitamdError("linear_recon_mse: expected images [B, c, H, W]")
    F, D = weight.shape[0], h.shape[-1]
    B, c, H, Wd = images.shape
    if H != grid * patch or Wd != grid * patch or F != patch * patch * c or h.numel() != B * grid * grid * D:
        raise ValueError(f"linear_recon_mse: h {tuple(h.shape)}, weight {tuple(weight.shape)} and images {tuple(images.shape)} do not fit "
                         f"grid {grid}, patch {patch}")
    if not h.is_cuda or not weight.is_cuda or not images.is_cuda:
        raise ops._lib.VitamdError("linear_recon_mse: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if not fused_head_applies(F, D):
        return recon_mse(linear(h, weight, bias).reshape(B, grid * grid, F), images, grid, patch)
    return LinearReconMSEFn.apply(h.reshape(-1, D), weight, bias, images, grid, patch)


# ------------------------------------------------------------------------------------------------ pixel tail of blocks.TiTokDecoder
def _zero_scalar(like):
    return torch.zeros((), dtype=F32, device=like.device)


def _check_conv_tail(what, rows, F, conv_w, conv_b, images, grid, patch):
    """shape and argument errors of the two pixel-tail entry points, before any device is looked at -> B"""
    if not isinstance(conv_w, torch.Tensor) or not isinstance(conv_b, torch.Tensor) or not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ops._lib.VitamdError(f"{what}: expected conv weight [3, 3, 3, 3], conv bias [3] and images [B, 3, H, W]")
    B, c, H, Wd = images.shape
    if tuple(conv_w.shape) != (3, 3, 3, 3) or tuple(conv_b.shape) != (3,) or c != 3:
        raise ValueError(f"{what}: conv weight {tuple(conv_w.shape)}, bias {tuple(conv_b.shape)} and images {tuple(images.shape)} are not "
                         "those of Conv2d(3, 3, 3, padding=1)")
    if grid < 1 or patch < 1 or H != grid * patch or Wd != grid * patch or F != patch * patch * 3 or rows != B * grid * grid:
        raise ValueError(f"{what}: {rows} token rows of width {F} and images {tuple(images.shape)} do not fit grid {grid}, patch {patch}")
    return B


class ConvReconMSEFn(torch.autograd.Function):
    """(loss, recon or None) of the pixel tail on tokens that exist already; the backward takes the gradients of both outputs at once"""

    @staticmethod
    def forward(ctx, tokens, conv_w, conv_b, images, grid, patch, want_recon):
        t = _rows(tokens)
        img, w, b = _f32c(images), _f32c(conv_w), _f32c(conv_b)
        loss, recon = ops.conv_recon_mse_fwd(t, w, b, img, grid, patch, want_recon)
        ctx.save_for_backward(t, w, b, img)
        ctx.meta = (tuple(tokens.shape), grid, patch)
        ctx.set_materialize_grads(False)
        return loss, recon

    @staticmethod
    def backward(ctx, g_loss, g_recon):
        t, w, b, img = ctx.saved_tensors
        shape, grid, patch = ctx.meta
        gl = _zero_scalar(t) if g_loss is None else _scalar(g_loss)
        dt, dw, db = ops.conv_recon_mse_bwd(t, w, b, img, grid, patch, gl, None if g_recon is None else _f32c(g_recon))
        return dt.view(shape), dw, db, None, None, None, None


def _conv_tail_torch(tokens3, conv_w, conv_b, images, grid, patch, return_recon):
    """the present operators: pixel-shuffle copy -> Conv3x3Fn -> mse_loss"""
    from .block_functions import Conv3x3Fn
    recon = Conv3x3Fn.apply(pixel_shuffle_tokens(tokens3.float(), grid, patch), conv_w, conv_b)
    loss = torch.nn.functional.mse_loss(recon, images)
    return (loss, recon) if return_recon else loss


def conv_recon_mse(tokens, conv_w, conv_b, images, grid, patch, return_recon=False):
    """mse_loss(conv3x3(pixel_shuffle_tokens(tokens), conv_w, padding 1) + conv_b, images) for tokens fp32 or bf16 [B, grid*grid, 3*patch*patch]
    (or [B*grid*grid, ...]), conv_w fp32 [3, 3, 3, 3], conv_b fp32 [3], images fp32 [B, 3, grid*patch, grid*patch]: the 0-dim fp32 loss in
    one kernel, fp32 arithmetic on the tokens as stored, the shuffled image never formed.  return_recon: -> (loss, recon fp32 [B, 3, H, W]),
    the convolved image as a second differentiable output; a gradient arriving on it joins the loss's own inside the backward kernel.
    The token gradient comes back in the tokens' dtype.  Shapes outside the kernels' 16-byte path (patch % 8 for bf16, % 4 for fp32,
    alignment) take the present operators."""
    if not isinstance(tokens, torch.Tensor) or tokens.dim() not in (2, 3):
        raise ops._lib.VitamdError("conv_recon_mse: expected tokens [B, grid*grid, F]")
    B = _check_conv_tail("conv_recon_mse", tokens.numel() // max(tokens.shape[-1], 1), tokens.shape[-1], conv_w, conv_b, images, grid, patch)
    if not tokens.is_cuda or not images.is_cuda or not conv_w.is_cuda or not conv_b.is_cuda:
        raise ops._lib.VitamdError("conv_recon_mse: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if not ops.conv_recon_mse_applies(_rows(tokens), patch):
        return _conv_tail_torch(tokens.reshape(B, grid * grid, -1), conv_w, conv_b, images, grid, patch, return_recon)
    loss, recon = ConvReconMSEFn.apply(tokens, conv_w, conv_b, images, grid, patch, bool(return_recon))
    return (loss, recon) if return_recon else loss


class LinearConvReconMSEFn(torch.autograd.Function):
    """(loss, recon or None) = conv_recon_mse(h W^T + b, ...) with bf16 tokens written once by the head GEMM and read by the tail kernel;
    the backward writes their gradient to a second buffer (a tile re-reads its neighbours' tokens) and feeds it to the two gradient GEMMs
    and the bias column sum.  One backward per forward, as LinearReconMSEFn."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, h, weight, bias, conv_w, conv_b, images, grid, patch, want_recon):
        hb = ops.cast_bf16(_f32c(h))
        wb, _ = WEIGHTS.get(weight, True)
        tokens = ops.gemm_nt(hb, wb, ops.EPI_BIAS_BF16, bias=None if bias is None else _f32c(bias))
        img, cw, cb = _f32c(images), _f32c(conv_w), _f32c(conv_b)
        loss, recon = ops.conv_recon_mse_fwd(tokens, cw, cb, img, grid, patch, want_recon)
        ctx.save_for_backward(hb, tokens, img, cw, cb)
        ctx.weight = weight
        ctx.meta = (h.dtype, bias is not None, grid, patch)
        ctx.consumed = False
        ctx.set_materialize_grads(False)
        return loss, recon

    @staticmethod
    @_amp_bwd
    def backward(ctx, g_loss, g_recon):
        if ctx.consumed:
            raise RuntimeError("linear_conv_recon_mse: one backward per forward (the contract of linear_recon_mse); "
                               "a second backward through the same loss needs a new forward")
        ctx.consumed = True
        hb, tokens, img, cw, cb = ctx.saved_tensors
        hdtype, has_bias, grid, patch = ctx.meta
        weight = ctx.weight
        _, wbt = WEIGHTS.get(weight, True)
        gl = _zero_scalar(tokens) if g_loss is None else _scalar(g_loss)
        dy, dcw, dcb = ops.conv_recon_mse_bwd(tokens, cw, cb, img, grid, patch, gl, None if g_recon is None else _f32c(g_recon))
        dx = ops.gemm_nt(dy, wbt, ops.EPI_BIAS_BF16).to(hdtype) if ctx.needs_input_grad[0] else None
        dW = torch.empty((weight.shape[0], weight.numel() // weight.shape[0]), dtype=F32, device=dy.device)
        ops.gemm_tn(dy, hb, dW, accumulate=False)
        db = ops.colsum(dy) if has_bias else None
        return dx, dW.view(weight.shape), db, dcw, dcb, None, None, None, None


def linear_conv_recon_mse(h, ffn_w, ffn_b, conv_w, conv_b, images, grid, patch, return_recon=False):
    """conv_recon_mse(nn.Linear(h), ...) for h [..., D] (B*grid*grid rows), ffn_w fp32 [F, D] (or a 1x1 conv's [F, D, 1, 1]), ffn_b fp32 [F]
    or None - blocks.TiTokDecoder's `ffn` and `conv_out` on the ln_post rows.  F % 64 == 0 and D % 64 == 0 and a patch the tail kernels
    take: the fused head (LinearConvReconMSEFn: bf16 tokens written once; one backward per forward).  Other shapes: functions.linear
    followed by conv_recon_mse.  return_recon as conv_recon_mse."""
    if not isinstance(h, torch.Tensor) or not isinstance(ffn_w, torch.Tensor) or h.dim() < 1 or ffn_w.dim() < 2 \
            or ffn_w.numel() != ffn_w.shape[0] * h.shape[-1]:
        raise ops._lib.VitamdError("linear_conv_recon_mse: expected h [..., D] and ffn weight [F, D]")
    F, D = ffn_w.shape[0], h.shape[-1]
    B = _check_conv_tail("linear_conv_recon_mse", h.numel() // max(D, 1), F, conv_w, conv_b, images, grid, patch)
    if not h.is_cuda or not ffn_w.is_cuda or not images.is_cuda or not conv_w.is_cuda or not conv_b.is_cuda:
        raise ops._lib.VitamdError("linear_conv_recon_mse: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if not fused_head_applies(F, D) or patch % 8 != 0:
        return conv_recon_mse(linear(h, ffn_w, ffn_b).reshape(B, grid * grid, F), conv_w, conv_b, images, grid, patch, return_recon)
    loss, recon = LinearConvReconMSEFn.apply(h.reshape(-1, D), ffn_w, ffn_b, conv_w, conv_b, images, grid, patch, bool(return_recon))
    return (loss, recon) if return_recon else loss
