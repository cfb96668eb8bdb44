"""Training a next-token model on the HIP kernels: the cross-entropy over the vocabulary, the output head fused with it, and the
token + position embedding (csrc/loss.hip).

    loss = lm.cross_entropy(logits, target)                       # F.cross_entropy(logits.float(), target), mean, on the device
    loss = lm.soft_cross_entropy(logits, ya, yb, lam, 0.1)        # Mixup / CutMix label pairs + label smoothing
    loss = lm.linear_cross_entropy(h, proj.weight, proj.bias, y)  # head GEMM -> bf16 logits -> loss, nothing in fp32 in between
    x = lm.token_embed(ids, tok_embed.weight, pos_embed.weight)   # tok[ids] + pos[:S], fp32
    x = lm.prefixed_token_embed(ids, tok, pos, prefix)            # cat([prefix rows, tok[ids] + pos[:S]], 1), one kernel (csrc/assemble.hip)
    x = lm.prefixed_rows(body, pos, prefix)                       # cat([prefix rows, body + pos[:S]], 1), DESIGN.md section 16

Every value the backward needs stays on the device (the upstream gradient is read by the kernel), so a step built from these records
into a graph (vitamd.graph.GraphedStep) like the rest of the path.
"""
from __future__ import annotations

import torch

from . import ops
from .functions import WEIGHTS, _amp_bwd, _amp_fwd, _f32c, linear

BF16, F32 = torch.bfloat16, torch.float32


def _rows(logits):
    """logits of any leading shape as [M, V] with unit inner stride (a copy only when the layout demands one)"""
    x = logits.detach()
    x = x.reshape(-1, x.shape[-1])
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def _target(target, M):
    if not isinstance(target, torch.Tensor) or target.dtype != torch.int64:
        raise ops._lib.VitamdError(f"target: expected an int64 tensor, got {getattr(target, 'dtype', type(target))}")
    t = target.reshape(-1).contiguous()
    if t.numel() != M:
        raise ops._lib.VitamdError(f"target: expected {M} elements (one per row of logits), got {t.numel()}")
    return t


def _scalar(g):
    """the upstream gradient of a 0-dim loss as a device fp32 scalar the kernel reads (never .item())"""
    return g.detach().to(F32).contiguous()


class CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        if not isinstance(logits, torch.Tensor) or logits.dim() < 1:
            raise ops._lib.VitamdError("logits: expected a tensor [..., V]")
        x = _rows(logits)
        t = _target(target, x.shape[0])
        _, lse, stats = ops.cross_entropy_fwd(x, t, ignore_index)
        ctx.save_for_backward(x, t, lse, stats)
        ctx.meta = (tuple(logits.shape), int(ignore_index))
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        x, t, lse, stats = ctx.saved_tensors
        shape, ignore_index = ctx.meta
        d = ops.cross_entropy_bwd(x, t, lse, stats, _scalar(g), ignore_index)        # dense, the logits' dtype
        return d.view(shape), None, None


def cross_entropy(logits, target, ignore_index=-100):
    """Mean cross-entropy of logits [..., V] (fp32 or bf16, device) against target int64 [...] over the targets != ignore_index, computed
    in fp32 on the logits as stored: the 0-dim fp32 loss.  Its gradient comes back in the logits' dtype.  A drop-in `loss_fn` for
    train_vit.train_step and vitamd.graph.GraphedStep."""
    return CrossEntropyFn.apply(logits, target, ignore_index)


class SoftCrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, target_b, lam, smoothing):
        if not isinstance(logits, torch.Tensor) or logits.dim() < 1:
            raise ops._lib.VitamdError("logits: expected a tensor [..., V]")
        x = _rows(logits)
        M = x.shape[0]
        t = _target(target, M)
        if lam is not None:
            if not isinstance(lam, torch.Tensor) or lam.numel() != M:
                raise ops._lib.VitamdError(f"lam: expected a tensor of {M} elements (one per row of logits)")
            tb, lam = _target(target_b, M), lam.detach().reshape(-1).to(F32).contiguous()
        else:
            tb = None
        soft = (tb, lam, float(smoothing))
        _, lse, stats = ops.cross_entropy_fwd(x, t, soft=soft)
        ctx.save_for_backward(x, t, lse, stats, *(() if lam is None else (tb, lam)))
        ctx.meta = (tuple(logits.shape), float(smoothing))
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        x, t, lse, stats, *pair = ctx.saved_tensors
        shape, smoothing = ctx.meta
        tb, lam = pair if pair else (None, None)
        d = ops.cross_entropy_bwd(x, t, lse, stats, _scalar(g), soft=(tb, lam, smoothing))           # dense, the logits' dtype
        return d.view(shape), None, None, None, None


def soft_cross_entropy(logits, target, target_b=None, lam=None, smoothing=0.0):
    """Mean soft-target cross-entropy of logits [..., V] (fp32 or bf16, device) against the target
    (1 - smoothing) * (lam * onehot(target) + (1 - lam) * onehot(target_b)) + smoothing / V per row - Mixup / CutMix label pairs and
    label smoothing (timm's SoftTargetCrossEntropy on its mixup_target) without the [M, V] target tensor: the 0-dim fp32 loss, the mean
    over all rows.  lam: device fp32 [...] read by the kernels (None: target alone, target_b is not looked at).  With smoothing 0 and
    lam None it is cross_entropy without ignored rows, bit for bit.  A drop-in loss for train_vit.train_step through
    vitamd.mix.SoftTargetLoss."""
    return SoftCrossEntropyFn.apply(logits, target, target_b, lam, smoothing)


def fused_head_applies(V, D):
    """the shapes linear_cross_entropy runs unpadded on the MFMA GEMMs (their own rules); others take functions.linear + cross_entropy"""
    return V % 64 == 0 and D % 64 == 0


class LinearCrossEntropyFn(torch.autograd.Function):
    """loss = cross_entropy(h W^T + b, target) with bf16 logits that exist once: written by the head GEMM, read by the loss, overwritten
    in place by their own gradient in the backward, which then feeds the two gradient GEMMs and the bias column sum."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, h, weight, bias, target, ignore_index):
        M, D = h.shape
        hb = ops.cast_bf16(_f32c(h))
        wb, _ = WEIGHTS.get(weight, True)
        logits = ops.gemm_nt(hb, wb, ops.EPI_BIAS_BF16, bias=None if bias is None else _f32c(bias))
        t = _target(target, M)
        _, lse, stats = ops.cross_entropy_fwd(logits, t, ignore_index)
        ctx.save_for_backward(hb, logits, t, lse, stats)
        ctx.weight = weight
        ctx.meta = (h.dtype, bias is not None, int(ignore_index))
        ctx.consumed = False
        return stats[0]

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        if ctx.consumed:
            raise RuntimeError("linear_cross_entropy: the logits were overwritten by their gradient in the first backward; "
                               "a second backward through the same loss needs a new forward")
        ctx.consumed = True
        hb, logits, t, lse, stats = ctx.saved_tensors
        hdtype, has_bias, ignore_index = ctx.meta
        weight = ctx.weight
        _, wbt = WEIGHTS.get(weight, True)
        dl = ops.cross_entropy_bwd(logits, t, lse, stats, _scalar(g), ignore_index, out=logits)     # in place
        dx = ops.gemm_nt(dl, wbt, ops.EPI_BIAS_BF16).to(hdtype) if ctx.needs_input_grad[0] else None
        dW = torch.empty(tuple(weight.shape), dtype=F32, device=dl.device)
        ops.gemm_tn(dl, hb, dW, accumulate=False)
        db = ops.colsum(dl) if has_bias else None
        return dx, dW, db, None, None


def linear_cross_entropy(h, weight, bias, target, ignore_index=-100):
    """cross_entropy(nn.Linear(h), target) for h [..., D], weight fp32 [V, D], bias fp32 [V] or None, target int64 [...]: the 0-dim fp32
    mean loss.  V % 64 == 0 and D % 64 == 0: the fused head (LinearCrossEntropyFn; its backward consumes the logits, so a second
    backward through the same loss raises RuntimeError).  Other shapes: functions.linear followed by cross_entropy."""
    if not isinstance(h, torch.Tensor) or not isinstance(weight, torch.Tensor) or h.dim() < 1 or weight.dim() != 2 or h.shape[-1] != weight.shape[1]:
        raise ops._lib.VitamdError("linear_cross_entropy: expected h [..., D] and weight [V, D]")
    V, D = weight.shape
    if not 2 <= V <= ops.CE_MAX_V:
        raise ValueError(f"cross_entropy: the vocabulary must hold 2 .. {ops.CE_MAX_V} entries, got {V}")
    if not h.is_cuda or not weight.is_cuda:
        raise ops._lib.VitamdError("linear_cross_entropy: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if not fused_head_applies(V, D):
        return cross_entropy(linear(h, weight, bias), target, ignore_index)
    return LinearCrossEntropyFn.apply(h.reshape(-1, D), weight, bias, target, ignore_index)


class TokenEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, tok_weight, pos_weight):
        if not isinstance(ids, torch.Tensor) or ids.dim() != 2:
            raise ops._lib.VitamdError("token_embed: ids must be int64 [B, S]")
        B, S = ids.shape
        tok, pos = tok_weight.detach(), pos_weight.detach()
        x = ops.embed_tokens_fwd(ids.contiguous(), tok, pos)
        ctx.save_for_backward(ids)
        ctx.meta = (tuple(tok.shape), tuple(pos.shape))
        return x.view(B, S, tok.shape[1])

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        tok_shape, pos_shape = ctx.meta
        B, S = ids.shape
        dtok = torch.zeros(tok_shape, dtype=F32, device=g.device)
        dpos = torch.zeros(pos_shape, dtype=F32, device=g.device)          # the full table: rows >= S stay zero
        ops.embed_tokens_bwd(_f32c(g).view(B * S, tok_shape[1]), ids.contiguous(), dtok, dpos)
        return None, dtok, dpos


def token_embed(ids, tok_weight, pos_weight):
    """tok_weight[ids] + pos_weight[:S] for ids int64 [B, S] -> fp32 [B, S, D] (the bits of the torch gather-and-add), with the gradients
    of both tables from one pass over the incoming gradient."""
    return TokenEmbedFn.apply(ids, tok_weight, pos_weight)


# ------------------------------------------------------------------------------------------------ sequence assembly
def _table(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ops._lib.VitamdError(f"{name}: expected a 2-d fp32 table [rows, D]")
    return t.detach()


class PrefixedTokenEmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, tok_weight, pos_weight, prefix_weight):
        if not isinstance(ids, torch.Tensor) or ids.dim() != 2:
            raise ops._lib.VitamdError("prefixed_token_embed: ids must be int64 [B, S]")
        tok, pos, prefix = _table(tok_weight, "tok_weight"), _table(pos_weight, "pos_weight"), _table(prefix_weight, "prefix_weight")
        ids = ids.contiguous()
        x = ops.assemble_tokens_fwd(prefix if prefix.shape[0] else None, pos, ids=ids, tok_table=tok)
        ctx.save_for_backward(ids)
        ctx.meta = (tuple(tok.shape), tuple(pos.shape), tuple(prefix.shape))
        return x

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        tok_shape, pos_shape, prefix_shape = ctx.meta
        dtok = torch.zeros(tok_shape, dtype=F32, device=g.device)
        dpos = torch.zeros(pos_shape, dtype=F32, device=g.device)          # the full table: rows >= S stay zero
        dprefix = torch.zeros(prefix_shape, dtype=F32, device=g.device)
        ops.assemble_tokens_bwd(_f32c(g), dprefix if prefix_shape[0] else None, dpos, ids=ids, dtok=dtok)
        return None, dtok, dpos, dprefix


def prefixed_token_embed(ids, tok_weight, pos_weight, prefix_weight):
    """cat([prefix_weight expanded over the batch, tok_weight[ids] + pos_weight[:S]], dim=1) for ids int64 [B, S] and prefix_weight fp32
    [E, D] -> fp32 [B, E+S, D] (the bits of the torch embedding / add / expand / cat) in one kernel, with the gradients of the three
    tables from one pass over the incoming gradient: those of the prefix and the positions summed over the batch in a fixed order."""
    return PrefixedTokenEmbedFn.apply(ids, tok_weight, pos_weight, prefix_weight)


class PrefixedRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, body, pos_weight, prefix_weight):
        if not isinstance(body, torch.Tensor) or body.dim() != 3 or body.dtype not in (F32, BF16):
            raise ops._lib.VitamdError("prefixed_rows: body must be fp32 or bf16 [B, S, D]")
        pos, prefix = _table(pos_weight, "pos_weight"), _table(prefix_weight, "prefix_weight")
        x = ops.assemble_tokens_fwd(prefix if prefix.shape[0] else None, pos, body=_f32c(body))
        ctx.meta = (body.dtype, tuple(pos.shape), tuple(prefix.shape))
        return x

    @staticmethod
    def backward(ctx, g):
        dtype, pos_shape, prefix_shape = ctx.meta
        g = _f32c(g)
        dpos = torch.zeros(pos_shape, dtype=F32, device=g.device)
        dprefix = torch.zeros(prefix_shape, dtype=F32, device=g.device)
        ops.assemble_tokens_bwd(g, dprefix if prefix_shape[0] else None, dpos)
        dbody = g[:, prefix_shape[0]:]                                     # a view: the body's gradient needs no kernel work
        return (dbody if dtype == F32 else dbody.to(dtype)), dpos, dprefix


def prefixed_rows(body, pos_weight, prefix_weight):
    """cat([prefix_weight expanded over the batch, body + pos_weight[:S]], dim=1) for body fp32 or bf16 [B, S, D] -> fp32 [B, E+S, D] in
    one kernel; the body's gradient (in its dtype) is the tail of the incoming one, those of the two tables come from one pass over it."""
    return PrefixedRowsFn.apply(body, pos_weight, prefix_weight)


# ------------------------------------------------------------------------------------------------ the head alone
def head_logits(h, weight, bias):
    """nn.Linear(h) for evaluation, h [..., D] -> logits [M, V] with the leading dimensions flattened, no gradient.  Where
    fused_head_applies(V, D): bf16, written by the head GEMM exactly as LinearCrossEntropyFn.forward writes them (the numbers the
    training loss is taken of; no fp32 logits exist).  Other shapes: functions.linear's fp32 logits."""
    if not isinstance(h, torch.Tensor) or not isinstance(weight, torch.Tensor) or h.dim() < 1 or weight.dim() != 2 or h.shape[-1] != weight.shape[1]:
        raise ops._lib.VitamdError("head_logits: expected h [..., D] and weight [V, D]")
    V, D = weight.shape
    if not h.is_cuda or not weight.is_cuda:
        raise ops._lib.VitamdError("head_logits: expected ROCm device tensors (the HIP kernels are the only implementation)")
    with torch.no_grad():
        if not fused_head_applies(V, D):
            return linear(h.reshape(-1, D), weight, bias)
        hb = ops.cast_bf16(_f32c(h.reshape(-1, D)))
        wb, _ = WEIGHTS.get(weight, True)
        return ops.gemm_nt(hb, wb, ops.EPI_BIAS_BF16, bias=None if bias is None else _f32c(bias))
