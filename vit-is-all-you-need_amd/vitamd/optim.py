"""Fused AdamW on the HIP path: same constructor arguments and update
rule as the reference's `torch.optim.AdamW` (train_vit.py:82), state kept in fp32.  Works with
`utils.get_lr_scheduler` (it is a torch.optim.Optimizer).

Two paths with the same arithmetic, element for element.  The default is one kernel per parameter tensor.  `multi_tensor=True` (implied by
`max_grad_norm`) walks a row table in device memory instead, one row per tensor with a gradient: the whole step is one launch, or three
with gradient-norm clipping (per-chunk sums of squares, one workgroup that derives the norm and the clip coefficient in a fixed order,
then the update, which reads the coefficient from device memory: no host synchronisation, the same bits on every rank).  `grad_norm` and
`clip_grad_norm_` give the norm and the in-place clip to users of other optimisers.  DESIGN.md section 12."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import lib as _lib

# struct vitamd_mt_row of include/vitamd.h
ROW_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("first_chunk", "<i4"), ("lr", "<f4"),
                      ("weight_decay", "<f4"), ("beta1", "<f4"), ("one_minus_beta1", "<f4"), ("beta2", "<f4"), ("one_minus_beta2", "<f4"),
                      ("eps", "<f4"), ("inv_bc1", "<f4"), ("inv_sqrt_bc2", "<f4")])
_HYPER = ("lr", "weight_decay", "beta1", "one_minus_beta1", "beta2", "one_minus_beta2", "eps", "inv_bc1", "inv_sqrt_bc2")


def plan_chunks(sizes, chunk):
    """Element counts -> (index of each tensor's first chunk, total chunks): a tensor of n elements takes ceil(n / chunk) chunks."""
    first, total = [], 0
    for n in sizes:
        if n < 1:
            raise ValueError("plan_chunks: a tensor in the table has at least one element")
        first.append(total)
        total += -(-int(n) // chunk)
    return first, total


def hyper_row(lr, betas, eps, weight_decay, step):
    """The nine per-tensor floats of a row, each rounded to fp32 once from the doubles, as vitamd_adamw_step_d forms them."""
    b1, b2 = float(betas[0]), float(betas[1])
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return tuple(np.float32(x) for x in (lr, weight_decay, b1, 1.0 - b1, b2, 1.0 - b2, eps, 1.0 / bc1, 1.0 / math.sqrt(bc2)))


def _chunk_elems(L):
    assert ROW_DTYPE.itemsize == L.vitamd_mt_row_bytes(), "vitamd_mt_row: the binding and the library disagree on the layout"
    return L.vitamd_mt_chunk_elems()


def _require(t, device, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise _lib.VitamdError(f"{what} must be a contiguous fp32 ROCm device tensor")
    if t.device != device:
        raise _lib.VitamdError(f"{what} is on {t.device}, the first one on {device}: one table holds one device")
    if t.data_ptr() % 16:
        raise _lib.VitamdError(f"{what} is not 16-byte aligned")


def _upload(rows, device):
    """One asynchronous copy from a freshly obtained pinned block (torch's pinned allocator keeps it until the copy has run); no staging
    buffer is ever rewritten while an earlier copy may be queued, and no pageable copy makes the host wait for the stream."""
    return torch.from_numpy(rows.view(np.uint8)).pin_memory().to(device, non_blocking=True)


def _norm(L, rows, dev_rows, total, device, max_norm, stream):
    """Launches the sum of squares and its finish; returns the two-float device buffer {norm, coef}."""
    partials = torch.empty(total, dtype=torch.float32, device=device)
    norm_coef = torch.empty(2, dtype=torch.float32, device=device)
    _lib.check(L.vitamd_mt_sumsq(rows.ctypes.data, dev_rows.data_ptr(), len(rows), total, partials.data_ptr(), norm_coef.data_ptr(),
                                 max_norm, stream), "mt_sumsq")
    return norm_coef


def _grad_table(L, parameters, what, copy_ok):
    """(rows with g / n / first_chunk filled, total chunks, device, the gradient tensors) of the parameters that have a gradient."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return None, 0, None, grads
    device = grads[0].device
    for i, g in enumerate(grads):
        if not g.is_contiguous():
            if not copy_ok:
                raise _lib.VitamdError(f"{what}: a gradient is not contiguous (a scaled copy would not be written back)")
            if not (g.is_cuda and g.dtype == torch.float32 and g.device == device):
                raise _lib.VitamdError(f"{what}: gradients must be fp32 ROCm device tensors on one device")
            continue
        _require(g, device, f"{what}: a gradient")
    grads = [g if g.is_contiguous() else g.contiguous() for g in grads]
    rows = np.zeros(len(grads), ROW_DTYPE)
    sizes = [g.numel() for g in grads]
    rows["first_chunk"], total = plan_chunks(sizes, _chunk_elems(L))
    rows["n"] = sizes
    rows["g"] = [g.data_ptr() for g in grads]
    return rows, total, device, grads


@torch.no_grad()
def grad_norm(parameters):
    """The global L2 norm of the gradients as a 0-dim device tensor (reading it is the caller's synchronisation).  Deterministic: the same
    gradients give the same bits on every call and every rank."""
    L = _lib.load()
    rows, total, device, grads = _grad_table(L, parameters, "grad_norm", copy_ok=True)
    if rows is None:
        return torch.zeros(())
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        return _norm(L, rows, _upload(rows, device), total, device, 0.0, stream)[0]


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm):
    """torch.nn.utils.clip_grad_norm_ (L2) without a host synchronisation: scales the gradients in place by min(1, max_norm / (norm + 1e-6))
    and returns the norm from before as a 0-dim device tensor.  Gradients must be contiguous."""
    max_norm = float(max_norm)
    if not max_norm > 0:
        raise ValueError("clip_grad_norm_: max_norm must be positive")
    L = _lib.load()
    rows, total, device, grads = _grad_table(L, parameters, "clip_grad_norm_", copy_ok=False)
    if rows is None:
        return torch.zeros(())
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        dev_rows = _upload(rows, device)
        norm_coef = _norm(L, rows, dev_rows, total, device, max_norm, stream)
        _lib.check(L.vitamd_mt_scale(rows.ctypes.data, dev_rows.data_ptr(), len(rows), total, norm_coef.data_ptr() + 4, stream), "mt_scale")
    return norm_coef[0]


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, multi_tensor=False, max_grad_norm=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameter")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("AdamW: max_grad_norm must be positive (None = no clipping)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.multi_tensor = bool(multi_tensor) or max_grad_norm is not None
        # of the last step on the multi-tensor path with clipping: 0-dim device tensors (reading one is the caller's synchronisation)
        self.grad_norm = None
        self.clip_coef = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.multi_tensor:
            self._step_multi()
        else:
            self._step_per_tensor()
        from .functions import WEIGHTS
        WEIGHTS.clear()   # the kernel updated the weights behind torch's version counters: drop the bf16 copies
        return loss

    def _state(self, p):
        st = self.state[p]
        if not st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        return st

    def _step_per_tensor(self):
        L = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.VitamdError("AdamW: parameters must be contiguous fp32 ROCm device tensors")
                st = self._state(p)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                code = L.vitamd_adamw_step_d(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                             p.numel(), float(group["lr"]), float(b1), float(b2), group["eps"], group["weight_decay"],
                                             int(st["step"]), stream)
                _lib.check(code, "adamw_step")

    def _step_multi(self):
        L = _lib.load()
        items = [(group, p) for group in self.param_groups for p in group["params"] if p.grad is not None]
        self.grad_norm = self.clip_coef = None
        if not items:
            return
        # everything is checked before anything is launched or any step count advances
        device = items[0][1].device
        for _, p in items:
            _require(p, device, "AdamW: a parameter")
            g = p.grad
            if not (g.is_cuda and g.dtype == torch.float32 and g.device == device):
                raise _lib.VitamdError("AdamW: gradients must be fp32 ROCm device tensors on the parameters' device")
            if g.is_contiguous() and g.data_ptr() % 16:
                raise _lib.VitamdError("AdamW: a gradient is not 16-byte aligned")
        states = [self._state(p) for _, p in items]
        for (_, p), st in zip(items, states):
            for key in ("exp_avg", "exp_avg_sq"):
                if st[key].shape != p.shape:
                    raise _lib.VitamdError(f"AdamW: {key} does not have its parameter's shape")
                _require(st[key], device, f"AdamW: {key}")
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for _, p in items]   # read only: p.grad is never rewritten
        rows = np.zeros(len(items), ROW_DTYPE)
        sizes = [p.numel() for _, p in items]
        rows["first_chunk"], total = plan_chunks(sizes, _chunk_elems(L))
        rows["n"] = sizes
        rows["p"] = [p.data_ptr() for _, p in items]
        rows["g"] = [g.data_ptr() for g in grads]
        rows["m"] = [st["exp_avg"].data_ptr() for st in states]
        rows["v"] = [st["exp_avg_sq"].data_ptr() for st in states]
        hyper, cols = {}, []
        for (group, _), st in zip(items, states):
            k = int(st["step"]) + 1
            key = (id(group), k)
            if key not in hyper:
                hyper[key] = hyper_row(float(group["lr"]), group["betas"], group["eps"], group["weight_decay"], k)
            cols.append(hyper[key])
        for name, col in zip(_HYPER, zip(*cols)):
            rows[name] = col
        for st in states:
            st["step"] += 1
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream().cuda_stream
            dev_rows = _upload(rows, device)
            coef = None
            if self.max_grad_norm is not None:
                norm_coef = _norm(L, rows, dev_rows, total, device, self.max_grad_norm, stream)
                self.grad_norm, self.clip_coef = norm_coef[0], norm_coef[1]
                coef = norm_coef.data_ptr() + 4
            _lib.check(L.vitamd_mt_adamw(rows.ctypes.data, dev_rows.data_ptr(), len(rows), total, coef, stream), "mt_adamw")
