"""Fused AdamW on the HIP path: same constructor arguments and update
rule as the reference's `torch.optim.AdamW` (train_vit.py:82), state kept in fp32.  Works with
`utils.get_lr_scheduler` (it is a torch.optim.Optimizer).

Two paths with the same arithmetic, element for element.  The default is one kernel per parameter tensor.  `multi_tensor=True` (implied by
`max_grad_norm`) walks a row table in device memory instead, one row per tensor with a gradient: the whole step is one launch, or three
with gradient-norm clipping (per-chunk sums of squares, one workgroup that derives the norm and the clip coefficient in a fixed order,
then the update, which reads the coefficient from device memory: no host synchronisation, the same bits on every rank).  `grad_norm` and
`clip_grad_norm_` give the norm and the in-place clip to users of other optimisers.  DESIGN.md section 12.

`capturable=True` keeps that table in device memory from step to step.  What changes with the step - the learning rate and the two bias
corrections - is rewritten by one more small launch from a device-resident step counter and schedule position (vitamd_sched_advance), so
`step()` uploads nothing, allocates nothing and reads nothing back: it can be recorded in a graph (vitamd.graph.GraphedTrainStep records
the whole iteration).  `schedule=(warmup_steps, train_steps, min_lr)` is the schedule of utils.get_lr_scheduler evaluated there; the
host keeps mirrors (`state[p]["step"]`, `group["lr"]`, `group["sched_t"]`) that need no device read.  DESIGN.md section 12.1."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import lib as _lib

# The record layouts of include/vitamd.h, hand-written because the code below indexes them by field name; tests/test_abi_parser_host.py has the
# compiler compare every offset and size with the header's structs.
# struct vitamd_mt_row
ROW_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("first_chunk", "<i4"), ("lr", "<f4"),
                      ("weight_decay", "<f4"), ("beta1", "<f4"), ("one_minus_beta1", "<f4"), ("beta2", "<f4"), ("one_minus_beta2", "<f4"),
                      ("eps", "<f4"), ("inv_bc1", "<f4"), ("inv_sqrt_bc2", "<f4")])
# struct vitamd_sched_row
SCHED_DTYPE = np.dtype([("step", "<i8"), ("sched_t", "<i8"), ("base_lr", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"), ("min_ratio", "<f8"),
                        ("warmup_steps", "<i8"), ("train_steps", "<i8")])
# struct vitamd_cast_desc (functions.WeightCache.prepare fills it)
CAST_DTYPE = np.dtype([("w", "<u8"), ("wb", "<u8"), ("wbt", "<u8"), ("N", "<i4"), ("K", "<i4"), ("first_tile", "<i4"), ("tiles_k", "<i4")])
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


def check_schedule(schedule):
    """(warmup_steps, train_steps, min_lr) of utils.get_lr_scheduler -> the tuple with plain ints and a float; anything else: ValueError"""
    try:
        warmup, train, min_lr = schedule
    except (TypeError, ValueError):
        raise ValueError("AdamW: schedule is (warmup_steps, train_steps, min_lr), the arguments of utils.get_lr_scheduler") from None
    for name, v, least in (("warmup_steps", warmup, 0), ("train_steps", train, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
            raise ValueError(f"AdamW: schedule {name} must be an integer >= {least}, got {v!r}")
    if isinstance(min_lr, bool) or not isinstance(min_lr, (int, float)) or not (0 <= min_lr < math.inf):
        raise ValueError(f"AdamW: schedule min_lr must be a finite number >= 0, got {min_lr!r}")
    return int(warmup), int(train), float(min_lr)


def lr_factor(step, warmup_steps, train_steps, min_ratio):
    """utils.lr_factor (the package does not import the training scripts' module): the reference's SequentialLR in closed form."""
    if step < warmup_steps:
        return min(1.0, step / warmup_steps)
    if step < train_steps:
        return min_ratio + (1.0 - min_ratio) * (1.0 + math.cos(math.pi * (step - warmup_steps) / train_steps)) / 2.0
    return 1.0


class _Table:
    """The resident table of a capturable AdamW: host copies, device buffers, and what they were built from."""
    __slots__ = ("items", "states", "rows", "sched", "dev_rows", "dev_sched", "partials", "norm_coef", "total", "device", "ptrs", "hypers",
                 "bound", "uploaded")


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, multi_tensor=False, max_grad_norm=None,
                 capturable=False, schedule=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameter")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("AdamW: max_grad_norm must be positive (None = no clipping)")
        if schedule is not None:
            if not capturable:
                raise ValueError("AdamW: schedule= is evaluated on the device and needs capturable=True (else use utils.get_lr_scheduler)")
            schedule = check_schedule(schedule)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.capturable = bool(capturable)
        self.schedule = schedule
        self.multi_tensor = bool(multi_tensor) or max_grad_norm is not None or self.capturable
        # of the last step on the multi-tensor path with clipping: 0-dim device tensors (reading one is the caller's synchronisation);
        # capturable: views of the resident {norm, coef} buffer, rewritten by every step
        self.grad_norm = None
        self.clip_coef = None
        self._table = None
        if self.capturable:
            self._seed_groups()

    def __setattr__(self, name, value):
        # torch's LR schedulers wrap `optimizer.step` on construction: the one place to refuse them before they rewrite group["lr"]
        if name == "step" and self.__dict__.get("schedule") is not None:
            raise ValueError("AdamW(schedule=...) evaluates its learning-rate schedule on the device: do not attach a torch LR scheduler "
                             "(param_groups[g]['lr'] already follows the schedule)")
        super().__setattr__(name, value)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.capturable:
            self._step_resident()
        elif self.multi_tensor:
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

    # ------------------------------------------------------------------------------------------ capturable: the resident table
    # The table, its schedule array, `partials` and {norm, coef} are built and uploaded when something they were built from has changed -
    # an address (p, p.grad, exp_avg, exp_avg_sq), the set of parameters that have a gradient, a hyper-parameter, a loaded state dict - and
    # otherwise only launched over.  The host's copy of the addresses is what is compared, before every launch.
    def _base_lr(self, group):
        return float(group["initial_lr"] if self.schedule is not None else group["lr"])

    def _sched_fields(self, group):
        """(warmup_steps, train_steps, min_ratio) of a group; train_steps == 0: its lr is constant"""
        if self.schedule is None:
            return 0, 0, 0.0
        warmup, train, min_lr = self.schedule
        base = self._base_lr(group)
        return warmup, train, (min_lr / base if base else 0.0)

    def _lr_at(self, group, t):
        """what a LambdaLR over utils.lr_factor leaves in group["lr"] at schedule position t"""
        if self.schedule is None:
            return group["lr"]
        return self._base_lr(group) * lr_factor(t, *self._sched_fields(group))

    def _seed_groups(self):
        """The base rate (under LambdaLR's key, `initial_lr`), the schedule position and the lr mirror of every group that lacks them.  A
        group that arrives without a position (a state dict of another optimiser) is taken to be where its parameters' step counts are."""
        for group in self.param_groups:
            if self.schedule is not None:
                group.setdefault("initial_lr", group["lr"])
            if "sched_t" not in group:
                group["sched_t"] = max((int(self.state[p]["step"]) for p in group["params"] if p in self.state and "step" in self.state[p]),
                                       default=0)
            group["lr"] = self._lr_at(group, group["sched_t"])
        self._lr_mirror = [group["lr"] for group in self.param_groups]

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if self.__dict__.get("capturable"):
            self._seed_groups()
            self._table = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._table = None                                   # the moments are new tensors and the counters are re-seeded from the loaded steps
        if self.capturable:
            self._seed_groups()

    def _hypers(self):
        return tuple((self._base_lr(g), float(g["betas"][0]), float(g["betas"][1]), g["eps"], g["weight_decay"]) for g in self.param_groups)

    def _check_lr(self):
        if self.schedule is not None and [g["lr"] for g in self.param_groups] != self._lr_mirror:
            raise ValueError("AdamW(schedule=...): param_groups[g]['lr'] was changed from outside (a torch LR scheduler?); the schedule "
                             "runs on the device from group['initial_lr'] and group['sched_t']")

    def _live(self):
        """(group, parameter) of everything that has a gradient now, and the four addresses of each"""
        items, ptrs = [], []
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                items.append((group, p))
                st = self.state[p] if p in self.state else None
                ptrs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr() if st else 0, st["exp_avg_sq"].data_ptr() if st else 0))
        return items, ptrs

    def _build(self, items=None, bind=True):
        """The host copies and the device buffers of `items` (default: every parameter that has a gradient).  bind=False leaves the
        gradient addresses and the upload to _bind() / _upload_table(): GraphedTrainStep learns them only while it records backward."""
        L = _lib.load()
        if items is None:
            items, _ = self._live()
        self._table = None
        if not items:
            return None
        device = items[0][1].device
        for _, p in items:
            _require(p, device, "AdamW: a parameter")
        states = [self._state(p) for _, p in items]
        for (_, p), st in zip(items, states):
            for key in ("exp_avg", "exp_avg_sq"):
                if st[key].shape != p.shape:
                    raise _lib.VitamdError(f"AdamW: {key} does not have its parameter's shape")
                _require(st[key], device, f"AdamW: {key}")
            st["step"] = int(st["step"])                     # a loaded torch state holds a tensor: the mirror is a Python int
        assert SCHED_DTYPE.itemsize == L.vitamd_sched_row_bytes(), "vitamd_sched_row: the binding and the library disagree on the layout"
        t = _Table()
        t.items, t.states, t.device = items, states, device
        rows, sched = np.zeros(len(items), ROW_DTYPE), np.zeros(len(items), SCHED_DTYPE)
        sizes = [p.numel() for _, p in items]
        rows["first_chunk"], t.total = plan_chunks(sizes, _chunk_elems(L))
        rows["n"] = sizes
        rows["p"] = [p.data_ptr() for _, p in items]
        rows["m"] = [st["exp_avg"].data_ptr() for st in states]
        rows["v"] = [st["exp_avg_sq"].data_ptr() for st in states]
        cols, fields = [], []
        for (group, _), st in zip(items, states):
            base = self._base_lr(group)
            # lr and the bias corrections are placeholders (those of the next step at the base rate): the advance kernel rewrites them
            cols.append(hyper_row(base, group["betas"], group["eps"], group["weight_decay"], st["step"] + 1))
            warmup, train, ratio = self._sched_fields(group)
            fields.append((st["step"], int(group["sched_t"]), base, float(group["betas"][0]), float(group["betas"][1]), ratio, warmup, train))
        for name, col in zip(_HYPER, zip(*cols)):
            rows[name] = col
        for name, col in zip(SCHED_DTYPE.names, zip(*fields)):
            sched[name] = col
        t.rows, t.sched, t.hypers = rows, sched, self._hypers()
        with torch.cuda.device(device):
            t.dev_rows = torch.empty(rows.nbytes, dtype=torch.uint8, device=device)
            t.dev_sched = torch.empty(sched.nbytes, dtype=torch.uint8, device=device)
            t.partials = torch.empty(t.total, dtype=torch.float32, device=device)
            t.norm_coef = torch.empty(2, dtype=torch.float32, device=device)
        t.ptrs, t.bound, t.uploaded = None, False, False
        self._table = t
        if bind:
            self._bind()
            self._upload_table()
        return t

    def _bind(self):
        """Host work only: the gradient addresses into the host rows, checked; every row must have one"""
        t = self._table
        grads = []
        for _, p in t.items:
            g = p.grad
            if g is None:
                raise _lib.VitamdError("AdamW(capturable=True): a parameter of the resident table has no gradient")
            if not g.is_contiguous():
                raise _lib.VitamdError("AdamW(capturable=True): a gradient is not contiguous (a copy would move with every step)")
            _require(g, t.device, "AdamW: a gradient")
            grads.append(g)
        t.rows["g"] = [g.data_ptr() for g in grads]
        t.ptrs = [(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
                  for (_, p), g, st in zip(t.items, grads, t.states)]
        t.bound = True

    def _upload_table(self):
        """Both arrays to their device buffers on the current stream (never inside a capture)"""
        t = self._table
        if not t.bound:
            raise _lib.VitamdError("AdamW(capturable=True): the table has no gradient addresses yet")
        with torch.cuda.device(t.device):
            t.dev_rows.copy_(torch.from_numpy(t.rows.view(np.uint8)).pin_memory(), non_blocking=True)
            t.dev_sched.copy_(torch.from_numpy(t.sched.view(np.uint8)).pin_memory(), non_blocking=True)
        t.uploaded = True

    def _enqueue(self, stream):
        """The launches of one step over the resident table: advance, [sum of squares + finish], update.  Nothing else reaches the device."""
        L, t = _lib.load(), self._table
        n = len(t.rows)
        _lib.check(L.vitamd_sched_advance(t.dev_rows.data_ptr(), t.dev_sched.data_ptr(), n, stream), "sched_advance")
        coef = None
        if self.max_grad_norm is not None:
            _lib.check(L.vitamd_mt_sumsq(t.rows.ctypes.data, t.dev_rows.data_ptr(), n, t.total, t.partials.data_ptr(), t.norm_coef.data_ptr(),
                                         self.max_grad_norm, stream), "mt_sumsq")
            self.grad_norm, self.clip_coef = t.norm_coef[0], t.norm_coef[1]
            coef = t.norm_coef.data_ptr() + 4
        _lib.check(L.vitamd_mt_adamw(t.rows.ctypes.data, t.dev_rows.data_ptr(), n, t.total, coef, stream), "mt_adamw")

    def _advance_mirrors(self):
        """What the step just launched (or replayed) did to the counters, on the host: no device read"""
        for st in self._table.states:
            st["step"] += 1
        for group in self.param_groups:
            group["sched_t"] += 1
            group["lr"] = self._lr_at(group, group["sched_t"])
        self._lr_mirror = [group["lr"] for group in self.param_groups]

    def _table_is_current(self, ptrs):
        t = self._table
        return t is not None and t.uploaded and t.ptrs == ptrs and t.hypers == self._hypers()

    def _step_resident(self):
        self._check_lr()
        items, ptrs = self._live()
        if not items:
            self.grad_norm = self.clip_coef = None
            return
        if not self._table_is_current(ptrs):
            if items[0][1].is_cuda and torch.cuda.is_current_stream_capturing():
                raise _lib.VitamdError("AdamW(capturable=True): the resident table does not match the parameters, gradients and moments of "
                                       "this step, and it cannot be rebuilt while a stream capture is recording (step once eagerly first)")
            self.grad_norm = self.clip_coef = None
            self._build(items)
        t = self._table
        with torch.cuda.device(t.device):
            self._enqueue(torch.cuda.current_stream().cuda_stream)
        self._advance_mirrors()

    def warm_launches(self, device):
        """The launches of a step once, on the current stream, over a throw-away table of four floats: code objects are loaded and
        first-launch attributes set before a capture records the same launches."""
        L = _lib.load()
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream().cuda_stream
            p, g, m, v = (torch.zeros(4, dtype=torch.float32, device=device) for _ in range(4))
            rows, sched = np.zeros(1, ROW_DTYPE), np.zeros(1, SCHED_DTYPE)
            rows["n"], rows["p"], rows["g"], rows["m"], rows["v"] = 4, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            for name, x in zip(_HYPER, hyper_row(0.0, (0.9, 0.999), 1e-8, 0.0, 1)):
                rows[name] = x
            sched["beta1"], sched["beta2"] = 0.9, 0.999
            dev_rows, dev_sched = _upload(rows, device), _upload(sched, device)
            _lib.check(L.vitamd_sched_advance(dev_rows.data_ptr(), dev_sched.data_ptr(), 1, stream), "sched_advance")
            norm_coef = None
            if self.max_grad_norm is not None:
                norm_coef = _norm(L, rows, dev_rows, 1, device, self.max_grad_norm, stream)
            _lib.check(L.vitamd_mt_adamw(rows.ctypes.data, dev_rows.data_ptr(), 1, 1, None if norm_coef is None else norm_coef.data_ptr() + 4,
                                         stream), "mt_adamw")
