"""Poisoned allocations: run the package with every uninitialised buffer filled with 0xFF bytes and demand the same bits.

Plain torch; importable without a GPU and without the library.  The kernel-level tests fill the "may be anything" regions of a single
call with NaN.  This harness checks the layer above them, the wrappers of vitamd/*.py that decide whether a kernel gets `torch.empty`
or `torch.zeros`: a workload is run clean and then inside `poisoned()`, where every buffer the wrappers leave uninitialised holds
poison, and `compare()` demands equal bit patterns.  A wrapper that hands an uninitialised buffer to an accumulating kernel, reads a
row a launch skipped, or relies on what a reused scratch held, changes the result (NaN spreads through sums; -1 is outside every
integer input's range, so the kernels skip it instead of forming an address from it).

The poison is the value whose every byte is 0xFF: a NaN for every floating type, -1 for signed integers, the maximum for unsigned
ones; bool gets True.
"""
from __future__ import annotations

import ast
import contextlib
import glob
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "vit-is-all-you-need_amd", "vitamd")

PATCHED = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"),
           (torch.Tensor, "new_empty"), (torch.Tensor, "new_empty_strided"))
EMPTY_NAMES = ("empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided")
_INT_OF_SIZE = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_active = False


def poison_(t):
    """Fill `t` in place with 0xFF bytes (bool: True).  meta tensors and tensors without elements are left alone.  One fill kernel and
    no host-to-device copy, so it may run inside a stream capture."""
    if not isinstance(t, torch.Tensor) or t.is_meta or t.numel() == 0:
        return t
    with torch.no_grad():
        if t.dtype == torch.bool:
            t.fill_(True)
        elif t.dtype.is_complex:
            poison_(torch.view_as_real(t))
        elif t.dtype == torch.uint8:
            t.fill_(255)
        else:
            t.view(_INT_OF_SIZE[t.element_size()]).fill_(-1)       # a same-size view exists for every stride pattern
    return t


def _in_package(filename):
    return os.path.basename(os.path.dirname(os.path.abspath(filename))) == "vitamd"


def _wrap(orig, log):
    def poisoning(*args, **kwargs):
        out = poison_(orig(*args, **kwargs))
        if log is not None and isinstance(out, torch.Tensor) and not out.is_meta and out.numel():
            frame = sys._getframe(1)
            if _in_package(frame.f_code.co_filename):
                log.append((os.path.basename(frame.f_code.co_filename), frame.f_lineno, tuple(out.shape), out.dtype))
        return out
    poisoning.__name__ = getattr(orig, "__name__", "empty")
    poisoning.__wrapped__ = orig
    return poisoning


@contextlib.contextmanager
def poisoned(log=None):
    """While active, torch.empty / empty_like / empty_strided and Tensor.new_empty / new_empty_strided return their tensor filled with
    poison.  log: a list; every poisoned allocation made from a file of vitamd/ is appended as (file basename, line, shape, dtype).
    The originals are put back on exit, also when the body raises; nesting raises RuntimeError."""
    global _active
    if _active:
        raise RuntimeError("poisoned() is already active: it does not nest")
    saved = [(owner, name, getattr(owner, name), name in vars(owner)) for owner, name in PATCHED]
    _active = True
    try:
        for owner, name, orig, _ in saved:
            setattr(owner, name, _wrap(orig, log))
        yield log
    finally:
        for owner, name, orig, own in saved:
            if own:
                setattr(owner, name, orig)
            else:
                delattr(owner, name)      # inherited (Tensor.new_empty lives on the C base class): uncover it again
        _active = False


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v)


def dirty_scratch(*holders):
    """Poison every long-lived scratch tensor the package keeps between calls; returns how many tensors were filled.

    Found by reading vitamd/*.py:
      - ops._WORKSPACES: the split-K / decode workspace of every (device, stream), always;
      - the resident table of a multi-tensor optimiser (`optim.AdamW._table`, also reachable as `GraphedTrainStep._table`): its
        `partials` and `norm_coef` - pass the optimiser, the graphed step or the table;
      - `PerceptualLoss.prepared()["scratch"]`: the dgamma / dbeta sinks of the frozen network's affine LayerNorms - pass the
        PerceptualLoss, the dict `prepared()` returns, or its "scratch" entry.
    Everything else that outlives a call holds VALUES and is left alone: functions.WEIGHTS and functions._PADDED (bf16 weight copies),
    perceptual._TABLES and data._TABLES (band and normalisation tables), the optimiser table's dev_rows / dev_sched (addresses and
    hyper-parameters), the static input, token and output buffers of the graphed steps, a KVCache (its contents are the model's
    state; a fresh one is torch.empty and poisoned by `poisoned()` itself), the loader's staging slots, the per-layer gradient
    buckets of vitamd.ddp's GradSink (they ARE the gradients until the all-reduce has read them; multi-GPU, not exercised here)."""
    n = 0
    ops = sys.modules.get("vitamd.ops")
    targets = list(ops._WORKSPACES.values()) if ops is not None else []
    for h in holders:
        if h is None:
            continue
        table = getattr(h, "_table", None)
        if table is None and hasattr(h, "partials"):
            table = h
        if table is not None:
            targets += [table.partials, table.norm_coef]
            continue
        if hasattr(h, "prepared"):
            h = h.prepared()
        if isinstance(h, dict) and "scratch" in h:
            h = h["scratch"]
        targets += list(_tensors(h))
    for t in targets:
        if isinstance(t, torch.Tensor):
            poison_(t)
            n += 1
    return n


def _bits(t):
    """an integer view of the tensor's bytes (bool and integers as they are)"""
    t = t.detach().contiguous()
    if t.dtype.is_complex:
        t = torch.view_as_real(t).contiguous()
    if t.dtype.is_floating_point or t.dtype in (torch.uint16, torch.uint32, torch.uint64):
        return t.view(_INT_OF_SIZE[t.element_size()])
    return t


def _first(mask):
    """index of the first True of a mask, as a tuple"""
    flat = int(torch.nonzero(mask.reshape(-1))[0])
    return tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), mask.shape)) if mask.dim() else ()


def compare(clean, dirty, exact):
    """clean, dirty: dicts of tensors with the same keys.  Keys in `exact` must have equal bit patterns (integer views: -0 against +0
    and NaN against NaN cannot hide); the others must be finite in `dirty` wherever they are in `clean`.  -> list of failure strings,
    each naming the key and the first differing index."""
    failures = []
    if set(clean) != set(dirty):
        failures.append(f"keys differ: only clean {sorted(set(clean) - set(dirty))}, only dirty {sorted(set(dirty) - set(clean))}")
    unknown = set(exact) - set(clean)
    if unknown:
        failures.append(f"exact names keys that do not exist: {sorted(unknown)}")
    for key in clean:
        if key not in dirty:
            continue
        a, b = clean[key], dirty[key]
        if tuple(a.shape) != tuple(b.shape) or a.dtype != b.dtype:
            failures.append(f"{key}: {a.dtype} {tuple(a.shape)} became {b.dtype} {tuple(b.shape)}")
            continue
        if a.numel() == 0:
            continue
        a, b = a.detach().cpu(), b.detach().cpu()
        if key in exact:
            bad = _bits(a) != _bits(b)
            if bool(bad.any()):
                i = _first(bad)
                failures.append(f"{key}: {int(bad.sum())} of {bad.numel()} elements differ in their bits, first at {i}: "
                                f"{a[i].item()!r} became {b[i].item()!r}")
        elif a.dtype.is_floating_point or a.dtype.is_complex:
            bad = torch.isfinite(a) & ~torch.isfinite(b)
            if bool(bad.any()):
                i = _first(bad)
                failures.append(f"{key}: {int(bad.sum())} of {bad.numel()} finite elements became non-finite, first at {i}: "
                                f"{a[i].item()!r} became {b[i].item()!r}")
    return failures


def site_spans(source=None):
    """{(file basename, first line): last line} of every torch.empty / empty_like / empty_strided / new_empty / new_empty_strided call:
    in `source` (a string; the file is then "<string>") or in every vitamd/*.py."""
    if source is not None:
        texts = [("<string>", source)]
    else:
        texts = []
        for path in sorted(glob.glob(os.path.join(PKG_DIR, "*.py"))):
            with open(path) as f:
                texts.append((os.path.basename(path), f.read()))
    spans = {}
    for name, text in texts:
        for node in ast.walk(ast.parse(text)):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in EMPTY_NAMES:
                spans[(name, node.lineno)] = max(spans.get((name, node.lineno), 0), node.end_lineno)
    return spans


def empty_sites(source=None):
    """The set of (file basename, line) of every such call, found with `ast`"""
    return set(site_spans(source))


def sites_hit(log, spans=None):
    """The sites of `spans` (default: the package's) the entries of a poisoned() log fall into: a call that spans several lines is hit
    by a frame line anywhere inside it."""
    spans = site_spans() if spans is None else spans
    lines = {(entry[0], entry[1]) for entry in log}
    return {(name, first) for (name, first), last in spans.items()
            if any((name, line) in lines for line in range(first, last + 1))}
