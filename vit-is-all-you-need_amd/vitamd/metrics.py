"""Evaluation on the device: mean loss, top-1 and top-k accuracy of a classifier or a next-token model, from
counters that never leave the device until they are asked for.

    m = ClassifyMetrics(topk=5)
    for images, labels in val_batches:
        m.update(model(images), labels)          # one row walk + one single-workgroup sum (csrc/loss.hip): no host read, no fp32 copy
    r = m.result()                               # the only synchronisation: {"loss", "top1", "topk", "count", "perplexity"}

`update` reads the logits once, in the dtype they have (fp32 or bf16), so the bf16 logits of the fused head go straight in.  Both
accumulators are plain sums (`loss_sum` fp64 [1], `counts` int64 [3] = rows, top-1 hits, top-k hits): a data-parallel user adds them
across ranks with one all_reduce each before `result()`.  An update only enqueues two launches on the current stream, so a whole
validation step records into a graph.
"""
from __future__ import annotations

import math

import torch

from . import ops
from .lm import _rows, _target


class ClassifyMetrics:
    """Running loss / top-1 / top-k over the rows whose target is not ignore_index.  The per-row scratch (loss_row fp32, rank int32) is
    kept between updates and grown when a batch has more rows; `rows()` gives the last update's part of it."""

    def __init__(self, topk=5, ignore_index=-100, device=None):
        if not isinstance(topk, int) or isinstance(topk, bool) or topk < 1:
            raise ValueError(f"ClassifyMetrics: topk must be a positive integer, got {topk!r}")
        self.topk, self.ignore_index = topk, int(ignore_index)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.loss_sum = torch.zeros((1,), dtype=torch.float64, device=self.device)
        self.counts = torch.zeros((3,), dtype=torch.int64, device=self.device)
        self._loss_row = self._rank = None
        self._last = 0

    def reset(self):
        self.loss_sum.zero_()
        self.counts.zero_()
        self._last = 0
        return self

    def update(self, logits, target):
        """logits [..., V] fp32 or bf16 on the device, target int64 [...] (the hard labels): adds this batch, returns self"""
        if type(target).__name__ == "MixedLabels":
            raise TypeError("ClassifyMetrics.update: a MixedLabels target describes a mixed training batch; accuracy is defined on the hard "
                            "labels - evaluate on unmixed batches (a loader with train=False) and pass their int64 labels")
        if not isinstance(logits, torch.Tensor) or logits.dim() < 1:
            raise ops._lib.VitamdError("logits: expected a tensor [..., V]")
        V = logits.shape[-1]
        if 2 <= V <= ops.CE_MAX_V and self.topk > V:
            raise ValueError(f"ClassifyMetrics.update: topk = {self.topk} exceeds the {V} classes of these logits")
        x = _rows(logits)
        M = x.shape[0]
        t = _target(target, M)
        ops._need_logits(x)
        if x.device != self.device:
            raise ops._lib.VitamdError(f"ClassifyMetrics.update: logits on {x.device}, the accumulators on {self.device}")
        if self._loss_row is None or self._loss_row.numel() < M:
            self._loss_row = torch.zeros((M,), dtype=torch.float32, device=self.device)
            self._rank = torch.zeros((M,), dtype=torch.int32, device=self.device)
        ops.classify_metrics(x, t, self.loss_sum, self.counts, self.topk, self.ignore_index, self._loss_row, self._rank)
        self._last = M
        return self

    def rows(self):
        """(loss_row fp32 [M], rank int32 [M]) of the last update: views of the scratch, overwritten by the next one.  rank: how many
        other classes rank above the target (0 = the argmax), -1 for an ignored row"""
        if self._last == 0:
            raise RuntimeError("ClassifyMetrics.rows: no update since the last reset")
        return self._loss_row[:self._last], self._rank[:self._last]

    def result(self):
        """The one call that synchronises: {"loss": loss_sum / count (formed in fp64 on the host), "top1", "topk": fractions of count,
        "count": the rows counted, "perplexity": exp(loss)}.  Nothing counted: NaN everywhere but count."""
        loss_sum = float(self.loss_sum.cpu()[0])
        count, top1, topk = (int(v) for v in self.counts.cpu())
        if count == 0:
            nan = float("nan")
            return {"loss": nan, "top1": nan, "topk": nan, "count": 0, "perplexity": nan}
        loss = loss_sum / count
        try:
            ppl = math.exp(loss)
        except OverflowError:
            ppl = float("inf")
        return {"loss": loss, "top1": top1 / count, "topk": topk / count, "count": count, "perplexity": ppl}
