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

The tokenizers have the same thing in ReconMetrics (per-image MSE, MAE, PSNR and SSIM of a reconstruction against its target) and
CodebookMetrics (the code-usage histogram), with evaluate_tokenizer on top (csrc/recon_metrics.hip).
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


# ------------------------------------------------------------------------------------------------ the tokenizers
class ReconMetrics:
    """Running per-image MSE, MAE, PSNR and SSIM of reconstructions against their targets (include/vitamd_eval.h vitamd_recon_metrics):

        m = ReconMetrics()                           # data_range 1: the tokenizers' images live in [0, 1]
        for x in val_batches:
            m.update(model(x)[0], x)                 # two launches, no host read
        r = m.result()                               # the only synchronisation: {"mse", "mae", "psnr", "ssim", "count"}

    `sums` fp64 [4] holds the sums over the images of mse_b, mae_b, psnr_b and ssim_b, `count` int64 [1] the images: plain sums, which a
    data-parallel user all_reduces before result().  The per-image scratch and the workspace are kept between updates and grown when a
    batch needs more; `rows()` gives the last update's per-image values."""

    def __init__(self, data_range=1.0, clamp=False, ssim=True, device=None):
        if isinstance(data_range, bool) or not isinstance(data_range, (int, float)) or not 0.0 < float(data_range) <= 3.0e38:
            raise ValueError(f"ReconMetrics: data_range must be a finite number above 0, got {data_range!r}")
        self.data_range, self.clamp, self.ssim = float(data_range), bool(clamp), bool(ssim)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.sums = torch.zeros((4,), dtype=torch.float64, device=self.device)
        self.count = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._per_image = self._ws = None
        self._last = 0

    def reset(self):
        self.sums.zero_()
        self.count.zero_()
        self._last = 0
        return self

    def update(self, recon, target):
        """recon fp32 or bf16 [B, C, H, W], target fp32 [B, C, H, W], contiguous, on the device: adds this batch, returns self"""
        if not isinstance(recon, torch.Tensor) or not isinstance(target, torch.Tensor) or recon.dim() != 4 or recon.shape != target.shape:
            raise ops._lib.VitamdError(f"ReconMetrics.update: expected recon and target of one shape [B, C, H, W], got "
                                       f"{tuple(getattr(recon, 'shape', ()))} and {tuple(getattr(target, 'shape', ()))}")
        if not recon.is_cuda or not target.is_cuda:
            raise ops._lib.VitamdError("ReconMetrics.update: expected ROCm device tensors (the HIP kernels are the only implementation)")
        if recon.device != self.device:
            raise ops._lib.VitamdError(f"ReconMetrics.update: recon on {recon.device}, the accumulators on {self.device}")
        B, C, H, W = (int(v) for v in recon.shape)
        with torch.cuda.device(self.device):
            need = ops.recon_metrics_ws_bytes(B, C, H, W, self.ssim)
        if self._per_image is None or self._per_image.shape[0] < B:
            self._per_image = torch.zeros((B, 4), dtype=torch.float64, device=self.device)
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = torch.zeros((need // 4,), dtype=torch.float32, device=self.device)
        ops.recon_metrics(recon, target, self.sums, self.count, self._per_image, self._ws, self.data_range, self.clamp, self.ssim)
        self._last = B
        return self

    def rows(self):
        """fp64 [B, 4] = (mse_b, mae_b, psnr_b, ssim_b) of the last update: a view of the scratch, overwritten by the next one"""
        if self._last == 0:
            raise RuntimeError("ReconMetrics.rows: no update since the last reset")
        return self._per_image[:self._last]

    def result(self):
        """The one call that synchronises: the means over the images, formed in fp64 on the host, and the count.  Nothing counted: NaN
        everywhere but count.  psnr is the mean of the per-image values (+inf as soon as one image is reproduced exactly)."""
        sums = self.sums.cpu().tolist()
        count = int(self.count.cpu()[0])
        if count == 0:
            nan = float("nan")
            return {"mse": nan, "mae": nan, "psnr": nan, "ssim": nan, "count": 0}
        return {"mse": sums[0] / count, "mae": sums[1] / count, "psnr": sums[2] / count, "ssim": sums[3] / count, "count": count}


def codebook_stats(hist, bad=0):
    """hist: the K integer counts of a code-usage histogram (a list or a tensor on any device) -> {"usage": the fraction of codes with
    a count above 0 (the reference loops' codebook_usage.sum() / codebook_size), "used", "dead": K - used, "entropy": -sum p ln p over
    p = hist / count, "perplexity": exp(entropy), "count": the ids counted, "bad": the ids outside [0, K)}, formed in fp64 on the host.
    Nothing counted: entropy and perplexity are NaN."""
    h = torch.as_tensor(hist).detach().cpu().to(torch.float64).reshape(-1)
    K = h.numel()
    count = int(h.sum())
    used = int((h > 0).sum())
    out = {"usage": used / K, "used": used, "dead": K - used, "count": count, "bad": int(bad)}
    if count == 0:
        out["entropy"] = out["perplexity"] = float("nan")
        return out
    p = h[h > 0] / float(count)
    entropy = max(0.0, float(-(p * p.log()).sum()))
    out["entropy"], out["perplexity"] = entropy, math.exp(entropy)
    return out


class CodebookMetrics:
    """Running code-usage histogram of a quantiser's ids (include/vitamd_eval.h vitamd_code_hist): `hist` int64 [codebook_size] and `bad`
    int64 [1] (ids outside [0, codebook_size)) on the device, plain sums.  update() is one launch and reads nothing back; result()
    reads hist once and forms usage, dead codes, entropy and perplexity on the host (codebook_stats)."""

    def __init__(self, codebook_size, device=None):
        if not isinstance(codebook_size, int) or isinstance(codebook_size, bool) or not 2 <= codebook_size <= ops.CODE_HIST_MAX_K:
            raise ValueError(f"CodebookMetrics: codebook_size must be an integer in 2 .. {ops.CODE_HIST_MAX_K}, got {codebook_size!r}")
        self.codebook_size = codebook_size
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.hist = torch.zeros((codebook_size,), dtype=torch.int64, device=self.device)
        self.bad = torch.zeros((1,), dtype=torch.int64, device=self.device)

    def reset(self):
        self.hist.zero_()
        self.bad.zero_()
        return self

    def update(self, ids):
        """ids: int64 of any shape on the device: adds their counts, returns self"""
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64:
            raise ops._lib.VitamdError(f"CodebookMetrics.update: expected int64 ids, got {getattr(ids, 'dtype', type(ids).__name__)}")
        if ids.is_cuda and ids.device != self.device:
            raise ops._lib.VitamdError(f"CodebookMetrics.update: ids on {ids.device}, the histogram on {self.device}")
        ops.code_hist(ids.contiguous() if ids.is_cuda else ids, self.hist, self.bad)
        return self

    def result(self):
        """The one call that synchronises -> codebook_stats(hist, bad)"""
        return codebook_stats(self.hist.cpu(), int(self.bad.cpu()[0]))


def _tokenizer_outputs(out):
    """(reconstruction or logits, int64 ids) from what a tokenizer's forward returns: (recon, ids, qloss) of TiTok / ViTVQGAN, or
    (decoded, result_dict) of train_tatitok.TiTok, whose ids are result_dict["min_encoding_indices"]"""
    if isinstance(out, (tuple, list)) and len(out) >= 2:
        if isinstance(out[1], dict) and "min_encoding_indices" in out[1]:
            return out[0], out[1]["min_encoding_indices"]
        if isinstance(out[1], torch.Tensor):
            return out[0], out[1]
    raise TypeError("evaluate_tokenizer: model(x) must return (reconstruction, ids, ...) or (reconstruction, {'min_encoding_indices': ids, ...})")


def evaluate_tokenizer(model, batches, recon=None, codes=None, patch=None):
    """The validation half of the tokenizer loops: the model in eval mode under torch.no_grad() over `batches` of fp32 images
    [B, C, H, W] or vitamd.data.Frames (whose fp32 target comes from materialise(patch, image=True).images(), as in train_step; patch:
    the encoder's patch size, so that one launch makes its rows and the target), every batch's reconstruction added to a ReconMetrics
    and its code ids to a CodebookMetrics (recon, codes: ones to continue; None: fresh ones, data_range 1, of model.config.codebook_size
    codes).  The host reads nothing before the final results -> the two result dicts merged ("count": images, "codes": ids counted).
    model.training is put back, also when a batch raises."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for x in batches:
                target = x if isinstance(x, torch.Tensor) else x.materialise(patch, image=True).images()
                image, ids = _tokenizer_outputs(model(x))
                if recon is None:
                    recon = ReconMetrics(device=target.device)
                if codes is None:
                    codes = CodebookMetrics(int(model.config.codebook_size), device=target.device)
                recon.update(image.contiguous(), target.contiguous())
                codes.update(ids)
    finally:
        model.train(was_training)
    if recon is None or codes is None:
        raise ValueError("evaluate_tokenizer: no batches")
    out = codes.result()
    out["codes"] = out.pop("count")
    out.update(recon.result())
    return out
