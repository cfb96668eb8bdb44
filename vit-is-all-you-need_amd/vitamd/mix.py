"""Mixup, CutMix and label smoothing for ViT training: the second half of the DeiT / timm recipe, fused into the
device input feed (csrc/input.hip, vitamd_frames_prep_mix) and the loss (csrc/loss.hip, vitamd_soft_cross_entropy_fwd / _bwd).

    mix = Mix(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1)
    loader = MixLoader(host_iter, "cuda", 224, mix, patch=16, image=False)     # yields (MixedFrames, MixedLabels)
    loss_fn = SoftTargetLoss(mix.label_smoothing)
    for frames, labels in loader:
        loss = train_vit.train_step(model, frames, labels, optim, loss_fn=loss_fn)
    loader = ResizeMixLoader(host_iter, "cuda", 224, mix, mode="rrc", patch=16, image=False)      # RandomResizedCrop AND the mix, one launch

What is mixed is decided on the HOST, from a counter-based generator keyed by (seed, step): a record of six integers and one float
per sample, which crosses to the device through a pinned buffer.  The prep kernel then cuts sample b and its partner, each with its
own crop and flip, and blends or pastes them on the way to the patch rows: the fp32 batch, the three torch passes over it and the
im2col behind them do not exist.  The loss takes the two label vectors and lam as they are; no [B, classes] target is built."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import data, lm, ops, resize

MODE_NONE, MODE_MIXUP, MODE_CUTMIX = 0, 1, 2


class Mix:
    """The draw of timm's Mixup: mixup_alpha / cutmix_alpha are the Beta parameters (0 disables that mode), prob the chance that a
    batch (or, per_sample=True, a sample) is mixed at all, switch_prob the chance of CutMix when both modes are enabled.  The partner
    of sample b is sample B-1-b (the batch reversed).  label_smoothing is carried for the loss (SoftTargetLoss); the draw ignores it."""

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=False, label_smoothing=0.1, seed=0):
        for name, v in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v) or v < 0:
                raise ValueError(f"Mix: {name} must be a finite number >= 0, got {v!r}")
        for name, v in (("prob", prob), ("switch_prob", switch_prob), ("label_smoothing", label_smoothing)):
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not 0.0 <= v <= 1.0:
                raise ValueError(f"Mix: {name} must lie in [0, 1], got {v!r}")
        if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 64:
            raise ValueError(f"Mix: seed must be an integer in [0, 2^64), got {seed!r}")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.per_sample = float(prob), float(switch_prob), bool(per_sample)
        self.label_smoothing, self.seed = float(label_smoothing), seed

    @property
    def enabled(self):
        return self.prob > 0 and (self.mixup_alpha > 0 or self.cutmix_alpha > 0)

    def _decide(self, rng, H, W):
        """one decision -> (mode, yl, yh, xl, xh, lam as a Python float); all in float64 / Python integers"""
        u_mix, u_switch = rng.random(), rng.random()
        if not self.enabled or not u_mix < self.prob:
            return MODE_NONE, 0, 0, 0, 0, 1.0
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            mode = MODE_CUTMIX if u_switch < self.switch_prob else MODE_MIXUP
        else:
            mode = MODE_MIXUP if self.mixup_alpha > 0 else MODE_CUTMIX
        alpha = self.mixup_alpha if mode == MODE_MIXUP else self.cutmix_alpha
        lam0 = float(rng.beta(alpha, alpha))
        if mode == MODE_MIXUP:
            return mode, 0, 0, 0, 0, lam0
        r = math.sqrt(1.0 - lam0)
        ch, cw = int(H * r), int(W * r)
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        yl, yh = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
        xl, xh = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
        return mode, yl, yh, xl, xh, 1.0 - (yh - yl) * (xh - xl) / (H * W)

    def draw(self, B, hw, step):
        """-> (rec int32 [B, 6] = (partner, mode, yl, yh, xl, xh), lam fp32 [B]) on the CPU, from numpy's Philox keyed by (seed, step):
        the same (seed, step) gives the same record, and no device value is read.  Mixup rows: lam ~ Beta(alpha, alpha), the box is
        zeros.  CutMix rows: the box of timm's rand_bbox around a uniform centre, clipped to the image, and lam = 1 - its area / (H W)
        (rounded once, to fp32).  Unmixed rows: mode 0, lam = 1."""
        H, W = data._hw(hw)
        if not isinstance(B, int) or isinstance(B, bool) or B < 1:
            raise ValueError(f"Mix.draw: B must be a positive integer, got {B!r}")
        if not isinstance(step, int) or isinstance(step, bool) or not 0 <= step < 1 << 64:
            raise ValueError(f"Mix.draw: step must be an integer in [0, 2^64), got {step!r}")
        rng = np.random.Generator(np.random.Philox(key=np.array([self.seed, step], dtype=np.uint64)))
        rows = [self._decide(rng, H, W) for _ in range(B)] if self.per_sample else [self._decide(rng, H, W)] * B
        rec = torch.tensor([[B - 1 - b, *row[:5]] for b, row in enumerate(rows)], dtype=torch.int32)
        lam = torch.tensor([row[5] for row in rows], dtype=torch.float64).to(torch.float32)
        return rec, lam


class MixedLabels:
    """The labels of a mixed batch: a, b int64 [B] (b = a[partner]) and lam fp32 [B] on the device; row m's target is
    lam[m] * onehot(a[m]) + (1 - lam[m]) * onehot(b[m])."""

    def __init__(self, a, b, lam):
        self.a, self.b, self.lam = a, b, lam

    @classmethod
    def of(cls, labels, pair):
        """the labels of a batch mixed by pair = (rec, lam) on the device: b = labels[partner]"""
        rec, lam = pair
        return cls(labels, labels[rec[:, 0].long()], lam)

    def __iter__(self):
        return iter((self.a, self.b, self.lam))


class SoftTargetLoss:
    """loss_fn of train_vit.train_step: lm.soft_cross_entropy with this label smoothing, on an int64 label tensor or on MixedLabels."""

    def __init__(self, smoothing=0.0):
        if not isinstance(smoothing, (int, float)) or isinstance(smoothing, bool) or not 0.0 <= smoothing <= 1.0:
            raise ValueError(f"SoftTargetLoss: smoothing must lie in [0, 1], got {smoothing!r}")
        self.smoothing = float(smoothing)

    def __call__(self, logits, labels):
        if isinstance(labels, MixedLabels):
            return lm.soft_cross_entropy(logits, labels.a, labels.b, labels.lam, self.smoothing)
        return lm.soft_cross_entropy(logits, labels, smoothing=self.smoothing)


def _need_mix(mix, B, who):
    """the (rec, lam) pair of a mixed batch of B samples, checked"""
    if not (isinstance(mix, (tuple, list)) and len(mix) == 2):
        raise ValueError(f"{who}: mix must be (rec int32 [B, 6], lam fp32 [B])")
    rec, lam = mix
    if not isinstance(rec, torch.Tensor) or rec.dtype != torch.int32 or tuple(rec.shape) != (B, 6):
        raise ValueError(f"{who}: rec must be int32 [{B}, 6]")
    if not isinstance(lam, torch.Tensor) or lam.dtype != torch.float32 or tuple(lam.shape) != (B,):
        raise ValueError(f"{who}: lam must be fp32 [{B}]")
    return rec, lam


class _Mixed:
    """what the two mixed frames classes share: the checked pair on the device, held once their base constructor has run"""

    def _hold_mix(self, mix, who):
        rec, lam = _need_mix(mix, self.shape[0], who)
        self._mix = (rec.to(self.device).contiguous(), lam.to(self.device).contiguous())

    @property
    def mix(self):
        """(rec, lam) on the device, as this batch is mixed"""
        return self._mix


class MixedFrames(_Mixed, data.Frames):
    """data.Frames whose samples are mixed with their partners on the way out of the prep kernel.  mix = (rec int32 [B, 6], lam fp32
    [B]) on the device (Mix.draw brought over): what images() and patches(p) return is the mixed batch."""

    def __init__(self, src_u8, size, index=None, geom=None, table=None, *, mix):
        super().__init__(src_u8, size, index=index, geom=geom, table=table)
        self._hold_mix(mix, "MixedFrames")

    def _launch(self, patch, image):
        return ops.frames_prep(self._src, self.shape[2:], self._table, patch, image, self._index, self._geom, mix=self._mix)


class MixLoader(data.DeviceLoader):
    """DeviceLoader that mixes: with train=True every batch is cut as DeviceLoader cuts it (the same crops and flips under the same
    (seed, step)), mixed by `mix.draw(B, size, step)` with the loader's own step, and handed out as (MixedFrames, MixedLabels) with
    b = labels[partner].  With train=False it is DeviceLoader.  host_iter must yield int64 labels [B].

    The record crosses through `depth` pinned staging buffers with non_blocking copies on the current stream; a staging buffer is
    rewritten only behind the event of the copy that last read it (recorded `depth` batches earlier): DeviceLoader._stage_over."""

    def __init__(self, host_iter, device, size, mix, **kwargs):
        if any(k in kwargs for k in ("mode", "scale", "ratio", "resize_to")):
            raise ValueError("MixLoader: this loader does not resize (ResizeMixLoader mixes resized samples in one launch)")
        super().__init__(host_iter, device, size, **kwargs)
        if not isinstance(mix, Mix):
            raise ValueError(f"MixLoader: mix must be a vitamd.mix.Mix, got {type(mix).__name__}")
        self.mix = mix
        self._stage = [None] * self.depth
        self._pair = None                  # (rec, lam) on the device, of the batch being handed out

    def _staged(self, rec, lam):
        """the host record -> the device, through the staging buffer of this step"""
        return self._stage_over(self._stage, rec=rec, lam=lam)

    def _frames(self, src, geom, table):
        if not self.train:
            return super()._frames(src, geom, table)
        self._pair = self._staged(*self.mix.draw(src.shape[0], self.out_hw, self.step))
        return MixedFrames(src, self.out_hw, geom=geom, table=table, mix=self._pair)

    def _labels(self, labels):
        if not self.train:
            return super()._labels(labels)
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() != 1:
            raise ValueError("MixLoader: a mixed batch needs int64 labels [B] from host_iter")
        return MixedLabels.of(labels, self._pair)


class MixedResizedFrames(_Mixed, resize.ResizedFrames):
    """resize.ResizedFrames whose samples are mixed with their partners on the way out of the prep kernel (csrc/resize.hip,
    vitamd_frames_prep_resize_mix): every sample is resized with its own row of `box` and normalised, then mixed
    by mix = (rec int32 [B, 6], lam fp32 [B]) as MixedFrames mixes.  What images() and patches(p) return is the mixed batch."""

    def __init__(self, src_u8, size, box, index=None, mean=None, std=None, *, mix):
        if isinstance(box, torch.Tensor) and box.dim() == 2:
            _need_mix(mix, box.shape[0], "MixedResizedFrames")       # before the base class looks at a device
        super().__init__(src_u8, size, box, index=index, mean=mean, std=std)
        self._hold_mix(mix, "MixedResizedFrames")

    def _launch(self, patch, image):
        return ops.frames_prep_resize_mix(self._src, self.shape[2:], patch, image, self._index, self._box, self._mean, self._std, *self._mix)


class ResizeMixLoader(resize.ResizeLoader):
    """resize.ResizeLoader that mixes: the DeiT / timm recipe's RandomResizedCrop (or Resize + crop) and its Mixup / CutMix in the one
    launch of vitamd_frames_prep_resize_mix.  With train=True every batch is cut by self.boxes(...) exactly as ResizeLoader cuts it
    under the same (seed, step), mixed by `mix.draw(B, size, step)` exactly as MixLoader mixes it, and handed out as
    (MixedResizedFrames, MixedLabels(a, a[partner], lam)).  With train=False it is ResizeLoader's centre form with plain labels.
    host_iter must yield int64 labels [B] when train=True.

    Both records cross through pinned staging buffers with non_blocking copies on the current stream: the box through ResizeLoader's,
    the mix record through `depth` buffers of this class, each rewritten only behind the event of the copy that last read it."""

    def __init__(self, host_iter, device, size, mix, mode="rrc", scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), resize_to=None, **kwargs):
        if not isinstance(mix, Mix):
            raise ValueError(f"ResizeMixLoader: mix must be a vitamd.mix.Mix, got {type(mix).__name__}")
        super().__init__(host_iter, device, size, mode=mode, scale=scale, ratio=ratio, resize_to=resize_to, **kwargs)
        self.mix = mix
        self._mix_stage = [None] * self.depth
        self._pair = None                  # (rec, lam) on the device, of the batch being handed out

    def _check(self, batch):
        """ResizeLoader._check, and a mixed batch needs its labels: refused before anything touches the device"""
        if self.train and isinstance(batch, (tuple, list)) and len(batch) in (2, 3):
            labels = batch[1]
            if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() != 1:
                raise ValueError("ResizeMixLoader: a mixed batch needs int64 labels [B] from host_iter")
        return super()._check(batch)

    def _staged_mix(self, rec, lam):
        """the host mix record -> the device, through the staging buffer of this step (as MixLoader._staged)"""
        return self._stage_over(self._mix_stage, rec=rec, lam=lam)

    def _frames(self, src, geom, table):
        if not self.train:
            return super()._frames(src, geom, table)
        box = self.boxes(src.shape[0], tuple(src.shape[1:3]), self.step, self._extents.popleft())
        self._pair = self._staged_mix(*self.mix.draw(src.shape[0], self.out_hw, self.step))
        return MixedResizedFrames(src, self.out_hw, self._staged(box), mean=self.mean, std=self.std, mix=self._pair)

    def _labels(self, labels):
        if not self.train:
            return super()._labels(labels)
        return MixedLabels.of(labels, self._pair)
