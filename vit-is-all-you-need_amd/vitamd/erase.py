"""Random Erasing for ViT training: the last augmentation of the DeiT / timm recipe (--reprob 0.25 --remode
pixel), as a post-pass over the finished batch of the device input feed (csrc/erase.hip, vitamd_frames_erase).

    erase  = Erase(probability=0.25, mode="pixel")
    loader = EraseResizeMixLoader(host_iter, "cuda", 224, mix, erase=erase, mode="rrc", patch=16, image=False)
    frames = erased(Frames(u8, 224, geom=geom), erase.draw(B, 224, step), seed=0, step=step)      # any data.Frames

Which boxes are erased is decided on the HOST, as vitamd.mix decides what is mixed: five integers per box, from numpy's Philox keyed
by (seed, step), crossing to the device through a pinned buffer.  The kernel then rewrites only those boxes of the patch rows (and
of the image, where one is asked for) in place, behind whichever of the four prep kernels made them: the fp32 batch, the Python loop
over its samples and the second im2col do not exist.  Per-pixel noise is drawn on the device, a pure function of
(seed, step, sample, channel, y, x).

ORDER: the batch is erased after crop / resize / flip / normalise and after Mixup / CutMix, labels untouched - timm's train.py with
its prefetcher (collate-time Mixup, then RandomErasing on the normalised device batch).  DeiT's own loader erases every sample before
the mix; that order is not built."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import data, mix, ops, resize

MODE_NONE, MODE_FILL, MODE_NOISE = 0, 1, 2
ATTEMPTS = 10


class Erase:
    """The draw of timm's RandomErasing: with chance `probability` a sample gets `count` boxes, an integer in [min_count, max_count];
    each box is tried up to ten times with target area uniform in [min_area, max_area] x H W / count and log-uniform aspect in
    [min_aspect, max_aspect] (None: 1 / min_aspect), and kept when it is smaller than the image on both axes.  mode "const" fills with
    zeros, "rand" with one N(0, 1) value per channel (drawn here), "pixel" with one per pixel and channel (drawn by the kernel)."""

    def __init__(self, probability=0.25, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode="pixel", min_count=1, max_count=None,
                 seed=0):
        def number(name, v):
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v):
                raise ValueError(f"Erase: {name} must be a finite number, got {v!r}")
            return float(v)
        if not 0.0 <= number("probability", probability) <= 1.0:
            raise ValueError(f"Erase: probability must lie in [0, 1], got {probability!r}")
        if not 0.0 < number("min_area", min_area) <= number("max_area", max_area) <= 1.0:
            raise ValueError(f"Erase: needs 0 < min_area <= max_area <= 1, got {min_area!r} and {max_area!r}")
        max_aspect = 1 / min_aspect if max_aspect is None and isinstance(min_aspect, (int, float)) and min_aspect > 0 else max_aspect
        if not 0.0 < number("min_aspect", min_aspect) <= number("max_aspect", max_aspect):
            raise ValueError(f"Erase: needs 0 < min_aspect <= max_aspect, got {min_aspect!r} and {max_aspect!r}")
        if mode not in ("const", "rand", "pixel"):
            raise ValueError(f"Erase: mode must be 'const', 'rand' or 'pixel', got {mode!r}")
        max_count = min_count if max_count is None else max_count
        for name, v in (("min_count", min_count), ("max_count", max_count)):
            if not isinstance(v, int) or isinstance(v, bool) or not 1 <= v <= ops.ERASE_MAX_BOXES:
                raise ValueError(f"Erase: {name} must be an integer in [1, {ops.ERASE_MAX_BOXES}], got {v!r}")
        if min_count > max_count:
            raise ValueError(f"Erase: min_count {min_count} exceeds max_count {max_count}")
        if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 1 << 64:
            raise ValueError(f"Erase: seed must be an integer in [0, 2^64), got {seed!r}")
        self.probability, self.min_area, self.max_area = float(probability), float(min_area), float(max_area)
        self.min_aspect, self.max_aspect, self.mode = float(min_aspect), float(max_aspect), mode
        self.min_count, self.max_count, self.seed = min_count, max_count, seed

    @property
    def enabled(self):
        return self.probability > 0

    def _decide(self, rng, H, W):
        """one sample -> max_count rows of (mode, yl, yh, xl, xh) and of four fill values; all in float64 / Python integers"""
        K = self.max_count
        rows, fills = [[MODE_NONE, 0, 0, 0, 0] for _ in range(K)], [[0.0] * 4 for _ in range(K)]
        if not rng.random() < self.probability:
            return rows, fills
        count = self.min_count if self.min_count == self.max_count else int(rng.integers(self.min_count, self.max_count + 1))
        log_aspect = (math.log(self.min_aspect), math.log(self.max_aspect))
        for k in range(count):
            for _ in range(ATTEMPTS):
                target = float(rng.uniform(self.min_area, self.max_area)) * H * W / count
                aspect = math.exp(float(rng.uniform(log_aspect[0], log_aspect[1])))
                h, w = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
                if h < H and w < W:
                    top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
                    if self.mode == "rand":
                        fills[k] = [float(v) for v in rng.standard_normal(4)]
                    if h > 0 and w > 0:                                   # a box rounded to nothing erases nothing
                        rows[k] = [MODE_NOISE if self.mode == "pixel" else MODE_FILL, top, top + h, left, left + w]
                    break
        return rows, fills

    def draw(self, B, hw, step):
        """-> (rec int32 [B, K, 5] = (mode, yl, yh, xl, xh), fill fp32 [B, K, 4]) on the CPU, K = max_count, from numpy's Philox with
        key (seed, step) and counter (0, 0, 0, 2) - the non-zero counter keeps the draw apart from Mix.draw's under the same seed and
        step.  The same (seed, step) gives the same record, and no device value is read.  Rows beyond a sample's count, rows of a
        sample that is not erased and boxes none of whose ten attempts fit are mode 0."""
        H, W = data._hw(hw)
        if not isinstance(B, int) or isinstance(B, bool) or B < 1:
            raise ValueError(f"Erase.draw: B must be a positive integer, got {B!r}")
        if not isinstance(step, int) or isinstance(step, bool) or not 0 <= step < 1 << 64:
            raise ValueError(f"Erase.draw: step must be an integer in [0, 2^64), got {step!r}")
        rng = np.random.Generator(np.random.Philox(key=np.array([self.seed, step], dtype=np.uint64), counter=np.array([0, 0, 0, 2], dtype=np.uint64)))
        drawn = [self._decide(rng, H, W) for _ in range(B)]
        rec = torch.tensor([rows for rows, _ in drawn], dtype=torch.int32)
        fill = torch.tensor([fills for _, fills in drawn], dtype=torch.float64).to(torch.float32)
        return rec, fill


def _need_pair(pair, B, who):
    """the (rec, fill) pair of an erased batch of B samples, checked"""
    if not (isinstance(pair, (tuple, list)) and len(pair) == 2):
        raise ValueError(f"{who}: pair must be (rec int32 [B, K, 5], fill fp32 [B, K, 4] or None)")
    rec, fill = pair
    if not isinstance(rec, torch.Tensor) or rec.dtype != torch.int32 or rec.dim() != 3 or rec.shape[0] != B or rec.shape[2] != 5 \
            or not 1 <= rec.shape[1] <= ops.ERASE_MAX_BOXES:
        raise ValueError(f"{who}: rec must be int32 [{B}, K <= {ops.ERASE_MAX_BOXES}, 5]")
    if fill is not None and (not isinstance(fill, torch.Tensor) or fill.dtype != torch.float32 or tuple(fill.shape) != (B, rec.shape[1], 4)):
        raise ValueError(f"{who}: fill must be fp32 [{B}, {rec.shape[1]}, 4] or None")
    return rec, fill


class _Erased:
    """The mixin erased() puts over a batch's class: the launch of that class, then the erasing launch on what it returned.  The noise
    is a function of (seed, step, b, c, y, x) alone, so patches(8), patches(16) and images() of one batch, materialised by separate
    launches, agree."""

    def _launch(self, patch, image):
        patches, img = super()._launch(patch, image)
        ops.frames_erase(patches, img, patch, *self._erase_pair, self._erase_seed, self._erase_step, hw=tuple(self.shape[2:]))
        return patches, img

    @property
    def erase(self):
        """(rec, fill) on the device, as this batch is erased"""
        return self._erase_pair


_CLASSES = {}         # frames class -> its erased subclass


def erased(frames, pair, seed, step):
    """-> the same batch, erased: `frames` is any data.Frames (plain, mixed, resized, both, or a user's subclass) nothing of which is
    materialised yet; pair = (rec int32 [B, K, 5], fill fp32 [B, K, 4] or None) as Erase.draw gives it, on any device (held on the
    batch's); seed and step key the per-pixel noise.  The batch stays an instance of its class - PatchEmbedFn and the tokenizer routes
    keep recognising it - and what patches(p) and images() return from now on is the erased batch."""
    if not isinstance(frames, data.Frames):
        raise ValueError(f"erased: expected a vitamd.data.Frames, got {type(frames).__name__}")
    if isinstance(frames, _Erased):
        raise ValueError("erased: this batch is erased already (one record holds up to 8 boxes per sample)")
    rec, fill = _need_pair(pair, frames.shape[0], "erased")
    for name, v in (("seed", seed), ("step", step)):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 1 << 64:
            raise ValueError(f"erased: {name} must be an integer in [0, 2^64), got {v!r}")
    if frames._patches or frames._image is not None:
        raise ValueError("erased: this batch is materialised already; erase it before patches() / images() are asked of it")
    base = type(frames)
    cls = _CLASSES.get(base)
    if cls is None:
        cls = _CLASSES[base] = type("Erased" + base.__name__, (_Erased, base), {"__doc__": f"{base.__name__} with Random Erasing behind its launch"})
    frames._erase_pair = (rec.to(frames.device).contiguous(), None if fill is None else fill.to(frames.device).contiguous())
    frames._erase_seed, frames._erase_step = seed, step
    frames.__class__ = cls
    return frames


class _EraseFeed:
    """The loader mixin: with train=True and an enabled Erase, the batch of the loader below is drawn a record with the loader's own
    step (Erase.draw(B, size, step)), which crosses through `depth` pinned staging buffers of this mixin (DeviceLoader._stage_over),
    and is handed on erased; the noise is keyed by (erase.seed, step).  Labels are untouched.  With train=False it changes nothing."""

    def __init__(self, *args, erase, **kwargs):
        if not isinstance(erase, Erase):
            raise ValueError(f"{type(self).__name__}: erase must be a vitamd.erase.Erase, got {type(erase).__name__}")
        super().__init__(*args, **kwargs)
        self.erase = erase
        self._erase_stage = [None] * self.depth

    def _frames(self, src, geom, table):
        frames = super()._frames(src, geom, table)
        if not (self.train and self.erase.enabled):
            return frames
        rec, fill = self.erase.draw(src.shape[0], self.out_hw, self.step)
        return erased(frames, self._stage_over(self._erase_stage, erase_rec=rec, erase_fill=fill), self.erase.seed, self.step)


class EraseLoader(_EraseFeed, data.DeviceLoader):
    """data.DeviceLoader whose training batches are erased: EraseLoader(host_iter, device, size, erase=Erase(...), **DeviceLoader's)"""


class EraseResizeLoader(_EraseFeed, resize.ResizeLoader):
    """resize.ResizeLoader whose training batches are erased behind the resizing launch"""


class EraseMixLoader(_EraseFeed, mix.MixLoader):
    """mix.MixLoader whose training batches are erased after the mix: EraseMixLoader(host_iter, device, size, mix, erase=Erase(...))"""


class EraseResizeMixLoader(_EraseFeed, mix.ResizeMixLoader):
    """mix.ResizeMixLoader whose training batches are erased after RandomResizedCrop and the mix: the whole DeiT / timm recipe"""
