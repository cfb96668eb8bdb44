"""Resizing in the device input feed: RandomResizedCrop and Resize + crop on uint8 frames of any size, in the one
launch that also gathers, flips, normalises and patchifies (csrc/resize.hip, vitamd_frames_prep_resize).

    box    = rrc_boxes(B, (Hs, Ws), 224, seed=0, step=i)                          # torchvision's RandomResizedCrop.get_params per sample
    box    = resize_crop_boxes(B, (Hs, Ws), 224, 224, seed=0, step=i)             # the reference's Resize(224) -> RandomCrop -> flip
    frames = ResizedFrames(u8, 224, box.to("cuda"), mean=IMAGENET_MEAN, std=IMAGENET_STD)     # stands where a data.Frames stands
    for frames, labels in ResizeLoader(host_iter, "cuda", 224, mode="rrc", patch=16, image=False): ...

What is cut is decided on the HOST, as vitamd.mix decides what is mixed: ten integers per sample - the source box, the virtual size it
is resized to, the window of that virtual image, the flip - drawn from numpy's Philox keyed by (seed, step) in float64 Python
arithmetic, crossing to the device through a pinned buffer.  The kernel's weights are integer expressions of that record
(include/vitamd.h), equal to those of F.interpolate(mode="bilinear", antialias=True, align_corners=False) on the cropped box.  Not
bit-equal to Pillow's fixed-point resize; bilinear only; no backward."""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from . import data, ops

MAX_DOWN = 8                 # the kernel's down-scaling cap per axis (16 taps)
_NORMS = {}                  # (device, mean, std) -> (mean, std) fp32 [C] on the device


def _int(v, name, lo=1):
    if not isinstance(v, int) or isinstance(v, bool) or v < lo:
        raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
    return v


def _counter(seed, step, who):
    for name, v in (("seed", seed), ("step", step)):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 1 << 64:
            raise ValueError(f"{who}: {name} must be an integer in [0, 2^64), got {v!r}")
    return np.random.Generator(np.random.Philox(key=np.array([seed, step], dtype=np.uint64)))


def _extents(B, src_hw, extents, who):
    """-> the valid (hs, ws) of every sample as Python integers; None: the full frame"""
    _int(B, f"{who}: B")
    Hs, Ws = data._hw(tuple(src_hw) if isinstance(src_hw, (tuple, list, torch.Size)) else src_hw)
    if max(Hs, Ws) > ops.FRAMES_MAX_SIZE:
        raise ValueError(f"{who}: sizes up to {ops.FRAMES_MAX_SIZE}, got src {(Hs, Ws)}")
    if extents is None:
        return [(Hs, Ws)] * B
    if not isinstance(extents, torch.Tensor) or extents.dtype != torch.int32 or tuple(extents.shape) != (B, 2) or extents.is_cuda:
        raise ValueError(f"{who}: extents must be an int32 CPU tensor [{B}, 2] of (hs, ws)")
    rows = [(int(h), int(w)) for h, w in extents.tolist()]
    if any(not (1 <= h <= Hs and 1 <= w <= Ws) for h, w in rows):
        raise ValueError(f"{who}: every extent must lie in [1, {Hs}] x [1, {Ws}]")
    return rows


def _need_scale(box_hw, virt_hw, who):
    if box_hw[0] > MAX_DOWN * virt_hw[0] or box_hw[1] > MAX_DOWN * virt_hw[1]:
        raise ValueError(f"{who}: {box_hw} -> {virt_hw} scales down by more than {MAX_DOWN}x, the kernel's cap (resize on the host first)")


def resized_size(hs, ws, resize_to):
    """torchvision's Resize(int): the shorter side to resize_to, the longer to int(resize_to * long / short)  -> (Hv, Wv)"""
    short, long = (ws, hs) if ws <= hs else (hs, ws)
    new_long = int(resize_to * long / short)
    return (new_long, resize_to) if ws <= hs else (resize_to, new_long)


def _rrc_params(rng, height, width, scale, log_ratio, ratio):
    """torchvision's RandomResizedCrop.get_params -> (i, j, h, w)"""
    area = height * width
    for _ in range(10):
        target_area = area * float(rng.uniform(scale[0], scale[1]))
        aspect = math.exp(float(rng.uniform(log_ratio[0], log_ratio[1])))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            return int(rng.integers(0, height - h + 1)), int(rng.integers(0, width - w + 1)), h, w
    in_ratio = width / height                        # the central fallback, with the ratio clamp
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    h, w = min(max(h, 1), height), min(max(w, 1), width)
    return (height - h) // 2, (width - w) // 2, h, w


def rrc_boxes(B, src_hw, out_hw, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), seed=0, step=0, flip=True, extents=None):
    """int32 [B, 10] on the CPU: per sample the crop of torchvision's RandomResizedCrop.get_params (10 attempts of area ~ U(scale) x the
    extent's, log-uniform aspect in `ratio`, w = int(round(sqrt(area * aspect))); then the central fallback with the ratio clamp) inside
    its extent, resized to out_hw (Hv = H, Wv = W, no offset), and a RandomHorizontalFlip(0.5) decision.  From numpy's Philox keyed by
    (seed, step) in float64 Python arithmetic: the same (seed, step) gives the same boxes, and no device value is read.  extents int32
    [B, 2]: each sample's valid (hs, ws) inside the canvas src_hw (None: the whole frame)."""
    who = "rrc_boxes"
    H, W = data._hw(out_hw)
    rows = _extents(B, src_hw, extents, who)
    for name, pair in (("scale", scale), ("ratio", ratio)):
        if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0 for v in pair)
                and pair[0] <= pair[1]):
            raise ValueError(f"{who}: {name} must be an ascending pair of positive numbers, got {pair!r}")
    if max(H, W) > ops.FRAMES_MAX_SIZE:
        raise ValueError(f"{who}: sizes up to {ops.FRAMES_MAX_SIZE}, got out {(H, W)}")
    for hs, ws in set(rows):
        _need_scale((hs, ws), (H, W), who)           # the whole extent may be drawn
    rng = _counter(seed, step, who)
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    out = []
    for hs, ws in rows:
        i, j, h, w = _rrc_params(rng, hs, ws, (float(scale[0]), float(scale[1])), log_ratio, (float(ratio[0]), float(ratio[1])))
        f = int(float(rng.random()) < 0.5)
        out.append([i, h, H, 0, j, w, W, 0, f if flip else 0, 0])
    return torch.tensor(out, dtype=torch.int32)


def _resize_rows(B, src_hw, resize_to, out_hw, extents, who):
    H, W = data._hw(out_hw)
    _int(resize_to, f"{who}: resize_to")
    rows = _extents(B, src_hw, extents, who)
    virt = {}
    for hs, ws in set(rows):
        Hv, Wv = resized_size(hs, ws, resize_to)
        if Hv < H or Wv < W:
            raise ValueError(f"{who}: Resize({resize_to}) of {(hs, ws)} gives {(Hv, Wv)}, smaller than the crop {(H, W)}")
        if max(Hv, Wv) > ops.FRAMES_MAX_SIZE:
            raise ValueError(f"{who}: Resize({resize_to}) of {(hs, ws)} gives {(Hv, Wv)}: sizes up to {ops.FRAMES_MAX_SIZE}")
        _need_scale((hs, ws), (Hv, Wv), who)
        virt[(hs, ws)] = (Hv, Wv)
    return H, W, rows, virt


def resize_crop_boxes(B, src_hw, resize_to, out_hw, seed, step, flip=True, extents=None):
    """int32 [B, 10] on the CPU: Resize(resize_to) of each sample's extent (torchvision's rule: resized_size), then RandomCrop(out_hw)
    offsets and a RandomHorizontalFlip(0.5) decision from the Philox of rrc_boxes - the reference's training transform (datasets.py)."""
    who = "resize_crop_boxes"
    H, W, rows, virt = _resize_rows(B, src_hw, resize_to, out_hw, extents, who)
    rng = _counter(seed, step, who)
    out = []
    for hs, ws in rows:
        Hv, Wv = virt[(hs, ws)]
        oy, ox = int(rng.integers(0, Hv - H + 1)), int(rng.integers(0, Wv - W + 1))
        f = int(float(rng.random()) < 0.5)
        out.append([0, hs, Hv, oy, 0, ws, Wv, ox, f if flip else 0, 0])
    return torch.tensor(out, dtype=torch.int32)


def resize_center_boxes(B, src_hw, resize_to, out_hw, extents=None):
    """int32 [B, 10] on the CPU: Resize(resize_to) then CenterCrop(out_hw), offsets int(round((Hv - H) / 2.0)) as data.center_geom; no flip"""
    who = "resize_center_boxes"
    H, W, rows, virt = _resize_rows(B, src_hw, resize_to, out_hw, extents, who)
    out = []
    for hs, ws in rows:
        Hv, Wv = virt[(hs, ws)]
        out.append([0, hs, Hv, int(round((Hv - H) / 2.0)), 0, ws, Wv, int(round((Wv - W) / 2.0)), 0, 0])
    return torch.tensor(out, dtype=torch.int32)


def _norm(mean, std, C, device, who):
    """(mean, std) as fp32 [C] on the device, uploaded once per device and pair; (None, None) without normalisation"""
    if (mean is None) != (std is None):
        raise ValueError(f"{who}: give mean and std together, or neither")
    if mean is None:
        return None, None
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != C or len(std) != C or any(s == 0 for s in std):
        raise ValueError(f"{who}: mean and std need {C} entries and no zero in std, got {mean} and {std}")
    key = (str(data._lib_device(device)), mean, std)
    got = _NORMS.get(key)
    if got is None:
        got = _NORMS[key] = (torch.tensor(mean, dtype=torch.float32).to(device), torch.tensor(std, dtype=torch.float32).to(device))
    return got


class ResizedFrames(data.Frames):
    """A data.Frames whose samples are resized on the way out of the prep kernel.  src_u8 as Frames takes it, of any frame size; box
    int32 [B, 10] (rrc_boxes / resize_crop_boxes / resize_center_boxes, or any record of include/vitamd.h vitamd_frames_prep_resize);
    index int64 [B] or None; mean / std: C numbers each, or neither (v / 255).  The record carries crop and flip, so there is no geom
    and no table.  The source goes through Frames._take with the resizing kernel's shape rules (an output larger than the source)."""

    def __init__(self, src_u8, size, box, index=None, mean=None, std=None):
        def own(B, C):
            if not isinstance(box, torch.Tensor) or box.dtype != torch.int32 or tuple(box.shape) != (B, 10):
                raise ValueError(f"ResizedFrames: box must be int32 [{B}, 10]")
            if (mean is None) != (std is None):
                raise ValueError("ResizedFrames: give mean and std together, or neither")
        self._take("ResizedFrames", "ResizeLoader", src_u8, size, index, True, own)
        self._geom = self._table = None
        self._box = box.to(self.device).contiguous()
        self._mean, self._std = _norm(mean, std, self.shape[1], self.device, "ResizedFrames")

    @property
    def box(self):
        """the records this batch is cut with, int32 [B, 10] on the device"""
        return self._box

    def _launch(self, patch, image):
        return ops.frames_prep(self._src, self.shape[2:], None, patch, image, self._index, resize=(self._box, self._mean, self._std))


class ResizeLoader(data.DeviceLoader):
    """DeviceLoader for host frames that are not yet at the model's size.  host_iter yields (uint8 CPU tensor [B, Hs, Ws, C], labels or
    None) or (frames, labels, extents) with extents int32 [B, 2] = each sample's valid (hs, ws) inside the padded canvas.  With
    train=True, mode "rrc" draws rrc_boxes(B, (Hs, Ws), size, scale, ratio, seed, step) and mode "resize_crop"
    resize_crop_boxes(B, (Hs, Ws), resize_to, size, seed, step), with the loader's own step; with train=False both modes take
    resize_center_boxes(B, (Hs, Ws), resize_to, size).  resize_to None: the shorter side of `size` (the reference's Resize(image_size)).
    Yields (ResizedFrames already materialised, labels on the device).

    The record crosses through `depth` pinned staging buffers with non_blocking copies on the current stream; a staging buffer is
    rewritten only behind the event of the copy that last read it (recorded `depth` batches earlier): DeviceLoader._stage_over.
    Slots, copy stream and labels are DeviceLoader's."""

    def __init__(self, host_iter, device, size, mode="rrc", scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), resize_to=None, **kwargs):
        super().__init__(host_iter, device, size, **kwargs)
        if mode not in ("rrc", "resize_crop"):
            raise ValueError(f"ResizeLoader: mode must be 'rrc' or 'resize_crop', got {mode!r}")
        self.mode, self.scale, self.ratio = mode, tuple(scale), tuple(ratio)
        self.resize_to = min(self.out_hw) if resize_to is None else _int(resize_to, "ResizeLoader: resize_to")
        self._stage = [None] * self.depth
        self._extents = collections.deque()          # of the batches fed and not yet handed out, in order

    def _check(self, batch):
        """a host batch, refused before anything touches the device (DeviceLoader's checks with the resizing kernel's shape rules)"""
        if not (isinstance(batch, (tuple, list)) and len(batch) in (2, 3)):
            raise ValueError("ResizeLoader: host_iter must yield (uint8 frames, labels or None[, extents])")
        u8, labels = self._check_frames("ResizeLoader", *batch[:2], resize=True)
        extents = batch[2] if len(batch) == 3 else None
        if extents is not None:
            _extents(u8.shape[0], tuple(u8.shape[1:3]), extents, "ResizeLoader")
        self._extents.append(None if extents is None else extents.clone())
        return u8, labels

    def boxes(self, B, src_hw, step, extents=None):
        """the record of batch `step` of B samples, on the CPU: what this loader cuts that batch with"""
        if not self.train:
            return resize_center_boxes(B, src_hw, self.resize_to, self.out_hw, extents=extents)
        if self.mode == "rrc":
            return rrc_boxes(B, src_hw, self.out_hw, self.scale, self.ratio, seed=self.seed, step=step, flip=True, extents=extents)
        return resize_crop_boxes(B, src_hw, self.resize_to, self.out_hw, seed=self.seed, step=step, flip=True, extents=extents)

    def _staged(self, box):
        """the host record -> the device, through the staging buffer of this step"""
        return self._stage_over(self._stage, box=box)[0]

    def _geom(self, n, src_hw):
        return None                        # crop and flip are in the record

    def _frames(self, src, geom, table):
        box = self.boxes(src.shape[0], tuple(src.shape[1:3]), self.step, self._extents.popleft())
        return ResizedFrames(src, self.out_hw, self._staged(box), mean=self.mean, std=self.std)
