"""The device input pipeline: raw uint8 frames on the host -> the patch-embed GEMM's bf16 operand and the fp32
image the tokenizers' losses take as their target, in one kernel launch (csrc/input.hip), behind a double-buffered loader.

    table  = norm_table(IMAGENET_MEAN, IMAGENET_STD)           # ToTensor + Normalize as a 256-entry lookup per channel
    frames = Frames(u8, size=224, geom=random_geom(...))        # a stand-in for the fp32 [B, C, H, W] batch; not a Tensor
    logits = model(frames)                                      # PatchEmbedFn takes frames.patches(p) where it would run im2col
    for frames, labels in DeviceLoader(host_iter, "cuda", 224, patch=16): ...

Frame gather, crop and flip are an index map and the value arithmetic is a table built on the CPU with torch's own ops, so what comes out
equals torchvision's ToTensor / Normalize / crop / flip bit for bit.  Resizing is NOT in this module: frames of another size go through
vitamd.resize (ResizedFrames, ResizeLoader).  No backward: a uint8 input takes no gradient."""
from __future__ import annotations

import torch

from . import lib as _lib
from . import ops

IMAGENET_MEAN = (0.485, 0.456, 0.406)        # the reference's Normalize constants (datasets.py)
IMAGENET_STD = (0.229, 0.224, 0.225)

_TABLES = {}          # (device, mean, std, channels) -> device table


def _hw(size):
    """size -> (H, W); an int means a square"""
    if isinstance(size, int) and not isinstance(size, bool):
        size = (size, size)
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) and v >= 1 for v in size)):
        raise ValueError(f"size must be a positive int or a pair of them, got {size!r}")
    return int(size[0]), int(size[1])


def norm_table(mean=None, std=None, channels=3, device=None):
    """fp32 [channels, 256]: table[c][v] = ToTensor then Normalize of byte v, with torch's CPU arithmetic (v / 255, then - mean[c], then
    / std[c], each rounded to fp32 as torchvision's in-place sub_ / div_ do).  device: also upload it, once per device and (mean, std)."""
    if (mean is None) != (std is None):
        raise ValueError("norm_table: give mean and std together, or neither")
    if not isinstance(channels, int) or not 1 <= channels <= 4:
        raise ValueError(f"norm_table: channels must be in 1..4, got {channels!r}")
    if mean is not None:
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(mean) != channels or len(std) != channels or any(s == 0 for s in std):
            raise ValueError(f"norm_table: mean and std need {channels} entries and no zero in std, got {mean} and {std}")
    key = (None if device is None else str(_lib_device(device)), mean, std, channels)
    got = _TABLES.get(key)
    if got is not None:
        return got
    t = torch.arange(256, dtype=torch.float32).div(255).repeat(channels, 1)
    if mean is not None:
        t = t.sub(torch.tensor(mean, dtype=torch.float32)[:, None]).div(torch.tensor(std, dtype=torch.float32)[:, None])
    t = t.contiguous()
    if device is not None:
        t = t.to(device)
    _TABLES[key] = t
    return t


def _lib_device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def center_geom(B, src_hw, out_hw):
    """int32 [B, 3] on the CPU: the offsets of torchvision's CenterCrop, int(round((Hs - H) / 2.0)) with Python's rounding, no flip"""
    (Hs, Ws), (H, W) = _hw(tuple(src_hw)), _hw(tuple(out_hw))
    if B < 1 or H > Hs or W > Ws:
        raise ValueError(f"center_geom: needs B >= 1 and out {(H, W)} <= src {(Hs, Ws)}")
    return torch.tensor([[int(round((Hs - H) / 2.0)), int(round((Ws - W) / 2.0)), 0]], dtype=torch.int32).repeat(B, 1)


def random_geom(B, src_hw, out_hw, seed, step, flip=True, device="cuda"):
    """int32 [B, 3] on the device: RandomCrop offsets and a RandomHorizontalFlip(0.5) decision per sample, drawn by the kernel from
    Philox4x32-10 under (seed, step) - the same values on every device and in tests/_data_ref.py"""
    return ops.crop_flip_draw(B, src_hw, out_hw, seed, step, flip=flip, device=device)


class Frames:
    """A batch of uint8 frames standing in for the fp32 [B, C, H, W] tensor the models take.  src_u8: [N, Hs, Ws, C] or [B, T, Hs, Ws, C]
    (flattened to [B*T, ...]) on the device; index int64 [B] picks the source frame of each sample (None: all, in order); geom int32
    [B, 3] = (y0, x0, flip) (None: the top-left corner, no flip); table fp32 [C, 256] (None: v / 255).  Not a Tensor: it has .shape and
    .device, and PatchEmbedFn, the tokenizer losses and frames_to_tokens know what to ask of it."""

    def __init__(self, src_u8, size, index=None, geom=None, table=None):
        def own(B, C):
            if geom is not None and (not isinstance(geom, torch.Tensor) or geom.dtype != torch.int32 or tuple(geom.shape) != (B, 3)):
                raise ValueError(f"Frames: geom must be int32 [{B}, 3]")
            if table is not None and (not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (C, 256)):
                raise ValueError(f"Frames: table must be fp32 [{C}, 256]")
        self._take("Frames", "DeviceLoader", src_u8, size, index, False, own)
        self._geom = None if geom is None else geom.to(self.device).contiguous()
        self._table = norm_table(channels=self.shape[1], device=self.device) if table is None else table.to(self.device).contiguous()

    def _take(self, who, loader, src_u8, size, index, resize, own):
        """What every frames class does with its source: the refusals of src_u8, size and index under the prefix `who` (resize: with
        the resizing kernel's shape rules), then own(B, C) - the refusals of the class's further arguments, which need no device -
        and only then the look at the device; sets _src, _index, shape, device and the empty cache of materialise."""
        if not isinstance(src_u8, torch.Tensor) or src_u8.dtype != torch.uint8:
            raise ValueError(f"{who}: expected a uint8 tensor, got {getattr(src_u8, 'dtype', type(src_u8).__name__)}")
        if src_u8.dim() == 5:
            src_u8 = src_u8.reshape(-1, *src_u8.shape[2:])
        if index is not None and (not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or index.numel() < 1):
            raise ValueError(f"{who}: index must be a 1-d int64 tensor")
        H, W = _hw(size)
        B, _, _, _, C, _, _ = ops.check_frames(src_u8.shape, (H, W), None, None if index is None else index.numel(), index is not None,
                                               resize=resize)
        own(B, C)
        if not src_u8.is_cuda:
            raise _lib.VitamdError(f"{who}: src_u8 must be on a ROCm device ({loader} brings host batches over)")
        self._src = src_u8.contiguous()
        self._index = None if index is None else index.to(src_u8.device).contiguous()
        self.shape = torch.Size((B, C, H, W))
        self.device = src_u8.device
        self._patches = {}
        self._image = None

    @property
    def geom(self):
        """the (y0, x0, flip) rows this batch was cut with, int32 [B, 3] on the device, or None"""
        return self._geom

    def _launch(self, patch, image):
        """the route of this class through the frame kernels: -> (patch rows or None, image or None), as ops.frames_prep hands them back"""
        return ops.frames_prep(self._src, self.shape[2:], self._table, patch, image, self._index, self._geom)

    def materialise(self, patch=None, image=True):
        """ONE launch (self._launch, the one thing a subclass changes) for whatever of (patch rows at this patch size, fp32 image) is not
        there yet; both are kept.  -> self"""
        want_p = patch is not None and patch not in self._patches
        want_i = bool(image) and self._image is None
        if patch is not None and (not isinstance(patch, int) or isinstance(patch, bool) or patch < 1 or self.shape[2] % patch or self.shape[3] % patch):
            raise ValueError(f"Frames: patch {patch!r} does not tile the output {tuple(self.shape[2:])}")
        if want_p or want_i:
            if self._src is None:
                raise _lib.VitamdError(f"Frames: this batch was materialised by its loader and its source slot is reused; patch={patch}, "
                                       f"image={image} was not asked of the loader")
            patches, img = self._launch(patch if want_p else None, want_i)
            if want_p:
                self._patches[patch] = patches
            if want_i:
                self._image = img
        return self

    def patches(self, p):
        """bf16 [B*gh*gw, C*p*p]: the rows ops.im2col makes of images(), bit for bit"""
        return self.materialise(p, image=False)._patches[p]

    def images(self):
        """fp32 [B, C, H, W]"""
        return self.materialise(None, image=True)._image

    def release_source(self):
        """drop the uint8 source (DeviceLoader: the slot behind it is about to be overwritten); what is materialised stays"""
        self._src = None
        return self


def to_u8(frames):
    """fp32 [..., C, H, W] in [0, 1] -> uint8 [..., H, W, C] = (x.clamp(0, 1) * 255).round(), on the kernel"""
    if not isinstance(frames, torch.Tensor) or frames.dim() < 4:
        raise ValueError(f"to_u8: expected fp32 [..., C, H, W], got {tuple(getattr(frames, 'shape', ()))}")
    lead = frames.shape[:-3]
    out = ops.frames_to_u8(frames.detach().reshape(-1, *frames.shape[-3:]).to(torch.float32).contiguous())
    return out.reshape(*lead, *out.shape[1:])


class DeviceLoader:
    """host_iter yields (uint8 CPU tensor [B, Hs, Ws, C], labels tensor or None) -> yields (Frames, already materialised; labels on the
    device).  `depth` pinned staging buffers and `depth` device slots; ONE copy stream of its own.  Each __next__ copies batch i+1 on
    the copy stream (non_blocking, from pinned memory), makes the current stream wait for batch i's copy event, draws the geometry
    (random crop + flip under (seed, its own step counter) for train=True, centred and unflipped otherwise), launches the prep kernel on
    the current stream and records the slot's "consumed" event there.  A slot is written again only behind its consumed event, and every
    event is recorded before anything waits on it.

    Multi-GPU: call functions.claim_streams(device), then loader.claim(), BEFORE torch.distributed.init_process_group - streams take
    hardware queues in order of first use; with the two compute streams this one makes three of the default four."""

    def __init__(self, host_iter, device, size, patch=None, image=True, mean=None, std=None, train=True, seed=0, depth=2):
        self.out_hw = _hw(size)
        if patch is not None and (not isinstance(patch, int) or isinstance(patch, bool) or patch < 1 or self.out_hw[0] % patch or self.out_hw[1] % patch):
            raise ValueError(f"DeviceLoader: patch {patch!r} does not tile the output {self.out_hw}")
        if patch is None and not image:
            raise ValueError("DeviceLoader: nothing to produce (give a patch size, image=True, or both)")
        if not isinstance(depth, int) or isinstance(depth, bool) or depth < 2:
            raise ValueError(f"DeviceLoader: depth must be an integer >= 2 (one slot in use, one being filled), got {depth!r}")
        if not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"DeviceLoader: seed must be an integer in [0, 2^64), got {seed!r}")
        if (mean is None) != (std is None):
            raise ValueError("DeviceLoader: give mean and std together, or neither")
        if torch.device(device).type != "cuda":
            raise ValueError(f"DeviceLoader: device must be a ROCm device, got {device!r}")
        self.device, self.patch, self.image, self.train, self.seed, self.depth = device, patch, bool(image), bool(train), seed, depth
        self.mean, self.std = mean, std
        self.step = 0                      # batches handed out: the counter of the geometry draw
        self._it = iter(host_iter)
        self._copy_stream = None
        self._slots = None                 # per slot: pinned, dev, copy_done, consumed (+ label staging)
        self._ahead = None                 # (slot, n, labels on the device) of the batch whose copy is under way
        self._fed = 0
        self._done = False

    def claim(self):
        """create the copy stream and give it its first work (see the class docstring for when)"""
        if self._copy_stream is None:
            self.device = _lib_device(self.device)
            self._copy_stream = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(self._copy_stream):
                torch.zeros(16, device=self.device).add_(1)
            self._copy_stream.synchronize()
        return self

    def _check(self, batch):
        """a host batch, refused before anything touches the device"""
        if not (isinstance(batch, (tuple, list)) and len(batch) == 2):
            raise ValueError("DeviceLoader: host_iter must yield (uint8 frames, labels or None)")
        return self._check_frames("DeviceLoader", *batch)

    def _feed(self):
        """take the next host batch and start its copy into the next slot; False at the end of host_iter"""
        try:
            u8, labels = self._check(next(self._it))
        except StopIteration:
            self._done = True
            return False
        self.claim()
        if self._slots is None:
            self._slots = [{"pinned": torch.empty(u8.shape, dtype=torch.uint8).pin_memory(),
                            "dev": torch.empty(u8.shape, dtype=torch.uint8, device=self.device),
                            "copy_done": torch.cuda.Event(), "consumed": None, "lab": None} for _ in range(self.depth)]
        s = self._slots[self._fed % self.depth]
        n = u8.shape[0]
        s["copy_done"].synchronize()                       # host: the copy that last read this pinned buffer is over (no-op when never recorded)
        s["pinned"][:n].copy_(u8)
        lab_dev = None
        with torch.cuda.stream(self._copy_stream):
            if s["consumed"] is not None:
                self._copy_stream.wait_event(s["consumed"])    # device: the kernel that last read this slot is over
            s["dev"][:n].copy_(s["pinned"][:n], non_blocking=True)
            if labels is not None:
                if s["lab"] is None or s["lab"].shape[1:] != labels.shape[1:] or s["lab"].dtype != labels.dtype or s["lab"].shape[0] < n:
                    s["lab"] = torch.empty(labels.shape, dtype=labels.dtype).pin_memory()
                s["lab"][:n].copy_(labels)
                lab_dev = s["lab"][:n].to(self.device, non_blocking=True)
            s["copy_done"].record(self._copy_stream)
        self._ahead = (s, n, lab_dev)
        self._fed += 1
        return True

    def __iter__(self):
        return self

    def __next__(self):
        if self._ahead is None and (self._done or not self._feed()):
            raise StopIteration
        s, n, labels = self._ahead
        self._ahead = None
        if not self._done:
            self._feed()                                   # batch i+1 goes over while batch i is prepared and used
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(s["copy_done"])
        if labels is not None:
            labels.record_stream(cur)                      # allocated under the copy stream, used on this one
        src = s["dev"][:n]
        src_hw = tuple(src.shape[1:3])
        with torch.cuda.device(self.device):
            geom = self._geom(n, src_hw)
            table = norm_table(self.mean, self.std, channels=src.shape[3], device=self.device)
            frames = self._frames(src, geom, table).materialise(self.patch, self.image).release_source()
            labels = self._labels(labels)
        consumed = torch.cuda.Event()
        consumed.record(cur)
        s["consumed"] = consumed
        self.step += 1
        return frames, labels

    def _frames(self, src, geom, table):
        """the batch object of this step, before it is materialised (vitamd.mix.MixLoader overrides it; self.step is this batch's)"""
        return Frames(src, self.out_hw, geom=geom, table=table)

    def _labels(self, labels):
        """what is handed out beside the frames: the labels on the device as they came (or None)"""
        return labels

    def _geom(self, n, src_hw):
        """(y0, x0, flip) of this step's n samples, on the device: random crop + flip under (seed, step) for train=True, centred and
        unflipped otherwise (vitamd.resize.ResizeLoader, whose record carries the crop, overrides it)"""
        if self.train:
            return random_geom(n, src_hw, self.out_hw, self.seed, self.step, flip=True, device=self.device)
        return center_geom(n, src_hw, self.out_hw).to(self.device)

    def _stage_over(self, stage, **host):
        """One record of this step - host tensors of one row per sample, by name - to the device, in the order given: through entry
        step % depth of `stage` (a list of `depth` entries the subclass keeps), pinned buffers that are rewritten only behind the
        event of the copy that last read them (recorded `depth` batches earlier), with non_blocking copies on the current stream."""
        st = stage[self.step % self.depth]
        if st is None or any(st[k].shape[0] < t.shape[0] for k, t in host.items()):
            st = {k: torch.zeros(t.shape, dtype=t.dtype).pin_memory() for k, t in host.items()}
            st["done"] = torch.cuda.Event()
            stage[self.step % self.depth] = st
        st["done"].synchronize()           # host: the copy that last read these buffers is over (no-op when never recorded)
        for k, t in host.items():
            st[k][:t.shape[0]].copy_(t)
        dev = tuple(st[k][:t.shape[0]].to(self.device, non_blocking=True) for k, t in host.items())
        st["done"].record(torch.cuda.current_stream(self.device))
        return dev

    def _check_frames(self, who, u8, labels, resize=False):
        """the frames and labels of a host batch and their fit into the slots (resize: under the resizing kernel's shape rules)"""
        if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.is_cuda:
            raise ValueError(f"{who}: frames must be a uint8 CPU tensor, got {getattr(u8, 'dtype', type(u8).__name__)}"
                             f"{' on ' + str(u8.device) if isinstance(u8, torch.Tensor) else ''}")
        if u8.dim() != 4:
            raise ValueError(f"{who}: frames must be [B, Hs, Ws, C], got shape {tuple(u8.shape)}")
        ops.check_frames(u8.shape, self.out_hw, self.patch, resize=resize)
        if labels is not None and (not isinstance(labels, torch.Tensor) or labels.is_cuda or labels.dim() < 1 or labels.shape[0] != u8.shape[0]):
            raise ValueError(f"{who}: labels must be a CPU tensor with one row per frame ({u8.shape[0]}) or None")
        if self._slots is not None:
            first = self._slots[0]["pinned"]
            if tuple(u8.shape[1:]) != tuple(first.shape[1:]) or u8.shape[0] > first.shape[0]:
                raise ValueError(f"{who}: a batch of shape {tuple(u8.shape)} does not fit the slots of the first one {tuple(first.shape)}")
        return u8, labels
