"""CPU restatements of the device input pipeline (include/vitamd.h, vitamd_frames_prep / vitamd_crop_flip_draw / vitamd_frames_to_u8),
shared by test_data_host.py and test_gpu_data.py.  Torch on the CPU and the numpy Philox of _sampling_ref.py only.

Two independent statements of the frame semantics: frames_ref walks the definition with indexing (no table anywhere), frames_ref_tv is
what a torchvision pipeline does (permute, float, div 255, sub mean, div std, slice, flip).  They must agree bit for bit, and so must
the kernel with both."""
import numpy as np
import torch

import _sampling_ref as S


def value(v, c, mean, std):
    """ToTensor + Normalize of bytes v (uint8 tensor) of channel c, with torch's CPU fp32 arithmetic"""
    t = v.to(torch.float32).div(255)
    if mean is not None:
        t = t.sub(torch.tensor(mean[c], dtype=torch.float32)).div(torch.tensor(std[c], dtype=torch.float32))
    return t


def clamp_geom(index, geom, B, Nsrc, Hs, Ws, H, W):
    """the clamps of the header: index into [0, Nsrc), y0 into [0, Hs-H], x0 into [0, Ws-W], any non-zero flip = 1"""
    idx = list(range(B)) if index is None else [min(max(int(i), 0), Nsrc - 1) for i in index]
    if geom is None:
        return idx, [(0, 0, 0)] * B
    return idx, [(min(max(int(y0), 0), Hs - H), min(max(int(x0), 0), Ws - W), int(f != 0)) for y0, x0, f in geom.tolist()]


def frames_ref(src, out_hw, index=None, geom=None, mean=None, std=None):
    """the definition, by indexing: image[b, c, y, x] = value(src[index[b], y0 + y, x0 + (flip ? W-1-x : x), c])  -> fp32 [B, C, H, W]"""
    Nsrc, Hs, Ws, C = src.shape
    H, W = out_hw
    B = Nsrc if index is None else len(index)
    idx, g = clamp_geom(index, geom, B, Nsrc, Hs, Ws, H, W)
    out = torch.empty((B, C, H, W), dtype=torch.float32)
    ys = torch.arange(H)
    xs = torch.arange(W)
    for b in range(B):
        y0, x0, flip = g[b]
        cols = x0 + (W - 1 - xs if flip else xs)
        for c in range(C):
            out[b, c] = value(src[idx[b]][(y0 + ys)[:, None], cols[None, :], c], c, mean, std)
    return out


def frames_ref_tv(src, out_hw, index=None, geom=None, mean=None, std=None):
    """the same through the transform chain: the WHOLE frame to float, normalised, then cropped and flipped"""
    Nsrc, Hs, Ws, C = src.shape
    H, W = out_hw
    B = Nsrc if index is None else len(index)
    idx, g = clamp_geom(index, geom, B, Nsrc, Hs, Ws, H, W)
    full = src.permute(0, 3, 1, 2).float().div(255)
    if mean is not None:
        full = full.sub(torch.tensor(mean, dtype=torch.float32)[None, :, None, None]).div(torch.tensor(std, dtype=torch.float32)[None, :, None, None])
    out = []
    for b in range(B):
        y0, x0, flip = g[b]
        img = full[idx[b], :, y0:y0 + H, x0:x0 + W]
        out.append(img.flip(-1) if flip else img)
    return torch.stack(out).contiguous()


def patch_rows(image, p):
    """fp32 [B, C, H, W] -> [B*gh*gw, C*p*p], row (b*gh + ph)*gw + pw, column (c*p + kh)*p + kw: the permutation alone, no rounding"""
    B, C, H, W = image.shape
    gh, gw = H // p, W // p
    return image.view(B, C, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * p * p).contiguous()


def draw_ref(B, src_hw, out_hw, seed, step, flip=True):
    """int32 [B, 3]: Philox4x32-10, key (seed lo, seed hi), counter (b, 1, step lo, step hi); y0 = (w0 * (Hs-H+1)) >> 32,
    x0 = (w1 * (Ws-W+1)) >> 32, flip = w2 >> 31"""
    (Hs, Ws), (H, W) = src_hw, out_hw
    b = np.arange(B, dtype=np.uint64)
    w = S.philox4x32_10((b, 1, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    y0 = (w[0].astype(np.uint64) * np.uint64(Hs - H + 1)) >> np.uint64(32)
    x0 = (w[1].astype(np.uint64) * np.uint64(Ws - W + 1)) >> np.uint64(32)
    f = (w[2] >> np.uint32(31)) if flip else np.zeros(B, dtype=np.uint32)
    return torch.from_numpy(np.stack([y0, x0, f.astype(np.uint64)], axis=1).astype(np.int32))


def to_u8_ref(x):
    """fp32 [B, C, H, W] -> uint8 [B, H, W, C]; NaN -> 0 (the torch expression leaves NaN to the cast)"""
    y = (torch.nan_to_num(x, nan=0.0, posinf=float("inf"), neginf=-float("inf")).clamp(0, 1) * 255).round().to(torch.uint8)
    return y.permute(0, 2, 3, 1).contiguous()
