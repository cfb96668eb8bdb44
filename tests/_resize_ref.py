"""CPU restatements of the resizing input feed (include/vitamd.h, vitamd_frames_prep_resize), shared by test_resize_host.py and
test_gpu_resize.py.  Plain torch on the CPU and Python integers; no GPU, no library.

resize_ref is the float64 statement of the header: the numerators n_j in Python integers, everything else in float64, the clamps
included.  resize_f32 restates it in fp32 in both pass orders (what a kernel may do), standin() is resize_f32 with one planted mistake,
built on a float triangle filter so that each mistake is a change of one line.  bound() is derived, not measured:

  every n_j and their sum is an exact fp32 integer (<= 16 * 16384), so a weight carries one rounding; a dot product of T non-negative
  terms then carries a relative error <= (T + 1) 2^-24; two passes and the three normalisation roundings, on values with r / 255 <= 1
  and 0 <= mean <= 1, give |err| <= (Tx + Ty + 6) 2^-24 / std to first order.  bound = 2 x that: the factor covers the second-order
  terms and the freedom in the order of the additions.  A tap list shifted by one pixel errs by about 1 on the same scale."""
import torch

import _data_ref as D

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MAX_SIZE = 8192
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)


# ------------------------------------------------------------------------------------------------ the record
def clamp_box(row, Hs, Ws, H, W):
    """the clamps of the header on one record -> (y0, h, Hv, oy, x0, w, Wv, ox, flip)"""
    cl = lambda v, lo, hi: min(max(int(v), lo), hi)
    y0 = cl(row[0], 0, Hs - 1)
    h = cl(row[1], 1, Hs - y0)
    Hv = cl(row[2], max(H, -(-h // 8)), MAX_SIZE)
    oy = cl(row[3], 0, Hv - H)
    x0 = cl(row[4], 0, Ws - 1)
    w = cl(row[5], 1, Ws - x0)
    Wv = cl(row[6], max(W, -(-w // 8)), MAX_SIZE)
    ox = cl(row[7], 0, Wv - W)
    return y0, h, Hv, oy, x0, w, Wv, ox, int(int(row[8]) != 0)


def clamp_index(index, B, Nsrc):
    return list(range(B)) if index is None else [min(max(int(i), 0), Nsrc - 1) for i in index]


def numerators(O, off, n, nv):
    """Python integers [O][n]: n_j = max(0, 2S - |(2j+1) nv - u n|), S = max(n, nv), u = 2 (o + off) + 1"""
    S = max(n, nv)
    return [[max(0, 2 * S - abs((2 * j + 1) * nv - (2 * (o + off) + 1) * n)) for j in range(n)] for o in range(O)]


def weights(O, off, n, nv, dtype=F64):
    """[O, n]: n_j / sum_j n_j, the division in `dtype` (both operands are exact there)"""
    num = torch.tensor(numerators(O, off, n, nv), dtype=torch.int64)
    assert int(num.sum(1).min()) > 0
    return num.to(dtype) / num.sum(1, keepdim=True).to(dtype)


def taps(box_row, H, W):
    """(Tx, Ty): the largest number of non-zero taps of an output column / row of a clamped record"""
    y0, h, Hv, oy, x0, w, Wv, ox, flip = box_row
    ty = max(sum(v > 0 for v in r) for r in numerators(H, oy, h, Hv))
    tx = max(sum(v > 0 for v in r) for r in numerators(W, ox, w, Wv))
    return tx, ty


def bound(Tx, Ty, std_c=1.0):
    return 2.0 * (Tx + Ty + 6) * 2.0 ** -24 / abs(std_c)


def bounds(src_shape, out_hw, box, std=None):
    """fp64 [B, C, 1, 1]: bound() per sample and channel for a record tensor"""
    Nsrc, Hs, Ws, C = src_shape
    H, W = out_hw
    rows = []
    for r in box.tolist():
        tx, ty = taps(clamp_box(r, Hs, Ws, H, W), H, W)
        rows.append([bound(tx, ty, 1.0 if std is None else std[c]) for c in range(C)])
    return torch.tensor(rows, dtype=F64)[:, :, None, None]


# ------------------------------------------------------------------------------------------------ the references
def _normalise(r, mean, std, dtype):
    """r [C, H, W] on the 0..255 scale -> r / 255, - mean, / std: three operations of `dtype`"""
    v = r / torch.tensor(255.0, dtype=dtype)
    if mean is not None:
        C = r.shape[0]
        v = (v - torch.tensor(mean[:C], dtype=dtype)[:, None, None]) / torch.tensor(std[:C], dtype=dtype)[:, None, None]
    return v


def resize_ref(src, out_hw, index, box, mean=None, std=None, dtype=F64, order="xy"):
    """[B, C, H, W] in `dtype` (float64: the reference; fp32: the restatement, `order` = which pass runs first)"""
    Nsrc, Hs, Ws, C = src.shape
    H, W = out_hw
    B = box.shape[0]
    idx = clamp_index(index, B, Nsrc)
    out = torch.zeros((B, C, H, W), dtype=dtype)
    for b, row in enumerate(box.tolist()):
        y0, h, Hv, oy, x0, w, Wv, ox, flip = clamp_box(row, Hs, Ws, H, W)
        wy, wx = weights(H, oy, h, Hv, dtype), weights(W, ox, w, Wv, dtype)
        if flip:
            wx = wx.flip(0)                          # out[x] = window[W-1-x]
        px = src[idx[b], y0:y0 + h, x0:x0 + w].permute(2, 0, 1).to(dtype)          # [C, h, w]
        if order == "xy":
            r = torch.matmul(wy, torch.matmul(px, wx.t()))
        else:
            r = torch.matmul(torch.matmul(wy, px), wx.t())
        out[b] = _normalise(r, mean, std, dtype)
    return out


def resize_f32(src, out_hw, index, box, mean=None, std=None, order="xy"):
    return resize_ref(src, out_hw, index, box, mean, std, dtype=F32, order=order)


def interpolate_ref(src, out_hw, index, box):
    """float64 [B, C, H, W] on the 0..255 scale by torch itself: F.interpolate(antialias=True) of the cropped box to (Hv, Wv), then the
    window, then the flip.  For in-range records only."""
    H, W = out_hw
    out = []
    for b, (y0, h, Hv, oy, x0, w, Wv, ox, flip, _) in enumerate(box.tolist()):
        f = b if index is None else index[b]
        crop = src[f, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].to(F64)
        virt = torch.nn.functional.interpolate(crop, size=(Hv, Wv), mode="bilinear", antialias=True, align_corners=False)[0]
        win = virt[:, oy:oy + H, ox:ox + W]
        out.append(win.flip(-1) if flip else win)
    return torch.stack(out)


def bf16_rows(image, p):
    """the round-to-nearest-even patch rows of an fp32 image, in vitamd_im2col_bf16's layout"""
    return D.patch_rows(image.to(F32), p).to(BF16)


# ------------------------------------------------------------------------------------------------ the stand-in with planted mistakes
BUGS = ("no_half_pixel", "support_one", "no_clip", "no_renorm", "flip_virtual", "no_offset", "swap_scales", "no_index", "swap_norm",
        "short_taps", "bf16_trunc")


def _tri(O, off, n, nv, origin, size, scale=None, bug=None):
    """float64 [O, size] over the FRAME's rows (the box starts at `origin`): the triangle filter of support max(scale, 1) about
    (o + off + 0.5) scale, taps clipped to the box and renormalised - each `bug` changes one step"""
    scale = n / nv if scale is None else scale
    support = 1.0 if bug == "support_one" else max(scale, 1.0)
    out = torch.zeros((O, size), dtype=F64)
    lo, hi = (-origin, size - origin) if bug == "no_clip" else (0, n)
    for o in range(O):
        centre = (o + off + (0.0 if bug == "no_half_pixel" else 0.5)) * scale
        full = {j: max(0.0, 1.0 - abs(j + 0.5 - centre) / support) for j in range(int(centre - support) - 2, int(centre + support) + 3)}
        kept = {j: v for j, v in full.items() if lo <= j < hi and v > 0}
        if bug == "short_taps" and len(kept) > 1:
            kept.pop(max(kept))
        total = sum(full.values()) if bug == "no_renorm" else sum(kept.values())
        for j, v in kept.items():
            out[o, origin + j] = v / total
    return out


def standin(src, out_hw, index, box, mean=None, std=None, p=None, bug=None):
    """(image fp32 [B, C, H, W], patch rows bf16 or None): what the kernel computes, in fp32, with one of BUGS planted (None: clean)"""
    Nsrc, Hs, Ws, C = src.shape
    H, W = out_hw
    B = box.shape[0]
    idx = [b % Nsrc for b in range(B)] if bug == "no_index" else clamp_index(index, B, Nsrc)
    if bug == "swap_norm" and mean is not None:
        mean, std = tuple(reversed(mean[:C])), tuple(reversed(std[:C]))
    image = torch.zeros((B, C, H, W), dtype=F32)
    for b, row in enumerate(box.tolist()):
        y0, h, Hv, oy, x0, w, Wv, ox, flip = clamp_box(row, Hs, Ws, H, W)
        if bug == "no_offset":
            oy = ox = 0
        sy, sx = (w / Wv, h / Hv) if bug == "swap_scales" else (h / Hv, w / Wv)
        wy = _tri(H, oy, h, Hv, y0, Hs, sy, bug)
        if flip and bug == "flip_virtual":           # the virtual image mirrored, then the window cut
            wx = _tri(W, Wv - W - ox, w, Wv, x0, Ws, sx, bug).flip(0)
        else:
            wx = _tri(W, ox, w, Wv, x0, Ws, sx, bug)
            wx = wx.flip(0) if flip else wx
        px = src[idx[b]].permute(2, 0, 1).to(F32)                                  # the whole frame: the weights select the box
        r = torch.matmul(wy.to(F32), torch.matmul(px, wx.to(F32).t()))
        image[b] = _normalise(r, mean, std, F32)
    rows = None
    if p is not None:
        rows = D.patch_rows(image, p)
        if bug == "bf16_trunc":
            rows = (rows.view(torch.int32) & ~0xFFFF).view(F32).to(BF16)
        else:
            rows = rows.to(BF16)
    return image, rows


def check_image(got, ref, bnd, what=""):
    """the GPU test's check of an image against the float64 reference: every element within its bound -> list of failures"""
    err = (got.to(F64) - ref).abs()
    bad = ~(err <= bnd)                              # NaN fails
    if bool(bad.any()):
        worst = float((err / bnd).nan_to_num(nan=float("inf")).max())
        return [f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst {worst:.3g} x bound"]
    return []


def check_rows(rows, image, p, what=""):
    """the GPU test's check of the bf16 rows: bit-equal to the round-to-nearest-even im2col of the image they came with"""
    want = bf16_rows(image, p)
    if rows.dtype != BF16 or rows.shape != want.shape or not torch.equal(rows.view(torch.int16), want.view(torch.int16)):
        return [f"{what}: the bf16 rows are not the round-to-nearest-even of the image"]
    return []


# ------------------------------------------------------------------------------------------------ shared cases
# name -> (Nsrc, Hs, Ws, C, H, W, p); B = 5 everywhere.  Source rows of 53 * 3 = 159 and 140 * 3 = 420 bytes.
CASES = {
    "a16_p4":    (4, 37, 53, 3, 16, 16, 4),          # fast form, one tile per sample
    "a16_p8":    (4, 37, 53, 3, 16, 16, 8),
    "a12x20_p4": (4, 37, 53, 3, 12, 20, 4),          # H != W
    "b16_p4":    (3, 131, 140, 3, 16, 16, 4),        # exactly 8x: 136 source rows for a tile = two strip chunks
    "b40x36_p4": (3, 131, 140, 3, 40, 36, 4),        # 2 x 2 tiles per sample, every one of them partial
    "c1_p4":     (4, 37, 53, 1, 16, 16, 4),          # generic form: C != 3
    "c4_p4":     (4, 37, 53, 4, 16, 16, 4),
    "w14_p7":    (4, 37, 53, 3, 14, 14, 7),          # generic form: W % 4 != 0, p % 4 != 0
}
INDEX = {4: [3, 1, 1, 0, 2], 3: [2, 1, 1, 0, 2]}     # repeated and out of order


def resized_size(hs, ws, resize_to):
    """torchvision's Resize(int), restated"""
    short, long = (ws, hs) if ws <= hs else (hs, ws)
    new_long = int(resize_to * long / short)
    return (new_long, resize_to) if ws <= hs else (resize_to, new_long)


def records(Hs, Ws, H, W):
    """int32 [5, 10]: an interior down-scale with different x and y scales (23 x 31 -> 16 x 16 at H = W = 16); a 3 x 1 box in the
    bottom-left corner scaled up, flipped; the largest box the 8x cap admits from the top-right corner (the whole frame where it is
    small enough: every border; exactly 8x from 131 x 140 to 16); Resize(S) of the whole frame + crop at offset 0, flipped; the same
    at offset (Hv - H, Wv - W)"""
    h0, w0 = min(Hs - 2, round(1.45 * H)), min(Ws - 2, round(1.95 * W))
    hb, wb = min(Hs, 8 * H), min(Ws, 8 * W)
    S = 1
    while min(a - b for a, b in zip(resized_size(Hs, Ws, S), (H + 2, W + 2))) < 0:
        S += 1
    Hv, Wv = resized_size(Hs, Ws, S)
    rows = [[(Hs - h0) // 2, h0, H, 0, (Ws - w0) // 2, w0, W, 0, 0, 0],
            [Hs - 3, 3, H, 0, 0, 1, W, 0, 1, 0],
            [0, hb, H, 0, Ws - wb, wb, W, 0, 0, 0],
            [0, Hs, Hv, 0, 0, Ws, Wv, 0, 1, 0],
            [0, Hs, Hv, Hv - H, 0, Ws, Wv, Wv - W, 0, 0]]
    return torch.tensor(rows, dtype=torch.int32)


def case(name):
    """(src uint8 [Nsrc, Hs, Ws, C], index list, box int32 [5, 10]) on the CPU, from the name alone"""
    Nsrc, Hs, Ws, C, H, W, p = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    src = torch.randint(0, 256, (Nsrc, Hs, Ws, C), generator=g, dtype=torch.uint8)
    return src, INDEX[Nsrc], records(Hs, Ws, H, W)
