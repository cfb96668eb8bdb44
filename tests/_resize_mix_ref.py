"""CPU restatement of the resizing AND mixing input feed (include/vitamd.h, vitamd_frames_prep_resize_mix), shared by
test_resize_mix_host.py and test_gpu_resize_mix.py.  Plain torch on the CPU; no GPU, no library.  It is the COMPOSITION of the two
references the suite already has - _resize_ref (the resize) and _mix_ref (the record's clamps) - and restates neither.

mixed_resized_ref has two modes:

  float64 (images=None): R = _resize_ref.resize_ref in float64, mixed in float64 with l = float64(lam), m = 1 - l.  This is what the
  bound is held against.
  from the images (images = the fp32 R of a stand-alone vitamd_frames_prep_resize launch of the same records): the exact expected bits,
  by torch's own CPU operators as the header writes them: a.mul(l).add(p.mul(1 - l)) for mode 1, torch.where for mode 2.

bounds() is derived, not measured.  Write bnd_j for _resize_ref.bound of sample j (its own taps and std), R'_j for the float64
reference and R_j = R'_j + e_j, |e_j| <= bnd_j, for what the kernel holds.  With u = 2^-24 (fp32 unit roundoff) and 0 <= l <= 1:

  mode 0 and every pixel of mode 2 are ONE sample's value, unchanged: the chosen sample's bnd.
  mode 1 computes v = fl(fl(R_b l) + fl(R_q m)), m = fl(1 - l), against l R'_b + (1 - l) R'_q:
      the two resizes contribute            l bnd_b + m bnd_q
      the rounding of m (|1 - l| <= 1)      |m - (1 - l)| |R_q| <= u |R_q|
      the two products                      u (l |R_b| + m |R_q|)
      the sum                               u |fl(R_b l) + fl(R_q m)| <= u (1 + u) (l |R_b| + m |R_q|)
    together, to first order, <= l bnd_b + m bnd_q + u (2 |R_b| + 3 |R_q|).  The form used is
      bound = l bnd_b + m bnd_q + 2^-22 (|R'_b| + |R'_q|)
    4 u on each magnitude: sufficient, and the slack over (2, 3) covers the second-order terms and |R_j| against |R'_j|.

standin() is what the kernel computes, built on _resize_ref.standin's fp32 images, with one planted mistake (BUGS).

Cases: the shapes and records of _resize_ref.CASES at B = 5 with every name of _mix_ref.RECORDS (partner = the batch reversed, so
sample 2 is its own partner).  The records of _resize_ref flip samples 1 and 3, which are each other's partners; case() inverts the
flips of samples 3 and 4, so that of every pair one sample is flipped and the other is not (as _mix_ref's batches are) and a partner
mirrored with the receiver's flip shows.  On b40x36_p4 (2 x 2 partial tiles of 32 x 32) two CutMix boxes are added: COVER contains
tile (0, 0) wholly and cuts the other three; TOUCH meets tile (1, 1) in the single pixel (32, 32)."""
import torch

import _mix_ref as M
import _resize_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
B = 5
TILE = 32                                        # the fast form's output tile (csrc/resize.hip TH, TW)
CASE_NAMES = ("a16_p4", "b16_p4", "b40x36_p4", "c4_p4", "w14_p7")
EXTRA_BOXES = {"cut_cover": (0, 36, 0, 34), "cut_touch": (20, 33, 20, 33)}      # (yl, yh, xl, xh) on the 40 x 36 output


def case(name):
    """(src uint8, index list, box int32 [5, 10]) of _resize_ref.case with the flips of samples 3 and 4 inverted"""
    src, index, box = R.case(name)
    box = box.clone()
    box[3:, 8] ^= 1
    return src, index, box


def record_names(case_name):
    return M.RECORDS + (tuple(EXTRA_BOXES) if case_name == "b40x36_p4" else ())


def record(name, H, W):
    """(rec int32 [5, 6], lam fp32 [5]): _mix_ref.record, or every row CutMix with one of EXTRA_BOXES"""
    if name in EXTRA_BOXES:
        rec = torch.tensor([[B - 1 - b, 2, *EXTRA_BOXES[name]] for b in range(B)], dtype=torch.int32)
        return rec, torch.full((B,), 0.75, dtype=F32)
    return M.record(name, B, H, W)


# ------------------------------------------------------------------------------------------------ the composition
def compose(images, rec, lam, bug=None):
    """[B, C, H, W] of images' dtype: sample b mixed with sample q = partner[b] by the clamped record.  fp32: the header's three
    rounded operations by torch's CPU operators; float64: the same expression in float64.  bug: box_inclusive, lam_swapped, fma,
    skip_touching_tile (mistakes of the mixing step alone)."""
    n, C, H, W = images.shape
    dtype = images.dtype
    out = images.clone()
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    for b, (q, mode, yl, yh, xl, xh) in enumerate(M.clamp_rec(rec, n, H, W)):
        if mode == 0:
            continue
        a, p = images[b], images[q]
        if mode == 1:
            l = torch.ones((), dtype=F32) if lam is None else lam[b].to(F32)
            m = 1 - l                                # fp32: one rounding
            if bug == "lam_swapped":
                l, m = m, l
            if dtype == F64:
                l = l.to(F64)
                out[b] = a.mul(l).add(p.mul(1 - l))
            elif bug == "fma":                       # a * l unrounded inside the sum: what a fused multiply-add computes
                out[b] = (a.to(F64) * l.to(F64) + p.mul(m).to(F64)).to(F32)
            else:
                out[b] = a.mul(l).add(p.mul(m))
        else:
            if bug == "box_inclusive":
                yh, xh = min(yh + 1, H), min(xh + 1, W)
            inside = (ys >= yl) & (ys < yh) & (xs >= xl) & (xs < xh)
            if bug == "skip_touching_tile":          # a tile that the box meets in one pixel only keeps the receiver
                for ty in range(0, H, TILE):
                    for tx in range(0, W, TILE):
                        if int(inside[ty:ty + TILE, tx:tx + TILE].sum()) == 1:
                            inside[ty:ty + TILE, tx:tx + TILE] = False
            out[b] = torch.where(inside[None], p, a)
    return out


def mixed_resized_ref(src, out_hw, index, box, rec, lam, mean=None, std=None, dtype=F64, images=None):
    """images None: the float64 (or `dtype`) reference from the source.  images = fp32 [B, C, H, W], the output of a stand-alone
    vitamd_frames_prep_resize launch of (index, box, mean, std): the exact bits the mixing entry must give."""
    if images is None:
        images = R.resize_ref(src, out_hw, index, box, mean, std, dtype=dtype)
    return compose(images, rec, lam)


def bounds(src_shape, out_hw, box, rec, lam, ref_images, std=None, bnd=None):
    """fp64 [B, C, H, W]: the bound of the module docstring per element; ref_images = the float64 R' of every sample; bnd: the
    _resize_ref.bounds of `box` where the caller has them already"""
    H, W = out_hw
    n = box.shape[0]
    bnd = (R.bounds(src_shape, out_hw, box, std) if bnd is None else bnd).expand(n, ref_images.shape[1], H, W)
    out = bnd.clone()
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    for b, (q, mode, yl, yh, xl, xh) in enumerate(M.clamp_rec(rec, n, H, W)):
        if mode == 1:
            l = 1.0 if lam is None else float(lam[b])
            assert 0.0 <= l <= 1.0, "the derivation takes lam in [0, 1]"
            m = float(torch.tensor(1.0, dtype=F32) - torch.tensor(l, dtype=F32))
            out[b] = l * bnd[b] + m * bnd[q] + 2.0 ** -22 * (ref_images[b].abs() + ref_images[q].abs())
        elif mode == 2:
            inside = (ys >= yl) & (ys < yh) & (xs >= xl) & (xs < xh)
            out[b] = torch.where(inside[None], bnd[q], bnd[b])
    return out


# ------------------------------------------------------------------------------------------------ the stand-in with planted mistakes
BUGS = ("partner_receiver_box", "partner_receiver_flip", "box_inclusive", "lam_swapped", "fma", "blend_before_norm", "skip_touching_tile")


def _normalise(v, mean, std):
    C = v.shape[1]
    return (v - torch.tensor(mean[:C], dtype=F32)[None, :, None, None]) / torch.tensor(std[:C], dtype=F32)[None, :, None, None]


def standin(src, out_hw, index, box, rec, lam, mean=None, std=None, p=None, bug=None):
    """(image fp32 [B, C, H, W], patch rows bf16 or None): every sample by _resize_ref.standin (clean), then mixed; one of BUGS planted"""
    H, W = out_hw
    n = box.shape[0]
    idx = R.clamp_index(index, n, src.shape[0])
    if bug == "blend_before_norm":                   # mixed on the r / 255 scale, normalised afterwards
        image = compose(R.standin(src, out_hw, idx, box)[0], rec, lam)
        image = image if mean is None else _normalise(image, mean, std)
    elif bug in ("partner_receiver_box", "partner_receiver_flip"):
        own = R.standin(src, out_hw, idx, box, mean, std)[0]
        image = own.clone()
        for b, (q, mode, *_rest) in enumerate(M.clamp_rec(rec, n, H, W)):
            if mode == 0:
                continue
            row = box[b].clone() if bug == "partner_receiver_box" else box[q].clone()
            row[8] = box[b, 8]                       # the partner's frame, cut (or only mirrored) as the receiver is
            wrong = R.standin(src, out_hw, [idx[q]], row[None], mean, std)[0][0]
            pair = torch.stack([own[b], wrong])
            rec_b = torch.tensor([[1, rec[b, 1], *rec[b, 2:].tolist()], [1, 0, 0, 0, 0, 0]], dtype=torch.int32)
            image[b] = compose(pair, rec_b, None if lam is None else torch.stack([lam[b], lam[b]]))[0]
    else:
        image = compose(R.standin(src, out_hw, idx, box, mean, std)[0], rec, lam, bug=bug)
    return image, (None if p is None else R.bf16_rows(image, p))


def check_bits(got, want, what=""):
    """bit-equality of two fp32 images (integer views: -0 / +0 and NaN cannot hide) -> list of failures"""
    if got.dtype != F32 or got.shape != want.shape:
        return [f"{what}: {got.dtype} {tuple(got.shape)} where fp32 {tuple(want.shape)} is expected"]
    bad = got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
    if bool(bad.any()):
        return [f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits from the composition of the stand-alone images"]
    return []
