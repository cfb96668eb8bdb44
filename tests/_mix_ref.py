"""CPU restatements of the mixing input feed and the soft-target cross-entropy (include/vitamd.h, vitamd_frames_prep_mix and
vitamd_soft_cross_entropy_fwd / _bwd), shared by test_mix_host.py and test_gpu_mix.py.  Plain torch on the CPU; no GPU, no library.

mixed_frames_ref is built on _data_ref.frames_ref with torch's own CPU operators, exactly as the header writes the blend.  soft_ce_ref
is the float64 statement of the loss, soft_ce_torch32 torch's own fp32 evaluation of the expression a user would write (the yardstick
of _lm_ref.bound), and standin() a torch restatement of what the kernels compute that the host test plants mistakes in.  The error
measures and bound() are _lm_ref's (the suite's rule); nothing of them is restated here."""
import torch

import _data_ref as D
from _lm_ref import (BF16, F32, F64, FLOOR, bound, check_bf16_grad, check_cross_entropy,  # noqa: F401  (re-exported to the tests)
                     cross_entropy_errors)

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


# ------------------------------------------------------------------------------------------------ the mixed frames
def clamp_rec(rec, B, H, W):
    """the clamps of the header: partner into [0, B), yl / yh into [0, H], xl / xh into [0, W], a mode outside {1, 2} (or a sample that
    is its own partner) = 0  -> list of (q, mode, yl, yh, xl, xh)"""
    out = []
    for b, (q, mode, yl, yh, xl, xh) in enumerate(rec.tolist()):
        q = min(max(q, 0), B - 1)
        mode = mode if mode in (1, 2) and q != b else 0
        out.append((q, mode, min(max(yl, 0), H), min(max(yh, 0), H), min(max(xl, 0), W), min(max(xh, 0), W)))
    return out


def mixed_frames_ref(src, out_hw, index, geom, rec, lam, mean=None, std=None, bug=None, base=None):
    """fp32 [B, C, H, W]: every sample cut with its own index and geom row (frames_ref), then sample b mixed with sample q = partner[b]:
    mode 1 a.mul(l).add(p.mul(1 - l)) with l = lam[b] as an fp32 tensor (three rounded fp32 operations), mode 2 the partner's pixels
    inside [yl, yh) x [xl, xh).  bug: one of FRAME_BUGS (the host test's planted mistakes).  base: the unmixed frames where the caller
    has them already (a large batch through frames_ref_tv)."""
    H, W = out_hw
    base = D.frames_ref(src, out_hw, index, geom, mean, std) if base is None else base
    B = base.shape[0]
    if bug == "partner_receiver_geom":            # the partner's frame, cut with the RECEIVER's crop and flip
        Nsrc = src.shape[0]
        idx = list(range(B)) if index is None else [min(max(int(i), 0), Nsrc - 1) for i in index]
    out = base.clone()
    for b, (q, mode, yl, yh, xl, xh) in enumerate(clamp_rec(rec, B, H, W)):
        if mode == 0:
            continue
        p = base[q]
        if bug == "partner_receiver_geom":
            p = D.frames_ref(src, out_hw, [idx[q]], None if geom is None else geom[b:b + 1], mean, std)[0]
        a = base[b]
        if mode == 1:
            l = lam[b].to(F32)
            m = 1 - l
            if bug == "lam_swapped":
                l, m = m, l
            if bug == "fma":                      # a * l unrounded inside the sum: what a fused multiply-add computes
                out[b] = (a.to(F64) * l.to(F64) + p.mul(m).to(F64)).to(F32)
            else:
                out[b] = a.mul(l).add(p.mul(m))
        else:
            if bug == "box_inclusive":
                yh, xh = min(yh + 1, H), min(xh + 1, W)
            out[b, :, yl:yh, xl:xh] = p[:, yl:yh, xl:xh]
    return out


FRAME_BUGS = ("partner_receiver_geom", "box_inclusive", "lam_swapped", "fma")


# ------------------------------------------------------------------------------------------------ the soft-target cross-entropy
def soft_target(V, ya, yb, lam, smoothing, dtype=F64):
    """t [M, V] = (1-e) (l onehot(ya) + (1-l) onehot(yb)) + e / V; lam None: l = 1, yb unused"""
    M = ya.numel()
    t = torch.zeros((M, V), dtype=dtype)
    if lam is None:
        t.scatter_add_(1, ya[:, None], torch.ones((M, 1), dtype=dtype))
    else:
        l = lam.to(dtype)
        t.scatter_add_(1, ya[:, None], l[:, None])
        t.scatter_add_(1, yb[:, None], (1 - l)[:, None])
    return t * (1 - smoothing) + smoothing / V


def soft_ce_ref(logits, ya, yb=None, lam=None, smoothing=0.0, grad_out=1.0):
    """float64, on the logits as stored: loss_row, lse, mean (over all M rows), count = M, grad = (softmax - t) * grad_out / M.
    A zero weight forms no term (0 * -inf is not formed), and smoothing == 0 forms no sum over the row."""
    x = logits.to(F64)
    M, V = x.shape
    m = x.max(dim=-1, keepdim=True).values
    lse = (m + (x - m).exp().sum(dim=-1, keepdim=True).log()).squeeze(1)
    t = soft_target(V, ya, yb, lam, smoothing)
    tx = torch.where(t != 0, t * x, torch.zeros_like(x))
    loss_row = lse - tx.sum(-1)
    grad = ((x - lse[:, None]).exp() - t) * (grad_out / M)
    return {"loss_row": loss_row, "lse": lse, "mean": loss_row.sum() / M, "count": M, "grad": grad}


def soft_ce_torch32(logits, ya, yb=None, lam=None, smoothing=0.0, grad_out=1.0):
    """torch's own fp32 CPU evaluation of (-t * log_softmax(x.float())).sum(-1).mean() and its autograd gradient: the yardstick e32"""
    x = logits.detach().to(F32).clone().requires_grad_(True)
    t = soft_target(x.shape[1], ya, yb, lam, smoothing, F32)
    logp = torch.log_softmax(x, dim=-1)
    loss_row = -torch.where(t != 0, t * logp, torch.zeros_like(logp)).sum(-1)
    mean = loss_row.mean()
    (mean * grad_out).backward()
    return {"loss_row": loss_row.detach(), "lse": torch.logsumexp(x.detach(), dim=-1), "mean": mean.detach(), "grad": x.grad}


def standin_ce(logits, ya, yb=None, lam=None, smoothing=0.0, grad_out=1.0, bug=None):
    """What the kernels compute, in torch fp32: max, exp of the difference, sum, log; the row's plain sum; the loss of the header's
    formula; the one-pass gradient.  bug: one of CE_BUGS."""
    x = logits.to(F32)
    M, V = x.shape
    e = smoothing
    m = x.max(dim=-1, keepdim=True).values
    lse = (m + (x - m).exp().sum(dim=-1, keepdim=True).log()).squeeze(1)
    xa = x.gather(1, ya[:, None]).squeeze(1)
    if lam is None:
        l, yb_, xb = torch.ones(M, dtype=F32), ya, xa
    else:
        l, yb_, xb = lam.to(F32), yb, x.gather(1, yb[:, None]).squeeze(1)
    lb = 1 - l
    if bug == "smooth_ya_only":                   # the smoothing applied to ya's one-hot alone
        wa, wb, ua = (1 - e) * l, lb, l * e / V
    else:
        wa, wb, ua = (1 - e) * l, (1 - e) * lb, torch.full((M,), e / V, dtype=F32)
    inner = torch.where(wa != 0, wa * xa, torch.zeros_like(xa)) + torch.where(wb != 0, wb * xb, torch.zeros_like(xb))
    if e != 0 and bug != "no_sum_x":
        inner = inner + ua * x.sum(-1)
    loss_row = lse - inner
    count = (M - 1 if M > 1 else 2) if bug == "mean_wrong_count" else M
    mean = loss_row.sum() / count
    t = torch.zeros_like(x)
    t.scatter_add_(1, ya[:, None], wa[:, None])
    if bug != "grad_no_yb":
        t.scatter_add_(1, yb_[:, None], wb[:, None])
    t = t + ua[:, None]
    grad = ((x - lse[:, None]).exp() - t) * torch.tensor(grad_out / M, dtype=F32)
    return {"loss_row": loss_row, "lse": lse, "mean": mean, "grad": grad}


CE_BUGS = ("smooth_ya_only", "no_sum_x", "grad_no_yb", "mean_wrong_count")


def standin(what, *args, bug=None, **kwargs):
    """the torch stand-in of the prep kernel ("frames": mixed_frames_ref's arguments) or of the loss ("ce": standin_ce's), with one of
    the planted mistakes"""
    if what == "frames":
        return mixed_frames_ref(*args, bug=bug, **kwargs)
    if what == "ce":
        return standin_ce(*args, bug=bug, **kwargs)
    raise ValueError(what)


# ------------------------------------------------------------------------------------------------ shared cases
MEAN, STD = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
# the geometry family of test_gpu_data.py: name -> (Nsrc, Hs, Ws, C, H, W, p); source rows of 13 * 3 = 39 bytes in the small ones
GEOMS = {
    "fast_p4":       (5, 11, 13, 3, 8, 8, 4),
    "generic_c1_p2": (5, 11, 13, 1, 8, 8, 2),
    "generic_c3_p2": (5, 11, 13, 3, 8, 8, 2),
    "generic_c4_p4": (5, 11, 13, 4, 8, 8, 4),
    "fast_p16":      (4, 37, 41, 3, 32, 32, 16),
}
# B -> (index, geom) per family: B = 3 has a middle sample that is its own partner, B = 4 repeated and out-of-order frames; of every
# pair (b, B-1-b) one sample is flipped and the other is not
SMALL_BATCH = {3: ([4, 0, 4], [[0, 3, 1], [3, 5, 1], [1, 0, 0]]),
               4: ([4, 2, 2, 0], [[2, 5, 1], [0, 0, 0], [3, 1, 1], [1, 4, 0]])}
BIG_BATCH = {3: ([3, 0, 3], [[5, 9, 1], [0, 0, 0], [2, 7, 0]]),
             4: ([3, 1, 1, 0], [[5, 9, 1], [0, 0, 0], [2, 7, 1], [5, 8, 0]])}
RECORDS = ("none", "mixup", "cut_a", "cut_b", "mixed")
MIX_LAMS = (0.3, 1.0, 0.0, 0.5)              # 0.5, 0 and 1 make exact products: 0.3 sits where B = 3 has a mixed row


def boxes(H, W):
    """(yl, yh, xl, xh): an empty box, the whole image, columns 1..5 of every row (cuts two 4-pixel lane groups), the last row and column"""
    return [(3, 3, 2, 5), (0, H, 0, W), (0, H, 1, 6), (H - 1, H, W - 1, W)]


def record(name, B, H, W):
    """(rec int32 [B, 6], lam fp32 [B]) of one of RECORDS; partner = B-1-b"""
    bx = boxes(H, W)
    rows, lams = [], []
    for b in range(B):
        if name == "none":
            mode, box, lam = 0, (0, 0, 0, 0), 1.0
        elif name == "mixup":
            mode, box, lam = 1, (0, 0, 0, 0), MIX_LAMS[b % 4]
        elif name in ("cut_a", "cut_b"):
            mode, box, lam = 2, bx[(b + (2 if name == "cut_b" else 0)) % 4], 0.75
        else:                                     # mixed modes per row
            mode, box, lam = [(1, (0, 0, 0, 0), 0.3), (2, bx[2], 0.5), (0, bx[1], 1.0), (2, bx[3], 0.25)][b % 4]
        rows.append([B - 1 - b, mode, *box])
        lams.append(lam)
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(lams, dtype=F32)


def frames_case(geom_name, B):
    """(src uint8 [Nsrc, Hs, Ws, C], index list, geom int32 [B, 3]) on the CPU, from the names alone"""
    Nsrc, Hs, Ws, C, H, W, p = GEOMS[geom_name]
    g = torch.Generator().manual_seed(sum(map(ord, geom_name)) + B)
    src = torch.randint(0, 256, (Nsrc, Hs, Ws, C), generator=g, dtype=torch.uint8)
    index, geom = (BIG_BATCH if geom_name == "fast_p16" else SMALL_BATCH)[B]
    return src, index, torch.tensor(geom, dtype=torch.int32)


LAMS = (0.3, 0.625, 0.0, 1.0, 0.5)


def ce_case(M, V, seed=0, bf16=False):
    """(logits [M, V], ya, yb, lam) on the CPU: lam cycles through LAMS (0 and 1 among them), row 1 has ya == yb, every other row
    ya != yb.  Computed from the seed alone; callers must not write to it."""
    g = torch.Generator().manual_seed(1000 * seed + V + M)
    x = torch.randn((M, V), generator=g) * 2.0
    rows = torch.arange(M)
    ya = (rows * 7 + 1) % V
    yb = (ya + 1 + rows % (V - 1)) % V
    yb[rows == 1] = ya[rows == 1]
    lam = torch.tensor([LAMS[i % len(LAMS)] for i in range(M)], dtype=F32)
    return (x.to(BF16) if bf16 else x), ya, yb, lam
