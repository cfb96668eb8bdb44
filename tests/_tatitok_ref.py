"""float64 restatement of the kernels of the 1D TiTok tokenizer (csrc/tokenizer.hip) - the fused pixel tail
(pixel shuffle -> conv3x3 -> mean squared error, forward and backward) and the unit-code quantiser - with the bounds their tests hold them
to, torch's own fp32 evaluation of the same expressions (the yardstick) and torch fp32 stand-ins that the host test plants mistakes in.
No GPU, no library: plain torch.  The tail's reference is F.conv2d in float64 on the tokens as stored.

Bounds: those of tests/_tokenizer_ref.py.  Every fp32 result is measured against float64 as max |got - ref| / max(1, |ref|) and held to
bound(e32) = max(4 e32, 8 * 2^-24), e32 being the same distance for torch's fp32 CPU evaluation at that shape.  Gradients that carry a
1 / (number of elements) factor are brought to order one first: the tail's by E = B 3 H W (the upstream g_recon of the cases is drawn
at scale 1 / E for that reason, as a perceptual term's is), dcodebook by M d.  On top: a bf16 gradient may be half a bf16 ulp (+1/16) of
the reference away; dw / db and dcodebook may be n 2^-24 sum|terms| further away, n the number of terms of the sum (the order in which
fp32 adds them is free): n = B H W for dw and db; for a code picked by n_k rows, n = n_k + d and the terms are the rows' terms divided by
|e_k| plus those of the projection's dot product, |e^_c| |t_c|."""
import torch
import torch.nn.functional as F

import _tokenizer_ref as R
from _tokenizer_ref import BF16_HALF_ULP, EPS, _dist, bound

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


# ------------------------------------------------------------------------------------------------ pixel tail
# (B, grid, patch): every pixel on a border; token seams and an image boundary inside one launch; a 40-pixel side (more than the kernel's
# 32-pixel tile and no multiple of it); a patch of 16
TAIL_SHAPES = [(1, 1, 8), (2, 3, 8), (1, 5, 8), (1, 2, 16)]
G_LOSS = 2.5


def tail_inputs(B, G, p, seed, dtype=F32):
    """tokens ~ N(0.5, 0.5) in dtype [B*G*G, 3 p p], images ~ U(0, 1), conv weight ~ N(0, 0.3), bias ~ N(0, 0.3), g_recon ~ N(0, 1) / E"""
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B * G * G, p * p * 3, generator=g) * 0.5 + 0.5).to(dtype)
    img = torch.rand(B, 3, G * p, G * p, generator=g)
    w = torch.randn(3, 3, 3, 3, generator=g) * 0.3
    b = torch.randn(3, generator=g) * 0.3
    g_recon = torch.randn(B, 3, G * p, G * p, generator=g) / img.numel()
    return y, img, w, b, g_recon


def _autograd_tail(y, img, w, b, G, p, g_loss, g_recon, dtype):
    B = img.shape[0]
    t = y.detach().to(dtype).clone().requires_grad_(True)
    w_, b_ = w.detach().to(dtype).clone().requires_grad_(True), b.detach().to(dtype).clone().requires_grad_(True)
    yimg = R.pixel_shuffle(t, B, G, p, 3)
    r = F.conv2d(yimg, w_, b_, padding=1)
    loss = (r - img.to(dtype)).pow(2).mean()
    total = loss * g_loss
    if g_recon is not None:
        total = total + (r * g_recon.to(dtype)).sum()
    total.backward()
    return t, w_, b_, yimg.detach(), r.detach(), loss.detach()


def tail_ref(y, img, w, b, G, p, g_loss=1.0, g_recon=None):
    """float64 (autograd through F.conv2d): loss, recon, dtok (token layout), dw, db, and the sums of |terms| of dw and db"""
    t, w_, b_, yimg, r, loss = _autograd_tail(y, img, w, b, G, p, g_loss, g_recon, F64)
    E = img.numel()
    e = g_loss * 2 * (r - img.to(F64)) / E + (0 if g_recon is None else g_recon.to(F64))
    wz = torch.zeros(3, 3, 3, 3, dtype=F64, requires_grad=True)
    (F.conv2d(yimg.abs(), wz, None, padding=1) * e.abs()).sum().backward()           # linear in wz: its gradient is sum |e| |yimg shifted|
    return {"loss": loss, "recon": r, "dtok": t.grad, "dw": w_.grad, "db": b_.grad, "dw_abs": wz.grad, "db_abs": e.abs().sum(dim=(0, 2, 3)),
            "E": E, "n": E // 3}


def tail_torch(y, img, w, b, G, p, g_loss=1.0, g_recon=None):
    """torch's own fp32 evaluation (CPU autograd) of the same expressions"""
    t, w_, b_, _, r, loss = _autograd_tail(y, img, w, b, G, p, g_loss, g_recon, F32)
    return {"loss": loss, "recon": r, "dtok": t.grad, "dw": w_.grad, "db": b_.grad}


CONV_BUGS = ("unflipped_taps", "chan_order", "replicate_pad", "neighbour_halo", "no_db", "no_g_recon", "mean_tokens")


def tail_standin32(y, img, w, b, G, p, g_loss=1.0, g_recon=None, bug=None):
    """what the two tail kernels compute, in torch fp32 with a hand-written backward; bug: one of CONV_BUGS.  neighbour_halo: the halo
    rows above and below an image come from the images before and after it in the batch (cyclically, so that a batch of one shows it)"""
    B, H = img.shape[0], G * p
    y32, w32, b32 = y.to(F32), w.to(F32), b.to(F32)
    row, col = R.recon_index(B, G, p, 3, "cp1p2" if bug == "chan_order" else "p1p2c")
    yimg = y32[row, col]
    ypad = F.pad(yimg, (1, 1, 1, 1), mode="replicate" if bug == "replicate_pad" else "constant")
    if bug == "neighbour_halo":
        ypad[:, :, 0, 1:-1] = yimg.roll(1, 0)[:, :, -1]
        ypad[:, :, -1, 1:-1] = yimg.roll(-1, 0)[:, :, 0]
    r = F.conv2d(ypad, w32, b32)
    count = B * G * G if bug == "mean_tokens" else img.numel()
    loss = (r - img).pow(2).sum() / count
    e = 2 * (r - img) * torch.tensor(g_loss / count, dtype=F32)
    if g_recon is not None and bug != "no_g_recon":
        e = e + g_recon.to(F32)
    wt = w32.transpose(0, 1)
    dimg = F.conv2d(e, wt if bug == "unflipped_taps" else wt.flip(2, 3), padding=1)
    dw = torch.nn.grad.conv2d_weight(ypad, w32.shape, e)
    db = torch.zeros(3) if bug == "no_db" else e.sum(dim=(0, 2, 3))
    dtok = torch.zeros_like(y32)
    dtok[row, col] = dimg
    return {"loss": loss, "recon": r, "dtok": dtok, "dw": dw, "db": db}


def _over(got, ref, allow, scale):
    """max over the elements of (|got - ref| - allow)+ * scale / max(1, |ref| * scale); NaN or inf counts as infinite"""
    d = ((got.to(F64) - ref).abs() - allow).clamp_min(0.0) * scale / (ref * scale).abs().clamp_min(1.0)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    return float(d.max())


def tail_errors(got, ref):
    """the normalised distances of whatever of loss, recon, dtok, dw, db is in got (gradients times E; dw and db with the summation-order
    allowance taken off)"""
    E, n = ref["E"], ref["n"]
    out = {}
    if "loss" in got:
        out["loss"] = _dist(got["loss"].reshape(1), ref["loss"].reshape(1))
    if "recon" in got:
        out["recon"] = _dist(got["recon"], ref["recon"])
    if "dtok" in got:
        out["dtok"] = _dist(got["dtok"].to(F64) * E, ref["dtok"] * E)
    for k in ("dw", "db"):
        if k in got:
            out[k] = _over(got[k], ref[k], n * 2.0 ** -24 * ref[k + "_abs"], E)
    return out


def check_tail(got, ref, t32, label=""):
    """-> list of failure strings (empty = within every bound); prints every figure"""
    e, e32 = tail_errors(got, ref), tail_errors(t32, ref)
    fails = []
    for k, v in e.items():
        bd = bound(e32[k])
        print(f"{label} {k}: {v:.3e} (torch fp32 {e32[k]:.3e}, bound {bd:.3e})")
        if not v <= bd:
            fails.append(f"{label} {k}: {v:.3e} > {bd:.3e}")
    return fails


def check_tail_bf16(got_bf16, ref, t32, label=""):
    """the bf16 token gradient: |got - ref| <= 2^-8 (1 + 1/16) |ref| + the fp32 bound of that element, on every element"""
    E = ref["E"]
    e32 = tail_errors({"dtok": t32["dtok"]}, ref)["dtok"]
    allow = BF16_HALF_ULP * ref["dtok"].abs() + bound(e32) * (ref["dtok"] * E).abs().clamp_min(1.0) / E
    d = (got_bf16.to(F64) - ref["dtok"]).abs()
    bad = ~(d <= allow)
    worst = float((d / allow.clamp_min(1e-300)).max())
    print(f"{label} bf16 dtok: worst |got - ref| / allowance {worst:.3f}")
    return [f"{label} bf16 dtok: {int(bad.sum())} elements outside, worst ratio {worst:.3f}"] if bool(bad.any()) else []


# ------------------------------------------------------------------------------------------------ unit-code quantiser
def vq_unit_ref(x, cb, g_q=None, g_loss=1.0, idx=None):
    """float64, from the formulas of include/vitamd.h (vitamd_vq_quantize_unit_*): the search of _tokenizer_ref.vq_ref, then q, the loss
    and dx on the NORMALISED code rows and the codebook gradient through the normalisation.  Same keys as vq_ref."""
    base = R.vq_ref(x, cb, g_q, g_loss, idx)
    x, cb = x.to(F64), cb.to(F64)
    (M, d), K = x.shape, cb.shape[0]
    use, u, eunit = base["idx"], base["unit"], base["eunit"]
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    den = n.clamp_min(EPS)
    p = eunit[use]
    s = float(g_loss)
    gq = torch.zeros_like(x) if g_q is None else g_q.to(F64)
    du = gq + 0.5 * s * (u - p) / (M * d)
    dx = torch.where(n >= EPS, (du - u * (u * du).sum(-1, keepdim=True)) / den, du / EPS)
    terms = 2 * s * (p - u) / (M * d)
    T = torch.zeros_like(cb).index_add_(0, use, terms)
    Tabs = torch.zeros_like(cb).index_add_(0, use, terms.abs())
    enorm = cb.pow(2).sum(-1, keepdim=True).sqrt()
    dcb = torch.where(enorm >= EPS, (T - eunit * (eunit * T).sum(-1, keepdim=True)) / enorm.clamp_min(EPS), T / EPS)
    terms_abs = (Tabs + eunit.abs() * (eunit.abs() * Tabs).sum(-1, keepdim=True)) / enorm.clamp_min(EPS)
    return dict(base, q=u + (p - u), loss=1.25 * (p - u).pow(2).mean(), dx=dx, dcb=dcb, terms_abs=terms_abs, n_k=base["n_k"] + d)


def vq_unit_torch(x, cb, idx, g_q, g_loss=1.0, dtype=F32):
    """torch's own evaluation (CPU autograd) of blocks.VectorQuantizer(use_l2_norm=True, commitment_cost=0.25).forward's expressions
    with the ids given: unit, q, loss, dx, dcb"""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    cb = cb.detach().to(dtype).clone().requires_grad_(True)
    unit = F.normalize(x, dim=-1)
    picked = F.normalize(cb[idx], dim=-1)
    commit = 0.25 * torch.mean((picked.detach() - unit) ** 2)
    code = torch.mean((picked - unit.detach()) ** 2)
    loss = commit + code
    q = unit + (picked - unit).detach()
    ((q * g_q.to(dtype)).sum() + loss * g_loss).backward()
    return {"unit": unit.detach(), "q": q.detach(), "loss": loss.detach(), "dx": x.grad, "dcb": cb.grad}


VQ_UNIT_BUGS = ("raw_codes", "no_projection", "no_quarter")


def vq_unit_standin32(x, cb, idx, g_q, g_loss=1.0, bug=None):
    """what the two unit-code quantiser kernels compute, in torch fp32 with a hand-written backward; bug: one of VQ_UNIT_BUGS"""
    x, cb, g_q = x.to(F32), cb.to(F32), g_q.to(F32)
    M, d = x.shape
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    den = n.clamp_min(EPS)
    u = x / den
    enorm = cb.pow(2).sum(-1, keepdim=True).sqrt()
    eunit = cb / enorm.clamp_min(EPS)
    p = cb[idx] if bug == "raw_codes" else eunit[idx]
    commit = 1.0 if bug == "no_quarter" else 0.25
    loss = (1 + commit) * (p - u).pow(2).sum() / (M * d)
    s = torch.tensor(g_loss, dtype=F32)
    du = g_q + 2 * commit * s * (u - p) / (M * d)
    dx = torch.where(n >= EPS, (du - u * (u * du).sum(-1, keepdim=True)) / den, du / EPS)
    T = torch.zeros_like(cb).index_add_(0, idx, 2 * s * (p - u) / (M * d))
    if bug == "raw_codes":
        dcb = T
    else:
        proj = 0.0 if bug == "no_projection" else eunit * (eunit * T).sum(-1, keepdim=True)
        dcb = torch.where(enorm >= EPS, (T - proj) / enorm.clamp_min(EPS), T / EPS)
    return {"unit": u, "q": u + (p - u), "loss": loss, "dx": dx, "dcb": dcb}


# the checkers of the quantiser are _tokenizer_ref's: check_ids, vq_errors and check_vq read the keys vq_unit_ref fills
check_vq, check_ids, vq_errors = R.check_vq, R.check_ids, R.vq_errors
