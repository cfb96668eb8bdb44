"""float64 restatement of the four tokenizer kernels (csrc/tokenizer.hip: the cosine-similarity VQ quantiser and the reconstruction loss on
tokens, forward and backward), the bounds their tests hold them to, torch's own evaluation of the same expressions (the yardstick, and in
float64 the check of the restatement), and torch fp32 stand-ins that the host test plants mistakes in.  No GPU, no library: plain torch.

Bounds.  Every fp32 result is measured against float64 as max |got - ref| / scale and held to max(4 e32, 8 * 2^-24), e32 being the same
distance for torch's fp32 CPU evaluation at that shape (the rule of tests/_lm_ref.py).  Scales: max(1, |ref|) per element, after the
result has been brought to order one - gradients that carry a 1 / (number of elements) factor are multiplied by that number first (dy by
E = B c H W, dcodebook by M d), as the cross-entropy gradient is by its row count.  On top: a bf16 gradient may be half a bf16 ulp (+1/16)
of the reference away; a dcodebook element may be n_k 2^-24 sum|terms| further away, n_k rows having picked its code (the order in which
fp32 adds n_k terms is free)."""
import torch
import torch.nn.functional as F

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EPS = 1e-12
FLOOR = 8 * 2.0 ** -24
BF16_HALF_ULP = 2.0 ** -8 * (1 + 1 / 16)
GAP = 1e-5                       # rows whose best and second-best squared distance are closer than this may pick either code


def bound(e32):
    return max(4 * e32, FLOOR)


def _dist(got, ref, scale=None):
    """max |got - ref| / max(1, |ref|) (or the given scale); a NaN or inf in got where ref is finite counts as infinite"""
    ref = ref.to(F64)
    d = (got.to(F64) - ref).abs() / (ref.abs().clamp_min(1.0) if scale is None else scale)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    return float(d.max()) if d.numel() else 0.0


# ------------------------------------------------------------------------------------------------ quantiser
def vq_inputs(M, K, d, seed):
    """x ~ N(0, 1), codebook ~ U(-1/K, 1/K) as train_titok.Quantizer initialises it, g_q ~ N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, d, generator=g), (torch.rand(K, d, generator=g) * 2 - 1) / K, torch.randn(M, d, generator=g)


def vq_ref(x, cb, g_q=None, g_loss=1.0, idx=None):
    """float64, from the formulas of include/vitamd.h.  idx: use these ids instead of the search's own (the search still runs: idx_ref, gap).
    -> dict: unit, rnorm, eunit, idx_ref, gap (second-best minus best squared distance, inf when K == 1), idx (the ids used), q, loss,
    dx, dcb, terms_abs (sum over the rows of a code of |their dcb terms|), n_k (rows per code)"""
    x, cb = x.to(F64), cb.to(F64)
    (M, d), K = x.shape, cb.shape[0]
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    den = n.clamp_min(EPS)
    u = x / den
    eunit = cb / cb.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(EPS)
    dist = torch.stack([(u - eunit[k]).pow(2).sum(-1) for k in range(K)], dim=1)           # [M, K]
    idx_ref = dist.argmin(dim=1)                                                          # the first minimum
    best = dist.gather(1, idx_ref[:, None]).squeeze(1)
    if K > 1:
        rest = dist.clone().scatter_(1, idx_ref[:, None], float("inf"))
        gap = rest.min(dim=1).values - best
    else:
        gap = torch.full((M,), float("inf"), dtype=F64)
    use = idx_ref if idx is None else idx
    p = cb[use]
    s = float(g_loss)
    gq = torch.zeros_like(x) if g_q is None else g_q.to(F64)
    du = gq + 0.5 * s * (u - p) / (M * d)
    dx = torch.where(n >= EPS, (du - u * (u * du).sum(-1, keepdim=True)) / den, du / EPS)
    terms = 2 * s * (p - u) / (M * d)
    dcb = torch.zeros_like(cb).index_add_(0, use, terms)
    terms_abs = torch.zeros_like(cb).index_add_(0, use, terms.abs())
    n_k = torch.zeros(K, dtype=F64).index_add_(0, use, torch.ones(M, dtype=F64))
    return {"unit": u, "rnorm": (1 / den).squeeze(1), "eunit": eunit, "idx_ref": idx_ref, "gap": gap, "idx": use, "q": u + (p - u),
            "loss": 1.25 * (p - u).pow(2).mean(), "dx": dx, "dcb": dcb, "terms_abs": terms_abs, "n_k": n_k}


def vq_torch(x, cb, idx, g_q, g_loss=1.0, dtype=F32):
    """torch's own evaluation (CPU autograd) of train_titok.Quantizer.forward's expressions with the ids given: unit, q, loss, dx, dcb"""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    cb = cb.detach().to(dtype).clone().requires_grad_(True)
    unit = F.normalize(x, dim=-1)
    picked = cb[idx]
    sq = lambda t: t.pow(2).mean()
    loss = sq(picked - unit.detach()) + 0.25 * sq(picked.detach() - unit)
    q = unit + (picked - unit).detach()
    ((q * g_q.to(dtype)).sum() + loss * g_loss).backward()
    return {"unit": unit.detach(), "q": q.detach(), "loss": loss.detach(), "dx": x.grad, "dcb": cb.grad}


VQ_BUGS = ("unit_codes", "no_quarter", "dcb_from_gq", "no_projection", "mean_tokens")


def vq_standin32(x, cb, idx, g_q, g_loss=1.0, bug=None):
    """what the two quantiser kernels compute, in torch fp32 with a hand-written backward; bug: one of VQ_BUGS"""
    x, cb, g_q = x.to(F32), cb.to(F32), g_q.to(F32)
    M, d = x.shape
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    den = n.clamp_min(EPS)
    u = x / den
    p = cb[idx]
    if bug == "unit_codes":
        p = p / p.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(EPS)
    count = M if bug == "mean_tokens" else M * d
    commit = 1.0 if bug == "no_quarter" else 0.25
    loss = (1 + commit) * (p - u).pow(2).sum() / count
    s = torch.tensor(g_loss, dtype=F32)
    du = g_q + 2 * commit * s * (u - p) / count
    proj = 0.0 if bug == "no_projection" else u * (u * du).sum(-1, keepdim=True)
    dx = torch.where(n >= EPS, (du - proj) / den, du / EPS)
    terms = 2 * s * (p - u) / count + (g_q if bug == "dcb_from_gq" else 0.0)
    return {"unit": u, "q": u + (p - u), "loss": loss, "dx": dx, "dcb": torch.zeros_like(cb).index_add_(0, idx, terms)}


def vq_errors(got, ref):
    """the normalised distances of whatever of unit, q, loss, dx, dcb is in got (dcb: times M d, the summation-order allowance taken off)"""
    M, d = ref["unit"].shape
    out = {}
    for k in ("unit", "q", "dx"):
        if k in got:
            out[k] = _dist(got[k], ref[k])
    if "loss" in got:
        out["loss"] = _dist(got["loss"].reshape(1), ref["loss"].reshape(1))
    if "dcb" in got:
        md = M * d
        over = ((got["dcb"].to(F64) - ref["dcb"]).abs() - ref["n_k"][:, None] * 2.0 ** -24 * ref["terms_abs"]).clamp_min(0.0) * md
        over = over / (ref["dcb"] * md).abs().clamp_min(1.0)
        out["dcb"] = float(torch.where(torch.isfinite(over), over, torch.full_like(over, float("inf"))).max())
    return out


def check_vq(got, ref, t32, label=""):
    """-> list of failure strings (empty = within every bound); prints every figure"""
    e, e32 = vq_errors(got, ref), vq_errors(t32, ref)
    fails = []
    for k, v in e.items():
        b = bound(e32[k])
        print(f"{label} {k}: {v:.3e} (torch fp32 {e32[k]:.3e}, bound {b:.3e})")
        if not v <= b:
            fails.append(f"{label} {k}: {v:.3e} > {b:.3e}")
    return fails


def check_ids(got_idx, ref, label=""):
    """ids equal to the reference's wherever its gap is >= GAP; at most 1 % of the rows exempt -> (failures, exempt mask)"""
    exempt = ref["gap"] < GAP
    wrong = (got_idx != ref["idx_ref"]) & ~exempt
    print(f"{label} ids: {int(wrong.sum())} wrong, {int(exempt.sum())} of {exempt.numel()} rows exempt")
    fails = []
    if bool(wrong.any()):
        fails.append(f"{label} ids: {int(wrong.sum())} rows differ outside near-ties")
    if float(exempt.double().mean()) > 0.01:
        fails.append(f"{label} ids: {int(exempt.sum())} of {exempt.numel()} rows are near-ties (more than 1 %)")
    return fails, exempt


# ------------------------------------------------------------------------------------------------ reconstruction loss
def recon_inputs(B, G, p, c, seed, dtype=F32):
    """tokens ~ N(0.5, 0.5) in dtype, images ~ U(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B * G * G, p * p * c, generator=g) * 0.5 + 0.5).to(dtype)
    return y, torch.rand(B, c, G * p, G * p, generator=g)


def recon_index(B, G, p, c, order="p1p2c"):
    """for every image element [B, c, H, W]: (token row, token column) by the formula of include/vitamd.h; order 'cp1p2': the planted
    mistake that lays a token out channel-first"""
    H = G * p
    b, ch, h, w = torch.meshgrid(torch.arange(B), torch.arange(c), torch.arange(H), torch.arange(H), indexing="ij")
    gh, p1, gw, p2 = h // p, h % p, w // p, w % p
    row = b * G * G + gh * G + gw
    col = (p1 * p + p2) * c + ch if order == "p1p2c" else (ch * p + p1) * p + p2
    return row, col


def recon_ref(y, img, G, p, grad_out=1.0):
    """float64: loss and dy (token layout) of mean((float(y)[row, col] - img)^2)"""
    B, c = img.shape[:2]
    row, col = recon_index(B, G, p, c)
    y64, img64 = y.to(F64), img.to(F64)
    diff = y64[row, col] - img64
    dy = torch.zeros_like(y64)
    dy[row, col] = 2 * diff * float(grad_out) / img.numel()
    return {"loss": diff.pow(2).mean(), "dy": dy, "E": img.numel()}


def pixel_shuffle(y, B, G, p, c):
    """train_titok.pixel_shuffle_tokens on [B*G*G, F]"""
    return y.view(B, G, G, p, p, c).permute(0, 5, 1, 3, 2, 4).reshape(B, c, G * p, G * p)


def recon_torch(y, img, G, p, grad_out=1.0, dtype=F32):
    """torch's own evaluation (CPU autograd) of mse_loss(pixel_shuffle_tokens(float(tokens)), images)"""
    B, c = img.shape[:2]
    t = y.detach().to(dtype).clone().requires_grad_(True)
    loss = F.mse_loss(pixel_shuffle(t, B, G, p, c), img.to(dtype))
    (loss * grad_out).backward()
    return {"loss": loss.detach(), "dy": t.grad}


RECON_BUGS = ("chan_order", "no_upstream", "mean_tokens")


def recon_standin32(y, img, G, p, grad_out=1.0, bug=None):
    """what the two reconstruction kernels compute, in torch fp32; bug: one of RECON_BUGS"""
    B, c = img.shape[:2]
    row, col = recon_index(B, G, p, c, "cp1p2" if bug == "chan_order" else "p1p2c")
    y32 = y.to(F32)
    diff = y32[row, col] - img
    count = B * G * G if bug == "mean_tokens" else img.numel()
    dy = torch.zeros_like(y32)
    dy[row, col] = 2 * diff * torch.tensor((1.0 if bug == "no_upstream" else grad_out) / count, dtype=F32)
    return {"loss": diff.pow(2).sum() / count, "dy": dy}


def recon_errors(got, ref):
    out = {}
    if "loss" in got:
        out["loss"] = _dist(got["loss"].reshape(1), ref["loss"].reshape(1))
    if "dy" in got:
        out["dy"] = _dist(got["dy"].to(F64) * ref["E"], ref["dy"] * ref["E"])
    return out


def check_recon(got, ref, t32, label=""):
    e, e32 = recon_errors(got, ref), recon_errors(t32, ref)
    fails = []
    for k, v in e.items():
        b = bound(e32[k])
        print(f"{label} {k}: {v:.3e} (torch fp32 {e32[k]:.3e}, bound {b:.3e})")
        if not v <= b:
            fails.append(f"{label} {k}: {v:.3e} > {b:.3e}")
    return fails


def check_recon_bf16(got_bf16, ref, t32, label=""):
    """|got - ref| <= 2^-8 (1 + 1/16) |ref| + the fp32 bound of that element, on every element -> list of failure strings"""
    E = ref["E"]
    e32 = recon_errors({"dy": t32["dy"]}, ref)["dy"]
    allow = BF16_HALF_ULP * ref["dy"].abs() + bound(e32) * (ref["dy"] * E).abs().clamp_min(1.0) / E
    d = (got_bf16.to(F64) - ref["dy"]).abs()
    bad = ~(d <= allow)
    worst = float((d / allow.clamp_min(1e-300)).max())
    print(f"{label} bf16 dy: worst |got - ref| / allowance {worst:.3f}")
    return [f"{label} bf16 dy: {int(bad.sum())} elements outside, worst ratio {worst:.3f}"] if bool(bad.any()) else []


# ------------------------------------------------------------------------------------------------ the cases both test files use
VQ_SHAPES = [(1, 1, 1), (255, 2, 1), (257, 257, 17), (600, 513, 12), (300, 300, 64)]      # (M, K, d)
# (B, G, p, c): the last three take the kernel's other paths - 12-KiB fp32 tokens cut a grid row of 5 into strips of 4 + 1; a patch of 2
# has no four consecutive pixels in one token (the image is then read pixel by pixel); a grid row of 9 is the shortest that is cut in bf16
# too (6-KiB tokens: strips of 8 + 1, fp32 4 + 4 + 1)
RECON_SHAPES = [(2, 1, 4, 3), (1, 2, 16, 3), (2, 16, 16, 3), (1, 3, 8, 1), (1, 5, 32, 3), (1, 3, 2, 2), (1, 9, 32, 3)]
G_LOSS, G_UP = 2.5, 2.5          # upstream gradients other than 1


def vq_seed(i):
    """case 1 (K = 2, d = 1) takes a seed whose two codes differ in sign: with equal signs both unit codes are the same point and every
    row is an exact tie, which the first-minimum rule decides but the near-tie exemption would hide"""
    return 204 if i == 1 else 200 + i
