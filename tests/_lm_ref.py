"""float64 restatement of the cross-entropy and token-embedding kernels (csrc/loss.hip), the bounds their tests hold them to, and a
torch fp32 stand-in of the cross-entropy kernel that the host test plants mistakes in.  No GPU, no library: plain torch on the CPU."""
import torch
import torch.nn.functional as F

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FLOOR = 8 * 2.0 ** -24          # two 1-ulp hardware transcendentals and two roundings (4 x 2^-24 relative to the lse), doubled
BF16_HALF_ULP = 2.0 ** -8 * (1 + 1 / 16)       # half a bf16 ulp, widened by a sixteenth (truncation reaches 2^-7)


# ------------------------------------------------------------------------------------------------ cross-entropy
def cross_entropy_ref(logits, target, ignore_index=-100, grad_out=1.0):
    """logits [M, V] (any float dtype, taken as stored), target int64 [M] -> float64 dict: loss_row (0 where ignored), lse, mean
    (NaN when every row is ignored), count, grad = (softmax - onehot) * grad_out / count with zero rows where ignored."""
    x = logits.to(F64)
    M, V = x.shape
    m = x.max(dim=-1, keepdim=True).values
    lse = (m + (x - m).exp().sum(dim=-1, keepdim=True).log()).squeeze(1)
    valid = target != ignore_index
    tg = torch.where(valid, target, torch.zeros_like(target))
    loss_row = torch.where(valid, lse - x.gather(1, tg[:, None]).squeeze(1), torch.zeros_like(lse))
    count = int(valid.sum())
    mean = loss_row.sum() / count if count else torch.tensor(float("nan"), dtype=F64)
    onehot = torch.zeros_like(x).scatter_(1, tg[:, None], 1.0)
    grad = ((x - lse[:, None]).exp() - onehot) * (grad_out / max(count, 1))
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return {"loss_row": loss_row, "lse": lse, "mean": mean, "count": count, "grad": grad}


def cross_entropy_torch32(logits, target, ignore_index=-100, grad_out=1.0):
    """the same quantities from torch's own fp32 CPU evaluation of F.cross_entropy(logits.float(), target): the yardstick e32"""
    x = logits.detach().to(F32).clone().requires_grad_(True)
    mean = F.cross_entropy(x, target, ignore_index=ignore_index)
    (mean * grad_out).backward()
    with torch.no_grad():
        loss_row = F.cross_entropy(x, target, ignore_index=ignore_index, reduction="none")
        lse = torch.logsumexp(x, dim=-1)
    return {"loss_row": loss_row.detach(), "lse": lse, "mean": mean.detach(), "grad": x.grad}


def standin32(logits, target, ignore_index=-100, grad_out=1.0, bug=None):
    """What the kernel computes, in torch fp32 (max, exp of the difference, sum, log; mean over the counted rows; one-pass gradient).
    bug: one of the planted mistakes of BUGS."""
    x = logits.to(F32)
    M, V = x.shape
    m = x.max(dim=-1, keepdim=True).values
    if bug == "no_max":
        m = torch.zeros_like(m)
    lse = (m + (x - m).exp().sum(dim=-1, keepdim=True).log()).squeeze(1)
    valid = target != ignore_index
    tg = torch.where(valid, target, torch.zeros_like(target))
    loss_row = torch.where(valid, lse - x.gather(1, tg[:, None]).squeeze(1), torch.zeros_like(lse))
    count = M if bug == "mean_all" else int(valid.sum())
    mean = loss_row.sum() / count
    hot = (tg + 1) % V if bug == "onehot_off" else tg
    onehot = torch.zeros_like(x).scatter_(1, hot[:, None], 1.0)
    g = 1.0 if bug == "no_upstream" else grad_out
    p = (x - lse[:, None]).exp()
    grad = (p - onehot) * torch.tensor(g / count, dtype=F32)
    grad = torch.where(valid[:, None], grad, p if bug == "ignored_softmax" else torch.zeros_like(grad))
    return {"loss_row": loss_row, "lse": lse, "mean": mean, "grad": grad}


BUGS = ("mean_all", "no_max", "onehot_off", "no_upstream", "ignored_softmax")


def _dist(got, ref, scale):
    """max |got - ref| / scale over every element; NaN or inf anywhere in got (where ref is finite) counts as infinite"""
    d = (got.to(F64) - ref).abs() / scale
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    return float(d.max()) if d.numel() else 0.0


def cross_entropy_errors(got, ref):
    """The normalised distances the bounds are stated on: per-row loss and lse over max(1, |lse_ref|), the mean over max(1, |mean_ref|),
    the gradient times count over max(1, |lse_ref|) of its row.  got: dict with loss_row, lse, mean, grad (any present)."""
    row_scale = ref["lse"].abs().clamp_min(1.0)
    out = {}
    if "loss_row" in got:
        out["loss_row"] = _dist(got["loss_row"], ref["loss_row"], row_scale)
    if "lse" in got:
        out["lse"] = _dist(got["lse"], ref["lse"], row_scale)
    if "mean" in got:
        out["mean"] = _dist(got["mean"].reshape(1), ref["mean"].reshape(1), ref["mean"].abs().clamp_min(1.0).reshape(1))
    if "grad" in got:
        out["grad"] = _dist(got["grad"].to(F64) * max(ref["count"], 1), ref["grad"] * max(ref["count"], 1), row_scale[:, None])
    return out


def bound(e32):
    """max(4 x torch fp32's own distance from float64 at this shape, the floor): the suite's rule of test_gpu_streaming.py"""
    return max(4 * e32, FLOOR)


def check_cross_entropy(got, ref, t32, label=""):
    """-> list of failure strings (empty = within every bound).  got / t32: dicts as cross_entropy_torch32 returns."""
    e, e32 = cross_entropy_errors(got, ref), cross_entropy_errors(t32, ref)
    fails = []
    for k, v in e.items():
        b = bound(e32[k])
        print(f"{label} {k}: {v:.3e} (torch fp32 {e32[k]:.3e}, bound {b:.3e})")
        if not v <= b:
            fails.append(f"{label} {k}: {v:.3e} > {b:.3e}")
    return fails


def check_bf16_grad(got_bf16, ref, t32, label=""):
    """|got - ref| <= 2^-8 (1 + 1/16) |ref| + the fp32 bound of that row, on every element -> list of failure strings"""
    e32 = cross_entropy_errors({"grad": t32["grad"]}, ref)["grad"]
    row_scale = ref["lse"].abs().clamp_min(1.0)[:, None]
    allow = BF16_HALF_ULP * ref["grad"].abs() + bound(e32) * row_scale / max(ref["count"], 1)
    d = (got_bf16.to(F64) - ref["grad"]).abs()
    bad = ~(d <= allow)
    worst = float((d / allow.clamp_min(1e-300)).max())
    print(f"{label} bf16 grad: worst |got - ref| / allowance {worst:.3f}")
    return [f"{label} bf16 grad: {int(bad.sum())} elements outside, worst ratio {worst:.3f}"] if bool(bad.any()) else []


# ------------------------------------------------------------------------------------------------ embedding
def embed_ref(tok, pos, ids):
    """tok[ids] + pos[:S] in the tables' dtype (one add per element)"""
    return tok[ids] + pos[: ids.shape[1]]


def embed_grads_ref(g, ids, tok_rows, pos_rows):
    """float64 scatter sums of g [B, S, D]: dtok [tok_rows, D] (ids outside the table add nothing), dpos [pos_rows, D] (rows >= S zero)"""
    B, S, D = g.shape
    g64 = g.to(F64)
    flat = ids.reshape(-1)
    ok = (flat >= 0) & (flat < tok_rows)
    dtok = torch.zeros((tok_rows, D), dtype=F64).index_add_(0, flat[ok], g64.reshape(B * S, D)[ok])
    dpos = torch.zeros((pos_rows, D), dtype=F64)
    dpos[:S] = g64.sum(dim=0)
    return dtok, dpos
