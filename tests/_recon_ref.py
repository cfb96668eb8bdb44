"""float64 statement of the tokenizer evaluation (include/vitamd_eval.h vitamd_recon_metrics and vitamd_code_hist), the
bounds its GPU tests hold the kernels to, the comparison they call, a torch fp32 restatement of the kernel's arithmetic, and the planted
mistakes the host test proves the comparison against.  No GPU, no library: plain torch on the CPU.  Our own statement of the
definitions, written from the header's contract.

The bounds (u = 2^-24, the unit roundoff of fp32; every other stage is fp64 and adds nothing visible):

mse_b, mae_b   the terms are non-negative, so the bound is relative: (SUM_DEPTH + 3) u.  SUM_DEPTH = 18 is the depth of the kernel's fp32
               summation per tile (8 serial adds per thread at most, 6 butterfly levels, 4 waves: csrc/recon_metrics.hip says the same
               number and vitamd_recon_metrics_sum_depth() returns it); + 3 for the difference, its square and a spare.
psnr_b         10 / ln 10 times the relative bound of mse_b (d psnr = -10 / ln 10 * d mse / mse).
ssim_b         derived per window from the reference's own values and averaged.  With h = R / 2 the kernel blurs the five planes
               p in {x', y', x'^2, y'^2, x'y'} of x' = fl(x - h), y' = fl(y - h).  A blurred value is two chains of 11 fused multiply-adds
               (22 roundings) over weights rounded once per pass (2) and terms that carry the shift's rounding and, for the second
               moments, the other factor's and the product's (<= 3): each blurred plane is off by at most
                   E_p = (22 + 5) u max_window |p|.
               Then  mu = fl(mu' + h):                  e_mu  = E_x' + u |mu|
                     var = fma(-mu', mu', blur(x'^2)):   e_var = E_x'x' + 2 |mu'_x| E_x' + u |var|     (cov alike, with both means)
                     A1 = 2 mu_x mu_y + C1:             dA1 = 2 (|mu_y| e_mux + |mu_x| e_muy) + 3 u |A1|
                     B1 = mu_x^2 + mu_y^2 + C1:         dB1 = 2 (|mu_x| e_mux + |mu_y| e_muy) + 4 u B1
                     A2 = 2 cov + C2:                   dA2 = 2 e_cov + 3 u (|A2| + C2)
                     B2 = var_x + var_y + C2:           dB2 = e_varx + e_vary + 3 u B2
                     S = A1 A2 / (B1 B2):               dS = [(|A2| dA1 + |A1| dA2) / (B1 B2) + |S| (dB1 / B1 + dB2 / B2)] / (1 - dB1 / B1 - dB2 / B2)
                                                             + 3 u |S|
               and ssim_b may be off by the mean of dS over the image's windows plus (SUM_DEPTH + 1) u mean |S| for the map's own sum.
running sums   the sum of the per-image bounds.
Integers (hist, bad, count) must be equal."""
import math

import torch
import torch.nn.functional as F

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
SUM_DEPTH = 18
TAP_ROUNDINGS = 22 + 5
K1, K2 = 0.01, 0.03

BUGS = ("same_padding", "unnormalised", "window7", "unbiased", "c1c2_swapped", "channel_mean", "psnr_batch_mse", "clamp_target", "nan_dropped")
ACC_BUGS = ("overwrite",)
HIST_BUGS = ("oor_bin0", "oor_binK", "usage_from_count")


def gauss(taps=11, sigma=1.5, normalise=True):
    k = torch.arange(taps, dtype=F64) - (taps - 1) / 2
    g = torch.exp(-k * k / (2 * sigma * sigma))
    return g / g.sum() if normalise else g


def _clamp(v, R):
    """the clamp of the contract: comparisons a NaN fails"""
    return torch.where(v < 0, torch.zeros_like(v), torch.where(v > R, torch.full_like(v, R), v))


def _moments(r, t, g):
    """the five blurred planes over whole windows only -> mu_x, mu_y, blur(x^2), blur(y^2), blur(xy)"""
    C, k = r.shape[1], g.numel()
    win = torch.outer(g, g).to(r.dtype).expand(C, 1, k, k).contiguous()
    blur = lambda z: F.conv2d(z, win, groups=C)
    return blur(r), blur(t), blur(r * r), blur(t * t), blur(r * t)


def ssim_map(r, t, R, bug=None):
    """float64 [B, C, H - 10, W - 10]: the SSIM map of the contract"""
    g = gauss(7 if bug == "window7" else 11, normalise=bug != "unnormalised")
    if bug == "channel_mean":
        r, t = r.mean(dim=1, keepdim=True), t.mean(dim=1, keepdim=True)
    if bug == "same_padding":
        pad = (g.numel() - 1) // 2
        r, t = F.pad(r, (pad,) * 4), F.pad(t, (pad,) * 4)
    mx, my, xx, yy, xy = _moments(r, t, g)
    vx, vy, vxy = xx - mx * mx, yy - my * my, xy - mx * my
    if bug == "unbiased":
        w2 = float((torch.outer(g, g) ** 2).sum())
        vx, vy, vxy = vx / (1 - w2), vy / (1 - w2), vxy / (1 - w2)
    c1, c2 = (K1 * R) ** 2, (K2 * R) ** 2
    if bug == "c1c2_swapped":
        c1, c2 = c2, c1
    return ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim_bound(r, t, R):
    """float64 [B]: what ssim_b may be off by (the derivation in the module docstring), from the reference's own values"""
    h = R / 2
    xs, ys = r - h, t - h
    mxs, mys, xx, yy, xy = _moments(xs, ys, gauss())
    top = lambda z: F.max_pool2d(z, 11, 1)
    E = TAP_ROUNDINGS * U
    ex, ey, exx, eyy, exy = E * top(xs.abs()), E * top(ys.abs()), E * top(xs * xs), E * top(ys * ys), E * top((xs * ys).abs())
    mx, my = mxs + h, mys + h
    vx, vy, vxy = xx - mxs * mxs, yy - mys * mys, xy - mxs * mys
    emx, emy = ex + U * mx.abs(), ey + U * my.abs()
    evx, evy = exx + 2 * mxs.abs() * ex + U * vx.abs(), eyy + 2 * mys.abs() * ey + U * vy.abs()
    evxy = exy + mxs.abs() * ey + mys.abs() * ex + U * vxy.abs()
    c1, c2 = (K1 * R) ** 2, (K2 * R) ** 2
    A1, B1, A2, B2 = 2 * mx * my + c1, mx * mx + my * my + c1, 2 * vxy + c2, vx + vy + c2
    dA1 = 2 * (my.abs() * emx + mx.abs() * emy) + 3 * U * A1.abs()
    dB1 = 2 * (mx.abs() * emx + my.abs() * emy) + 4 * U * B1
    dA2 = 2 * evxy + 3 * U * (A2.abs() + c2)
    dB2 = evx + evy + 3 * U * B2
    S = A1 * A2 / (B1 * B2)
    dS = ((A2.abs() * dA1 + A1.abs() * dA2) / (B1 * B2) + S.abs() * (dB1 / B1 + dB2 / B2)) / (1 - dB1 / B1 - dB2 / B2) + 3 * U * S.abs()
    return dS.mean(dim=(1, 2, 3)) + (SUM_DEPTH + 1) * U * S.abs().mean(dim=(1, 2, 3))


def recon_ref(recon, target, data_range=1.0, clamp=False, ssim=True, bug=None):
    """recon [B, C, H, W] in any float dtype (taken as stored), target fp32 -> {"rows": float64 [B, 4] = mse_b, mae_b, psnr_b, ssim_b,
    "bound": float64 [B, 4], what each may be off by, "sums": float64 [4], "count": B}.  bug: one of BUGS."""
    R = float(data_range)
    r, t = recon.to(F64), target.to(F64)
    if clamp:
        r = torch.nan_to_num(r, nan=0.0).clamp(0.0, R) if bug == "nan_dropped" else _clamp(r, R)
        if bug == "clamp_target":
            t = _clamp(t, R)
    d = r - t
    mse, mae = (d * d).mean(dim=(1, 2, 3)), d.abs().mean(dim=(1, 2, 3))
    psnr = 10.0 * torch.log10(R * R / (mse.mean().expand_as(mse) if bug == "psnr_batch_mse" else mse))
    rel = (SUM_DEPTH + 3) * U
    nan = torch.full_like(mse, float("nan"))
    if ssim:
        s, sb = ssim_map(r, t, R, bug).mean(dim=(1, 2, 3)), ssim_bound(r, t, R)
    else:
        s, sb = nan, nan
    rows = torch.stack([mse, mae, psnr, s], dim=1)
    bound = torch.stack([rel * mse, rel * mae, torch.full_like(mse, 10.0 / math.log(10.0) * rel), sb], dim=1)
    return {"rows": rows, "bound": bound, "sums": rows.sum(dim=0), "count": recon.shape[0]}


def accumulate(results, bug=None):
    """what the accumulators hold after the updates whose recon_ref results are given, in order"""
    sums, bound, count = torch.zeros(4, dtype=F64), torch.zeros(4, dtype=F64), 0
    for r in results:
        if bug == "overwrite":
            sums, count = r["sums"].clone(), r["count"]
        else:
            sums, count = sums + r["sums"], count + r["count"]
        bound = bound + r["bound"].sum(dim=0)
    return {"sums": sums, "count": count, "sum_bound": bound}


def kernel32(recon, target, data_range=1.0, clamp=False):
    """The kernel's arithmetic restated with torch in fp32 -> float64 [B, 4] rows: differences of the unshifted values, the five planes
    of the values shifted by R / 2 blurred by the separable fp32 taps (rows, then columns), variances from the shifted moments, the
    means with the shift added back.  Only the order of the sums differs from the kernel's (torch's convolution and reductions)."""
    R = float(data_range)
    r, t = recon.to(F32), target.to(F32)
    if clamp:
        r = _clamp(r, R)
    d = r - t
    mse, mae = (d * d).to(F64).mean(dim=(1, 2, 3)), d.abs().to(F64).mean(dim=(1, 2, 3))
    h = torch.tensor(R / 2, dtype=F32)
    xs, ys = r - h, t - h
    C = r.shape[1]
    g = gauss().to(F32)
    blur = lambda z: F.conv2d(F.conv2d(z, g.reshape(1, 1, 1, 11).expand(C, 1, 1, 11).contiguous(), groups=C),
                              g.reshape(1, 1, 11, 1).expand(C, 1, 11, 1).contiguous(), groups=C)
    m0, m1, m2, m3, m4 = blur(xs), blur(ys), blur(xs * xs), blur(ys * ys), blur(xs * ys)
    vx, vy, vxy = m2 - m0 * m0, m3 - m1 * m1, m4 - m0 * m1
    mx, my = m0 + h, m1 + h
    c1, c2 = torch.tensor((K1 * R) ** 2, dtype=F32), torch.tensor((K2 * R) ** 2, dtype=F32)
    S = ((2 * (mx * my) + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return torch.stack([mse, mae, 10.0 * torch.log10(R * R / mse), S.to(F64).mean(dim=(1, 2, 3))], dim=1)


NAMES = ("mse", "mae", "psnr", "ssim")
WORST = {}        # name -> the largest |got - ref| / bound any comparison of this process has seen (the GPU visit writes it down)


def _close(g, r, bound, what, fails, kind):
    """one number against its reference: a non-finite reference demands the same kind of non-finite value, never a number"""
    if r != r or r in (float("inf"), float("-inf")):
        if not (g != g if r != r else g == r):
            fails.append(f"{what}: got {g!r}, reference {r!r}")
        return
    err = abs(g - r)
    if bound > 0:
        WORST[kind] = max(WORST.get(kind, 0.0), err / bound)
    if not err <= bound:
        fails.append(f"{what}: |{g!r} - {r!r}| = {err:.3e} > {bound:.3e}")


def check_rows(rows, ref, label=""):
    """per-image values [B, 4] (any device) against a recon_ref result -> list of failure strings"""
    fails = []
    got = rows.detach().to(F64).cpu()
    if tuple(got.shape) != tuple(ref["rows"].shape):
        return [f"{label} rows: shape {tuple(got.shape)}, reference {tuple(ref['rows'].shape)}"]
    for b in range(got.shape[0]):
        for k, name in enumerate(NAMES):
            _close(float(got[b, k]), float(ref["rows"][b, k]), float(ref["bound"][b, k]), f"{label} image {b} {name}", fails, name)
    return fails


def check_sums(sums, count, ref, label=""):
    """the accumulators against an accumulate() result (or a recon_ref result: its own sums and the sum of its bounds)"""
    fails = []
    bound = ref["sum_bound"] if "sum_bound" in ref else ref["bound"].sum(dim=0)
    if int(count) != int(ref["count"]):
        fails.append(f"{label} count: got {int(count)}, reference {int(ref['count'])}")
    got = sums.detach().to(F64).cpu()
    for k, name in enumerate(NAMES):
        _close(float(got[k]), float(ref["sums"][k]), float(bound[k]), f"{label} sum of {name}", fails, "sum " + name)
    return fails


def report_worst():
    return "largest |error| / bound seen: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items()))


# ------------------------------------------------------------------------------------------------ the inputs both test files use
def draw(kind, B, C, H, W, seed):
    """-> (recon fp32, target fp32, data_range, clamp) of one named value pattern"""
    g = torch.Generator().manual_seed(seed)
    u = lambda: torch.rand(B, C, H, W, generator=g)
    if kind == "noise":
        return u(), u(), 1.0, False
    if kind == "near":
        t = u()
        return t + 0.02 * torch.randn(B, C, H, W, generator=g), t, 1.0, False
    if kind == "flat":                                       # bright and flat: the raw second moments would cancel worst here
        return 0.9 + 1e-3 * (2 * u() - 1), 0.9 + 1e-3 * (2 * u() - 1), 1.0, False
    if kind == "identical":
        t = u()
        return t.clone(), t, 1.0, False
    if kind in ("outside", "outside_clamped"):
        return 1.6 * u() - 0.3, u(), 1.0, kind == "outside_clamped"
    if kind == "range255":
        return 255.0 * u(), 255.0 * u(), 255.0, False
    raise ValueError(kind)


KINDS = ("noise", "near", "flat", "identical", "outside", "outside_clamped", "range255")


def sizes(T):
    """(H, W) pairs at the edges of a T-pixel tile: a single window, one and two tiles, the last tile with and without windows of its
    own, an odd W (no 16-byte pieces), and widths of whole 4- and 8-element pieces"""
    return [(11, 12), (12, 11), (T + 9, T + 11), (T + 10, 37), (T + 11, T + 10), (2 * T + 11, T + 9), (11, 2 * T + 11), (T + 11, 40), (12, 2 * T)]


# ------------------------------------------------------------------------------------------------ the histogram
def hist_ref(ids, K, bug=None):
    """ids: int64 of any shape -> {"hist": int64 [K], "bad": int, "count": int}"""
    flat = ids.reshape(-1)
    ok = (flat >= 0) & (flat < K)
    hist = torch.bincount(flat[ok], minlength=K)
    bad = int((~ok).sum())
    if bug == "oor_bin0":
        hist[0] += bad
    elif bug == "oor_binK":
        hist[K - 1] += bad
    return {"hist": hist, "bad": bad, "count": int(hist.sum())}


def stats_ref(hist, bug=None):
    """usage / used / dead / entropy / perplexity of a histogram, in float64"""
    h = hist.to(F64)
    K, n = h.numel(), float(h.sum())
    used = int((h > 0).sum())
    p = h[h > 0] / n
    entropy = float(-(p * p.log()).sum()) if n else float("nan")
    usage = min(1.0, n / K) if bug == "usage_from_count" else used / K
    return {"usage": usage, "used": used, "dead": K - used, "entropy": entropy, "perplexity": math.exp(entropy) if n else float("nan"),
            "count": int(n)}


def check_hist(hist, bad, ref, label=""):
    fails = []
    got = hist.detach().cpu()
    if got.dtype != torch.int64 or not torch.equal(got, ref["hist"]):
        n = int((got != ref["hist"]).sum()) if got.shape == ref["hist"].shape else -1
        fails.append(f"{label} hist: {n} bins differ")
    if int(bad) != ref["bad"]:
        fails.append(f"{label} bad: got {int(bad)}, reference {ref['bad']}")
    return fails


def check_stats(got, ref, label=""):
    fails = []
    for k in ("used", "dead", "count"):
        if got[k] != ref[k]:
            fails.append(f"{label} {k}: got {got[k]}, reference {ref[k]}")
    for k in ("usage", "entropy", "perplexity"):
        g, r = got[k], ref[k]
        if not (g != g and r != r) and not abs(g - r) <= 1e-12 * max(1.0, abs(r)):
            fails.append(f"{label} {k}: got {g!r}, reference {r!r}")
    return fails
