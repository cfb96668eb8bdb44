"""CPU restatements of Random Erasing (include/vitamd.h vitamd_frames_erase, vitamd/erase.py), shared by test_erase_host.py and
test_gpu_erase.py.  numpy float64 and the Philox of _sampling_ref.py only.

  noise_ref      the N(0, 1) value of (seed, step, b, c, y, x) in float64, with r = sqrt(-2 ln u1) beside it for the bound
  winners        the single-writer rule over a record: which box, if any, owns each pixel
  erase_ref      both together: what the kernel must leave in a batch
  check_erased   the comparison test_gpu_erase.py makes, as a list of failures (and the largest ratio to the noise bound)
  draw_ref       Erase.draw, restated
`bug=` plants one mistake in erase_ref (test_erase_host.py shows that check_erased then fails)."""
import math

import numpy as np
import torch

import _sampling_ref as S

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
Z_MAX = math.sqrt(48 * math.log(2))              # u1 >= 2^-24: r <= sqrt(2 * 24 ln 2)
BUGS = ("earliest_wins", "lane_swapped", "no_b")
# the record of the fast-form case (B = 5, H = W = 32, K = 2), shared by the two test files
FAST_RECORD = [[[2, 3, 20, 1, 7], [1, 10, 30, 4, 28]],                                    # fill over noise
               [[1, 2, 28, 2, 30], [2, 20, 32, 17, 32]],                                  # noise over fill, touching the right and bottom borders
               [[2, 0, 32, 9, 14], [2, 5, 5, 0, 32]],                                     # full height; an empty box
               [[7, 0, 32, 0, 32], [2, I32_MIN, 9, 25, I32_MAX]],                     # a mode 7; coordinates far out of range
               [[0, 0, 32, 0, 32], [0, 1, 2, 3, 4]]]                                      # nothing


def noise_ref(seed, step, b, C, H, W, bug=None):
    """-> (z float64 [C, H, W], r float64 [C, H, W]): pixel x of row y takes z[x & 3] of the Philox call with counter
    ((c*H + y) * ceil(W/4) + (x >> 2), (b << 2) | 2, step low, step high) under key (seed low, seed high)"""
    w4 = (W + 3) // 4
    c, y, g = np.meshgrid(np.arange(C, dtype=np.uint64), np.arange(H, dtype=np.uint64), np.arange(w4, dtype=np.uint64), indexing="ij")
    c0 = (c * np.uint64(H) + y) * np.uint64(w4) + g
    c1 = ((0 if bug == "no_b" else b) << 2) | 2
    w = S.philox4x32_10((c0.reshape(-1), c1, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    z, r = np.empty((4, c0.size)), np.empty((4, c0.size))
    for i in range(2):
        u1 = ((w[2 * i] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[2 * i + 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        rr = np.sqrt(-2.0 * np.log(u1))
        z[2 * i], z[2 * i + 1] = rr * np.cos(2.0 * np.pi * u2), rr * np.sin(2.0 * np.pi * u2)
        r[2 * i] = r[2 * i + 1] = rr
    if bug == "lane_swapped":
        z = z[[1, 0, 3, 2]]
    # [4, C*H*w4] -> [C, H, w4*4] -> the first W columns
    z = z.T.reshape(C, H, w4 * 4)[:, :, :W]
    r = r.T.reshape(C, H, w4 * 4)[:, :, :W]
    return z, r


def clamp_rec(rec, H, W):
    """the header's clamps: -> per sample a list of (mode, yl, yh, xl, xh); an empty box and a mode outside {1, 2} are mode 0"""
    out = []
    for rows in rec.tolist():
        boxes = []
        for mode, yl, yh, xl, xh in rows:
            yl, yh, xl, xh = min(max(yl, 0), H), min(max(yh, 0), H), min(max(xl, 0), W), min(max(xh, 0), W)
            if mode not in (1, 2) or yl >= yh or xl >= xh:
                mode = 0
            boxes.append((mode, yl, yh, xl, xh))
        out.append(boxes)
    return out


def winners(rec, H, W, bug=None):
    """int64 [B, H, W]: the k of the box that writes each pixel - the LARGEST k whose (clamped, non-empty, mode 1 or 2) box covers it -
    or -1 where no box does"""
    boxes = clamp_rec(rec, H, W)
    win = np.full((len(boxes), H, W), -1, dtype=np.int64)
    for b, rows in enumerate(boxes):
        order = list(enumerate(rows))
        for k, (mode, yl, yh, xl, xh) in (reversed(order) if bug == "earliest_wins" else order):     # painted in order: the last one stays
            if mode:
                win[b, yl:yh, xl:xh] = k
    return win


def erase_ref(before, rec, fill, seed, step, bug=None):
    """before: fp32 torch [B, C, H, W].  -> dict: want float64 [B, C, H, W] (before outside the boxes, fill in mode-1 pixels, noise_ref in
    mode-2 pixels), r float64 (of the noise, 1 elsewhere), kind int [B, C, H, W] (0 untouched, 1 fill, 2 noise)"""
    B, C, H, W = before.shape
    win = winners(rec, H, W, bug)
    boxes = clamp_rec(rec, H, W)
    want = before.numpy().astype(np.float64).copy()
    r = np.ones_like(want)
    kind = np.zeros(want.shape, dtype=np.int64)
    for b in range(B):
        z = None
        for k, (mode, *_) in enumerate(boxes[b]):
            m = win[b] == k
            if not m.any():
                continue
            if mode == 1:
                for c in range(C):
                    want[b, c][m] = 0.0 if fill is None else float(fill[b, k, c])
                kind[b][:, m] = 1
            else:
                if z is None:
                    z, rr = noise_ref(seed, step, b, C, H, W, bug)
                want[b][:, m], r[b][:, m] = z[:, m], rr[:, m]
                kind[b][:, m] = 2
    return {"want": want, "r": r, "kind": kind}


def bits(t):
    return t.contiguous().view(torch.int32)


def check_erased(got, before, ref):
    """got, before: fp32 torch [B, C, H, W] on the CPU; ref: erase_ref's dict.  -> (failures, the largest |got - want| / bound over the
    noise pixels).  Outside every box the bits are before's; a fill pixel holds fp32(fill) exactly; a noise pixel lies within
    6 * 2^-23 * max(r, 1) of the float64 value and within sqrt(48 ln 2) of zero."""
    fails = []
    kind, want = ref["kind"], ref["want"]
    g = got.numpy()
    same = (bits(got) == bits(before)).numpy()
    if not same[kind == 0].all():
        fails.append(f"outside: {int((~same[kind == 0]).sum())} untouched elements changed")
    if not np.array_equal(g[kind == 1], want[kind == 1].astype(np.float32)):
        fails.append(f"fill: {int((g[kind == 1] != want[kind == 1].astype(np.float32)).sum())} elements are not their fill value")
    noise = kind == 2
    ratio = 0.0
    if noise.any():
        err = np.abs(g[noise].astype(np.float64) - want[noise])
        bound = 6 * 2.0 ** -23 * np.maximum(ref["r"][noise], 1.0)
        ratio = float((err / bound).max())
        if not (err <= bound).all():
            fails.append(f"noise: {int((err > bound).sum())} of {err.size} elements beyond the bound, worst ratio {ratio:.3g}")
        if not (np.abs(g[noise]) <= Z_MAX).all():
            fails.append("noise: a value beyond sqrt(48 ln 2)")
    return fails, ratio


def moments_ok(z):
    """the caps of the issue on n standard normal values: |mean| < 5 / sqrt(n), |var - 1| < 5 sqrt(2 / n), no value beyond sqrt(48 ln 2)"""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    n = z.size
    return abs(z.mean()) < 5 / math.sqrt(n) and abs(z.var() - 1) < 5 * math.sqrt(2 / n) and float(np.abs(z).max()) <= Z_MAX


# ---------------------------------------------------------------------------------------------- the draw
def draw_ref(B, hw, step, seed=0, probability=0.25, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode="pixel", min_count=1,
             max_count=None):
    """Erase.draw restated: -> (rec list [B][K][5], fill list [B][K][4]) in Python numbers"""
    H, W = hw
    max_aspect = 1 / min_aspect if max_aspect is None else max_aspect
    K = max_count = min_count if max_count is None else max_count
    rng = np.random.Generator(np.random.Philox(key=np.array([seed, step], dtype=np.uint64), counter=np.array([0, 0, 0, 2], dtype=np.uint64)))
    rec, fill = [], []
    for _ in range(B):
        rows, fills = [[0, 0, 0, 0, 0] for _ in range(K)], [[0.0] * 4 for _ in range(K)]
        rec.append(rows)
        fill.append(fills)
        if not rng.random() < probability:
            continue
        count = min_count if min_count == max_count else int(rng.integers(min_count, max_count + 1))
        for k in range(count):
            for _ in range(10):
                target = float(rng.uniform(min_area, max_area)) * H * W / count
                aspect = math.exp(float(rng.uniform(math.log(min_aspect), math.log(max_aspect))))
                h, w = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
                if h < H and w < W:
                    top, left = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
                    if mode == "rand":
                        fills[k] = [float(v) for v in rng.standard_normal(4)]
                    if h > 0 and w > 0:
                        rows[k] = [2 if mode == "pixel" else 1, top, top + h, left, left + w]
                    break
    return rec, fill


def expected_box(hw, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, n=200000, seed=123):
    """(chance that one attempt fits, mean and standard deviation of the area h * w of a fitting attempt) under the restated rule, by a
    Monte-Carlo pass of n attempts with numpy's default generator (independent of the Philox stream under test): the expectation the
    statistics of a draw are held to, with its own standard error"""
    H, W = hw
    max_aspect = 1 / min_aspect if max_aspect is None else max_aspect
    rng = np.random.default_rng(seed)
    target = rng.uniform(min_area, max_area, n) * H * W
    aspect = np.exp(rng.uniform(math.log(min_aspect), math.log(max_aspect), n))
    h, w = np.rint(np.sqrt(target * aspect)), np.rint(np.sqrt(target / aspect))
    fits = (h < H) & (w < W)
    area = (h * w)[fits]
    return float(fits.mean()), float(area.mean()), float(area.std()), int(fits.sum())
