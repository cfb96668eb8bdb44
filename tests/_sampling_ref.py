"""float64 restatement of the sampling semantics (include/vitamd.h, vitamd_sample_logits), a numpy Philox4x32-10, and the validity check
that every GPU sampling test uses.  Shared by test_sampling_host.py and test_gpu_sampling.py; numpy only."""
import zlib

import numpy as np

EPS = 2e-5          # derived, not measured: fp32 sums of up to 65 536 non-negative terms as 256 runs of 256 plus a tree are off by at most about
                    # (256 + 8) * 2^-24 = 1.6e-5 relatively, the hardware exp2 adds an ulp per term and z * log2(e) at |z| <= 40 less than 5e-6
M32 = np.uint64(0xFFFFFFFF)


def f32(v):
    """the value the kernel receives for a float parameter"""
    return float(np.float32(v))


def logits(seed, name, shape, spread):
    """deterministic normals (oracle/weights.py's recipe) times spread, fp32"""
    rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))
    return (rng.standard_normal(size=shape) * spread).astype(np.float32)


# ---------------------------------------------------------------------------------------------- Philox4x32-10
def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints), key: two -> the four output words (uint32 arrays)"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32 for v in counter]
    k0, k1 = (np.uint64(int(v) & 0xFFFFFFFF) for v in key)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return [v.astype(np.uint32) for v in c]


def philox_u(seed, rows, step):
    """u of (seed, row, step) for rows 0 .. rows-1: key = seed (low, high), counter = (row, 0, step low, step high)"""
    r = np.arange(rows, dtype=np.uint64)
    out = philox4x32_10((r, 0, step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return ((out[0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the semantics, one row, float64
def topk_set(z, finite, top_k):
    """K of step 2 (ties with the k-th value kept); -inf is never kept"""
    V = z.shape[-1]
    if 0 < top_k < V:
        kth = np.partition(z, V - top_k, axis=-1)[..., V - top_k]
        return (z >= kth[..., None]) & finite
    return finite.copy()


def softmax_over(z, mask):
    zz = np.where(mask, z, -np.inf)
    w = np.exp(zz - zz.max(axis=-1, keepdims=True))
    return w / w.sum(axis=-1, keepdims=True)


def kept_set(x, temperature, top_k, top_p):
    """x fp32 [V] -> (S, q over K, K): the threshold form of steps 1-3"""
    z = x.astype(np.float64) / temperature
    finite = np.isfinite(x)
    K = topk_set(z, finite, top_k)
    q = softmax_over(z, K)
    if top_p >= 1:
        return K.copy(), q, K
    idx = np.flatnonzero(K)
    order = idx[np.argsort(-z[idx], kind="stable")]
    zs, cum = z[order], np.cumsum(q[order])
    last_of_value = np.append(zs[1:] != zs[:-1], True)          # mass(z >= v) is the running sum at the LAST copy of v
    reach = np.flatnonzero(last_of_value & (cum >= top_p))
    t = zs[reach[0]] if reach.size else zs[-1]
    return K & (z >= t), q, K


def kept_set_sorted(x, temperature, top_k, top_p):
    """the common sort-based formulation: scores below the k-th largest dropped; then, sorted ascending, the tokens whose cumulative
    probability is <= 1 - top_p dropped, at least one kept"""
    z = x.astype(np.float64) / temperature
    V = z.shape[0]
    keep = np.isfinite(x)
    if 0 < top_k < V:
        keep &= z >= np.sort(z)[V - top_k]
    if top_p < 1:
        q = softmax_over(z, keep)
        order = np.argsort(z, kind="stable")
        order = order[keep[order]]
        drop = np.cumsum(q[order]) <= 1 - top_p
        drop[-1] = False
        keep = keep.copy()
        keep[order[drop]] = False
    return keep


def draw(x, temperature, top_k, top_p, u):
    """step 4 on the float64 sets: the token of one row"""
    S, q, _ = kept_set(x, temperature, top_k, top_p)
    idx = np.flatnonzero(S)
    run = np.cumsum(q[idx])
    hit = np.flatnonzero(run > u * run[-1])
    return int(idx[hit[0]] if hit.size else idx[-1])


# ---------------------------------------------------------------------------------------------- the validity check (a-d), a batch of rows
def check_rows(x, temperature, top_k, top_p, u, token, info, eps=EPS):
    """x fp32 [B, V], u fp32 [B], token int64 [B], info fp32 [B, 4] as the kernel returned them; temperature / top_p as the kernel
    received them (f32()).  Asserts a-d on every row and returns the worst excess over the exact boundaries."""
    B, V = x.shape
    rows = np.arange(B)
    z = x.astype(np.float64) / temperature
    finite = np.isfinite(x)
    tmin = info[:, 0].astype(np.float32)
    S = x >= tmin[:, None]
    strict = x > tmin[:, None]
    # a
    assert np.isfinite(tmin).all()
    assert ((token >= 0) & (token < V)).all()
    assert S[rows, token].all(), "a: token outside the kept set"
    assert (S.sum(1) == info[:, 1]).all(), "a: |S| differs from the kernel's count"
    # b
    K = topk_set(z, finite, top_k)
    if 0 < top_k < V:
        assert (strict.sum(1) <= top_k - 1).all(), "b: more than top_k - 1 logits above the smallest kept one"
    assert not (S & ~K).any(), "b: a kept logit outside the top-k set"
    if top_p >= 1:
        assert (S == K).all(), "b: top_p = 1 must keep exactly the top-k set"
    # c
    q = softmax_over(z, K)
    qS, qstrict = (q * S).sum(1), (q * strict).sum(1)
    assert (qS >= top_p - eps).all(), f"c: kept mass {qS.min()} below top_p"
    if top_p < 1:
        assert (qstrict < top_p + eps).all(), "c: the set without its smallest value already reaches top_p"
    # d
    qs = q * S
    c = np.cumsum(qs, axis=1) / qS[:, None]
    c_hi = c[rows, token]
    c_lo = c_hi - qs[rows, token] / qS
    ud = u.astype(np.float64)
    assert (c_lo - eps <= ud).all() and (ud < c_hi + eps).all(), "d: u outside the token's interval of the cumulative distribution"
    # the two figures of info that a-d do not use: the kept share of the whole softmax, the token's probability
    share = (softmax_over(z, finite) * S).sum(1)
    assert np.abs(info[:, 2] - share).max() <= 2 * eps and np.abs(info[:, 3] - qs[rows, token] / qS).max() <= 2 * eps
    excess = np.maximum(np.maximum(top_p - qS, (qstrict - top_p) if top_p < 1 else -1.0), np.maximum(c_lo - ud, ud - c_hi))
    return float(excess.max())
