"""numpy restatement of the counter-based dropout contract documented in csrc/common.h, written from that comment and independent of the
kernel text: element `idx` (a 64-bit index) of a tensor is kept with probability 1 - p, decided by a stateless hash of (idx, seed);

    mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16          (all mod 2^32)
    keep(idx, seed) = mix32(mix32(lo32(idx) ^ lo32(seed)) ^ hi32(idx) ^ hi32(seed)) >= thresh
    thresh = max(1, floor(p * 2^32)) for p > 0;  kept elements are scaled by fp32(1 / (1 - p))

Index conventions of the consumers (what `idx` is): the flat element index for the elementwise kernels, index // group for grouped
(DropPath) masks, row * N + col for a [M, N] Linear output and for the LayerNorm backward that emits that output's gradient."""
import numpy as np

M32 = np.uint64(0xffffffff)


def mix32(x):
    """the 32-bit finaliser, on a uint32 array (arithmetic in uint64, masked: no reliance on numpy's overflow behaviour)"""
    x = np.asarray(x).astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def thresh(p):
    """p in [0, 1) -> the uint32 threshold; 0 means "dropout off" """
    p = float(np.float32(p))                    # the C ABI takes p as a float
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout: p must be in [0, 1), got {p}")
    if p == 0.0:
        return 0
    return max(1, int(np.floor(p * 4294967296.0)))


def scale(p):
    """1 / (1 - p) as the fp32 number the kernels multiply by"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep(idx, seed, p):
    """bool array: element idx (any integer array, values in [0, 2^64)) survives dropout (p, seed)"""
    idx = np.asarray(idx).astype(np.uint64)
    seed = int(seed) & 0xffffffffffffffff
    slo, shi = np.uint64(seed & 0xffffffff), np.uint64(seed >> 32)
    h = mix32((idx & M32) ^ slo).astype(np.uint64)
    h = mix32(h ^ (idx >> np.uint64(32)) ^ shi)
    return h >= np.uint32(thresh(p)) if thresh(p) else np.ones(idx.shape, dtype=bool)


def mask(n, seed, p, group=1, start=0):
    """keep() of the flat indices start .. start + n - 1, one decision per `group` consecutive elements"""
    idx = np.arange(start, start + n, dtype=np.uint64)
    return keep(idx // np.uint64(group) if group != 1 else idx, seed, p)
