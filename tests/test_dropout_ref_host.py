"""CPU-only checks of tests/_dropout_ref.py, the numpy restatement of the dropout contract of csrc/common.h that the GPU tests compare
every mask consumer with: the properties the restatement must have on its own, before a kernel is held to it."""
import math

import numpy as np
import pytest

import _dropout_ref as R

SEED = (0x9e3779b9 << 32) | 0x7f4a7c15          # both words non-zero


def test_mix32_is_a_bijection_fixing_zero_with_known_values():
    assert int(R.mix32(np.uint32(0))) == 0                                    # xor-shift / odd-multiply steps all fix 0
    x = np.arange(1 << 20, dtype=np.uint32)
    assert np.unique(R.mix32(x)).size == x.size                               # invertible steps: no collisions
    # worked by hand from the formula for x = 1: 1 -> 0x7feb352d -> ^>>15 -> * 0x846ca68b -> ^>>16
    v = 1
    v ^= v >> 16; v = (v * 0x7feb352d) & 0xffffffff; v ^= v >> 15; v = (v * 0x846ca68b) & 0xffffffff; v ^= v >> 16
    assert int(R.mix32(np.uint32(1))) == v
    assert R.mix32(np.array([0xffffffff], dtype=np.uint32)).dtype == np.uint32


def test_threshold_and_scale():
    assert R.thresh(0.0) == 0
    assert R.thresh(0.5) == 1 << 31
    assert R.thresh(1e-12) == 1                                               # p > 0 never rounds down to "off"
    assert R.thresh(0.3) == int(math.floor(float(np.float32(0.3)) * 2.0 ** 32))
    assert R.scale(0.5) == np.float32(2.0) and R.scale(0.3).dtype == np.float32
    with pytest.raises(ValueError):
        R.thresh(1.0)


def test_deterministic_and_seed_dependent():
    a, b = R.mask(100000, SEED, 0.3), R.mask(100000, SEED, 0.3)
    assert np.array_equal(a, b)
    assert np.array_equal(a[1000:2000], R.mask(1000, SEED, 0.3, start=1000))  # stateless: the index decides, not the call
    assert (R.mask(100000, SEED + 1, 0.3) != a).mean() > 0.3                  # independent masks differ at 2 p (1 - p) = 0.42 of the places
    assert R.mask(1000, SEED, 0.0).all()


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5, 0.9])
def test_keep_rate_within_four_binomial_standard_deviations(p):
    n = 10 ** 6
    rate = R.mask(n, SEED, p).mean()
    assert abs(rate - (1 - p)) < 4 * math.sqrt(p * (1 - p) / n), (p, rate)


def test_high_seed_word_changes_the_mask():
    lo = SEED & 0xffffffff
    a, b = R.mask(100000, lo, 0.3), R.mask(100000, lo | (1 << 32), 0.3)
    assert (a != b).mean() > 0.3


def test_index_above_2_pow_32_differs_from_the_same_index_mod_2_pow_32():
    n = 100000
    a, b = R.mask(n, SEED, 0.3), R.mask(n, SEED, 0.3, start=1 << 32)
    assert (a != b).mean() > 0.3
    # the high index word enters like the high seed word: (idx_hi, seed_hi) and (seed_hi, idx_hi) give the same mask
    lo = SEED & 0xffffffff
    assert np.array_equal(R.mask(n, lo | (5 << 32), 0.3), R.mask(n, lo, 0.3, start=5 << 32))


def test_grouped_mask_is_one_decision_per_group():
    g = 50 * 128
    m = R.mask(10 * g + 17, SEED, 0.5, group=g)
    per = R.keep(np.arange(11), SEED, 0.5)
    assert np.array_equal(m, np.repeat(per, g)[:m.size])
