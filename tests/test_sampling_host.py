"""CPU-only checks of sampled generation: the float64 restatement of the semantics against the common sort-based formulation, the numpy
Philox against the published known answers, and the refusals of the C entry point, the op and VideoGPT.generate before any device work."""
import ctypes

import numpy as np
import pytest
import torch

import _sampling_ref as R
from vitamd import lib, ops

PARAMS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.0, 0, 0.9), (1.3, 100, 0.95), (0.5, 0, 0.5), (1.0, 0, 1e-6)]


def test_threshold_form_equals_the_sort_based_formulation():
    n = 0
    for V, rows in ((64, 24), (257, 24), (1000, 16), (4096, 16), (16384, 8), (65536, 4)):
        for spread in (1, 3, 8):
            x = R.logits(11, f"rows{V}", (rows, V), spread)
            x[1, V // 4:V // 2] = -np.inf                        # a masked block
            for r in range(rows):
                for T, k, p in PARAMS:
                    S, q, K = R.kept_set(x[r], T, k, p)
                    assert S.any() and not (S & ~K).any()
                    assert (S == R.kept_set_sorted(x[r], T, k, p)).all(), (V, spread, r, T, k, p)
                    n += 1
    assert n == 3 * 6 * 92


def test_draw_walks_the_kept_set_in_index_order():
    x = np.array([0.0, 1.0, -np.inf, 1.0, 0.5], dtype=np.float32)
    assert R.draw(x, 1.0, 0, 1.0, 0.0) == 0
    assert R.draw(x, 1.0, 0, 1.0, 1 - 2.0 ** -24) == 4
    assert R.draw(x, 1.0, 1, 1.0, 0.0) == 1 and R.draw(x, 1.0, 1, 1.0, 0.75) == 3      # the tie with the maximum is kept whole
    assert R.draw(x, 1.0, 0, 1e-6, 0.25) == 1
    S, _, _ = R.kept_set(x, 0.5, 3, 1.0)
    assert S.tolist() == [False, True, False, True, True]


def test_numpy_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v[0]) for v in R.philox4x32_10(ctr, key)) == want
    u = R.philox_u(0, 4, 0)
    assert u.dtype == np.float32 and u[0] == np.float32((0x6627e8d5 >> 8) * 2.0 ** -24) and len(set(u.tolist())) == 4
    assert ((0 <= u) & (u < 1)).all()


def test_sample_logits_is_bound_and_the_abi_version_stays():
    assert "vitamd_sample_logits" in lib.SIGNATURES and len(lib.SIGNATURES["vitamd_sample_logits"]) == 13
    L = lib.load()
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "vitamd_sample_logits")
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION


def test_c_entry_point_refuses_before_any_launch():
    """null pointers, no device: the shape and argument rules come first"""
    L = lib.load()

    def call(B=4, V=1024, ld=1024, T=1.0, k=0, p=1.0):
        return L.vitamd_sample_logits(None, None, None, None, None, B, V, ld, T, k, p, 0, None)
    assert call(V=1, ld=1) == 1                       # VITAMD_ERR_SHAPE
    assert call(V=65537, ld=65537) == 1
    assert call(V=1024, ld=1023) == 1
    assert call(B=0) == 1
    assert call(T=0.0) == 2                           # VITAMD_ERR_ARG
    assert call(T=-1.0) == 2 and call(k=-1) == 2 and call(p=0.0) == 2 and call(p=1.5) == 2
    assert call() == 2                                # valid numbers, missing pointers


def _bad_parameters():
    return [dict(temperature=0.0), dict(temperature=-0.5), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.0001), dict(top_p=-0.1)]


def test_op_refuses_parameters_before_the_device():
    x = torch.zeros(4, 1024)
    for bad in _bad_parameters():
        with pytest.raises(ValueError):
            ops.sample_logits(x, **bad)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(4, 1))                       # V out of range
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 65537))
    with pytest.raises(lib.VitamdError):
        ops.sample_logits(x)                                       # valid parameters, CPU tensor
    with pytest.raises(lib.VitamdError):
        ops.sample_logits(x, 0.7, 50, 0.9, u=torch.zeros(4))
    from vitamd.sampling import Sampler
    for bad in _bad_parameters():
        with pytest.raises(ValueError):
            Sampler(**bad)
    s = Sampler(0.8, 40, 0.95, seed=3)
    with pytest.raises(lib.VitamdError):
        s(x)
    assert s.step == 0                                             # a refused call does not move the stream


def test_generate_refuses_parameters_before_the_device():
    import train_videogpt as V
    model = V.VideoGPT(V.VideoGPTConfig(16, 256, "S", 4, 0.0))
    tokens = torch.zeros(2, 8, dtype=torch.long)
    for bad in _bad_parameters():
        with pytest.raises(ValueError):
            model.generate(tokens, n=2, **bad)
        with pytest.raises(ValueError):
            model.generate_frames(tokens.view(2, 1, 8), n=1, use_cache=False, **bad)
    with pytest.raises(ValueError):
        model.generate(tokens, n=57, temperature=1.0)                               # 8 + 57 > max_tokens = 64: the length refusal
    drop = V.VideoGPT(V.VideoGPTConfig(16, 256, "S", 4, 0.1))
    with pytest.raises(ValueError):
        drop.generate(tokens, n=2, use_cache=True, temperature=1.0)                 # dropout > 0: the cache refusal
    with pytest.raises(ValueError, match="max_tokens"):
        drop.generate(tokens, n=57, temperature=0.0)                                # the existing checks come first
    with pytest.raises(ValueError, match="dropout"):
        drop.generate(tokens, n=2, use_cache=True, temperature=0.0)
    tiny = V.VideoGPT(V.VideoGPTConfig(16, 1, "S", 4, 0.0))                         # a one-entry codebook cannot be sampled
    with pytest.raises(ValueError):
        tiny.generate(tokens, n=2, top_k=1)
