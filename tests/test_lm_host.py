"""Host-side checks of the training path of the causal stack (vitamd/lm.py, csrc/loss.hip): the float64 reference of tests/_lm_ref.py
against torch, the bounds of the GPU test against planted mistakes, the C ABI's symbols and refusals.  No GPU is needed."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _abi
import _lm_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ERR_SHAPE, ERR_ARG = 1, 2


def _case(M, V, seed, scale=3.0, dtype=F32):
    """logits randn x scale with a -inf block in row 1, targets that include 0 and V - 1, about a quarter of the rows ignored"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, V, generator=g) * scale
    x[1, V // 4: max(V // 2, V // 4 + 1)] = float("-inf")
    t = torch.randint(0, V, (M,), generator=g)
    t[torch.rand(M, generator=g) < 0.25] = -100
    t[0], t[1], t[2] = 0, V - 1, -100
    return x.to(dtype), t


@pytest.mark.parametrize("V", [2, 10, 1000, 1024])
def test_reference_equals_torch_float64(V):
    x, t = _case(24, V, seed=V)
    ref = R.cross_entropy_ref(x, t, grad_out=2.5)
    x64 = x.to(F64).requires_grad_(True)
    mean = F.cross_entropy(x64, t, ignore_index=-100)
    (mean * 2.5).backward()
    rows = F.cross_entropy(x64.detach(), t, ignore_index=-100, reduction="none")
    assert ref["count"] == int((t != -100).sum()) and 0 < ref["count"] < 24
    assert torch.allclose(ref["mean"], mean.detach(), rtol=1e-13, atol=0)
    assert torch.allclose(ref["loss_row"], rows, rtol=1e-13, atol=1e-13)
    assert torch.allclose(ref["lse"], torch.logsumexp(x64.detach(), -1), rtol=1e-13, atol=0)
    assert torch.allclose(ref["grad"], x64.grad, rtol=1e-12, atol=1e-16)
    assert bool((ref["grad"][t == -100] == 0).all()) and bool((ref["grad"][1, V // 4: max(V // 2, V // 4 + 1)] == 0).all())
    none = R.cross_entropy_ref(x, torch.full_like(t, -100))
    assert bool(torch.isnan(none["mean"])) and bool((none["grad"] == 0).all())


def test_embedding_reference_equals_torch():
    g = torch.Generator().manual_seed(3)
    tok, pos = torch.randn(11, 8, generator=g), torch.randn(9, 8, generator=g)
    ids = torch.randint(0, 11, (3, 7), generator=g)
    tok_p, pos_p = tok.to(F64).requires_grad_(True), pos.to(F64).requires_grad_(True)
    dy = torch.randn(3, 7, 8, generator=g)
    (R.embed_ref(tok_p, pos_p, ids) * dy.to(F64)).sum().backward()
    dtok, dpos = R.embed_grads_ref(dy, ids, 11, 9)
    assert torch.allclose(dtok, tok_p.grad, rtol=1e-13, atol=1e-15) and torch.allclose(dpos, pos_p.grad, rtol=1e-13, atol=1e-15)
    assert bool((dpos[7:] == 0).all())


@pytest.mark.parametrize("V, scale", [(10, 3.0), (1000, 30.0)])
def test_bounds_pass_the_standin_and_catch_planted_mistakes(V, scale):
    """The stand-in is the kernel's arithmetic in torch fp32: it must pass every bound the GPU test applies, and each planted mistake
    must fail at least one (the missing max subtraction needs the large logits to overflow)."""
    x, t = _case(64, V, seed=100 + V, scale=scale)
    ref = R.cross_entropy_ref(x, t, grad_out=2.5)
    t32 = R.cross_entropy_torch32(x, t, grad_out=2.5)
    good = R.standin32(x, t, grad_out=2.5)
    assert R.check_cross_entropy(good, ref, t32, "stand-in") == []
    assert R.check_bf16_grad(good["grad"].to(BF16), ref, t32, "stand-in") == []
    for bug in R.BUGS:
        if bug == "no_max" and scale < 30:
            continue
        bad = R.standin32(x, t, grad_out=2.5, bug=bug)
        fails = R.check_cross_entropy(bad, ref, t32, bug) + R.check_bf16_grad(bad["grad"].to(BF16), ref, t32, bug)
        assert fails, bug


def test_bf16_rounding_bound_separates_rounding_from_truncation():
    """torch's own round-to-nearest of its fp32 gradient stays inside half a bf16 ulp (+1/16); truncating the low 16 bits does not"""
    x, t = _case(64, 1000, seed=7)
    ref = R.cross_entropy_ref(x, t, grad_out=2.5)
    t32 = R.cross_entropy_torch32(x, t, grad_out=2.5)
    rel = ((t32["grad"].to(BF16).to(F64) - ref["grad"]).abs() / ref["grad"].abs().clamp_min(1e-300))[ref["grad"] != 0]
    assert float(rel.max()) <= 2.0 ** -8
    assert R.check_bf16_grad(t32["grad"].to(BF16), ref, t32, "rounded") == []
    trunc = (t32["grad"].view(torch.int32) & -65536).view(F32)
    assert R.check_bf16_grad(trunc, ref, t32, "truncated") != []


# ------------------------------------------------------------------------------------------------ the library
NEW_SYMBOLS = ("vitamd_cross_entropy_grid_rows", "vitamd_cross_entropy_fwd", "vitamd_cross_entropy_bwd", "vitamd_embed_tokens_fwd", "vitamd_embed_tokens_bwd")


def test_symbols_are_exported_and_typed():
    from vitamd import lib
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert name in lib.SIGNATURES
        fn = getattr(L, name)
        assert fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    from vitamd import ops
    assert ops.cross_entropy_grid_rows(72) == ops.cross_entropy_grid_rows(4096) == 4 * ops.cross_entropy_grid_rows(4097) > 0
    assert L.vitamd_cross_entropy_grid_rows(1) == -ERR_SHAPE == L.vitamd_cross_entropy_grid_rows(65537)
    header = _abi.header()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header


def test_entry_points_refuse_before_any_launch():
    """null pointers everywhere: a shape error is reported first, valid numbers then give the argument error; nothing is launched"""
    from vitamd import lib
    L = lib.load()
    fwd = lambda M, V, ld: L.vitamd_cross_entropy_fwd(None, 0, None, None, None, None, M, V, ld, -100, None)
    bwd = lambda M, V, ld, ldo: L.vitamd_cross_entropy_bwd(None, 1, None, None, None, None, None, 1, M, V, ld, ldo, -100, None)
    for M, V, ld in ((4, 1, 1), (4, 65537, 65537), (4, 10, 9), (0, 10, 10)):
        assert fwd(M, V, ld) == ERR_SHAPE, (M, V, ld)
        assert bwd(M, V, ld, max(V, 1)) == ERR_SHAPE, (M, V, ld)
    assert bwd(4, 10, 10, 9) == ERR_SHAPE
    assert fwd(4, 10, 10) == ERR_ARG and fwd(1, 2, 2) == ERR_ARG and fwd(4, 65536, 65536) == ERR_ARG
    assert bwd(4, 10, 10, 16) == ERR_ARG
    efwd = lambda B, S, D, tok_rows, pos_rows: L.vitamd_embed_tokens_fwd(None, None, None, None, B, S, D, tok_rows, pos_rows, None)
    ebwd = lambda B, S, D, tok_rows: L.vitamd_embed_tokens_bwd(None, None, None, None, B, S, D, tok_rows, None)
    assert efwd(2, 8, 6, 10, 8) == ERR_SHAPE and efwd(2, 9, 8, 10, 8) == ERR_SHAPE and efwd(0, 8, 8, 10, 8) == ERR_SHAPE
    assert efwd(2, 8, 8, 10, 8) == ERR_ARG
    assert ebwd(2, 8, 6, 10) == ERR_SHAPE and ebwd(2, 0, 8, 10) == ERR_SHAPE
    assert ebwd(2, 8, 8, 10) == ERR_ARG


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    import train_videogpt as V
    from vitamd import lm, ops
    from vitamd.lib import VitamdError
    refuse = (ValueError, VitamdError)
    x, t = torch.randn(4, 10), torch.randint(0, 10, (4,))
    with pytest.raises(ValueError):
        ops.cross_entropy_fwd(torch.randn(4, 1), t)                       # V out of range: before any device is looked at
    with pytest.raises(ValueError):
        ops.cross_entropy_fwd(torch.randn(1, 65537), t[:1])
    with pytest.raises(ValueError):
        lm.linear_cross_entropy(torch.randn(4, 64), torch.randn(1, 64), None, t)
    for call in (lambda: ops.cross_entropy_fwd(x, t),
                 lambda: ops.cross_entropy_bwd(x, t, torch.zeros(4), torch.zeros(2)),
                 lambda: ops.embed_tokens_fwd(torch.zeros(2, 3, dtype=torch.long), torch.randn(5, 8), torch.randn(3, 8)),
                 lambda: ops.embed_tokens_bwd(torch.randn(6, 8), torch.zeros(2, 3, dtype=torch.long), torch.zeros(5, 8), torch.zeros(3, 8)),
                 lambda: lm.cross_entropy(x, t),
                 lambda: lm.cross_entropy(x, t.int()),
                 lambda: lm.cross_entropy(x, t[:3]),
                 lambda: lm.linear_cross_entropy(torch.randn(4, 64), torch.randn(128, 64), None, t),
                 lambda: lm.linear_cross_entropy(torch.randn(4, 64), torch.randn(128, 32), None, t),
                 lambda: lm.token_embed(torch.zeros(2, 3, dtype=torch.long), torch.randn(5, 8), torch.randn(3, 8)),
                 lambda: lm.token_embed(torch.zeros(6, dtype=torch.long), torch.randn(5, 8), torch.randn(3, 8))):
        with pytest.raises(refuse):
            call()
    assert callable(V.VideoGPT.loss) and callable(V.train_step) and callable(V.main)
    assert lm.fused_head_applies(1024, 768) and not lm.fused_head_applies(250, 384) and not lm.fused_head_applies(1000, 768)
