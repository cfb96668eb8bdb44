"""Host-side checks of the tokenizer training path (vitamd/tokenizer.py, csrc/tokenizer.hip): the float64 reference of
tests/_tokenizer_ref.py against torch autograd in float64, the bounds of the GPU test against planted mistakes, the C ABI's symbols and
refusals, the new model surface.  No GPU is needed."""
import ctypes
import inspect

import pytest
import torch

import _abi
import _tokenizer_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ERR_SHAPE, ERR_ARG = 1, 2


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("i", range(len(R.VQ_SHAPES)))
def test_quantiser_reference_equals_torch_float64(i):
    M, K, d = R.VQ_SHAPES[i]
    x, cb, g_q = R.vq_inputs(M, K, d, R.vq_seed(i))
    ref = R.vq_ref(x, cb, g_q, R.G_LOSS)
    # the search: torch.cdist on the unit vectors, as the reference model searches
    u64 = torch.nn.functional.normalize(x.to(F64), dim=-1)
    e64 = torch.nn.functional.normalize(cb.to(F64), dim=-1)
    far = ref["gap"] >= R.GAP
    assert torch.equal(torch.cdist(u64, e64).argmin(dim=-1)[far], ref["idx_ref"][far])
    assert int((~far).sum()) == 0, "the listed shapes hold no near-tie with these seeds"
    t64 = R.vq_torch(x, cb, ref["idx"], g_q, R.G_LOSS, dtype=F64)
    for k in ("unit", "q", "loss", "dx", "dcb"):
        assert torch.allclose(ref[k], t64[k], rtol=1e-12, atol=1e-13), k          # (d = 1: dx is an exact 0 here, 1e-14 from torch)
    # torch's fp32 CPU evaluation of the search agrees on every row
    u32 = torch.nn.functional.normalize(x, dim=-1)
    e32 = torch.nn.functional.normalize(cb, dim=-1)
    d32 = (u32[:, None, :] - e32[None]).pow(2).sum(-1)
    assert torch.equal(d32.argmin(dim=-1), ref["idx_ref"])


def test_quantiser_reference_on_zero_rows_and_duplicates():
    x, cb, g_q = R.vq_inputs(40, 9, 5, 7)
    x[3] = 0
    cb[4] = 0
    cb[7] = cb[2]
    x[5] = cb[2] * 1000                                  # the direction of codes 2 and 7: the first wins
    ref = R.vq_ref(x, cb, g_q, R.G_LOSS)
    assert int(ref["idx_ref"][5]) == 2 and float(ref["gap"][5]) == 0.0
    t64 = R.vq_torch(x, cb, ref["idx"], g_q, R.G_LOSS, dtype=F64)
    for k in ("unit", "q", "loss", "dx", "dcb"):
        assert torch.isfinite(ref[k]).all() and torch.allclose(ref[k], t64[k], rtol=1e-12, atol=1e-13), k
    p = cb[ref["idx"][3]].to(F64)
    assert torch.allclose(ref["dx"][3], (g_q[3].to(F64) - 0.5 * R.G_LOSS * p / 200) / R.EPS, rtol=1e-12)      # du / eps, u = 0


@pytest.mark.parametrize("i", range(len(R.RECON_SHAPES)))
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_reconstruction_reference_equals_torch_float64(i, dtype):
    B, G, p, c = R.RECON_SHAPES[i]
    y, img = R.recon_inputs(B, G, p, c, 300 + i, dtype)
    ref = R.recon_ref(y, img, G, p, R.G_UP)
    t64 = R.recon_torch(y, img, G, p, R.G_UP, dtype=F64)
    assert torch.allclose(ref["loss"], t64["loss"], rtol=1e-13, atol=0)
    assert torch.allclose(ref["dy"], t64["dy"], rtol=1e-13, atol=1e-20)


# ------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize("i", [2, 3, 4])
def test_quantiser_bounds_pass_the_standin_and_catch_planted_mistakes(i):
    M, K, d = R.VQ_SHAPES[i]
    x, cb, g_q = R.vq_inputs(M, K, d, R.vq_seed(i))
    ref = R.vq_ref(x, cb, g_q, R.G_LOSS)
    t32 = R.vq_torch(x, cb, ref["idx"], g_q, R.G_LOSS)
    assert R.check_vq(R.vq_standin32(x, cb, ref["idx"], g_q, R.G_LOSS), ref, t32, "stand-in") == []
    for bug in R.VQ_BUGS:
        assert R.check_vq(R.vq_standin32(x, cb, ref["idx"], g_q, R.G_LOSS, bug=bug), ref, t32, bug), bug
    # ids: one row moved to another code is caught, near-ties are not held
    moved = ref["idx_ref"].clone()
    moved[0] = (moved[0] + 1) % K
    assert R.check_ids(ref["idx_ref"], ref)[0] == [] and R.check_ids(moved, ref)[0]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_reconstruction_bounds_pass_the_standin_and_catch_planted_mistakes(i):
    B, G, p, c = R.RECON_SHAPES[i]
    y, img = R.recon_inputs(B, G, p, c, 300 + i)
    ref = R.recon_ref(y, img, G, p, R.G_UP)
    t32 = R.recon_torch(y, img, G, p, R.G_UP)
    good = R.recon_standin32(y, img, G, p, R.G_UP)
    assert R.check_recon(good, ref, t32, "stand-in") == []
    yb = y.to(BF16)
    refb, t32b = R.recon_ref(yb, img, G, p, R.G_UP), R.recon_torch(yb, img, G, p, R.G_UP)
    goodb = R.recon_standin32(yb, img, G, p, R.G_UP)
    assert R.check_recon_bf16(goodb["dy"].to(BF16), refb, t32b, "stand-in") == []
    trunc = (goodb["dy"].view(torch.int32) & -65536).view(F32)
    assert R.check_recon_bf16(trunc, refb, t32b, "truncated") != []
    for bug in R.RECON_BUGS:
        bad = R.recon_standin32(y, img, G, p, R.G_UP, bug=bug)
        assert R.check_recon(bad, ref, t32, bug), bug


# ------------------------------------------------------------------------------------------------ the library
NEW_SYMBOLS = {"vitamd_vq_quantize_fwd": 12, "vitamd_vq_quantize_bwd": 12, "vitamd_recon_mse_fwd": 11, "vitamd_recon_mse_bwd": 12}


def test_symbols_are_exported_and_typed():
    from vitamd import lib
    L = lib.load()
    header = _abi.header()
    for name, nargs in NEW_SYMBOLS.items():
        fn = getattr(L, name)
        assert len(lib.SIGNATURES[name]) == nargs and fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
        assert f"int {name}(" in header
    for name in ("vitamd_vq_quantize_ws_bytes", "vitamd_recon_mse_ws_bytes"):
        assert getattr(L, name).restype is ctypes.c_long and f"long {name}(" in header
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    assert L.vitamd_vq_quantize_ws_bytes(600, 513, 12) == (513 * 12 + 3) * 4
    assert L.vitamd_recon_mse_ws_bytes(256, 16, 16, 3, 1) == 256 * 16 * 4            # one strip per grid row: 16 tokens x 1536 B = 24 KiB
    assert L.vitamd_recon_mse_ws_bytes(1, 16, 32, 3, 0) == 16 * 4 * 4                # 12 KiB tokens: a grid row is cut into strips of 4


def test_entry_points_refuse_before_any_launch():
    """null pointers everywhere: a shape error is reported first, valid numbers then give the argument error; nothing is launched"""
    from vitamd import lib
    L = lib.load()
    qf = lambda M, K, d: L.vitamd_vq_quantize_fwd(None, None, None, None, None, None, None, None, M, K, d, None)
    qb = lambda M, K, d: L.vitamd_vq_quantize_bwd(None, None, None, None, None, None, None, None, M, K, d, None)
    for M, K, d in ((4, 8, 65), (4, 0, 12), (0, 8, 12), (4, 8, 0)):
        assert qf(M, K, d) == ERR_SHAPE and qb(M, K, d) == ERR_SHAPE, (M, K, d)
        assert L.vitamd_vq_quantize_ws_bytes(M, K, d) == -ERR_SHAPE
    assert qf(4, 8, 64) == ERR_ARG and qb(4, 8, 64) == ERR_ARG and qf(1, 1, 1) == ERR_ARG
    rf = lambda bf16, B, G, p, c, ld: L.vitamd_recon_mse_fwd(None, bf16, None, None, None, B, G, p, c, ld, None)
    rb = lambda bf16, B, G, p, c, ld, ldo: L.vitamd_recon_mse_bwd(None, bf16, None, None, None, B, G, p, c, ld, ldo, None)
    # F = 10 (p = 1, c = 10): no whole 16-byte pieces in either type; F = 12: fp32 only; a stride that breaks the alignment of later rows
    assert rf(1, 2, 2, 1, 10, 16) == ERR_SHAPE and rf(0, 2, 2, 1, 10, 12) == ERR_SHAPE and rb(1, 2, 2, 1, 10, 16, 16) == ERR_SHAPE
    assert rf(1, 2, 2, 2, 3, 16) == ERR_SHAPE and rf(0, 2, 2, 2, 3, 12) == ERR_ARG
    assert rf(1, 2, 2, 4, 3, 52) == ERR_SHAPE and rf(1, 2, 2, 4, 3, 40) == ERR_SHAPE and rf(1, 2, 2, 4, 3, 56) == ERR_ARG
    assert rb(1, 2, 2, 4, 3, 48, 44) == ERR_SHAPE and rb(1, 2, 2, 4, 3, 48, 48) == ERR_ARG
    assert rf(0, 1, 1, 64, 4, 16384) == ERR_SHAPE                                     # one token beyond the LDS budget
    assert rf(1, 0, 2, 4, 3, 48) == ERR_SHAPE and L.vitamd_recon_mse_ws_bytes(2, 2, 1, 10, 1) == -ERR_SHAPE
    # an unaligned token base is refused as a shape (the caller takes another route), with every pointer present
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    assert L.vitamd_recon_mse_fwd(base + 2, 1, base, base, base, 2, 2, 4, 3, 48, None) == ERR_SHAPE
    assert L.vitamd_recon_mse_bwd(base, 1, base, None, base + 2, 2, 2, 4, 3, 48, 48, None) == ERR_SHAPE


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    from vitamd import ops, tokenizer
    from vitamd.lib import VitamdError
    refuse = (ValueError, VitamdError)
    x, cb = torch.randn(6, 12), torch.randn(9, 12)
    img, tok = torch.rand(2, 3, 8, 8), torch.randn(8, 48)
    with pytest.raises(ValueError):
        ops.vq_quantize_fwd(torch.randn(6, 65), torch.randn(9, 65))                  # d out of range: before any device is looked at
    with pytest.raises(ValueError):
        ops.recon_mse_fwd(tok, torch.rand(2, 3, 16, 16), 2, 4)
    for call in (lambda: ops.vq_quantize_fwd(x, cb),
                 lambda: ops.vq_quantize_bwd(None, None, x, torch.zeros(6), torch.zeros(6, dtype=torch.long), cb),
                 lambda: ops.recon_mse_fwd(tok, img, 2, 4),
                 lambda: ops.recon_mse_bwd(tok, img, 2, 4),
                 lambda: tokenizer.vq_quantize(x, cb),
                 lambda: tokenizer.vq_quantize(x, cb[:, :5]),
                 lambda: tokenizer.vq_quantize(x.double(), cb.double()),
                 lambda: tokenizer.recon_mse(tok, img, 2, 4),
                 lambda: tokenizer.recon_mse(tok, img, 4, 2),
                 lambda: tokenizer.linear_recon_mse(torch.randn(8, 64), torch.randn(48, 64), None, img, 2, 4),
                 lambda: tokenizer.linear_recon_mse(torch.randn(8, 64), torch.randn(64, 64), None, img, 2, 4)):
        with pytest.raises(refuse):
            call()
    assert tokenizer.fused_head_applies(768, 384) and not tokenizer.fused_head_applies(48, 64) and not tokenizer.fused_head_applies(768, 100)
    assert not ops.recon_mse_applies(torch.zeros(4, 10, dtype=BF16)) and ops.recon_mse_applies(torch.zeros(4, 48, dtype=BF16))
    assert torch.equal(tokenizer.pixel_shuffle_tokens(tok.view(2, 4, 48), 2, 4), R.pixel_shuffle(tok, 2, 2, 4, 3))


def test_models_gain_loss_and_train_step_and_keep_forward():
    import train_titok as TT
    import train_vit_vqgan as TQ
    for mod, cls in ((TT, TT.TiTok), (TQ, TQ.ViTVQGAN)):
        assert callable(cls.loss) and callable(mod.train_step) and callable(mod.main) and callable(mod.parse_args)
        assert list(inspect.signature(cls.forward).parameters) == ["self", "x"]
        assert list(inspect.signature(cls.loss).parameters) == ["self", "x"]
        assert list(inspect.signature(mod.train_step).parameters) == ["model", "images", "optim", "lr_sched", "perceptual", "perceptual_weight"]
        assert inspect.signature(mod.train_step).parameters["perceptual_weight"].default == 1.0
    assert list(inspect.signature(TT.Quantizer.forward).parameters) == ["self", "x"]
    a = TT.parse_args([])
    assert (a.image_size, a.patch_size, a.latent_tokens, a.codebook_size, a.latent_dim, a.transformer, a.bs) == (128, 16, 256, 2048, 12, "B", 32)
    assert (a.lr, a.weight_decay, a.warmup_steps, a.max_grad_norm) == (1e-4, 1e-4, 5000, None)
    b = TQ.parse_args(["--max_grad_norm", "1.0"])
    assert (b.image_size, b.patch_size, b.codebook_size, b.latent_dim, b.max_grad_norm) == (128, 16, 2048, 12, 1.0) and not hasattr(b, "latent_tokens")
