"""CPU-side checks of the Enhancing ViT-VQGAN tokenizer (no GPU): the C-ABI surface of its kernels, the module surface against the
reference's golden (state-dict keys and shapes, the sincos tables, the initialisation rule, the refusals), and the float64 restatements
of tests/_enhancing_ref.py against torch - with the checks the GPU tests use shown to fail for the listed mistakes."""
import ctypes

import numpy as np
import pytest
import torch

import _abi
import _enhancing_ref as E
from conftest import load_golden

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NAMES = {"vitamd_tanh_bf16": 4, "vitamd_tanh_bwd_bf16": 5, "vitamd_recon_l1_fwd": 13, "vitamd_recon_l1_bwd": 13}


def _tiny(g=None):
    import train_enhancing_vitvqgan as EV
    c = (g or load_golden("enhancing_tiny.pt"))["cfg"]
    cfg = EV.ViTVQGANConfig(c["image_size"], c["patch_size"], c["codebook_size"], c["latent_dim"], c["transformer"])
    return EV, EV.ViTVQGAN(cfg, dim=c["dim"], depth=c["depth"], heads=c["heads"], mlp_dim=c["mlp_dim"])


# ------------------------------------------------------------------------------------------------ the library surface
def test_the_four_symbols_are_bound():
    from vitamd import lib
    header = _abi.header()
    dll = lib.load()
    for name, nargs in NAMES.items():
        assert name in lib.SIGNATURES and f"int {name}(" in header
        fn = getattr(dll, name)
        assert len(lib.SIGNATURES[name]) == nargs and fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
        params = _abi.declaration(name)
        assert params.count(",") + 1 == nargs
    assert dll.vitamd_abi_version() == 9 == lib.ABI_VERSION


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """null pointers, n < 1 and shapes that do not fit are answered with the library's error codes; no device is needed to ask"""
    from vitamd import lib
    dll = lib.load()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    OK, SHAPE, ARG = 0, 1, 2
    assert dll.vitamd_tanh_bf16(p, p, 0, None) == SHAPE and dll.vitamd_tanh_bf16(p, p, -3, None) == SHAPE
    assert dll.vitamd_tanh_bf16(None, p, 8, None) == ARG and dll.vitamd_tanh_bf16(p, None, 8, None) == ARG
    assert dll.vitamd_tanh_bf16(p + 1, p + 1, 8, None) == ARG                                   # not 2-byte aligned
    assert dll.vitamd_tanh_bwd_bf16(p, None, p, 8, None) == ARG and dll.vitamd_tanh_bwd_bf16(p, p, p, 0, None) == SHAPE
    # B, G, p, c, ld
    assert dll.vitamd_recon_l1_fwd(p, 1, p, p, None, p, 1 << 20, 0, 2, 8, 3, 192, None) == SHAPE        # B < 1
    assert dll.vitamd_recon_l1_fwd(p, 1, p, p, None, p, 1 << 20, 1, 2, 2, 3, 16, None) == SHAPE         # 12 bf16 features: not whole 16-byte pieces
    assert dll.vitamd_recon_l1_fwd(p, 1, p, p, None, p, 1 << 20, 1, 2, 8, 3, 190, None) == SHAPE        # row stride below the width
    assert dll.vitamd_recon_l1_fwd(None, 1, p, p, None, p, 1 << 20, 1, 2, 8, 3, 192, None) == ARG
    assert dll.vitamd_recon_l1_fwd(p, 1, p, p, None, p, 4, 1, 2, 8, 3, 192, None) == ARG                # workspace too small
    assert dll.vitamd_recon_l1_fwd(p + 2, 1, p, p, None, p, 1 << 20, 1, 2, 8, 3, 192, None) == SHAPE    # tokens off the 16-byte grid
    assert dll.vitamd_recon_l1_bwd(p, 1, p, None, None, None, 1, 2, 8, 3, 192, 192, None) == ARG
    assert dll.vitamd_recon_l1_bwd(p, 1, p, None, None, p, 1, 2, 8, 3, 192, 200, None) == ARG           # in place with another stride
    assert dll.vitamd_recon_l1_bwd(p, 0, p, None, None, p, 1, 2, 66, 3, 13068, 13068, None) == SHAPE    # one fp32 token beyond 48 KiB
    assert OK == 0


def test_host_ops_check_their_arguments():
    from vitamd import enhancing, ops
    from vitamd.lib import VitamdError
    x = torch.zeros(8, dtype=BF16)
    for call in (lambda: ops.tanh_bf16(x), lambda: ops.tanh_bwd_bf16(x, x), lambda: ops.tanh_bf16(torch.zeros(8)),
                 lambda: enhancing.tanh_mlp(torch.zeros(2, 64), torch.zeros(64, 64), None, torch.zeros(64, 64), None),
                 lambda: enhancing.tanh_mlp(torch.zeros(2, 64), torch.zeros(64, 48), None, torch.zeros(64, 64), None),
                 lambda: enhancing.recon_l1(torch.zeros(4, 192), torch.zeros(1, 3, 16, 16), 2, 8),
                 lambda: enhancing.linear_recon_l1(torch.zeros(4, 64), torch.zeros(64, 3, 8, 8), None, torch.zeros(1, 3, 16, 16), 2, 8)):
        with pytest.raises(VitamdError):
            call()
    with pytest.raises(ValueError):
        enhancing.recon_l1(torch.zeros(4, 192), torch.zeros(1, 3, 16, 16), 2, 4)
    with pytest.raises(ValueError):
        enhancing.linear_recon_l1(torch.zeros(5, 64), torch.zeros(64, 3, 8, 8), None, torch.zeros(1, 3, 16, 16), 2, 8)


# ------------------------------------------------------------------------------------------------ the module surface
def test_sincos_tables_match_the_reference():
    EV, _ = _tiny()
    g = load_golden("enhancing_tiny.pt")
    dim = g["cfg"]["dim"]
    for key, grid in (("4x4", (4, 4)), ("2x3", (2, 3))):
        got = EV.get_2d_sincos_pos_embed(dim, grid)
        assert isinstance(got, np.ndarray) and got.shape == (grid[0] * grid[1], dim) == tuple(g["sincos"][key].shape)
        assert np.abs(got - g["sincos"][key].double().numpy()).max() <= 2.0 ** -24          # the fixture holds the table rounded to fp32
    assert EV.get_2d_sincos_pos_embed(dim, 4).shape == (16, dim)
    assert np.array_equal(EV.get_2d_sincos_pos_embed(dim, 4), EV.get_2d_sincos_pos_embed(dim, (4, 4)))


def test_state_dict_contract_and_fixed_tables():
    g = load_golden("enhancing_tiny.pt")
    EV, m = _tiny(g)
    sd = m.state_dict()
    assert sorted(sd.keys()) == g["state_keys"]
    assert {k: list(v.shape) for k, v in sd.items()} == g["state_shapes"]
    assert sum(p.numel() for p in m.parameters()) == g["n_params"]
    for key in ("encoder.to_patch_embedding.0.weight", "encoder.transformer.layers.1.0.fn.to_qkv.weight", "decoder.to_pixel.1.bias",
                "decoder.transformer.layers.0.1.fn.net.2.bias", "encoder.transformer.layers.0.1.norm.weight", "decoder.transformer.norm.bias"):
        assert key in sd, key
    assert "encoder.transformer.layers.0.0.fn.to_qkv.bias" not in sd
    assert not m.encoder.en_pos_embedding.requires_grad and not m.decoder.de_pos_embedding.requires_grad
    assert isinstance(m.encoder.en_pos_embedding, torch.nn.Parameter) and m.encoder.en_pos_embedding.shape == (1, 16, g["cfg"]["dim"])
    assert torch.equal(m.encoder.en_pos_embedding[0], g["sincos"]["4x4"]) and torch.equal(m.decoder.de_pos_embedding[0], g["sincos"]["4x4"])
    assert m.get_last_layer() is m.decoder.to_pixel[1].weight and m.decoder.get_last_layer() is m.decoder.to_pixel[-1].weight


def test_default_sizes_are_the_references():
    """ViTVQGAN ignores config.transformer: 768 / 12 / 12 / 3072 (built on the meta device: no memory, no initialisation cost)"""
    import train_enhancing_vitvqgan as EV
    with torch.device("meta"):
        m = EV.ViTVQGAN(EV.ViTVQGANConfig(128, 16, 2048, 12, "S"))
    assert m.pre_quant_proj.weight.shape == (12, 768) and m.quant_proj.weight.shape == (768, 12) and m.quant.codebook.weight.shape == (2048, 12)
    assert len(m.encoder.transformer.layers) == 12 == len(m.decoder.transformer.layers)
    assert m.encoder.transformer.layers[0][0].fn.heads == 12 and m.encoder.transformer.layers[0][1].fn.net[0].weight.shape == (3072, 768)
    assert m.decoder.to_pixel[1].weight.shape == (768, 3, 16, 16) and m.encoder.en_pos_embedding.shape == (1, 64, 768)
    a = EV.parse_args([])
    assert (a.image_size, a.patch_size, a.latent_tokens, a.codebook_size, a.latent_dim, a.transformer, a.bs) == (128, 16, 256, 2048, 12, "B", 32)
    assert (a.lr, a.weight_decay, a.warmup_steps) == (1e-4, 1e-4, 10000)


def test_init_weights_rule():
    _, m = _tiny()
    for mod in m.encoder.modules():
        if isinstance(mod, torch.nn.Linear):
            assert mod.bias is None or not bool(mod.bias.any())
            bound = (6.0 / (mod.weight.shape[0] + mod.weight.shape[1])) ** 0.5
            assert 0.5 * bound < float(mod.weight.detach().abs().max()) <= bound
        elif isinstance(mod, torch.nn.LayerNorm):
            assert bool((mod.weight == 1).all()) and not bool(mod.bias.any())
    w = m.decoder.to_pixel[1].weight
    assert float(w.detach().abs().max()) <= (6.0 / (w.shape[0] + w[0].numel())) ** 0.5
    lin = torch.nn.Linear(4, 4)
    torch.nn.init.constant_(lin.bias, 3.0)
    import train_enhancing_vitvqgan as EV
    EV.init_weights(lin)
    assert not bool(lin.bias.any())


def test_refusals():
    """dim_head != 64, and heads * dim_head != dim (the reference's no-out-projection form heads == 1, dim_head == dim among them)"""
    import train_enhancing_vitvqgan as EV
    with pytest.raises(NotImplementedError):
        EV.Attention(128, heads=4, dim_head=32)
    with pytest.raises(NotImplementedError):
        EV.Transformer(128, 1, 4, 32, 256)
    with pytest.raises(NotImplementedError):
        EV.Attention(64, heads=2, dim_head=64)
    with pytest.raises(NotImplementedError):
        EV.Attention(128, heads=1, dim_head=128)
    with pytest.raises(NotImplementedError):
        EV.ViTEncoder((32, 64), 8, dim=128, depth=1, heads=2, mlp_dim=256)
    assert EV.Attention(64, heads=1, dim_head=64).to_out.weight.shape == (64, 64)
    _, m = _tiny()
    with pytest.raises(Exception):
        m(torch.zeros(1, 3, 32, 32))                   # no device: the product path refuses instead of falling back


# ------------------------------------------------------------------------------------------------ the restatements against torch
def test_tanh_restatements_match_torch_and_catch_the_derivative_from_the_pre_activation():
    g = torch.Generator().manual_seed(1)
    pre = (torch.randn(4096, generator=g, dtype=F64) * 1.5)
    x = pre.clone().requires_grad_(True)
    t = torch.tanh(x)
    dh = torch.randn(4096, generator=g, dtype=F64)
    t.backward(dh)
    assert torch.allclose(E.tanh_ref(pre), t.detach(), rtol=0, atol=0)
    assert torch.allclose(E.tanh_bwd_ref(dh, t.detach()), x.grad, rtol=1e-13, atol=1e-15)
    # the checks pass for correctly rounded results ...
    xb, _ = E.tanh_values(4099, 2)
    assert not E.check_tanh(torch.tanh(xb.to(F64)).to(BF16), xb, "exact")
    dhb, tb, _ = E.tanh_bwd_values(4099, 3)
    assert not E.check_tanh_bwd(E.tanh_bwd_ref(dhb, tb).to(BF16), dhb, tb, "exact")
    # ... and fail for exp-based forms that do not saturate, a lost zero sign, and the derivative taken from the bf16 pre-activation
    bad = torch.tanh(xb.to(F64)).to(BF16)
    bad[xb.float().abs() >= 20] = float("nan")                                 # inf / inf
    assert E.check_tanh(bad, xb)
    bad = torch.tanh(xb.to(F64)).abs().to(BF16) * torch.sign(xb.float()).to(BF16)          # -0 -> +0
    assert E.check_tanh(bad, xb)
    pre_b = (torch.randn(4096, generator=g) * 1.5).to(BF16)
    t_b = torch.tanh(pre_b.to(F64)).to(BF16)
    dh_b = torch.randn(4096, generator=g).to(BF16)
    from_pre = (dh_b.to(F64) * (1 - torch.tanh(pre_b.to(F64)) ** 2)).to(BF16)
    assert E.check_tanh_bwd(from_pre, dh_b, t_b, "from pre")
    assert not E.check_tanh_bwd(E.tanh_bwd_ref(dh_b, t_b).to(BF16), dh_b, t_b, "from t")


def test_conv_transpose_is_a_linear_head_and_the_c_p1_p2_shuffle():
    g = torch.Generator().manual_seed(5)
    B, G, p, c, dim = 2, 3, 4, 3, 16
    convt = torch.nn.ConvTranspose2d(dim, c, kernel_size=p, stride=p).double()
    h = torch.randn(B, G * G, dim, generator=g, dtype=F64)
    want = convt(h.transpose(1, 2).reshape(B, dim, G, G))
    y = h.reshape(-1, dim) @ convt.weight.reshape(dim, -1) + convt.bias.repeat_interleave(p * p)
    got = E.conv_shuffle(y, B, G, p, c)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    row, col = E.l1_index(B, G, p, c)
    assert torch.equal(y[row, col], got)
    from vitamd import enhancing
    assert torch.equal(enhancing.conv_shuffle_tokens(y.view(B, G * G, -1), G, p), got)
    # the other order is another image
    row2, col2 = E.l1_index(B, G, p, c, "p1p2c")
    assert not torch.allclose(y[row2, col2], want)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_l1_restatement_matches_torch_and_the_checks_catch_the_listed_mistakes(dtype):
    B, G, p, c = 3, 2, 4, 3
    y, img, g_img, tie = E.l1_inputs(B, G, p, c, 11, dtype)
    assert int(tie.sum()) >= 100
    ref = E.l1_ref(y, img, G, p, E.G_LOSS, g_img)
    # torch autograd in float64 agrees away from the ties (torch's sign(0) is 0 as well, so everywhere)
    t = y.to(F64).clone().requires_grad_(True)
    recon = E.conv_shuffle(t, B, G, p, c)
    loss = (recon - img.to(F64)).abs().mean()
    (loss * E.G_LOSS + (recon * g_img.to(F64)).sum()).backward()
    assert torch.allclose(loss.detach(), ref["loss"], rtol=1e-14) and torch.equal(recon.detach(), ref["recon"])
    assert torch.allclose(t.grad, ref["dy"], rtol=1e-12, atol=1e-18)
    t32 = E.l1_torch(y, img, G, p)
    good = E.l1_standin32(y, img, G, p, E.G_LOSS, g_img)
    assert not E.check_l1(good, ref, t32, tie, g_img, dtype, "stand-in")
    for bug in E.L1_BUGS:
        got = E.l1_standin32(y, img, G, p, E.G_LOSS, g_img, bug=bug)
        fails = E.check_l1(got, ref, t32, tie, g_img, dtype, bug)
        assert fails, bug
    # sign(0) = 1 is caught at the ties, a dropped g_image by the gradient alone
    assert any("ties" in f for f in E.check_l1(E.l1_standin32(y, img, G, p, E.G_LOSS, g_img, bug="sign0_is_1"), ref, t32, tie, g_img, dtype))
    only = E.check_l1(E.l1_standin32(y, img, G, p, E.G_LOSS, g_img, bug="no_g_image"), ref, t32, tie, g_img, dtype)
    assert only and all("gradient" in f for f in only)
    # without g_image the ties must be exactly zero
    ref0 = E.l1_ref(y, img, G, p, E.G_LOSS, None)
    assert not E.check_l1(E.l1_standin32(y, img, G, p, E.G_LOSS, None), ref0, t32, tie, None, dtype, "no g_image")
    assert E.check_l1(E.l1_standin32(y, img, G, p, E.G_LOSS, None, bug="sign0_is_1"), ref0, t32, tie, None, dtype)


def test_tanh_mlp_reference_is_the_module():
    g = torch.Generator().manual_seed(7)
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 8)).double()
    x = torch.randn(5, 8, generator=g, dtype=F64, requires_grad=True)
    dy = torch.randn(5, 8, generator=g, dtype=F64)
    net(x).backward(dy)
    ref = E.tanh_mlp_ref(x, net[0].weight, net[0].bias, net[2].weight, net[2].bias, dy)
    for k, v in (("dx", x.grad), ("dw1", net[0].weight.grad), ("db1", net[0].bias.grad), ("dw2", net[2].weight.grad), ("db2", net[2].bias.grad)):
        assert torch.allclose(ref[k], v, rtol=1e-12, atol=1e-14), k
