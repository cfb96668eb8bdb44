"""The 1D TiTok tokenizer without a GPU: the float64 restatements of tests/_tatitok_ref.py catch every planted mistake and pass torch's
own fp32 evaluation at the shapes the GPU test uses; the new entry points are bound; train_tatitok.TiTok has the reference's keys and
parameter groups; shape and argument errors come before any device is looked at."""
import ctypes

import pytest
import torch

import _abi
import _tatitok_ref as T
import _tokenizer_ref as R
from conftest import load_golden

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NEW_SYMBOLS = {"vitamd_vq_quantize_unit_fwd": 12, "vitamd_vq_quantize_unit_bwd": 12, "vitamd_conv_recon_mse_fwd": 13,
               "vitamd_conv_recon_mse_bwd": 17}
KEYS = ("loss", "recon", "dtok", "dw", "db")


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("i", range(len(T.TAIL_SHAPES)))
def test_tail_checker_passes_torch_fp32_and_fails_every_planted_mistake(i):
    B, G, p = T.TAIL_SHAPES[i]
    y, img, w, b, g_recon = T.tail_inputs(B, G, p, 400 + i)
    ref = T.tail_ref(y, img, w, b, G, p, T.G_LOSS, g_recon)
    t32 = T.tail_torch(y, img, w, b, G, p, T.G_LOSS, g_recon)
    # the restatement against torch's own float64 backward of the same graph is the restatement itself; its layout is checked against
    # the independent index formula of the reconstruction-loss reference
    row, col = R.recon_index(B, G, p, 3)
    assert torch.equal(R.pixel_shuffle(y.to(F64), B, G, p, 3), y.to(F64)[row, col])
    good = T.tail_standin32(y, img, w, b, G, p, T.G_LOSS, g_recon)
    assert T.check_tail({k: good[k] for k in KEYS}, ref, t32, "stand-in") == []
    assert T.check_tail({k: t32[k] for k in KEYS}, ref, t32, "torch fp32") == []
    for bug in T.CONV_BUGS:
        bad = T.tail_standin32(y, img, w, b, G, p, T.G_LOSS, g_recon, bug=bug)
        fails = T.check_tail({k: bad[k] for k in KEYS}, ref, t32, bug)
        assert fails, bug
    # the bf16 gradient check: passes the rounded reference, fails a gradient one bf16 ulp off
    yb = y.to(BF16)
    refb = T.tail_ref(yb, img, w, b, G, p, T.G_LOSS, g_recon)
    t32b = T.tail_torch(yb, img, w, b, G, p, T.G_LOSS, g_recon)
    assert T.check_tail_bf16(refb["dtok"].to(BF16), refb, t32b, "rounded") == []
    assert T.check_tail_bf16((refb["dtok"] * (1 + 2.0 ** -7)).to(BF16), refb, t32b, "one ulp off") != []
    for bug in ("unflipped_taps", "no_g_recon"):
        bad = T.tail_standin32(yb, img, w, b, G, p, T.G_LOSS, g_recon, bug=bug)
        assert T.check_tail_bf16(bad["dtok"].to(BF16), refb, t32b, bug) != []


def test_tail_reference_without_upstream_gradients():
    """g_loss = 1 and no g_recon is mse_loss's own backward"""
    B, G, p = T.TAIL_SHAPES[1]
    y, img, w, b, _ = T.tail_inputs(B, G, p, 7)
    ref = T.tail_ref(y, img, w, b, G, p)
    t = y.to(F64).requires_grad_(True)
    loss = torch.nn.functional.mse_loss(torch.nn.functional.conv2d(R.pixel_shuffle(t, B, G, p, 3), w.to(F64), b.to(F64), padding=1), img.to(F64))
    loss.backward()
    assert torch.allclose(ref["dtok"], t.grad, rtol=1e-12, atol=0) and abs(float(ref["loss"]) - float(loss.detach())) < 1e-15


@pytest.mark.parametrize("i", range(len(R.VQ_SHAPES)))
def test_unit_quantiser_checker_passes_torch_fp32_and_fails_every_planted_mistake(i):
    M, K, d = R.VQ_SHAPES[i]
    x, cb, g_q = R.vq_inputs(M, K, d, R.vq_seed(i))
    ref = T.vq_unit_ref(x, cb, g_q, R.G_LOSS)
    # the restatement against torch's float64 evaluation of the wrapper's expressions
    t64 = T.vq_unit_torch(x, cb, ref["idx"], g_q, R.G_LOSS, dtype=F64)
    for k in ("unit", "q", "loss", "dx", "dcb"):
        assert torch.allclose(ref[k], t64[k], rtol=1e-9, atol=1e-12), k
    t32 = T.vq_unit_torch(x, cb, ref["idx"], g_q, R.G_LOSS)
    good = T.vq_unit_standin32(x, cb, ref["idx"], g_q, R.G_LOSS)
    assert T.check_vq(good, ref, t32, "stand-in") == []
    # width one: a unit row and its nearest unit code are the same point (+1 or -1), every loss and codebook term is exactly zero, and only
    # the raw codes can be told apart; the three wider shapes show every mistake (as _tokenizer_ref's own host test has it)
    for bug in (T.VQ_UNIT_BUGS if d > 1 else ("raw_codes",)):
        bad = T.vq_unit_standin32(x, cb, ref["idx"], g_q, R.G_LOSS, bug=bug)
        assert T.check_vq(bad, ref, t32, bug), bug


# ------------------------------------------------------------------------------------------------ binding
def test_new_symbols_are_bound_and_the_abi_version_stays():
    from vitamd import lib
    L = lib.load()
    header = _abi.header()
    for name, nargs in NEW_SYMBOLS.items():
        fn = getattr(L, name)
        assert len(lib.SIGNATURES[name]) == nargs and fn.argtypes == lib.SIGNATURES[name] and fn.restype is ctypes.c_int
        assert _abi.declared()[1][name] == "int" and len(_abi.declaration(name).split(",")) == nargs, name
    assert L.vitamd_conv_recon_mse_ws_bytes.restype is ctypes.c_long and "long vitamd_conv_recon_mse_ws_bytes(" in header
    assert L.vitamd_abi_version() == 9 == lib.ABI_VERSION
    # one 32 x 32 tile per workgroup: 256 px = 64 tiles an image; one loss partial forward, 84 gradient partials backward
    assert L.vitamd_conv_recon_mse_ws_bytes(256, 16, 16, 1, 0) == 256 * 64 * 4
    assert L.vitamd_conv_recon_mse_ws_bytes(256, 16, 16, 1, 1) == 256 * 64 * 84 * 4
    assert L.vitamd_conv_recon_mse_ws_bytes(1, 5, 8, 1, 0) == 4 * 4                    # 40 px: two tiles a side
    assert L.vitamd_conv_recon_mse_ws_bytes(1, 4, 4, 1, 0) == -1                       # bf16 needs patch % 8
    assert L.vitamd_conv_recon_mse_ws_bytes(1, 4, 4, 0, 0) == 4 and L.vitamd_conv_recon_mse_ws_bytes(1, 4, 6, 0, 0) == -1


def test_entry_points_refuse_before_any_launch():
    """null pointers everywhere: a shape error is reported first, valid numbers then give the argument error; nothing is launched"""
    from vitamd import lib
    L = lib.load()
    SHAPE, ARG = 1, 2
    N = None
    assert L.vitamd_conv_recon_mse_fwd(N, 1, N, N, N, N, N, N, 2, 4, 12, 432, N) == SHAPE          # patch 12 in bf16
    assert L.vitamd_conv_recon_mse_fwd(N, 1, N, N, N, N, N, N, 2, 4, 8, 190, N) == SHAPE           # row stride below 3 p p
    assert L.vitamd_conv_recon_mse_fwd(N, 0, N, N, N, N, N, N, 2, 4, 8, 194, N) == SHAPE           # row stride no multiple of 4
    assert L.vitamd_conv_recon_mse_fwd(N, 1, N, N, N, N, N, N, 2, 4, 8, 192, N) == ARG
    assert L.vitamd_conv_recon_mse_bwd(N, 1, N, N, N, N, N, N, N, N, N, 2, 4, 8, 192, 100, N) == SHAPE
    assert L.vitamd_conv_recon_mse_bwd(N, 1, N, N, N, N, N, N, N, N, N, 2, 4, 8, 192, 200, N) == ARG
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)
    assert L.vitamd_conv_recon_mse_bwd(a, 0, a, a, a, N, N, a, a, a, a, 1, 1, 4, 48, 48, N) == ARG  # in place
    assert L.vitamd_vq_quantize_unit_fwd(N, N, N, N, N, N, N, N, 4, 4, 65, N) == SHAPE
    assert L.vitamd_vq_quantize_unit_fwd(N, N, N, N, N, N, N, N, 4, 4, 64, N) == ARG
    assert L.vitamd_vq_quantize_unit_bwd(N, N, N, N, N, N, N, N, 0, 4, 8, N) == SHAPE
    assert L.vitamd_vq_quantize_unit_bwd(N, N, N, N, N, N, N, N, 4, 4, 8, N) == ARG


def test_python_entry_points_check_shapes_before_any_device():
    from vitamd import ops, tokenizer
    from vitamd.lib import VitamdError
    B, G, p = 2, 3, 8
    tok, img = torch.zeros(B, G * G, 3 * p * p), torch.zeros(B, 3, G * p, G * p)
    w, b = torch.zeros(3, 3, 3, 3), torch.zeros(3)
    h, fw, fb = torch.zeros(B, G * G, 64), torch.zeros(3 * p * p, 64), torch.zeros(3 * p * p)
    with pytest.raises(ValueError):
        tokenizer.conv_recon_mse(tok, w, b, img, G + 1, p)
    with pytest.raises(ValueError):
        tokenizer.conv_recon_mse(tok, torch.zeros(3, 3, 5, 5), b, img, G, p)
    with pytest.raises(ValueError):
        tokenizer.conv_recon_mse(tok[:, :, :-3], w, b, img, G, p)
    with pytest.raises(ValueError):
        tokenizer.linear_conv_recon_mse(h, fw, fb, w, b, img[:1], G, p)
    with pytest.raises(VitamdError):
        tokenizer.linear_conv_recon_mse(h, fw[:, :32], fb, w, b, img, G, p)
    with pytest.raises(ValueError):
        ops.conv_recon_mse_fwd(tok.view(-1, 3 * p * p), w, b[:2], img, G, p)
    # right shapes on the host: refused as host tensors, never computed there
    for call in (lambda: tokenizer.conv_recon_mse(tok, w, b, img, G, p), lambda: tokenizer.linear_conv_recon_mse(h, fw, fb, w, b, img, G, p),
                 lambda: ops.conv_recon_mse_fwd(tok.view(-1, 3 * p * p), w, b, img, G, p),
                 lambda: ops.conv_recon_mse_bwd(tok.view(-1, 3 * p * p), w, b, img, G, p),
                 lambda: tokenizer.vq_quantize(torch.zeros(4, 12), torch.zeros(8, 12), unit_codes=True)):
        with pytest.raises(VitamdError):
            call()
    with pytest.raises(ValueError):
        ops.vq_quantize_unit_fwd(torch.zeros(4, 65), torch.zeros(8, 65))
    # the 16-byte path's rule, without a device
    assert ops.conv_recon_mse_applies(torch.zeros(4, 48), 4) and not ops.conv_recon_mse_applies(torch.zeros(4, 48, dtype=BF16), 4)
    assert ops.conv_recon_mse_applies(torch.zeros(4, 192, dtype=BF16), 8) and not ops.conv_recon_mse_applies(torch.zeros(4, 108), 6)
    assert tokenizer.fused_head_applies(192, 512) and not tokenizer.fused_head_applies(48, 512)


# ------------------------------------------------------------------------------------------------ the model
def _cfg(c):
    import train_tatitok as TA
    return TA.TiTokConfig(c["image_size"], c["patch_size"], c["latent_tokens"], c["codebook_size"], c["latent_dim"], c["transformer"],
                          c["use_l2_norm"])


def test_titok_has_the_reference_keys_shapes_and_init():
    import train_tatitok as TA
    g = load_golden("tatitok_tiny.pt")
    m = TA.TiTok(_cfg(g["cfg"]))
    assert sorted(m.state_dict().keys()) == g["state_keys"]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == g["state_shapes"]
    assert sum(p.numel() for p in m.parameters()) == g["n_params"]
    for attr in ("encoder", "decoder", "latent_tokens", "quantize"):
        assert hasattr(m, attr)
    K = g["cfg"]["codebook_size"]
    # the initialisation pass runs before the quantiser exists: uniform codebook, truncated-normal projections, unit LayerNorms
    assert float(m.quantize.embedding.weight.abs().max()) <= 1.0 / K + 1e-9
    assert float(m.decoder.ffn[0].bias.abs().max()) == 0 and 0.01 < float(m.decoder.ffn[0].weight.std()) < 0.03
    assert 0.015 < float(m.encoder.patch_embed.weight.std()) < 0.025 and float(m.encoder.patch_embed.bias.abs().max()) == 0
    assert bool((m.encoder.ln_pre.weight == 1).all()) and m.quantize.use_l2_norm and m.quantize.commitment_cost == 0.25
    assert TA.TiTok(dict(g["cfg"])).num_latent_tokens == g["cfg"]["latent_tokens"]      # a plain dict is accepted, as by the reference
    assert hasattr(m.decoder, "features")


def test_make_optim_builds_the_reference_groups():
    import train_tatitok as TA
    from types import SimpleNamespace as NS
    m = TA.TiTok(TA.TiTokConfig(32, 8, 8, 64, 12, "small"))
    groups = TA.param_groups(m, 1e-4)
    assert [len(gr["params"]) for gr in groups] == [152, 67] and [gr["weight_decay"] for gr in groups] == [0.0, 1e-4]
    names = {id(p): n for n, p in m.named_parameters()}
    no_decay, decay = ({names[id(p)] for p in gr["params"]} for gr in groups)
    assert {"encoder.patch_embed.weight", "decoder.decoder_embed.weight", "quantize.embedding.weight", "latent_tokens",
            "decoder.mask_token", "encoder.transformer.0.ln_1.weight"} <= no_decay
    assert {"encoder.transformer.0.attn.in_proj_weight", "decoder.transformer.7.mlp.c_fc.weight", "decoder.ffn.0.weight",
            "encoder.conv_out.weight", "decoder.conv_out.weight", "encoder.transformer.0.attn.out_proj.weight"} <= decay
    assert len(no_decay) + len(decay) == 219 == len(list(m.parameters()))
    o = TA.make_optim(m, NS(lr=1e-4, weight_decay=1e-4, max_grad_norm=None))
    assert type(o) is torch.optim.AdamW and [len(gr["params"]) for gr in o.param_groups] == [152, 67]
    assert o.param_groups[0]["weight_decay"] == 0.0 and o.param_groups[1]["weight_decay"] == 1e-4 and o.param_groups[0]["betas"] == (0.9, 0.999)
    args = TA.parse_args([])
    assert args.max_grad_norm == 1.0 and args.transformer == "small" and args.codebook_size == 16384 and args.latent_tokens == 256


def test_video_bridge_rearranges_as_the_reference_loop_does():
    """with a stand-in tokenizer on the host: frame order, shapes, dtype, the clamp, and the training flag put back"""
    import train_videogpt as TV

    class Tok(torch.nn.Module):
        def encode(self, x):
            assert not self.training and not torch.is_grad_enabled()
            ids = (x.mean(dim=(1, 2)) * 10).long()[:, None, :]                      # [B*T, 1, W]: one id per image column
            return x, {"min_encoding_indices": ids}

        def decode_tokens(self, ids):
            assert not self.training
            ids = ids.squeeze(1)
            return (ids.float()[:, None, None, :] / 5 - 0.5).expand(-1, 3, 2, -1)   # values from -0.5 to 1.3

    tok = Tok().train()
    videos = torch.rand(2, 3, 3, 4, 5)
    ids = TV.frames_to_tokens(tok, videos)
    assert ids.shape == (2, 3, 5) and ids.dtype == torch.int64 and tok.training
    tok.eval()
    with torch.no_grad():
        for bi in range(2):
            for ti in range(3):
                assert torch.equal(ids[bi, ti], tok.encode(videos[bi, ti][None])[1]["min_encoding_indices"][0, 0])
    tok.train()
    frames = TV.tokens_to_frames(tok, ids.reshape(2, 15), 3)
    assert frames.shape == (2, 3, 3, 2, 5) and float(frames.min()) >= 0.0 and float(frames.max()) <= 1.0 and tok.training
    want = torch.clamp(tok.eval().decode_tokens(ids[1, 2][None]), 0, 1)[0]
    assert torch.equal(frames[1, 2], want)
    with pytest.raises(ValueError):
        TV.tokens_to_frames(tok, ids.reshape(2, 15), 4)
    with pytest.raises(ValueError):
        TV.frames_to_tokens(tok, videos[0])
    assert TV.parse_args(["--tokenizer", "tatitok"]).tokenizer == "tatitok" and TV.parse_args([]).tokenizer == "none"
