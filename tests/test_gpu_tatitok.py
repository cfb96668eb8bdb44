"""The 1D TiTok tokenizer on the GPU: the fused pixel tail and the unit-code quantiser (csrc/tokenizer.hip) against the float64
restatements of tests/_tatitok_ref.py, vitamd.tokenizer on top of them, train_tatitok.TiTok against the reference's golden and against
the present route, and the video bridge of train_videogpt.

Bounds (tests/_tatitok_ref.py, those of tests/_tokenizer_ref.py), all measured against float64, never against the kernel's own output:
every fp32 result within max(4 e32, 8 * 2^-24) of the reference on the scale max(1, |ref|), e32 being the same distance for torch's fp32
CPU evaluation at that shape; gradients that carry 1 / (element count) are brought to order one first; the bf16 gradient within half a
bf16 ulp (+1/16) on top; dw / db and dcodebook n 2^-24 sum|terms| on top for the order of their sums."""
import functools

import pytest
import torch

import _tatitok_ref as T
import _tokenizer_ref as R
import vit_oracle as O
import weights as W
from conftest import load_golden

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
PAD, SENT = 8, 7.0


# ------------------------------------------------------------------------------------------------ 1. the tail kernels
@functools.lru_cache(maxsize=None)
def _tail_case(i, dtype, with_loss, with_recon):
    B, G, p = T.TAIL_SHAPES[i]
    y, img, w, b, g_recon = T.tail_inputs(B, G, p, 400 + i, dtype)
    g_loss = T.G_LOSS if with_loss else 1.0
    gr = g_recon if with_recon else None
    return y, img, w, b, g_recon, T.tail_ref(y, img, w, b, G, p, g_loss, gr), T.tail_torch(y, img, w, b, G, p, g_loss, gr)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32), b.contiguous().view(torch.int16 if b.dtype == BF16 else torch.int32))


@pytest.mark.parametrize("with_recon", [True, False])
@pytest.mark.parametrize("with_loss", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("i", range(len(T.TAIL_SHAPES)))
def test_tail_kernels_match_float64(hip, i, dtype, with_loss, with_recon):
    """tokens as a view of a wider buffer whose pad columns hold NaN; the gradient into a second padded buffer whose pads stay untouched;
    the upstream gradient of the loss given (2.5) and absent (1), that of the reconstruction given and absent; the same bits twice"""
    from vitamd import ops
    B, G, p = T.TAIL_SHAPES[i]
    y, img, w, b, g_recon, ref, t32 = _tail_case(i, dtype, with_loss, with_recon)
    M, F = y.shape
    buf = torch.full((M, F + PAD), float("nan"), dtype=dtype)
    buf[:, :F] = y
    bufd, imgd, wd, bd = buf.cuda(), img.cuda(), w.cuda(), b.cuda()
    tok = bufd[:, :F]
    gl = torch.tensor(T.G_LOSS, device="cuda") if with_loss else None
    gr = g_recon.cuda() if with_recon else None

    def run():
        loss, recon = ops.conv_recon_mse_fwd(tok, wd, bd, imgd, G, p, want_recon=True)
        obuf = torch.full((M, F + 2 * PAD), SENT, dtype=dtype, device="cuda")
        dtok, dw, db = ops.conv_recon_mse_bwd(tok, wd, bd, imgd, G, p, gl, gr, out=obuf[:, :F])
        return loss, recon, obuf, dtok, dw, db

    loss, recon, obuf, dtok, dw, db = run()
    loss_only, none = ops.conv_recon_mse_fwd(tok, wd, bd, imgd, G, p)
    assert none is None and _same_bits(loss_only, loss)
    assert bool(torch.isnan(bufd[:, F:]).all()) and torch.equal(bufd[:, :F].cpu(), y)            # the tokens and their pads are as they were
    assert bool((obuf[:, F:] == SENT).all()) and dtok.dtype == dtype and dtok.data_ptr() == obuf.data_ptr()
    assert recon.shape == img.shape and recon.dtype == F32 and dw.shape == (3, 3, 3, 3) and db.shape == (3,)
    label = f"case {T.TAIL_SHAPES[i]} {dtype} g_loss {with_loss} g_recon {with_recon}"
    got = {"loss": loss.cpu(), "recon": recon.cpu(), "dw": dw.cpu(), "db": db.cpu()}
    if dtype == F32:
        got["dtok"] = dtok.cpu()
    fails = T.check_tail(got, ref, t32, label)
    if dtype == BF16:
        fails += T.check_tail_bf16(dtok.cpu(), ref, t32, label)
    assert not fails, fails
    again = run()
    for name, a, c in zip(("loss", "recon", "dtokens", "dtokens", "dw", "db"), (loss, recon, obuf, dtok, dw, db), again):
        assert _same_bits(a, c), name
    dense, _, _ = ops.conv_recon_mse_bwd(tok, wd, bd, imgd, G, p, gl, gr)
    assert dense.is_contiguous() and _same_bits(dense, dtok)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_tail_refuses_what_its_16_byte_path_cannot_take(hip, dtype):
    """a patch of 4 in bf16 / 6 in fp32, an unaligned base, the tokens as their own gradient buffer: ops refuses; tokenizer.conv_recon_mse
    takes the present operators on those shapes and is still right"""
    from vitamd import ops, tokenizer
    from vitamd.lib import VitamdError
    B, G, p = 2, 3, (4 if dtype == BF16 else 6)
    y, img, w, b, g_recon = T.tail_inputs(B, G, p, 77, dtype)
    yd, imgd, wd, bd = y.cuda(), img.cuda(), w.cuda(), b.cuda()
    assert not ops.conv_recon_mse_applies(yd, p)
    with pytest.raises(VitamdError):
        ops.conv_recon_mse_fwd(yd, wd, bd, imgd, G, p)
    with pytest.raises(VitamdError):
        ops.conv_recon_mse_bwd(yd, wd, bd, imgd, G, p)
    y8, img8, _, _, _ = T.tail_inputs(1, 2, 8, 78, dtype)
    buf = torch.zeros((4, 192 + 8), dtype=dtype, device="cuda")
    buf[:, 1:193] = y8.cuda()
    off = buf[:, 1:193]
    assert off.data_ptr() % 16 != 0 and not ops.conv_recon_mse_applies(off, 8) and ops.conv_recon_mse_applies(y8.cuda(), 8)
    with pytest.raises(VitamdError):
        ops.conv_recon_mse_fwd(off, wd, bd, img8.cuda(), 2, 8)
    with pytest.raises(VitamdError):
        ops.conv_recon_mse_bwd(y8.cuda(), wd, bd, img8.cuda(), 2, 8, out=off)
    t8 = y8.cuda()
    with pytest.raises(VitamdError):
        ops.conv_recon_mse_bwd(t8, wd, bd, img8.cuda(), 2, 8, out=t8)                    # never in place
    # the fallback, with both outputs carrying a gradient
    ref = T.tail_ref(y, img, w, b, G, p, T.G_LOSS, g_recon)
    t32 = T.tail_torch(y, img, w, b, G, p, T.G_LOSS, g_recon)
    t = yd.view(B, G * G, -1).detach().requires_grad_(True)
    wp, bp = wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    loss, recon = tokenizer.conv_recon_mse(t, wp, bp, imgd, G, p, return_recon=True)
    (loss * T.G_LOSS + (recon * g_recon.cuda()).sum()).backward()
    got = {"loss": loss.detach().cpu(), "recon": recon.detach().cpu(), "dw": wp.grad.cpu(), "db": bp.grad.cpu()}
    g = t.grad.cpu().view(B * G * G, -1)
    if dtype == F32:
        got["dtok"] = g
    fails = T.check_tail(got, ref, t32, "fallback")
    if dtype == BF16:
        fails += T.check_tail_bf16(g, ref, t32, "fallback")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 2. the unit-code quantiser
@functools.lru_cache(maxsize=None)
def _vq_case(i):
    M, K, d = R.VQ_SHAPES[i]
    x, cb, g_q = R.vq_inputs(M, K, d, R.vq_seed(i))
    return x, cb, g_q, T.vq_unit_ref(x, cb, g_q, R.G_LOSS)


def _run_unit_quantiser(x, cb, g_q, g_loss):
    from vitamd import ops
    xd, cbd = x.cuda(), cb.cuda()
    unit, rnorm, q, idx, loss, eunit = ops.vq_quantize_unit_fwd(xd, cbd, return_unit_codes=True)
    eunit = eunit.clone()
    dx, dcb = ops.vq_quantize_unit_bwd(g_q.cuda(), torch.tensor(g_loss, device="cuda"), unit, rnorm, idx, cbd)
    return {"unit": unit, "rnorm": rnorm, "q": q, "idx": idx, "loss": loss, "eunit": eunit, "dx": dx, "dcb": dcb}


@pytest.mark.parametrize("i", range(len(R.VQ_SHAPES)))
def test_unit_quantiser_kernels_match_float64(hip, i):
    from vitamd import ops
    x, cb, g_q, ref0 = _vq_case(i)
    label = f"unit case {R.VQ_SHAPES[i]}"
    dev = _run_unit_quantiser(x, cb, g_q, R.G_LOSS)
    got = {k: v.cpu() for k, v in dev.items()}
    fails, exempt = T.check_ids(got["idx"], ref0, label)
    assert int(got["idx"].min()) >= 0 and int(got["idx"].max()) < cb.shape[0]
    use = torch.where(exempt, got["idx"], ref0["idx_ref"])
    ref = ref0 if torch.equal(use, ref0["idx"]) else T.vq_unit_ref(x, cb, g_q, R.G_LOSS, idx=use)
    fails += T.check_vq(got, ref, T.vq_unit_torch(x, cb, use, g_q, R.G_LOSS), label)
    assert not fails, fails
    # the search is the raw-code quantiser's, bit for bit; the forward gives the same bits twice
    raw = ops.vq_quantize_fwd(x.cuda(), cb.cuda())
    assert torch.equal(dev["idx"], raw[3]) and torch.equal(dev["unit"], raw[0]) and torch.equal(dev["rnorm"], raw[1])
    again = _run_unit_quantiser(x, cb, g_q, R.G_LOSS)
    for k in ("unit", "rnorm", "q", "loss", "dx"):
        assert torch.equal(dev[k].view(torch.int32), again[k].view(torch.int32)), k
    # q is the unit code row the search compared against
    assert torch.equal((dev["unit"] + (dev["eunit"][dev["idx"]] - dev["unit"])).view(torch.int32), dev["q"].view(torch.int32))


def test_vq_quantize_unit_codes_matches_the_reference_golden(hip):
    """blocks_tokenizers.pt["vq_l2norm"], as test_gpu_parity holds the wrapper to it: indices equal, losses to 1e-6, values to fp32 rounding;
    then the wrapper itself on the same tensors, and the wide-code fallback against the wrapper"""
    import blocks as BK
    from test_gpu_parity import _err
    from test_oracle import vq_case_tensors
    from vitamd import tokenizer
    case = load_golden("blocks_tokenizers.pt")["vq_l2norm"]
    code, z, dy = vq_case_tensors(case)
    cb = code.cuda().requires_grad_(True)
    zd = z.cuda().requires_grad_(True)
    q, ids, loss = tokenizer.vq_quantize(zd.permute(0, 2, 3, 1), cb, unit_codes=True)
    zq = q.permute(0, 3, 1, 2)
    assert ids.dtype == torch.int64 and not ids.requires_grad and loss.dim() == 0
    ((zq * dy.cuda()).sum() + loss).backward()
    assert torch.equal(ids.cpu(), case["indices"])
    assert abs(float(loss.detach()) - case["quantizer_loss"]) < 1e-6
    assert _err(zq.detach(), case["zq"]) < 1e-6 and _err(zd.grad, case["dz"]) < 1e-5
    assert _err(cb.grad, case["dcodebook"]) < 1e-5
    # wide codes (d = 80) stay on the torch expressions: equal to the wrapper
    x, cbw, g_q = R.vq_inputs(300, 40, 80, 130)
    vq = BK.VectorQuantizer(codebook_size=40, token_size=80, use_l2_norm=True).cuda()
    with torch.no_grad():
        vq.embedding.weight.copy_(cbw)
    xa = x.view(2, 1, 150, 80).cuda().requires_grad_(True)
    z0, info = vq(xa.permute(0, 3, 1, 2))
    ((z0.permute(0, 2, 3, 1) * g_q.view(2, 1, 150, 80).cuda()).sum() + info["quantizer_loss"] * R.G_LOSS).backward()
    xb = x.view(2, 1, 150, 80).cuda().requires_grad_(True)
    cbp = cbw.cuda().requires_grad_(True)
    q1, ids1, l1 = tokenizer.vq_quantize(xb, cbp, unit_codes=True)
    ((q1 * g_q.view(2, 1, 150, 80).cuda()).sum() + l1 * R.G_LOSS).backward()
    assert torch.equal(ids1, info["min_encoding_indices"].view(2, 1, 150))
    assert O.rel_l2(q1.detach().cpu(), z0.permute(0, 2, 3, 1).detach().cpu()) < 1e-6 and abs(float(l1.detach()) - float(info["quantizer_loss"].detach())) < 1e-6
    assert O.rel_l2(xb.grad.cpu(), xa.grad.cpu()) < 1e-5 and O.rel_l2(cbp.grad.cpu(), vq.embedding.weight.grad.cpu()) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. autograd
@pytest.mark.parametrize("F_D_p, fused", [((192, 64, 8), True), ((192, 48, 8), False), ((48, 64, 4), False)])
@pytest.mark.parametrize("with_recon", [False, True])
def test_linear_conv_recon_mse_matches_the_present_tail(hip, F_D_p, fused, with_recon):
    """head + tail against functions.linear + pixel shuffle + Conv3x3Fn + mse_loss on the same device tensors, with a 1x1-conv weight as
    the decoder holds it; with_recon: (recon * dy).sum() added to the loss; the fused form refuses a second backward"""
    from vitamd import tokenizer
    from vitamd.block_functions import Conv3x3Fn
    from vitamd.functions import linear
    F, D, p = F_D_p
    B, G = 2, 3
    assert (tokenizer.fused_head_applies(F, D) and p % 8 == 0) == fused
    g = torch.Generator().manual_seed(19)
    h = torch.randn(B, G * G, D, generator=g)
    img = torch.rand(B, 3, G * p, G * p, generator=g)
    dy = torch.randn(B, 3, G * p, G * p, generator=g) / img.numel()
    ffn = torch.nn.Conv2d(D, F, 1).cuda()
    conv = torch.nn.Conv2d(3, 3, 3, padding=1).cuda()
    params = [ffn.weight, ffn.bias, conv.weight, conv.bias]
    ha = h.cuda().requires_grad_(True)
    y = linear(ha, ffn.weight.view(F, D), ffn.bias)
    recon0 = Conv3x3Fn.apply(tokenizer.pixel_shuffle_tokens(y, G, p), conv.weight, conv.bias)
    want = torch.nn.functional.mse_loss(recon0, img.cuda())
    (want * T.G_LOSS + ((recon0 * dy.cuda()).sum() if with_recon else 0)).backward()
    ref_g = [ha.grad.clone()] + [q.grad.clone() for q in params]
    for q in params:
        q.grad = None
    hb = h.cuda().requires_grad_(True)
    out = tokenizer.linear_conv_recon_mse(hb, ffn.weight, ffn.bias, conv.weight, conv.bias, img.cuda(), G, p, return_recon=with_recon)
    loss, recon = out if with_recon else (out, None)
    assert loss.dim() == 0 and loss.dtype == F32 and (recon is None or (recon.shape == img.shape and recon.requires_grad))
    total = loss * T.G_LOSS + ((recon * dy.cuda()).sum() if with_recon else 0)
    total.backward(retain_graph=fused)
    if fused:
        with pytest.raises(RuntimeError):
            total.backward()
    # both routes round the tokens to bf16 once (2^-9 relative on values of order one) and the token gradient to bf16 once more: the loss
    # within 2^-9 relative, the image within 2^-8 in relative L2, every gradient tensor within 2 * 2^-8 in relative L2
    assert abs(float(loss.detach()) - float(want.detach())) <= 2.0 ** -9 * float(want.detach())
    if with_recon:
        assert O.rel_l2(recon.detach().cpu(), recon0.detach().cpu()) <= 2.0 ** -8
    assert ffn.weight.grad.shape == ffn.weight.shape and conv.weight.grad.shape == (3, 3, 3, 3)
    for name, a, b_ in zip(("dh", "dffn_w", "dffn_b", "dconv_w", "dconv_b"), [hb.grad] + [q.grad for q in params], ref_g):
        e = O.rel_l2(a.cpu(), b_.cpu())
        print(f"{name}: rel L2 new vs present {e:.3e}")
        assert e <= 2 * 2.0 ** -8, (name, e)


def test_conv_recon_mse_autograd_takes_a_gradient_on_the_reconstruction_alone(hip):
    """only the second output used: the loss's own term must drop out (its upstream gradient is zero, not the kernel's default of one)"""
    from vitamd import tokenizer
    B, G, p = T.TAIL_SHAPES[1]
    y, img, w, b, g_recon = T.tail_inputs(B, G, p, 401)
    ref = T.tail_ref(y, img, w, b, G, p, 0.0, g_recon)
    t32 = T.tail_torch(y, img, w, b, G, p, 0.0, g_recon)
    t = y.view(B, G * G, -1).cuda().requires_grad_(True)
    wp, bp = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    loss, recon = tokenizer.conv_recon_mse(t, wp, bp, img.cuda(), G, p, return_recon=True)
    (recon * g_recon.cuda()).sum().backward()
    got = {"loss": loss.detach().cpu(), "recon": recon.detach().cpu(), "dtok": t.grad.cpu().view(B * G * G, -1), "dw": wp.grad.cpu(), "db": bp.grad.cpu()}
    fails = T.check_tail(got, ref, t32, "recon only")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 4. the model
def _tatitok_model():
    import train_tatitok as TA
    g = load_golden("tatitok_tiny.pt")
    c = g["cfg"]
    m = TA.TiTok(TA.TiTokConfig(c["image_size"], c["patch_size"], c["latent_tokens"], c["codebook_size"], c["latent_dim"], c["transformer"],
                                c["use_l2_norm"]))
    assert sorted(m.state_dict().keys()) == g["state_keys"]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == g["state_shapes"]
    m.load_state_dict(W.module_state(c["seed"], g["state_shapes"]), strict=True)
    images = W.uniform(c["seed"], "images", (c["batch"], 3, c["image_size"], c["image_size"]), 0.5) + 0.5
    return g, m.cuda(), images.cuda()


def _present_loss(m, images):
    recon, info = m(images)
    return torch.nn.functional.mse_loss(recon, images) + info["quantizer_loss"], recon, info


def test_titok_vs_reference_golden(hip):
    """the bounds of test_gpu_parity.py::test_tokenizer_vs_reference_golden on the composed model, and decode_tokens on the golden's ids"""
    from test_gpu_parity import _err
    g, m, images = _tatitok_model()
    floor = g["ref_bf16_floor"]
    with torch.no_grad():
        from_ids = m.decode_tokens(g["indices"].cuda())                 # [B, 1, N]
        from_ids2 = m.decode_tokens(g["indices"].squeeze(1).cuda())     # [B, N]
        z = m.encoder(pixel_values=images, latent_tokens=m.latent_tokens)
    assert from_ids.shape == images.shape and torch.equal(from_ids, from_ids2)
    assert _err(from_ids, g["recon_from_indices"]) < 2 * floor["recon"] + 3e-3
    print("latents rel L2", O.rel_l2(z.cpu(), g["latents"]))
    loss, recon, info = _present_loss(m, images)
    agree = float((info["min_encoding_indices"].cpu() == g["indices"]).float().mean())
    assert agree >= min(floor["index_agreement"], 1.0) - 0.03, agree
    assert abs(float(info["quantizer_loss"].detach()) - g["quantize_loss"]) < 2e-3
    assert abs(float(loss.detach()) - g["loss"]) < 5e-3
    loss.backward()
    torch.cuda.synchronize()
    bad = []
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        if p.grad is None or ref["norm"] == 0.0 or p.numel() == 0:
            continue
        assert torch.isfinite(p.grad).all(), k
        e = _err(p.grad, ref)
        if e > 2 * floor["grads"][k] + 1e-2:
            bad.append((k, round(e, 4), round(floor["grads"][k], 4)))
    assert not bad, bad[:8]


def test_titok_loss_route_matches_golden_and_present_route(hip):
    """the rule of test_gpu_tokenizer.py::test_model_loss_route_matches_golden_and_present_route"""
    from test_gpu_parity import _err
    g, m, images = _tatitok_model()
    floor = g["ref_bf16_floor"]
    loss0, _, info = _present_loss(m, images)
    loss0.backward()
    e_parent = {k: _err(p.grad, g["grads"][k]) for k, p in m.named_parameters()
                if p.grad is not None and g["grads"][k]["norm"] != 0.0 and p.numel() > 0}
    m.zero_grad(set_to_none=True)
    recon_loss, qloss1, ids = m.loss(images)
    assert recon_loss.dim() == 0 and qloss1.dim() == 0 and ids.shape == info["min_encoding_indices"].shape
    assert abs(float(qloss1.detach()) - g["quantize_loss"]) < 2e-3
    loss1 = recon_loss + qloss1
    assert abs(float(loss1.detach()) - g["loss"]) < 5e-3
    loss1.backward(retain_graph=True)
    with pytest.raises(RuntimeError):
        loss1.backward()
    torch.cuda.synchronize()
    agree = float((ids == info["min_encoding_indices"]).float().mean())
    print(f"ids agree {agree:.5f}, qloss {float(qloss1.detach()):.6f} / {float(info['quantizer_loss'].detach()):.6f}, "
          f"loss {float(loss1.detach()):.6f} / {float(loss0.detach()):.6f}")
    assert agree >= 0.999
    assert abs(float(qloss1.detach()) - float(info["quantizer_loss"].detach())) < 1e-5 and abs(float(loss1.detach()) - float(loss0.detach())) < 1e-3
    bad = []
    for k, p in m.named_parameters():
        if k not in e_parent:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        e = _err(p.grad, g["grads"][k])
        print(f"{k}: new {e:.3e} present {e_parent[k]:.3e} floor {floor['grads'][k]:.3e}")
        if e > 2 * floor["grads"][k] + 1e-2 or e > 1.5 * e_parent[k] + 1e-3:
            bad.append((k, round(e, 4), round(e_parent[k], 4), round(floor["grads"][k], 4)))
    assert not bad, bad[:8]
    # the image as a fourth result: that of forward(), differentiable
    m.zero_grad(set_to_none=True)
    out = m.loss(images, return_recon=True)
    with torch.no_grad():
        recon0, _ = m(images)
    assert len(out) == 4 and out[3].shape == images.shape and out[3].requires_grad
    assert O.rel_l2(out[3].detach().cpu(), recon0.cpu()) < 2.0 ** -7


def test_titok_loss_without_l2_norm_keeps_the_wrapper_quantiser(hip):
    """use_l2_norm=False is not what the quantiser kernels compute: loss() runs the VectorQuantizer wrapper there and still the fused tail"""
    import train_tatitok as TA
    torch.manual_seed(3)
    m = TA.TiTok(TA.TiTokConfig(32, 8, 8, 64, 12, "small", use_l2_norm=False)).cuda()
    images = (W.uniform(6, "images", (2, 3, 32, 32), 0.5) + 0.5).cuda()
    assert not m._fused_quantiser()
    loss0, _, info = _present_loss(m, images)
    recon_loss, qloss, ids = m.loss(images)
    assert "LinearConvReconMSEFn" in type(recon_loss.grad_fn).__name__
    assert torch.equal(ids, info["min_encoding_indices"]) and abs(float(qloss.detach()) - float(info["quantizer_loss"].detach())) < 1e-6
    assert abs(float((recon_loss + qloss).detach()) - float(loss0.detach())) < 1e-3
    (recon_loss + qloss).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_titok_train_step_follows_the_present_route(hip):
    """the rule of test_gpu_tokenizer.py::test_train_step_follows_the_present_route: two steps against the present route under
    torch.optim.AdamW, a third that has brought the loss down; with a perceptual term the step stays on the fused tail; the grouped
    optimiser with clipping gives finite, changing weights"""
    import train_tatitok as TA
    from types import SimpleNamespace as NS
    _, new, images = _tatitok_model()
    _, old, _ = _tatitok_model()
    o_new = torch.optim.AdamW(new.parameters(), lr=1e-4, weight_decay=1e-4)
    o_old = torch.optim.AdamW(old.parameters(), lr=1e-4, weight_decay=1e-4)
    got, ref = [], []
    for _ in range(3):
        loss = TA.train_step(new, images, o_new)
        assert not loss.requires_grad and loss.is_cuda
        got.append(float(loss))
    for _ in range(2):
        o_old.zero_grad(set_to_none=True)
        loss, _, _ = _present_loss(old, images)
        loss.backward()
        o_old.step()
        ref.append(float(loss.detach()))
    print("train_step losses", got, "present route", ref)
    for a, b in zip(got, ref):
        assert abs(a - b) < 3e-2 * max(1.0, abs(b)), (got, ref)
    assert got[2] < got[0]
    seen = []

    def perceptual(recon, imgs):
        seen.append((tuple(recon.shape), type(recon.grad_fn).__name__))
        return (recon - imgs).abs().mean(dim=(1, 2, 3))
    lp = float(TA.train_step(new, images, o_new, perceptual=perceptual, perceptual_weight=0.5))
    assert len(seen) == 1 and seen[0][0] == tuple(images.shape) and "LinearConvReconMSEFn" in seen[0][1] and lp > got[2] * 0.5
    # the reference's groups, clipped on the device before the update
    optim = TA.make_optim(new, NS(lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0))
    assert [len(gr["params"]) for gr in optim.param_groups] == [152, 67] and type(optim).__module__ == "vitamd.optim"
    before = {k: p.detach().clone() for k, p in new.named_parameters()}
    for _ in range(2):
        loss = TA.train_step(new, images, optim)
    assert bool(torch.isfinite(loss))
    for k, p in new.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        assert p.grad is not None and (not bool(p.grad.any()) or not torch.equal(p.detach(), before[k])), k      # a gradient moves its parameter
    assert sum(int(not torch.equal(p.detach(), before[k])) for k, p in new.named_parameters()) >= 200


# ------------------------------------------------------------------------------------------------ 5. the video bridge
def test_video_bridge_end_to_end(hip):
    """frames -> code ids -> VideoGPT (preset S, frame_size 8, 4 frames) -> generated ids -> frames"""
    import train_videogpt as TV
    _, titok, _ = _tatitok_model()
    titok.train()
    B, Tn, N, K = 2, 4, 8, 64
    videos = (W.uniform(5, "videos", (B, Tn, 3, 32, 32), 0.5) + 0.5).cuda()
    tokens = TV.frames_to_tokens(titok, videos)
    assert tokens.shape == (B, Tn, N) and tokens.dtype == torch.int64 and not tokens.requires_grad and titok.training
    assert int(tokens.min()) >= 0 and int(tokens.max()) < K
    titok.eval()
    with torch.no_grad():
        direct = titok.encode(videos[1])[1]["min_encoding_indices"]                  # the four frames of video 1
    assert torch.equal(tokens[1], direct.squeeze(1))
    frames = TV.tokens_to_frames(titok, tokens.reshape(B, Tn * N), Tn)
    assert frames.shape == (B, Tn, 3, 32, 32) and float(frames.min()) >= 0.0 and float(frames.max()) <= 1.0
    with torch.no_grad():
        want = torch.clamp(titok.decode_tokens(tokens[1]), 0.0, 1.0)
    assert torch.equal(frames[1], want)
    torch.manual_seed(0)
    gpt = TV.VideoGPT(TV.VideoGPTConfig(N, K, "S", Tn, 0.0)).cuda()
    loss = TV.train_step(gpt, tokens, torch.optim.AdamW(gpt.parameters(), lr=1e-4))
    assert bool(torch.isfinite(loss))
    gpt.eval()
    gen = gpt.generate_frames(tokens[:, :1], n=Tn - 1)
    assert gen.shape == (B, Tn * N) and torch.equal(gen[:, :N], tokens[:, 0]) and int(gen.max()) < K
    out = TV.tokens_to_frames(titok, gen, Tn)
    assert out.shape == (B, Tn, 3, 32, 32) and bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    assert torch.equal(out[:, 0], frames[:, 0])                                       # the conditioning frame decodes as before
