"""The Enhancing ViT-VQGAN tokenizer on the GPU: the tanh kernels and the L1 pixel tail (csrc/enhancing.hip) against the float64
restatements of tests/_enhancing_ref.py, vitamd.enhancing on top of them, and train_enhancing_vitvqgan.ViTVQGAN against the reference's
golden (tests/golden/enhancing_tiny.pt).

Bounds, none of them taken from the kernels' own output (tests/_enhancing_ref.py has the reasoning): one bf16 ulp on every element of both
tanh kernels; the squared-error loss's bound on the L1 loss; the image exact; one ulp of the tokens' dtype on the tail's gradient and
exactly g_image at the ties; 2 * 2^-8 in relative L2 on tanh_mlp against float64 on the same bf16 operands (the multiple
tests/test_gpu_tatitok.py uses where two routes each round to bf16); 2 x the reference's own bf16-autocast deviation plus the constants of
tests/test_gpu_tatitok.py::test_titok_vs_reference_golden on the model."""
import functools

import pytest
import torch

import _enhancing_ref as E
import vit_oracle as O
import weights as W
from _tokenizer_ref import _dist, bound
from conftest import load_golden

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SWEEP = 2048 * 256 * 8                       # elements one sweep of the tanh kernels' grid-stride loop covers (ops.TANH_SWEEP_ELEMS)
TANH_SIZES = [1, 7, 8, 4099, SWEEP + 4099]
PAD, SENT = 8, 7.0


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. tanh
@functools.lru_cache(maxsize=None)
def _tanh_case(n):
    return E.tanh_values(n, 500 + n % 97)


@functools.lru_cache(maxsize=None)
def _tanh_bwd_case(n):
    return E.tanh_bwd_values(n, 600 + n % 97)


def _placed(values, off, fill=SENT):
    """values inside a longer device buffer, `off` elements behind its (256-byte aligned) start -> (buffer, the view)"""
    buf = torch.full((values.numel() + off + PAD,), fill, dtype=values.dtype, device="cuda")
    view = buf[off:off + values.numel()]
    view.copy_(values)
    return buf, view


@pytest.mark.parametrize("off_in, off_out", [(0, 0), (1, 1), (3, 5)])
@pytest.mark.parametrize("n", TANH_SIZES)
def test_tanh_forward_matches_float64(hip, n, off_in, off_out):
    """(1, 1): the vector body cannot start at the buffer's start; (3, 5): input and output out of phase, element by element throughout"""
    from vitamd import ops
    assert ops.TANH_SWEEP_ELEMS == SWEEP
    x, _ = _tanh_case(n)
    ibuf, xin = _placed(x, off_in)
    obuf, out = _placed(torch.zeros(n, dtype=BF16), off_out)
    obuf.fill_(SENT)
    assert off_in == 0 or xin.data_ptr() % 16 != 0
    got = ops.tanh_bf16(xin, out=out)
    assert got.data_ptr() == out.data_ptr()
    fails = E.check_tanh(got.cpu(), x, f"n {n} offsets {off_in}/{off_out}")
    assert not fails, fails
    assert bool((obuf[:off_out] == SENT).all()) and bool((obuf[off_out + n:] == SENT).all())      # nothing outside the n elements
    assert torch.equal(xin.cpu().view(torch.int16), x.view(torch.int16))                           # the input is as it was
    fresh = ops.tanh_bf16(xin)
    assert fresh.is_contiguous() and _same_bits(fresh, got)
    ops.tanh_bf16(xin, out=xin)                                                                    # in place
    assert _same_bits(xin, got)
    assert bool((ibuf[:off_in] == SENT).all()) and bool((ibuf[off_in + n:] == SENT).all())


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", TANH_SIZES)
def test_tanh_backward_matches_float64(hip, n, off):
    from vitamd import ops
    dh, t, _ = _tanh_bwd_case(n)
    dbuf, dhin = _placed(dh, off)
    _, tin = _placed(t, off)
    got = ops.tanh_bwd_bf16(dhin, tin)
    fails = E.check_tanh_bwd(got.cpu(), dh, t, f"n {n} offset {off}")
    assert not fails, fails
    assert torch.equal(tin.cpu().view(torch.int16), t.view(torch.int16)) and torch.equal(dhin.cpu().view(torch.int16), dh.view(torch.int16))
    ops.tanh_bwd_bf16(dhin, tin, out=dhin)                                                         # in place on dh
    assert _same_bits(dhin, got)
    assert bool((dbuf[:off] == SENT).all()) and bool((dbuf[off + n:] == SENT).all())
    if n == 4099:                                                                                  # t out of phase with dh: element by element
        _, t2 = _placed(t, off + 2)
        assert _same_bits(ops.tanh_bwd_bf16(_placed(dh, off)[1], t2), got)


# ------------------------------------------------------------------------------------------------ 2. the L1 tail
@functools.lru_cache(maxsize=None)
def _l1_case(B, G, p, c, dtype, with_g):
    y, img, g_img, tie = E.l1_inputs(B, G, p, c, 700 + 10 * p + G, dtype)
    g_loss = E.G_LOSS if with_g else 1.0
    gi = g_img if with_g else None
    return y, img, gi, tie, E.l1_ref(y, img, G, p, g_loss, gi), E.l1_torch(y, img, G, p)


@pytest.mark.parametrize("with_g", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", E.L1_SHAPES + [(3, 3, 2, 3)])
def test_l1_tail_kernels_match_float64(hip, shape, dtype, with_g):
    """tokens as a view of a wider buffer whose pad columns hold NaN; with_g: the upstream gradients of the loss (2.5) and of the image
    given, else absent (1 and 0); the same bits twice; in place.  (3, 3, 2, 3): a patch of 2, fp32 only here - its 12-feature bf16 row is
    not whole 16-byte pieces, the kernel refuses it and vitamd.enhancing.recon_l1 takes the torch expressions (the next test)."""
    from vitamd import ops
    from vitamd.lib import VitamdError
    B, G, p, c = shape
    y, img, g_img, tie, ref, t32 = _l1_case(B, G, p, c, dtype, with_g)
    M, F = y.shape
    buf = torch.full((M, F + PAD), float("nan"), dtype=dtype)
    buf[:, :F] = y
    bufd, imgd = buf.cuda(), img.cuda()
    tok = bufd[:, :F]
    if p == 2 and dtype == BF16:
        assert not ops.recon_l1_applies(tok)
        with pytest.raises(VitamdError):
            ops.recon_l1_fwd(tok, imgd, G, p)
        with pytest.raises(VitamdError):
            ops.recon_l1_bwd(tok, imgd, G, p)
        return
    assert ops.recon_l1_applies(tok)
    gl = torch.tensor(E.G_LOSS, device="cuda") if with_g else None
    gi = g_img.cuda() if with_g else None
    loss, recon = ops.recon_l1_fwd(tok, imgd, G, p, want_recon=True)
    loss2, none = ops.recon_l1_fwd(tok, imgd, G, p)
    loss3, recon3 = ops.recon_l1_fwd(tok, imgd, G, p, want_recon=True)
    assert none is None and loss.dim() == 0 and _same_bits(loss, loss2) and _same_bits(loss, loss3) and _same_bits(recon, recon3)
    dy = ops.recon_l1_bwd(tok, imgd, G, p, gl, gi)
    assert dy.is_contiguous() and dy.shape == (M, F)
    assert bool(torch.isnan(bufd[:, F:]).all()) and torch.equal(bufd[:, :F].cpu(), y)              # the tokens and their pads are as they were
    label = f"case {shape} {dtype} g {with_g}"
    fails = E.check_l1({"loss": loss.cpu(), "recon": recon.cpu(), "dy": dy.cpu()}, ref, t32, tie, g_img, dtype, label)
    assert not fails, fails
    obuf = torch.full((M, F + 2 * PAD), SENT, dtype=dtype, device="cuda")
    dy2 = ops.recon_l1_bwd(tok, imgd, G, p, gl, gi, out=obuf[:, :F])
    assert dy2.data_ptr() == obuf.data_ptr() and _same_bits(dy2, dy) and bool((obuf[:, F:] == SENT).all())
    ops.recon_l1_bwd(tok, imgd, G, p, gl, gi, out=tok)                                             # in place
    assert _same_bits(tok, dy) and bool(torch.isnan(bufd[:, F:]).all())


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_recon_l1_with_a_patch_of_two(hip, dtype):
    """12 features a token: fp32 rows are whole 16-byte pieces (the kernel, pixel by pixel), bf16 rows are not (the torch expressions);
    either way loss, image and gradient are right, with both outputs carrying a gradient"""
    from vitamd import enhancing
    B, G, p, c = 3, 3, 2, 3
    y, img, g_img, tie, ref, t32 = _l1_case(B, G, p, c, dtype, True)
    t = y.cuda().view(B, G * G, -1).requires_grad_(True)
    loss, recon = enhancing.recon_l1(t, img.cuda(), G, p, return_recon=True)
    assert ("ReconL1Fn" in type(loss.grad_fn).__name__) == (dtype == F32)
    (loss * E.G_LOSS + (recon * g_img.cuda()).sum()).backward()
    got = {"loss": loss.detach().cpu(), "recon": recon.detach().cpu(), "dy": t.grad.cpu().view(B * G * G, -1)}
    fails = E.check_l1(got, ref, t32, tie, g_img, dtype, f"patch 2 {dtype}")
    assert not fails, fails
    only = enhancing.recon_l1(t.detach(), img.cuda(), G, p)
    assert only.dim() == 0 and abs(float(only) - float(loss.detach())) <= 2.0 ** -22


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_l1_tail_feature_order_is_c_p1_p2(hip, dtype):
    """every feature holds its own index (exact in bf16 up to 255): the image must show ch*p*p + p1*p + p2 at (ch, gh*p + p1, gw*p + p2), and
    an image that lies above the tokens in channel 0, below in channel 1 and on them in channel 2 must give -g/N, +g/N and 0 by feature"""
    from vitamd import ops
    B, G, p, c = 2, 2, 8, 3
    F, H = c * p * p, G * p
    y = torch.arange(F, dtype=F32).repeat(B * G * G, 1).to(dtype)
    ch = torch.arange(c).view(1, c, 1, 1)
    h = torch.arange(H).view(1, 1, H, 1)
    w = torch.arange(H).view(1, 1, 1, H)
    want = (ch * p * p + (h % p) * p + (w % p)).expand(B, c, H, H).to(F32)
    img = (want + torch.tensor([1.0, -1.0, 0.0]).view(1, c, 1, 1)).contiguous()
    loss, recon = ops.recon_l1_fwd(y.cuda(), img.cuda(), G, p, want_recon=True)
    assert torch.equal(recon.cpu(), want)
    assert abs(float(loss) - 2.0 / 3.0) <= 2.0 ** -22
    dy = ops.recon_l1_bwd(y.cuda(), img.cuda(), G, p).cpu()
    step = torch.tensor(1.0 / img.numel(), dtype=F64).to(F32).to(dtype)
    by_feature = torch.cat([-step.expand(p * p), step.expand(p * p), torch.zeros(p * p, dtype=dtype)])
    assert torch.equal(dy.float(), by_feature.float().repeat(B * G * G, 1))


# ------------------------------------------------------------------------------------------------ 3. autograd
@pytest.mark.parametrize("M", [5, 200])
def test_tanh_mlp_matches_float64_on_the_same_operands(hip, M):
    """output and the five gradients against float64 on the bf16-rounded x, weights and upstream gradient; the hidden activations and
    their gradient are each rounded to bf16 once on the way: 2 * 2^-8 in relative L2"""
    from vitamd import enhancing
    dim, hid = 128, 256
    g = torch.Generator().manual_seed(40 + M)
    rb = lambda t: t.to(BF16).to(F32)
    x, dy = rb(torch.randn(M, dim, generator=g)), rb(torch.randn(M, dim, generator=g))
    w1, w2 = rb(torch.randn(hid, dim, generator=g) * dim ** -0.5), rb(torch.randn(dim, hid, generator=g) * hid ** -0.5)
    b1, b2 = rb(torch.randn(hid, generator=g) * 0.1), rb(torch.randn(dim, generator=g) * 0.1)
    ref = E.tanh_mlp_ref(x, w1, b1, w2, b2, dy)
    dev = [t.cuda().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    y = enhancing.tanh_mlp(*dev)
    assert y.shape == (M, dim) and y.dtype == F32 and "TanhMlpFn" in type(y.grad_fn).__name__
    y.backward(dy.cuda())
    worst = 0.0
    for name, got in zip(("y", "dx", "dw1", "db1", "dw2", "db2"), [y.detach()] + [t.grad for t in dev]):
        e = O.rel_l2(got.cpu(), ref[name].float())
        worst = max(worst, e / 2.0 ** -8)
        print(f"M {M} {name}: rel L2 {e:.3e} = {e / 2.0 ** -8:.3f} x 2^-8")
        assert e <= 2 * 2.0 ** -8, (name, e)
    print(f"M {M}: worst ratio to 2^-8: {worst:.3f} (bound 2)")
    # a leading shape, and the same bits on a second call
    y3 = enhancing.tanh_mlp(x.cuda().view(1, M, dim), *[t.detach() for t in dev[1:]])
    assert y3.shape == (1, M, dim) and torch.equal(y3.view(M, dim), y.detach())


@pytest.mark.parametrize("F_D_p, fused", [((192, 64, 8), True), ((48, 64, 4), False)])
@pytest.mark.parametrize("with_recon", [False, True])
def test_linear_recon_l1_matches_the_unfused_route(hip, F_D_p, fused, with_recon):
    """the ConvTranspose2d head + L1 tail against functions.linear on the transposed weight + the (c p1 p2) shuffle + abs().mean() on the
    same device tensors; with_recon: (recon * dy).sum() added to the loss; the fused form refuses a second backward.  Both routes round
    the tokens to bf16 once and their gradient once more: the bounds of the squared-error tail's test of this kind."""
    from vitamd import enhancing, tokenizer
    from vitamd.functions import linear
    F, D, p = F_D_p
    B, G, c = 2, 3, 3
    assert tokenizer.fused_head_applies(F, D) == fused and F == c * p * p
    g = torch.Generator().manual_seed(23)
    h = torch.randn(B, G * G, D, generator=g)
    img = torch.rand(B, c, G * p, G * p, generator=g)
    dy = torch.randn(B, c, G * p, G * p, generator=g) / img.numel()
    torch.manual_seed(4)
    convt = torch.nn.ConvTranspose2d(D, c, kernel_size=p, stride=p).cuda()
    params = [convt.weight, convt.bias]
    ha = h.cuda().requires_grad_(True)
    y = linear(ha, convt.weight.reshape(D, F).t(), convt.bias.repeat_interleave(p * p))
    recon0 = enhancing.conv_shuffle_tokens(y, G, p)
    want = (recon0 - img.cuda()).abs().mean()
    (want * E.G_LOSS + ((recon0 * dy.cuda()).sum() if with_recon else 0)).backward()
    ref_g = [ha.grad.clone()] + [q.grad.clone() for q in params]
    for q in params:
        q.grad = None
    hb = h.cuda().requires_grad_(True)
    out = enhancing.linear_recon_l1(hb, convt.weight, convt.bias, img.cuda(), G, p, return_recon=with_recon)
    loss, recon = out if with_recon else (out, None)
    assert loss.dim() == 0 and loss.dtype == F32 and (recon is None or (recon.shape == img.shape and recon.requires_grad))
    assert ("LinearReconL1Fn" in type(loss.grad_fn).__name__) == fused
    total = loss * E.G_LOSS + ((recon * dy.cuda()).sum() if with_recon else 0)
    total.backward(retain_graph=fused)
    if fused:
        with pytest.raises(RuntimeError):
            total.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 2.0 ** -9 * float(want.detach())
    if with_recon:
        assert O.rel_l2(recon.detach().cpu(), recon0.detach().cpu()) <= 2.0 ** -8
    assert convt.weight.grad.shape == convt.weight.shape and convt.bias.grad.shape == (c,)
    for name, a, b_ in zip(("dh", "dconvt_w", "dconvt_b"), [hb.grad] + [q.grad for q in params], ref_g):
        e = O.rel_l2(a.cpu(), b_.cpu())
        print(f"{name}: rel L2 fused vs unfused {e:.3e}")
        assert e <= 2 * 2.0 ** -8, (name, e)


# ------------------------------------------------------------------------------------------------ 4. the model
def _model():
    import train_enhancing_vitvqgan as EV
    g = load_golden("enhancing_tiny.pt")
    c = g["cfg"]
    cfg = EV.ViTVQGANConfig(c["image_size"], c["patch_size"], c["codebook_size"], c["latent_dim"], c["transformer"])
    m = EV.ViTVQGAN(cfg, dim=c["dim"], depth=c["depth"], heads=c["heads"], mlp_dim=c["mlp_dim"])
    assert sorted(m.state_dict().keys()) == g["state_keys"]
    sd = W.module_state(c["seed"], {k: v for k, v in g["state_shapes"].items() if k not in g["fixed_keys"]})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert sorted(missing) == sorted(g["fixed_keys"]) and not unexpected
    images = W.uniform(c["seed"], "images", (c["batch"], 3, c["image_size"], c["image_size"]), 0.5) + 0.5
    return EV, g, m.cuda(), images.cuda()


def _gerr(got, ref, stride):
    """rel-L2 against a summarised gradient: the full tensor when the fixture holds it, else its every-`stride`-th element"""
    got = got.detach().float().cpu()
    return O.rel_l2(got, ref["full"]) if "full" in ref else O.rel_l2(got.flatten()[::stride].clone(), ref["sample"])


def test_forward_vs_reference_golden(hip):
    """the bounds of tests/test_gpu_tatitok.py::test_titok_vs_reference_golden: 2 x the reference's own bf16-autocast deviation + 3e-3 on
    the reconstruction (and the latents), 2e-3 / 5e-3 absolute on the quantiser loss / the losses, 2 x + 1e-2 on every gradient.
    Indices: compared where the fixture's margin between best and second-best code exceeds 4 x the largest move of a unit latent under
    the reference's own bf16 run (tools/gen_enhancing_golden.py has the argument); that rule leaves out at most 25 % of the tokens."""
    from test_gpu_parity import _err
    EV, g, m, images = _model()
    floor = g["ref_bf16_floor"]
    with torch.no_grad():
        z = m._latents(images)
    e_lat = O.rel_l2(z.cpu(), g["latents"])
    unit = lambda t: torch.nn.functional.normalize(t.double(), dim=-1)
    moved = float((unit(z.cpu()) - unit(g["latents"])).norm(dim=-1).max())
    print(f"latents rel L2 {e_lat:.3e} (floor {floor['latents']:.3e}); largest unit-latent move {moved:.3e} = {moved / floor['unit_dev']:.2f} x the reference's bf16 run")
    assert e_lat < 2 * floor["latents"] + 3e-3
    recon, ids, qloss = m(images)
    assert recon.shape == images.shape and ids.shape == g["indices"].shape and ids.dtype == torch.int64 and qloss.dim() == 0
    compared = g["index_margin"] > 4 * floor["unit_dev"]
    left_out = 1.0 - float(compared.float().mean())
    wrong = int((ids.cpu() != g["indices"])[compared].sum())
    print(f"indices: {left_out:.3f} of the tokens left out, {wrong} compared tokens differ, overall agreement {float((ids.cpu() == g['indices']).float().mean()):.3f}")
    assert g["cfg"]["index_share"] == 0.25 and left_out <= 0.25 and wrong == 0
    e_recon = _err(recon.detach(), g["recon"])
    l1 = (recon - images).abs().mean()
    loss = l1 + qloss
    print(f"recon rel L2 {e_recon:.3e} = {e_recon / floor['recon']:.2f} x floor; qloss {float(qloss.detach()):.6f} / {g['quantize_loss']:.6f}; "
          f"l1 {float(l1.detach()):.6f} / {g['l1_loss']:.6f}")
    assert e_recon < 2 * floor["recon"] + 3e-3
    assert abs(float(qloss.detach()) - g["quantize_loss"]) < 2e-3
    assert abs(float(l1.detach()) - g["l1_loss"]) < 5e-3 and abs(float(loss.detach()) - g["loss"]) < 5e-3
    loss.backward()
    torch.cuda.synchronize()
    bad, worst = [], 0.0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None, k
            continue
        ref = g["grads"][k]
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if ref["norm"] == 0.0:
            continue
        e = _gerr(p.grad, ref, g["grad_stride"])
        worst = max(worst, e / (2 * floor["grads"][k] + 1e-2))
        if e > 2 * floor["grads"][k] + 1e-2:
            bad.append((k, round(e, 4), round(floor["grads"][k], 4)))
    print(f"gradients: worst error / bound {worst:.3f}")
    assert not bad, bad[:8]


def test_loss_route_matches_forward_and_the_golden(hip):
    """loss() against forward(): the fused tail's recon loss is mean |recon - x| of forward()'s (bf16-valued) reconstruction within the L1
    kernel's loss bound; ids and the quantiser loss are the same; the gradients hold the golden's bounds; return_recon yields forward()'s image"""
    EV, g, m, images = _model()
    floor = g["ref_bf16_floor"]
    with torch.no_grad():
        recon0, ids0, q0 = m(images)
    assert torch.equal(recon0.to(BF16).float(), recon0)                                  # the head GEMM's bf16 output, as the tail reads it
    ref = (recon0.double() - images.double()).abs().mean().cpu()
    e32 = _dist((recon0 - images).abs().mean().cpu().reshape(1), ref.reshape(1))
    recon_loss, qloss, ids = m.loss(images)
    assert recon_loss.dim() == 0 and "LinearReconL1Fn" in type(recon_loss.grad_fn).__name__
    e = _dist(recon_loss.detach().cpu().reshape(1), ref.reshape(1))
    print(f"fused recon loss vs forward(): {e:.3e} (torch fp32 {e32:.3e}, bound {bound(e32):.3e})")
    assert e <= bound(e32)
    assert torch.equal(ids, ids0) and _same_bits(qloss.detach(), q0)
    loss = recon_loss + qloss
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError):
        loss.backward()
    assert abs(float(loss.detach()) - g["loss"]) < 5e-3
    bad = []
    for k, p in m.named_parameters():
        if not p.requires_grad or g["grads"][k]["norm"] == 0.0:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        e = _gerr(p.grad, g["grads"][k], g["grad_stride"])
        if e > 2 * floor["grads"][k] + 1e-2:
            bad.append((k, round(e, 4), round(floor["grads"][k], 4)))
    assert not bad, bad[:8]
    m.zero_grad(set_to_none=True)
    out = m.loss(images, return_recon=True)
    assert len(out) == 4 and out[3].shape == images.shape and out[3].requires_grad and torch.equal(out[3].detach(), recon0)
    assert _same_bits(out[0].detach(), recon_loss.detach())
    with torch.no_grad():
        assert torch.equal(m.encode(images), ids0)


def test_train_steps_run_and_move_every_trainable_parameter(hip):
    """two steps on seeded images: finite losses, every trainable parameter changed, the position tables bit-identical; a third step with
    a perceptual callable stays on the fused tail"""
    EV, g, m, images = _model()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    optim = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-4)
    losses = []
    for _ in range(2):
        loss = EV.train_step(m, images, optim)
        assert not loss.requires_grad and loss.is_cuda and bool(torch.isfinite(loss))
        losses.append(float(loss))
    print("train_step losses", losses)
    for k, p in m.named_parameters():
        assert bool(torch.isfinite(p).all()), k
        if p.requires_grad:
            assert not torch.equal(p.detach(), before[k]), k
        else:
            assert k in ("encoder.en_pos_embedding", "decoder.de_pos_embedding") and _same_bits(p.detach(), before[k]), k
    seen = []

    def perceptual(recon, imgs):
        seen.append((tuple(recon.shape), type(recon.grad_fn).__name__))
        return (recon - imgs).pow(2).mean(dim=(1, 2, 3))
    lp = EV.train_step(m, images, optim, perceptual=perceptual, perceptual_weight=0.5)
    assert bool(torch.isfinite(lp)) and len(seen) == 1 and seen[0][0] == tuple(images.shape) and "LinearReconL1Fn" in seen[0][1]


def test_frames_inputs_give_the_bits_of_their_images(hip):
    """uint8 vitamd.data.Frames where the sibling tokenizers accept them: forward(), loss() and train_step; pixels in [0, 1] (no table)"""
    from vitamd import data
    EV, g, m, _ = _model()
    gen = torch.Generator().manual_seed(11)
    src = torch.randint(0, 256, (3, 37, 41, 3), generator=gen, dtype=torch.uint8).cuda()
    make = lambda: data.Frames(src, 32)
    images = make().images()
    assert images.shape == (3, 3, 32, 32) and float(images.min()) >= 0.0 and float(images.max()) <= 1.0
    with torch.no_grad():
        for got, want in ((m.loss(make(), return_recon=True), m.loss(images, return_recon=True)), (m(make()), m(images))):
            for a, b in zip(got, want):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    optim = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4)
    seen = []

    def perceptual(recon, imgs):
        seen.append(torch.equal(imgs, images))
        return (recon - imgs).pow(2).mean(dim=(1, 2, 3))
    assert bool(torch.isfinite(EV.train_step(m, make(), optim))) and bool(torch.isfinite(EV.train_step(m, make(), optim, perceptual=perceptual)))
    assert seen == [True]
