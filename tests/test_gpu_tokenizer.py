"""The tokenizer training path on the GPU: the quantiser and reconstruction-loss kernels (csrc/tokenizer.hip) against the float64
restatement of tests/_tokenizer_ref.py, vitamd.tokenizer on top of them, TiTok.loss / ViTVQGAN.loss and train_step against the goldens
and the present route.

Bounds (tests/_tokenizer_ref.py), all measured against float64, never against the kernel's own output: every fp32 result within
max(4 e32, 8 * 2^-24) of the reference on the scale max(1, |ref|), e32 being the same distance for torch's fp32 CPU evaluation at that
shape; gradients that carry 1 / (element count) are brought to order one first; the bf16 gradient within half a bf16 ulp (+1/16) on top;
dcodebook n_k 2^-24 sum|terms| on top for the order of its sums.  Ids equal the reference's wherever its best and second-best squared
distances are 1e-5 or more apart."""
import functools

import pytest
import torch

import _tokenizer_ref as R
import vit_oracle as O

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


@functools.lru_cache(maxsize=None)
def _vq_case(i):
    M, K, d = R.VQ_SHAPES[i]
    x, cb, g_q = R.vq_inputs(M, K, d, R.vq_seed(i))
    return x, cb, g_q, R.vq_ref(x, cb, g_q, R.G_LOSS)


def _run_quantiser(x, cb, g_q, g_loss):
    from vitamd import ops
    xd, cbd = x.cuda(), cb.cuda()
    unit, rnorm, q, idx, loss, eunit = ops.vq_quantize_fwd(xd, cbd, return_unit_codes=True)
    eunit = eunit.clone()
    gl = None if g_loss is None else torch.tensor(g_loss, device="cuda")
    dx, dcb = ops.vq_quantize_bwd(None if g_q is None else g_q.cuda(), gl, unit, rnorm, idx, cbd)
    return {"unit": unit, "rnorm": rnorm, "q": q, "idx": idx, "loss": loss, "eunit": eunit, "dx": dx, "dcb": dcb}


def _against_float64(dev, x, cb, g_q, g_loss, ref0, label):
    """ids by the near-tie rule, then every float result against the reference taken at the ids the kernel used on exempt rows"""
    got = {k: v.cpu() for k, v in dev.items()}
    fails, exempt = R.check_ids(got["idx"], ref0, label)
    assert int(got["idx"].min()) >= 0 and int(got["idx"].max()) < cb.shape[0]
    use = torch.where(exempt, got["idx"], ref0["idx_ref"])
    ref = ref0 if torch.equal(use, ref0["idx"]) else R.vq_ref(x, cb, g_q, 0.0 if g_loss is None else g_loss, idx=use)
    gq = torch.zeros_like(x) if g_q is None else g_q
    t32 = R.vq_torch(x, cb, use, gq, 0.0 if g_loss is None else g_loss)
    fails += R.check_vq(got, ref, t32, label)
    rn = R._dist(got["rnorm"], ref["rnorm"], ref["rnorm"].abs())
    print(f"{label} rnorm: {rn:.3e} relative")
    if not rn <= R.FLOOR:
        fails.append(f"{label} rnorm: {rn:.3e}")
    return fails, ref


# ------------------------------------------------------------------------------------------------ 1. quantiser shapes
@pytest.mark.parametrize("i", range(len(R.VQ_SHAPES)))
def test_quantiser_kernels_match_float64(hip, i):
    from vitamd import ops
    x, cb, g_q, ref0 = _vq_case(i)
    dev = _run_quantiser(x, cb, g_q, R.G_LOSS)
    fails, _ = _against_float64(dev, x, cb, g_q, R.G_LOSS, ref0, f"case {R.VQ_SHAPES[i]}")
    assert not fails, fails
    # the search is vq_nearest's, bit for bit, on the kernel's own unit rows and unit codebook
    assert torch.equal(dev["idx"], ops.vq_nearest(dev["unit"], dev["eunit"].contiguous()))
    # forward: the same bits on a second call (fixed-order loss sum, order-free atomicMin)
    again = _run_quantiser(x, cb, g_q, R.G_LOSS)
    for k in ("unit", "rnorm", "q", "loss", "dx"):
        assert torch.equal(dev[k].view(torch.int32), again[k].view(torch.int32)), k
    assert torch.equal(dev["idx"], again["idx"])


# ------------------------------------------------------------------------------------------------ 2. special rows
def test_quantiser_duplicates_zero_rows_and_absent_gradients(hip):
    """300 rows over 9 codes (every 256-row block shares codes: the on-chip sums and the cross-block atomics both run); code 7 repeats
    code 2 and row 5 points at both: the lower index wins; a zero input row and a zero code row stay finite, the zero row's dx is du/eps"""
    x, cb, g_q = R.vq_inputs(300, 9, 5, 7)
    x[3] = 0
    cb[4] = 0
    cb[7] = cb[2]
    x[5] = cb[2] * 1000
    ref0 = R.vq_ref(x, cb, g_q, R.G_LOSS)
    dev = _run_quantiser(x, cb, g_q, R.G_LOSS)
    for k in ("unit", "rnorm", "q", "loss", "dx", "dcb"):
        assert bool(torch.isfinite(dev[k]).all()), k
    assert int(dev["idx"][5]) == 2 and int(ref0["idx_ref"][5]) == 2
    assert int(dev["idx"][3]) == 4 == int(ref0["idx_ref"][3])                       # |0 - 0|^2 = 0 against 1 for every unit code
    assert float(dev["rnorm"][3]) == float(torch.tensor(1.0) / torch.tensor(1e-12)) and bool((dev["unit"][3] == 0).all())
    # code 7 is code 2 bit for bit, so every row nearest to it is an EXACT tie (gap 0) that the first-minimum rule decides: those rows are
    # held to the reference's id here, and the near-tie rule (at most 1 % exempt) to the rows with 0 < gap < 1e-5
    tie = ref0["gap"] == 0
    assert int(tie.sum()) > 1 and torch.equal(dev["idx"].cpu()[tie], ref0["idx_ref"][tie]) and bool((ref0["idx_ref"][tie] == 2).all())
    held = dict(ref0, gap=torch.where(tie, torch.full_like(ref0["gap"], float("inf")), ref0["gap"]))
    fails, ref = _against_float64(dev, x, cb, g_q, R.G_LOSS, held, "special rows")
    assert not fails, fails
    p = cb[4].double()
    assert torch.allclose(dev["dx"][3].cpu().double(), (g_q[3].double() - 0.5 * R.G_LOSS * p / 1500) / R.EPS, rtol=1e-6)
    # no gradient into q: dx is the commitment term alone; no gradient into the loss: dcodebook stays zero, dx is the straight-through one
    for g_q_, g_loss_ in ((None, R.G_LOSS), (g_q, None)):
        d2 = _run_quantiser(x, cb, g_q_, g_loss_)
        r2 = R.vq_ref(x, cb, g_q_, 0.0 if g_loss_ is None else g_loss_)
        r2["gap"] = held["gap"]
        f2, _ = _against_float64(d2, x, cb, g_q_, g_loss_, r2, f"g_q {g_q_ is not None} g_loss {g_loss_}")
        assert not f2, f2
        if g_loss_ is None:
            assert bool((d2["dcb"] == 0).all())


# ------------------------------------------------------------------------------------------------ 3. reconstruction shapes
@functools.lru_cache(maxsize=None)
def _recon_case(i, dtype):
    B, G, p, c = R.RECON_SHAPES[i]
    y, img = R.recon_inputs(B, G, p, c, 300 + i, dtype)
    return y, img, R.recon_ref(y, img, G, p, R.G_UP), R.recon_torch(y, img, G, p, R.G_UP)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("i", range(len(R.RECON_SHAPES)))
def test_reconstruction_kernels_match_float64(hip, i, dtype):
    """tokens as a view of a wider buffer whose pad columns hold NaN; backward into a second padded buffer and in place"""
    from vitamd import ops
    B, G, p, c = R.RECON_SHAPES[i]
    y, img, ref, t32 = _recon_case(i, dtype)
    M, F = y.shape
    ld = F + 8
    buf = torch.full((M, ld), float("nan"), dtype=dtype)
    buf[:, :F] = y
    bufd, imgd = buf.cuda(), img.cuda()
    tok = bufd[:, :F]
    gup = torch.tensor(R.G_UP, device="cuda")
    loss = ops.recon_mse_fwd(tok, imgd, G, p)
    loss2 = ops.recon_mse_fwd(tok, imgd, G, p)
    SENT = 7.0
    obuf = torch.full((M, ld), SENT, dtype=dtype, device="cuda")
    dy = ops.recon_mse_bwd(tok, imgd, G, p, gup, out=obuf[:, :F])
    dense = ops.recon_mse_bwd(tok, imgd, G, p, gup)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32))                                # fixed-order sum
    assert dense.dtype == dtype and dense.is_contiguous() and torch.equal(dense, dy)
    assert bool(torch.isnan(bufd[:, F:]).all()) and torch.equal(bufd[:, :F].cpu(), y) and bool((obuf[:, F:] == SENT).all())
    label = f"case {R.RECON_SHAPES[i]} {dtype}"
    fails = R.check_recon({"loss": loss.cpu()}, ref, t32, label)
    if dtype == F32:
        fails += R.check_recon({"dy": dy.cpu()}, ref, t32, label)
    else:
        fails += R.check_recon_bf16(dy.cpu(), ref, t32, label)
    assert not fails, fails
    # in place: the same bits, the pad columns still NaN
    inplace = ops.recon_mse_bwd(tok, imgd, G, p, gup, out=tok)
    assert inplace.data_ptr() == tok.data_ptr() and torch.equal(tok, dy) and bool(torch.isnan(bufd[:, F:]).all())
    # no upstream gradient = 1
    one = ops.recon_mse_bwd(y.cuda(), imgd, G, p, None)
    ref1 = R.recon_ref(y, img, G, p, 1.0)
    t321 = R.recon_torch(y, img, G, p, 1.0)
    f1 = R.check_recon({"dy": one.cpu()}, ref1, t321, label) if dtype == F32 else R.check_recon_bf16(one.cpu(), ref1, t321, label)
    assert not f1, f1


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_reconstruction_refuses_what_its_16_byte_path_cannot_take(hip, dtype):
    """an unaligned base and a token width of 10: the kernels refuse, tokenizer.recon_mse takes the torch expressions and is still right"""
    from vitamd import ops, tokenizer
    from vitamd.lib import VitamdError
    B, G, p, c = R.RECON_SHAPES[0]
    y, img, ref, t32 = _recon_case(0, dtype)
    M, F = y.shape
    buf = torch.zeros((M, F + 8), dtype=dtype, device="cuda")
    buf[:, 1:F + 1] = y.cuda()
    tok = buf[:, 1:F + 1]
    assert tok.data_ptr() % 16 != 0 and not ops.recon_mse_applies(tok)
    with pytest.raises(VitamdError):
        ops.recon_mse_fwd(tok, img.cuda(), G, p)
    with pytest.raises(VitamdError):
        ops.recon_mse_bwd(tok, img.cuda(), G, p)
    with pytest.raises(VitamdError):
        ops.recon_mse_bwd(y.cuda(), img.cuda(), G, p, out=tok)
    t = tok.detach().requires_grad_(True)
    loss = tokenizer.recon_mse(t, img.cuda(), G, p)
    (loss * R.G_UP).backward()
    got = {"loss": loss.detach().cpu(), "dy": t.grad.float().cpu()}
    if dtype == F32:
        assert R.check_recon(got, ref, t32, "fallback") == []
    else:
        assert R.check_recon({"loss": got["loss"]}, ref, t32, "fallback") == [] and R.check_recon_bf16(got["dy"], ref, t32, "fallback") == []
    y10 = torch.randn(2 * 4, 10, device="cuda").to(dtype)                            # p = 1, c = 10
    img10 = torch.rand(2, 10, 2, 2, device="cuda")
    with pytest.raises(VitamdError):
        ops.recon_mse_fwd(y10, img10, 2, 1)
    want = torch.nn.functional.mse_loss(R.pixel_shuffle(y10.float(), 2, 2, 1, 10), img10)
    assert abs(float(tokenizer.recon_mse(y10, img10, 2, 1)) - float(want)) <= 1e-6 * float(want)


# ------------------------------------------------------------------------------------------------ 4. vitamd.tokenizer
def test_vq_quantize_matches_the_present_quantiser(hip):
    """the autograd function on a [2, 150, 12] input against train_titok.Quantizer.forward on the same device tensors, and the wide-code
    fallback (d = 80) against the same expressions"""
    import train_titok as TT
    from vitamd import tokenizer
    for d, K in ((12, 513), (80, 40)):
        x, cb, g_q = R.vq_inputs(300, K, d, 50 + d)
        quant = TT.Quantizer(type("C", (), {"codebook_size": K, "latent_dim": d})).cuda()
        with torch.no_grad():
            quant.codebook.weight.copy_(cb)
        xa = x.view(2, 150, d).cuda().requires_grad_(True)
        q0, ids0, l0 = quant(xa)
        ((q0 * g_q.view(2, 150, d).cuda()).sum() + l0 * R.G_LOSS).backward()
        want = (q0.detach(), ids0, l0.detach(), xa.grad.clone(), quant.codebook.weight.grad.clone())
        xb = x.view(2, 150, d).cuda().requires_grad_(True)
        quant.codebook.weight.grad = None
        q1, ids1, l1 = tokenizer.vq_quantize(xb, quant.codebook.weight)
        assert q1.shape == (2, 150, d) and ids1.shape == (2, 150) and ids1.dtype == torch.int64 and l1.dim() == 0 and not ids1.requires_grad
        ((q1 * g_q.view(2, 150, d).cuda()).sum() + l1 * R.G_LOSS).backward()
        got = (q1.detach(), ids1, l1.detach(), xb.grad, quant.codebook.weight.grad)
        ref = R.vq_ref(x, cb, g_q, R.G_LOSS)
        fails, _ = R.check_ids(ids1.cpu().view(-1), ref, f"d={d}")
        assert not fails, fails
        assert torch.equal(got[1], want[1])
        # two fp32 evaluations, each allowed max(4 e32, floor) from float64: at most twice that apart
        t32 = R.vq_torch(x, cb, ref["idx"], g_q, R.G_LOSS)
        e32 = R.vq_errors(t32, ref)
        for name, a, b, scale in (("q", got[0], want[0], 1.0), ("loss", got[2], want[2], 1.0), ("dx", got[3], want[3], 1.0),
                                  ("dcb", got[4], want[4], 300 * d)):
            a, b = a.double().cpu().reshape(-1) * scale, b.double().cpu().reshape(-1) * scale
            allow = 2 * R.bound(e32[name]) * b.abs().clamp_min(1.0)
            if name == "dcb":
                allow = allow + 2 * (ref["n_k"][:, None] * 2.0 ** -24 * ref["terms_abs"]).reshape(-1) * scale
            worst = float(((a - b).abs() / allow).max())
            print(f"d={d} {name}: worst |new - present| / allowance {worst:.3f}")
            assert worst <= 1.0, (d, name, worst)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_recon_mse_autograd(hip, dtype):
    from vitamd import tokenizer
    B, G, p, c = R.RECON_SHAPES[1]
    y, img, ref, t32 = _recon_case(1, dtype)
    t = y.view(B, G * G, -1).cuda().requires_grad_(True)
    loss = tokenizer.recon_mse(t, img.cuda(), G, p)
    assert loss.dim() == 0 and loss.dtype == F32
    (loss * R.G_UP).backward()
    assert t.grad.dtype == dtype and t.grad.shape == t.shape
    g = t.grad.cpu().view(B * G * G, -1)
    fails = R.check_recon({"loss": loss.detach().cpu()}, ref, t32, "recon_mse")
    fails += R.check_recon({"dy": g}, ref, t32, "recon_mse") if dtype == F32 else R.check_recon_bf16(g, ref, t32, "recon_mse")
    assert not fails, fails


@pytest.mark.parametrize("F_D, fused", [((64, 64), True), ((48, 64), False)])
def test_linear_recon_mse_matches_the_present_head(hip, F_D, fused):
    """head + loss against functions.linear + pixel_shuffle_tokens + mse_loss on the same device tensors, with a 1x1-conv weight as the
    decoders hold it; the fused form refuses a second backward"""
    import train_titok as TT
    from vitamd import tokenizer
    F, D = F_D
    B, G, p, c = (2, 4, 8, 1) if F == 64 else (2, 4, 4, 3)
    assert tokenizer.fused_head_applies(F, D) == fused
    g = torch.Generator().manual_seed(9)
    h = torch.randn(B, G * G, D, generator=g)
    img = torch.rand(B, c, G * p, G * p, generator=g)
    conv = TT.HipConv1x1(D, F, kernel_size=1).cuda()
    ha = h.cuda().requires_grad_(True)
    want = torch.nn.functional.mse_loss(TT.pixel_shuffle_tokens(conv(ha), G, p), img.cuda())
    (want * R.G_UP).backward()
    ref_g = (ha.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone())
    conv.zero_grad(set_to_none=True)
    hb = h.cuda().requires_grad_(True)
    loss = tokenizer.linear_recon_mse(hb, conv.weight, conv.bias, img.cuda(), G, p)
    assert loss.dim() == 0 and loss.dtype == F32
    (loss * R.G_UP).backward(retain_graph=fused)
    if fused:
        with pytest.raises(RuntimeError):
            loss.backward()
    # both routes round the tokens to bf16 once (2^-9 relative, on values of order one, averaged over F*B*G*G elements in the loss) and the
    # token gradient to bf16 once more: the loss within 2^-9 relative, every gradient tensor within 2 * 2^-8 in relative L2
    assert abs(float(loss.detach()) - float(want.detach())) <= 2.0 ** -9 * float(want.detach())
    assert conv.weight.grad.shape == conv.weight.shape
    for name, a, b in zip(("dh", "dW", "db"), (hb.grad, conv.weight.grad, conv.bias.grad), ref_g):
        e = O.rel_l2(a.cpu(), b.cpu())
        print(f"{name}: rel L2 new vs present {e:.3e}")
        assert e <= 2 * 2.0 ** -8, (name, e)


# ------------------------------------------------------------------------------------------------ 5. the models
@pytest.mark.parametrize("name", ["titok_s256.pt", "vitvqgan_b256.pt"])
def test_model_loss_route_matches_golden_and_present_route(hip, name):
    """the bounds of test_gpu_parity.py::test_tokenizer_vs_reference_golden on the new route, then the new route against the present one"""
    from test_gpu_parity import _err, _tokenizer_model
    g, m, enc, images = _tokenizer_model(name)
    floor = g["ref_bf16_floor"]
    recon, idx, qloss = m(images)
    loss0 = torch.nn.functional.mse_loss(recon, images) + qloss
    loss0.backward()
    e_parent = {k: _err(p.grad, g["grads"][k]) for k, p in m.named_parameters()
                if p.grad is not None and g["grads"][k]["norm"] != 0.0 and p.numel() > 0}
    m.zero_grad(set_to_none=True)
    recon_loss, qloss1, ids = m.loss(images)
    assert recon_loss.dim() == 0 and qloss1.dim() == 0 and ids.shape == idx.shape
    assert abs(float(qloss1.detach()) - g["quantize_loss"]) < 2e-3
    loss1 = recon_loss + qloss1
    assert abs(float(loss1.detach()) - g["loss"]) < 5e-3
    loss1.backward(retain_graph=True)
    with pytest.raises(RuntimeError):
        loss1.backward()                         # the tokens were overwritten by their gradient
    torch.cuda.synchronize()
    # against the present route on the same device: the encoder is the same code on the same input, so the latents are the same bits and
    # the search (the same arithmetic on a unit codebook that may differ in its last bit) may only differ on near-ties
    agree = float((ids == idx).float().mean())
    print(f"{name}: ids agree {agree:.5f}, qloss {float(qloss1.detach()):.6f} / {float(qloss.detach()):.6f}, loss {float(loss1.detach()):.6f} / {float(loss0.detach()):.6f}")
    assert agree >= 0.999
    assert abs(float(qloss1.detach()) - float(qloss.detach())) < 1e-5 and abs(float(loss1.detach()) - float(loss0.detach())) < 1e-3
    bad = []
    for k, p in m.named_parameters():
        if k not in e_parent:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        e = _err(p.grad, g["grads"][k])
        print(f"{k}: new {e:.3e} present {e_parent[k]:.3e} floor {floor['grads'][k]:.3e}")
        # the golden's bound, and as close as the present route: both are bf16 flows whose distance from the golden is rounding noise, so a
        # parameter's figure may move by a fraction of itself between routes, never by a multiple
        if e > 2 * floor["grads"][k] + 1e-2 or e > 1.5 * e_parent[k] + 1e-3:
            bad.append((k, round(e, 4), round(e_parent[k], 4), round(floor["grads"][k], 4)))
    assert not bad, bad[:8]


def test_train_step_follows_the_present_route(hip):
    """two steps of train_step against two steps of the present route under torch.optim.AdamW, and a third that has brought the loss down"""
    import train_titok as TT
    from test_gpu_parity import _tokenizer_model
    _, new, _, images = _tokenizer_model("titok_s256.pt")
    _, old, _, _ = _tokenizer_model("titok_s256.pt")
    o_new = torch.optim.AdamW(new.parameters(), lr=1e-4, weight_decay=1e-4)
    o_old = torch.optim.AdamW(old.parameters(), lr=1e-4, weight_decay=1e-4)
    got, ref = [], []
    for _ in range(3):
        loss = TT.train_step(new, images, o_new)
        assert not loss.requires_grad and loss.is_cuda
        got.append(float(loss))
    for _ in range(2):
        o_old.zero_grad(set_to_none=True)
        recon, _, qloss = old(images)
        loss = torch.nn.functional.mse_loss(recon, images) + qloss
        loss.backward()
        o_old.step()
        ref.append(float(loss.detach()))
    print("train_step losses", got, "present route", ref)
    for a, b in zip(got, ref):
        assert abs(a - b) < 3e-2 * max(1.0, abs(b)), (got, ref)          # the bound of the ViT and VideoGPT training-step tests
    assert got[2] < got[0]
    # with a perceptual term the step runs the route that yields the image
    seen = []
    def perceptual(recon, imgs):
        seen.append(tuple(recon.shape))
        return (recon - imgs).abs().mean(dim=(1, 2, 3))
    lp = float(TT.train_step(new, images, o_new, perceptual=perceptual, perceptual_weight=0.5))
    assert seen == [tuple(images.shape)] and lp > got[2] * 0.5
