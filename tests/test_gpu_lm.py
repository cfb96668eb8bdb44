"""The training path of the causal stack on the GPU: the cross-entropy and token-embedding kernels (csrc/loss.hip) against the float64
restatement of tests/_lm_ref.py, vitamd.lm on top of them, VideoGPT.loss and train_step against the present route.

Bounds (tests/_lm_ref.py), all measured against float64, never against the kernel's own output: per-row loss and lse within
max(4 e32, 8 * 2^-24) * max(1, |lse_ref|), e32 being the same distance for torch's fp32 CPU evaluation at that shape; the mean by the
same rule on max(1, |mean_ref|); the fp32 gradient by the same rule on |got - ref| * count; the bf16 gradient within half a bf16 ulp
(widened by 1/16) of the reference plus the fp32 bound.  No element is excluded from any comparison."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _lm_ref as R
import vit_oracle as O
import weights as W
from conftest import load_golden

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
IGN = -100
G_UP = 2.5          # the upstream gradient of every kernel-level case


def _grid_rows(V):
    from vitamd import ops
    return ops.cross_entropy_grid_rows(V)


# (M, V, ld, dtype, scale, first column of the view inside the [M, ld] buffer).  Case 7 crosses the grid cap (asked of the library) twice
# with a ragged remainder; 8 is bf16 on the element-wise path (ld % 8 != 0); 9 a bf16 view whose base is not 16-byte aligned.
def _shapes():
    return [(5, 2, 2, F32, 3.0, 0), (64, 10, 10, F32, 3.0, 0), (256, 1000, 1000, F32, 30.0, 0), (512, 1024, 1024, BF16, 3.0, 0),
            (64, 1001, 1008, BF16, 3.0, 0), (3, 40000, 40000, BF16, 3.0, 0), (8, 65536, 65536, F32, 3.0, 0),
            (2 * _grid_rows(72) + 7, 72, 72, BF16, 3.0, 0), (64, 10, 10, BF16, 3.0, 0), (33, 200, 208, BF16, 3.0, 1)]


@functools.lru_cache(maxsize=None)
def _case(idx):
    """inputs (a view of a buffer whose other columns hold NaN), the float64 reference and torch's fp32 CPU evaluation of case idx,
    computed once"""
    M, V, ld, dtype, scale, off = _shapes()[idx]
    g = torch.Generator().manual_seed(1000 + idx)
    x = torch.randn(M, V, generator=g) * scale
    lo = V // 4
    x[1, lo: max(V // 2, lo + 1)] = float("-inf")
    t = torch.randint(0, V, (M,), generator=g)
    t[torch.rand(M, generator=g) < 0.25] = IGN
    t[0], t[1], t[2] = 0, V - 1, IGN
    buf = torch.full((M, ld), float("nan"), dtype=dtype)
    buf[:, off: off + V] = x.to(dtype)
    xs = buf[:, off: off + V]
    pad = torch.ones(ld, dtype=torch.bool)
    pad[off: off + V] = False
    return {"buf": buf, "t": t, "ref": R.cross_entropy_ref(xs, t, IGN, G_UP), "t32": R.cross_entropy_torch32(xs, t, IGN, G_UP),
            "shape": (M, V, ld, dtype), "off": off, "pad": pad}


def _dev(c):
    M, V, ld, dtype = c["shape"]
    buf = c["buf"].cuda()
    return buf, buf[:, c["off"]: c["off"] + V], c["t"].cuda()


# ------------------------------------------------------------------------------------------------ 1. cross-entropy shapes
@pytest.mark.parametrize("idx", range(10))
def test_cross_entropy_kernels_match_float64(hip, idx):
    from vitamd import ops
    c = _case(idx)
    M, V, ld, dtype = c["shape"]
    buf, x, t = _dev(c)
    loss_row, lse, stats = ops.cross_entropy_fwd(x, t, IGN)
    gup = torch.tensor(G_UP, device="cuda")
    SENT = 7.0
    outs = {}
    for od in (F32, BF16):
        obuf = torch.full((M, ld), SENT, dtype=od, device="cuda")
        ops.cross_entropy_bwd(x, t, lse, stats, gup, IGN, out=obuf[:, :V])
        outs[od] = obuf.cpu()
    torch.cuda.synchronize()
    assert abs(float(stats[1]) * c["ref"]["count"] - 1) < 1e-6
    got = {"loss_row": loss_row.cpu(), "lse": lse.cpu(), "mean": stats[0].cpu(), "grad": outs[F32][:, :V]}
    fails = R.check_cross_entropy(got, c["ref"], c["t32"], f"case {c['shape']}")
    fails += R.check_bf16_grad(outs[BF16][:, :V], c["ref"], c["t32"], f"case {c['shape']}")
    assert not fails, fails
    # ignored rows: exact zeros, loss 0; the pad columns: NaN still on the input, the sentinel still on both outputs
    ign = c["t"] == IGN
    assert bool((got["loss_row"][ign] == 0).all()) and bool((outs[F32][:, :V][ign] == 0).all()) and bool((outs[BF16][:, :V][ign] == 0).all())
    if ld > V:
        assert bool(torch.isnan(buf.cpu()[:, c["pad"]]).all())
        assert bool((outs[F32][:, V:] == SENT).all()) and bool((outs[BF16][:, V:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 2. in place, repeatability
@pytest.mark.parametrize("idx", [1, 3, 4, 8, 9])
def test_in_place_backward_and_repeated_calls_are_bit_identical(hip, idx):
    from vitamd import ops
    c = _case(idx)
    M, V, ld, dtype = c["shape"]
    buf, x, t = _dev(c)
    gup = torch.tensor(G_UP, device="cuda")
    a = ops.cross_entropy_fwd(x, t, IGN)
    b = ops.cross_entropy_fwd(x, t, IGN)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))          # bits, NaN-safe
    d1 = ops.cross_entropy_bwd(x, t, a[1], a[2], gup, IGN)
    d2 = ops.cross_entropy_bwd(x, t, a[1], a[2], gup, IGN)
    assert d1.dtype == dtype and torch.equal(d1, d2)
    buf2 = buf.clone()
    x2 = buf2[:, c["off"]: c["off"] + V]
    d3 = ops.cross_entropy_bwd(x2, t, a[1], a[2], gup, IGN, out=x2)
    assert d3.data_ptr() == x2.data_ptr() and torch.equal(x2, d1)
    if ld > V:
        assert bool(torch.isnan(buf2.cpu()[:, c["pad"]]).all())


# ------------------------------------------------------------------------------------------------ 3. error rows
def test_all_rows_ignored_and_out_of_range_targets(hip):
    from vitamd import ops
    c = _case(3)
    M, V, ld, dtype = c["shape"]
    _, x, t = _dev(c)
    none = torch.full_like(t, IGN)
    loss_row, lse, stats = ops.cross_entropy_fwd(x, none, IGN)
    d = ops.cross_entropy_bwd(x, none, lse, stats, None, IGN, out_dtype=F32)
    assert bool(torch.isnan(stats[0])) and bool((d == 0).all()) and bool((loss_row == 0).all())
    # targets V and -1, never in the last row
    bad = c["t"].clone()
    bad[3], bad[10] = V, -1
    loss_row, lse, stats = ops.cross_entropy_fwd(x, bad.cuda(), IGN)
    d = ops.cross_entropy_bwd(x, bad.cuda(), lse, stats, torch.tensor(G_UP, device="cuda"), IGN, out_dtype=F32)
    assert bool(torch.isnan(stats[0])) and bool(torch.isnan(loss_row[3])) and bool(torch.isnan(loss_row[10]))
    assert bool((d[3] == 0).all()) and bool((d[10] == 0).all())
    # the other rows: the reference with the two rows ignored, its count raised to the kernel's (which counts the two bad rows)
    as_ign = bad.clone()
    as_ign[3], as_ign[10] = IGN, IGN
    ref = R.cross_entropy_ref(c["buf"][:, c["off"]: c["off"] + V], as_ign, IGN, G_UP)
    t32 = R.cross_entropy_torch32(c["buf"][:, c["off"]: c["off"] + V], as_ign, IGN, G_UP)
    n_kernel = ref["count"] + 2
    keep = torch.ones(M, dtype=torch.bool)
    keep[3] = keep[10] = False
    got = {"loss_row": loss_row.cpu()[keep], "lse": lse.cpu()[keep], "grad": d.cpu()[keep].double() * (n_kernel / ref["count"])}
    sub = {k: (v[keep] if k in ("loss_row", "lse", "grad") else v) for k, v in ref.items()}
    sub32 = {k: (v[keep] if k in ("loss_row", "lse", "grad") else v) for k, v in t32.items() if k != "mean"}
    assert R.check_cross_entropy(got, sub, sub32, "bad targets") == []


# ------------------------------------------------------------------------------------------------ 4. lm.cross_entropy
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_lm_cross_entropy_matches_torch(hip, dtype):
    from vitamd import lm
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(4, 16, 1000, generator=g) * 3).to(dtype)
    t = torch.randint(0, 1000, (4, 16), generator=g)
    t[0, :5] = IGN
    ref = R.cross_entropy_ref(x.reshape(64, 1000), t.reshape(64), IGN, G_UP)
    t32 = R.cross_entropy_torch32(x.reshape(64, 1000), t.reshape(64), IGN, G_UP)
    xd = x.cuda().requires_grad_(True)
    loss = lm.cross_entropy(xd, t.cuda())
    assert loss.dim() == 0 and loss.dtype == F32
    (loss * G_UP).backward()
    assert xd.grad.dtype == dtype and xd.grad.shape == x.shape
    xt = x.cuda().float().requires_grad_(True)
    loss_t = F.cross_entropy(xt.reshape(64, 1000), t.cuda().reshape(64), ignore_index=IGN)
    (loss_t * G_UP).backward()
    got = {"mean": loss.detach().cpu()}
    if dtype == F32:
        got["grad"] = xd.grad.cpu().reshape(64, 1000)
    fails = R.check_cross_entropy(got, ref, t32, f"lm.cross_entropy {dtype}")
    if dtype == BF16:
        fails += R.check_bf16_grad(xd.grad.cpu().reshape(64, 1000), ref, t32, "lm.cross_entropy")
    assert not fails, fails
    # and against the framework on the same device tensors.  Each of the two fp32 evaluations is allowed max(4 e32, floor) from float64
    # (e32 from torch's CPU evaluation, nothing from either device result), so they may be twice that apart; a bf16 gradient may also
    # be half a bf16 ulp (+1/16) from the framework's fp32 one.
    e32 = R.cross_entropy_errors(t32, ref)
    n = ref["count"]
    row_scale = ref["lse"].abs().clamp_min(1.0)[:, None]
    d_loss = abs(float(loss.detach()) - float(loss_t.detach()))
    grad_t = xt.grad.cpu().reshape(64, 1000).double()
    d_grad = (xd.grad.cpu().reshape(64, 1000).double() - grad_t).abs()
    allow = 2 * R.bound(e32["grad"]) * row_scale / n + (R.BF16_HALF_ULP * grad_t.abs() if dtype == BF16 else 0.0)
    print(f"vs device torch: loss {d_loss:.3e}, grad worst / allowance {float((d_grad / allow).max()):.3f}")
    assert d_loss <= 2 * R.bound(e32["mean"]) * max(1.0, abs(float(ref["mean"])))
    assert bool((d_grad <= allow).all())


def test_lm_cross_entropy_as_loss_fn_of_the_vit_training_step(hip):
    """the body of test_gpu_parity.py::test_training_steps_match_reference_loop with loss_fn = lm.cross_entropy: its three bounds"""
    import train_vit as TV
    import utils as U
    from vitamd import lm
    from vitamd.optim import AdamW
    g = load_golden("train_steps_s32.pt")
    c = g["cfg"]
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    m = TV.ViTClassifier(cfg, num_classes=c["num_classes"])
    m.load_state_dict(W.classifier_state(c["seed"], 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, c["num_classes"]))
    m = m.cuda()
    images = W.normal(c["seed"], "images", (c["batch"], 3, 32, 32)).cuda()
    labels = W.randint(c["seed"], "labels", (c["batch"],), c["num_classes"]).cuda()
    optim = AdamW(m.parameters(), lr=c["lr"], weight_decay=c["weight_decay"])
    sched = U.get_lr_scheduler(optim, c["warmup"], c["train_steps"], c["min_lr"])
    losses = [float(TV.train_step(m, images, labels, optim, sched, loss_fn=lm.cross_entropy)) for _ in range(c["steps"])]
    ref = g["losses"].tolist()
    assert abs(losses[0] - ref[0]) < 5e-3
    for a, b in zip(losses, ref):
        assert abs(a - b) < 3e-2 * max(1.0, abs(b)), (losses, ref)
    assert O.rel_l2(m.head.bias.detach().cpu(), g["final_head_bias"]) < 7.3e-4


def test_lm_cross_entropy_in_a_graphed_step(hip):
    """test_gpu_parity.py::test_graphed_step_matches_eager with lm.cross_entropy as the loss: replays on new inputs against the eager step"""
    import train_vit as TV
    from vitamd import lm
    from vitamd.graph import GraphedStep
    torch.manual_seed(0)
    m = TV.ViTClassifier(TV.ViTConfig(32, 3, 16, "S", 1, 0.0), num_classes=10).cuda()
    ce = lm.cross_entropy
    xs = [W.normal(90 + i, "x", (64, 3, 32, 32)).cuda() for i in range(3)]
    ys = [W.randint(90 + i, "y", (64,), 10).cuda() for i in range(3)]
    step = GraphedStep(m, ce, xs[0], ys[0])
    for i in (1, 2, 0):
        loss_g = float(step(xs[i], ys[i]))
        got = {k: p.grad.clone() for k, p in m.named_parameters()}
        m.zero_grad(set_to_none=True)
        loss_e = ce(m(xs[i]), ys[i]); loss_e.backward()
        assert abs(loss_g - float(loss_e)) < 1e-6
        for k, p in m.named_parameters():
            assert O.rel_l2(got[k].cpu(), p.grad.cpu()) < 1.0e-6, k


# ------------------------------------------------------------------------------------------------ 5.-7. embedding
def _embed_case(B, S, D, tok_rows, pos_rows, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tok_rows, D, generator=g), torch.randn(pos_rows, D, generator=g), torch.randint(0, tok_rows, (B, S), generator=g), g)


@pytest.mark.parametrize("B, S, D", [(5, 37, 68), (4, 64, 512)])
def test_embedding_forward_is_the_gather_and_add(hip, B, S, D):
    from vitamd import lm, ops
    tok, pos, ids, _ = _embed_case(B, S, D, 257, S + 3, seed=B)
    ids[:, 0] = 256
    x = lm.token_embed(ids.cuda(), tok.cuda(), pos.cuda())
    assert tuple(x.shape) == (B, S, D) and torch.equal(x.cpu(), tok[ids] + pos[:S])
    assert torch.equal(x, tok.cuda()[ids.cuda()] + pos.cuda()[:S])
    bad = ids.clone()
    bad[1, 2], bad[2, 5] = 257, -1
    out = torch.full((B * S, D), 7.0, device="cuda")
    ops.embed_tokens_fwd(bad.cuda(), tok.cuda(), pos.cuda(), out=out)
    want = (tok[ids] + pos[:S]).reshape(B * S, D).clone()
    want[1 * S + 2], want[2 * S + 5] = 7.0, 7.0
    assert torch.equal(out.cpu(), want)


def test_embedding_backward_is_exact_on_integer_gradients(hip):
    """integer-valued g in [-8, 8]: every partial sum is an integer below 2^24, so fp32 sums are exact in any order"""
    from vitamd import ops
    B, S, D, tok_rows, pos_rows = 6, 70, 68, 257, 80
    tok, pos, ids, g = _embed_case(B, S, D, tok_rows, pos_rows, seed=11)
    ids[ids == 17] = 18
    free = torch.ones(B, S, dtype=torch.bool)
    free[:, 0] = free[3, 9] = False
    where = free.view(-1).nonzero().view(-1)
    ids.view(-1)[where[torch.randperm(where.numel(), generator=g)[:100]]] = 17       # one id exactly a hundred times
    ids[:, 0] = 256                                   # the start-of-sequence id in every row
    ids[3, 9] = 300                                   # out of range: adds nothing to dtok, still counts for dpos
    gr = torch.randint(-8, 9, (B, S, D), generator=g).float()
    dtok0 = torch.randint(-4, 5, (tok_rows, D), generator=g).float()
    dpos0 = torch.randint(-4, 5, (pos_rows, D), generator=g).float()
    dtok, dpos = dtok0.cuda(), dpos0.cuda()
    ops.embed_tokens_bwd(gr.cuda().view(B * S, D), ids.cuda(), dtok, dpos)
    rtok, rpos = R.embed_grads_ref(gr, ids, tok_rows, pos_rows)
    assert int((ids == 17).sum()) == 100 and bool((ids[:, 0] == 256).all())
    assert torch.equal(dtok.cpu().double(), rtok + dtok0.double())
    assert torch.equal(dpos.cpu().double(), rpos + dpos0.double())


def test_embedding_backward_on_random_gradients(hip):
    from vitamd import lm
    B, S, D = 4, 64, 512
    tok, pos, ids, g = _embed_case(B, S, D, 257, 64, seed=12)
    ids[:, 0] = 256
    dy = torch.randn(B, S, D, generator=g)
    tp, pp = tok.cuda().requires_grad_(True), pos.cuda().requires_grad_(True)
    (lm.token_embed(ids.cuda(), tp, pp) * dy.cuda()).sum().backward()
    rtok, rpos = R.embed_grads_ref(dy, ids, 257, 64)
    t32, p32 = tok.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    ((t32[ids] + p32[:S]) * dy).sum().backward()
    for name, got, ref, f32 in (("dtok", tp.grad, rtok, t32.grad), ("dpos", pp.grad, rpos, p32.grad)):
        e, floor = O.rel_l2(got.cpu(), ref), O.rel_l2(f32, ref)
        print(f"{name}: {e:.3e} (torch fp32 {floor:.3e})")
        assert e <= 4 * floor, name


# ------------------------------------------------------------------------------------------------ 8. the model
def _videogpt_sized(codebook, seed=0):
    """test_gpu_decode._videogpt with another codebook size (250: the head shapes the fused route does not take)"""
    import train_videogpt as V
    cfg = V.VideoGPTConfig(frame_size=16, codebook_size=codebook, transformer="S", max_frames=4, dropout=0.0)
    D, Nc = cfg.n_embd, cfg.codebook_size
    sd = {"tok_embed.weight": W.normal(seed, "tok_embed", (Nc + 1, D)), "pos_embed.weight": W.normal(seed, "pos_embed", (cfg.max_tokens, D))}
    sd.update(W.transformer_state(seed, "transformer.", cfg.trans_config.n_layers, D, causal_block=cfg.max_tokens))
    sd.update(W.linear_state(seed, "proj.", Nc, D))
    model = V.VideoGPT(cfg)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval(), sd, cfg


VIDEOGPT_GRAD_BOUND = 1e-2          # rel-L2 of a parameter gradient of the loss route against the oracle (tests/test_gpu_poison.py holds it too)


def _oracle_grads(x, sd, cfg, names):
    from test_gpu_decode import _oracle_videogpt
    leaves = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    _, loss = _oracle_videogpt(x, leaves, cfg)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return loss.detach(), dict(zip(names, grads))


@pytest.mark.parametrize("codebook", [256, 250])
def test_videogpt_loss_route_matches_oracle_and_present_route(hip, codebook):
    from test_gpu_decode import _videogpt
    from vitamd import lm
    model, sd, cfg = _videogpt() if codebook == 256 else _videogpt_sized(codebook)
    assert lm.fused_head_applies(codebook, cfg.n_embd) == (codebook == 256)
    x = W.randint(0, "video", (4, cfg.max_frames, cfg.frame_size), cfg.codebook_size)
    names = [k for k, _ in model.named_parameters()]
    oloss, ograds = _oracle_grads(x, sd, cfg, names)
    model.zero_grad(set_to_none=True)
    model(x.cuda())[1].backward()
    e_parent = {k: O.rel_l2(p.grad.cpu(), ograds[k]) for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    loss = model.loss(x.cuda())
    assert loss.dim() == 0 and abs(float(loss.detach()) - float(oloss)) < 5e-3
    if codebook == 256:
        loss.backward(retain_graph=True)
        with pytest.raises(RuntimeError):
            loss.backward()                      # the logits were overwritten by their gradient
    else:
        loss.backward()
        with pytest.raises(RuntimeError):
            loss.backward()                      # fallback route: nothing is consumed; this is autograd's own refusal of a freed graph
    for k, p in model.named_parameters():
        e_new = O.rel_l2(p.grad.cpu(), ograds[k])
        print(f"{k}: new {e_new:.3e} parent {e_parent[k]:.3e}")
        assert e_new < 1.5 * e_parent[k] and e_new < VIDEOGPT_GRAD_BOUND, (k, e_new, e_parent[k])


# ------------------------------------------------------------------------------------------------ 9. the training step
def test_train_step_follows_the_present_route(hip):
    import train_videogpt as V
    from test_gpu_decode import _videogpt
    from vitamd.optim import AdamW
    new, sd, cfg = _videogpt()
    old, _, _ = _videogpt()
    x = W.randint(0, "video", (4, cfg.max_frames, cfg.frame_size), cfg.codebook_size).cuda()
    o_new = AdamW(new.parameters(), lr=1e-3, weight_decay=1e-2)
    o_old = AdamW(old.parameters(), lr=1e-3, weight_decay=1e-2)
    got, ref = [], []
    for _ in range(3):
        got.append(float(V.train_step(new, x, o_new)))
        o_old.zero_grad(set_to_none=True)
        loss = old(x)[1]
        loss.backward()
        o_old.step()
        ref.append(float(loss.detach()))
    print("train_step losses", got, "present route", ref)
    for a, b in zip(got, ref):
        assert abs(a - b) < 3e-2 * max(1.0, abs(b)), (got, ref)
    assert got[2] < got[0]
