"""The kept-row path of a stack's last layer (functions.KEEP_ROWS): the kept forms of the LayerNorm and attention
kernels against the full-size kernels on the same inputs (exact: the per-row arithmetic is the same code), the short GEMMs the path runs,
and the whole path against the old one (full stack, then slice) with the CPU oracle as the yardstick of how far two bf16 flows may differ."""
import pytest
import torch

import vit_oracle as O
import weights as W

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def r16(x):
    return x.to(BF16).float()


def _kept(t, B, N, k):
    """rows b*N + t', t' < k, of a [B*N, ...] tensor -> [B*k, ...]"""
    return t.view(B, N, *t.shape[1:])[:, :k].reshape(B * k, *t.shape[1:])


LN_SHAPES = [(2, 5, 1), (3, 197, 1), (2, 197, 33)]


# ------------------------------------------------------------------------------------------ 1. LayerNorm forward, kept form
@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("B,N,k", LN_SHAPES)
def test_layernorm_fwd_keep_equals_the_kept_rows_of_the_full_kernel(hip, D, B, N, k):
    from vitamd import ops
    x = randn((B * N, D), 1, 2.0).to(DEV)
    add_full = randn((B * N, D), 2).to(DEV, BF16)
    add_k = _kept(add_full, B, N, k).contiguous()
    xs, y, mean, rstd = ops.layernorm_fwd(x, addend=add_full)
    xs_k, y_k, mean_k, rstd_k = ops.layernorm_fwd_keep(x, add_k, B, N, k)
    assert tuple(xs_k.shape) == (B * k, D) and tuple(y_k.shape) == (B * k, D) and tuple(mean_k.shape) == (B * k,)
    assert torch.equal(xs_k, _kept(xs, B, N, k)) and torch.equal(y_k, _kept(y, B, N, k))
    assert torch.equal(mean_k, _kept(mean, B, N, k)) and torch.equal(rstd_k, _kept(rstd, B, N, k))


# ------------------------------------------------------------------------------------------ 2. LayerNorm backward, compact g_res
@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("B,N,k", LN_SHAPES)
def test_layernorm_bwd_compact_g_res_equals_zero_expanded_g_res(hip, D, B, N, k):
    from vitamd import ops
    M = B * N
    x = randn((M, D), 3, 2.0).to(DEV)
    dy = randn((M, D), 4).to(DEV, BF16)
    g_k = randn((B * k, D), 5).to(DEV)
    g_full = torch.zeros((B, N, D), device=DEV)
    g_full[:, :k] = g_k.view(B, k, D)
    g_full = g_full.view(M, D)
    _, y, mean, rstd = ops.layernorm_fwd(x)
    for xhat in (y, None):                                   # the xhat form (the layer's) and the plain one
        cs_a, cs_b = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        ga, gba = ops.layernorm_bwd(dy, x, mean, rstd, g_res=g_k, want_bf16=True, colsum=cs_a, xhat=xhat, keep=(N, k))
        gb, gbb = ops.layernorm_bwd(dy, x, mean, rstd, g_res=g_full, want_bf16=True, colsum=cs_b, xhat=xhat)
        assert bool((ga == gb).all()) and bool((gba == gbb).all())       # adding +0.0 is exact; == tolerates the sign of zero
        assert O.rel_l2(cs_a.cpu(), gba.float().cpu().sum(0)) < 1.0e-6   # float atomics: the bound of test_layernorm_fwd_bwd's column sums
        assert O.rel_l2(cs_a.cpu(), cs_b.cpu()) < 1.0e-6


# ------------------------------------------------------------------------------------------ 3. attention forward, nq
@pytest.mark.parametrize("nq", [1, 5, 32, 33])
@pytest.mark.parametrize("B,H,N", [(2, 2, 197), (2, 3, 160), (1, 2, 256)])
def test_attention_fwd_keep_equals_the_kept_queries_of_the_full_kernel(hip, B, H, N, nq):
    from vitamd import ops
    assert ops.attention_keep_forms(N, nq) & ops.KEEP_FWD
    qkv = randn((B * N, 3 * H * 64), 6).to(DEV, BF16)
    o, lse = ops.attention_fwd(qkv, B, N, H)
    o_k, lse_k = ops.attention_fwd_keep(qkv, B, N, H, nq)
    assert tuple(o_k.shape) == (B * nq, H * 64) and tuple(lse_k.shape) == (B, H, N)     # lse2 keeps [B, H, N]; [..., :nq] is written
    assert torch.equal(o_k, _kept(o, B, N, nq))
    assert torch.equal(lse_k[:, :, :nq], lse[:, :, :nq])


# ------------------------------------------------------------------------------------------ 4. attention backward, nq
@pytest.mark.parametrize("nq", [1, 5, 32, 33])
@pytest.mark.parametrize("B,H,N", [(2, 2, 197), (2, 2, 64), (1, 3, 224)])
def test_attention_bwd_keep_equals_the_full_kernel_on_zero_padded_dO(hip, B, H, N, nq):
    from vitamd import ops
    assert ops.attention_keep_forms(N, nq) & ops.KEEP_BWD
    D = H * 64
    qkv = randn((B * N, 3 * D), 7).to(DEV, BF16)
    o, lse = ops.attention_fwd(qkv, B, N, H)
    do_k = randn((B * nq, D), 8).to(DEV, BF16)
    do_full = torch.zeros((B, N, D), dtype=BF16, device=DEV)
    do_full[:, :nq] = do_k.view(B, nq, D)
    db_full, db_k = torch.zeros(3 * D, device=DEV), torch.zeros(3 * D, device=DEV)
    dqkv_full = ops.attention_bwd(qkv, o, lse, do_full.view(B * N, D), B, N, H, dbias=db_full)
    lse_k = torch.full_like(lse, float("nan"))               # whatever lies beyond the kept queries must not be read
    lse_k[:, :, :nq] = lse[:, :, :nq]
    dqkv_kept = ops.attention_bwd_keep(qkv, _kept(o, B, N, nq).contiguous(), lse_k, do_k, B, N, H, nq, dbias=db_k)
    # with dO = 0 the full kernel's dP, delta and dS are exact zeros, so equality is expected, not approximate
    assert bool((dqkv_kept == dqkv_full).all())
    assert O.rel_l2(db_k.cpu(), db_full.cpu()) < 1.0e-6      # atomics
    q_rows = dqkv_kept.view(B, N, 3, D)[:, nq:, 0]
    assert bool((q_rows == 0).all())


# ------------------------------------------------------------------------------------------ 5. the short GEMMs of the kept-row MLP
@pytest.mark.parametrize("M", [2, 6, 256])
def test_gemm_nt_epilogues_on_few_rows(hip, M):
    """bounds: those of test_gpu_kernels.test_gemm_nt_epilogues for the same epilogues"""
    from vitamd import ops
    N, K = 512, 256
    a, b = r16(randn((M, K), 3)), r16(randn((N, K), 4, 0.1))
    bias = randn((N,), 5)
    acc = a @ b.t()
    ad, bd, biasd = a.to(DEV, BF16), b.to(DEV, BF16), bias.to(DEV)
    ref = r16(acc + r16(bias))
    y = ops.gemm_nt(ad, bd, ops.EPI_BIAS_BF16, bias=biasd).float().cpu()
    assert O.rel_l2(y, ref) < 3.2e-5
    res = randn((M, N), 6)
    y = ops.gemm_nt(ad, bd, ops.EPI_RESID_F32, bias=biasd, aux=res.to(DEV)).cpu()
    assert O.rel_l2(y, res + ref) < 2.8e-5
    dgl, act = ops.gemm_nt(ad, bd, ops.EPI_GELU_DG, bias=biasd)
    assert O.rel_l2(act.float().cpu(), r16(O.gelu_erf(ref))) < 2e-3
    xp = ref.clone().requires_grad_(True)
    O.gelu_erf(xp).backward(torch.ones_like(ref))
    assert O.rel_l2(dgl.float().cpu(), r16(xp.grad)) < 4.5e-5
    cs = torch.zeros(N, device=DEV)
    dg_in = r16(randn((M, N), 17, 0.5))
    y2 = ops.gemm_nt(ad, bd, ops.EPI_DMUL, aux=dg_in.to(DEV, BF16), colsum=cs).float().cpu()
    assert O.rel_l2(y2, r16(r16(acc) * dg_in)) < 2.2e-5
    assert O.rel_l2(cs.cpu(), y2.sum(0)) < 1.0e-6


@pytest.mark.parametrize("R", [2, 70, 256])
def test_gemm_tn_on_few_rows_with_the_short_reduction_split_rule(hip, R):
    """bound: test_gpu_kernels.test_gemm_tn_exclusive_form_equals_shared_form's against fp32 torch"""
    from vitamd import functions as F, ops
    P, Q = 768, 3072
    l, r = r16(randn((R, P), 9)), r16(randn((R, Q), 10))
    ref = l.t() @ r
    for form in (ops.TN_FORM_SHARED, ops.TN_FORM_EXCLUSIVE):
        out = torch.full((P, Q), 3.0, device=DEV)
        splits = F._tn_splits(out, R)
        assert 1 <= splits <= max(1, (R + 63) // 64) and splits <= 4
        ops.gemm_tn(l.to(DEV, BF16), r.to(DEV, BF16), out, accumulate=False, splits=splits, form=form)
        assert O.rel_l2(out.cpu(), ref) < 2.0e-6


# ------------------------------------------------------------------------------------------ 6. whole path, KEEP_ROWS on against off
def _both_paths(run):
    from vitamd import functions as F
    saved = F.KEEP_ROWS
    try:
        out = {}
        for flag in (True, False):
            F.KEEP_ROWS = flag
            out[flag] = run()
    finally:
        F.KEEP_ROWS = saved
    return out[True], out[False]


def _assert_within_the_old_paths_own_error(kept, full, oracle):
    """The two paths differ only by fp32 summation order inside GEMMs and the bf16 re-rounding that follows, so a path that differs from
    the old one by more than the old one differs from the reference is wrong: rel_l2(kept, full) <= rel_l2(full, oracle) + 1e-6."""
    assert kept.keys() == full.keys() == oracle.keys()
    for k in kept:
        assert kept[k].shape == full[k].shape and kept[k].dtype == full[k].dtype, k
        e_new, e_old = O.rel_l2(kept[k], full[k]), O.rel_l2(full[k], oracle[k])
        print(f"{k}: kept vs full {e_new:.3e}   full vs oracle {e_old:.3e}")
        assert e_new <= e_old + 1e-6, (k, e_new, e_old)


def test_kept_path_classifier_s16_on_32px(hip):
    """N = 5: the attention forms without a kept-query kernel (full-size attention, zero-padded dO)"""
    import train_vit as TV
    cfg = TV.ViTConfig(32, 3, 16, "S", 1, 0.0)
    tc = cfg.trans_config
    sd = W.classifier_state(3, 3, 16, cfg.n_patches, 1, tc.n_layers, tc.n_embd, 10)
    m = TV.ViTClassifier(cfg, num_classes=10)
    m.load_state_dict(sd)
    m = m.cuda()
    images, labels = W.normal(3, "images", (8, 3, 32, 32)), W.randint(3, "labels", (8,), 10)

    def run():
        m.zero_grad(set_to_none=True)
        logits = m(images.cuda())
        torch.nn.functional.cross_entropy(logits, labels.cuda()).backward()
        torch.cuda.synchronize()
        assert tuple(logits.shape) == (8, 10) and logits.dtype == F32
        return {"logits": logits.detach().cpu(), **{k: p.grad.cpu() for k, p in m.named_parameters()}}

    kept, full = _both_paths(run)
    ologits, _, ograds = O.classifier_loss_and_grads(images, labels, sd, O.OracleViTConfig.preset(32, 3, 16, "S", 1), lowp=True)
    _assert_within_the_old_paths_own_error(kept, full, {"logits": ologits, **{k: ograds[k] for k in kept if k != "logits"}})


@pytest.mark.parametrize("D,H,N,B,keep", [(768, 12, 197, 2, 1), (768, 12, 197, 2, 33),       # pipelined kept-query kernels, one and two query tiles
                                          (512, 8, 96, 2, 32)])                                # a TiTok-like prefix; N = 96: full-size attention forms
def test_kept_path_two_layer_stack(hip, D, H, N, B, keep):
    import transformer as T
    L, seed = 2, 11
    sd = W.transformer_state(seed, "", L, D)
    m = T.Transformer(T.TransformerConfig(n_layers=L, n_heads=H, n_embd=D, block_size=N))
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    x0 = W.normal(seed, "x", (B, N, D))
    dy = W.normal(seed, "dy", (B, keep, D))

    def run():
        m.zero_grad(set_to_none=True)
        x = x0.cuda().requires_grad_(True)
        y = m(x, keep=keep)
        assert tuple(y.shape) == (B, keep, D) and y.dtype == F32
        (y * dy.cuda()).sum().backward()
        torch.cuda.synchronize()
        return {"y": y.detach().cpu(), "dx": x.grad.cpu(), **{k: p.grad.cpu() for k, p in m.named_parameters()}}

    kept, full = _both_paths(run)
    xo = x0.clone().requires_grad_(True)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    yo = O.transformer(xo, leaves, "", L, H, False, lowp=True)[:, :keep]
    names = list(leaves)
    go = torch.autograd.grad((yo * dy).sum(), [xo] + [leaves[k] for k in names])
    _assert_within_the_old_paths_own_error(kept, full, {"y": yo.detach(), "dx": go[0], **dict(zip(names, go[1:]))})


# ------------------------------------------------------------------------------------------ 7. captured step
def test_graphed_step_with_the_kept_path(hip):
    import train_vit as TV
    from vitamd import functions as F
    from vitamd.graph import GraphedStep
    assert F.KEEP_ROWS
    torch.manual_seed(0)
    m = TV.ViTClassifier(TV.ViTConfig(32, 3, 32, "S", 1, 0.0), num_classes=10).cuda()
    ce = torch.nn.functional.cross_entropy
    xs = [W.normal(70 + i, "x", (16, 3, 32, 32)).cuda() for i in range(2)]
    ys = [W.randint(70 + i, "y", (16,), 10).cuda() for i in range(2)]
    step = GraphedStep(m, ce, xs[0], ys[0])
    for i in (1, 0):
        loss_g = float(step(xs[i], ys[i]))
        m.zero_grad(set_to_none=True)
        loss_e = ce(m(xs[i]), ys[i])
        assert abs(loss_g - float(loss_e)) < 1e-6
