"""Bias gradients from the weight-gradient GEMM: ops.gemm_tn(colsum=) sums the columns of its L operand beside the
MFMAs, the dgrad-fc2 GEMM runs without the column sums in its epilogue, and the layer backward takes db1 / db2 (functions.BIAS_FROM_WGRAD)
and dbqkv (functions.BIAS_QKV_FROM_WGRAD) from there."""
import pytest
import torch

import weights as W

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24          # unit round-off of fp32


def dev():
    return torch.device("cuda")


def ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _forms():
    from vitamd import ops
    return (ops.TN_FORM_SHARED, ops.TN_FORM_EXCLUSIVE)


# ------------------------------------------------------------------------------------------ 1. the TN kernel
@pytest.mark.parametrize("Q", [256, 768])                    # 768: three column tiles - a second contributor would double-count
@pytest.mark.parametrize("P", [256, 264, 768])               # 264: ragged last row tile
@pytest.mark.parametrize("R", [64, 100, 1000])               # 100: ragged last quarter
def test_colsum_exact_on_integers_and_out_unchanged(hip, R, P, Q):
    """L = integers in [-8, 8]: every fp32 partial sum is an integer below 2^24, so the sums are exact in any order and must EQUAL the fp64
    column sums - for splits 1, 3 and 0 (auto, capped at the step count), both kernel forms, a zeroed and a non-zero colsum (added to).
    `out` is the exact integer product with and without colsum."""
    from vitamd import ops
    l, r = ints((R, P), -8, 8, 1), ints((R, Q), -2, 2, 2)
    want_cs, want_out = l.to(F64).sum(0), l.t() @ r
    ld, rd = l.to(dev(), BF16), r.to(dev(), BF16)
    init = ints((P,), -50, 50, 3)
    for splits in (1, 3, 0):
        for form in _forms():
            plain = torch.full((P, Q), 7.0, device=dev())
            ops.gemm_tn(ld, rd, plain, splits=splits, accumulate=False, form=form)
            for start in (torch.zeros(P), init):
                cs = start.clone().to(dev())
                out = torch.full((P, Q), -3.0, device=dev())
                ops.gemm_tn(ld, rd, out, splits=splits, accumulate=False, form=form, colsum=cs)
                torch.cuda.synchronize()
                what = (splits, form, bool(start.any()))
                assert torch.equal(cs.cpu().to(F64), start.to(F64) + want_cs), what
                assert torch.equal(out, plain) and torch.equal(out.cpu(), want_out), what


@pytest.mark.parametrize("R,P,Q,splits", [(1000, 264, 768, 3), (1000, 768, 256, 0), (100, 256, 256, 1)])
def test_colsum_on_gaussian_data_within_the_fp32_summation_bound_and_reproducible(hip, R, P, Q, splits):
    """|colsum - fp64 sum| <= (R - 1) 2^-24 sum_r |L[r,p]|, the worst-case bound of R - 1 rounded fp32 additions in any order; two identical
    calls agree bit for bit (no atomics: partials per split, summed in split order), and `out` equals the call without colsum."""
    from vitamd import ops
    l = randn((R, P), 5).to(BF16)
    ld, rd = l.to(dev()), randn((R, Q), 6).to(dev(), BF16)
    ref = l.to(F64).sum(0)
    bound = (R - 1) * U * l.to(F64).abs().sum(0)
    for form in _forms():
        got = []
        for _ in range(2):
            cs, out = torch.zeros(P, device=dev()), torch.empty((P, Q), device=dev())
            ops.gemm_tn(ld, rd, out, splits=splits, accumulate=False, form=form, colsum=cs)
            got.append((cs, out))
        plain = torch.empty((P, Q), device=dev())
        ops.gemm_tn(ld, rd, plain, splits=splits, accumulate=False, form=form)
        torch.cuda.synchronize()
        err = (got[0][0].cpu().to(F64) - ref).abs()
        print(f"form {form}: worst error / bound {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), form
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][1], plain), form


def test_colsum_needs_the_workspace_form(hip):
    from vitamd import ops, lib
    l, r = torch.ones((64, 256), device=dev(), dtype=BF16), torch.ones((64, 256), device=dev(), dtype=BF16)
    out, cs = torch.zeros((256, 256), device=dev()), torch.zeros(256, device=dev())
    with pytest.raises(lib.VitamdError):
        ops.gemm_tn(l, r, out, atomic=True, colsum=cs)
    st = torch.cuda.current_stream().cuda_stream
    small = torch.zeros(16, device=dev())
    need = hip.vitamd_gemm_tn_ws_bytes(64, 256, 256, 1)
    ws = torch.zeros(need // 4, device=dev())
    args = (l.data_ptr(), r.data_ptr(), out.data_ptr(), cs.data_ptr(), 64, 256, 256, 256, 256, 256, 1)
    assert hip.vitamd_gemm_tn_bf16_ws_colsum(*args, small.data_ptr(), 64, 1, 0, st) == 2             # workspace too small: VITAMD_ERR_ARG
    assert hip.vitamd_gemm_tn_bf16_ws_colsum(*args, ws.data_ptr(), need - 1024, 1, 0, st) == 2       # room for the tiles, none for the partials
    assert hip.vitamd_gemm_tn_bf16_ws_colsum(*args, ws.data_ptr(), need, 1, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(cs.cpu(), torch.full((256,), 64.0))


# ------------------------------------------------------------------------------------------ 2. dgrad-fc2 without column sums
@pytest.mark.parametrize("tile,form", [(2048, 5), (4096, 4)])          # loader form, seam form (VITAMD_NT_FORM_*)
def test_dgrad_fc2_without_colsum_is_bit_identical(hip, tile, form):
    """EPI_DMUL with colsum=None takes the instantiation whose epilogue has no column sums: the same `out`, bit for bit (M = 600: ragged last
    row tile; 3 x 2 tiles)."""
    from vitamd import ops
    M, N, K = 600, 512, 256
    assert hip.vitamd_gemm_nt_plan(M, N, K, N, ops.EPI_DMUL, tile) & 0x7f == form
    a, b = randn((M, K), 21).to(dev(), BF16), randn((N, K), 22, 0.05).to(dev(), BF16)
    aux = randn((M, N), 23, 0.5).to(dev(), BF16)
    cs = torch.zeros(N, device=dev())
    with_cs = ops.gemm_nt(a, b, ops.EPI_DMUL, aux=aux, colsum=cs, tile=tile)
    for _ in range(2):
        without = ops.gemm_nt(a, b, ops.EPI_DMUL, aux=aux, colsum=None, tile=tile)
        torch.cuda.synchronize()
        assert torch.equal(with_cs, without)
    assert float(cs.abs().sum()) > 0


# ------------------------------------------------------------------------------------------ 3. the layer stack, BIAS_FROM_WGRAD on against off
def _run_stack(flag, mode, record):
    """One forward + backward of a 2-layer stack (D = 256, H = 4, B = 3, N = 40).  record: list that receives, per weight-gradient GEMM of
    the backward in launch order, (rows, column sums of |L|) - the quantities the bias-gradient bound is made of."""
    import transformer as T
    from vitamd import functions as F, ops
    from vitamd.functions import TransformerStackFn
    L, D, H, B, N, seed = 2, 256, 4, 3, 40, 17
    keep = 1 if mode == "keep" else None
    p_mlp = 0.1 if mode == "p_mlp" else 0.0
    m = T.Transformer(T.TransformerConfig(n_layers=L, n_heads=H, n_embd=D, block_size=N))
    m.load_state_dict(W.transformer_state(seed, "", L, D), strict=True)
    m = m.cuda()
    x = W.normal(seed, "x", (B, N, D)).cuda().requires_grad_(True)
    dy = W.normal(seed, "dy", (B, N if keep is None else keep, D)).cuda()
    params = [p for layer in m.layers for p in layer._params()]
    saved_flags, saved_tn = (F.BIAS_FROM_WGRAD, F.BIAS_QKV_FROM_WGRAD), ops.gemm_tn

    def gemm_tn(l, r, out, *a, **kw):
        record.append((l.shape[0], l.shape[1], l.detach().to(F64).abs().sum(0).cpu()))
        return saved_tn(l, r, out, *a, **kw)

    try:
        F.BIAS_FROM_WGRAD = F.BIAS_QKV_FROM_WGRAD = flag
        ops.gemm_tn = gemm_tn
        torch.manual_seed(1234)                      # the dropout seeds come from torch's CPU generator: the same masks in every run
        y = TransformerStackFn.apply(x, H, False, 0.0, p_mlp, keep, *params)
        (y * dy).sum().backward()
        torch.cuda.synchronize()
    finally:
        (F.BIAS_FROM_WGRAD, F.BIAS_QKV_FROM_WGRAD), ops.gemm_tn = saved_flags, saved_tn
    return {"y": y.detach().cpu(), "dx": x.grad.cpu(), **{k: p.grad.cpu() for k, p in m.named_parameters()}}


@pytest.mark.parametrize("mode", ["plain", "p_mlp", "keep"])
def test_stack_bias_gradients_from_the_weight_gradient_gemms(hip, mode):
    """BIAS_FROM_WGRAD and BIAS_QKV_FROM_WGRAD on against off: the output, every weight gradient and the input gradient bit for bit; every
    bias gradient within 2 M 2^-24 sum|column| (M rows summed, `column` the column of dy2 / dpre / dqkv it is the sum of: both paths are
    fp32 sums of the same M numbers, each within (M - 1) 2^-24 sum|column| of the true sum).  With the flags on, two runs agree bit for bit
    in everything (no bias gradient of a layer depends on atomic order any more)."""
    rec_on, rec_off = [], []
    on, on2, off = _run_stack(True, mode, rec_on), _run_stack(True, mode, []), _run_stack(False, mode, rec_off)
    assert on.keys() == off.keys() and len(rec_on) == len(rec_off) == 6
    # launch order of the backward: top layer first, fc2, fc1, qkv in each
    bound = {}
    for i, layer in enumerate((1, 0)):
        for j, name in enumerate(("mlp.2.bias", "mlp.0.bias", "multi_attn.qkv.bias")):
            (rows, cols, s_on), (rows_off, _, s_off) = rec_on[3 * i + j], rec_off[3 * i + j]
            assert rows == rows_off and torch.equal(s_on, s_off)              # the same operand on both sides
            bound[f"layers.{layer}.{name}"] = (2 * rows * U * s_on, cols)
    n_bias = 0
    for k in on:
        if k.endswith(".bias"):
            b, cols = bound[k]
            assert on[k].numel() == cols
            err = (on[k].to(F64) - off[k].to(F64)).abs()
            print(f"{k}: worst |on - off| / bound {float((err / b.clamp_min(1e-300)).max()):.3e}")
            assert bool((err <= b).all()), k
            n_bias += 1
        else:
            assert torch.equal(on[k], off[k]), k
        assert torch.equal(on[k], on2[k]), k
    assert n_bias == 6
