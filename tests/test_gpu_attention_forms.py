"""Attention at every kernel instantiation a call can launch, at both edges of its tile count (_attention_ref.FORM_CASES;
tests/test_attention_forms_host.py proves from vitamd_attention_form that no instantiation is left out).  B = H = 2: B*H = 4 puts every
wave rotation of the pipelined backward on every tile count, B = 2 the batch stride of the compact o / d_o, H = 2 the head offset.

Ordinary cases: o, lse, dq, dk, dv to _attention_ref.compare's bounds (1.5 x the global floor, 2 x the worst-tile floor, lse 1e-6) against
the fp64 reference, exactly as test_gpu_attention_matrix.test_attention_matrix; dbias = the column sums of the stored dqkv; a second run
bit-identical; the residual form bit-equal in o and lse to the call without it, x1 = x0 + o exactly.
Kept-query cases: both contracts - bit-equality with the full-size kernels on zero-padded d_o (as tests/test_gpu_keep.py states it, with
NaN beyond nq in lse and delta, neither read nor written), AND compare() against the fp64 reference of the zero-padded problem: equality
with a full kernel that has itself never run at that tile count would prove little.
Every ratio over its floor is recorded (record_property); profiles/attention_forms/gpu_visit.md holds what was measured."""
import pytest
import torch

import _attention_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"


def _raw_form(*call):
    from vitamd import lib
    N, causal, p, resid, nq, bwd = call
    return lib.load().vitamd_attention_form(N, int(causal), p, int(resid), nq, int(bwd))


def _assert_forms(c, record_property):
    """the new binding gives the codes the case was chosen for"""
    from vitamd import ops
    got = [ops.attention_form(*call) for call in R.form_case_calls(c, _raw_form)]
    for code in R.FORM_EXPECT[c]:
        assert code in got, (R.code_name(code), [R.code_name(g) for g in got])
    record_property("forms", "; ".join(R.code_name(g) for g in got))


def _record(ratios, bad, record_property):
    for n, (g, t) in ratios.items():
        record_property(f"{n}_over_floor", round(g, 4) if n != "lse" else g)
        record_property(f"{n}_tile_over_tile_floor", round(t, 4) if n != "lse" else t)
    print("ratios (global / floor, worst tile / tile floor):", {n: (round(g, 3), round(t, 3)) if n != "lse" else g for n, (g, t) in ratios.items()})
    assert not bad, bad


def _kept(t, B, N, k):
    """rows b*N + t', t' < k, of a [B*N, ...] tensor -> [B*k, ...]"""
    return t.view(B, N, *t.shape[1:])[:, :k].reshape(B * k, *t.shape[1:])


def _ordinary(c, record_property):
    from vitamd import ops
    B, N, H, causal, p, resid, nq = c
    qkv, d_o, x0 = R.form_inputs(c)
    r = R.form_reference(c)
    drop = (p, R.SEED)
    qd, gd, x0d = qkv.to(DEV, BF16), d_o.to(DEV, BF16), x0.to(DEV)

    def run(dbias=None):
        o, lse, x1 = ops.attention_fwd(qd, B, N, H, causal, dropout=drop, resid=x0d)
        return o, lse, x1, ops.attention_bwd(qd, o, lse, gd, B, N, H, causal, dbias=dbias, dropout=drop)

    o_plain, lse_plain = ops.attention_fwd(qd, B, N, H, causal, dropout=drop)
    dbias = torch.full((3 * H * 64,), 1.0, device=DEV)                               # the sums are ADDED
    o, lse, x1, dqkv = run(dbias)
    assert torch.equal(o, o_plain) and torch.equal(lse, lse_plain)                   # the residual form: the same o and lse, bit for bit
    assert torch.equal(x1, x0d + o_plain.float())
    assert R.rel_l2(dbias.cpu() - 1.0, dqkv.float().cpu().sum(0)) < 1.0e-6           # fused QKV-bias gradient = column sums of what was stored
    got = R.kernel_outputs(o.cpu(), lse.cpu(), dqkv.cpu(), B, N, H)
    for t in got.values():
        assert bool(torch.isfinite(t).all())
    fl = r["floors"] if N > 1 else {n: r["floors"][n] for n in ("o", "dv")}          # N = 1: dq / dk by their residue, as in test_attention_matrix
    ratios, bad = R.compare({n: got[n] for n in (*fl, "lse")}, r["ref"], fl)
    if N == 1:
        bad += R.one_key_residue(got, r["in"])
    _record(ratios, bad, record_property)
    o2, lse2, x12, dqkv2 = run()                                                     # same seed: bit-identical
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(x1, x12) and torch.equal(dqkv, dqkv2)


def _kept_case(c, record_property):
    from vitamd import ops
    B, N, H, causal, p, resid, nq = c
    D = H * 64
    qkv, d_o, _ = R.form_inputs(c)                                                   # d_o: compact [B*nq, D]
    r = R.form_reference(c)                                                          # ... of d_o zero-padded to N rows
    served = ops.attention_keep_forms(N, nq)
    assert served
    qd, gd = qkv.to(DEV, BF16), d_o.to(DEV, BF16)
    o, lse = ops.attention_fwd(qd, B, N, H)
    ratios, bad = {}, []
    if served & ops.KEEP_FWD:
        o_k, lse_k = ops.attention_fwd_keep(qd, B, N, H, nq)
        assert tuple(o_k.shape) == (B * nq, D) and tuple(lse_k.shape) == (B, H, N)
        assert torch.equal(o_k, _kept(o, B, N, nq)) and torch.equal(lse_k[:, :, :nq], lse[:, :, :nq])
        ref_k = R.keep_slice(r["ref"], nq)
        got = {"o": R.heads(o_k.float().cpu(), B, nq, H), "lse": lse_k[:, :, :nq].cpu()}
        ratios, bad = R.compare(got, ref_k, R.floors(ref_k, R.keep_slice(r["restate"], nq), ("o",)))
        o_k2, lse_k2 = ops.attention_fwd_keep(qd, B, N, H, nq)
        assert torch.equal(o_k, o_k2) and torch.equal(lse_k[:, :, :nq], lse_k2[:, :, :nq])
    if served & ops.KEEP_BWD:
        g_full = R.pad_rows(gd, B, N, nq)
        db_full, db_k = torch.zeros(3 * D, device=DEV), torch.full((3 * D,), 1.0, device=DEV)
        dqkv_full = ops.attention_bwd(qd, o, lse, g_full, B, N, H, dbias=db_full)
        lse_k = torch.full_like(lse, float("nan"))                                   # whatever lies beyond the kept queries must not be read ...
        lse_k[:, :, :nq] = lse[:, :, :nq]
        lse_in = lse_k.clone()
        o_in = _kept(o, B, N, nq).contiguous()

        def run(dbias=None):
            delta = torch.full_like(lse, float("nan"))                               # ... nor written
            return ops.attention_bwd_keep(qd, o_in, lse_k, gd, B, N, H, nq, dbias=dbias, delta=delta), delta

        dqkv, delta = run(db_k)
        # with dO = 0 the full kernel's dP, delta and dS are exact zeros, so equality is expected, not approximate
        assert bool((dqkv == dqkv_full).all())
        assert bool((dqkv.view(B, N, 3, D)[:, nq:, 0] == 0).all())
        assert bool(torch.isfinite(delta[:, :, :nq]).all()) and bool(torch.isnan(delta[:, :, nq:]).all())
        assert torch.equal(lse_k.isnan(), lse_in.isnan()) and torch.equal(lse_k[:, :, :nq], lse_in[:, :, :nq])
        assert R.rel_l2(db_k.cpu() - 1.0, dqkv.float().cpu().sum(0)) < 1.0e-6         # the sums are ADDED; atomics
        assert R.rel_l2(db_k.cpu() - 1.0, db_full.cpu()) < 1.0e-6
        got = R.kernel_outputs(o.cpu(), lse.cpu(), dqkv.cpu(), B, N, H)
        for t in got.values():
            assert bool(torch.isfinite(t).all())
        grads = ("dq", "dk", "dv")
        ratios_b, bad_b = R.compare({n: got[n] for n in grads}, r["ref"], {n: r["floors"][n] for n in grads})
        ratios, bad = {**ratios, **ratios_b}, bad + bad_b
        dqkv2, delta2 = run()
        assert torch.equal(dqkv, dqkv2) and torch.equal(delta[:, :, :nq], delta2[:, :, :nq])
    _record(ratios, bad, record_property)


@pytest.mark.parametrize("c", R.FORM_CASES, ids=R.form_case_id)
def test_attention_form(hip, c, record_property):
    _assert_forms(c, record_property)
    (_kept_case if c[6] else _ordinary)(c, record_property)
