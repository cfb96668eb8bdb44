"""No GPU: proof that tests/test_gpu_attention_matrix.py can fail.  (a) on every case of that file the online restatement of the kernels'
arithmetic sits inside both bounds against the fp64 reference - the condition the cases were chosen for; (b) each listed mutation of the
restatement breaks a bound on at least one case (or, for the mask mutations, is also seen by the probe decoders); (c) the probe decoders
recover mask() exactly from restated outputs and see every single flipped decision; (d) mask() and ref64() agree with the definitions they
restate (_dropout_ref.keep at hand-written indices, oracle.sdpa); (e) the same for tests/test_gpu_attention_forms.py: (a) on every case of
FORM_CASES, and two mistakes a kept-query backward can make break a bound on every case with nq = 33."""
import numpy as np
import pytest
import torch

import _attention_ref as R
import _dropout_ref as DR
import vit_oracle as O


# ------------------------------------------------------------------------------------------ (a) the reference sits inside the bounds
def _check_reference_case(r, B, N, H, causal, sized=True):
    on = R.restate(*r["in"], r["M"], causal, online=True)
    fl = r["floors"] if N > 1 else {n: r["floors"][n] for n in ("o", "dv")}
    ratios, bad = R.compare({n: on[n] for n in (*fl, "lse")}, r["ref"], fl)
    if N == 1:
        bad += R.one_key_residue(on, r["in"]) + R.one_key_residue(r["restate"], r["in"])
    assert not bad, (bad, ratios)
    for n, (fg, ft) in fl.items():                 # the floors themselves are bf16-sized: a reference that lost its roundings would read 0
        if N > 1 and sized:
            assert 5e-4 < fg < 6e-3 and ft < 1.2e-2, (n, fg, ft)
        elif N > 1:
            assert fg > 0 and ft > 0, (n, fg, ft)


@pytest.mark.parametrize("c", R.MATRIX, ids=R.case_id)
def test_online_restatement_is_inside_the_bounds(c):
    B, N, H, causal, p = c
    _check_reference_case(R.matrix_reference(c), B, N, H, causal)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,key", R.SPIKE_CASES)
def test_online_restatement_is_inside_the_bounds_with_a_spike(N, key, causal):
    r = R.spike_reference(N, key, causal)
    _check_reference_case(r, 1, N, 1, causal, sized=False)     # inputs of scale 0.5 and one saturated row: other floors than the matrix
    if not causal:                                  # the spiked row is the dominating key's value row, in every form
        v = r["in"][2][0, 0, key].double()
        for o in (r["ref"]["o"], r["restate"]["o"]):
            assert R.rel_l2(o[0, 0, 10], v) < 1e-6


def test_row_chunked_forms_equal_the_full_ones():
    """N = 300 in blocks of 128 rows: the chunked forward / backward that serve N = 16 384 give ref64's and restate()'s numbers"""
    N, tiles = 300, (0, 3, 4, 9)
    qkv, d_o = R.long_inputs(N)
    q, k, v = qkv[:, :64], qkv[:, 64:128], qkv[:, 128:]
    full = [t[None, None] for t in (q, k, v, d_o)]
    ref, rs = R.ref64(*full, None, True), R.restate(*full, None, True)
    o, lse, o_rs = R.long_forward(q, k, v, True, block=128)
    assert R.rel_l2(o, ref["o"]) < 1e-13 and R.rel_l2(lse, ref["lse"]) < 1e-13 and R.rel_l2(o_rs, rs["o"]) < 1e-13
    g64 = R.long_backward(q, k, v, d_o, o, lse, True, tiles, False)
    g16 = R.long_backward(q, k, v, d_o, o_rs, lse, True, tiles, True)
    pad = torch.zeros(1, 1, 20, 64, dtype=torch.float64)
    for n in ("dq", "dk", "dv"):
        assert R.rel_l2(g64[n], R.take_tiles(torch.cat([ref[n], pad], -2)[0, 0], tiles)) < 1e-12, n
        # the full restatement rounds P once and derives dS from the same exp; equal up to the rounding ties an ulp of fp64 can flip
        assert R.rel_l2(g16[n], R.take_tiles(torch.cat([rs[n], pad], -2)[0, 0], tiles)) < 2e-4, n


# ------------------------------------------------------------------------------------------ (b) mutants
def _bound_failures(name, cases):
    """first case of `cases` on which mutant `name` breaks a bound -> (case, failures) or None"""
    for c in cases:
        B, N, H, causal, p = c
        r = R.matrix_reference(c)
        got = R.mutant_outputs(name, c)
        fl = r["floors"] if N > 1 else {n: r["floors"][n] for n in ("o", "dv")}
        _, bad = R.compare({n: got[n] for n in (*fl, "lse")}, r["ref"], fl)
        if bad:
            return c, bad
    return None


def _decoded_mask(M, N, causal, kinds=("fwd", "dq", "dkv"), exact_delta=None):
    """simulate the three probes on the CPU with restate() -> {kind: keep [B, H, N, N]} and the dQ probe's decoded quantity"""
    B, H = R.PROBE_B, R.PROBE_H
    Mt = M if not isinstance(M, dict) else M["fwd"]
    delta_ref = R.probe_delta_ref(Mt if exact_delta is None else exact_delta, causal)
    out = {kd: torch.zeros(B, H, N, N, dtype=torch.bool) for kd in kinds}
    qty = torch.zeros(B, H, N, N, dtype=torch.float64)
    for j in range(R.n_blocks(N)):
        sl = slice(64 * j, min(N, 64 * j + 64))
        for kd in kinds:
            qkv, d_o = R.probe_inputs(kd, B, N, H, j)
            rs = R.restate(*R.split(qkv, B, N, H), R.heads(d_o, B, N, H), M, causal)
            if kd == "fwd":
                out[kd][..., sl] = R.decode_fwd(rs["o"], j, N)
            elif kd == "dkv":
                out[kd][..., sl, :] = R.decode_dkv(rs["dv"], j, N)
            else:
                qty[..., sl] = R.dq_quantity(rs["dq"], j, N, delta_ref, causal)
                out[kd][..., sl] = R.decode_dq(rs["dq"], j, N, delta_ref, causal, R.PROBE_P)
    return out, qty


# which check is expected to catch which mutant (the table of profiles/attention_matrix/gpu_visit.md is printed from this test's findings)
@pytest.mark.parametrize("name", list(R.MUTANTS))
def test_every_mutant_breaks_a_bound(name):
    build, flag = R.MUTANTS[name]
    cases = [c for c in R.MATRIX if (build is None or c[4] > 0)]
    if flag in ("causal_lt", "diag_unmasked_dkv"):
        cases = [c for c in cases if c[3]]
    if flag in ("dq_no_keep", "dv_no_keep", "l_after_mask", "delta_pre_dropout"):
        cases = [c for c in cases if c[4] > 0]
    if flag == "pad_keys":
        cases = [c for c in cases if not c[3] and c[1] % 32]
    hit = _bound_failures(name, sorted(cases, key=lambda c: c[1]))
    assert hit is not None, f"mutant '{name}' passes every bound"
    print(f"\nMUTANT {name!r}: {R.case_id(hit[0])}: {hit[1][0]}")


@pytest.mark.parametrize("name", [n for n, (b, _) in R.MUTANTS.items() if b is not None])
def test_mask_mutants_are_also_seen_by_the_decoders(name):
    N = 70
    keep, _, M = R.probe_reference(N, False)
    Mm = R.MUTANTS[name][0](R.PROBE_B, R.PROBE_H, N, R.PROBE_P, R.SEED)
    got, _ = _decoded_mask(Mm, N, False, exact_delta=M)
    for kd, g in got.items():
        assert not torch.equal(g, keep), (name, kd)


# ------------------------------------------------------------------------------------------ (c) decoders
@pytest.mark.parametrize("N,causal", R.PROBE_CASES)
def test_decoders_recover_the_mask_exactly(N, causal):
    keep, region, M = R.probe_reference(N, causal)
    got, qty = _decoded_mask(M, N, causal)
    for kd, g in got.items():
        assert torch.equal(g & region, keep & region), kd
    s = float(DR.scale(R.PROBE_P))
    assert float(((qty - M.double()).abs() * region).max()) < 0.05 * s          # far from the threshold at s / 2


@pytest.mark.parametrize("N,causal", [(70, False), (70, True), (197, True)])
def test_decoders_see_every_flipped_decision(N, causal):
    """Each consumer's mask flipped in EVERY position while the other two keep the true one: the decoded pattern is the exact complement, so
    any single flip moves its own decoded element across the threshold (each decoded element depends on one decision only: the dQ
    probe's delta comes from the forward's o, which a flip in the dQ kernel leaves alone)."""
    keep, region, M = R.probe_reference(N, causal)
    s = float(DR.scale(R.PROBE_P))
    flipped = torch.where(M != 0, torch.zeros_like(M), torch.full_like(M, s))
    for kd in ("fwd", "dq", "dkv"):
        masks = {"fwd": M, "dq": M, "dkv": M, kd: flipped}
        got, qty = _decoded_mask(masks, N, causal, kinds=(kd,), exact_delta=M)
        assert torch.equal(got[kd] & region, ~keep & region), kd
        if kd == "dq":
            assert float(((qty - flipped.double()).abs() * region).max()) < 0.05 * s
    # and one decision at a time, at corners and tile edges
    for (b, h, q, k) in [(0, 0, 0, 0), (1, 1, N - 1, N - 1), (1, 0, N - 1, 0), (0, 1, 32, 31), (1, 1, 64, 63), (0, 0, 65, 64)]:
        one = M.clone()
        one[b, h, q, k] = flipped[b, h, q, k]
        for kd in ("fwd", "dq", "dkv"):
            got, _ = _decoded_mask({"fwd": M, "dq": M, "dkv": M, kd: one}, N, causal, kinds=(kd,), exact_delta=M)
            diff = (got[kd] != keep) & region
            assert int(diff.sum()) == 1 and bool(diff[b, h, q, k]), (kd, b, h, q, k)


# ------------------------------------------------------------------------------------------ (d) self-consistency
def test_mask_equals_the_dropout_contract_at_hand_written_indices():
    p, seed = 0.3, (1 << 40) + 777
    assert seed >= 1 << 32
    s = DR.scale(p)
    # (B, H, N) and (b, h, q, k) by hand; the last four lie at or beyond 2^32 (bh = 16 at N = 16384 starts at exactly 2^32)
    small = R.mask(2, 3, 5, p, seed)
    for (b, h, q, k) in [(0, 0, 0, 0), (0, 0, 0, 4), (0, 0, 4, 0), (0, 2, 3, 1), (1, 0, 0, 0), (1, 2, 4, 4)]:
        idx = ((b * 3 + h) * 5 + q) * 5 + k
        assert float(small[b, h, q, k]) == float(s) * bool(DR.keep(np.array([idx], dtype=np.uint64), seed, p)[0])
    N = 16384
    rows = R.mask_rows([15, 16], N, p, seed, q0=0, q1=N, keys=[0, 1, 70, N - 1])
    for (i, bh, q, kc, k) in [(0, 15, N - 1, 3, N - 1), (1, 16, 0, 0, 0), (1, 16, 0, 1, 1), (1, 16, 8191, 2, 70), (1, 16, N - 1, 3, N - 1)]:
        idx = (bh * N + q) * N + k
        assert (idx >= 1 << 32) == (bh == 16)
        assert float(rows[i, q, kc]) == float(s) * bool(DR.keep(np.array([idx], dtype=np.uint64), seed, p)[0])
    # the high index word matters: the same low word in head 0 decides differently somewhere
    assert not torch.equal(R.mask_rows([16], N, p, seed, 0, 64), R.mask_rows([0], N, p, seed, 0, 64))
    assert abs(float((small != 0).float().mean()) - 0.7) < 0.2 and torch.all(R.mask(1, 2, 7, 0.0, seed) == 1)


@pytest.mark.parametrize("causal", [False, True])
def test_ref64_without_dropout_is_the_oracle_sdpa(causal):
    B, N, H = 2, 45, 2
    qkv = R.r16(R.randn((B * N, 3 * H * 64), 3, 1.5))
    q, k, v = R.split(qkv, B, N, H)
    g = R.heads(R.r16(R.randn((B * N, H * 64), 4)), B, N, H)
    ref = R.ref64(q, k, v, g, None, causal)
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    o = O.sdpa(qd, kd, vd, causal, lowp=False)
    o.backward(g.double())
    for n, t in (("o", o.detach()), ("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        assert R.rel_l2(ref[n], t) < 1e-13, n
    assert R.rel_l2(ref["o"], R.ref64(q, k, v, g, torch.ones(B, H, N, N), causal)["o"]) == 0.0


# ------------------------------------------------------------------------------------------ (e) the kept-query backward (tests/test_gpu_attention_forms.py)
KEPT_33 = [c for c in R.FORM_CASES if c[6] == 33 and 33 < c[1] <= 224]      # (N = nq = 33 has no padded query and one stride)


@pytest.mark.parametrize("c", R.FORM_CASES, ids=R.form_case_id)
def test_online_restatement_is_inside_the_bounds_on_every_form_case(c):
    B, N, H, causal, p, resid, nq = c
    _check_reference_case(R.form_reference(c), B, N, H, causal, sized=False)      # (short sequences and zero-padded d_o: other floors than the matrix)


def test_the_restatement_of_a_kept_case_is_inside_the_bounds():
    """zero-padded d_o: the online restatement sits inside compare's bounds, and its kept forward rows inside those of the kept rows alone"""
    assert len(KEPT_33) >= 5
    for c in (KEPT_33[0], KEPT_33[-1]):
        B, N, H, causal, p, resid, nq = c
        r = R.form_reference(c)
        on = R.restate(*r["in"], None, False, online=True)
        ratios, bad = R.compare({n: on[n] for n in (*R.OUTS, "lse")}, r["ref"], r["floors"])
        assert not bad, (R.form_case_id(c), bad)
        ref_k, rs_k = R.keep_slice(r["ref"], nq), R.keep_slice(r["restate"], nq)
        ratios, bad = R.compare(R.keep_slice(on, nq), ref_k, R.floors(ref_k, rs_k, ("o",)))
        assert not bad, (R.form_case_id(c), bad)
        assert float(r["ref"]["dq"][..., nq:, :].abs().max()) == 0.0        # the reference's own Q rows >= nq are exact zeros


@pytest.mark.parametrize("name", list(R.KEEP_MUTANTS))
def test_compare_rejects_the_planted_mistakes_of_a_kept_backward(name):
    for c in KEPT_33:
        r = R.form_reference(c)
        got = R.keep_mutant_outputs(name, c)
        _, bad = R.compare({n: got[n] for n in (*R.OUTS, "lse")}, r["ref"], r["floors"])
        assert bad, (name, R.form_case_id(c))
        assert any(b.startswith(("dk", "dv")) for b in bad), bad
        print(f"\nMUTANT {name!r}: {R.form_case_id(c)}: {[b for b in bad if b.startswith('dk: rel_l2')][:1] or bad[:1]}")
