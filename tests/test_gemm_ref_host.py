"""CPU checks of tests/_gemm_ref.py for every parametrisation of tests/test_gpu_gemm_edges.py (the case lists are imported from there, so the
two files cannot drift apart): the bf16 rounding helper against torch's cast, the 2^24 exactness bounds, the share of GELU inputs inside the
table range, NaN padding that never reaches a reference, and the checks themselves - they pass on the reference and fail on a damaged copy."""
import numpy as np
import pytest
import torch

import _gemm_ref as G
import test_gpu_gemm_edges as E

BF16 = torch.bfloat16


def test_bf16_rne_helper_equals_the_torch_cast_on_every_upper_half_and_tie_pattern():
    hi = np.arange(65536, dtype=np.int64)
    lows = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], dtype=np.int64)       # exact, just above, below the tie, the tie, above it, top
    u = ((hi[:, None] << 16) | lows[None, :]).astype(np.uint32)
    f = u.view(np.float32)
    want = G.u16(G.bits(torch.from_numpy(f.copy()).to(BF16)))
    finite = np.isfinite(f) & (((want >> 7) & 0xff) != 0xff)                                 # the helper's domain: finite, rounding stays finite
    got = G.bf16_rne_exact(f[finite].astype(np.float64)) & 0xffff
    assert finite.sum() > 65000 * 6 - 2048 * 6
    assert np.array_equal(got, want[finite])
    # and r16 is that cast
    x = torch.from_numpy(f[finite].copy())
    assert np.array_equal(G.u16(G.bits(G.r16(x).to(BF16))), want[finite])


def test_case_lists_cover_what_the_issue_asks_for():
    small = E.NT_SMALL_CASES
    assert {c.tile for c in small} == {128, 256, 320, 2048, 4096} and {c.epi for c in small} == set(range(8))
    assert {c.M for c in small} == {1, 255, 257, 321, 600} and {c.K for c in small} == {64, 128, 192}
    assert {c.N for c in small} == {4, 260, 264, 512, 520}
    assert {c.ldo - c.N for c in small} == {0, 4, 8}
    for tile in E.NT_TILES:
        for epi in range(8):
            mine = [c for c in small if c.tile == tile and c.epi == epi]
            assert any(c.M % 64 for c in mine)                                               # a ragged M
            assert any(c.N % 8 == 0 and c.N % 256 for c in mine)                             # a ragged N on the row epilogue
            assert any(c.N % 8 == 4 for c in mine)                                           # the direct epilogue (or its refusal)
            assert any(c.ldo > c.N for c in mine)
            ok = [c for c in mine if E.nt_expected_plan(c) is not None]
            if tile in (128, 256) or (tile == 320 and epi in E.TALL_EPIS) or (tile in (2048, 4096) and epi in E.SEAM_EPIS):
                assert ok and any(c.ldo > c.N and c.M % 64 for c in ok), (tile, epi)         # the form runs this epilogue: at least one case is not a refusal
            else:
                assert not ok, (tile, epi)
    big = E.NT_BIG_CASES
    assert all(((c.M + 255) // 256) * ((c.N + 255) // 256) >= 192 and c.M > 256 * 64 and c.K == 64 for c in big)
    assert {c.N for c in big} == {776, 772} and {c.tile for c in big} == {0, 1024}
    assert {c.epi for c in big} == set(range(8))
    assert {c.epi for c in big if c.N == 772} == {G.EPI_RESID_F32, G.EPI_PATCH_F32, G.EPI_DGELU, G.EPI_DMUL, G.EPI_F32}
    assert E.SKINNY_MS == (1, 15, 16, 17, 33, 48, 49, 64) and {(m + 15) // 16 for m in E.SKINNY_MS} == {1, 2, 3, 4}
    assert set(E.SKINNY_NK) == {(4, 64), (260, 64), (1000, 320), (776, 192), (68, 1088), (2304, 768)}
    tn = E.TN_CASES
    assert {c.R for c in tn} == {1, 63, 100, 1000} and {c.P for c in tn} == {100, 260, 768} and {c.Q for c in tn} == {64, 258, 264}
    assert {c.ldo - c.Q for c in tn} >= {0, 4, 3} and {c.splits for c in tn} == {0, 1, 3} and {c.accumulate for c in tn} == {0, 1}
    assert any(c.P % 8 for c in tn) and any(c.Q % 4 for c in tn) and any(c.ldo % 4 for c in tn) and any(c.Q % 4 and c.ldo % 4 == 0 for c in tn)


def _damaged(buf, logical, inside=True):
    """a copy of an expected buffer with ONE element changed by one unit in the last place: inside the logical region or in the sentinel frame"""
    out = buf.clone()
    where = (logical if inside else ~logical).nonzero()
    r, c = where[len(where) * 2 // 3].tolist()
    out[r, c] += 1
    return out


def _nt_checks_pass_and_bite(case, sides=(True, False)):
    p = G.nt_problem(case)                                        # asserts the exactness bounds, the table share and NaN-free references
    ref = G.nt_reference_output(p)
    stats = G.nt_check(p, ref)
    if case.epi == G.EPI_DGELU:
        assert stats["dgelu_max_ulps"] == 0.0
    for inside in sides:
        if not inside and not bool((~p.logical).any()):
            continue
        bad = G.nt_reference_output(p)
        bad.out = _damaged(bad.out, p.logical, inside)
        if case.epi == G.EPI_DGELU and inside:
            bad.out = p.want.clone()
            where = p.logical.nonzero()[len(p.logical.nonzero()) // 2].tolist()
            bad.out[where[0], where[1]] += 2                      # one ulp is the tolerance of the formula path; two are not (and the colsum no longer matches)
        if case.epi in (G.EPI_GELU_DG,) and inside:
            bad.out = torch.where(p.logical, bad.out + 2, bad.out)
        with pytest.raises(AssertionError):
            G.nt_check(p, bad)
    if p.colsum_want is not None:
        bad = G.nt_reference_output(p)
        bad.colsum = bad.colsum.clone()
        bad.colsum[p.case.N // 2] += 1
        with pytest.raises(AssertionError):
            G.nt_check(p, bad)
    return p


@pytest.mark.parametrize("case", [c for c in E.NT_SMALL_CASES if c.tile == 256], ids=G.nt_id)
def test_nt_small_references(case):
    """the references do not depend on the tile code: the 56 (epilogue, shape) pairs, once"""
    same = [c for c in E.NT_SMALL_CASES if c[1:] == case[1:]]
    assert {c.tile for c in same} == set(E.NT_TILES)
    p = _nt_checks_pass_and_bite(case)
    if case.epi in (G.EPI_GELU, G.EPI_GELU_DG):
        assert p.stats["gelu_inside_share"] >= 0.9 and not bool(p.inside.all())
    if case.epi in (G.EPI_DGELU, G.EPI_DMUL):
        assert p.stats["colsum_units"] < G.EXACT
    for aux in (p.aux,):
        if aux is not None and case.ldo > case.N:
            assert bool(torch.isnan(aux[:, case.N:].float()).all())                          # the padding IS poisoned ...


@pytest.mark.parametrize("case", E.NT_BIG_CASES, ids=G.nt_id)
def test_nt_big_references(case):
    p = _nt_checks_pass_and_bite(case, sides=(False,))            # (the element checks bite on the small cases: same code)
    if case.epi in (G.EPI_DGELU, G.EPI_DMUL):
        assert p.stats["colsum_units"] < G.EXACT


@pytest.mark.parametrize("N,K,ldo,M", E.TAIL_SHAPES)
def test_nt_tail_split_references(N, K, ldo, M):
    """at the M a 256-CU part gives (the GPU test searches it through vitamd_gemm_nt_plan)"""
    p = G.nt_problem(G.NtCase(0, G.EPI_RESID_F32, M, N, K, ldo))
    G.nt_check(p, G.nt_reference_output(p))


def test_nt_expected_plan_restates_the_header():
    c = lambda tile, epi, M=257, N=512, K=128, ldo=512: G.NtCase(tile, epi, M, N, K, ldo)
    assert E.nt_expected_plan(c(128, 5)) == 1 | 128 << 8 and E.nt_expected_plan(c(256, 4)) == 2 | 256 << 8
    assert E.nt_expected_plan(c(320, 4)) is None and E.nt_expected_plan(c(320, 5)) is None and E.nt_expected_plan(c(320, 7)) == 2 | 320 << 8
    assert E.nt_expected_plan(c(2048, 0)) == 5 | 256 << 8 and E.nt_expected_plan(c(2048, 0, K=192)) is None and E.nt_expected_plan(c(2048, 3)) is None
    assert E.nt_expected_plan(c(4096, 7)) == 4 | 256 << 8 and E.nt_expected_plan(c(4096, 7, N=520, ldo=520)) is None
    assert E.nt_expected_plan(c(4096, 0, K=64)) is None and E.nt_expected_plan(c(4096, 0, N=260, ldo=260)) is None
    assert E.nt_expected_plan(c(4096, 1, ldo=516)) is None and E.nt_expected_plan(c(256, 0, K=96)) is None


@pytest.mark.parametrize("N,K", E.SKINNY_NK)
def test_skinny_references(N, K):
    gelu = []
    for M in E.SKINNY_MS:
        for epi in G.SKINNY_EPIS:
            p = G.skinny_problem(M, N, K, epi)
            ref = G.skinny_reference_output(p)
            G.skinny_check(p, ref)
            ref.out = _damaged(ref.out, p.logical, inside=M % 2 == 0)
            with pytest.raises(AssertionError):
                G.skinny_check(p, ref)
            if epi == G.EPI_GELU:
                gelu.append(p)
    share, outside = G.gelu_share(gelu)                       # one GELU case = one (N, K) over its eight M (M = 1, N = 4 has four elements)
    assert share >= 0.9 and outside >= 1, (share, outside)
    assert all(not bool(q.inside.all()) for q in gelu)        # in fact every single call has its planted zero


def test_skinny_split_candidates():
    assert G.skinny_ks_candidates(1088, 6) == [192] and G.skinny_ks_candidates(320, 2) == [192, 256]
    assert G.skinny_ks_candidates(64, 1) == [64] and G.skinny_ks_candidates(768, 6) == [128]
    for K, s in ((1088, 6), (320, 2)):
        assert all(K - (s - 1) * ks < ks for ks in G.skinny_ks_candidates(K, s))


@pytest.mark.parametrize("case", E.TN_CASES, ids=G.tn_id)
def test_tn_references(case):
    p = G.tn_problem(case)                                    # asserts the bounds and that no NaN of the padding reached a reference
    assert bool(torch.isnan(p.lbuf[:, :G.TN_LOFF].float()).all()) and bool(torch.isnan(p.lbuf[:, G.TN_LOFF + case.P:].float()).all())
    assert bool(torch.isnan(p.rbuf[:, :G.TN_ROFF].float()).all()) and bool(torch.isnan(p.rbuf[:, G.TN_ROFF + case.Q:].float()).all())
    for acc in (0, 1):
        before, after = G.tn_frames(p, acc)
        G.tn_check("ref", p, after, after)
        bad = after.clone()
        bad[case.P - 1, case.Q - 1] += 1
        with pytest.raises(AssertionError):
            G.tn_check("damaged", p, bad, after)
        bad = after.clone()
        bad[case.P - 1, case.ldo - 1 if case.ldo > case.Q else case.Q - 1] = torch.tensor(float("nan")).view(torch.int32)
        with pytest.raises(AssertionError):
            G.tn_check("leaked", p, bad, after)
        assert int((before != after).sum()) <= case.P * case.Q
