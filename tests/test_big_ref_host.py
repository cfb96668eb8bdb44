"""tests/_big_ref.py without a GPU: the bands cover every boundary of every case of tests/test_gpu_big_operands.py, the chunked comparison finds a
single changed element wherever it is, the device reference (run here on the CPU, at small shapes) agrees with _gemm_ref's arithmetic and a
damaged one does not, and the plans the big cases assert are the ones the library answers."""
import pytest
import torch

import _big_ref as B
import _gemm_ref as G
from _gemm_ref import BF16, GUARD

ALL_CASES = B.NT_CASES + [B.DROPOUT_CASE]


def _in_bands(bs, row):
    return any(lo <= row < hi for lo, hi in bs)


@pytest.mark.parametrize("case", ALL_CASES, ids=B.nt_id)
def test_bands_hold_every_boundary_row(case):
    bs = B.nt_bands(case)
    assert bs[0][0] == 0 and bs[-1][1] == case.M and all(lo < hi for lo, hi in bs)
    assert all(a[1] < b[0] for a, b in zip(bs, bs[1:])), bs                           # merged: no row is checked twice
    assert _in_bands(bs, B.BAND - 1) and _in_bands(bs, case.M - B.BAND)
    esz = 4 if case.epi in G.F32_OUT else 2
    for what, row_bytes in (("A", case.K * 2), ("out", case.ldo * esz)):
        total = case.M * row_bytes
        for byte in (2 ** 31, 2 ** 32):
            if byte < total:
                row = byte // row_bytes
                assert row * row_bytes <= byte < (row + 1) * row_bytes
                assert _in_bands(bs, row), (what, byte, row, bs)
                assert B.boundary_rows(case)[(what, byte)] == row
    landing = 2 ** 31 // (case.ldo * esz)                                                 # where a store sent to offset 2^31 of `out` lands
    if landing < case.M:
        assert _in_bands(bs, landing), (landing, bs)


def test_every_case_crosses_the_size_it_is_named_for():
    size = lambda c, what: c.M * B.nt_spans(c)[what]
    by = {c.name: c for c in ALL_CASES}
    for name in ("a-bias", "a-gelu", "a-dmul", "a-dmul-n8192", "a-bias-seam320"):
        assert 2 ** 31 < size(by[name], "out") < 2 ** 32 and size(by[name], "A") < 2 ** 31
    assert size(by["b-bias"], "out") > 2 ** 32
    assert 2 ** 31 < size(by["c-bias-A2G"], "A") < 2 ** 32 and size(by["c-bias-A4G"], "A") > 2 ** 32
    for name in ("d-resid", "d-f32", "d-dropout"):
        assert size(by[name], "out") > 2 ** 32
    for c in ALL_CASES:                                                                   # masked stores exist: ragged rows and (at N = 8200) ragged columns
        assert c.M % 256 == 77 and c.M % 320 != 0 and c.N * c.K * 2 < 2 ** 31
        assert B.nt_bytes_needed(c) < 24 * B.GIB
    assert by["a-bias"].N % 256 == 8 and by["a-dmul-n8192"].N % 256 == 0 and by["a-dmul-n8192"].ldo > by["a-dmul-n8192"].N


def test_flat_and_row_bands_of_the_streaming_cases():
    for n, marks in ((2 ** 31 + 11, [2 ** 29, 2 ** 30, 2 ** 31]), (2 ** 32 + 4096, [2 ** 30, 2 ** 31, 2 ** 32])):
        bs = B.flat_bands(n, marks)
        assert all(_in_bands(bs, m) and _in_bands(bs, m - 1) for m in marks) and bs[0][0] == 0 and bs[-1][1] == n
    bs = B.bands(2 ** 21 + 5, [2 ** 19, 2 ** 20, 2 ** 21])
    assert all(_in_bands(bs, r) and _in_bands(bs, r - 1) for r in (2 ** 19, 2 ** 20, 2 ** 21))


def test_row_chunks_tile_the_rows_within_the_element_budget():
    for M, N, K in ((B.M17, 8200, 128), (B.M19, 256, 4096), (5, 7, 0)):
        ch = B.row_chunks(M, N, K)
        assert ch[0][0] == 0 and ch[-1][1] == M and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all((r1 - r0) * max(N, K) <= B.CHUNK_ELEMS for r0, r1 in ch)
        assert B.CHUNK_ELEMS * 4 <= B.GIB


def test_chunked_comparison_reports_one_changed_element_in_a_later_chunk():
    want = B.sentinel(40, 16, BF16, "cpu")
    want[GUARD:-GUARD, :12] = torch.arange(36 * 12, dtype=torch.int16).view(36, 12)
    B.assert_equal_chunked("same", want.clone(), want, elems=64)                          # 4 rows per chunk: 10 chunks
    for r, col in ((0, 0), (3, 15), (4, 0), (21, 7), (39, 15)):
        got = want.clone()
        got[r, col] ^= 1
        with pytest.raises(AssertionError) as e:
            B.assert_equal_chunked("one bit", got, want, elems=64)
        msg = str(e.value)
        assert f"chunk {r // 4} " in msg and "1 elements differ" in msg and f"buffer row {r} " in msg and f"column {col}:" in msg, msg


SMALL = [B.BigNt("s-bias", G.EPI_BIAS_BF16, 1100, 24, 64, 32, (0,)), B.BigNt("s-gelu", G.EPI_GELU, 1100, 264, 128, 272, (0,)),
         B.BigNt("s-dmul", G.EPI_DMUL, 1100, 24, 64, 32, (0,)), B.BigNt("s-resid", G.EPI_RESID_F32, 1100, 24, 64, 32, (0,)),
         B.BigNt("s-f32", G.EPI_F32, 1100, 24, 64, 32, (0,))]


@pytest.mark.parametrize("case", SMALL, ids=B.nt_id)
def test_device_reference_agrees_with_the_cpu_arithmetic_and_a_damaged_one_does_not(case, monkeypatch):
    monkeypatch.setattr(B, "CHUNK_ELEMS", 4096)                                           # several row chunks at this size
    p = B.nt_problem(case, "cpu")
    assert p.units < G.EXACT
    bs = B.check_reference_bands(p)
    assert bs == [(0, 512), (588, 1100)]
    # the whole reference against _gemm_ref's formulas, and its frame
    o, o2 = B.cpu_rows(case, p.a, p.b, p.bias, p.aux)
    assert torch.equal(p.want[GUARD:-GUARD, :case.N], o)
    sent = G.SENT16 if p.want.dtype == torch.int16 else G.SENT32
    assert bool((p.want[:GUARD] == sent).all()) and bool((p.want[-GUARD:] == sent).all()) and bool((p.want[:, case.N:] == sent).all())
    if case.epi == G.EPI_GELU:
        assert torch.equal(p.want2[GUARD:-GUARD, :case.N], o2)
        inside = G.in_table(G.u16(o))
        assert 0.9 < inside.mean() < 1.0                                                  # both sides of the table's range occur
    if case.epi == G.EPI_DMUL:
        stored = p.want[GUARD:-GUARD, :case.N].view(BF16).double()
        assert torch.equal(p.colsum_want.double(), p.colsum0.double() + stored.sum(0))
    p.want[GUARD + 600, 3] ^= 1                                                           # one bit, inside the last band
    with pytest.raises(AssertionError):
        B.check_reference_bands(p)


def test_exactness_bound_is_asserted_on_the_reference():
    with pytest.raises(AssertionError, match="not below 2\\^24"):
        B.nt_problem(B.BigNt("too-deep", G.EPI_F32, 8, 8, 2 ** 22, 8, (0,)), "cpu")


def test_gelu_tolerance_stays_inside_the_logical_region_and_outside_the_table():
    M, N, ld = 6, 8, 12
    pre = B.sentinel(M + 2 * GUARD, ld, BF16, "cpu")
    vals = torch.tensor([0.5, 9.0, 2.0 ** -14, -12.0, 1.0, 0.0, -3.0, 7.5]).to(BF16).view(torch.int16)      # inside the table: 0.5, 1, -3, 7.5
    pre[GUARD:GUARD + M, :N] = vals
    want2 = pre.clone()
    settle = B.gelu_out2_settle(pre, M, N)
    for (r, col), ok in (((GUARD, 1), True), ((GUARD + 5, 3), True), ((GUARD, 0), False), ((GUARD + 2, 7), False), ((0, 1), False), ((GUARD, N + 1), False),
                         ((GUARD + M, 1), False)):
        got = want2.clone()
        got[r, col] += 1                                                                  # one unit in the last place
        if ok:
            B.assert_equal_chunked("tolerated", got, want2, settle=settle)
        else:
            with pytest.raises(AssertionError):
                B.assert_equal_chunked("not tolerated", got, want2, settle=settle)
    got = want2.clone()
    got[GUARD, 1] += 2                                                                    # two units: never
    with pytest.raises(AssertionError):
        B.assert_equal_chunked("two ulps", got, want2, settle=settle)


def test_tn_edge_is_the_guard_of_the_header():
    assert B.TN_MAX_R == 262079
    assert B.tn_guard_accepts(B.TN_MAX_R, B.TN_BIG_LD) and not B.tn_guard_accepts(B.TN_MAX_R + 1, B.TN_BIG_LD)
    assert (B.TN_MAX_R + 64) * B.TN_BIG_LD * 2 < 2 ** 31 <= (B.TN_MAX_R + 65) * B.TN_BIG_LD * 2
    p = B.tn_problem(300, "L", "cpu")
    l, r = p.lbuf[:, p.loff:p.loff + B.TN_PQ].float(), p.rbuf[:, p.roff:p.roff + B.TN_PQ].float()
    assert torch.equal(p.want_ovw, l.t() @ r) and torch.equal(p.want_acc, p.init + l.t() @ r) and torch.equal(p.colsum_want, p.colsum0 + l.sum(0))
    assert bool(torch.isnan(p.lbuf[:, :p.loff].float()).all()) and bool(torch.isnan(p.lbuf[:, p.loff + B.TN_PQ:].float()).all())
    assert (p.ldl, p.ldr) == (4096, 128) and B.tn_problem(8, "R", "cpu").ldr == 4096


@pytest.mark.parametrize("case", ALL_CASES, ids=B.nt_id)
def test_plans_of_the_big_cases(case):
    """vitamd_gemm_nt_plan needs no GPU (256 CUs are assumed without one, which is what an MI355X has): every tile code of every big case plans the
    form its case is here for - the form of its full-height row panels."""
    from vitamd import lib
    L = lib.load()
    for tile in case.tiles:
        plan = L.vitamd_gemm_nt_plan(case.M, case.N, case.K, case.ldo, case.epi, tile)
        assert B.form_ok(case, tile, plan), (case.name, tile, hex(plan))
    assert not B.form_ok(case, case.tiles[0], -1)
