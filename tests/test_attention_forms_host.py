"""No GPU: proof that tests/test_gpu_attention_forms.py reaches every attention kernel instantiation a call can launch.  The library's own
vitamd_attention_form (the function its launchers switch on) is swept over every length, mask, residual and kept-query form; each code
it can answer must be the code of a case of _attention_ref.FORM_CASES / MATRIX / PROBE_CASES / SPIKE_CASES / the long-sequence case, and
each tile-templated one at both edges of its tile count.  A dispatch change that creates an unreached instantiation fails here.  Also:
the query's refusals are the entry points' own."""
import ctypes
import re

import pytest

import _abi
import _attention_ref as R

SHAPE, ARG = 1, 2            # VITAMD_ERR_SHAPE, VITAMD_ERR_ARG
NAN = float("nan")
_buf = (ctypes.c_float * 64)()
P = ctypes.addressof(_buf)   # a dummy pointer no refused call dereferences


@pytest.fixture(scope="module")
def L():
    from vitamd import lib
    return lib.load()


@pytest.fixture(scope="module")
def form(L):
    return lambda N, causal, p, resid, nq, bwd: L.vitamd_attention_form(N, int(causal), p, int(resid), nq, int(bwd))


@pytest.fixture(scope="module")
def swept(form):
    """every non-negative code of the sweep"""
    codes = set()
    for N in [*range(1, 1101), 16384]:
        for causal in (0, 1):
            for p in (0.0, 0.3):
                for resid in ((0, 1) if N <= 256 else (0,)):
                    for bwd in (0, 1):
                        codes.add(form(N, causal, p, resid, 0, bwd))
    for N in range(1, 261):
        for nq in range(1, min(N, 130) + 1):
            for bwd in (0, 1):
                codes.add(form(N, 0, 0.0, 0, nq, bwd))
    return {c for c in codes if c >= 0}


# ------------------------------------------------------------------------------------------ the binding
def test_the_query_is_in_header_and_binding_and_the_numbers_agree():
    from vitamd import lib, ops
    header = _abi.header()
    assert _abi.declared()[1]["vitamd_attention_form"] == "int" and "vitamd_attention_form" in lib.SIGNATURES
    assert lib.ABI_VERSION == 9          # additive: the version does not move
    defines = {n: int(v, 0) for n, v in re.findall(r"#define VITAMD_ATTN_(\w+) (0x[0-9a-f]+|\d+)\b", header)}
    for name in ("FWD_SMALL", "FWD_SMALL8", "FWD_LOOP", "FWD_LONG", "BWD_PIPE", "BWD_LOOP", "BWD_LONG"):
        assert defines[name] == getattr(ops, "ATTN_" + name) == getattr(R, name), name
    for name in ("DROP", "CAUSAL", "RES", "KEEP"):
        assert defines[name] == getattr(ops, "ATTN_" + name) == getattr(R, "F_" + name), name
    assert ops.attention_form_fields(R.form_code(R.BWD_PIPE, 7, 3, keep=True)) == (R.BWD_PIPE, 7, 3, R.F_KEEP)


# ------------------------------------------------------------------------------------------ coverage
FAMILY_COUNTS = {R.FWD_SMALL: 56, R.FWD_SMALL8: 12, R.FWD_LOOP: 2, R.FWD_LONG: 2, R.BWD_PIPE: 6 + 21, R.BWD_LOOP: 4, R.BWD_LONG: 2}


def test_the_sweep_finds_the_instantiations_the_dispatch_can_reach(swept):
    """8 tile counts x DROP x CAUSAL x RES less the eight that the eight-wave kernel takes; 4 x RES + 4 KEEP; the pipelined backward 6 plain +
    21 kept (NQT <= min(NT, 4)); DROP alone for attn_fwd_kernel and the long kernels (causal is a run-time argument there)"""
    by_family = {}
    for code in swept:
        by_family.setdefault(code & 0xf, set()).add(code)
    print(f"\n{len(swept)} distinct forms:", {R.FAMILY_NAMES[f]: len(s) for f, s in sorted(by_family.items())})
    assert {f: len(s) for f, s in by_family.items()} == FAMILY_COUNTS
    kept = {c for c in by_family[R.BWD_PIPE] if c & R.F_KEEP}
    assert len(kept) == 21 and {(c >> 4 & 0xf, c >> 8 & 0xf) for c in kept} == {(t, q) for t in range(2, 8) for q in range(1, min(t, 4) + 1)}
    for code in swept:                   # a family that is not templated on a tile count answers none
        assert (code >> 4 & 0xf != 0) == (code & 0xf in R.TILED_FAMILIES), hex(code)
        assert (code >> 8 & 0xf != 0) == (code & 0xf == R.BWD_PIPE), hex(code)


def test_every_form_the_library_can_answer_is_reached_by_a_case(swept, form):
    reached = {}
    for c in R.FORM_CASES:
        for call in R.form_case_calls(c, form):
            reached.setdefault(form(*call), []).append(R.form_case_id(c))
    for call in R.other_case_calls():
        reached.setdefault(form(*call), []).append(f"matrix/probe/spike/long N{call[0]}")
    print(f"\n{len(swept)} distinct forms, {len(R.FORM_CASES)} form cases")
    for code in sorted(swept):
        print(f"  {code:#06x} {R.code_name(code)}: {', '.join(sorted(set(reached.get(code, ['-']))))}")
    assert not R.ONE_EDGE                # an entry needs its reason
    gaps = R.coverage_gaps(swept, form)
    assert not gaps, gaps
    assert set(reached) <= swept         # and no case reaches a form the sweep does not know


def test_every_case_reports_the_code_it_was_chosen_for(form):
    for c in R.FORM_CASES:
        got = [form(*call) for call in R.form_case_calls(c, form)]
        for code in R.FORM_EXPECT[c]:
            assert code in got, (R.form_case_id(c), R.code_name(code), [R.code_name(g) for g in got])
    for c, (fwd, bwd) in zip(R.MATRIX, R.MATRIX_FAMILIES):
        B, N, H, causal, p = c
        assert (form(N, causal, p, False, 0, False) & 0xf, form(N, causal, p, False, 0, True) & 0xf) == (fwd, bwd), R.case_id(c)


def test_dropping_any_one_form_case_leaves_a_form_unreached(swept, form):
    """the table is minimal: every entry is the only one that reaches some form at some edge, so the coverage test notices its loss"""
    for i, c in enumerate(R.FORM_CASES):
        gaps = R.coverage_gaps(swept, form, R.FORM_CASES[:i] + R.FORM_CASES[i + 1:])
        assert gaps, R.form_case_id(c)
    # ... and names it.  Without the ordinary 4-tile ragged case: the RES form of the 4-tile forward (the kept cases at N = 97 still make the
    # full-size calls they are compared with); without a kept one: its (key tiles, query tiles) pair
    for lost, what in (((R.FORM_B, 97, R.FORM_H, False, 0.0, True, 0), "0x4041 attn_fwd_small_kernel<4 tiles, RES>: not run at N = [97]"),
                       ((R.FORM_B, 97, R.FORM_H, False, 0.0, False, 33), "0x8245 attn_bwd_*_pipe_kernel<4 tiles, 2 query tiles, KEEP>: not run at N = [97]")):
        assert lost in R.FORM_CASES
        assert R.coverage_gaps(swept, form, [c for c in R.FORM_CASES if c != lost]) == [what]
    # ... and a form no case reaches at all
    gaps = R.coverage_gaps(swept, form, [c for c in R.FORM_CASES if (c[1] + 31) // 32 != 6])
    assert "0x665 attn_bwd_*_pipe_kernel<6 tiles, 6 query tiles>: no case" in gaps and "0x62 attn_fwd_small8_kernel<6 tiles>: no case" in gaps


def test_the_case_table_follows_its_rules():
    for (B, N, H, causal, p, resid, nq) in R.FORM_CASES:
        assert (B, H) == (R.FORM_B, R.FORM_H) and 1 <= N <= 256 and N in R.edges((N + 31) // 32) and 0 <= nq <= N
        assert not nq or not (causal or p or resid)
    kept_fwd = [(N, nq) for (B, N, H, causal, p, resid, nq) in R.FORM_CASES if nq and N >= 129]
    assert {(N + 31) // 32 for N, nq in kept_fwd} == {5, 6, 7, 8}
    assert {1, 33, 128} <= {nq for N, nq in kept_fwd} and any(nq == N for N, nq in kept_fwd)
    assert any(nq == 128 for (B, N, H, causal, p, resid, nq) in R.FORM_CASES)


# ------------------------------------------------------------------------------------------ refusals
def _entry_points(L, N, causal, p, resid, nq, bwd):
    """the matching entry point with dummy pointers (refused calls only: nothing is launched)"""
    if nq:
        if bwd:
            return L.vitamd_attention_bwd_keep(P, P, P, P, P, P, P, 2, N, 2, 64, nq, None)
        return L.vitamd_attention_fwd_keep(P, P, P, 2, N, 2, 64, nq, None)
    if bwd:
        return L.vitamd_attention_bwd(P, P, P, P, P, P, P, 2, N, 2, 64, causal, p, 7, None)
    if resid:
        return L.vitamd_attention_fwd_resid(P, P, P, P, P, 2, N, 2, 64, causal, p, 7, None)
    return L.vitamd_attention_fwd(P, P, P, 2, N, 2, 64, causal, p, 7, None)


REFUSED = ([(N, c, p, r, 0, b, SHAPE) for N in (0, -1, 16385, 2**30) for c in (0, 1) for p in (0.0, 0.3, 1.0, NAN) for r in (0, 1) for b in (0, 1)]
           + [(N, c, p, 1, 0, 0, SHAPE) for N in (257, 300, 513, 16384) for c in (0, 1) for p in (0.0, 0.3, -0.1, NAN)]       # resid past 256 tokens
           + [(N, c, p, r, 0, b, ARG) for N in (1, 97, 256, 257, 600, 16384) for c in (0, 1) for p in (-0.1, 1.0, 1.5, NAN) for r in ((0, 1) if N <= 256 else (0,)) for b in (0, 1)]
           + [(N, 0, 0.0, 0, nq, b, SHAPE) for N, nq, b in ((128, 1, 0), (257, 1, 0), (32, 1, 1), (225, 1, 1), (197, 129, 1), (197, 198, 0), (197, 198, 1),
                                                              (5, 1, 0), (5, 1, 1), (288, 32, 0), (288, 32, 1), (16385, 1, 0), (16385, 1, 1))])


def test_the_query_refuses_what_the_entry_points_refuse(L, form):
    for (N, causal, p, resid, nq, bwd, want) in REFUSED:
        if bwd and resid:
            continue                      # the backward has no residual form: the argument is ignored there (asked below)
        assert _entry_points(L, N, causal, p, resid, nq, bwd) == want, (N, causal, p, resid, nq, bwd)
        assert form(N, causal, p, resid, nq, bwd) == -want, (N, causal, p, resid, nq, bwd)
    # the backward ignores resid, a refused shape included
    for N in (0, 97, 300, 16385):
        assert form(N, 0, 0.0, 1, 0, 1) == form(N, 0, 0.0, 0, 0, 1)
    # nq < 0 names nothing; a kept form takes no mask and no residual epilogue, and its shape still answers first
    assert form(197, 0, 0.0, 0, -1, 0) == -SHAPE
    for bad in ((1, 0.0, 0), (0, 0.3, 0), (0, 0.0, 1), (0, NAN, 0)):
        assert form(197, *bad, 33, 0) == -ARG and form(197, *bad, 33, 1) == -ARG
        assert form(288, *bad, 33, 0) == -SHAPE and form(32, *bad, 1, 1) == -SHAPE


def test_the_query_agrees_with_keep_forms(L, form):
    for N in range(0, 300):
        for nq in (1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, N - 1, N, N + 1):
            served = L.vitamd_attention_keep_forms(N, nq)
            if nq <= 0:
                assert served == 0
                continue
            assert bool(served & 1) == (form(N, 0, 0.0, 0, nq, 0) >= 0) and bool(served & 2) == (form(N, 0, 0.0, 0, nq, 1) >= 0), (N, nq)
            assert served == ((129 <= N <= 256 and nq <= N) * 1 | (33 <= N <= 224 and nq <= min(N, 128)) * 2), (N, nq)
