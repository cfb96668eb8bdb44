"""No GPU: proof that tests/test_gpu_decode_edges.py can fail.  (a) on every case of that file restate() - the contract's function in fp32,
in groups of 8 to 128 keys and chunks of 128 to 16384 - returns V[j*] bit for bit on the spike cases and sits inside the per-row bound
on the random cases; (b) the condition the spike cases rest on holds for every one of them; (c) each mutation of _decode_ref.MUTANTS
fails a spike case or breaks the random-data bound, and the case that kills it is printed; (d) ref64() agrees with the oracle's sdpa,
and kv_frame() with hand-written expectations."""
import pytest
import torch

import _decode_ref as R
import _gemm_ref as G
import vit_oracle as O

RANDOM_FLAT = [(B, H, Lmax, n) for (B, H, Lmax, ns) in R.RANDOM_CASES for n in ns]


# ------------------------------------------------------------------------------------------ (a) the restatement passes
@pytest.mark.parametrize("table", R.SPIKE_TABLES, ids=lambda t: "B{}-H{}-Lmax{}".format(*t))
def test_restatement_returns_the_spiked_value_row_bit_for_bit(table):
    cases = [c for c in R.SPIKE_CASES if c[:3] == table]
    assert len(cases) > 100
    for c in cases:
        B, H, Lmax, n, j = c
        inp = R.spike_inputs(c)
        for group, chunk in R.GROUPS:
            bad = R.check_spike(R.restate(*inp, n, H, group, chunk).to(R.BF16), inp[2][:, :, j])
            assert not bad, (R.spike_id(c), group, chunk, bad)


def test_case_tables_cover_every_edge_the_issue_names():
    for Lmax in (640, 1000):
        ns = R.spike_ns(Lmax)
        assert set(range(1, 41)) <= set(ns) and Lmax in ns and max(ns) == Lmax
        for k in range(1, Lmax // 128 + 1):
            assert {128 * k - 1, 128 * k} <= set(ns) and (128 * k + 1 in ns or 128 * k + 1 > Lmax)
    assert R.spike_js(300) == [0, 256, 299] and R.spike_js(257) == [0, 256] and R.spike_js(256) == [0, 128, 255] and R.spike_js(1) == [0]
    assert {t[2] for t in R.SPIKE_TABLES} == {640, 1000} and {t[:2] for t in R.SPIKE_TABLES} == {(1, 2), (2, 3)}
    assert R.SPIKE_LIMIT[0] * R.SPIKE_LIMIT[1] == 65535


@pytest.mark.parametrize("B,H,Lmax,n", RANDOM_FLAT, ids=[R.random_id(*c) for c in RANDOM_FLAT])
def test_restatement_is_inside_the_random_data_bound(B, H, Lmax, n):
    r = R.random_reference(B, H, Lmax, n)
    print(f"\nFLOOR {R.random_id(B, H, Lmax, n)}: " + ", ".join(f"group {g} chunk {c}: {f:.3e}" for (g, c), f in r["floors"].items())
          + f"; bound {r['bound']:.3e}")
    # one bf16 rounding of each element: at most 2^-8 of its magnitude (half a unit in the last of 8 bits), and not zero (a restatement
    # that lost its rounding would read ~1e-7)
    if n == 1:                                                        # one key: o is its value row, and a zero floor admits only a zero error
        assert all(f == 0.0 for f in r["floors"].values()), r["floors"]
    else:
        assert all(2.0 ** -13 < f <= 2.0 ** -8 * 1.01 for f in r["floors"].values()), r["floors"]
    assert set(g for g, _ in r["floors"]) >= {8, 128}
    assert r["bound"] == R.MARGIN * max(r["floors"].values())
    inp = R.random_inputs(B, H, Lmax, n)
    for group, chunk in ((8, 128), (128, 128)):                       # the margin: no grouping uses more than three quarters of the bound
        worst, bad = R.check_random(R.restate(*inp, n, H, group, chunk), r)
        assert not bad and worst <= 0.75 * r["bound"], (group, chunk, worst, bad)
    nan = torch.full_like(r["ref"], float("nan"))
    assert R.check_random(nan, r)[1] and R.check_random(r["ref"] * (1 + 3 * r["bound"] + 1e-6), r)[1]


# ------------------------------------------------------------------------------------------ (b) the spike condition
def test_spike_weights_underflow_in_every_case():
    worst = float("-inf")
    for c in R.SPIKE_CASES + [R.SPIKE_LIMIT]:
        m = R.spike_log2_margin(c)
        assert m < R.SPIKE_UNDERFLOW, (R.spike_id(c), m)
        worst = max(worst, m)
    print(f"\nSPIKE largest other weight over {len(R.SPIKE_CASES) + 1} cases: 2^{worst:.1f} of the spike's")
    # and the figure the module quotes: fp32 holds nothing between 0 and 2^-149
    assert float(torch.exp2(torch.tensor(R.SPIKE_UNDERFLOW, dtype=torch.float32))) == 0.0
    assert float(torch.exp2(torch.tensor(-149.0, dtype=torch.float32))) > 0.0


def test_spike_limit_case_on_the_restatement():
    B, H, Lmax, n, j = R.SPIKE_LIMIT
    inp = R.spike_inputs(R.SPIKE_LIMIT)
    assert not R.check_spike(R.restate(*inp, n, H).to(R.BF16), inp[2][:, :, j])


# ------------------------------------------------------------------------------------------ (c) mutants
def _first_spike_kill(name):
    for c in R.SPIKE_CASES:
        inp = R.spike_inputs(c)
        bad = R.check_spike(R.mutant_output(name, inp, c[3], c[1]).to(R.BF16), inp[2][:, :, c[4]])
        if bad:
            return R.spike_id(c), bad[0]
    return None


def _first_random_kill(name):
    for (B, H, Lmax, n) in sorted(RANDOM_FLAT, key=lambda c: c[0] * c[1] * c[3]):      # cheapest first
        _, bad = R.check_random(R.mutant_output(name, R.random_inputs(B, H, Lmax, n), n, H), R.random_reference(B, H, Lmax, n))
        if bad:
            return R.random_id(B, H, Lmax, n), bad[0]
    return None


@pytest.mark.parametrize("name", list(R.MUTANTS))
def test_every_mutant_is_rejected(name):
    spike, rand = _first_spike_kill(name), _first_random_kill(name)
    print(f"\nMUTANT {name!r}: spike {spike[0] + ': ' + spike[1] if spike else 'passes every case'}; "
          f"random {rand[0] + ': ' + rand[1] if rand else 'passes every case'}")
    assert spike is not None or rand is not None, f"mutant '{name}' passes every check"


def test_mutant_list_holds_what_the_issue_lists():
    assert len(R.MUTANTS) >= 11 and len({f for f, _ in R.MUTANTS.values()}) == len(R.MUTANTS)


# ------------------------------------------------------------------------------------------ (d) self-consistency
def test_ref64_is_the_oracle_sdpa_of_the_last_row():
    B, H, Lmax, n = 2, 3, 50, 37
    qkv, kc, vc = R._base(B, H, Lmax, 11, False)
    kc, vc = R.fill_past(kc, vc, n)
    q = qkv[:, :H * 64].double().view(B, H, 1, 64)
    o = O.sdpa(q, kc[:, :, :n].double(), vc[:, :, :n].double(), False, lowp=False)
    ref = R.ref64(qkv, kc, vc, n, H)
    assert float((ref - o.reshape(B, H * 64)).norm() / o.norm()) < 1e-13
    assert float(R.row_errors(R.restate(qkv, kc, vc, n, H), ref).max()) < 2.0 ** -8


def test_kv_frame_drops_rows_outside_the_cache():
    B, T, H, Lmax = 2, 5, 3, 8
    qkv = R.randn_bf16((B * T, 3 * H * 64), 5)
    src = G.bits(qkv).view(B, T, 3, H, 64)
    for length, landed in ((Lmax - 2, {Lmax - 2: 0, Lmax - 1: 1}), (-2, {0: 2, 1: 3, 2: 4}), (1, {1: 0, 2: 1, 3: 2, 4: 3, 5: 4})):
        for want, which in zip(R.kv_frame(qkv, B, T, H, Lmax, length), (1, 2)):
            G.assert_untouched("guards", torch.cat([want[:G.GUARD], want[-G.GUARD:]]))
            body = want[G.GUARD:-G.GUARD].view(B, H, Lmax, 64)
            for pos in range(Lmax):
                if pos in landed:
                    assert torch.equal(body[:, :, pos], src[:, landed[pos], which]), (length, pos)
                else:
                    G.assert_untouched(f"position {pos}", body[:, :, pos].reshape(-1, 64))
