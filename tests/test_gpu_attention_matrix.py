"""Attention under dropout and causal masks in every kernel form, against tests/_attention_ref.py (fp64 reference, bf16 floor from the
restatement, worst 32-row tile next to the global rel-L2; tests/test_attention_ref_host.py proves on the CPU that these checks fail for
ten listed mistakes).

Which kernels a case reaches is not restated here: vitamd_attention_form (include/vitamd.h, VITAMD_ATTN_*) answers with the function the
launchers switch on, test_attention_matrix asserts of each case the family _attention_ref.MATRIX_FAMILIES lists for it (dropout with 5-8
tiles leaves the eight-wave forward for the four-wave one, dropout or causal with 2-7 tiles the pipelined backward for the plain loops),
and tests/test_gpu_attention_forms.py runs every instantiation.
Every dropout case uses a seed with bit 40 set, so the high seed word takes part."""
import pytest
import torch

import _attention_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _run(qkv, d_o, B, N, H, causal, drop, dbias=None):
    """-> (o, lse, dqkv) on the device"""
    from vitamd import ops
    qd = qkv.to("cuda", BF16)
    o, lse = ops.attention_fwd(qd, B, N, H, causal, dropout=drop)
    dqkv = ops.attention_bwd(qd, o, lse, d_o.to("cuda", BF16), B, N, H, causal, dbias=dbias, dropout=drop)
    return o, lse, dqkv


def _hold_to_bounds(got, r, N, record_property):
    """the bounds of _attention_ref.compare: 1.5 x the global floor, 2 x the worst-tile floor, lse 1e-6; N = 1: dq / dk by their residue"""
    fl = r["floors"] if N > 1 else {n: r["floors"][n] for n in ("o", "dv")}
    ratios, bad = R.compare({n: got[n] for n in (*fl, "lse")}, r["ref"], fl)
    if N == 1:
        bad += R.one_key_residue(got, r["in"])
    for n, (g, t) in ratios.items():
        record_property(f"{n}_over_floor", round(g, 4) if n != "lse" else g)
        record_property(f"{n}_tile_over_tile_floor", round(t, 4) if n != "lse" else t)
    print("ratios (global / floor, worst tile / tile floor):", {n: (round(g, 3), round(t, 3)) if n != "lse" else g for n, (g, t) in ratios.items()})
    for t in got.values():
        assert bool(torch.isfinite(t).all())
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 3.1 numeric matrix
@pytest.mark.parametrize("c", R.MATRIX, ids=R.case_id)
def test_attention_matrix(hip, c, record_property):
    from vitamd import ops
    B, N, H, causal, p = c
    fwd, bwd = R.MATRIX_FAMILIES[R.MATRIX.index(c)]
    assert ops.attention_form(N, causal, p) & 0xf == fwd and ops.attention_form(N, causal, p, backward=True) & 0xf == bwd
    qkv, d_o = R.matrix_inputs(c)
    r = R.matrix_reference(c)
    drop = (p, R.SEED)
    b0 = 1.0 if N <= 512 else 0.0                                                   # the sums are ADDED; the long kernels are checked from zero, as in test_attention_long_sequences
    dbias = torch.full((3 * H * 64,), b0, device="cuda")
    o, lse, dqkv = _run(qkv, d_o, B, N, H, causal, drop, dbias)
    assert R.rel_l2(dbias.cpu() - b0, dqkv.float().cpu().sum(0)) < 1.0e-6           # fused QKV-bias gradient = column sums of what was stored
    _hold_to_bounds(R.kernel_outputs(o.cpu(), lse.cpu(), dqkv.cpu(), B, N, H), r, N, record_property)
    o2, lse2, dqkv2 = _run(qkv, d_o, B, N, H, causal, drop)                         # same seed: bit-identical
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)
    if p > 0:                                                                       # another seed: another mask, the same lse
        o3, lse3, dqkv3 = _run(qkv, d_o, B, N, H, causal, (p, R.SEED + 1))
        other = not torch.equal(R.mask(B, H, N, p, R.SEED + 1) * R.allowed(N, causal), r["M"] * R.allowed(N, causal))   # N = 1 has four decisions
        assert other or N == 1
        assert torch.equal(o, o3) != other and torch.equal(dqkv, dqkv3) != other and torch.equal(lse, lse3)


# ------------------------------------------------------------------------------------------ 3.2 the mask, bit for bit
def _probe_fwd(B, N, H, causal, drop, blocks):
    """{j: keep [B, H, N, cols]} as the forward applies it"""
    from vitamd import ops
    out = {}
    for j in blocks:
        qkv, _ = R.probe_inputs("fwd", B, N, H, j)
        o, _ = ops.attention_fwd(qkv.to("cuda", BF16), B, N, H, causal, dropout=drop)
        out[j] = R.decode_fwd(R.heads(o, B, N, H), j, N).cpu()
    return out


def _probe_dkv(B, N, H, causal, drop, blocks):
    """{j: keep [B, H, rows, N]} as the dK/dV kernel applies it"""
    from vitamd import ops
    out = {}
    qd = torch.zeros(B * N, 3 * H * 64, device="cuda", dtype=BF16)
    o, lse = ops.attention_fwd(qd, B, N, H, causal, dropout=drop)              # V = 0: o = 0, lse = log2(keys seen)
    for j in blocks:
        _, d_o = R.probe_inputs("dkv", B, N, H, j)
        dqkv = ops.attention_bwd(qd, o, lse, d_o.to("cuda", BF16), B, N, H, causal, dropout=drop)
        out[j] = R.decode_dkv(R.split(dqkv, B, N, H)[2], j, N).cpu()
    return out


def _probe_dq(B, N, H, causal, drop, blocks, delta_ref):
    """{j: keep [B, H, N, cols]} as the dQ kernel applies it"""
    out = {}
    for j in blocks:
        qkv, d_o = R.probe_inputs("dq", B, N, H, j)
        _, _, dqkv = _run(qkv, d_o, B, N, H, causal, drop)
        out[j] = R.decode_dq(R.split(dqkv.float().cpu(), B, N, H)[0], j, N, delta_ref, causal, drop[0])
    return out


@pytest.mark.parametrize("N,causal", R.PROBE_CASES)
def test_attention_dropout_mask_equals_the_reference_in_every_consumer(hip, N, causal):
    """Every (b, h, q, k) decision of the forward, of the dQ kernel and of the dK/dV kernel against _attention_ref.mask(): N = 70 and 197 the
    small forward and the plain backward loops, 300 attn_fwd_kernel, 600 the long kernels (two chunks, ragged last tile)."""
    B, H, drop = R.PROBE_B, R.PROBE_H, (R.PROBE_P, R.SEED)
    keep, region, M = R.probe_reference(N, causal)
    blocks = range(R.n_blocks(N))
    got = {"fwd": torch.cat([t for _, t in sorted(_probe_fwd(B, N, H, causal, drop, blocks).items())], -1),
           "dkv": torch.cat([t for _, t in sorted(_probe_dkv(B, N, H, causal, drop, blocks).items())], -2),
           "dq": torch.cat([t for _, t in sorted(_probe_dq(B, N, H, causal, drop, blocks, R.probe_delta_ref(M, causal)).items())], -1)}
    for kind, g in got.items():
        wrong = (g != keep) & region
        assert not bool(wrong.any()), (kind, int(wrong.sum()), wrong.nonzero()[:4].tolist())


# ------------------------------------------------------------------------------------------ 3.3 the index past 2^32 and the length limit
def test_attention_dropout_mask_past_2_to_32(hip):
    """N = 16384, B * H = 17: ((bh N + q) N + k) reaches 2^32 at bh = 16, where the high index word enters the hash.  Forward and dK/dV
    probes on the first, a middle and the last block of 64 keys (queries); compared for bh = 15 and 16."""
    B, N, H, drop = 1, R.LONG_N, 17, (R.PROBE_P, R.SEED)
    blocks = (0, 129, N // 64 - 1)
    bhs = [15, 16]
    fwd = _probe_fwd(B, N, H, False, drop, blocks)
    dkv = _probe_dkv(B, N, H, False, drop, blocks)
    for j in blocks:
        cols = range(64 * j, 64 * j + 64)
        want = R.mask_rows(bhs, N, *drop, keys=list(cols)) != 0                      # [2, N, 64]
        assert torch.equal(fwd[j][0, bhs], want), ("fwd", j)
        want = R.mask_rows(bhs, N, *drop, q0=cols[0], q1=cols[-1] + 1) != 0          # [2, 64, N]
        assert torch.equal(dkv[j][0, bhs], want), ("dkv", j)


def test_attention_at_16384_tokens(hip, record_property):
    """The advertised length, causal, one head: 512 y-blocks, 32 chunks.  Full o and lse, dq on eight query tiles and dk / dv on the
    matching key tiles (first, last, both sides of the chunk edges at 512 and 8192 and of the y-block edge at 8320), against the
    row-chunked reference."""
    N, tiles = R.LONG_N, R.LONG_TILES
    r = R.long_reference()
    o, lse, dqkv = _run(r["qkv"], r["d_o"], 1, N, 1, True, (0.0, 0))
    dqkv = dqkv.float().cpu()
    got = {"o": o.float().cpu(), "lse": lse.cpu().view(N), "dq": R.take_tiles(dqkv[:, :64], tiles), "dk": R.take_tiles(dqkv[:, 64:128], tiles),
           "dv": R.take_tiles(dqkv[:, 128:], tiles)}
    assert bool(torch.isfinite(dqkv).all())
    _hold_to_bounds(got, r, N, record_property)


def test_attention_refuses_16385_tokens(hip):
    from vitamd import ops, lib
    N = R.LONG_N + 1
    qkv = torch.zeros(N, 192, device="cuda", dtype=BF16)
    with pytest.raises(lib.VitamdError):
        ops.attention_fwd(qkv, 1, N, 1, True)
    o, lse = torch.zeros(N, 64, device="cuda", dtype=BF16), torch.zeros(1, 1, N, device="cuda")
    with pytest.raises(lib.VitamdError):
        ops.attention_bwd(qkv, o, lse, o, 1, N, 1, True)


# ------------------------------------------------------------------------------------------ 3.4 residual epilogue under dropout and causal
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,N,H", [(3, 37, 2), (1, 256, 2)])
def test_attention_fwd_fused_residual_with_dropout(hip, B, N, H, causal):
    """attn_fwd_small_kernel<K, DROP = true, CAUSAL, RES = true>: o and lse bit-equal to the call without resid, x1 = x0 + o exactly"""
    from vitamd import ops
    drop = (0.3, R.SEED)
    qkv = R.r16(R.randn((B * N, 3 * H * 64), 431 + N, 1.5)).to("cuda", BF16)
    x0 = R.randn((B * N, H * 64), 432 + N, 2.0).to("cuda")
    o_ref, lse_ref = ops.attention_fwd(qkv, B, N, H, causal, dropout=drop)
    o, lse, x1 = ops.attention_fwd(qkv, B, N, H, causal, dropout=drop, resid=x0)
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    assert torch.equal(x1, x0 + o_ref.float())
    assert not torch.equal(o, ops.attention_fwd(qkv, B, N, H, causal)[0])            # the mask was applied


# ------------------------------------------------------------------------------------------ 3.5 spike across tiles and chunks, and in backward
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("N,key", R.SPIKE_CASES)
def test_attention_softmax_spike_late_and_in_backward(hip, N, key, causal, record_property):
    """test_attention_softmax_spike's dominating key, late in attn_fwd_kernel's tile loop (N = 300) and in the second chunk of the long
    kernels (N = 600): the rescale of everything accumulated before it, and backward's exp2(s c - lse) with one key holding the row"""
    qkv, d_o = R.spike_inputs(N, key)
    r = R.spike_reference(N, key, causal)
    o, lse, dqkv = _run(qkv, d_o, 1, N, 1, causal, (0.0, 0))
    if not causal:
        assert R.rel_l2(o[10].float().cpu(), qkv[key, 128:192]) < 1.0e-6
    _hold_to_bounds(R.kernel_outputs(o.cpu(), lse.cpu(), dqkv.cpu(), 1, N, 1), r, N, record_property)
