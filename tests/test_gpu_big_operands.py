"""Operands and outputs of 2^31 and 2^32 bytes and more, on a real MI355X (include/vitamd.h: the size rules of vitamd_gemm_nt_bf16,
vitamd_linear_dropout_resid_bf16 and the vitamd_gemm_tn_bf16* entry points).

The kernels on 256-column tiles address memory through buffer descriptors with 32-bit byte offsets; vitamd_gemm_nt_impl therefore cuts a big
call into row panels, and the TN GEMM refuses what it cannot address.  Three things can go wrong past a boundary, and each would show in these
cases as wrong numbers, never as an error code: an offset row x (bytes per row) that wraps at 2^32, a descriptor size truncated to 32 bits,
and a store "masked" by sending it to offset 2^31, which is inside a buffer of more than 2 GiB (rows >= M and columns >= N exist in every NT
case here: M % 256 = 77, N % 256 = 8).  tests/_big_ref.py builds the references on the device without the library and holds them to the CPU
arithmetic of tests/_gemm_ref.py on bands of rows around every boundary; the whole output is compared on bit patterns, guard rows and
padding columns included.  Every case frees what it holds before the next and prints FORM / PEAK / WALL lines (peak device memory is
asserted to stay within 24 GiB); a case is skipped only when the device has less free memory than it needs."""
import time

import numpy as np
import pytest
import torch

import _big_ref as B
import _dropout_ref as DR
import _gemm_ref as G
from _gemm_ref import BF16, F32, GUARD

pytestmark = pytest.mark.gpu

ERR_SHAPE = 1
PEAK_LIMIT = 24 * B.GIB
DEV = "cuda"


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t, offset_bytes=0):
    return None if t is None else t.data_ptr() + offset_bytes


@pytest.fixture(scope="module")
def hip_init(hip):
    from vitamd import ops
    ops.init()
    return hip


class _Budget:
    """free the allocator's cache, skip when the device cannot hold the case, then report PEAK and WALL when the case is over"""

    def __init__(self, name, need):
        self.name, self.need = name, need

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free, total = torch.cuda.mem_get_info()
        print(f"FREE {self.name} free={free / B.GIB:.1f}GiB of {total / B.GIB:.1f}GiB, needs {self.need / B.GIB:.1f}GiB")
        if free < self.need:
            pytest.skip(f"{self.name} needs {self.need / B.GIB:.1f} GiB of free device memory, {free / B.GIB:.1f} GiB are free")
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        print(f"PEAK {self.name} peak={peak / B.GIB:.2f}GiB")
        print(f"WALL {self.name} wall={time.perf_counter() - self.t0:.2f}s")
        torch.cuda.empty_cache()
        if exc[0] is None:
            assert peak <= PEAK_LIMIT, f"{self.name}: peak device memory {peak / B.GIB:.2f} GiB is above 24 GiB"
        return False


# ---------------------------------------------------------------------------------------------- NT GEMM
def _nt_call(hip, p, tile, out, out2, colsum):
    c = p.case
    esz = B.out_esz(c.epi)
    code = hip.vitamd_gemm_nt_bf16(_ptr(p.a), _ptr(p.b), _ptr(out, GUARD * c.ldo * esz), _ptr(out2, GUARD * c.ldo * 2), _ptr(p.bias), _ptr(p.aux), _ptr(colsum),
                                   c.M, c.N, c.K, c.ldo, c.epi, 0, 0, 0, tile, _st())
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize("case", B.NT_CASES, ids=B.nt_id)
def test_nt_outputs_and_operands_past_2g_and_4g(hip_init, case):
    """Every tile code of the case against the device reference: the whole framed `out` (and `out2`) on bit patterns, colsum exactly."""
    hip = hip_init
    with _Budget(case.name, B.nt_bytes_needed(case)):
        p = B.nt_problem(case, DEV)
        bs = B.check_reference_bands(p)
        print(f"BANDS {case.name} {bs} boundary rows {B.boundary_rows(case)} exactness {p.units:.0f} of 2^24")
        rows = case.M + 2 * GUARD
        gelu = case.epi == G.EPI_GELU
        for tile in case.tiles:
            plan = hip.vitamd_gemm_nt_plan(case.M, case.N, case.K, case.ldo, case.epi, tile)
            print(f"FORM nt {case.name} tile={tile} plan={plan:#x}" if plan >= 0 else f"FORM nt {case.name} tile={tile} refused={-plan}")
            assert B.form_ok(case, tile, plan), (case.name, tile, hex(plan))
            for with_colsum in ((True, False) if case.epi == G.EPI_DMUL else (False,)):
                t0 = time.perf_counter()
                out = B.sentinel(rows, case.ldo, p.out_dtype, DEV)
                out2 = B.sentinel(rows, case.ldo, BF16, DEV) if gelu else None
                cs = p.colsum0.clone() if with_colsum else None
                code = _nt_call(hip, p, tile, out, out2, cs)
                assert code == 0, (case.name, tile, code)
                B.assert_equal_chunked(f"{case.name} tile {tile} out", out, p.want)
                if gelu:
                    B.assert_equal_chunked(f"{case.name} tile {tile} out2", out2, p.want2, settle=B.gelu_out2_settle(p.want, case.M, case.N))
                if cs is not None:
                    assert torch.equal(cs, p.colsum_want), f"{case.name} tile {tile}: colsum differs in {int((cs != p.colsum_want).sum())} columns"
                print(f"WALL nt {case.name} tile={tile} colsum={with_colsum} wall={time.perf_counter() - t0:.2f}s")
                del out, out2, cs
        del p


def test_linear_dropout_resid_mask_past_4g(hip_init):
    """vitamd_linear_dropout_resid_bf16 with an fp32 output past 2^32 bytes: a zero GEMM with bias 2 and a zero residual shows the mask.  Every
    element is 0 or bf16(2 / (1 - p)); on the bands the mask is the reference's, with index row * N + col of the WHOLE call on every panel."""
    hip = hip_init
    c = B.DROPOUT_CASE
    P, SEED = 0.25, 0x5EED1234ABCD
    with _Budget(c.name, 2 * (c.M + 2 * GUARD) * c.N * 4 + 4 * B.CHUNK_ELEMS * 4):
        a = torch.zeros((c.M, c.K), dtype=BF16, device=DEV)
        w = torch.zeros((c.N, c.K), dtype=BF16, device=DEV)
        bias = torch.full((c.N,), 2.0, device=DEV)
        resid = torch.zeros((c.M, c.N), device=DEV)
        out = B.sentinel(c.M + 2 * GUARD, c.N, F32, DEV)
        plan = hip.vitamd_gemm_nt_plan(c.M, c.N, c.K, c.N, G.EPI_RESID_F32, 0)
        print(f"FORM nt {c.name} tile=0 plan={plan:#x}")
        assert plan > 0 and plan & 0x7f in (B.FORM_PP, B.FORM_PP_PERSISTENT), hex(plan)
        code = hip.vitamd_linear_dropout_resid_bf16(a.data_ptr(), w.data_ptr(), out.data_ptr() + GUARD * c.N * 4, bias.data_ptr(), resid.data_ptr(),
                                                    c.M, c.N, c.K, P, SEED, 0, _st())
        torch.cuda.synchronize()
        assert code == 0
        G.assert_untouched("guard rows", torch.cat([out[:GUARD], out[GUARD + c.M:]]).cpu())
        y = out[GUARD:GUARD + c.M].view(torch.float32)
        kept = G.r16(torch.tensor(2.0 * float(DR.scale(P)))).item()
        nkept = 0
        for r0, r1 in B.row_chunks(c.M, c.N):
            yc = y[r0:r1]
            assert bool(((yc == 0) | (yc == kept)).all()), f"rows {r0}..{r1 - 1}: a value that is neither 0 nor {kept}"
            nkept += int((yc != 0).sum())
        n = c.M * c.N
        assert abs(nkept - n * (1 - P)) < 6 * (n * P * (1 - P)) ** 0.5, (nkept, n)         # six standard deviations of the binomial count
        for lo, hi in B.nt_bands(c):
            idx = np.arange(lo, hi, dtype=np.uint64)[:, None] * np.uint64(c.N) + np.arange(c.N, dtype=np.uint64)[None, :]
            keep = torch.from_numpy(DR.keep(idx, SEED, P))
            bad = ((y[lo:hi] != 0).cpu() != keep).nonzero()
            assert bad.numel() == 0, f"mask differs in {bad.shape[0]} elements of rows {lo}..{hi - 1}; first at row {lo + int(bad[0][0])}, column {int(bad[0][1])}"
        del a, w, bias, resid, out, y


# ---------------------------------------------------------------------------------------------- TN GEMM at its size guard
def _tn_frame(device):
    return B.sentinel(B.TN_PQ + 2, B.TN_PQ, F32, device)


@pytest.mark.parametrize("big", ["L", "R"])
def test_tn_largest_accepted_r_is_exact(hip, big):
    """R = 262 079, the largest the guard accepts at a row stride of 4096: the operand is a 64-column slice of a 2-GiB buffer whose other columns hold
    NaN, and the last stage's offsets end just below 2^31.  Both workspace forms (with and without colsum) and the atomic form, against
    float64 on the device; integers, so equality."""
    R = B.TN_MAX_R
    assert B.tn_guard_accepts(R, B.TN_BIG_LD) and not B.tn_guard_accepts(R + 1, B.TN_BIG_LD)
    with _Budget(f"tn-{big}", R * (B.TN_BIG_LD + 128) * 2 + B.GIB):
        p = B.tn_problem(R, big, DEV)
        lp, rp = p.lbuf.data_ptr() + p.loff * 2, p.rbuf.data_ptr() + p.roff * 2
        PQ = B.TN_PQ
        ws_bytes = hip.vitamd_gemm_tn_ws_bytes(R, PQ, PQ, 0)
        ws = torch.full((ws_bytes // 4,), float("nan"), device=DEV)
        print(f"FORM tn-{big} R={R} ldl={p.ldl} ldr={p.ldr} ws_bytes={ws_bytes}")

        def check(name, out, want):
            o = out.cpu()
            frame = _tn_frame("cpu")
            frame[:PQ] = G.bits(want.cpu())
            assert not bool(torch.isnan(o.view(torch.float32)).any()), f"{name}: NaN in out: a padding column leaked"
            G.assert_bits_equal(name, o, frame, guard=0)

        for form in (0, 1):
            for accumulate in (0, 1):
                out = _tn_frame(DEV)
                if accumulate:
                    out[:PQ] = G.bits(p.init)
                assert hip.vitamd_gemm_tn_bf16_ws(lp, rp, out.data_ptr(), R, PQ, PQ, p.ldl, p.ldr, PQ, 0, ws.data_ptr(), ws_bytes, accumulate, form, _st()) == 0
                torch.cuda.synchronize()
                check(f"tn-{big} form {form} accumulate {accumulate}", out, p.want_acc if accumulate else p.want_ovw)
            out, cs = _tn_frame(DEV), p.colsum0.clone()
            assert hip.vitamd_gemm_tn_bf16_ws_colsum(lp, rp, out.data_ptr(), cs.data_ptr(), R, PQ, PQ, p.ldl, p.ldr, PQ, 0, ws.data_ptr(), ws_bytes, 0, form, _st()) == 0
            torch.cuda.synchronize()
            check(f"tn-{big} form {form} colsum call", out, p.want_ovw)
            assert torch.equal(cs, p.colsum_want), f"tn-{big} form {form}: colsum differs in {int((cs != p.colsum_want).sum())} columns"
        out = _tn_frame(DEV)
        out[:PQ] = G.bits(p.init)
        assert hip.vitamd_gemm_tn_bf16(lp, rp, out.data_ptr(), R, PQ, PQ, p.ldl, p.ldr, PQ, 0, _st()) == 0
        torch.cuda.synchronize()
        check(f"tn-{big} atomic", out, p.want_acc)

        # one more row: refused by all three entry points, nothing written (the buffers are never read: the same pointers serve)
        ws.fill_(7.0)
        for form in (0, 1):
            out, cs = _tn_frame(DEV), p.colsum0.clone()
            codes = (hip.vitamd_gemm_tn_bf16_ws(lp, rp, out.data_ptr(), R + 1, PQ, PQ, p.ldl, p.ldr, PQ, 0, ws.data_ptr(), ws_bytes, 0, form, _st()),
                     hip.vitamd_gemm_tn_bf16_ws_colsum(lp, rp, out.data_ptr(), cs.data_ptr(), R + 1, PQ, PQ, p.ldl, p.ldr, PQ, 0, ws.data_ptr(), ws_bytes, 0, form, _st()),
                     hip.vitamd_gemm_tn_bf16(lp, rp, out.data_ptr(), R + 1, PQ, PQ, p.ldl, p.ldr, PQ, 0, _st()))
            torch.cuda.synchronize()
            assert codes == (ERR_SHAPE,) * 3, codes
            G.assert_untouched(f"tn-{big} refused out", out.cpu())
            assert torch.equal(cs, p.colsum0) and bool((ws == 7.0).all())
        del p, ws, out, cs


# ---------------------------------------------------------------------------------------------- streaming kernels past 2^31 / 2^32 elements
CAST_N = 2 ** 31 + 11
DROP_N = 2 ** 32 + 4096
LN_M, LN_D, LN_EPS = 2 ** 21 + 5, 1024, 1e-5
TAIL = 64                                      # sentinel elements behind a flat output


def _randn_into(t, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    for i0 in range(0, flat.numel(), B.CHUNK_ELEMS):
        c = flat[i0:i0 + B.CHUNK_ELEMS]
        c.normal_(generator=g)
        if scale != 1.0 or shift != 0.0:
            c.mul_(scale).add_(shift)


def test_cast_f32_bf16_past_2g_elements(hip):
    """n = 2^31 + 11: the first element index that does not fit a signed 32-bit integer, with a scalar tail (n % 8 = 3).  The whole output is the
    round-to-nearest-even cast (torch's, which tests/test_gemm_ref_host.py holds to exact arithmetic), and nothing behind element n - 1 is written."""
    n = CAST_N
    with _Budget("cast", n * 6 + 8 * B.CHUNK_ELEMS):
        x = torch.empty(n, device=DEV)
        _randn_into(x, 41)
        out = torch.full((n + TAIL,), G.SENT16, dtype=torch.int16, device=DEV)
        assert hip.vitamd_cast_f32_bf16(x.data_ptr(), out.data_ptr(), n, _st()) == 0
        torch.cuda.synchronize()
        assert bool((out[n:] == G.SENT16).all()), "elements behind n were written"
        for i0 in range(0, n, B.CHUNK_ELEMS):
            i1 = min(n, i0 + B.CHUNK_ELEMS)
            want = x[i0:i1].to(BF16).view(torch.int16)
            if not torch.equal(out[i0:i1], want):
                bad = (out[i0:i1] != want).nonzero()
                raise AssertionError(f"cast: {bad.shape[0]} elements differ in [{i0}, {i1}); first at {i0 + int(bad[0][0])}")
        for lo, hi in B.flat_bands(n, [2 ** 29, 2 ** 30, 2 ** 31]):                     # byte 2^31 / 2^32 of the input and the output, element 2^31
            ref = x[lo:hi].double()
            got = out[lo:hi].view(BF16)
            assert float(B.bf16_ulps(got, ref).max()) <= 0.5, (lo, hi)                  # one rounding of an exact conversion: half a unit in the last place
        del x, out


def test_dropout_bf16_in_place_past_4g_elements(hip):
    """n = 2^32 + 4096 in place: the first element indices with a high word.  Bands against _dropout_ref.mask(..., start=...); everywhere a value is
    its input times 0 or times bf16-rounded 1 / (1 - p)."""
    n, P, SEED = DROP_N, 0.25, 0xC0FFEE1234567
    with _Budget("dropout", n * 2 + 10 * B.CHUNK_ELEMS):
        x = torch.empty(n + TAIL, dtype=BF16, device=DEV)
        for i0 in range(0, n + TAIL, B.CHUNK_ELEMS):
            i1 = min(n + TAIL, i0 + B.CHUNK_ELEMS)
            x[i0:i1] = B.device_ints((i1 - i0,), 1, 7, 900 + i0 // B.CHUNK_ELEMS, DEV)                     # non-zero: a dropped element shows
        bs = B.flat_bands(n, [2 ** 30, 2 ** 31, 2 ** 32])                                                      # byte 2^31, byte 2^32 / element 2^31, element 2^32
        before = {b: x[b[0]:b[1]].clone() for b in bs}
        tail = x[n:].clone()
        assert hip.vitamd_dropout_bf16(x.data_ptr(), x.data_ptr(), n, 1, P, SEED, _st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(x[n:], tail), "elements behind n were written"
        scale = float(DR.scale(P))
        for (lo, hi), xin in before.items():
            keep = torch.from_numpy(DR.mask(hi - lo, SEED, P, start=lo)).to(DEV)
            want = (xin.float() * torch.where(keep, scale, 0.0)).to(BF16)
            bad = (x[lo:hi] != want).nonzero()
            assert bad.numel() == 0, f"dropout: {bad.shape[0]} elements of [{lo}, {hi}) differ from the reference mask; first at {lo + int(bad[0][0])}"
        nkept = sum(int((x[i0:min(n, i0 + B.CHUNK_ELEMS)] != 0).sum()) for i0 in range(0, n, B.CHUNK_ELEMS))
        assert abs(nkept - n * (1 - P)) < 6 * (n * P * (1 - P)) ** 0.5, (nkept, n)
        del x, before, tail


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_layernorm_fwd_bwd_past_2g_elements(hip):
    """M = 2^21 + 5 rows of D = 1024: more than 2^31 elements, x and g of 8 GiB each.  Bands of rows (the first, the last - which hold element
    2^31 and byte 2^32 of the bf16 tensors - and those around byte 2^31 and byte 2^32 of the fp32 tensors) against float64 on the device.
    Bounds: y, mean and g are those of test_gpu_kernels.py::test_layernorm_fwd_bwd (the same input distribution); rstd: 16 + 6 fp32 additions
    per lane and wave reduction (22 x 2^-24 on the variance, half of it on rstd) plus two units of rsqrtf = 0.8e-6 < 1e-6.  The backward's dy
    is drawn into y's buffer once y has been checked."""
    M, D = LN_M, LN_D
    with _Budget("layernorm", M * D * (4 + 2 + 4) + 8 * B.CHUNK_ELEMS * 4):
        x = torch.empty((M, D), device=DEV)
        _randn_into(x, 21, 2.0, 0.5)
        y = torch.full((M + 1, D), G.SENT16, dtype=torch.int16, device=DEV)                # one sentinel row behind
        mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        assert hip.vitamd_layernorm_fwd(x.data_ptr(), None, None, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, D, LN_EPS, _st()) == 0
        torch.cuda.synchronize()
        assert bool((y[M] == G.SENT16).all()), "the row behind y was written"
        bs = B.bands(M, [2 ** 19, 2 ** 20, 2 ** 21])
        print(f"BANDS layernorm {bs}")
        for lo, hi in bs:
            yr, mr, rr = B.ln_reference_rows(x[lo:hi].double(), LN_EPS)
            e = {"y": _rel_l2(y[lo:hi].view(BF16), yr.to(BF16)), "mean": _rel_l2(mean[lo:hi], mr), "rstd": _rel_l2(rstd[lo:hi], rr)}
            print(f"STAT layernorm fwd rows {lo}..{hi - 1} " + " ".join(f"{k}={v:.3g}" for k, v in e.items()))
            assert e["y"] < 2.9e-5 and e["mean"] < 1.0e-6 and e["rstd"] < 1.0e-6, (lo, hi, e)
        dy = y[:M].view(BF16)
        _randn_into(dy, 23)
        g = torch.full((M + 1, D), G.SENT32, dtype=torch.int32, device=DEV)
        assert hip.vitamd_layernorm_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, g.data_ptr(), None, None, M, D, _st()) == 0
        torch.cuda.synchronize()
        assert bool((g[M] == G.SENT32).all()), "the row behind g_out was written"
        for lo, hi in bs:
            xr = x[lo:hi].double().requires_grad_(True)
            yr, _, _ = B.ln_reference_rows(xr, LN_EPS)
            yr.backward(dy[lo:hi].double())
            e = _rel_l2(g[lo:hi].view(torch.float32), xr.grad)
            print(f"STAT layernorm bwd rows {lo}..{hi - 1} g={e:.3g}")
            assert e < 1.0e-6, (lo, hi, e)
        del x, y, dy, g, mean, rstd


# ---------------------------------------------------------------------------------------------- attention past 2^31 qkv elements
ATT_B, ATT_N, ATT_H = 4732, 197, 12            # the ViT-B shape: 4732 x 197 x 2304 = 2^31 + 302 912 elements of qkv (4.3e9 bytes)


def test_attention_fwd_bwd_past_2g_qkv_elements(hip):
    """The ViT-B shape at a batch that puts qkv and dqkv past 2^31 ELEMENTS (and 2^32 bytes): the eight-wave forward and the pipelined
    backward, the kernels whose per-(batch, head) bases were read as 64-bit throughout (csrc/attention.hip: head_addr, stat_index and the
    o / d_o / dqkv bases are size_t, rows inside a head are (size_t)row x stride).  The batches that hold byte 2^31 of qkv (2365), element
    2^31 = byte 2^32 (4731, the last), and the first two go to the host and are held to tests/_attention_ref.py at its own bounds (1.5 x
    the bf16 floor, 2 x the worst-tile floor, lse 1e-6); a sentinel row in front of and behind o and dqkv must stay."""
    import _attention_ref as R
    Bt, N, H = ATT_B, ATT_N, ATT_H
    D, D3 = H * 64, 3 * H * 64
    assert Bt * N * D3 > 2 ** 31 and (Bt - 1) * N * D3 <= 2 ** 31 < Bt * N * D3
    with _Budget("attention", 2 * Bt * N * (D3 + D) * 2 + 4 * B.CHUNK_ELEMS * 4):
        qkv = torch.empty((Bt * N, D3), dtype=BF16, device=DEV)
        _randn_into(qkv, 31, 1.5)
        d_o = torch.empty((Bt * N, D), dtype=BF16, device=DEV)
        _randn_into(d_o, 32)
        o = B.sentinel(Bt * N + 2, D, BF16, DEV)
        dqkv = B.sentinel(Bt * N + 2, D3, BF16, DEV)
        lse = torch.full((Bt + 2, H, N), 7.0, device=DEV)
        delta = torch.full((Bt + 2, H, N), 7.0, device=DEV)
        op, dp, lp, tp = o.data_ptr() + D * 2, dqkv.data_ptr() + D3 * 2, lse.data_ptr() + H * N * 4, delta.data_ptr() + H * N * 4
        assert hip.vitamd_attention_fwd(qkv.data_ptr(), op, lp, Bt, N, H, 64, 0, 0.0, 0, _st()) == 0
        assert hip.vitamd_attention_bwd(qkv.data_ptr(), op, lp, d_o.data_ptr(), dp, tp, None, Bt, N, H, 64, 0, 0.0, 0, _st()) == 0
        torch.cuda.synchronize()
        for name, t in (("o", o), ("dqkv", dqkv)):
            G.assert_untouched(f"guard rows of {name}", torch.stack([t[0], t[-1]]).cpu())
        for name, t in (("lse", lse), ("delta", delta)):
            assert bool((t[0] == 7.0).all()) and bool((t[-1] == 7.0).all()), f"{name} written outside [B, H, N]"
        bs = B.bands(Bt, [2 ** 30 // (N * D3), 2 ** 31 // (N * D3)], band=2)
        print(f"BANDS attention batches {bs}")
        assert any(lo <= 2365 < hi for lo, hi in bs) and bs[-1][1] == Bt
        for lo, hi in bs:
            nb, r0, r1 = hi - lo, lo * N, hi * N
            r = R._reference(qkv[r0:r1].float().cpu(), d_o[r0:r1].float().cpu(), nb, N, H, False, 0.0, 0)
            got = R.kernel_outputs(o[1 + r0:1 + r1].view(BF16).cpu(), lse[1 + lo:1 + hi].cpu(), dqkv[1 + r0:1 + r1].view(BF16).cpu(), nb, N, H)      # (o, dqkv: bit patterns)
            ratios, bad = R.compare({n: got[n] for n in (*r["floors"], "lse")}, r["ref"], r["floors"])
            print(f"STAT attention batches {lo}..{hi - 1} (global / floor, worst tile / tile floor):",
                  {n: (round(g, 3), round(t, 3)) if n != "lse" else g for n, (g, t) in ratios.items()})
            assert all(bool(torch.isfinite(t).all()) for t in got.values())
            assert not bad, (lo, hi, bad)
        del qkv, d_o, o, dqkv, lse, delta
