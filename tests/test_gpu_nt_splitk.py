"""The split-K form of the 128x128 NT GEMM kernel (vitamd_gemm_nt_bf16_ws) on a real MI355X, through the C ABI with a
caller-owned, poisoned workspace.  Every epilogue the form serves, at row counts around the 128-row tile, the three widths of the kept-row layer
and the head (N = 1000 zero-padded to 1024, as functions.linear pads it), K from one K-tile pair to 48 K-tiles, and the split count forced to 1,
to 2 and left to the rule.

Reference: float64 on the same bf16 inputs.  Bound: the split form differs from the unsplit kernel by fp32 summation order only, so its rel-L2
against float64 must stay within 2 x the unsplit kernel's own, measured here on the same inputs (the factor covers seed-to-seed variation of a
rounding-order change).  Two runs of the split form are torch.equal; one split IS the unsplit kernel (torch.equal)."""
import functools
import math

import pytest
import torch

import _poison as P
import vit_oracle as O

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
EPI_BIAS_BF16, EPI_GELU, EPI_RESID_F32, EPI_DGELU, EPI_F32, EPI_GELU_DG, EPI_DMUL = 0, 1, 2, 3, 5, 6, 7
EPIS = [EPI_BIAS_BF16, EPI_F32, EPI_GELU, EPI_GELU_DG, EPI_RESID_F32, EPI_DGELU, EPI_DMUL]
ROWS = [1, 127, 128, 129, 256]
WIDTHS = [128, 768, 1000]                 # 1000: the classifier head, zero-padded to a multiple of 64
DEPTHS = [128, 192, 768, 3072]            # 2, 3 (no split: a split is at least 2 K-tiles), 12 and 48 K-tiles
FORM_SPLITK, TILE_BYTES = 6, 128 * 128 * 4
MAXM = max(ROWS)


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _pad64(n):
    return (n + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _inputs(N, K):
    """bf16 operands on the device, and the float64 product of exactly those values; computed once per shape, never written to"""
    Np = _pad64(N)
    a = randn((MAXM, K), 1).to(BF16)
    b = torch.zeros((Np, K), dtype=BF16)
    b[:N] = randn((N, K), 2, 0.05).to(BF16)
    bias = torch.zeros(Np)
    bias[:N] = randn((N,), 3)
    res = randn((MAXM, Np), 4)
    aux = randn((MAXM, Np), 5, 0.8).to(BF16)
    acc = a.to(F64) @ b.to(F64).t()
    return {"Np": Np, "a": a.to(DEV), "b": b.to(DEV), "bias": bias.to(DEV), "res": res.to(DEV), "aux": aux.to(DEV), "acc": acc,
            "bias64": bias.to(BF16).to(F64), "res64": res.to(F64), "aux64": aux.to(F64)}


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _reference(I, epi, M):
    """float64 outputs (out, out2 or None) of the epilogue on the exact product"""
    acc = I["acc"][:M]
    if epi == EPI_F32:
        return acc, None
    if epi in (EPI_DGELU, EPI_DMUL):
        return acc * (_dgelu64(I["aux64"][:M]) if epi == EPI_DGELU else I["aux64"][:M]), None
    pre = acc + I["bias64"]
    if epi == EPI_BIAS_BF16:
        return pre, None
    if epi == EPI_RESID_F32:
        return I["res64"][:M] + pre, None
    return (pre if epi == EPI_GELU else _dgelu64(pre)), _gelu64(pre)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(hip, I, epi, M, K, splits, ws):
    """splits None: vitamd_gemm_nt_bf16 (the unsplit kernel); else the workspace form.  Outputs start poisoned."""
    Np = I["Np"]
    out = P.poison_(torch.empty((M, Np), dtype=F32 if epi in (EPI_RESID_F32, EPI_F32) else BF16, device=DEV))
    out2 = P.poison_(torch.empty((M, Np), dtype=BF16, device=DEV)) if epi in (EPI_GELU, EPI_GELU_DG) else None
    bias = I["bias"].data_ptr() if epi in (EPI_BIAS_BF16, EPI_GELU, EPI_GELU_DG, EPI_RESID_F32) else None
    aux = {EPI_RESID_F32: I["res"], EPI_DGELU: I["aux"], EPI_DMUL: I["aux"]}.get(epi)
    args = (I["a"].data_ptr(), I["b"].data_ptr(), out.data_ptr(), None if out2 is None else out2.data_ptr(), bias,
            None if aux is None else aux.data_ptr(), None, M, Np, K, Np, epi, 0, 0, 0, 0)
    if splits is None:
        code = hip.vitamd_gemm_nt_bf16(*args, _stream())
    else:
        P.poison_(ws)
        code = hip.vitamd_gemm_nt_bf16_ws(*args, splits, ws.data_ptr(), ws.numel() * 4, _stream())
    assert code == 0, (code, epi, M, Np, K, splits)
    return out, out2


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rule(M, Np, K, cus):
    """the split count is a function of N and K alone (two tile rows assumed), for launches of at most 256 rows"""
    tiles = 2 * ((Np + 127) // 128)
    return max(1, min(cus // tiles if tiles < cus and M <= 256 else 1, K // 128))


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("epi", EPIS)
def test_split_form_within_twice_the_unsplit_kernels_error(hip, epi, N):
    from vitamd import ops
    ops.init(torch.device(DEV))
    cus = _cus()
    ws = torch.empty((cus * TILE_BYTES // 4,), dtype=F32, device=DEV)       # the rule never asks for more; forced 2 on <= 16 tiles neither
    worst = 0.0
    for K in DEPTHS:
        I = _inputs(N, K)
        Np = I["Np"]
        for M in ROWS:
            want, want2 = _reference(I, epi, M)
            old, old2 = _launch(hip, I, epi, M, K, None, None)
            e_old = O.rel_l2(old.double().cpu(), want)
            e_old2 = O.rel_l2(old2.double().cpu(), want2) if old2 is not None else None
            rule = _rule(M, Np, K, cus)
            for splits in (1, 2, 0):
                expect = {1: 1, 2: min(2, max(1, K // 128)), 0: rule}[splits]
                plan = hip.vitamd_gemm_nt_ws_plan(M, Np, K, Np, epi, 0, splits)
                need = hip.vitamd_gemm_nt_ws_bytes(M, Np, K, Np, epi, 0, splits)
                tiles = ((M + 127) // 128) * ((Np + 127) // 128)
                if expect == 1:
                    assert plan == hip.vitamd_gemm_nt_plan(M, Np, K, Np, epi, 0) and plan & 0x7f != FORM_SPLITK and need == 0
                else:
                    assert plan == FORM_SPLITK | 128 << 8 | expect << 16 and need == expect * tiles * TILE_BYTES <= ws.numel() * 4
                    assert K // 64 // expect >= 2 and (splits != 0 or tiles * expect <= cus)
                got, got2 = _launch(hip, I, epi, M, K, splits, ws)
                again, again2 = _launch(hip, I, epi, M, K, splits, ws)
                assert torch.equal(got, again) and (got2 is None or torch.equal(got2, again2))
                if expect == 1:
                    assert torch.equal(got, old) and (got2 is None or torch.equal(got2, old2))
                e_new = O.rel_l2(got.double().cpu(), want)
                print(f"epi {epi} M {M} N {Np} K {K} splits {splits}->{expect}: split {e_new:.3e} unsplit {e_old:.3e}")
                worst = max(worst, e_new / e_old)
                assert e_new <= 2.0 * e_old, (epi, M, Np, K, splits, e_new, e_old)
                if got2 is not None:
                    e_new2 = O.rel_l2(got2.double().cpu(), want2)
                    print(f"   second output: split {e_new2:.3e} unsplit {e_old2:.3e}")
                    assert e_new2 <= 2.0 * e_old2, (epi, M, Np, K, splits, e_new2, e_old2)
    print(f"epi {epi} N {N}: worst split / unsplit ratio {worst:.3f}")


def test_refusals_and_the_launches_that_stay_unsplit(hip):
    from vitamd import ops
    I = _inputs(768, 768)
    M, Np, K = 256, 768, 768
    ws = torch.empty((_cus() * TILE_BYTES // 4,), dtype=F32, device=DEV)
    args = (I["a"].data_ptr(), I["b"].data_ptr(), None, None, I["bias"].data_ptr(), None, None, M, Np, K, Np, EPI_BIAS_BF16, 0, 0, 0)
    old, _ = _launch(hip, I, EPI_BIAS_BF16, M, K, None, None)
    out = torch.empty((M, Np), dtype=BF16, device=DEV)
    a = args[:2] + (out.data_ptr(),) + args[3:]
    need = hip.vitamd_gemm_nt_ws_bytes(M, Np, K, Np, EPI_BIAS_BF16, 0, 0)
    assert need > 0
    assert hip.vitamd_gemm_nt_bf16_ws(*a, 0, 0, ws.data_ptr(), need - 4, _stream()) == 2          # a workspace that is too small: VITAMD_ERR_ARG
    assert hip.vitamd_gemm_nt_bf16_ws(*a, 0, -1, ws.data_ptr(), need, _stream()) == 2
    assert hip.vitamd_gemm_nt_ws_bytes(M, Np, K, Np, EPI_BIAS_BF16, 0, -1) == -2
    # no workspace, an explicit tile code, the patch epilogue, more than two tile rows: the unsplit launch
    P.poison_(out)
    assert hip.vitamd_gemm_nt_bf16_ws(*a, 0, 0, None, 0, _stream()) == 0 and torch.equal(out, old)
    P.poison_(out)
    assert hip.vitamd_gemm_nt_bf16_ws(*a, 128, 0, ws.data_ptr(), ws.numel() * 4, _stream()) == 0 and torch.equal(out, old)
    assert hip.vitamd_gemm_nt_ws_bytes(M, Np, K, Np, EPI_BIAS_BF16, 128, 0) == 0
    assert hip.vitamd_gemm_nt_ws_bytes(M, Np, K, Np, 4, 0, 0) == 0                                  # VITAMD_EPI_PATCH_F32
    assert hip.vitamd_gemm_nt_ws_bytes(257, Np, K, Np, EPI_BIAS_BF16, 0, 0) == 0
    # the host wrapper: the switch off is the unsplit kernel, on is the rule's split form
    saved = ops.NT_SPLITS
    try:
        ops.NT_SPLITS = 1
        off = ops.gemm_nt(I["a"], I["b"], ops.EPI_BIAS_BF16, bias=I["bias"])
        ops.NT_SPLITS = 0
        on = ops.gemm_nt(I["a"], I["b"], ops.EPI_BIAS_BF16, bias=I["bias"])
    finally:
        ops.NT_SPLITS = saved
    split, _ = _launch(hip, I, EPI_BIAS_BF16, M, K, 0, ws)
    assert torch.equal(off, old) and torch.equal(on, split)


@pytest.mark.parametrize("epi", [EPI_BIAS_BF16, EPI_RESID_F32])
def test_a_rows_result_does_not_depend_on_the_number_of_rows(hip, epi):
    """The rule's K ranges are a function of N and K: the first rows of a 256-row launch are the bits of a launch of those rows alone, as they are
    with the unsplit kernel (a sample's logits in a batch of 256 and in a batch of 32)."""
    I = _inputs(768, 3072)
    ws = torch.empty((_cus() * TILE_BYTES // 4,), dtype=F32, device=DEV)
    full, _ = _launch(hip, I, epi, 256, 3072, 0, ws)
    for M in (1, 32, 129):
        assert hip.vitamd_gemm_nt_ws_plan(M, 768, 3072, 768, epi, 0, 0) == hip.vitamd_gemm_nt_ws_plan(256, 768, 3072, 768, epi, 0, 0)
        part, _ = _launch(hip, I, epi, M, 3072, 0, ws)
        assert torch.equal(part, full[:M])
    assert hip.vitamd_gemm_nt_ws_bytes(384, 768, 3072, 768, epi, 0, 0) == 0          # more than two tile rows: the unsplit kernel


@pytest.mark.parametrize("M", [3, 120, 256])
def test_column_sums_do_not_change_the_output(hip, M):
    """EPI_DMUL with column sums (the path with functions.BIAS_FROM_WGRAD off) splits like the launch without them: the same `out`, bit for bit,
    and the sums of the stored tile (atomics: the bound of test_gpu_keep.py's column sums)."""
    I = _inputs(768, 768)
    Np, K = 768, 768
    ws = torch.empty((_cus() * TILE_BYTES // 4,), dtype=F32, device=DEV)
    without, _ = _launch(hip, I, EPI_DMUL, M, K, 0, ws)
    out = P.poison_(torch.empty((M, Np), dtype=BF16, device=DEV))
    cs = torch.zeros(Np, device=DEV)
    P.poison_(ws)
    assert hip.vitamd_gemm_nt_bf16_ws(I["a"].data_ptr(), I["b"].data_ptr(), out.data_ptr(), None, None, I["aux"].data_ptr(), cs.data_ptr(),
                                      M, Np, K, Np, EPI_DMUL, 0, 0, 0, 0, 0, ws.data_ptr(), ws.numel() * 4, _stream()) == 0
    assert torch.equal(out, without)
    assert O.rel_l2(cs.cpu(), out.float().cpu().sum(0)) < 1.0e-6
