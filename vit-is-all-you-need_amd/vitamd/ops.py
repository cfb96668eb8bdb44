"""Host wrappers: torch device tensors in, libvitamd.so kernel launches on torch's current HIP stream.

PyTorch is plumbing here (HBM allocation, streams); every computation on the path is a kernel of
libvitamd.so.  All functions require ROCm device tensors and raise otherwise — no CPU fallback.
"""
from __future__ import annotations

import torch

from . import lib as _lib
from .lib import CONSTANTS as _H      # the VITAMD_* macros of include/vitamd.h: every code and limit below is read from there, none is restated
EPI_BIAS_BF16, EPI_GELU, EPI_RESID_F32, EPI_DGELU, EPI_PATCH_F32, EPI_F32, EPI_GELU_DG, EPI_DMUL = (_H["VITAMD_EPI_" + _n] for _n in "BIAS_BF16 GELU RESID_F32 DGELU PATCH_F32 F32 GELU_DG DMUL".split())
# Large NT GEMMs are launched persistent by default (one workgroup per CU: -0.3 ms/step inside the training step and the reason the
# weight-gradient stream can use the whole chip).  A persistent workgroup whose CU is held by another
# long-running kernel starts late with its whole tile list still to do, so the form is sensitive to resident foreign kernels
# (DESIGN.md section 7); VITAMD_NT_PERSISTENT=0 (or ops.NT_PERSISTENT = False at any time: it is read on every call, and the
# weight-gradient split rule of functions._tn_splits follows it) selects one workgroup per tile instead.  vitamd.ddp.DataParallel
# measures both forms beside its collectives at construction and sets it for multi-rank jobs (ddp.choose_launch_form).
import os as _os
NT_PERSISTENT = _os.environ.get("VITAMD_NT_PERSISTENT", "1") != "0"
# The seam form of the persistent NT kernel (csrc/gemm_nt_seam.h) issues its epilogue as a burst of buffer stores from inline asm.  On one box of the
# pool, round 3 saw buffer stores issued from inside a GEMM run several times slower than anywhere else (profiles/r03/store_trickle_README.md, last
# row); the form is therefore PROBED once per process and DEVICE against the plain persistent form on a QKV-sized problem and switched off there if it
# loses by more than 25 % (VITAMD_NT_SEAM=1 / 0 decides for every device and skips the probe).  Every GELU epilogue reads the same table, so the
# decision changes timing only, never bits.
_seam_env = _os.environ.get("VITAMD_NT_SEAM", "auto")
NT_SEAM = {"1": True, "0": False}.get(_seam_env)      # process-wide override (None = per device, by probe)
SEAM_PROBE = {}          # device index -> {"seam_us", "plain_us", "enabled"}: the source of truth for the per-device decision
NT_FORM_SEAM, NT_FORM_LOADER = _H["VITAMD_NT_FORM_SEAM"], _H["VITAMD_NT_FORM_LOADER"]      # (vitamd_gemm_nt_plan): the two forms whose epilogue is a burst of asm buffer stores
_RAW_AUTO = -1
LN_EPS = 1e-5
BF16, F32 = torch.bfloat16, torch.float32


def _L():
    return _lib.load()


_INITIALISED = set()     # device indices vitamd_init has run for


def init(device=None):
    """Per-device set-up of the library (C ABI vitamd_init: builds the 16-KiB erf-GELU table image - the only allocation / synchronisation the
    library ever makes).  Idempotent and cheap after the first call; called by the GEMM wrapper before a GELU launch, by functions.claim_streams
    and by GraphedStep's eager warm-up, so it never first happens inside a stream capture."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _INITIALISED:
        return
    if torch.cuda.is_current_stream_capturing():
        raise _lib.VitamdError("vitamd.ops.init: first use of a device inside a stream capture; run one eager step (or ops.init(device)) before capturing")
    _lib.check(_L().vitamd_init(idx, torch.cuda.current_stream(device).cuda_stream), f"vitamd_init[device {idx}]")
    _INITIALISED.add(idx)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _need(t, dtype, name, ndim=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.VitamdError(f"{name}: expected a ROCm device tensor (the HIP kernels are the only implementation)")
    if t.dtype != dtype:
        raise _lib.VitamdError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.VitamdError(f"{name}: must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise _lib.VitamdError(f"{name}: expected {ndim}-d, got {t.dim()}-d")
    return t


# ------------------------------------------------------------------------------------------ GEMMs
def gemm_nt(a, b, epi, *, bias=None, aux=None, out=None, out2=None, colsum=None, n_patches=0, seq=0, extra=0,
            out_rows=None, tile=0):
    """out = epilogue(a[M,K] @ b[N,K]^T).  Returns out (and out2 for EPI_GELU / EPI_GELU_DG)."""
    _need(a, BF16, "a", 2); _need(b, BF16, "b", 2)
    M, K = a.shape
    N, K2 = b.shape
    if K != K2:
        raise _lib.VitamdError(f"gemm_nt: K mismatch {K} vs {K2}")
    out_dtype = F32 if epi in (EPI_RESID_F32, EPI_PATCH_F32, EPI_F32) else BF16
    if out is None:
        out = torch.empty((out_rows if out_rows is not None else M, N), dtype=out_dtype, device=a.device)
    _need(out, out_dtype, "out")
    if epi in (EPI_GELU, EPI_GELU_DG) and out2 is None:
        out2 = torch.empty((M, N), dtype=BF16, device=a.device)
    if bias is not None:
        _need(bias, F32, "bias", 1)
    if epi in (EPI_GELU, EPI_GELU_DG):
        init(a.device)
    if tile == 0:
        tile = auto_tile(a.device, M, N, K, epi)
    elif tile == _RAW_AUTO:             # the library's own automatic choice, no host-side policy (the probe's seam arm)
        tile = 0
    code = _nt_launch(a.device, (_p(a), _p(b), _p(out), _p(out2), _p(bias), _p(aux), _p(colsum), M, N, K, N, epi,
                                 n_patches, seq, extra, tile))
    _lib.check(code, f"gemm_nt[M={M},N={N},K={K},epi={epi}]")
    return (out, out2) if epi in (EPI_GELU, EPI_GELU_DG) else out


def seam_enabled(device):
    """The seam form's switch for `device`: the process-wide override, else this device's probe result, else None (not probed yet)."""
    if NT_SEAM is not None:
        return NT_SEAM
    idx = device.index if device.index is not None else torch.cuda.current_device()
    rec = SEAM_PROBE.get(idx)
    return None if rec is None else rec["enabled"]


def auto_tile(device, M, N, K, epi):
    """The ABI `tile` code behind tile = 0: 512 (one workgroup per tile) when persistent launches are off; 1024 (persistent, no seam form) on a
    device whose seam / loader forms are switched off - ALWAYS, whatever the shape: the library treats 1024 as plain auto where its seam rule would not
    apply anyway; 0 otherwise.  The device is probed the first time the library's own rule (vitamd_gemm_nt_plan) would pick the seam or the loader form for a
    launch; never inside a stream capture (the form then stays on, unrecorded, until an eager launch probes)."""
    if not NT_PERSISTENT:
        return 512
    on = seam_enabled(device)
    if on is None:
        if _L().vitamd_gemm_nt_plan(M, N, K, N, epi, 0) & 0x7f not in (NT_FORM_SEAM, NT_FORM_LOADER) or torch.cuda.is_current_stream_capturing():
            return 0
        on = seam_probe(device)
    return 0 if on else 1024


def seam_probe(device, rows=49152, reps=3):
    """Time the seam form against the plain persistent form (QKV shape of ViT-B at `rows` rows: 192 x 9 tiles = 6.75 per CU, K = 768; the seam form is worth ~5 % there and costs ~5 % at 3.4 tiles per CU) on `device`; the result is kept per device in SEAM_PROBE.
    ~3 ms once per process and device."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    x = torch.randn(rows, 768, device=device).to(BF16)
    w = torch.randn(2304, 768, device=device).mul_(0.03).to(BF16)
    out = torch.empty((rows, 2304), dtype=BF16, device=device)
    times = {}
    for name, tile in (("seam_us", _RAW_AUTO), ("plain_us", 1024)):
        launch = lambda: gemm_nt(x, w, EPI_BIAS_BF16, out=out, tile=tile)
        launch()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            launch()
        e.record()
        e.synchronize()
        times[name] = s.elapsed_time(e) / reps * 1e3
    on = times["seam_us"] <= 1.25 * times["plain_us"]           # the probe guards against a pathologically slow store path, not against a 5 % difference
    SEAM_PROBE[device.index] = {"seam_us": round(times["seam_us"], 1), "plain_us": round(times["plain_us"], 1), "enabled": on}
    if not on:
        import warnings
        warnings.warn(f"vitamd: the seam form of the NT GEMM is slower than the plain persistent form on {device} "
                      f"({times['seam_us']:.0f} vs {times['plain_us']:.0f} us): switched off for this device")
    return on


_WORKSPACES = {}


def _workspace(device, nbytes):
    """split-K scratch, one per (device, stream): kernels on different streams never share it"""
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _WORKSPACES[key] = torch.empty((nbytes + 3) // 4, dtype=F32, device=device)
    return ws


NT_SPLITS = 0             # split-K of the NT GEMMs that take the 128x128 kernel on fewer tiles than the device has CUs (the kept-row layer, the classifier
                          # head: include/vitamd.h vitamd_gemm_nt_bf16_ws): 0 = the library's rule, 1 = never (the unsplit kernel: tests, A/B), n = n splits.
                          # Read on every call.  Results differ from the unsplit kernel's by fp32 summation order only, and are the same in every run.
NT_FORM_SPLITK = _H["VITAMD_NT_FORM_SPLITK"]        # (vitamd_gemm_nt_ws_plan)


def _nt_launch(device, args):
    """vitamd_gemm_nt_bf16 on `args` (everything but the stream), or its workspace form where the library would split this launch.  The partial
    tiles go to this stream's split-K scratch (_workspace: launches of one stream run one after the other, so the weight-gradient GEMMs share
    it).  Inside a stream capture the scratch is not grown: a launch it is too small for stays unsplit (an eager step before the capture, as
    GraphedStep makes, has sized it)."""
    L = _L()
    M, N, K, ldo, epi, tile = args[7], args[8], args[9], args[10], args[11], args[15]
    need = L.vitamd_gemm_nt_ws_bytes(M, N, K, ldo, epi, tile, NT_SPLITS) if NT_SPLITS != 1 else 0
    if need > 0 and torch.cuda.is_current_stream_capturing():
        ws = _WORKSPACES.get((device, torch.cuda.current_stream().cuda_stream))
        if ws is None or ws.numel() * 4 < need:
            need = 0
    if need <= 0:
        return L.vitamd_gemm_nt_bf16(*args, _stream())
    ws = _workspace(device, need)
    return L.vitamd_gemm_nt_bf16_ws(*args, NT_SPLITS, _p(ws), ws.numel() * 4, _stream())


TN_FORM_SHARED, TN_FORM_EXCLUSIVE = _H["VITAMD_TN_FORM_SHARED"], _H["VITAMD_TN_FORM_EXCLUSIVE"]


def gemm_tn(l, r, out, splits=0, accumulate=True, atomic=False, form=TN_FORM_SHARED, colsum=None):
    """out[P,Q] (fp32) (+)= l[R,P]^T @ r[R,Q].  Split-K partials go through a workspace + reduce
    pass (reproducible) unless atomic=True (fp32 atomics straight into `out`, accumulate only).
    form: TN_FORM_SHARED (8-wave workgroups that leave room on the CU for another stream's LayerNorm waves) or TN_FORM_EXCLUSIVE (12 waves,
    four of them dedicated to the LDS-DMA requests: 15 % faster alone, fills the CU); bit-identical results.
    colsum: fp32 [P], ADDED to: the column sums of l (the bias gradient that goes with this weight gradient), formed beside the MFMAs
    from the tiles the GEMM stages anyway and summed by the reduce pass in a fixed order; `out` does not change by a bit.  Not with atomic=True."""
    _need(l, BF16, "l", 2); _need(r, BF16, "r", 2); _need(out, F32, "out", 2)
    R, P = l.shape
    R2, Q = r.shape
    if R != R2 or tuple(out.shape) != (P, Q):
        raise _lib.VitamdError("gemm_tn: shape mismatch")
    if colsum is not None:
        _need(colsum, F32, "colsum", 1)
        if colsum.numel() != P:
            raise _lib.VitamdError("gemm_tn: colsum must be fp32 [P]")
    if atomic:
        if not accumulate:
            raise _lib.VitamdError("gemm_tn: the atomic form can only accumulate")
        if colsum is not None:
            raise _lib.VitamdError("gemm_tn: the atomic form has no reduce pass to sum colsum in")
        code = _L().vitamd_gemm_tn_bf16(_p(l), _p(r), _p(out), R, P, Q, P, Q, Q, splits, _stream())
    else:
        nbytes = _L().vitamd_gemm_tn_ws_bytes(R, P, Q, splits)
        ws = _workspace(l.device, nbytes)
        if colsum is not None:
            code = _L().vitamd_gemm_tn_bf16_ws_colsum(_p(l), _p(r), _p(out), _p(colsum), R, P, Q, P, Q, Q, splits, _p(ws), ws.numel() * 4,
                                                      int(accumulate), int(form), _stream())
        else:
            code = _L().vitamd_gemm_tn_bf16_ws(_p(l), _p(r), _p(out), R, P, Q, P, Q, Q, splits, _p(ws), ws.numel() * 4, int(accumulate),
                                               int(form), _stream())
    _lib.check(code, f"gemm_tn[R={R},P={P},Q={Q}]")
    return out


# ------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, addend=None, addend2=None, store=True):
    """x fp32 [M,D] (+ addend bf16) -> (x_sum fp32 or x itself, y bf16, mean, rstd).
    addend2 (bf16 [M,D], needs addend): added after addend - x_sum = (x + addend) + addend2, the bits of layernorm_fwd(layernorm_fwd(x, addend)[0],
    addend2) in one pass over x.  store=False (needs addend): x_sum is not written and None is returned in its place, for a caller that only
    needs the sum as this LayerNorm's input."""
    _need(x, F32, "x", 2)
    M, D = x.shape
    y = torch.empty((M, D), dtype=BF16, device=x.device)
    mean = torch.empty((M,), dtype=F32, device=x.device)
    rstd = torch.empty((M,), dtype=F32, device=x.device)
    x_out = None
    if addend is not None:
        _need(addend, BF16, "addend", 2)
        x_out = torch.empty_like(x) if store else None
    if addend2 is not None or not store:
        if addend is None or tuple(addend.shape) != (M, D) or (addend2 is not None and tuple(_need(addend2, BF16, "addend2", 2).shape) != (M, D)):
            raise _lib.VitamdError("layernorm_fwd: addend2 and store=False need addend; the addends are bf16 [M, D] like x")
        code = _L().vitamd_layernorm_fwd_add2(_p(x), _p(addend), _p(addend2), _p(x_out), _p(y), _p(mean), _p(rstd), M, D, LN_EPS, _stream())
        _lib.check(code, f"layernorm_fwd_add2[M={M},D={D}]")
        return x_out, y, mean, rstd
    code = _L().vitamd_layernorm_fwd(_p(x), _p(addend), _p(x_out), _p(y), _p(mean), _p(rstd), M, D, LN_EPS, _stream())
    _lib.check(code, f"layernorm_fwd[M={M},D={D}]")
    return (x_out if addend is not None else x), y, mean, rstd


def layernorm_fwd_keep(x, addend, B, seq, keep, pending=None):
    """Kept-row form: x fp32 [B*seq, D] (the full stream), addend bf16 [B*keep, D] (compact) -> compact (x_sum fp32 [B*keep, D], y bf16,
    mean, rstd); output row b*keep + t = LN(x[b*seq + t] + addend[b*keep + t]), the same per-row arithmetic as layernorm_fwd.
    pending (bf16 [B*seq, D], full size like x): added to x first - row b*keep + t = LN((x[b*seq + t] + pending[b*seq + t]) + addend[b*keep + t]),
    the bits of layernorm_fwd_keep(layernorm_fwd(x, pending)[0], addend, ...) without the full-size sum in memory."""
    _need(x, F32, "x", 2); _need(addend, BF16, "addend", 2)
    D = x.shape[1]
    if x.shape[0] != B * seq or tuple(addend.shape) != (B * keep, D) or not 0 < keep <= seq:
        raise _lib.VitamdError(f"layernorm_fwd_keep: x must be [B*seq, D], addend [B*keep, D], 0 < keep <= seq (B={B}, seq={seq}, keep={keep})")
    Mk = B * keep
    x_out = torch.empty((Mk, D), dtype=F32, device=x.device)
    y = torch.empty((Mk, D), dtype=BF16, device=x.device)
    mean = torch.empty((Mk,), dtype=F32, device=x.device)
    rstd = torch.empty((Mk,), dtype=F32, device=x.device)
    if pending is not None:
        if _need(pending, BF16, "pending", 2).shape != x.shape:
            raise _lib.VitamdError("layernorm_fwd_keep: pending must be bf16 [B*seq, D] like x")
        _lib.check(_L().vitamd_layernorm_fwd_keep_add2(_p(x), _p(pending), _p(addend), _p(x_out), _p(y), _p(mean), _p(rstd), B, seq, keep, D, LN_EPS,
                                                       _stream()), f"layernorm_fwd_keep_add2[B={B},seq={seq},keep={keep},D={D}]")
        return x_out, y, mean, rstd
    _lib.check(_L().vitamd_layernorm_fwd_keep(_p(x), _p(addend), _p(x_out), _p(y), _p(mean), _p(rstd), B, seq, keep, D, LN_EPS, _stream()),
               f"layernorm_fwd_keep[B={B},seq={seq},keep={keep},D={D}]")
    return x_out, y, mean, rstd


XHAT_WIDTHS = (256, 512, 768, 1024)       # (a set, so no header macro: csrc/layernorm.hip register_width() is its other copy) the widths whose LayerNorm backward reads xhat from the forward's bf16 output (register-resident kernels)


def layernorm_bwd(dy, x, mean, rstd, g_res=None, want_bf16=False, colsum=None, dropout=(0.0, 0), xhat=None, keep=None):
    """g = (g_res or 0) + LN'(dy); returns (g fp32, bf16(g) or None).  dropout=(p, seed): the bf16 copy
    also gets that dropout mask (it is then the gradient of a dropped-out Linear output).
    xhat: the forward's bf16 output (= xhat for this non-affine LayerNorm); given, and D in {256,512,768,1024}, the kernel reads
    it instead of recomputing xhat from the fp32 x (2 B instead of 4 B per element of an HBM-bound kernel).
    keep=(seq, k): g_res is COMPACT fp32 [M/seq*k, D] - row b*seq + t adds g_res[b*k + t] when t < k, nothing otherwise.
    x may be None where xhat takes its place (xhat given and D in XHAT_WIDTHS): a forward that did not store the LayerNorm's fp32 input."""
    _need(dy, BF16, "dy", 2)
    if x is not None:
        _need(x, F32, "x", 2)
    M, D = dy.shape if x is None else x.shape
    if x is None and (xhat is None or D not in XHAT_WIDTHS):
        raise _lib.VitamdError(f"layernorm_bwd: without x the backward needs xhat and D in {XHAT_WIDTHS} (D={D})")
    g = torch.empty((M, D), dtype=F32, device=dy.device)
    gb = torch.empty((M, D), dtype=BF16, device=dy.device) if want_bf16 else None
    if g_res is not None:
        _need(g_res, F32, "g_res", 2)
    if keep is not None:
        seq, k = keep
        if g_res is None or M % seq or not 0 < k <= seq or tuple(g_res.shape) != (M // seq * k, D):
            raise _lib.VitamdError(f"layernorm_bwd: keep=({seq}, {k}) needs M % seq == 0 and g_res fp32 [M/seq*k, D]")
        use_xhat = xhat is not None and D in XHAT_WIDTHS
        if use_xhat:
            _need(xhat, BF16, "xhat", 2)
        code = _L().vitamd_layernorm_bwd_keep(_p(dy), _p(xhat if use_xhat else x), _p(mean), _p(rstd), _p(g_res), _p(g), _p(gb), _p(colsum),
                                              M // seq, seq, k, D, int(use_xhat), float(dropout[0]), int(dropout[1]), _stream())
        _lib.check(code, f"layernorm_bwd_keep[M={M},D={D},seq={seq},keep={k}]")
        return g, gb
    if xhat is not None and D in XHAT_WIDTHS:
        _need(xhat, BF16, "xhat", 2)
        code = _L().vitamd_layernorm_bwd_xhat(_p(dy), _p(xhat), _p(rstd), _p(g_res), _p(g), _p(gb), _p(colsum), M, D,
                                              float(dropout[0]), int(dropout[1]), _stream())
        _lib.check(code, f"layernorm_bwd_xhat[M={M},D={D}]")
        return g, gb
    code = _L().vitamd_layernorm_bwd_dropout(_p(dy), _p(x), _p(mean), _p(rstd), _p(g_res), _p(g), _p(gb), _p(colsum), M, D,
                                             float(dropout[0]), int(dropout[1]), _stream())
    _lib.check(code, f"layernorm_bwd[M={M},D={D}]")
    return g, gb


def layernorm_affine_fwd(x, gamma, beta, eps=LN_EPS):
    """x fp32 [M,D] -> (y bf16 = LN(x)*gamma+beta, mean, rstd)."""
    _need(x, F32, "x", 2); _need(gamma, F32, "gamma", 1); _need(beta, F32, "beta", 1)
    M, D = x.shape
    y = torch.empty((M, D), dtype=BF16, device=x.device)
    mean = torch.empty((M,), dtype=F32, device=x.device)
    rstd = torch.empty((M,), dtype=F32, device=x.device)
    _lib.check(_L().vitamd_layernorm_affine_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), M, D, float(eps), _stream()),
               "layernorm_affine_fwd")
    return y, mean, rstd


def layernorm_affine_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, g_res=None, want_bf16=False, colsum=None):
    """returns (g fp32, bf16(g) or None); dgamma / dbeta (fp32 [D]) are accumulated into."""
    _need(dy, BF16, "dy", 2); _need(x, F32, "x", 2); _need(gamma, F32, "gamma", 1)
    _need(dgamma, F32, "dgamma", 1); _need(dbeta, F32, "dbeta", 1)
    M, D = x.shape
    g = torch.empty_like(x)
    gb = torch.empty((M, D), dtype=BF16, device=x.device) if want_bf16 else None
    _lib.check(_L().vitamd_layernorm_affine_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(g_res), _p(g), _p(gb), _p(colsum),
                                                _p(dgamma), _p(dbeta), M, D, _stream()), "layernorm_affine_bwd")
    return g, gb


def layernorm_affine_fwd_f32(x, gamma, beta, eps=LN_EPS):
    """x fp32 [M,D] -> (y fp32 = LN(x)*gamma+beta, mean, rstd): the LayerNorm whose output is not a GEMM operand."""
    _need(x, F32, "x", 2); _need(gamma, F32, "gamma", 1); _need(beta, F32, "beta", 1)
    M, D = x.shape
    y = torch.empty_like(x)
    mean = torch.empty((M,), dtype=F32, device=x.device)
    rstd = torch.empty((M,), dtype=F32, device=x.device)
    _lib.check(_L().vitamd_layernorm_affine_fwd_f32(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), M, D, float(eps), _stream()),
               "layernorm_affine_fwd_f32")
    return y, mean, rstd


def layernorm_affine_bwd_f32(dy, x, mean, rstd, gamma, dgamma, dbeta):
    """dy fp32 -> dx fp32; dgamma / dbeta (fp32 [D]) are accumulated into."""
    _need(dy, F32, "dy", 2); _need(x, F32, "x", 2); _need(gamma, F32, "gamma", 1)
    _need(dgamma, F32, "dgamma", 1); _need(dbeta, F32, "dbeta", 1)
    M, D = x.shape
    g = torch.empty_like(x)
    _lib.check(_L().vitamd_layernorm_affine_bwd_f32(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(g), _p(dgamma), _p(dbeta), M, D,
                                                    _stream()), "layernorm_affine_bwd_f32")
    return g


# ------------------------------------------------------------------------------------------ attention
ATTN_RESID_MAX_N = _H["VITAMD_ATTN_RESID_MAX_N"]    # the fused residual add lives in the register-resident-softmax forward kernel


def attention_fwd(qkv, B, N, H, causal=False, dropout=(0.0, 0), resid=None):
    """qkv bf16 [B*N, 3*H*64] (packed (qkv, head, dh)) -> o bf16 [B*N, H*64], lse2 fp32 [B,H,N].
    dropout=(p, seed): dropout on the softmax probabilities.
    resid (fp32 [B*N, H*64], N <= 256): also returns x1 = resid + o, written by the attention kernel itself -> (o, lse2, x1)."""
    _need(qkv, BF16, "qkv", 2)
    D = H * 64
    if tuple(qkv.shape) != (B * N, 3 * D):
        raise _lib.VitamdError("attention_fwd: qkv must be [B*N, 3*H*64] (head_dim 64 only)")
    o = torch.empty((B * N, D), dtype=BF16, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=F32, device=qkv.device)
    if resid is not None:
        _need(resid, F32, "resid", 2)
        if tuple(resid.shape) != (B * N, D):
            raise _lib.VitamdError("attention_fwd: resid must be [B*N, H*64]")
        x1 = torch.empty_like(resid)
        code = _L().vitamd_attention_fwd_resid(_p(qkv), _p(o), _p(lse), _p(resid), _p(x1), B, N, H, 64, int(causal), float(dropout[0]),
                                               int(dropout[1]), _stream())
        _lib.check(code, f"attention_fwd_resid[B={B},N={N},H={H}]")
        return o, lse, x1
    code = _L().vitamd_attention_fwd(_p(qkv), _p(o), _p(lse), B, N, H, 64, int(causal), float(dropout[0]), int(dropout[1]), _stream())
    _lib.check(code, f"attention_fwd[B={B},N={N},H={H}]")
    return o, lse


def attention_bwd(qkv, o, lse, d_o, B, N, H, causal=False, dbias=None, dropout=(0.0, 0)):
    """dqkv bf16 [B*N, 3*H*64]; the column sums of dqkv (QKV bias gradient) are added to `dbias` if given."""
    _need(qkv, BF16, "qkv", 2); _need(o, BF16, "o", 2); _need(d_o, BF16, "d_o", 2); _need(lse, F32, "lse")
    if dbias is not None:
        _need(dbias, F32, "dbias", 1)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    code = _L().vitamd_attention_bwd(_p(qkv), _p(o), _p(lse), _p(d_o), _p(dqkv), _p(delta), _p(dbias), B, N, H, 64, int(causal),
                                     float(dropout[0]), int(dropout[1]), _stream())
    _lib.check(code, f"attention_bwd[B={B},N={N},H={H}]")
    return dqkv


# include/vitamd.h VITAMD_ATTN_* (vitamd_attention_form): family | key tiles << 4 | query tiles << 8 | flags
ATTN_FWD_SMALL, ATTN_FWD_SMALL8, ATTN_FWD_LOOP, ATTN_FWD_LONG, ATTN_BWD_PIPE, ATTN_BWD_LOOP, ATTN_BWD_LONG = (_H["VITAMD_ATTN_" + _n] for _n in "FWD_SMALL FWD_SMALL8 FWD_LOOP FWD_LONG BWD_PIPE BWD_LOOP BWD_LONG".split())
ATTN_DROP, ATTN_CAUSAL, ATTN_RES, ATTN_KEEP = (_H["VITAMD_ATTN_" + _n] for _n in "DROP CAUSAL RES KEEP".split())


def attention_form(N, causal=False, dropout_p=0.0, resid=False, nq=0, backward=False):
    """The kernels attention_fwd (resid=: its residual form) / attention_bwd (backward=True) would launch at this length, or with nq > 0
    attention_fwd_keep / attention_bwd_keep: the code of include/vitamd.h (family, tile counts and flags of the instantiation; equal codes
    = the same machine code).  Nothing is launched.  A call the entry point would refuse raises VitamdError."""
    code = int(_L().vitamd_attention_form(int(N), int(causal), float(dropout_p), int(bool(resid)), int(nq), int(backward)))
    if code < 0:
        raise _lib.VitamdError(f"attention_form[N={N},causal={int(causal)},p={dropout_p},resid={int(bool(resid))},nq={nq},backward={int(backward)}]: "
                               f"{_lib.ERRORS.get(-code, code)}")
    return code


def attention_form_fields(code):
    """code -> (family, key tiles, query tiles, flags)"""
    return code & 0xf, code >> 4 & 0xf, code >> 8 & 0xf, code & 0xf000


KEEP_FWD, KEEP_BWD = _H["VITAMD_ATTN_KEEP_FWD"], _H["VITAMD_ATTN_KEEP_BWD"]          # the mask bits of vitamd_attention_keep_forms


def attention_keep_forms(N, nq):
    """Which kept-query attention kernels serve (N, nq): a mask of KEEP_FWD (129 <= N <= 256) and KEEP_BWD (33 <= N <= 224, nq <= 128)."""
    return int(_L().vitamd_attention_keep_forms(int(N), int(nq)))


def attention_fwd_keep(qkv, B, N, H, nq):
    """Kept-query forward (non-causal, no dropout): qkv bf16 [B*N, 3*H*64] -> o bf16 COMPACT [B*nq, H*64] (row b*nq + t) for the queries
    t < nq, and lse2 fp32 [B, H, N] of which only [..., :nq] is written.  The kept rows are bit-identical to attention_fwd's."""
    _need(qkv, BF16, "qkv", 2)
    D = H * 64
    if tuple(qkv.shape) != (B * N, 3 * D) or not 0 < nq <= N:
        raise _lib.VitamdError("attention_fwd_keep: qkv must be [B*N, 3*H*64] (head_dim 64 only) and 0 < nq <= N")
    o = torch.empty((B * nq, D), dtype=BF16, device=qkv.device)
    lse = torch.empty((B, H, N), dtype=F32, device=qkv.device)
    _lib.check(_L().vitamd_attention_fwd_keep(_p(qkv), _p(o), _p(lse), B, N, H, 64, nq, _stream()), f"attention_fwd_keep[B={B},N={N},H={H},nq={nq}]")
    return o, lse


def attention_bwd_keep(qkv, o, lse, d_o, B, N, H, nq, dbias=None, delta=None):
    """Kept-query backward: o, d_o bf16 COMPACT [B*nq, H*64]; lse fp32 [B, H, N] (entries [..., :nq] read) -> dense dqkv bf16 [B*N, 3*H*64]
    whose Q rows >= nq are zeros; equal to attention_bwd given d_o zero-padded to N rows.  dbias as in attention_bwd.
    delta: the caller's own scratch fp32 [B, H, N] (entries [..., :nq] are written, the rest left alone); allocated here when None."""
    _need(qkv, BF16, "qkv", 2); _need(o, BF16, "o", 2); _need(d_o, BF16, "d_o", 2); _need(lse, F32, "lse")
    D = H * 64
    if tuple(qkv.shape) != (B * N, 3 * D) or tuple(o.shape) != (B * nq, D) or tuple(d_o.shape) != (B * nq, D) or lse.numel() != B * H * N:
        raise _lib.VitamdError("attention_bwd_keep: qkv [B*N, 3*H*64], o and d_o compact [B*nq, H*64], lse [B, H, N]")
    if dbias is not None:
        _need(dbias, F32, "dbias", 1)
    dqkv = torch.empty_like(qkv)
    if delta is None:
        delta = torch.empty_like(lse)
    else:
        _need(delta, F32, "delta")
        if delta.numel() != B * H * N:
            raise _lib.VitamdError("attention_bwd_keep: delta must be [B, H, N]")
    _lib.check(_L().vitamd_attention_bwd_keep(_p(qkv), _p(o), _p(lse), _p(d_o), _p(dqkv), _p(delta), _p(dbias), B, N, H, 64, nq, _stream()),
               f"attention_bwd_keep[B={B},N={N},H={H},nq={nq}]")
    return dqkv


def linear_dropout_resid(a, b, bias, resid, dropout):
    """out f32 = resid + dropout_p(bf16(a @ b^T + bias)); dropout = (p, seed)."""
    _need(a, BF16, "a", 2); _need(b, BF16, "b", 2); _need(resid, F32, "resid", 2); _need(bias, F32, "bias", 1)
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty((M, N), dtype=F32, device=a.device)
    code = _L().vitamd_linear_dropout_resid_bf16(_p(a), _p(b), _p(out), _p(bias), _p(resid), M, N, K, float(dropout[0]), int(dropout[1]),
                                                 0 if NT_PERSISTENT else 512, _stream())
    _lib.check(code, f"linear_dropout_resid[M={M},N={N},K={K}]")
    return out


# ------------------------------------------------------------------------------------------ helpers
def cast_bf16_dropout(x, dropout):
    _need(x, F32, "x")
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    _lib.check(_L().vitamd_cast_f32_bf16_dropout(_p(x), _p(out), x.numel(), float(dropout[0]), int(dropout[1]), _stream()), "cast_dropout")
    return out


def dropout(x, p, seed, group=1, inplace=False):
    """x (bf16 or fp32) * keep(seed, index // group): training-mode nn.Dropout (group 1) / DropPath (group = elements per sample)."""
    if x.dtype not in (BF16, F32):
        raise _lib.VitamdError(f"dropout: expected bf16 or fp32, got {x.dtype}")
    _need(x, x.dtype, "x")
    out = x if inplace else torch.empty_like(x)
    fn = _L().vitamd_dropout_bf16 if x.dtype == BF16 else _L().vitamd_dropout_f32
    _lib.check(fn(_p(x), _p(out), x.numel(), int(group), float(p), int(seed), _stream()), "dropout")
    return out


def cast_bf16(x):
    _need(x, F32, "x")
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    _lib.check(_L().vitamd_cast_f32_bf16(_p(x), _p(out), x.numel(), _stream()), "cast_f32_bf16")
    return out


def cast_weight(w, want_plain=True, want_transposed=False):
    """fp32 [N,K] weight -> (bf16 [N,K] or None, bf16 [K,N] or None)."""
    _need(w, F32, "w", 2)
    N, K = w.shape
    wb = torch.empty((N, K), dtype=BF16, device=w.device) if want_plain else None
    wbt = torch.empty((K, N), dtype=BF16, device=w.device) if want_transposed else None
    _lib.check(_L().vitamd_cast_transpose_weight(_p(w), _p(wb), _p(wbt), N, K, _stream()), "cast_transpose_weight")
    return wb, wbt


def im2col(img, p):
    _need(img, F32, "img", 4)
    B, C, H, W = img.shape
    out = torch.empty((B * (H // p) * (W // p), C * p * p), dtype=BF16, device=img.device)
    _lib.check(_L().vitamd_im2col_bf16(_p(img), _p(out), B, C, H, W, p, _stream()), "im2col")
    return out


def colsum(x, out=None):
    _need(x, BF16, "x", 2)
    M, N = x.shape
    if out is None:
        out = torch.zeros((N,), dtype=F32, device=x.device)
    _lib.check(_L().vitamd_colsum_bf16(_p(x), _p(out), M, N, N, _stream()), "colsum")
    return out


def embed_bwd(g, B, seq, extra, D):
    """g fp32 [B*seq, D] -> dpos [seq-extra, D], dextra [extra, D], dyp bf16 [B*(seq-extra), D], dbias [D]."""
    _need(g, F32, "g", 2)
    n_p = seq - extra
    dev = g.device
    dpos = torch.zeros((n_p, D), dtype=F32, device=dev)
    dextra = torch.zeros((extra, D), dtype=F32, device=dev)
    dyp = torch.empty((B * n_p, D), dtype=BF16, device=dev)
    dbias = torch.zeros((D,), dtype=F32, device=dev)
    rows = torch.zeros((max(n_p, 1), D), dtype=F32, device=dev)
    _lib.check(_L().vitamd_embed_bwd(_p(g), _p(dpos), _p(dextra) if extra > 0 else None, _p(dyp), _p(dbias), _p(rows), B, seq, extra, D,
                                     _stream()), "embed_bwd")
    return dpos, dextra, dyp, dbias


def vq_nearest(x, codebook):
    """x fp32 [M,d], codebook fp32 [K,d] -> int64 [M] index of the nearest code (first minimum)."""
    _need(x, F32, "x", 2); _need(codebook, F32, "codebook", 2)
    M, d = x.shape
    K, d2 = codebook.shape
    if d != d2:
        raise _lib.VitamdError("vq_nearest: dim mismatch")
    idx = torch.empty((M,), dtype=torch.int64, device=x.device)
    _lib.check(_L().vitamd_vq_nearest(_p(x), _p(codebook), _p(idx), M, K, d, _stream()), "vq_nearest")
    return idx


def conv3x3_fwd(x, w, bias):
    """x fp32 [B,3,H,W], w fp32 [3,3,3,3], bias fp32 [3] or None -> y fp32 [B,3,H,W] (stride 1, zero padding 1)."""
    _need(x, F32, "x", 4); _need(w, F32, "w", 4)
    B, C, H, W = x.shape
    Co = w.shape[0]
    if tuple(w.shape) != (Co, C, 3, 3):
        raise _lib.VitamdError("conv3x3: weight must be [Cout, Cin, 3, 3]")
    y = torch.empty((B, Co, H, W), dtype=F32, device=x.device)
    _lib.check(_L().vitamd_conv3x3_fwd(_p(x), _p(w), _p(bias), _p(y), B, C, Co, H, W, _stream()), f"conv3x3_fwd[Cin={C},Cout={Co}]")
    return y


def conv3x3_bwd(x, w, dy, need_dx=True, need_dw=True, has_bias=True):
    """-> (dx or None, dw or None, db or None), all fp32."""
    _need(x, F32, "x", 4); _need(w, F32, "w", 4); _need(dy, F32, "dy", 4)
    B, C, H, W = x.shape
    Co = w.shape[0]
    if tuple(dy.shape) != (B, Co, H, W):
        raise _lib.VitamdError("conv3x3_bwd: dy shape mismatch")
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.zeros_like(w) if need_dw else None
    db = torch.zeros((Co,), dtype=F32, device=x.device) if (need_dw and has_bias) else None
    _lib.check(_L().vitamd_conv3x3_bwd(_p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), B, C, Co, H, W, _stream()), "conv3x3_bwd")
    return dx, dw, db


# ------------------------------------------------------------------------------------------ KV-cached decoding
SKINNY_MAX_M = _H["VITAMD_SKINNY_MAX_M"]         # vitamd_gemm_skinny_bf16
SKINNY_EPIS = (EPI_BIAS_BF16, EPI_GELU, EPI_RESID_F32, EPI_F32)
DECODE_MAX_LEN = _H["VITAMD_DECODE_MAX_LEN"]    # cache capacity limit


def _need_len(length):
    _need(length, torch.int32, "len")
    if length.numel() != 1:
        raise _lib.VitamdError("len: expected a one-element device int32")
    return length


def _need_cache(k_cache, v_cache, B, H):
    _need(k_cache, BF16, "k_cache", 4); _need(v_cache, BF16, "v_cache", 4)
    if k_cache.shape != v_cache.shape or k_cache.shape[0] != B or k_cache.shape[1] != H or k_cache.shape[3] != 64:
        raise _lib.VitamdError(f"cache: expected k and v bf16 [B={B}, H={H}, Lmax, 64], got {tuple(k_cache.shape)} / {tuple(v_cache.shape)}")
    Lmax = k_cache.shape[2]
    if not 1 <= Lmax <= DECODE_MAX_LEN:
        raise _lib.VitamdError(f"cache: Lmax must be in [1, {DECODE_MAX_LEN}], got {Lmax}")
    return Lmax


def kv_append(qkv, k_cache, v_cache, length, B, T, H, host_len=None):
    """Copy the k / v slices of qkv bf16 [B*T, 3*H*64] to cache positions len .. len+T-1 of k_cache / v_cache bf16 [B, H, Lmax, 64].
    length: device int32 [1] (read by the kernel).  host_len: the caller's copy of it, checked against Lmax when given."""
    _need(qkv, BF16, "qkv", 2); _need_len(length)
    Lmax = _need_cache(k_cache, v_cache, B, H)
    if tuple(qkv.shape) != (B * T, 3 * H * 64):
        raise _lib.VitamdError(f"kv_append: qkv must be [B*T, 3*H*64] = [{B * T}, {3 * H * 64}], got {tuple(qkv.shape)}")
    if T > Lmax or (host_len is not None and host_len + T > Lmax):
        raise _lib.VitamdError(f"kv_append: len {host_len} + T {T} exceeds the cache length {Lmax}")
    _lib.check(_L().vitamd_kv_append(_p(qkv), _p(k_cache), _p(v_cache), _p(length), B, T, H, 64, Lmax, _stream()),
               f"kv_append[B={B},T={T},H={H},Lmax={Lmax}]")


def decode_attention(qkv, k_cache, v_cache, length, B, H, host_len=None):
    """One query row per sequence: qkv bf16 [B, 3*H*64] (its K/V already appended at position len) against cache positions 0 .. len ->
    o bf16 [B, H*64].  length: device int32 [1]; host_len: the caller's copy, checked (len + 1 <= Lmax) when given."""
    _need(qkv, BF16, "qkv", 2); _need_len(length)
    Lmax = _need_cache(k_cache, v_cache, B, H)
    if tuple(qkv.shape) != (B, 3 * H * 64):
        raise _lib.VitamdError(f"decode_attention: qkv must be [B, 3*H*64] = [{B}, {3 * H * 64}], got {tuple(qkv.shape)}")
    if host_len is not None and host_len + 1 > Lmax:
        raise _lib.VitamdError(f"decode_attention: len {host_len} + 1 exceeds the cache length {Lmax}")
    nbytes = _L().vitamd_decode_attention_ws_bytes(B, H, Lmax)
    if nbytes < 0:
        raise _lib.VitamdError(f"decode_attention[B={B},H={H},Lmax={Lmax}]: {_lib.ERRORS.get(-nbytes, nbytes)}")
    ws = _workspace(qkv.device, nbytes) if nbytes > 0 else None
    o = torch.empty((B, H * 64), dtype=BF16, device=qkv.device)
    _lib.check(_L().vitamd_decode_attention(_p(qkv), _p(k_cache), _p(v_cache), _p(o), _p(length), B, H, 64, Lmax, _p(ws),
                                            0 if ws is None else ws.numel() * 4, _stream()), f"decode_attention[B={B},H={H},Lmax={Lmax}]")
    return o


def gemm_skinny(a, w, epi, *, bias=None, aux=None, out=None):
    """out = epilogue(a[M,K] @ w[N,K]^T) for 1 <= M <= 64 (the decode-step Linears): weights streamed once across the chip, split-K
    partials in the per-stream workspace, summed in a fixed order.  epi: EPI_BIAS_BF16, EPI_GELU (-> (pre, gelu)), EPI_RESID_F32 (aux fp32
    [M,N]) or EPI_F32 (fp32 acc + bias).  Epilogue semantics as gemm_nt's."""
    _need(a, BF16, "a", 2); _need(w, BF16, "w", 2)
    M, K = a.shape
    N, K2 = w.shape
    if K != K2:
        raise _lib.VitamdError(f"gemm_skinny: K mismatch {K} vs {K2}")
    if epi not in SKINNY_EPIS:
        raise _lib.VitamdError(f"gemm_skinny: unsupported epilogue {epi}")
    if not 1 <= M <= SKINNY_MAX_M or N % 4 != 0 or K % 64 != 0:
        raise _lib.VitamdError(f"gemm_skinny[M={M},N={N},K={K}]: needs 1 <= M <= {SKINNY_MAX_M}, N % 4 == 0, K % 64 == 0")
    out_dtype = F32 if epi in (EPI_RESID_F32, EPI_F32) else BF16
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    _need(out, out_dtype, "out", 2)
    out2 = torch.empty((M, N), dtype=BF16, device=a.device) if epi == EPI_GELU else None
    if bias is not None:
        _need(bias, F32, "bias", 1)
        if bias.numel() != N:
            raise _lib.VitamdError(f"gemm_skinny: bias must have {N} elements")
    if epi == EPI_RESID_F32:
        _need(aux, F32, "aux", 2)
        if tuple(aux.shape) != (M, N):
            raise _lib.VitamdError(f"gemm_skinny: aux must be [{M}, {N}]")
    if tuple(out.shape) != (M, N):
        raise _lib.VitamdError(f"gemm_skinny: out must be [{M}, {N}]")
    if epi == EPI_GELU:
        init(a.device)
    nbytes = _L().vitamd_gemm_skinny_ws_bytes(M, N, K)
    ws = _workspace(a.device, nbytes) if nbytes > 0 else None
    code = _L().vitamd_gemm_skinny_bf16(_p(a), _p(w), _p(out), _p(out2), _p(bias), _p(aux) if epi == EPI_RESID_F32 else None, M, N, K, epi,
                                        _p(ws), 0 if ws is None else ws.numel() * 4, _stream())
    _lib.check(code, f"gemm_skinny[M={M},N={N},K={K},epi={epi}]")
    return (out, out2) if epi == EPI_GELU else out


def gemm_skinny_qkv_append(a, w, bias, k_cache, v_cache, length, H, host_len=None):
    """The QKV Linear of a decode step with the K/V append in its store step: qkv bf16 [M, 3*H*64] = gemm_skinny(a, w, EPI_BIAS_BF16,
    bias) (the same bits), and its K / V column ranges also written to row len of k_cache / v_cache bf16 [M, H, Lmax, 64] (the bits
    kv_append(T=1) copies).  1 <= M <= 64; length: device int32 [1]; host_len: the caller's copy, checked (len + 1 <= Lmax) when given."""
    _need(a, BF16, "a", 2); _need(w, BF16, "w", 2); _need_len(length)
    M, K = a.shape
    N, K2 = w.shape
    Lmax = _need_cache(k_cache, v_cache, M, H)
    if K != K2:
        raise _lib.VitamdError(f"gemm_skinny_qkv_append: K mismatch {K} vs {K2}")
    if N != 3 * H * 64:
        raise _lib.VitamdError(f"gemm_skinny_qkv_append: w must be [3*H*64, K] = [{3 * H * 64}, {K}], got {tuple(w.shape)}")
    if not 1 <= M <= SKINNY_MAX_M or K % 64 != 0:
        raise _lib.VitamdError(f"gemm_skinny_qkv_append[M={M},N={N},K={K}]: needs 1 <= M <= {SKINNY_MAX_M}, K % 64 == 0")
    if bias is not None:
        _need(bias, F32, "bias", 1)
        if bias.numel() != N:
            raise _lib.VitamdError(f"gemm_skinny_qkv_append: bias must have {N} elements")
    if host_len is not None and host_len + 1 > Lmax:
        raise _lib.VitamdError(f"gemm_skinny_qkv_append: len {host_len} + 1 exceeds the cache length {Lmax}")
    qkv = torch.empty((M, N), dtype=BF16, device=a.device)
    nbytes = _L().vitamd_gemm_skinny_ws_bytes(M, N, K)
    ws = _workspace(a.device, nbytes) if nbytes > 0 else None
    code = _L().vitamd_gemm_skinny_qkv_append(_p(a), _p(w), _p(qkv), _p(bias), _p(k_cache), _p(v_cache), _p(length), M, H, K, 64, Lmax,
                                              _p(ws), 0 if ws is None else ws.numel() * 4, _stream())
    _lib.check(code, f"gemm_skinny_qkv_append[M={M},H={H},K={K},Lmax={Lmax}]")
    return qkv


def decode_embed(tok_table, pos_table, tokens, length, out=None):
    """x fp32 [B, D] = tok_table[tokens] + pos_table[len] (a single fp32 add, the bits of the torch gather-and-add) with the position read
    from the device: tables fp32 [rows, D], tokens int64 [B] on the device, length device int32 [1].  A token or position outside its
    table leaves that row of `out` as it was (the kernel never reads outside a table)."""
    _need(tok_table, F32, "tok_table", 2); _need(pos_table, F32, "pos_table", 2); _need(tokens, torch.int64, "tokens", 1); _need_len(length)
    B, D = tokens.shape[0], tok_table.shape[1]
    if pos_table.shape[1] != D or D % 4 != 0 or D < 4:
        raise _lib.VitamdError(f"decode_embed: tables must share D with D % 4 == 0, got {tuple(tok_table.shape)} / {tuple(pos_table.shape)}")
    if B < 1:
        raise _lib.VitamdError("decode_embed: expected at least one token")
    if out is None:
        out = torch.empty((B, D), dtype=F32, device=tokens.device)
    _need(out, F32, "out", 2)
    if tuple(out.shape) != (B, D):
        raise _lib.VitamdError(f"decode_embed: out must be [{B}, {D}], got {tuple(out.shape)}")
    _lib.check(_L().vitamd_decode_embed(_p(tok_table), _p(pos_table), _p(tokens), _p(length), _p(out), B, D, tok_table.shape[0],
                                        pos_table.shape[0], _stream()), f"decode_embed[B={B},D={D}]")
    return out


# ------------------------------------------------------------------------------------------ sampled generation
SAMPLE_MAX_V = _H["VITAMD_SAMPLE_MAX_V"]      # vitamd_sample_logits


def check_sampling(temperature, top_k, top_p, V=None):
    """The parameter rules of sample_logits, as ValueError (no device is looked at)."""
    if not (isinstance(temperature, (int, float)) and 0 < temperature < float("inf")):
        raise ValueError(f"sampling: temperature must be a finite number > 0, got {temperature!r}")
    if not (isinstance(top_k, int) and not isinstance(top_k, bool) and top_k >= 0):
        raise ValueError(f"sampling: top_k must be an integer >= 0 (0 = off), got {top_k!r}")
    if not (isinstance(top_p, (int, float)) and 0 < top_p <= 1):
        raise ValueError(f"sampling: top_p must be in (0, 1] (1 = off), got {top_p!r}")
    if V is not None and not 2 <= V <= SAMPLE_MAX_V:
        raise ValueError(f"sampling: the vocabulary must hold 2 .. {SAMPLE_MAX_V} entries, got {V}")


def sample_logits(logits, temperature=1.0, top_k=0, top_p=1.0, *, u=None, seed=0, step=None, return_info=False):
    """One token per row of logits fp32 [B, V] (unit inner stride; the row stride may exceed V): temperature -> top-k (0 = off) -> top-p
    (1 = off) -> draw, in one kernel launch and without host synchronisation (semantics: include/vitamd.h vitamd_sample_logits).
    u: fp32 [B] in [0, 1), the caller's uniform numbers; None = Philox4x32-10 keyed by `seed`, counter (row, step), with `step` a device
    uint64 [1] read by the kernel (None = 0) that the caller advances (Sampler does).  -> tokens int64 [B], and with return_info the kernel's
    account of its decision, fp32 [B, 4] = (smallest kept logit, number kept, kept share of the softmax mass, probability of the token)."""
    V = logits.shape[-1] if isinstance(logits, torch.Tensor) and logits.dim() == 2 else None
    check_sampling(temperature, top_k, top_p, V)
    if not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"sampling: seed must be an integer in [0, 2^64), got {seed!r}")
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise _lib.VitamdError("logits: expected a ROCm device tensor (the HIP kernels are the only implementation)")
    if logits.dtype != F32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        raise _lib.VitamdError(f"logits: expected fp32 [B, V] with unit inner stride, got {logits.dtype} {tuple(logits.shape)} strides {logits.stride()}")
    B, V = logits.shape
    if B < 1:
        raise _lib.VitamdError("logits: expected at least one row")
    if u is not None:
        _need(u, F32, "u", 1)
        if u.numel() != B:
            raise _lib.VitamdError(f"u: expected {B} elements, got {u.numel()}")
    if step is not None:
        _need(step, torch.uint64, "step")
        if step.numel() != 1:
            raise _lib.VitamdError("step: expected a one-element device uint64")
    token = torch.empty((B,), dtype=torch.int64, device=logits.device)
    info = torch.empty((B, 4), dtype=F32, device=logits.device) if return_info else None
    _lib.check(_L().vitamd_sample_logits(_p(logits), _p(token), _p(info), _p(u), _p(step), B, V, logits.stride(0), float(temperature), int(top_k),
                                         float(top_p), seed, _stream()), f"sample_logits[B={B},V={V},T={temperature},top_k={top_k},top_p={top_p}]")
    return (token, info) if return_info else token


# ------------------------------------------------------------------------------------------ training the causal stack
CE_MAX_V = _H["VITAMD_CE_MAX_V"]          # vitamd_cross_entropy_fwd


def cross_entropy_grid_rows(V):
    """rows one sweep of the capped cross-entropy grid covers at this V (asked of the library); more rows make workgroups loop"""
    n = int(_L().vitamd_cross_entropy_grid_rows(int(V)))
    if n < 0:
        raise ValueError(f"cross_entropy: the vocabulary must hold 2 .. {CE_MAX_V} entries, got {V}")
    return n


def _need_logits(logits, name="logits"):
    """[M, V] fp32 or bf16 with unit inner stride (the row stride may exceed V) -> (M, V, ld, is_bf16); V out of range: ValueError"""
    V = logits.shape[-1] if isinstance(logits, torch.Tensor) and logits.dim() == 2 else None
    if V is not None and not 2 <= V <= CE_MAX_V:
        raise ValueError(f"cross_entropy: the vocabulary must hold 2 .. {CE_MAX_V} entries, got {V}")
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda:
        raise _lib.VitamdError(f"{name}: expected a ROCm device tensor (the HIP kernels are the only implementation)")
    if logits.dtype not in (F32, BF16) or logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        raise _lib.VitamdError(f"{name}: expected fp32 or bf16 [M, V] with unit inner stride, got {logits.dtype} {tuple(logits.shape)} "
                               f"strides {logits.stride()}")
    if logits.shape[0] < 1:
        raise _lib.VitamdError(f"{name}: expected at least one row")
    return logits.shape[0], logits.shape[1], logits.stride(0), int(logits.dtype == BF16)


def _need_soft(soft, M):
    """soft = (target_b int64 [M] or None, lam fp32 [M] or None, smoothing) of the soft-target entries -> the same, checked"""
    if not (isinstance(soft, (tuple, list)) and len(soft) == 3):
        raise ValueError("soft: expected (target_b or None, lam or None, smoothing)")
    target_b, lam, smoothing = soft
    smoothing = float(smoothing)
    if not 0.0 <= smoothing <= 1.0:
        raise ValueError(f"soft: smoothing must lie in [0, 1], got {smoothing!r}")
    if lam is not None:
        _need(lam, F32, "lam", 1); _need(target_b, torch.int64, "target_b", 1)
        if lam.numel() != M or target_b.numel() != M:
            raise _lib.VitamdError(f"soft: expected lam [{M}] and target_b [{M}]")
    else:
        target_b = None
    return target_b, lam, smoothing


def cross_entropy_fwd(logits, target, ignore_index=-100, soft=None):
    """Mean cross-entropy of logits fp32 / bf16 [M, V] (unit inner stride) against target int64 [M] over the rows whose target is not
    ignore_index, fp32 arithmetic -> (loss_row fp32 [M], lse fp32 [M], stats fp32 [2] = (mean loss, 1 / count)); semantics:
    include/vitamd.h vitamd_cross_entropy_fwd.  Nothing synchronises: a target outside [0, V) shows as a NaN mean.
    soft = (target_b int64 [M] or None, lam fp32 [M] or None, smoothing): the soft-target loss of vitamd_soft_cross_entropy_fwd
    instead (Mixup / CutMix pairs and label smoothing; the mean is over all rows, ignore_index is not looked at)."""
    M, V, ld, is_bf16 = _need_logits(logits)
    _need(target, torch.int64, "target", 1)
    if target.numel() != M:
        raise _lib.VitamdError(f"target: expected {M} elements, got {target.numel()}")
    if soft is not None:
        soft = _need_soft(soft, M)
    loss_row = torch.empty((M,), dtype=F32, device=logits.device)
    lse = torch.empty((M,), dtype=F32, device=logits.device)
    stats = torch.empty((2,), dtype=F32, device=logits.device)
    if soft is not None:
        _lib.check(_L().vitamd_soft_cross_entropy_fwd(_p(logits), is_bf16, _p(target), _p(soft[0]), _p(soft[1]), soft[2], _p(loss_row), _p(lse),
                                                      _p(stats), M, V, ld, _stream()), f"soft_cross_entropy_fwd[M={M},V={V},ld={ld}]")
        return loss_row, lse, stats
    _lib.check(_L().vitamd_cross_entropy_fwd(_p(logits), is_bf16, _p(target), _p(loss_row), _p(lse), _p(stats), M, V, ld, int(ignore_index),
                                             _stream()), f"cross_entropy_fwd[M={M},V={V},ld={ld}]")
    return loss_row, lse, stats


def cross_entropy_bwd(logits, target, lse, stats, grad_out=None, ignore_index=-100, out=None, out_dtype=None, soft=None):
    """dlogits = (softmax(logits) - onehot(target)) * grad_out / count from the forward's lse and stats; ignored rows are zeros.
    grad_out: device fp32 scalar (None = 1).  out: where to write (fp32 or bf16 [M, V], unit inner stride; `logits` itself = in place);
    None allocates a dense tensor of out_dtype (default: the logits' dtype).  soft: as cross_entropy_fwd's (the forward's own): the
    soft target takes the one-hot's place (vitamd_soft_cross_entropy_bwd)."""
    M, V, ld, is_bf16 = _need_logits(logits)
    if soft is not None:
        soft = _need_soft(soft, M)
    _need(target, torch.int64, "target", 1); _need(lse, F32, "lse", 1); _need(stats, F32, "stats", 1)
    if target.numel() != M or lse.numel() != M or stats.numel() != 2:
        raise _lib.VitamdError(f"cross_entropy_bwd: expected target [{M}], lse [{M}] and stats [2]")
    if grad_out is not None:
        _need(grad_out, F32, "grad_out")
        if grad_out.numel() != 1:
            raise _lib.VitamdError("grad_out: expected a one-element device fp32")
    if out is None:
        out = torch.empty((M, V), dtype=out_dtype or logits.dtype, device=logits.device)
    Mo, Vo, ldo, out_bf16 = _need_logits(out, "out")
    if (Mo, Vo) != (M, V):
        raise _lib.VitamdError(f"out: expected [{M}, {V}], got {tuple(out.shape)}")
    if out.data_ptr() == logits.data_ptr() and (out_bf16 != is_bf16 or ldo != ld):
        raise _lib.VitamdError("cross_entropy_bwd: in place needs the logits' own dtype and stride")
    if soft is not None:
        _lib.check(_L().vitamd_soft_cross_entropy_bwd(_p(logits), is_bf16, _p(target), _p(soft[0]), _p(soft[1]), soft[2], _p(lse), _p(stats),
                                                      _p(grad_out), _p(out), out_bf16, M, V, ld, ldo, _stream()),
                   f"soft_cross_entropy_bwd[M={M},V={V},ld={ld},ldo={ldo}]")
        return out
    _lib.check(_L().vitamd_cross_entropy_bwd(_p(logits), is_bf16, _p(target), _p(lse), _p(stats), _p(grad_out), _p(out), out_bf16, M, V, ld,
                                             ldo, int(ignore_index), _stream()), f"cross_entropy_bwd[M={M},V={V},ld={ld},ldo={ldo}]")
    return out


def _need_embed(ids, tok_table, pos_table, what):
    _need(tok_table, F32, "tok_table", 2); _need(pos_table, F32, "pos_table", 2); _need(ids, torch.int64, "ids", 2)
    B, S = ids.shape
    D = tok_table.shape[1]
    if pos_table.shape[1] != D or D % 4 != 0 or D < 4:
        raise _lib.VitamdError(f"{what}: tables must share D with D % 4 == 0, got {tuple(tok_table.shape)} / {tuple(pos_table.shape)}")
    if B < 1 or not 1 <= S <= pos_table.shape[0]:
        raise _lib.VitamdError(f"{what}: ids [B, S] need B >= 1 and 1 <= S <= {pos_table.shape[0]} positions, got {tuple(ids.shape)}")
    return B, S, D


def embed_tokens_fwd(ids, tok_table, pos_table, out=None):
    """x fp32 [B*S, D] = tok_table[ids] + pos_table[:S] (one fp32 add, the bits of the torch gather-and-add): ids int64 [B, S], tables fp32
    [rows, D], D % 4 == 0.  An id outside the table leaves that row of `out` as it was (the kernel never reads outside a table)."""
    B, S, D = _need_embed(ids, tok_table, pos_table, "embed_tokens_fwd")
    if out is None:
        out = torch.empty((B * S, D), dtype=F32, device=ids.device)
    _need(out, F32, "out", 2)
    if tuple(out.shape) != (B * S, D):
        raise _lib.VitamdError(f"embed_tokens_fwd: out must be [{B * S}, {D}], got {tuple(out.shape)}")
    _lib.check(_L().vitamd_embed_tokens_fwd(_p(tok_table), _p(pos_table), _p(ids), _p(out), B, S, D, tok_table.shape[0], pos_table.shape[0],
                                            _stream()), f"embed_tokens_fwd[B={B},S={S},D={D}]")
    return out


def embed_tokens_bwd(g, ids, dtok, dpos):
    """g fp32 [B*S, D], ids int64 [B, S]: dtok fp32 [tok_rows, D] += the rows of g at their ids (fp32 atomics), dpos fp32 [pos_rows, D]:
    rows < S += the sum over the batch in ascending order (reproducible).  Both are accumulated into."""
    B, S, D = _need_embed(ids, dtok, dpos, "embed_tokens_bwd")
    _need(g, F32, "g", 2)
    if tuple(g.shape) != (B * S, D):
        raise _lib.VitamdError(f"embed_tokens_bwd: g must be [{B * S}, {D}], got {tuple(g.shape)}")
    _lib.check(_L().vitamd_embed_tokens_bwd(_p(g), _p(ids), _p(dtok), _p(dpos), B, S, D, dtok.shape[0], _stream()),
               f"embed_tokens_bwd[B={B},S={S},D={D}]")
    return dtok, dpos


def assemble_tokens_grid_cap():
    """workgroups per launch of the two assembly kernels (asked of the library); more work makes workgroups loop"""
    return int(_L().vitamd_assemble_tokens_grid_cap())


def _need_assemble(what, x_shape, prefix, pos, ids, tok, named):
    """The checks of _need_embed for the assembly ops, dtypes and shapes first (before any device is looked at), then device and
    contiguity of every tensor in `named`.  x_shape: (B, E+S, D) when the [B, E+S, D] tensor is given (the backward's g), else None;
    prefix [E, D] or None (E = 0), pos [pos_rows, D], ids int64 [B, S] with tok [tok_rows, D] in gather mode -> (B, E, S, D)"""
    for name, (t, dtype, ndim) in named.items():
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != ndim:
            raise _lib.VitamdError(f"{what}: {name}: expected a {ndim}-d {dtype} tensor, got "
                                   f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    D = pos.shape[1]
    E = 0 if prefix is None else prefix.shape[0]
    widths = {name: t.shape[-1] for name, (t, dtype, _) in named.items() if dtype == F32}
    if any(w != D for w in widths.values()) or D % 4 != 0 or D < 4:
        raise _lib.VitamdError(f"{what}: prefix, positions, source and output must share D with D % 4 == 0, got {widths}")
    if ids is not None:
        B, S = ids.shape
        if x_shape is not None and tuple(x_shape[:2]) != (B, E + S):
            raise _lib.VitamdError(f"{what}: ids {tuple(ids.shape)} behind a prefix of {E} do not fit {tuple(x_shape)}")
    else:
        B, S = x_shape[0], x_shape[1] - E
    if B < 1 or not 1 <= S <= pos.shape[0] or (tok is not None and tok.shape[0] < 1):
        raise _lib.VitamdError(f"{what}: needs B >= 1, 1 <= S <= {pos.shape[0]} positions (pos_rows >= S) and a table with rows, "
                               f"got B={B}, S={S}, E={E}")
    for name, (t, dtype, ndim) in named.items():
        _need(t, dtype, name, ndim)
    return B, E, S, D


def assemble_tokens_fwd(prefix, pos_table, *, ids=None, tok_table=None, body=None, out=None):
    """x fp32 [B, E+S, D]: x[:, :E] = prefix, x[:, E:] = tok_table[ids] + pos_table[:S] (gather mode) or body + pos_table[:S] (dense mode;
    body fp32 [B, S, D]) - one fp32 add, the bits of the torch embedding / add / expand / cat.  prefix fp32 [E, D] or None.  An id outside
    the table leaves that row of `out` as it was (the kernel never reads outside a table)."""
    if (ids is None) != (tok_table is None) or (ids is None) == (body is None):
        raise _lib.VitamdError("assemble_tokens_fwd: give either ids with a token table or a dense body")
    named = {"pos_table": (pos_table, F32, 2)}
    if prefix is not None:
        named["prefix"] = (prefix, F32, 2)
    if ids is not None:
        named.update(ids=(ids, torch.int64, 2), tok_table=(tok_table, F32, 2))
    else:
        named["body"] = (body, F32, 3)
    if out is not None:
        named["out"] = (out, F32, 3)
    E = prefix.shape[0] if isinstance(prefix, torch.Tensor) and prefix.dim() == 2 else 0
    src_shape = (body.shape[0], body.shape[1] + E) if isinstance(body, torch.Tensor) and body.dim() == 3 else None
    B, E, S, D = _need_assemble("assemble_tokens_fwd", src_shape, prefix, pos_table, ids, tok_table, named)
    if out is None:
        out = torch.empty((B, E + S, D), dtype=F32, device=pos_table.device)
    if tuple(out.shape) != (B, E + S, D):
        raise _lib.VitamdError(f"assemble_tokens_fwd: out must be [{B}, {E + S}, {D}], got {tuple(out.shape)}")
    _lib.check(_L().vitamd_assemble_tokens_fwd(_p(prefix) if E else None, _p(pos_table), _p(tok_table), _p(ids), _p(body), _p(out), B, E, S, D,
                                               0 if tok_table is None else tok_table.shape[0], pos_table.shape[0], _stream()),
               f"assemble_tokens_fwd[B={B},E={E},S={S},D={D}]")
    return out


def assemble_tokens_bwd(g, dprefix, dpos, *, ids=None, dtok=None):
    """g fp32 [B, E+S, D]: dprefix fp32 [E, D] (or None, E = 0) += the sum over the batch of g[:, :E], dpos fp32 [pos_rows, D]: rows < S +=
    that of g[:, E:], both in ascending order (reproducible); with ids int64 [B, S] and dtok fp32 [tok_rows, D] (gather mode) dtok += the
    rows of g[:, E:] at their ids (fp32 atomics).  All are accumulated into.  Dense mode: the body's gradient is the view g[:, E:]."""
    if (ids is None) != (dtok is None):
        raise _lib.VitamdError("assemble_tokens_bwd: ids and dtok go together (gather mode) or are both absent (dense mode)")
    named = {"g": (g, F32, 3), "dpos": (dpos, F32, 2)}
    if dprefix is not None:
        named["dprefix"] = (dprefix, F32, 2)
    if ids is not None:
        named.update(ids=(ids, torch.int64, 2), dtok=(dtok, F32, 2))
    g_shape = tuple(g.shape) if isinstance(g, torch.Tensor) and g.dim() == 3 else None
    B, E, S, D = _need_assemble("assemble_tokens_bwd", g_shape, dprefix, dpos, ids, dtok, named)
    _lib.check(_L().vitamd_assemble_tokens_bwd(_p(g), _p(ids), _p(dprefix) if E else None, _p(dpos), _p(dtok), B, E, S, D,
                                               0 if dtok is None else dtok.shape[0], dpos.shape[0], _stream()),
               f"assemble_tokens_bwd[B={B},E={E},S={S},D={D}]")
    return dprefix, dpos, dtok


# ------------------------------------------------------------------------------------------ training the image tokenizers
VQ_MAX_D = _H["VITAMD_VQ_MAX_D"]             # vitamd_vq_quantize_fwd: wider codes stay on vq_nearest and the torch expressions


def _need_vq(x, codebook, what):
    """x fp32 [M, d], codebook fp32 [K, d], 1 <= d <= VQ_MAX_D (shape errors before any device is looked at) -> (M, K, d)"""
    if not isinstance(x, torch.Tensor) or not isinstance(codebook, torch.Tensor) or x.dim() != 2 or codebook.dim() != 2:
        raise _lib.VitamdError(f"{what}: expected x [M, d] and codebook [K, d]")
    (M, d), (K, d2) = x.shape, codebook.shape
    if d != d2 or not 1 <= d <= VQ_MAX_D or M < 1 or K < 1:
        raise ValueError(f"{what}: needs M >= 1 rows, K >= 1 codes and one code width 1 .. {VQ_MAX_D}, got x {tuple(x.shape)}, "
                         f"codebook {tuple(codebook.shape)}")
    _need(x, F32, "x", 2); _need(codebook, F32, "codebook", 2)
    return M, K, d


def _need_g(g_loss, g_recon=None, images=None, name="g_loss"):
    """the upstream gradients of a loss tail: g_loss a one-element device fp32 or None, g_recon fp32 of the images' shape or None"""
    if g_loss is not None:
        _need(g_loss, F32, name)
        if g_loss.numel() != 1:
            raise _lib.VitamdError(f"{name}: expected a one-element device fp32")
    if g_recon is not None:
        _need(g_recon, F32, "g_recon", 4)
        if tuple(g_recon.shape) != tuple(images.shape):
            raise _lib.VitamdError(f"g_recon: expected {tuple(images.shape)}, got {tuple(g_recon.shape)}")


def _vq_quantize_fwd(what, x, codebook, return_unit_codes):
    M, K, d = _need_vq(x, codebook, what)
    dev = x.device
    unit, q = torch.empty((M, d), dtype=F32, device=dev), torch.empty((M, d), dtype=F32, device=dev)
    rnorm = torch.empty((M,), dtype=F32, device=dev)
    idx = torch.empty((M,), dtype=torch.int64, device=dev)
    loss = torch.empty((), dtype=F32, device=dev)
    ws = torch.empty((int(_L().vitamd_vq_quantize_ws_bytes(M, K, d)) // 4,), dtype=F32, device=dev)
    _lib.check(getattr(_L(), "vitamd_" + what)(_p(x), _p(codebook), _p(unit), _p(rnorm), _p(q), _p(idx), _p(loss), _p(ws), M, K, d, _stream()),
               f"{what}[M={M},K={K},d={d}]")
    return (unit, rnorm, q, idx, loss) + ((ws[:K * d].view(K, d),) if return_unit_codes else ())


def _vq_quantize_bwd(what, g_q, g_loss, unit, rnorm, idx, codebook, dcodebook):
    M, K, d = _need_vq(unit, codebook, what)
    _need(rnorm, F32, "rnorm", 1); _need(idx, torch.int64, "idx", 1)
    if rnorm.numel() != M or idx.numel() != M:
        raise _lib.VitamdError(f"{what}: expected rnorm [{M}] and idx [{M}]")
    if g_q is not None:
        _need(g_q, F32, "g_q", 2)
        if tuple(g_q.shape) != (M, d):
            raise _lib.VitamdError(f"g_q: expected [{M}, {d}], got {tuple(g_q.shape)}")
    _need_g(g_loss)
    if dcodebook is None:
        dcodebook = torch.zeros((K, d), dtype=F32, device=unit.device)
    _need(dcodebook, F32, "dcodebook", 2)
    if tuple(dcodebook.shape) != (K, d):
        raise _lib.VitamdError(f"dcodebook: expected [{K}, {d}], got {tuple(dcodebook.shape)}")
    dx = torch.empty((M, d), dtype=F32, device=unit.device)
    _lib.check(getattr(_L(), "vitamd_" + what)(_p(g_q), _p(g_loss), _p(unit), _p(rnorm), _p(idx), _p(codebook), _p(dx), _p(dcodebook), M, K, d,
                                               _stream()), f"{what}[M={M},K={K},d={d}]")
    return dx, dcodebook


def vq_quantize_fwd(x, codebook, return_unit_codes=False):
    """The cosine-similarity quantiser forward (include/vitamd.h vitamd_vq_quantize_fwd): x fp32 [M, d], codebook fp32 [K, d] ->
    (unit [M, d], rnorm [M], q [M, d], idx int64 [M], loss fp32 0-dim); return_unit_codes: the unit codebook the search used as a sixth."""
    return _vq_quantize_fwd("vq_quantize_fwd", x, codebook, return_unit_codes)


def vq_quantize_bwd(g_q, g_loss, unit, rnorm, idx, codebook, dcodebook=None):
    """-> (dx fp32 [M, d], dcodebook fp32 [K, d]).  g_q fp32 [M, d] or None, g_loss device fp32 scalar or None; dcodebook is accumulated
    into when given (else a zeroed one is made).  Semantics: include/vitamd.h vitamd_vq_quantize_bwd."""
    return _vq_quantize_bwd("vq_quantize_bwd", g_q, g_loss, unit, rnorm, idx, codebook, dcodebook)


def recon_mse_applies(tokens, F=None):
    """whether the reconstruction-loss kernels take these tokens (their 16-byte path: aligned base, F and the row stride multiples of 8
    bf16 / 4 fp32 elements, one token within 48 KiB); callers take the torch expressions otherwise"""
    if not isinstance(tokens, torch.Tensor) or tokens.dim() != 2 or tokens.dtype not in (F32, BF16) or tokens.stride(1) != 1:
        return False
    F = tokens.shape[1] if F is None else F
    w = 8 if tokens.dtype == BF16 else 4
    return (F % w == 0 and tokens.stride(0) % w == 0 and tokens.stride(0) >= F and tokens.data_ptr() % 16 == 0
            and F * tokens.element_size() <= 48 * 1024)


def _need_recon(tokens, images, grid, patch, what):
    """tokens fp32 / bf16 [B*grid*grid, patch*patch*c] (unit inner stride), images fp32 [B, c, grid*patch, grid*patch] contiguous ->
    (B, c, ld, is_bf16); shape errors before any device is looked at"""
    if not isinstance(tokens, torch.Tensor) or not isinstance(images, torch.Tensor) or tokens.dim() != 2 or images.dim() != 4:
        raise _lib.VitamdError(f"{what}: expected tokens [B*grid*grid, patch*patch*c] and images [B, c, H, W]")
    B, c, H, Wd = images.shape
    if grid < 1 or patch < 1 or B < 1 or c < 1 or H != grid * patch or Wd != grid * patch or tuple(tokens.shape) != (B * grid * grid, patch * patch * c):
        raise ValueError(f"{what}: tokens {tuple(tokens.shape)} and images {tuple(images.shape)} do not fit grid {grid}, patch {patch}")
    _need(images, F32, "images", 4)
    if not tokens.is_cuda:
        raise _lib.VitamdError(f"{what}: expected ROCm device tensors (the HIP kernels are the only implementation)")
    if tokens.dtype not in (F32, BF16) or tokens.stride(1) != 1 or tokens.stride(0) < tokens.shape[1]:
        raise _lib.VitamdError(f"{what}: tokens must be fp32 or bf16 with unit inner stride, got {tokens.dtype} strides {tokens.stride()}")
    return B, c, tokens.stride(0), int(tokens.dtype == BF16)


def recon_mse_fwd(tokens, images, grid, patch):
    """mean((pixel_shuffle(tokens) - images)^2) as a 0-dim device fp32, the image-shaped tensor never formed (include/vitamd.h
    vitamd_recon_mse_fwd).  Shapes outside the kernel's 16-byte path raise (recon_mse_applies tells beforehand)."""
    B, c, ld, is_bf16 = _need_recon(tokens, images, grid, patch, "recon_mse_fwd")
    nbytes = int(_L().vitamd_recon_mse_ws_bytes(B, grid, patch, c, is_bf16))
    _lib.check(-nbytes if nbytes < 0 else 0, f"recon_mse_fwd[B={B},G={grid},p={patch},c={c}]")
    ws = torch.empty((nbytes // 4,), dtype=F32, device=tokens.device)
    loss = torch.empty((), dtype=F32, device=tokens.device)
    _lib.check(_L().vitamd_recon_mse_fwd(_p(tokens), is_bf16, _p(images), _p(loss), _p(ws), B, grid, patch, c, ld, _stream()),
               f"recon_mse_fwd[B={B},G={grid},p={patch},c={c},ld={ld}]")
    return loss


def _need_tail_out(out, tokens, what):
    """where a tail's backward writes the token gradient: a device tensor of the tokens' shape and dtype; None allocates a dense one"""
    if out is None:
        out = torch.empty(tuple(tokens.shape), dtype=tokens.dtype, device=tokens.device)
    if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != tokens.dtype or tuple(out.shape) != tuple(tokens.shape)
            or out.stride(1) != 1 or out.stride(0) < out.shape[1]):
        raise _lib.VitamdError(f"{what}: out must be a device tensor of the tokens' shape and dtype with unit inner stride")
    return out


def recon_mse_bwd(tokens, images, grid, patch, grad_out=None, out=None):
    """d loss / d tokens = 2 (tokens - pixel_unshuffle(images)) * grad_out / images.numel(), in the tokens' layout and dtype.  grad_out:
    device fp32 scalar (None = 1).  out: where to write (`tokens` itself = in place); None allocates a dense tensor."""
    B, c, ld, is_bf16 = _need_recon(tokens, images, grid, patch, "recon_mse_bwd")
    _need_g(grad_out, name="grad_out")
    out = _need_tail_out(out, tokens, "recon_mse_bwd")
    _lib.check(_L().vitamd_recon_mse_bwd(_p(tokens), is_bf16, _p(images), _p(grad_out), _p(out), B, grid, patch, c, ld, out.stride(0), _stream()),
               f"recon_mse_bwd[B={B},G={grid},p={patch},c={c},ld={ld}]")
    return out


# ------------------------------------------------------------------------------------------ the 1D TiTok tokenizer's kernels
def vq_quantize_unit_fwd(x, codebook, return_unit_codes=False):
    """vq_quantize_fwd with UNIT codes (include/vitamd.h vitamd_vq_quantize_unit_fwd: blocks.VectorQuantizer(use_l2_norm=True)): q and
    the loss are taken on the normalised code rows.  Same arguments and results."""
    return _vq_quantize_fwd("vq_quantize_unit_fwd", x, codebook, return_unit_codes)


def vq_quantize_unit_bwd(g_q, g_loss, unit, rnorm, idx, codebook, dcodebook=None):
    """vq_quantize_bwd with UNIT codes: the codebook gradient goes through the normalisation (include/vitamd.h vitamd_vq_quantize_unit_bwd).
    `codebook` is the raw codebook.  -> (dx fp32 [M, d], dcodebook fp32 [K, d])"""
    return _vq_quantize_bwd("vq_quantize_unit_bwd", g_q, g_loss, unit, rnorm, idx, codebook, dcodebook)


def conv_recon_mse_applies(tokens, patch):
    """whether the pixel-tail kernels take these tokens (their 16-byte path: recon_mse_applies' alignment rules, and a patch side that is
    a multiple of 8 for bf16 / 4 for fp32); callers take the present operators otherwise"""
    if not isinstance(patch, int) or patch < 1 or not recon_mse_applies(tokens):
        return False
    return patch % (8 if tokens.dtype == BF16 else 4) == 0 and tokens.shape[1] == 3 * patch * patch


def _need_conv_recon(tokens, w, bias, images, grid, patch, what):
    """_need_recon with c = 3, w fp32 [3, 3, 3, 3], bias fp32 [3] -> (B, ld, is_bf16); shape errors before any device is looked at"""
    if not isinstance(w, torch.Tensor) or not isinstance(bias, torch.Tensor) or tuple(w.shape) != (3, 3, 3, 3) or tuple(bias.shape) != (3,):
        raise ValueError(f"{what}: expected a convolution weight [3, 3, 3, 3] and bias [3]")
    if isinstance(images, torch.Tensor) and images.dim() == 4 and images.shape[1] != 3:
        raise ValueError(f"{what}: expected three image channels, got images {tuple(images.shape)}")
    B, _, ld, is_bf16 = _need_recon(tokens, images, grid, patch, what)
    _need(w, F32, "conv weight", 4); _need(bias, F32, "conv bias", 1)
    return B, ld, is_bf16


def _conv_recon_ws(B, grid, patch, is_bf16, backward, device, what):
    nbytes = int(_L().vitamd_conv_recon_mse_ws_bytes(B, grid, patch, is_bf16, backward))
    _lib.check(-nbytes if nbytes < 0 else 0, f"{what}[B={B},G={grid},p={patch}]")
    return torch.empty((nbytes // 4,), dtype=F32, device=device)


def conv_recon_mse_fwd(tokens, w, bias, images, grid, patch, want_recon=False):
    """mean((conv3x3(pixel_shuffle(tokens), w, padding 1) + bias - images)^2) as a 0-dim device fp32 and, with want_recon, the convolved
    image fp32 [B, 3, H, W] (else None); the shuffled image is never formed (include/vitamd.h vitamd_conv_recon_mse_fwd).  Shapes outside
    the kernel's 16-byte path raise (conv_recon_mse_applies tells beforehand)."""
    B, ld, is_bf16 = _need_conv_recon(tokens, w, bias, images, grid, patch, "conv_recon_mse_fwd")
    ws = _conv_recon_ws(B, grid, patch, is_bf16, 0, tokens.device, "conv_recon_mse_fwd")
    loss = torch.empty((), dtype=F32, device=tokens.device)
    recon = torch.empty(tuple(images.shape), dtype=F32, device=tokens.device) if want_recon else None
    _lib.check(_L().vitamd_conv_recon_mse_fwd(_p(tokens), is_bf16, _p(w), _p(bias), _p(images), _p(loss), _p(recon), _p(ws), B, grid, patch, ld,
                                              _stream()), f"conv_recon_mse_fwd[B={B},G={grid},p={patch},ld={ld}]")
    return loss, recon


def conv_recon_mse_bwd(tokens, w, bias, images, grid, patch, g_loss=None, g_recon=None, out=None):
    """-> (dtokens in the tokens' layout and dtype, dw fp32 [3, 3, 3, 3], db fp32 [3]) at e = g_loss * 2 (r - images) / images.numel()
    + g_recon.  g_loss: device fp32 scalar (None = 1); g_recon: fp32 [B, 3, H, W] (None = 0).  out: where dtokens go (never the tokens
    themselves); None allocates a dense tensor.  The same bits on every call."""
    B, ld, is_bf16 = _need_conv_recon(tokens, w, bias, images, grid, patch, "conv_recon_mse_bwd")
    _need_g(g_loss, g_recon, images)
    out = _need_tail_out(out, tokens, "conv_recon_mse_bwd")
    if out.data_ptr() == tokens.data_ptr():
        raise _lib.VitamdError("conv_recon_mse_bwd: the gradient cannot overwrite the tokens (neighbouring tiles re-read them)")
    ws = _conv_recon_ws(B, grid, patch, is_bf16, 1, tokens.device, "conv_recon_mse_bwd")
    dw = torch.empty((3, 3, 3, 3), dtype=F32, device=tokens.device)
    db = torch.empty((3,), dtype=F32, device=tokens.device)
    _lib.check(_L().vitamd_conv_recon_mse_bwd(_p(tokens), is_bf16, _p(w), _p(bias), _p(images), _p(g_loss), _p(g_recon), _p(out), _p(dw), _p(db),
                                              _p(ws), B, grid, patch, ld, out.stride(0), _stream()),
               f"conv_recon_mse_bwd[B={B},G={grid},p={patch},ld={ld}]")
    return out, dw, db


# ------------------------------------------------------------------------------------------ the perceptual loss
def _need_dwconv(x, w, what):
    """x fp32 / bf16 rows [B, H, W, C] (channels last, contiguous), w fp32 [C, 7, 7] -> (B, H, W, C, is_bf16); shape errors before any
    device is looked at"""
    if not isinstance(x, torch.Tensor) or not isinstance(w, torch.Tensor) or x.dim() != 4 or w.dim() != 3:
        raise _lib.VitamdError(f"{what}: expected rows [B, H, W, C] and a weight [C, 7, 7]")
    B, H, W, C = x.shape
    if tuple(w.shape) != (C, 7, 7) or C % 4 != 0 or min(B, H, W, C) < 1:
        raise ValueError(f"{what}: needs rows [B, H, W, C] with C % 4 == 0 and a weight [C, 7, 7], got {tuple(x.shape)} and {tuple(w.shape)}")
    if x.dtype not in (F32, BF16):
        raise _lib.VitamdError(f"{what}: rows must be fp32 or bf16, got {x.dtype}")
    _need(x, x.dtype, "rows", 4); _need(w, F32, "w", 3)
    return B, H, W, C, int(x.dtype == BF16)


def dwconv7_fwd(x, w, bias=None):
    """Depthwise 7x7 convolution (stride 1, zero padding 3) on channels-last rows: x fp32 / bf16 [B, H, W, C], w fp32 [C, 7, 7], bias fp32
    [C] or None -> y fp32 [B, H, W, C] (include/vitamd.h vitamd_dwconv7_fwd)."""
    B, H, W, C, is_bf16 = _need_dwconv(x, w, "dwconv7_fwd")
    if bias is not None:
        _need(bias, F32, "bias", 1)
        if bias.numel() != C:
            raise _lib.VitamdError(f"dwconv7_fwd: bias must have {C} elements")
    y = torch.empty((B, H, W, C), dtype=F32, device=x.device)
    _lib.check(_L().vitamd_dwconv7_fwd(_p(x), is_bf16, _p(w), _p(bias), _p(y), B, H, W, C, _stream()), f"dwconv7_fwd[B={B},H={H},W={W},C={C}]")
    return y


def dwconv7_bwd(dy, w, add=None):
    """Its input gradient: dy fp32 / bf16 [B, H, W, C] -> dx fp32 [B, H, W, C] = (add or 0) + conv^T(dy); add: fp32 rows of the same shape
    (the gradient arriving along the residual branch).  No weight gradient: the network is frozen."""
    B, H, W, C, is_bf16 = _need_dwconv(dy, w, "dwconv7_bwd")
    if add is not None:
        _need(add, F32, "add", 4)
        if tuple(add.shape) != (B, H, W, C) or add.data_ptr() == dy.data_ptr():
            raise _lib.VitamdError(f"dwconv7_bwd: add must be other fp32 rows of shape {(B, H, W, C)}")
    dx = torch.empty((B, H, W, C), dtype=F32, device=dy.device)
    _lib.check(_L().vitamd_dwconv7_bwd(_p(dy), is_bf16, _p(w), _p(add), _p(dx), B, H, W, C, _stream()), f"dwconv7_bwd[B={B},H={H},W={W},C={C}]")
    return dx


RESIZE_ROW_LD = _H["VITAMD_RESIZE_ROW_LD"]        # vitamd_resize_norm_fwd: 3 * 4 * 4 = 48 patch values, zero-padded to the GEMM's K % 64 == 0


def _need_band(table, n_index, n_other, name):
    """a band table (start int32 [n_index], taps fp32 [n_index, T]) whose bands lie inside [0, n_other) -> T"""
    start, taps = table
    _need(start, torch.int32, f"{name}.start", 1); _need(taps, F32, f"{name}.taps", 2)
    T = taps.shape[1]
    if start.numel() != n_index or taps.shape[0] != n_index or not 1 <= T <= n_other:
        raise _lib.VitamdError(f"{name}: expected start [{n_index}] and taps [{n_index}, T] with 1 <= T <= {n_other}")
    return T


def resize_norm_fwd(img, table_h, table_w, mean, std, size, want_rows=True, want_nchw=False):
    """Antialiased bilinear resize to size x size, then (x - mean) / std: img fp32 [B, 3, H, W]; table_h / table_w: the band tables of the
    two resize matrices (vitamd.perceptual.band_tables(n_in, size, device)[0], whose bands are inside the image by construction);
    mean, std fp32 with 3 elements -> (rows bf16 [B*(size/4)^2, 64] or None, nchw fp32 [B, 3, size, size] or None)."""
    if not isinstance(img, torch.Tensor) or img.dim() != 4 or img.shape[1] != 3 or min(img.shape) < 1 or size < 4 or size % 4 != 0:
        raise ValueError(f"resize_norm_fwd: needs images [B, 3, H, W] and size % 4 == 0, got {tuple(getattr(img, 'shape', ()))} and size {size}")
    if not (want_rows or want_nchw):
        raise ValueError("resize_norm_fwd: nothing to write")
    _need(img, F32, "img", 4); _need(mean, F32, "mean"); _need(std, F32, "std")
    B, _, H, W = img.shape
    if mean.numel() != 3 or std.numel() != 3:
        raise _lib.VitamdError("resize_norm_fwd: mean and std must have 3 elements")
    Th, Tw = _need_band(table_h, size, H, "table_h"), _need_band(table_w, size, W, "table_w")
    rows = torch.empty((B * (size // 4) ** 2, RESIZE_ROW_LD), dtype=BF16, device=img.device) if want_rows else None
    nchw = torch.empty((B, 3, size, size), dtype=F32, device=img.device) if want_nchw else None
    _lib.check(_L().vitamd_resize_norm_fwd(_p(img), _p(table_h[0]), _p(table_h[1]), Th, _p(table_w[0]), _p(table_w[1]), Tw, _p(mean), _p(std),
                                           _p(rows), _p(nchw), B, 3, H, W, size, _stream()), f"resize_norm_fwd[B={B},H={H},W={W},S={size}]")
    return rows, nchw


def resize_norm_bwd(g_rows, table_h_t, table_w_t, std, B, H, W, size):
    """Backward of resize_norm_fwd: g_rows fp32 [B*(size/4)^2, ld >= 48] in the patch-row layout -> dimg fp32 [B, 3, H, W]; the tables
    are those of the transposed matrices (band_tables(...)[1])."""
    if size < 4 or size % 4 != 0 or min(B, H, W) < 1:
        raise ValueError(f"resize_norm_bwd: needs B, H, W >= 1 and size % 4 == 0, got {(B, H, W)} and size {size}")
    if not isinstance(g_rows, torch.Tensor) or g_rows.dim() != 2 or g_rows.shape[0] != B * (size // 4) ** 2 or g_rows.shape[1] < 48:
        raise ValueError(f"resize_norm_bwd: g_rows must be [{B * (size // 4) ** 2}, >= 48], got {tuple(getattr(g_rows, 'shape', ()))}")
    _need(g_rows, F32, "g_rows", 2); _need(std, F32, "std")
    Th, Tw = _need_band(table_h_t, H, size, "table_h_t"), _need_band(table_w_t, W, size, "table_w_t")
    dimg = torch.empty((B, 3, H, W), dtype=F32, device=g_rows.device)
    _lib.check(_L().vitamd_resize_norm_bwd(_p(g_rows), g_rows.shape[1], _p(table_h_t[0]), _p(table_h_t[1]), Th, _p(table_w_t[0]), _p(table_w_t[1]),
                                           Tw, _p(std), _p(dimg), B, 3, H, W, size, _stream()), f"resize_norm_bwd[B={B},H={H},W={W},S={size}]")
    return dimg


# ------------------------------------------------------------------------------------------ device input pipeline
def frames_prep_grid_cap():
    """workgroups one launch of the frame kernels has at most (asked of the library); more work makes them loop"""
    return int(_L().vitamd_frames_prep_grid_cap())


def frames_prep_resize_grid_cap():
    """workgroups one launch of the resizing frame kernels has at most (asked of the library); more tiles make them loop"""
    return int(_L().vitamd_frames_prep_resize_grid_cap())


FRAMES_MAX_SIZE = _H["VITAMD_FRAMES_MAX_SIZE"]      # of Hs, Ws, H, W where the kernel resizes (vitamd_frames_prep_resize)


def check_frames(src_shape, out_hw, patch=None, B=None, has_index=False, resize=False):
    """The shape rules of vitamd_frames_prep as ValueError, without looking at a device: src [Nsrc, Hs, Ws, C] -> B samples of out_hw.
    resize=True: those of vitamd_frames_prep_resize (the output may be larger than the source; no size beyond 8192).
    -> (B, Nsrc, Hs, Ws, C, H, W)"""
    if len(src_shape) != 4:
        raise ValueError(f"frames: expected uint8 [N, Hs, Ws, C] (channels last), got shape {tuple(src_shape)}")
    Nsrc, Hs, Ws, C = (int(v) for v in src_shape)
    H, W = (int(v) for v in out_hw)
    B = Nsrc if B is None else int(B)
    if min(B, Nsrc, Hs, Ws, H, W) < 1 or not 1 <= C <= 4:
        raise ValueError(f"frames: every size must be >= 1 and C in 1..4, got src {tuple(src_shape)}, out {(H, W)}, B {B}")
    if resize:
        if max(Hs, Ws, H, W) > FRAMES_MAX_SIZE:
            raise ValueError(f"frames: the resizing kernel takes sizes up to {FRAMES_MAX_SIZE}, got src {(Hs, Ws)}, out {(H, W)}")
    elif H > Hs or W > Ws:
        raise ValueError(f"frames: the output {(H, W)} does not fit the source {(Hs, Ws)} (resizing stays with the host loader)")
    if not has_index and Nsrc < B:
        raise ValueError(f"frames: {B} samples need {B} source frames or an index, got {Nsrc}")
    if patch is not None and (not isinstance(patch, int) or patch < 1 or H % patch or W % patch):
        raise ValueError(f"frames: patch {patch!r} does not tile the output {(H, W)}")
    return B, Nsrc, Hs, Ws, C, H, W


def frames_prep(src, out_hw, table, patch=None, image=True, index=None, geom=None, mix=None, resize=None, _resize_mix=False):
    """uint8 frames [Nsrc, Hs, Ws, C] -> (patch rows bf16 [B*gh*gw, C*p*p] or None, image fp32 [B, C, H, W] or None) in one launch
    (semantics, clamps and refusals: include/vitamd.h vitamd_frames_prep).  index int64 [B] or None, geom int32 [B, 3] or None,
    table fp32 [C, 256], all on the device of src.  mix = (rec int32 [B, 6], lam fp32 [B] or None) on that device: Mixup / CutMix on the
    way (vitamd_frames_prep_mix; lam None promises that no row of rec has mode 1).  resize = (box int32 [B, 10], mean fp32 [C] or None,
    std fp32 [C] or None) on that device: the antialiased bilinear resize of vitamd_frames_prep_resize in front of the crop; the record
    carries the crop and the flip and mean / std stand where the table stood, so table and geom must be None, and mix is refused:
    mixing resized samples is frames_prep_resize_mix's route.  That function alone sets _resize_mix, and then comes through here with
    both, so that every route of the frame kernels shares these checks and the one pair of output allocations below."""
    if resize is not None and mix is not None and not _resize_mix:
        raise ValueError("frames_prep: give mix or resize, not both (frames_prep_resize_mix mixes resized samples in one launch)")
    if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8:
        raise ValueError(f"frames_prep: src must be a uint8 tensor, got {getattr(src, 'dtype', type(src).__name__)}")
    if patch is None and not image:
        raise ValueError("frames_prep: nothing to write (give a patch size, image=True, or both)")
    if index is not None and (not isinstance(index, torch.Tensor) or index.dim() != 1 or index.numel() < 1):
        raise ValueError("frames_prep: index must be a 1-d int64 tensor with one entry per output sample")
    if resize is not None:
        if not (isinstance(resize, (tuple, list)) and len(resize) == 3):
            raise ValueError("frames_prep: resize must be (box int32 [B, 10], mean fp32 [C] or None, std fp32 [C] or None)")
        if (resize[1] is None) != (resize[2] is None):
            raise ValueError("frames_prep: give mean and std together, or neither")
        if table is not None or geom is not None:
            raise ValueError("frames_prep: with resize= the record carries crop and flip and (mean, std) the normalisation: table and geom must be None")
    B, Nsrc, Hs, Ws, C, H, W = check_frames(src.shape, out_hw, patch, None if index is None else index.numel(), index is not None,
                                            resize=resize is not None)
    _need(src, torch.uint8, "src", 4)
    if resize is None:
        _need(table, F32, "table", 2)
        if tuple(table.shape) != (C, 256):
            raise _lib.VitamdError(f"table: expected [{C}, 256], got {tuple(table.shape)}")
    else:
        _need(resize[0], torch.int32, "box", 2)
        if tuple(resize[0].shape) != (B, 10):
            raise _lib.VitamdError(f"box: expected [{B}, 10], got {tuple(resize[0].shape)}")
        for name, v in (("mean", resize[1]), ("std", resize[2])):
            if v is not None:
                _need(v, F32, name, 1)
                if v.numel() != C:
                    raise _lib.VitamdError(f"{name}: expected [{C}], got {tuple(v.shape)}")
    if index is not None:
        _need(index, torch.int64, "index", 1)
    if geom is not None:
        _need(geom, torch.int32, "geom", 2)
        if tuple(geom.shape) != (B, 3):
            raise _lib.VitamdError(f"geom: expected [{B}, 3], got {tuple(geom.shape)}")
    if mix is not None:
        if not (isinstance(mix, (tuple, list)) and len(mix) == 2):
            raise ValueError("frames_prep: mix must be (rec int32 [B, 6], lam fp32 [B] or None)")
        rec, lam = mix
        _need(rec, torch.int32, "rec", 2)
        if tuple(rec.shape) != (B, 6):
            raise _lib.VitamdError(f"rec: expected [{B}, 6], got {tuple(rec.shape)}")
        if lam is not None:
            _need(lam, F32, "lam", 1)
            if lam.numel() != B:
                raise _lib.VitamdError(f"lam: expected [{B}], got {tuple(lam.shape)}")
    patches = torch.empty((B * (H // patch) * (W // patch), C * patch * patch), dtype=BF16, device=src.device) if patch is not None else None
    img = torch.empty((B, C, H, W), dtype=F32, device=src.device) if image else None
    # the four entries take the same arguments but for what cuts a sample (geom and table, or the resize record) and the mix record at the end
    name = "frames_prep" + ("_resize" if resize is not None else "") + ("_mix" if mix is not None else "")
    args = [_p(src), _p(index), *((_p(geom), _p(table)) if resize is None else (_p(v) for v in resize)), _p(patches), _p(img), B, Nsrc, Hs, Ws, C,
            H, W, patch if patch is not None else 0, *(() if mix is None else (_p(mix[0]), _p(mix[1]))), _stream()]
    _lib.check(getattr(_L(), "vitamd_" + name)(*args), f"{name}[B={B},src={Nsrc}x{Hs}x{Ws}x{C},out={H}x{W},p={patch}]")
    return patches, img


def frames_prep_resize_mix(src, out_hw, patch, image, index, box, mean, std, rec, lam):
    """uint8 frames [Nsrc, Hs, Ws, C] of any size -> (patch rows bf16 or None, image fp32 or None): every sample resized with its own
    row of box int32 [B, 10] and normalised (mean, std fp32 [C], both or neither) as frames_prep(resize=) does, then mixed with its
    partner by rec int32 [B, 6] and lam fp32 [B] (None promises that no row has mode 1) as frames_prep(mix=) does - in one launch
    (include/vitamd.h vitamd_frames_prep_resize_mix).  patch None: no rows; image False: no image; index int64 [B] or None.  Everything
    on the device of src.  The argument checks are those of both routes, and the outputs are frames_prep's."""
    if box is None or rec is None:
        raise ValueError("frames_prep_resize_mix: needs box int32 [B, 10] and rec int32 [B, 6] (frames_prep takes a batch that is only "
                         "resized or only mixed)")
    return frames_prep(src, out_hw, None, patch, image, index, None, mix=(rec, lam), resize=(box, mean, std), _resize_mix=True)


def crop_flip_draw(B, src_hw, out_hw, seed, step, flip=True, device=None, out=None):
    """geom int32 [B, 3] = (y0, x0, flip) per sample from Philox4x32-10 keyed by `seed`, counter (b, 1, step) - include/vitamd.h
    vitamd_crop_flip_draw.  seed and step are Python integers in [0, 2^64): nothing is read back from the device."""
    (Hs, Ws), (H, W) = (int(v) for v in src_hw), (int(v) for v in out_hw)
    if min(B, Hs, Ws, H, W) < 1 or H > Hs or W > Ws:
        raise ValueError(f"crop_flip_draw: needs B >= 1 and 1 <= out {(H, W)} <= src {(Hs, Ws)}, got B {B}")
    for name, v in (("seed", seed), ("step", step)):
        if not isinstance(v, int) or not 0 <= v < 1 << 64:
            raise ValueError(f"crop_flip_draw: {name} must be an integer in [0, 2^64), got {v!r}")
    if out is None:
        out = torch.empty((B, 3), dtype=torch.int32, device=torch.device("cuda") if device is None else device)
    _need(out, torch.int32, "geom", 2)
    if tuple(out.shape) != (B, 3):
        raise _lib.VitamdError(f"geom: expected [{B}, 3], got {tuple(out.shape)}")
    with torch.cuda.device(out.device):
        _lib.check(_L().vitamd_crop_flip_draw(_p(out), B, Hs, Ws, H, W, int(bool(flip)), seed, step, _stream()),
                   f"crop_flip_draw[B={B},src={Hs}x{Ws},out={H}x{W}]")
    return out


def frames_to_u8(img):
    """fp32 [B, C, H, W] -> uint8 [B, H, W, C] = rint(clamp(v, 0, 1) * 255), NaN -> 0 (include/vitamd.h vitamd_frames_to_u8)"""
    if not isinstance(img, torch.Tensor) or img.dim() != 4 or min(img.shape) < 1 or img.shape[1] > 4:
        raise ValueError(f"frames_to_u8: needs fp32 [B, C <= 4, H, W], got shape {tuple(getattr(img, 'shape', ()))}")
    _need(img, F32, "img", 4)
    B, C, H, W = img.shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8, device=img.device)
    _lib.check(_L().vitamd_frames_to_u8(_p(img), _p(out), B, C, H, W, _stream()), f"frames_to_u8[B={B},C={C},H={H},W={W}]")
    return out


# ------------------------------------------------------------------------------------------ the Enhancing ViT-VQGAN kernels
TANH_SWEEP_ELEMS = 2048 * 256 * 8     # include/vitamd.h vitamd_tanh_bf16: elements one sweep of the grid-stride loop covers under its grid cap


def _need_tanh_out(out, like, what):
    if out is None:
        return torch.empty(like.shape, dtype=BF16, device=like.device)
    _need(out, BF16, f"{what}: out")
    if tuple(out.shape) != tuple(like.shape) or out.device != like.device:
        raise _lib.VitamdError(f"{what}: out must have the input's shape {tuple(like.shape)} on its device, got {tuple(out.shape)}")
    return out


def tanh_bf16(pre, out=None):
    """bf16(tanh(float(pre))) on a contiguous bf16 tensor of any shape and any element offset (include/vitamd.h vitamd_tanh_bf16).
    out: where to write (`pre` itself = in place); None allocates."""
    _need(pre, BF16, "tanh_bf16: pre")
    if pre.numel() < 1:
        raise _lib.VitamdError("tanh_bf16: needs at least one element")
    out = _need_tanh_out(out, pre, "tanh_bf16")
    _lib.check(_L().vitamd_tanh_bf16(_p(pre), _p(out), pre.numel(), _stream()), f"tanh_bf16[n={pre.numel()}]")
    return out


def tanh_bwd_bf16(dh, t, out=None):
    """bf16(float(dh) * (1 - float(t)^2)) from the saved tanh OUTPUT t (include/vitamd.h vitamd_tanh_bwd_bf16).  out: where to write
    (`dh` itself = in place); None allocates."""
    _need(dh, BF16, "tanh_bwd_bf16: dh"); _need(t, BF16, "tanh_bwd_bf16: t")
    if dh.numel() < 1 or tuple(dh.shape) != tuple(t.shape) or dh.device != t.device:
        raise _lib.VitamdError(f"tanh_bwd_bf16: dh {tuple(dh.shape)} and t {tuple(t.shape)} must be non-empty, of one shape, on one device")
    out = _need_tanh_out(out, dh, "tanh_bwd_bf16")
    _lib.check(_L().vitamd_tanh_bwd_bf16(_p(dh), _p(t), _p(out), dh.numel(), _stream()), f"tanh_bwd_bf16[n={dh.numel()}]")
    return out


recon_l1_applies = recon_mse_applies      # the L1 tail takes what the squared-error kernels take: include/vitamd.h vitamd_recon_l1_fwd


def recon_l1_fwd(tokens, images, grid, patch, want_recon=False):
    """-> (mean |depatchify(tokens) - images| as a 0-dim device fp32, the depatchified tokens fp32 [B, c, H, W] or None).  tokens fp32 /
    bf16 [B*grid*grid, c*patch*patch] in the feature order (c p1 p2) of nn.ConvTranspose2d's weight (include/vitamd.h vitamd_recon_l1_fwd).
    Shapes outside the kernel's 16-byte path raise (recon_l1_applies tells beforehand)."""
    B, c, ld, is_bf16 = _need_recon(tokens, images, grid, patch, "recon_l1_fwd")
    nbytes = int(_L().vitamd_recon_mse_ws_bytes(B, grid, patch, c, is_bf16))
    _lib.check(-nbytes if nbytes < 0 else 0, f"recon_l1_fwd[B={B},G={grid},p={patch},c={c}]")
    ws = torch.empty((nbytes // 4,), dtype=F32, device=tokens.device)
    loss = torch.empty((), dtype=F32, device=tokens.device)
    recon = torch.empty(tuple(images.shape), dtype=F32, device=tokens.device) if want_recon else None
    _lib.check(_L().vitamd_recon_l1_fwd(_p(tokens), is_bf16, _p(images), _p(loss), _p(recon), _p(ws), nbytes, B, grid, patch, c, ld, _stream()),
               f"recon_l1_fwd[B={B},G={grid},p={patch},c={c},ld={ld}]")
    return loss, recon


def recon_l1_bwd(tokens, images, grid, patch, g_loss=None, g_recon=None, out=None):
    """g_loss * sign(depatchify(tokens) - images) / images.numel() + g_recon in the tokens' layout and dtype; sign(0) = 0.  g_loss: device
    fp32 scalar (None = 1); g_recon: fp32 [B, c, H, W] (None = 0).  out: where to write (`tokens` itself = in place); None allocates a
    dense tensor."""
    B, c, ld, is_bf16 = _need_recon(tokens, images, grid, patch, "recon_l1_bwd")
    _need_g(g_loss, g_recon, images)
    out = _need_tail_out(out, tokens, "recon_l1_bwd")
    _lib.check(_L().vitamd_recon_l1_bwd(_p(tokens), is_bf16, _p(images), _p(g_loss), _p(g_recon), _p(out), B, grid, patch, c, ld, out.stride(0),
                                        _stream()), f"recon_l1_bwd[B={B},G={grid},p={patch},c={c},ld={ld}]")
    return out


# ------------------------------------------------------------------------------------------ Random Erasing on the finished batch
ERASE_MAX_BOXES = _H["VITAMD_ERASE_MAX_BOXES"]         # vitamd_frames_erase: K, the boxes one sample's record holds


def frames_erase_grid_cap():
    """workgroups one launch of the erasing kernel has at most (asked of the library); more (sample, box, strip) units make it loop"""
    return int(_L().vitamd_frames_erase_grid_cap())


def frames_erase(patches, image, patch, rec, fill, seed, step, hw=None):
    """Random Erasing IN PLACE on the outputs of frames_prep (include/vitamd.h vitamd_frames_erase): patches bf16 [B*gh*gw, C*patch*patch]
    or None, image fp32 [B, C, H, W] or None (not both None); rec int32 [B, K, 5] = (mode, yl, yh, xl, xh), K <= 8, and fill fp32
    [B, K, 4] or None (zeros), on the same device.  Mode 1 writes fill[b, k, c], mode 2 the N(0, 1) value of (seed, step, b, c, y, x); a
    pixel under several boxes takes the one with the largest k; nothing outside the boxes is touched.  hw = (H, W): needed without an
    image, which otherwise says it.  seed and step are Python integers in [0, 2^64).  Returns nothing."""
    if patches is None and image is None:
        raise ValueError("frames_erase: nothing to erase (give patches, image, or both)")
    if not isinstance(rec, torch.Tensor) or rec.dtype != torch.int32 or rec.dim() != 3 or rec.shape[2] != 5 or not 1 <= rec.shape[1] <= ERASE_MAX_BOXES \
            or rec.shape[0] < 1:
        raise ValueError(f"frames_erase: rec must be int32 [B, K <= {ERASE_MAX_BOXES}, 5], got {getattr(rec, 'dtype', type(rec).__name__)} "
                         f"{tuple(getattr(rec, 'shape', ()))}")
    B, K = int(rec.shape[0]), int(rec.shape[1])
    if fill is not None and (not isinstance(fill, torch.Tensor) or fill.dtype != F32 or tuple(fill.shape) != (B, K, 4)):
        raise ValueError(f"frames_erase: fill must be fp32 [{B}, {K}, 4] or None")
    for name, v in (("seed", seed), ("step", step)):
        if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v < 1 << 64:
            raise ValueError(f"frames_erase: {name} must be an integer in [0, 2^64), got {v!r}")
    if image is not None:
        if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[0] != B or not 1 <= image.shape[1] <= 4 or min(image.shape) < 1:
            raise ValueError(f"frames_erase: image must be fp32 [{B}, C <= 4, H, W], got shape {tuple(getattr(image, 'shape', ()))}")
        if hw is not None and tuple(int(v) for v in hw) != tuple(image.shape[2:]):
            raise ValueError(f"frames_erase: hw {tuple(hw)} is not the image's {tuple(image.shape[2:])}")
        hw = tuple(image.shape[2:])
    elif not (isinstance(hw, (tuple, list, torch.Size)) and len(hw) == 2 and all(isinstance(v, int) and v >= 1 for v in hw)):
        raise ValueError("frames_erase: patch rows alone do not say (H, W): give hw=")
    H, W = int(hw[0]), int(hw[1])
    C = None if image is None else int(image.shape[1])
    if patches is not None:
        if not isinstance(patch, int) or isinstance(patch, bool) or patch < 1 or H % patch or W % patch:
            raise ValueError(f"frames_erase: patch {patch!r} does not tile {(H, W)}")
        rows = B * (H // patch) * (W // patch)
        if not isinstance(patches, torch.Tensor) or patches.dim() != 2 or patches.shape[0] != rows or patches.shape[1] % (patch * patch) \
                or not 1 <= patches.shape[1] // (patch * patch) <= 4 or (C is not None and patches.shape[1] != C * patch * patch):
            raise ValueError(f"frames_erase: patches must be bf16 [{rows}, C * {patch * patch}] with C "
                             f"{'in 1..4' if C is None else '= ' + str(C)}, got shape {tuple(getattr(patches, 'shape', ()))}")
        C = int(patches.shape[1]) // (patch * patch)
        _need(patches, BF16, "patches", 2)
    if image is not None:
        _need(image, F32, "image", 4)
    _need(rec, torch.int32, "rec", 3)
    if fill is not None:
        _need(fill, F32, "fill", 3)
    dev = (patches if patches is not None else image).device
    if any(t is not None and t.device != dev for t in (image, rec, fill)):
        raise _lib.VitamdError("frames_erase: patches, image, rec and fill must be on one device")
    with torch.cuda.device(dev):
        _lib.check(_L().vitamd_frames_erase(_p(patches), _p(image), B, C, H, W, patch if patches is not None else 0, _p(rec), _p(fill), K, seed, step,
                                            _stream()), f"frames_erase[B={B},C={C},out={H}x{W},p={patch},K={K}]")


# ------------------------------------------------------------------------------------------ evaluation
def classify_metrics(logits, target, loss_sum, counts, topk=5, ignore_index=-100, loss_row=None, rank=None):
    """One validation batch, added to counters on the device (include/vitamd.h vitamd_classify_metrics): logits fp32 / bf16 [M, V] (unit
    inner stride, read once as stored) against target int64 [M].  loss_sum fp64 [1] += the sum of the per-row losses, counts int64 [3] +=
    (rows, rows whose target is the argmax, rows whose target is among the topk largest), over the rows whose target is not
    ignore_index.  loss_row fp32 [>= M] and rank int32 [>= M]: the per-row scratch (None: zeros of this call's own); their first M
    elements hold the row losses and the targets' ranks afterwards (-1: ignored).  Nothing synchronises and nothing is read back; a
    target outside [0, V) counts as a wrong row with a NaN loss.  -> (loss_row[:M], rank[:M])."""
    V = logits.shape[-1] if isinstance(logits, torch.Tensor) and logits.dim() == 2 else None
    if not isinstance(topk, int) or isinstance(topk, bool) or topk < 1 or (V is not None and topk > max(V, 2)):
        raise ValueError(f"classify_metrics: topk must be an integer in 1 .. V{'' if V is None else ' = ' + str(V)}, got {topk!r}")
    M, V, ld, is_bf16 = _need_logits(logits)          # V outside 2 .. 65536: its own ValueError
    _need(target, torch.int64, "target", 1)
    if target.numel() != M:
        raise _lib.VitamdError(f"target: expected {M} elements, got {target.numel()}")
    _need(loss_sum, torch.float64, "loss_sum", 1); _need(counts, torch.int64, "counts", 1)
    if loss_sum.numel() != 1 or counts.numel() != 3:
        raise _lib.VitamdError("classify_metrics: expected loss_sum fp64 [1] and counts int64 [3]")
    if loss_row is None:
        loss_row = torch.zeros((M,), dtype=F32, device=logits.device)
    if rank is None:
        rank = torch.zeros((M,), dtype=torch.int32, device=logits.device)
    _need(loss_row, F32, "loss_row", 1); _need(rank, torch.int32, "rank", 1)
    if loss_row.numel() < M or rank.numel() < M:
        raise _lib.VitamdError(f"classify_metrics: loss_row and rank must hold at least {M} elements")
    if any(t.device != logits.device for t in (target, loss_sum, counts, loss_row, rank)):
        raise _lib.VitamdError("classify_metrics: logits, target, the accumulators and the scratch must be on one device")
    with torch.cuda.device(logits.device):
        _lib.check(_L().vitamd_classify_metrics(_p(logits), is_bf16, _p(target), _p(loss_row), _p(rank), _p(loss_sum), _p(counts), M, V, ld, topk,
                                                int(ignore_index), _stream()), f"classify_metrics[M={M},V={V},ld={ld},topk={topk}]")
    return loss_row[:M], rank[:M]


# ------------------------------------------------------------------------------------------ tokenizer evaluation
RECON_METRICS_MAX_DIM = _H["VITAMD_RECON_METRICS_MAX_DIM"]
CODE_HIST_MAX_K = _H["VITAMD_CODE_HIST_MAX_K"]
CODE_HIST_MAX_M = _H["VITAMD_CODE_HIST_MAX_M"]


def recon_metrics_tile():
    """the side of the square tiles one workgroup of vitamd_recon_metrics owns (asked of the library)"""
    return int(_L().vitamd_recon_metrics_tile())


def recon_metrics_grid_cap():
    """workgroups the first launch of vitamd_recon_metrics has at most; more tiles make it loop"""
    return int(_L().vitamd_recon_metrics_grid_cap())


def recon_metrics_ws_bytes(B, C, H, W, ssim=True):
    """bytes of the workspace one call needs (three fp32 partial sums per tile); a refused shape raises"""
    n = int(_L().vitamd_recon_metrics_ws_bytes(int(B), int(C), int(H), int(W), int(bool(ssim))))
    if n < 0:
        _lib.check(-n, f"recon_metrics_ws_bytes[B={B},C={C},H={H},W={W},ssim={int(bool(ssim))}]")
    return n


def code_hist_lds_max_k():
    """the largest codebook vitamd_code_hist counts in LDS; above it the kernel uses global atomics directly"""
    return int(_L().vitamd_code_hist_lds_max_k())


def code_hist_grid_cap():
    return int(_L().vitamd_code_hist_grid_cap())


def recon_metrics(recon, target, sums, count, per_image=None, ws=None, data_range=1.0, clamp=False, ssim=True):
    """One validation batch of image pairs, added to accumulators on the device (include/vitamd_eval.h vitamd_recon_metrics): recon fp32 / bf16
    [B, C, H, W] against target fp32 [B, C, H, W], both contiguous (a view that starts off 16-byte alignment is read element by
    element).  sums fp64 [4] += the sums over the batch of the per-image mse, mae, psnr and ssim; count int64 [1] += B.  per_image fp64
    [>= B, 4] and ws (any dtype, >= recon_metrics_ws_bytes bytes): scratch, None = zeros of this call's own.  clamp limits recon to
    [0, data_range] first (a NaN stays); ssim=False skips the windows (H, W >= 1 suffice; the ssim fields are NaN).  Nothing
    synchronises and nothing is read back.  -> per_image[:B] = (mse_b, mae_b, psnr_b, ssim_b)."""
    if isinstance(data_range, bool) or not isinstance(data_range, (int, float)) or not 0.0 < float(data_range) <= 3.0e38:
        raise ValueError(f"recon_metrics: data_range must be a finite number above 0, got {data_range!r}")
    if not isinstance(clamp, (bool, int)) or not isinstance(ssim, (bool, int)) or clamp not in (0, 1) or ssim not in (0, 1):
        raise ValueError(f"recon_metrics: clamp and ssim are flags (0 / 1), got {clamp!r}, {ssim!r}")
    if not isinstance(recon, torch.Tensor) or recon.dtype not in (F32, BF16):
        raise _lib.VitamdError(f"recon: expected an fp32 or bf16 tensor [B, C, H, W], got {getattr(recon, 'dtype', type(recon).__name__)}")
    _need(recon, recon.dtype, "recon", 4)
    _need(target, F32, "target", 4)
    if recon.shape != target.shape:
        raise _lib.VitamdError(f"recon_metrics: recon {tuple(recon.shape)} and target {tuple(target.shape)} differ in shape")
    B, C, H, W = (int(v) for v in recon.shape)
    lo = 11 if ssim else 1
    if B < 1 or C < 1 or H < lo or W < lo or H > RECON_METRICS_MAX_DIM or W > RECON_METRICS_MAX_DIM:
        raise _lib.VitamdError(f"recon_metrics: shape {tuple(recon.shape)} needs B, C >= 1 and {lo} <= H, W <= {RECON_METRICS_MAX_DIM}"
                               f"{' (an 11 x 11 window must fit)' if ssim else ''}")
    _need(sums, torch.float64, "sums", 1); _need(count, torch.int64, "count", 1)
    if sums.numel() != 4 or count.numel() != 1:
        raise _lib.VitamdError("recon_metrics: expected sums fp64 [4] and count int64 [1]")
    with torch.cuda.device(recon.device):
        need = recon_metrics_ws_bytes(B, C, H, W, ssim)
        if per_image is None:
            per_image = torch.zeros((B, 4), dtype=torch.float64, device=recon.device)
        if ws is None:
            ws = torch.zeros((need // 4,), dtype=F32, device=recon.device)
        _need(per_image, torch.float64, "per_image", 2)
        if per_image.shape[0] < B or per_image.shape[1] != 4:
            raise _lib.VitamdError(f"recon_metrics: per_image must be fp64 [>= {B}, 4], got {tuple(per_image.shape)}")
        if not isinstance(ws, torch.Tensor) or not ws.is_cuda or not ws.is_contiguous() or ws.numel() * ws.element_size() < need:
            raise _lib.VitamdError(f"recon_metrics: ws must be a contiguous device tensor of at least {need} bytes")
        if any(t.device != recon.device for t in (target, sums, count, per_image, ws)):
            raise _lib.VitamdError("recon_metrics: recon, target, the accumulators and the scratch must be on one device")
        _lib.check(_L().vitamd_recon_metrics(_p(recon), int(recon.dtype == BF16), _p(target), _p(per_image), _p(sums), _p(count), _p(ws),
                                             ws.numel() * ws.element_size(), B, C, H, W, float(data_range), int(clamp), int(ssim), _stream()),
                   f"recon_metrics[B={B},C={C},H={H},W={W},clamp={int(clamp)},ssim={int(ssim)}]")
    return per_image[:B]


def code_hist(ids, hist, bad):
    """hist int64 [K] += the occurrences of every id of ids (int64, any shape, contiguous) in [0, K); bad int64 [1] += the ids outside
    that range, which form no address (include/vitamd_eval.h vitamd_code_hist).  Integer atomics: exact and reproducible.  Returns nothing."""
    K = hist.numel() if isinstance(hist, torch.Tensor) else None
    if K is not None and not 2 <= K <= CODE_HIST_MAX_K:
        raise ValueError(f"code_hist: the codebook must hold 2 .. {CODE_HIST_MAX_K} codes, got {K}")
    _need(ids, torch.int64, "ids")
    _need(hist, torch.int64, "hist", 1); _need(bad, torch.int64, "bad", 1)
    M = ids.numel()
    if not 1 <= M <= CODE_HIST_MAX_M or bad.numel() != 1:
        raise _lib.VitamdError(f"code_hist: expected 1 .. {CODE_HIST_MAX_M} ids and bad int64 [1], got {M} ids and bad {tuple(bad.shape)}")
    if hist.device != ids.device or bad.device != ids.device:
        raise _lib.VitamdError("code_hist: ids, hist and bad must be on one device")
    with torch.cuda.device(ids.device):
        _lib.check(_L().vitamd_code_hist(_p(ids), M, K, _p(hist), _p(bad), _stream()), f"code_hist[M={M},K={K}]")
