"""ctypes binding of libvitamd.so (C ABI declared in include/vitamd.h).

The library is built in-tree by `csrc/Makefile` (see __graft_entry__.build).  There is no
fallback: if it is missing, `load()` raises — the product path never routes around the HIP kernels.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvitamd.so")
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
ABI_VERSION = 9

_c = ctypes
_P, _I, _F, _L, _U64, _D, _LL = _c.c_void_p, _c.c_int, _c.c_float, _c.c_long, _c.c_ulonglong, _c.c_double, _c.c_longlong

# name -> argtypes ; every function returns int (VITAMD_OK == 0)
SIGNATURES = {
    "vitamd_abi_version": [],
    "vitamd_init": [_I, _P],
    "vitamd_gemm_nt_plan": [_I, _I, _I, _I, _I, _I],
    "vitamd_gemm_nt_bf16": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "vitamd_gemm_nt_bf16_ws": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _L, _P],
    "vitamd_gemm_nt_ws_bytes": [_I, _I, _I, _I, _I, _I, _I],
    "vitamd_gemm_nt_ws_plan": [_I, _I, _I, _I, _I, _I, _I],
    "vitamd_gemm_tn_bf16": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "vitamd_gemm_tn_bf16_ws": [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _L, _I, _I, _P],
    "vitamd_gemm_tn_bf16_ws_colsum": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _L, _I, _I, _P],
    "vitamd_gemm_tn_ws_bytes": [_I, _I, _I, _I],
    "vitamd_layernorm_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _F, _P],
    "vitamd_layernorm_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "vitamd_layernorm_affine_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _F, _P],
    "vitamd_layernorm_affine_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "vitamd_layernorm_affine_fwd_f32": [_P, _P, _P, _P, _P, _P, _I, _I, _F, _P],
    "vitamd_layernorm_affine_bwd_f32": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "vitamd_attention_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _F, _U64, _P],
    "vitamd_attention_fwd_resid": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _U64, _P],
    "vitamd_attention_bwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _U64, _P],
    "vitamd_layernorm_bwd_dropout": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _F, _U64, _P],
    "vitamd_layernorm_bwd_xhat": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _F, _U64, _P],
    "vitamd_linear_dropout_resid_bf16": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _U64, _I, _P],
    "vitamd_cast_f32_bf16_dropout": [_P, _P, _L, _F, _U64, _P],
    "vitamd_cast_f32_bf16": [_P, _P, _L, _P],
    "vitamd_dropout_bf16": [_P, _P, _L, _L, _F, _U64, _P],
    "vitamd_dropout_f32": [_P, _P, _L, _L, _F, _U64, _P],
    "vitamd_cast_transpose_weight": [_P, _P, _P, _I, _I, _P],
    "vitamd_cast_transpose_batched": [_P, _I, _I, _P],
    "vitamd_im2col_bf16": [_P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_colsum_bf16": [_P, _P, _I, _I, _I, _P],
    "vitamd_embed_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vitamd_vq_nearest": [_P, _P, _P, _I, _I, _I, _P],
    "vitamd_conv3x3_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_conv3x3_bwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_adamw_step": [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _P],
    "vitamd_adamw_step_d": [_P, _P, _P, _P, _L, _F, _D, _D, _F, _F, _I, _P],
    "vitamd_mt_row_bytes": [],
    "vitamd_mt_chunk_elems": [],
    "vitamd_mt_grid_cap": [],
    "vitamd_mt_sumsq": [_P, _P, _I, _I, _P, _P, _F, _P],
    "vitamd_mt_adamw": [_P, _P, _I, _I, _P, _P],
    "vitamd_mt_scale": [_P, _P, _I, _I, _P, _P],
    "vitamd_sched_row_bytes": [],
    "vitamd_sched_advance": [_P, _P, _I, _P],
    "vitamd_kv_append": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_decode_attention_ws_bytes": [_I, _I, _I],
    "vitamd_decode_attention": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _L, _P],
    "vitamd_gemm_skinny_ws_bytes": [_I, _I, _I],
    "vitamd_gemm_skinny_bf16": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _L, _P],
    "vitamd_gemm_skinny_qkv_append": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _L, _P],
    "vitamd_decode_embed": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vitamd_sample_logits": [_P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _F, _U64, _P],
    "vitamd_layernorm_fwd_keep": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "vitamd_layernorm_bwd_keep": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _U64, _P],
    "vitamd_layernorm_fwd_add2": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _F, _P],
    "vitamd_layernorm_fwd_keep_add2": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "vitamd_attention_keep_forms": [_I, _I],
    "vitamd_attention_fwd_keep": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_attention_bwd_keep": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_attention_form": [_I, _I, _F, _I, _I, _I],
    "vitamd_cross_entropy_grid_rows": [_I],
    "vitamd_cross_entropy_fwd": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _LL, _P],
    "vitamd_cross_entropy_bwd": [_P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _LL, _P],
    "vitamd_soft_cross_entropy_fwd": [_P, _I, _P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _P],
    "vitamd_soft_cross_entropy_bwd": [_P, _I, _P, _P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_classify_metrics": [_P, _I, _P, _P, _P, _P, _P, _L, _I, _L, _I, _LL, _P],
    "vitamd_embed_tokens_fwd": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_embed_tokens_bwd": [_P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vitamd_assemble_tokens_grid_cap": [],
    "vitamd_assemble_tokens_fwd": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "vitamd_assemble_tokens_bwd": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "vitamd_vq_quantize_ws_bytes": [_I, _I, _I],
    "vitamd_vq_quantize_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "vitamd_vq_quantize_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "vitamd_recon_mse_ws_bytes": [_I, _I, _I, _I, _I],
    "vitamd_recon_mse_fwd": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_recon_mse_bwd": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "vitamd_vq_quantize_unit_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "vitamd_vq_quantize_unit_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "vitamd_conv_recon_mse_ws_bytes": [_I, _I, _I, _I, _I],
    "vitamd_conv_recon_mse_fwd": [_P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "vitamd_conv_recon_mse_bwd": [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_dwconv7_fwd": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P],
    "vitamd_dwconv7_bwd": [_P, _I, _P, _P, _P, _I, _I, _I, _I, _P],
    "vitamd_resize_norm_fwd": [_P, _P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_resize_norm_bwd": [_P, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P],
    "vitamd_frames_prep": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "vitamd_frames_prep_mix": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    "vitamd_frames_prep_resize": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "vitamd_frames_prep_resize_mix": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    "vitamd_frames_prep_resize_grid_cap": [],
    "vitamd_frames_prep_grid_cap": [],
    "vitamd_crop_flip_draw": [_P, _I, _I, _I, _I, _I, _I, _U64, _U64, _P],
    "vitamd_frames_to_u8": [_P, _P, _I, _I, _I, _I, _P],
    "vitamd_frames_erase": [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _U64, _U64, _P],
    "vitamd_frames_erase_grid_cap": [],
    "vitamd_tanh_bf16": [_P, _P, _L, _P],
    "vitamd_tanh_bwd_bf16": [_P, _P, _P, _L, _P],
    "vitamd_recon_l1_fwd": [_P, _I, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    "vitamd_recon_l1_bwd": [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
}

ERRORS = {1: "unsupported shape", 2: "bad argument", 3: "HIP launch failure", 4: "vitamd_init has not run for this device"}

_lib = None


class VitamdError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile libvitamd.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode != 0:
        raise VitamdError("building libvitamd.so failed")
    return LIB_PATH


def hip_runtimes(maps_path="/proc/self/maps"):
    """The distinct libamdhip64 files mapped into this process (by real path)."""
    found = set()
    with open(maps_path) as fh:
        for line in fh:
            parts = line.split(None, 5)
            if len(parts) == 6 and "libamdhip64" in os.path.basename(parts[5].strip()):
                found.add(os.path.realpath(parts[5].strip()))
    return sorted(found)


def check_single_hip_runtime(maps_path="/proc/self/maps"):
    """Two HIP runtimes in one process - e.g. /opt/rocm's libamdhip64 pulled in by an early dlopen of libvitamd.so AND the copy a PyTorch wheel
    bundles - register kernels with one and pass streams and pointers of the other: the first launch fails with `HIP launch failure` (round 3,
    gpurun_out/r3/smoke_dbg*.log).  Detected here instead of relying on import order: raises VitamdError naming both files."""
    found = hip_runtimes(maps_path)
    if len(found) > 1 and os.environ.get("VITAMD_ALLOW_TWO_HIP_RUNTIMES") != "1":      # (the variable: for a tool that maps a second copy it never launches through)
        raise VitamdError("two HIP runtimes are mapped into this process: " + " and ".join(found) + " - libvitamd.so must resolve libamdhip64 to "
                          "the runtime that owns the caller's streams and pointers (import torch / load the framework BEFORE dlopen-ing libvitamd.so)")
    return found


def load():
    """Load the library (once) and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VitamdError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the HIP kernels are the only implementation of this path; there is no fallback)")
    # torch FIRST: its wheel bundles its own HIP runtime (libamdhip64.so of the ROCm it was built against).  Loaded before torch, libvitamd.so would pull
    # /opt/rocm's copy in and torch then its own: two HIP runtimes in one process - kernels registered with one, streams and pointers from the other -
    # and the first launch fails (seen on a GPU box with `build(); smoke()` in one process).  With torch imported first the library's libamdhip64
    # dependency resolves to the runtime already in the process.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    check_single_hip_runtime()
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.argtypes = argtypes
        fn.restype = ctypes.c_long if name.endswith("_bytes") else ctypes.c_int
    if lib.vitamd_abi_version() != ABI_VERSION:
        raise VitamdError("libvitamd.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        raise VitamdError(f"{what}: {ERRORS.get(code, code)}")
