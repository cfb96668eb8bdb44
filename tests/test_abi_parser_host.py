"""The binding is derived from include/vitamd.h (vitamd/lib.py parse_header).  Here: the parser on hand-written snippets, the derived table
against the hand-written one it replaced, and the host compiler as referee between the derived types, the three numpy record layouts and
the header itself.  No GPU; nothing is loaded or run."""
import ctypes
import os
import re
import subprocess

import pytest

import _abi
from conftest import PKG

_c = ctypes
_P, _I, _F, _L, _U64, _D, _LL = _c.c_void_p, _c.c_int, _c.c_float, _c.c_long, _c.c_ulonglong, _c.c_double, _c.c_longlong

# The table vitamd/lib.py held by hand up to ABI 9, kept as data: test_derived_table_is_the_hand_written_one pins the derivation to it.
SIGNATURES_AT_ABI_9 = {
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


LONG_RETURNS = {"vitamd_gemm_nt_ws_bytes", "vitamd_gemm_tn_ws_bytes", "vitamd_decode_attention_ws_bytes", "vitamd_gemm_skinny_ws_bytes",
                "vitamd_vq_quantize_ws_bytes", "vitamd_recon_mse_ws_bytes", "vitamd_conv_recon_mse_ws_bytes", "vitamd_mt_row_bytes",
                "vitamd_sched_row_bytes"}

SNIPPET = """
/* a header ( with ; , ) in its comments */
#define VITAMD_OK 0
#define VITAMD_FLAG 0x80     /* hex */
#define VITAMD_FAMILY(code) ((code) & 0xf)
#define VITAMD_NOT_A_NUMBER (1 << 4)
int vitamd_three_lines(const float* a,   /* in ( , ; */
                       float* b, // out ) ,
                       int n /* rows; cols */, void* stream);
typedef struct vitamd_mt_row {
  float* p;       /* parameter; (may be NULL) */
  long long n;
  int first_chunk, other;
} vitamd_mt_row;
int vitamd_table(const vitamd_mt_row* rows_host, const void* rows_dev, int n_rows);
int vitamd_wide(const long long* __restrict__ x, unsigned long long seed, long long ignore, long n, double beta, float eps,
                const unsigned char* src);
long vitamd_bytes(void);
int vitamd_cap();
"""


def test_parser_on_snippets():
    from vitamd import lib
    protos, constants = lib.parse_header(SNIPPET)
    assert constants == {"VITAMD_OK": 0, "VITAMD_FLAG": 0x80}                      # function-like and expression macros are not constants
    assert protos == {
        "vitamd_three_lines": ("int", ["const float*", "float*", "int", "void*"]),
        "vitamd_table": ("int", ["const vitamd_mt_row*", "const void*", "int"]),
        "vitamd_wide": ("int", ["const long long*", "unsigned long long", "long long", "long", "double", "float", "const unsigned char*"]),
        "vitamd_bytes": ("long", []),
        "vitamd_cap": ("int", []),
    }


@pytest.mark.parametrize("param", ["size_t n", "unsigned n", "char c", "short s", "unsigned char c", "int", "const float*", "long long",
                                   "vitamd_mt_row row", "struct vitamd_mt_row row"])
def test_parser_refuses_what_it_cannot_type(param):
    """no guessing: an integer type outside the map, a parameter without a name and a by-value struct raise, naming the function"""
    from vitamd import lib
    with pytest.raises(lib.VitamdError, match="vitamd_bad_one"):
        lib.parse_header(f"int vitamd_fine(int a);\nint vitamd_bad_one(float* x, {param}, void* stream);\n")


def test_parser_refuses_another_return_type():
    from vitamd import lib
    for ret in ("long long", "float", "void", "const int"):
        with pytest.raises(lib.VitamdError, match="vitamd_bad_one"):
            lib.parse_header(f"{ret} vitamd_bad_one(int a);")


def test_real_header_counts_and_return_types():
    from vitamd import lib
    assert len(lib.SIGNATURES) == 101 == len(lib.RESTYPES)
    assert {n for n, r in lib.RESTYPES.items() if r is ctypes.c_long} == LONG_RETURNS
    assert all(r is ctypes.c_int for n, r in lib.RESTYPES.items() if n not in LONG_RETURNS)
    counts, returns = _abi.declared()                                              # the tests' own reader agrees with the parser
    assert counts == {n: len(a) for n, a in lib.SIGNATURES.items()}
    assert returns == {n: ret for n, (ret, _) in lib.PROTOTYPES.items()}
    assert lib.CONSTANTS["VITAMD_OK"] == 0 and sorted(lib.ERRORS) == [1, 2, 3, 4]
    assert not any("(" in n for n in lib.CONSTANTS) and "VITAMD_ATTN_FAMILY" not in lib.CONSTANTS


def test_derived_table_is_the_hand_written_one():
    """SIGNATURES_AT_ABI_9 is the table lib.py carried by hand before it was derived; the derivation must reproduce it entry for entry.  A
    later ABI change updates this copy in the same commit that bumps the ABI number."""
    from vitamd import lib
    assert lib.ABI_VERSION == 9
    assert set(lib.SIGNATURES) == set(SIGNATURES_AT_ABI_9)
    for name, argtypes in SIGNATURES_AT_ABI_9.items():
        assert lib.SIGNATURES[name] == argtypes, name


STRUCTS = {"ROW_DTYPE": "vitamd_mt_row", "SCHED_DTYPE": "vitamd_sched_row", "CAST_DTYPE": "vitamd_cast_desc"}


def test_the_compiler_agrees_with_the_binding_and_the_record_layouts(tmp_path):
    """One C++ translation unit over the header: a function pointer of the parser's types initialised from every entry point (C++ refuses
    any difference in a parameter or the return type), and a static_assert on the size of each record and the offset and size of each
    field as the numpy dtypes have them.  -fsyntax-only: any diagnostic fails the test."""
    from vitamd import lib, optim
    lines = ['#include <cstddef>', f'#include "{_abi.HEADER}"']
    for name, (ret, types) in lib.PROTOTYPES.items():
        lines.append(f"{ret} (*chk_{name})({', '.join(types)}) = &{name};")
    for dtype_name, struct in STRUCTS.items():
        assert re.search(r"typedef\s+struct\s+%s\s*\{" % struct, _abi.header()), struct
        dtype = getattr(optim, dtype_name)
        lines.append(f'static_assert(sizeof({struct}) == {dtype.itemsize}, "{struct}");')
        for field in dtype.names:
            lines.append(f'static_assert(offsetof({struct}, {field}) == {dtype.fields[field][1]}, "{struct}.{field}");')
            lines.append(f'static_assert(sizeof((({struct}*)0)->{field}) == {dtype.fields[field][0].itemsize}, "{struct}.{field}");')
    src = tmp_path / "abi_check.cpp"
    src.write_text("\n".join(lines) + "\n")
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", makefile, flags=re.M).group(1)
    r = subprocess.run([hipcc, "-fsyntax-only", "-x", "c++", "-std=c++17", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip() and not r.stdout.strip(), r.stderr + r.stdout
