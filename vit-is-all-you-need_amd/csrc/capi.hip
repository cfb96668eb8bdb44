// extern "C" entry points of libvitamd.so that wrap C++ argument blocks (see include/vitamd.h).
#include "common.h"
#include "vitamd_internal.h"
#include "../../include/vitamd.h"

extern "C" int vitamd_abi_version(void) { return 9; }

// Per-device set-up: the only entry point that allocates (16 KiB: the erf-GELU table) or synchronises.  Idempotent; device < 0 = the current device.
extern "C" int vitamd_init(int device, void* stream) { return vitamd_init_impl(device, (hipStream_t)stream); }

extern "C" int vitamd_gemm_nt_bf16(const void* A, const void* B, void* out, void* out2, const float* bias, const void* aux,
                                   float* colsum, int M, int N, int K, int ldo, int epi, int n_patches, int seq, int extra,
                                   int tile, void* stream) {
  // ABI codes 6 / 7 are the GELU / dGELU epilogues in stored-derivative form (out = gelu'(pre) ; multiply by aux as stored)
  const int dg = (epi == 6 || epi == 7) ? 1 : 0;
  if (epi == 6) epi = EPI_GELU;
  if (epi == 7) epi = EPI_DGELU;
  GemmNtArgs p{A, B, out, out2, bias, aux, colsum, M, N, K, ldo, epi, n_patches, seq, extra, tile, 0u, 1.0f, 0u, 0u, 0, dg};
  if (!is_auto(tile) && tile != NT_TILE_128 && tile != NT_TILE_256 && tile != NT_TILE_320 && tile != NT_TILE_LOADER && tile != NT_TILE_SEAM) return VITAMD_ERR_ARG;
  return vitamd_gemm_nt_impl(p, (hipStream_t)stream);
}

// Which kernel the call above would launch on the current device (no launch, no pointer is read): see include/vitamd.h VITAMD_NT_FORM_*.
extern "C" int vitamd_gemm_nt_plan(int M, int N, int K, int ldo, int epi, int tile) {
  const int dg = (epi == 6 || epi == 7) ? 1 : 0;
  if (epi == 6) epi = EPI_GELU;
  if (epi == 7) epi = EPI_DGELU;
  static char dummy[16];                   // the launch rules only ask whether the optional pointers are present
  GemmNtArgs p{dummy, dummy, dummy, dummy, nullptr, dummy, (float*)dummy, M, N, K, ldo, epi, 1, 1, 0, tile, 0u, 1.0f, 0u, 0u, 0, dg};
  if (!is_auto(tile) && tile != NT_TILE_128 && tile != NT_TILE_256 && tile != NT_TILE_320 && tile != NT_TILE_LOADER && tile != NT_TILE_SEAM) return -VITAMD_ERR_ARG;
  return vitamd_gemm_nt_plan_impl(p);
}

// vitamd_gemm_nt_bf16 with a caller's workspace: launches that take the 128 x 128 kernel on fewer tiles than CUs run its split-K form + reduce pass.
extern "C" int vitamd_gemm_nt_bf16_ws(const void* A, const void* B, void* out, void* out2, const float* bias, const void* aux,
                                      float* colsum, int M, int N, int K, int ldo, int epi, int n_patches, int seq, int extra,
                                      int tile, int splits, float* ws, long ws_bytes, void* stream) {
  const int dg = (epi == 6 || epi == 7) ? 1 : 0;
  if (epi == 6) epi = EPI_GELU;
  if (epi == 7) epi = EPI_DGELU;
  GemmNtArgs p{A, B, out, out2, bias, aux, colsum, M, N, K, ldo, epi, n_patches, seq, extra, tile, 0u, 1.0f, 0u, 0u, 0, dg};
  if (!is_auto(tile) && tile != NT_TILE_128 && tile != NT_TILE_256 && tile != NT_TILE_320 && tile != NT_TILE_LOADER && tile != NT_TILE_SEAM) return VITAMD_ERR_ARG;
  return vitamd_gemm_nt_ws_impl(p, splits, ws, (size_t)(ws_bytes < 0 ? 0 : ws_bytes), (hipStream_t)stream);
}

static GemmNtArgs nt_query_args(int M, int N, int K, int ldo, int epi, int tile) {
  const int dg = (epi == 6 || epi == 7) ? 1 : 0;
  if (epi == 6) epi = EPI_GELU;
  if (epi == 7) epi = EPI_DGELU;
  static char dummy[16];                   // the launch rules only ask whether the optional pointers are present
  return GemmNtArgs{dummy, dummy, dummy, dummy, nullptr, dummy, nullptr, M, N, K, ldo, epi, 1, 1, 0, tile, 0u, 1.0f, 0u, 0u, 0, dg};
}
static bool nt_tile_code_ok(int tile) {
  return is_auto(tile) || tile == NT_TILE_128 || tile == NT_TILE_256 || tile == NT_TILE_320 || tile == NT_TILE_LOADER || tile == NT_TILE_SEAM;
}

extern "C" long vitamd_gemm_nt_ws_bytes(int M, int N, int K, int ldo, int epi, int tile, int splits) {
  if (!nt_tile_code_ok(tile) || splits < 0) return -VITAMD_ERR_ARG;
  return vitamd_gemm_nt_ws_bytes_impl(nt_query_args(M, N, K, ldo, epi, tile), splits);
}

extern "C" int vitamd_gemm_nt_ws_plan(int M, int N, int K, int ldo, int epi, int tile, int splits) {
  if (!nt_tile_code_ok(tile) || splits < 0) return -VITAMD_ERR_ARG;
  return vitamd_gemm_nt_ws_plan_impl(nt_query_args(M, N, K, ldo, epi, tile), splits);
}

extern "C" int vitamd_gemm_tn_bf16(const void* L, const void* Rm, float* out, int R, int P, int Q, int ldl, int ldr, int ldo,
                                   int splits, void* stream) {
  GemmTnArgs a{L, Rm, out, R, P, Q, ldl, ldr, ldo, splits, nullptr, 0, 1, 0};
  return vitamd_gemm_tn_impl(a, (hipStream_t)stream);
}

extern "C" int vitamd_gemm_tn_bf16_ws(const void* L, const void* Rm, float* out, int R, int P, int Q, int ldl, int ldr, int ldo,
                                      int splits, float* ws, long ws_bytes, int accumulate, int form, void* stream) {
  if (form != 0 && form != 1) return VITAMD_ERR_ARG;
  GemmTnArgs a{L, Rm, out, R, P, Q, ldl, ldr, ldo, splits, ws, (size_t)(ws_bytes < 0 ? 0 : ws_bytes), accumulate, form};
  return vitamd_gemm_tn_impl(a, (hipStream_t)stream);
}

extern "C" int vitamd_gemm_tn_bf16_ws_colsum(const void* L, const void* Rm, float* out, float* colsum, int R, int P, int Q, int ldl, int ldr,
                                             int ldo, int splits, float* ws, long ws_bytes, int accumulate, int form, void* stream) {
  if (form != 0 && form != 1) return VITAMD_ERR_ARG;
  GemmTnArgs a{L, Rm, out, R, P, Q, ldl, ldr, ldo, splits, ws, (size_t)(ws_bytes < 0 ? 0 : ws_bytes), accumulate, form, colsum};
  if (colsum && !ws) return VITAMD_ERR_ARG;
  return vitamd_gemm_tn_impl(a, (hipStream_t)stream);
}

// fc2 with dropout: out f32 = resid + dropout_p(bf16(A.B^T + bias)) — reference transformer.py:39-40,44
extern "C" int vitamd_linear_dropout_resid_bf16(const void* A, const void* B, float* out, const float* bias, const float* resid,
                                                int M, int N, int K, float dropout_p, unsigned long long seed, int tile, void* stream) {
  if (!is_auto(tile) && tile != NT_TILE_128 && tile != NT_TILE_256 && tile != NT_TILE_320) return VITAMD_ERR_ARG;
  const DropoutParams d = dropout_params(dropout_p, seed);
  if (!d.ok) return VITAMD_ERR_ARG;
  GemmNtArgs p{A, B, out, nullptr, bias, resid, nullptr, M, N, K, N, EPI_RESID_F32, 0, 0, 0, tile, d.thresh, d.scale, d.seed_lo, d.seed_hi, 0, 0};
  return vitamd_gemm_nt_impl(p, (hipStream_t)stream);
}
