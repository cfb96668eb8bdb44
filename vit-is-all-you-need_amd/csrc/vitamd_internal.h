// Internal (C++) argument blocks shared between the kernel files and capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vitamd.h"

enum GemmEpilogue {              // the first six are the ABI's numbers (include/vitamd.h VITAMD_EPI_*)
  EPI_BIAS_BF16 = VITAMD_EPI_BIAS_BF16,  // out bf16 = bf16(acc + bias)            (bias may be null)
  EPI_GELU = VITAMD_EPI_GELU,            // out bf16 = pre = bf16(acc + bias); out2 bf16 = gelu(pre)
  EPI_RESID_F32 = VITAMD_EPI_RESID_F32,  // out f32  = aux_f32 + bf16(acc + bias)   (residual stream stays fp32)
  EPI_DGELU = VITAMD_EPI_DGELU,          // out bf16 = bf16(bf16(acc) * gelu'(aux_bf16)); colsum[n] += column sums of out
  EPI_PATCH_F32 = VITAMD_EPI_PATCH_F32,  // out f32[b*seq + extra + p] = bf16(acc + bias) + aux_f32[p]  (patch embed + pos_emb)
  EPI_F32 = VITAMD_EPI_F32,              // out f32 = acc
  EPI_DGELU_NOCS = 6, // NOT an ABI code (6 is VITAMD_EPI_GELU_DG there, which capi.hip maps to EPI_GELU + gelu_dg: the two never meet).  A
                      // template argument of the seam / loader kernels only (never GemmNtArgs::epi): EPI_DGELU launched with colsum == null - the
                      // column sums, their butterfly and the atomic compiled out (the bias gradient then comes from the weight-gradient GEMM)
};

// `tile` codes of the NT GEMM entry points (include/vitamd.h documents the numbers; they are part of the C ABI)
enum NtTileCode {
  NT_TILE_AUTO = 0,                   // the library picks kernel, tile height and launch form
  NT_TILE_128 = 128,                  // the 128x128 kernel
  NT_TILE_256 = 256,                  // the ping-pong kernel on 256-row tiles, one workgroup per tile
  NT_TILE_320 = 320,                  // ... on 320-row tiles
  NT_TILE_AUTO_NO_PERSISTENT = 512,   // auto without persistent launches
  NT_TILE_AUTO_NO_SEAM = 1024,        // auto with persistent launches but without the seam / loader forms
  NT_TILE_LOADER = 2048,              // the loader-wave form
  NT_TILE_SEAM = 4096,                // the seam form on 256-row tiles
};
inline bool is_auto(int tile) { return tile == NT_TILE_AUTO || tile == NT_TILE_AUTO_NO_PERSISTENT || tile == NT_TILE_AUTO_NO_SEAM; }

struct GemmNtArgs {
  const void* A;      // [M,K] bf16
  const void* B;      // [N,K] bf16
  void* out;          // [M(or token rows), ldo]
  void* out2;         // EPI_GELU second output
  const float* bias;  // [N] fp32 or null
  const void* aux;    // residual f32 / pre-activation bf16 / pos_emb f32
  float* colsum;      // [N] fp32 atomics target or null
  int M, N, K, ldo;
  int epi;
  int n_patches, seq, extra;  // EPI_PATCH_F32 row remap
  int tile;                   // NtTileCode
  // EPI_RESID_F32 only: dropout on the Linear output before the residual add (reference nn.Dropout, transformer.py:40)
  unsigned drop_thresh;       // p * 2^32, 0 = off
  float drop_scale;           // 1 / (1 - p)
  unsigned drop_seed_lo, drop_seed_hi;
  int row0;                   // global row of this launch's row 0 (tail split): dropout indices stay global
  // stored-derivative GELU (ABI codes VITAMD_EPI_GELU_DG / VITAMD_EPI_DMUL): EPI_GELU writes out = bf16(gelu'(pre)) instead
  // of pre, EPI_DGELU multiplies by aux as stored instead of evaluating gelu'(aux)
  int gelu_dg;
  const unsigned* gelu_tab;   // EPI_GELU: device image of the erf-GELU table (vitamd_init; set by vitamd_gemm_nt_impl for every GELU launch)
};

struct GemmTnArgs {
  const void* L;   // [R, P] bf16 (row stride ldl)
  const void* Rm;  // [R, Q] bf16 (row stride ldr)
  float* out;      // [P, Q] fp32, ACCUMULATED into (atomics)
  int R, P, Q, ldl, ldr, ldo;
  int splits;      // 0 = auto
  float* ws;       // optional split-K workspace: [splits][tiles][256][256] fp32 partial tiles (plain stores) + reduce pass
  size_t ws_bytes;
  int accumulate;  // with a workspace: 1 = out += sum, 0 = out = sum (no pre-zeroing needed)
  int form;        // with a workspace: 0 = 8-wave ping-pong kernel, 1 = 12-wave loader form (VITAMD_TN_FORM_*)
  float* colsum;   // optional, workspace form only: colsum[p] += sum_r L[r,p] (fp32 [P], caller-zeroed); partials behind the tiles in `ws`
};

// Host side of the counter-based dropout (common.h, dropout_keep): (p, seed) -> the four scalars every dropout kernel takes.
// ok is false for a p outside [0, 1), NaN included (the entry points answer VITAMD_ERR_ARG); thresh = p * 2^32, 0 only for p == 0 (off).
struct DropoutParams {
  unsigned thresh;
  float scale;               // 1 / (1 - p)
  unsigned seed_lo, seed_hi;
  bool ok;
};
inline DropoutParams dropout_params(float p, unsigned long long seed) {
  DropoutParams d{0u, 1.0f, (unsigned)seed, (unsigned)(seed >> 32), p >= 0.f && p < 1.f};
  if (!d.ok) return d;
  d.thresh = p > 0.f ? (unsigned)((double)p * 4294967296.0) : 0u;
  if (p > 0.f && d.thresh == 0u) d.thresh = 1u;
  d.scale = 1.0f / (1.0f - p);
  return d;
}

int vitamd_gemm_nt_impl(const GemmNtArgs& p, hipStream_t stream);
int vitamd_gemm_nt_plan_impl(const GemmNtArgs& p);
int vitamd_gemm_nt_ws_impl(const GemmNtArgs& p, int splits, float* ws, size_t ws_bytes, hipStream_t stream);   // split-K where the rule says so
long vitamd_gemm_nt_ws_bytes_impl(const GemmNtArgs& p, int splits);
int vitamd_gemm_nt_ws_plan_impl(const GemmNtArgs& p, int splits);
int vitamd_init_impl(int device, hipStream_t stream);
const unsigned* vitamd_gelu_table();   // the current device's erf-GELU table image (vitamd_init), or null: shared by every GELU epilogue
int vitamd_gemm_tn_impl(const GemmTnArgs& p, hipStream_t stream);
