// Tokenizer evaluation: per-image MSE / MAE / PSNR / SSIM of a reconstruction against its target, and the
// code-usage histogram of the quantiser's ids, both added to accumulators that stay on the device.  The contract is in include/vitamd_eval.h
// (vitamd_recon_metrics, vitamd_code_hist); this comment says how the kernels keep it.
//
// recon_tiles_kernel.  One workgroup of 256 threads per TILE x TILE (32 x 32) tile of one channel of one image, looping over further
// tiles beyond the grid cap.  A tile owns the pixels (y, x) and the SSIM windows with top-left corner (y, x) in
// [ty*32, ty*32+32) x [tx*32, tx*32+32): every pixel and every window has exactly one owner.  With SSIM the tile stages its 42 x 42
// region (the tile plus the 10-pixel halo below and to the right, zeros past the image) of both images in LDS once, as x - R/2 and
// y - R/2: the variances are shift-invariant, and the raw second moments E[x^2] - mu^2 of the shifted values cancel against numbers
// of size (R/2)^2 at worst instead of R^2, typically far less.  The squared and absolute differences of the owned pixels are formed
// from the UNSHIFTED values while they are in registers on their way to LDS.  Then the separable 11-tap pass: horizontally over the
// five planes x, y, x^2, y^2, xy (42 rows x 32 columns, into LDS), vertically (32 x 32, in registers), 11 fused multiply-adds each in
// tap order, and the SSIM map with every product and sum spelled out (__fmul_rn / __fadd_rn / fmaf: no contraction the compiler may
// choose differently for numerator and denominator), so identical images give a map of exactly 1.
// Sums: every thread adds its own terms in a fixed order (at most 8 owned pixels per thread on any load path, 4 windows), lanes by
// __shfl_xor (6 levels), the four waves through LDS in wave order: an fp32 summation of depth d = 8 + 6 + 4 = 18 at most
// (RECON_SUM_DEPTH; tests/_recon_ref.py uses the same number).  Three fp32 partials per tile go to the workspace with plain stores.
// Without SSIM the region is the 32 x 32 tile alone and both moment passes are skipped.
// Rows are loaded in 16-byte pieces (4 fp32 / 8 bf16) when both bases are 16-byte aligned and W is a multiple of the piece of both
// dtypes in use; element by element otherwise.
//
// recon_sum_kernel.  One workgroup, a fixed order: wave w takes images w, w + 16, ...; its lanes sum that image's partials in fp64
// (lane l: tiles l, l + 64, ... in ascending order, then the xor butterfly), lane 0 forms the four values in fp64 and writes them to
// per_image.  After a barrier the batch sums are formed the same way over the images and thread 0 ADDS them to the accumulators.
//
// code_hist_kernel.  Integer atomics only.  LDS form (K <= CODE_HIST_LDS_MAX_K): each workgroup counts chunks of 4 096 ids into an
// int32 histogram in LDS (M < 2^31, so a bin cannot overflow) and flushes its non-zero bins with one 64-bit global atomic each.
// Global form: one 64-bit global atomic per id.  An id outside [0, K) forms no address; each wave adds its count of them to bad[0].
#include "common.h"
#include "../../include/vitamd_eval.h"   // the entry points and limits of this file

namespace {

constexpr int TILE = 32;                  // owned pixels / window corners per tile side
constexpr int HALO = 10;                  // an 11 x 11 window reaches 10 pixels past its corner
constexpr int REG = TILE + HALO;          // 42: staged rows and columns with SSIM
constexpr int SW = 48;                    // LDS row stride in floats: six 8-element bf16 pieces, twelve 4-element fp32 pieces
constexpr int RECON_THREADS = 256;
constexpr int RECON_GRID_CAP = 2048;      // 8 workgroups per CU of the MI355X's 256
constexpr int RECON_SUM_DEPTH = 18;       // see above
constexpr int HIST_THREADS = 1024;
constexpr int HIST_CHUNK = 4096;          // ids one workgroup counts per sweep
constexpr int HIST_GRID_CAP = 256;
constexpr int CODE_HIST_LDS_MAX_K = 32768;   // 128 KiB of the CU's 160 KiB of LDS

// the 11 taps of the Gaussian (sigma 1.5), normalised to sum 1 in fp64, rounded to fp32 once
__constant__ float GAUSS[11] = {0.0010283801f, 0.007598758f, 0.036000773f, 0.10936069f, 0.21300554f, 0.26601171f,
                                0.21300554f,   0.10936069f,   0.036000773f, 0.007598758f, 0.0010283801f};

struct ReconArgs {
  const void* recon;
  const float* target;
  float* ws;
  int C, H, W, tiles_y, tiles_x;
  long long tiles;
  float range, half, c1, c2;
  int clamp;
};

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the clamp spelled out: a NaN fails both comparisons and stays
__device__ __forceinline__ float clamp_keep_nan(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

// sum over the workgroup in a fixed order, returned to thread 0: lanes by xor butterfly, waves through LDS in wave order
__device__ __forceinline__ float block_sum_ordered(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                       // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

template <bool BF16, bool VEC, bool SSIM>
__global__ __launch_bounds__(RECON_THREADS) void recon_tiles_kernel(const ReconArgs a) {
  constexpr int ROWS = SSIM ? REG : TILE;                // staged rows; columns likewise
  constexpr int PIECE = VEC ? (BF16 ? 8 : 4) : 1;
  constexpr int PIECES = (ROWS + PIECE - 1) / PIECE;     // per staged row: 42 -> 11 (fp32) / 6 (bf16) / 42; 32 -> 8 / 4 / 32
  __shared__ float sx[SSIM ? REG * SW : 1], sy[SSIM ? REG * SW : 1];
  __shared__ float hx[SSIM ? 5 * REG * TILE : 1];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int plane_tiles = a.tiles_y * a.tiles_x;
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long long plane = tile / plane_tiles;          // b * C + c
    const int in_plane = (int)(tile - plane * plane_tiles);
    const int y0 = (in_plane / a.tiles_x) * TILE, x0 = (in_plane % a.tiles_x) * TILE;
    const size_t base = (size_t)plane * (size_t)a.H * (size_t)a.W;
    float sse = 0.f, sae = 0.f;
    for (int i = tid; i < ROWS * PIECES; i += RECON_THREADS) {
      const int r = i / PIECES, c = (i - r * PIECES) * PIECE;
      const int y = y0 + r, x = x0 + c;
      float rv[PIECE], tv[PIECE];
      bool in[PIECE];
      if constexpr (VEC) {
        // W is a multiple of PIECE and x0, c are too: a piece lies wholly inside the row or wholly outside
        const bool inside = y < a.H && x < a.W;
#pragma unroll
        for (int j = 0; j < PIECE; ++j) { in[j] = inside; rv[j] = 0.f; tv[j] = 0.f; }
        if (inside) {
          const size_t off = base + (size_t)y * a.W + x;
          if constexpr (BF16) {
            const u32x4 q = *(const u32x4*)((const __bf16*)a.recon + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) { rv[2 * j] = bf16lo(q[j]); rv[2 * j + 1] = bf16hi(q[j]); }
            const f32x4 t0 = *(const f32x4*)(a.target + off), t1 = *(const f32x4*)(a.target + off + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { tv[j] = t0[j]; tv[4 + j] = t1[j]; }
          } else {
            const f32x4 q = *(const f32x4*)((const float*)a.recon + off), t0 = *(const f32x4*)(a.target + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) { rv[j] = q[j]; tv[j] = t0[j]; }
          }
        }
      } else {
        in[0] = y < a.H && x < a.W;
        rv[0] = tv[0] = 0.f;
        if (in[0]) {
          const size_t off = base + (size_t)y * a.W + x;
          rv[0] = BF16 ? bf2f(((const __bf16*)a.recon)[off]) : ((const float*)a.recon)[off];
          tv[0] = a.target[off];
        }
      }
#pragma unroll
      for (int j = 0; j < PIECE; ++j) {
        if (a.clamp) rv[j] = clamp_keep_nan(rv[j], a.range);
        if (in[j] && r < TILE && c + j < TILE) {         // an owned pixel: the differences of the values as they are
          const float d = __fsub_rn(rv[j], tv[j]);
          sse = fmaf(d, d, sse);
          sae = __fadd_rn(sae, fabsf(d));
        }
        if constexpr (SSIM) {
          if (c + j < SW) {                              // (always: PIECES * PIECE <= SW)
            sx[r * SW + c + j] = in[j] ? __fsub_rn(rv[j], a.half) : 0.f;
            sy[r * SW + c + j] = in[j] ? __fsub_rn(tv[j], a.half) : 0.f;
          }
        }
      }
    }
    float smap = 0.f;
    if constexpr (SSIM) {
      __syncthreads();
      // horizontal pass: rows 0 .. 41, columns 0 .. 31 (columns c .. c + 10 <= 41 of the staged region)
      for (int i = tid; i < REG * TILE; i += RECON_THREADS) {
        const int r = i >> 5, c = i & 31;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const float w = GAUSS[k], xv = sx[r * SW + c + k], yv = sy[r * SW + c + k];
          m0 = fmaf(w, xv, m0);
          m1 = fmaf(w, yv, m1);
          m2 = fmaf(w, __fmul_rn(xv, xv), m2);
          m3 = fmaf(w, __fmul_rn(yv, yv), m3);
          m4 = fmaf(w, __fmul_rn(xv, yv), m4);
        }
        hx[0 * REG * TILE + i] = m0;
        hx[1 * REG * TILE + i] = m1;
        hx[2 * REG * TILE + i] = m2;
        hx[3 * REG * TILE + i] = m3;
        hx[4 * REG * TILE + i] = m4;
      }
      __syncthreads();
      // vertical pass and the map: window corners (y0 + r, x0 + c), those with the whole window inside the image
      for (int i = tid; i < TILE * TILE; i += RECON_THREADS) {
        const int r = i >> 5, c = i & 31;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const float w = GAUSS[k];
          const int at = (r + k) * TILE + c;
          m0 = fmaf(w, hx[0 * REG * TILE + at], m0);
          m1 = fmaf(w, hx[1 * REG * TILE + at], m1);
          m2 = fmaf(w, hx[2 * REG * TILE + at], m2);
          m3 = fmaf(w, hx[3 * REG * TILE + at], m3);
          m4 = fmaf(w, hx[4 * REG * TILE + at], m4);
        }
        const float vx = fmaf(-m0, m0, m2), vy = fmaf(-m1, m1, m3), vxy = fmaf(-m0, m1, m4);   // biased moments of the shifted values
        const float mx = __fadd_rn(m0, a.half), my = __fadd_rn(m1, a.half);                       // the means, shift added back
        const float num = __fmul_rn(__fadd_rn(__fmul_rn(2.f, __fmul_rn(mx, my)), a.c1), __fadd_rn(__fmul_rn(2.f, vxy), a.c2));
        const float den = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my)), a.c1), __fadd_rn(__fadd_rn(vx, vy), a.c2));
        if (y0 + r + HALO < a.H && x0 + c + HALO < a.W) smap = __fadd_rn(smap, __fdiv_rn(num, den));
      }
    }
    const float t0 = block_sum_ordered(sse, red), t1 = block_sum_ordered(sae, red), t2 = block_sum_ordered(smap, red);
    if (tid == 0) {
      a.ws[tile * 3 + 0] = t0;
      a.ws[tile * 3 + 1] = t1;
      a.ws[tile * 3 + 2] = t2;
    }
    __syncthreads();                                      // LDS is restaged by the next tile
  }
}

// sum of v over the 1024 threads in a fixed order, valid in thread 0
__device__ __forceinline__ double block_sum_1024(double v, double* part) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < 16; ++i) s += part[i];
  return s;
}

__global__ __launch_bounds__(1024) void recon_sum_kernel(const float* __restrict__ ws, double* per_image, double* __restrict__ sums,
                                                       long long* __restrict__ count, int B, long long image_tiles, double pixels,
                                                       double windows, double range, int ssim) {
  __shared__ double part[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += 16) {
    const float* p = ws + (size_t)b * (size_t)image_tiles * 3;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long long t = lane; t < image_tiles; t += 64) {
      s0 += (double)p[t * 3 + 0];
      s1 += (double)p[t * 3 + 1];
      s2 += (double)p[t * 3 + 2];
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
    if (lane == 0) {
      const double mse = s0 / pixels, mae = s1 / pixels;
      per_image[(size_t)b * 4 + 0] = mse;
      per_image[(size_t)b * 4 + 1] = mae;
      per_image[(size_t)b * 4 + 2] = 10.0 * log10(range * range / mse);         // mse == 0: +inf; NaN stays NaN
      per_image[(size_t)b * 4 + 3] = ssim ? s2 / windows : __builtin_nan("");
    }
  }
  __threadfence_block();
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += 1024)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += per_image[(size_t)b * 4 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = block_sum_1024(acc[k], part);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) sums[k] += acc[k];
  count[0] += B;
}

template <bool LDS>
__global__ __launch_bounds__(HIST_THREADS) void code_hist_kernel(const long long* __restrict__ ids, long long M, int K,
                                                                unsigned long long* __restrict__ hist, unsigned long long* __restrict__ bad) {
  extern __shared__ int bins[];
  if constexpr (LDS) {
    for (int k = threadIdx.x; k < K; k += HIST_THREADS) bins[k] = 0;
    __syncthreads();
  }
  int nbad = 0;
  for (long long c0 = (long long)blockIdx.x * HIST_CHUNK; c0 < M; c0 += (long long)gridDim.x * HIST_CHUNK) {
#pragma unroll
    for (int j = 0; j < HIST_CHUNK / HIST_THREADS; ++j) {
      const long long i = c0 + j * HIST_THREADS + threadIdx.x;
      if (i >= M) continue;
      const long long id = ids[i];
      if (id < 0 || id >= (long long)K) { nbad += 1; continue; }
      if constexpr (LDS) atomicAdd(&bins[(int)id], 1);
      else atomicAdd(&hist[id], 1ull);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, 64);
  if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
  if constexpr (LDS) {
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += HIST_THREADS) {
      const int n = bins[k];
      if (n) atomicAdd(&hist[k], (unsigned long long)n);
    }
  }
}

// tiles of one call, or -1 where the shape is refused
long long recon_tiles(long B, int C, int H, int W, int ssim) {
  const int lo = ssim ? HALO + 1 : 1;
  if (B < 1 || C < 1 || H < lo || W < lo || H > VITAMD_RECON_METRICS_MAX_DIM || W > VITAMD_RECON_METRICS_MAX_DIM) return -1;
  const long long per_plane = (long long)((H + TILE - 1) / TILE) * ((W + TILE - 1) / TILE);     // <= 2^20
  if (B > VITAMD_RECON_METRICS_MAX_TILES / per_plane || (long long)C > VITAMD_RECON_METRICS_MAX_TILES / (B * per_plane)) return -1;
  return (long long)B * C * per_plane;
}

}  // namespace

extern "C" int vitamd_recon_metrics_tile(void) { return TILE; }
extern "C" int vitamd_recon_metrics_grid_cap(void) { return RECON_GRID_CAP; }
extern "C" int vitamd_recon_metrics_sum_depth(void) { return RECON_SUM_DEPTH; }

extern "C" long vitamd_recon_metrics_ws_bytes(long B, int C, int H, int W, int ssim) {
  const long long tiles = recon_tiles(B, C, H, W, ssim);
  return tiles < 0 ? -(long)VITAMD_ERR_SHAPE : (long)(tiles * 3 * (long long)sizeof(float));
}

extern "C" int vitamd_recon_metrics(const void* recon, int recon_bf16, const float* target, double* per_image, double* sums, long long* count,
                                    void* ws, long ws_bytes, long B, int C, int H, int W, double data_range, int clamp, int ssim,
                                    void* stream) {
  const long long tiles = recon_tiles(B, C, H, W, ssim);
  if (tiles < 0 || ws_bytes < tiles * 3 * (long long)sizeof(float)) return VITAMD_ERR_SHAPE;
  if (!(data_range > 0.0) || !(data_range <= 3.0e38) || !recon || !target || !per_image || !sums || !count || !ws) return VITAMD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  ReconArgs a;
  a.recon = recon; a.target = target; a.ws = (float*)ws;
  a.C = C; a.H = H; a.W = W;
  a.tiles_y = (H + TILE - 1) / TILE; a.tiles_x = (W + TILE - 1) / TILE;
  a.tiles = tiles;
  a.range = (float)data_range; a.half = (float)(0.5 * data_range);
  a.c1 = (float)((0.01 * data_range) * (0.01 * data_range)); a.c2 = (float)((0.03 * data_range) * (0.03 * data_range));
  a.clamp = clamp ? 1 : 0;
  const bool vec = aligned16(recon) && aligned16(target) && W % (recon_bf16 ? 8 : 4) == 0;
  const dim3 grid((unsigned)(tiles < RECON_GRID_CAP ? tiles : RECON_GRID_CAP)), block(RECON_THREADS);
#define RECON_LAUNCH(BF, VE, SS) hipLaunchKernelGGL((recon_tiles_kernel<BF, VE, SS>), grid, block, 0, s, a)
  if (ssim) {
    if (recon_bf16) { if (vec) RECON_LAUNCH(true, true, true); else RECON_LAUNCH(true, false, true); }
    else { if (vec) RECON_LAUNCH(false, true, true); else RECON_LAUNCH(false, false, true); }
  } else {
    if (recon_bf16) { if (vec) RECON_LAUNCH(true, true, false); else RECON_LAUNCH(true, false, false); }
    else { if (vec) RECON_LAUNCH(false, true, false); else RECON_LAUNCH(false, false, false); }
  }
#undef RECON_LAUNCH
  const long long image_tiles = tiles / B;
  const double windows = ssim ? (double)C * (double)(H - HALO) * (double)(W - HALO) : 0.0;
  hipLaunchKernelGGL(recon_sum_kernel, dim3(1), dim3(1024), 0, s, (const float*)ws, per_image, sums, count, (int)B, image_tiles,
                     (double)C * (double)H * (double)W, windows, data_range, ssim ? 1 : 0);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_code_hist_lds_max_k(void) { return CODE_HIST_LDS_MAX_K; }
extern "C" int vitamd_code_hist_grid_cap(void) { return HIST_GRID_CAP; }

extern "C" int vitamd_code_hist(const long long* ids, long M, int K, long long* hist, long long* bad, void* stream) {
  if (M < 1 || M > VITAMD_CODE_HIST_MAX_M || K < 2 || K > VITAMD_CODE_HIST_MAX_K) return VITAMD_ERR_SHAPE;
  if (!ids || !hist || !bad) return VITAMD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long chunks = (M + HIST_CHUNK - 1) / HIST_CHUNK;
  const dim3 grid((unsigned)(chunks < HIST_GRID_CAP ? chunks : HIST_GRID_CAP)), block(HIST_THREADS);
  if (K <= CODE_HIST_LDS_MAX_K) {
    if (int e = launch<code_hist_kernel<true>>(grid, block, K * (int)sizeof(int), s, ids, (long long)M, K, (unsigned long long*)hist,
                                               (unsigned long long*)bad))
      return e;
  } else {
    hipLaunchKernelGGL(code_hist_kernel<false>, grid, block, 0, s, ids, (long long)M, K, (unsigned long long*)hist, (unsigned long long*)bad);
  }
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
