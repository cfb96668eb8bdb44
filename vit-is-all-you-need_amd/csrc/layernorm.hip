// Non-affine LayerNorm (eps 1e-5, biased variance) forward / backward on the fp32 residual stream,
// reference transformer.py:43-44 `F.layer_norm(x, (n_embd,))`, fused with the residual adds either
// side of it (transformer.py:43-44 `x = x + f(LN(x))`).  HBM-bound: one wave per row, 16-B loads,
// the row lives in registers between the statistics and the normalisation (one read of x).
//   forward : x = x_in (+ addend_bf16)   -> x_out fp32 (optional), y = bf16(LN(x)), mean, rstd
//   backward: g = g_res + LNbwd(dy_bf16; x, mean, rstd) -> g_out fp32, optional bf16(g) copy and
//             per-column sums of that bf16 copy (the bias gradient of the Linear whose output
//             gradient it is).
#include "common.h"
#include "vitamd_internal.h"
#include <type_traits>

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // 4 waves, one row each per iteration
constexpr int MAXV = 4;            // up to 4 float4 per lane: D <= 1024, D % 256 == 0

// KEEP (kept-row form, M = B * keep): output row b*keep + t takes row b*seq + t of x_in and row b*keep + t of the addend (the compact
// output of the kept-query attention); x_out, y, mean, rstd are compact.  The per-row arithmetic is the same code.
// ADD2: a second bf16 addend, added AFTER the first: s = fl(x + addend), then s = fl(s + addend2) - the bits a launch with `addend` that
// stored s followed by a launch on that s with `addend2` gives, without the 4 + 4 B per element of the store and the read back.  With
// KEEP the first addend is then a full-size tensor like x_in (row b*seq + t) and addend2 the compact one.  NOSTORE: x_out is not written.
template <int NV, bool HAS_ADD, bool KEEP = false, bool ADD2 = false, bool NOSTORE = false>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x_in, const __bf16* __restrict__ addend,
                                                     float* __restrict__ x_out, __bf16* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int M, float eps,
                                                     int seq = 0, int keep = 0, const __bf16* __restrict__ addend2 = nullptr) {
  static_assert(HAS_ADD || (!ADD2 && !NOSTORE), "the second addend and the store-free form go with a first addend");
  constexpr int D = NV * 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = blockIdx.x * ROWS_PER_BLOCK + wave; row < M; row += gridDim.x * ROWS_PER_BLOCK) {
    f32x4 v[NV];
    const size_t base = (size_t)row * D;
    size_t base_in = base;
    if constexpr (KEEP) base_in = ((size_t)(row / keep) * seq + row % keep) * D;
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = *(const f32x4*)(x_in + base_in + j * 256 + lane * 4);
    if constexpr (HAS_ADD) {
      const size_t base_add = ADD2 ? base_in : base;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const u32x2 a = *(const u32x2*)(addend + base_add + j * 256 + lane * 4);
        v[j][0] += bf16lo(a[0]); v[j][1] += bf16hi(a[0]); v[j][2] += bf16lo(a[1]); v[j][3] += bf16hi(a[1]);
        if constexpr (ADD2) {
          const u32x2 a2 = *(const u32x2*)(addend2 + base + j * 256 + lane * 4);
          v[j][0] += bf16lo(a2[0]); v[j][1] += bf16hi(a2[0]); v[j][2] += bf16lo(a2[1]); v[j][3] += bf16hi(a2[1]);
        }
        if constexpr (!NOSTORE) *(f32x4*)(x_out + base + j * 256 + lane * 4) = v[j];
      }
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) s += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    const float mu = wave_sum(s) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) { const float d = v[j][c] - mu; q += d * d; }
    const float rs = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      u32x2 o = {pack_bf16x2((v[j][0] - mu) * rs, (v[j][1] - mu) * rs), pack_bf16x2((v[j][2] - mu) * rs, (v[j][3] - mu) * rs)};
      *(u32x2*)(y + base + j * 256 + lane * 4) = o;
    }
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
  }
}

// generic-width fallback (D % 4 == 0): three passes over the row through L1/L2
template <bool HAS_ADD, bool KEEP = false>
__global__ __launch_bounds__(256) void ln_fwd_generic(const float* __restrict__ x_in, const __bf16* __restrict__ addend,
                                                      float* __restrict__ x_out, __bf16* __restrict__ y,
                                                      float* __restrict__ mean, float* __restrict__ rstd, int M, int D, float eps,
                                                      int seq = 0, int keep = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = blockIdx.x * ROWS_PER_BLOCK + wave; row < M; row += gridDim.x * ROWS_PER_BLOCK) {
    const size_t base = (size_t)row * D;
    const float* xr = x_in + base;
    if constexpr (KEEP) xr = x_in + ((size_t)(row / keep) * seq + row % keep) * D;      // kept-row form: see ln_fwd_kernel
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
      float t = xr[c];
      if constexpr (HAS_ADD) { t += bf2f(addend[base + c]); x_out[base + c] = t; }
      s += t;
    }
    if constexpr (HAS_ADD) xr = x_out + base;
    const float mu = wave_sum(s) / D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) { const float d = xr[c] - mu; q += d * d; }
    const float rs = rsqrtf(wave_sum(q) / D + eps);
    for (int c = lane; c < D; c += 64) y[base + c] = f2bf((xr[c] - mu) * rs);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
  }
}

// The generic-width fallback of the ADD2 / NOSTORE forms of ln_fwd_kernel (an addend is always there; with KEEP it is full size and addend2
// compact).  Every pass forms the sum again - the same two roundings, so the same bits - instead of reading it back: there may be no x_out.
template <bool KEEP, bool ADD2, bool NOSTORE>
__global__ __launch_bounds__(256) void ln_fwd_generic_add2(const float* __restrict__ x_in, const __bf16* __restrict__ addend,
                                                           const __bf16* __restrict__ addend2, float* __restrict__ x_out,
                                                           __bf16* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
                                                           int M, int D, float eps, int seq, int keep) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = blockIdx.x * ROWS_PER_BLOCK + wave; row < M; row += gridDim.x * ROWS_PER_BLOCK) {
    const size_t base = (size_t)row * D;
    size_t base_in = base;
    if constexpr (KEEP) base_in = ((size_t)(row / keep) * seq + row % keep) * D;
    const float* xr = x_in + base_in;
    const __bf16* ar = addend + (ADD2 ? base_in : base);
    auto summed = [&](int c) {                  // (x + addend) + addend2, in this order
      float t = xr[c] + bf2f(ar[c]);
      if constexpr (ADD2) t += bf2f(addend2[base + c]);
      return t;
    };
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
      const float t = summed(c);
      if constexpr (!NOSTORE) x_out[base + c] = t;
      s += t;
    }
    const float mu = wave_sum(s) / D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) { const float d = summed(c) - mu; q += d * d; }
    const float rs = rsqrtf(wave_sum(q) / D + eps);
    for (int c = lane; c < D; c += 64) y[base + c] = f2bf((summed(c) - mu) * rs);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
  }
}

// XH: xhat is read back from the forward's bf16 output y (= LN(x) exactly for this non-affine LayerNorm, saved anyway as the
// weight-gradient operand of the following Linear) through the `x` pointer, instead of being recomputed from the fp32 input:
// 2 B instead of 4 B per element of an HBM-bound kernel (16 -> 14 B/elem), `mean` unused.  The bf16 rounding of xhat only
// touches the xhat * mean(dy * xhat) term (|.| ~ 0.1 |dy|): ~2e-4 relative on g, far below the bf16 roundings around it.
// GK: g_res is COMPACT [B*keep, D] - the gradient of a stack output of which only the first `keep` tokens of every `seq` were kept: row
// b*seq + t adds g_res[b*keep + t] when t < keep and nothing otherwise (no read at all for the other rows).
template <int NV, bool XH = false, bool GK = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const __bf16* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ g_res, float* __restrict__ g_out,
                                                     __bf16* __restrict__ g_bf16, float* __restrict__ colsum, int M,
                                                     unsigned dthresh, float dscale, unsigned dseed_lo, unsigned dseed_hi,
                                                     int seq = 0, int keep = 0) {
  constexpr int D = NV * 256;
  __shared__ float red[ROWS_PER_BLOCK][D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 cs[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) cs[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int row = blockIdx.x * ROWS_PER_BLOCK + wave; row < M; row += gridDim.x * ROWS_PER_BLOCK) {
    const size_t base = (size_t)row * D;
    const float mu = XH ? 0.f : mean[row], rs = rstd[row];
    const float* gres_row = nullptr;            // GK: this row's compact g_res row, if it has one
    if constexpr (GK) {
      const int t = row % seq;
      if (t < keep) gres_row = g_res + ((size_t)(row / seq) * keep + t) * D;
    }
    f32x4 d[NV], xh[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const u32x2 a = *(const u32x2*)(dy + base + j * 256 + lane * 4);
      d[j] = (f32x4){bf16lo(a[0]), bf16hi(a[0]), bf16lo(a[1]), bf16hi(a[1])};
      if constexpr (XH) {
        const u32x2 yb = *(const u32x2*)((const __bf16*)x + base + j * 256 + lane * 4);
        xh[j] = (f32x4){bf16lo(yb[0]), bf16hi(yb[0]), bf16lo(yb[1]), bf16hi(yb[1])};
      } else {
        const f32x4 xv = *(const f32x4*)(x + base + j * 256 + lane * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) xh[j][c] = (xv[c] - mu) * rs;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s1 += d[j][c];
        s2 += d[j][c] * xh[j][c];
      }
    }
    const float m1 = wave_sum(s1) * (1.0f / D), m2 = wave_sum(s2) * (1.0f / D);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      f32x4 g;
#pragma unroll
      for (int c = 0; c < 4; ++c) g[c] = rs * (d[j][c] - m1 - xh[j][c] * m2);
      if constexpr (GK) {
        if (gres_row) g += *(const f32x4*)(gres_row + j * 256 + lane * 4);
      } else {
        if (g_res) g += *(const f32x4*)(g_res + base + j * 256 + lane * 4);
      }
      *(f32x4*)(g_out + base + j * 256 + lane * 4) = g;
      if (g_bf16) {
        u32x2 o = {pack_bf16x2(g[0], g[1]), pack_bf16x2(g[2], g[3])};
        if (dthresh) {   // the bf16 copy is the gradient of a dropped-out Linear output: same mask as the forward
          const unsigned long long e0 = (unsigned long long)base + j * 256 + lane * 4;
          o[0] = pack_bf16x2(bf16lo(o[0]) * dropout_keep(e0, dseed_lo, dseed_hi, dthresh, dscale),
                             bf16hi(o[0]) * dropout_keep(e0 + 1, dseed_lo, dseed_hi, dthresh, dscale));
          o[1] = pack_bf16x2(bf16lo(o[1]) * dropout_keep(e0 + 2, dseed_lo, dseed_hi, dthresh, dscale),
                             bf16hi(o[1]) * dropout_keep(e0 + 3, dseed_lo, dseed_hi, dthresh, dscale));
        }
        *(u32x2*)(g_bf16 + base + j * 256 + lane * 4) = o;
        if (colsum) {
          cs[j][0] += bf16lo(o[0]); cs[j][1] += bf16hi(o[0]); cs[j][2] += bf16lo(o[1]); cs[j][3] += bf16hi(o[1]);
        }
      }
    }
  }
  if (colsum && g_bf16) {
#pragma unroll
    for (int j = 0; j < NV; ++j) *(f32x4*)(&red[wave][j * 256 + lane * 4]) = cs[j];
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 256) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < ROWS_PER_BLOCK; ++w) s += red[w][c];
      atomicAdd(colsum + c, s);  // 256 contiguous bytes per wave-instruction
    }
  }
}

template <bool GK = false>       // GK: compact g_res, see ln_bwd_kernel
__global__ __launch_bounds__(256) void ln_bwd_generic(const __bf16* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      const float* __restrict__ g_res, float* __restrict__ g_out,
                                                      __bf16* __restrict__ g_bf16, float* __restrict__ colsum, int M, int D,
                                                      unsigned dthresh, float dscale, unsigned dseed_lo, unsigned dseed_hi,
                                                      int seq = 0, int keep = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = blockIdx.x * ROWS_PER_BLOCK + wave; row < M; row += gridDim.x * ROWS_PER_BLOCK) {
    const size_t base = (size_t)row * D;
    const float mu = mean[row], rs = rstd[row];
    const float* gr = nullptr;                  // GK: this row's compact g_res row, if it has one
    if constexpr (GK) {
      if (row % seq < keep) gr = g_res + ((size_t)(row / seq) * keep + row % seq) * D;
    }
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < D; c += 64) {
      const float d = bf2f(dy[base + c]);
      s1 += d;
      s2 += d * (x[base + c] - mu) * rs;
    }
    const float m1 = wave_sum(s1) / D, m2 = wave_sum(s2) / D;
    for (int c = lane; c < D; c += 64) {
      const float d = bf2f(dy[base + c]);
      float g = rs * (d - m1 - (x[base + c] - mu) * rs * m2);
      if constexpr (GK) {
        if (gr) g += gr[c];
      } else {
        if (g_res) g += g_res[base + c];
      }
      g_out[base + c] = g;
      if (g_bf16) {
        __bf16 gb = f2bf(g);
        if (dthresh) gb = f2bf(bf2f(gb) * dropout_keep((unsigned long long)base + c, dseed_lo, dseed_hi, dthresh, dscale));
        g_bf16[base + c] = gb;
        if (colsum) atomicAdd(colsum + c, bf2f(gb));
      }
    }
  }
}

// One row per wave where nothing is shared between rows (12 608 workgroups at M = 50 432: 4-7 % faster than a 2 048-workgroup grid-stride
// launch, tools/bench_ln.py); the column-sum form keeps a grid-stride loop - every workgroup ends with D atomics (12 608 of them: 312 us).
int grid_for(int M, bool colsum = false) {
  int blocks = (M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  int cap = !colsum ? 16384 : 1024;                 // column-sum form: 2048 -> 118 us, 1024 -> 111, 512 -> 110, 4096 -> 135
  return blocks < cap ? blocks : cap;
}

// The width as a template argument: f is a generic lambda that gets std::integral_constant<int, NV> for D = 256 NV, NV = 1 .. 4 (the
// register-resident kernels), and <int, 0> for every other D (the generic kernels).
bool register_width(int D) { return D == 256 || D == 512 || D == 768 || D == 1024; }
template <typename F>
void with_width(int D, F f) {
  if (D == 256) f(std::integral_constant<int, 1>{});
  else if (D == 512) f(std::integral_constant<int, 2>{});
  else if (D == 768) f(std::integral_constant<int, 3>{});
  else if (D == 1024) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 0>{});
}

// Every forward launch.  KEEP: the kept-row form (M = B * keep; the addend is required there, so only HAS_ADD = true exists).
// add2 / x_out == nullptr with an addend: the forms with a second addend / without the stream store (ln_fwd_kernel); the entry points
// decide which combinations they let through.
template <bool KEEP>
int ln_fwd_launch(const float* x_in, const void* addend_bf16, const void* addend2_bf16, float* x_out, void* y_bf16, float* mean, float* rstd, int M,
                  int D, float eps, int seq, int keep, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const __bf16* add = (const __bf16*)addend_bf16;
  const __bf16* add2 = (const __bf16*)addend2_bf16;
  __bf16* y = (__bf16*)y_bf16;
  const dim3 grid(grid_for(M)), block(256);
  with_width(D, [&](auto W) {
    constexpr int NV = decltype(W)::value;
    auto go = [&](auto ADD, auto SECOND, auto DROP_STORE) {
      constexpr bool HAS_ADD = decltype(ADD)::value, ADD2 = decltype(SECOND)::value, NOSTORE = decltype(DROP_STORE)::value;
      if constexpr (NV != 0) hipLaunchKernelGGL((ln_fwd_kernel<NV, HAS_ADD, KEEP, ADD2, NOSTORE>), grid, block, 0, stream, x_in, add, x_out, y, mean, rstd, M, eps, seq, keep, add2);
      else if constexpr (ADD2 || NOSTORE) hipLaunchKernelGGL((ln_fwd_generic_add2<KEEP, ADD2, NOSTORE>), grid, block, 0, stream, x_in, add, add2, x_out, y, mean, rstd, M, D, eps, seq, keep);
      else hipLaunchKernelGGL((ln_fwd_generic<HAS_ADD, KEEP>), grid, block, 0, stream, x_in, add, x_out, y, mean, rstd, M, D, eps, seq, keep);
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (add2 && !x_out) go(yes, yes, yes);
    else if (add2) go(yes, yes, no);
    else if constexpr (KEEP) go(yes, no, no);   // (the kept-row form without a second addend always has its addend and always stores)
    else if (!add) go(no, no, no);
    else if (!x_out) go(yes, no, yes);
    else go(yes, no, no);
  });
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

// Every backward launch.  GK: compact g_res (M = B * seq).  xhat: x_or_y is the forward's bf16 output (XH = true; the callers have refused
// the widths without a register-resident kernel) and mean is not read.
template <bool GK>
int ln_bwd_launch(const void* dy_bf16, const void* x_or_y, const float* mean, const float* rstd, const float* g_res, float* g_out, void* g_bf16,
                  float* colsum, int M, int D, bool xhat, const DropoutParams& dp, int seq, int keep, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const __bf16* dy = (const __bf16*)dy_bf16;
  const float* x = (const float*)x_or_y;          // XH: the kernel reinterprets it
  __bf16* gb = (__bf16*)g_bf16;
  const dim3 grid(grid_for(M, colsum != nullptr && g_bf16 != nullptr)), block(256);
  with_width(D, [&](auto W) {
    constexpr int NV = decltype(W)::value;
    if constexpr (NV != 0) {
      if (xhat) hipLaunchKernelGGL((ln_bwd_kernel<NV, true, GK>), grid, block, 0, stream, dy, x, mean, rstd, g_res, g_out, gb, colsum, M, dp.thresh, dp.scale, dp.seed_lo, dp.seed_hi, seq, keep);
      else hipLaunchKernelGGL((ln_bwd_kernel<NV, false, GK>), grid, block, 0, stream, dy, x, mean, rstd, g_res, g_out, gb, colsum, M, dp.thresh, dp.scale, dp.seed_lo, dp.seed_hi, seq, keep);
    } else {
      hipLaunchKernelGGL(ln_bwd_generic<GK>, grid, block, 0, stream, dy, x, mean, rstd, g_res, g_out, gb, colsum, M, D, dp.thresh, dp.scale, dp.seed_lo, dp.seed_hi, seq, keep);
    }
  });
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

}  // namespace

// The entry points keep their own checks, in this order: shape -> VITAMD_ERR_SHAPE, then null pointers, then the dropout probability -> VITAMD_ERR_ARG.
extern "C" int vitamd_layernorm_fwd(const float* x_in, const void* addend_bf16, float* x_out, void* y_bf16, float* mean,
                                    float* rstd, int M, int D, float eps, void* stream) {
  if (M <= 0 || D <= 0 || D % 4) return VITAMD_ERR_SHAPE;
  if (!x_in || !y_bf16 || !mean || !rstd || (addend_bf16 && !x_out)) return VITAMD_ERR_ARG;
  return ln_fwd_launch<false>(x_in, addend_bf16, nullptr, x_out, y_bf16, mean, rstd, M, D, eps, 0, 0, stream);
}

// the bf16 copy (and its column sums) additionally gets the dropout mask (p, seed) of the
// Linear output whose gradient it is (index = row * D + column, as in vitamd_linear_dropout_resid_bf16)
extern "C" int vitamd_layernorm_bwd_dropout(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                            const float* g_res, float* g_out, void* g_bf16, float* colsum, int M, int D,
                                            float dropout_p, unsigned long long seed, void* stream) {
  if (M <= 0 || D <= 0 || D % 4) return VITAMD_ERR_SHAPE;
  if (!dy_bf16 || !x || !mean || !rstd || !g_out) return VITAMD_ERR_ARG;
  const DropoutParams dp = dropout_params(dropout_p, seed);
  if (!dp.ok) return VITAMD_ERR_ARG;
  return ln_bwd_launch<false>(dy_bf16, x, mean, rstd, g_res, g_out, g_bf16, colsum, M, D, false, dp, 0, 0, stream);
}

extern "C" int vitamd_layernorm_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                    const float* g_res, float* g_out, void* g_bf16, float* colsum, int M, int D,
                                    void* stream) {
  return vitamd_layernorm_bwd_dropout(dy_bf16, x, mean, rstd, g_res, g_out, g_bf16, colsum, M, D, 0.f, 0ull, stream);
}

// LayerNorm backward with xhat taken from the forward's bf16 output (see ln_bwd_kernel<NV, true>): D in {256, 512, 768, 1024}.
extern "C" int vitamd_layernorm_bwd_xhat(const void* dy_bf16, const void* y_bf16, const float* rstd, const float* g_res, float* g_out,
                                         void* g_bf16, float* colsum, int M, int D, float dropout_p, unsigned long long seed,
                                         void* stream) {
  if (M <= 0 || !register_width(D)) return VITAMD_ERR_SHAPE;
  if (!dy_bf16 || !y_bf16 || !rstd || !g_out) return VITAMD_ERR_ARG;
  const DropoutParams dp = dropout_params(dropout_p, seed);
  if (!dp.ok) return VITAMD_ERR_ARG;
  return ln_bwd_launch<false>(dy_bf16, y_bf16, nullptr, rstd, g_res, g_out, g_bf16, colsum, M, D, true, dp, 0, 0, stream);
}

// Kept-row forward: M = B * keep output rows; row b*keep + t = LN(x_in[b*seq + t] + addend[b*keep + t]).  x_out, y, mean, rstd are compact
// [B*keep, ...].  addend (bf16 [B*keep, D], the kept-query attention output) and x_out are required.
extern "C" int vitamd_layernorm_fwd_keep(const float* x_in, const void* addend_bf16, float* x_out, void* y_bf16, float* mean, float* rstd,
                                         int B, int seq, int keep, int D, float eps, void* stream) {
  if (B <= 0 || seq <= 0 || keep <= 0 || keep > seq || D <= 0 || D % 4) return VITAMD_ERR_SHAPE;
  if ((long long)B * seq > 2147483647LL) return VITAMD_ERR_SHAPE;
  if (!x_in || !y_bf16 || !mean || !rstd || !addend_bf16 || !x_out) return VITAMD_ERR_ARG;
  return ln_fwd_launch<true>(x_in, addend_bf16, nullptr, x_out, y_bf16, mean, rstd, B * keep, D, eps, seq, keep, stream);
}

// LayerNorm backward over M = B * seq rows with a COMPACT g_res [B*keep, D]: row b*seq + t adds g_res[b*keep + t] when t < keep, nothing
// otherwise.  use_xhat != 0: x_or_y is the forward's bf16 output (vitamd_layernorm_bwd_xhat; D in {256, 512, 768, 1024}, mean unused);
// else the fp32 input with mean / rstd (vitamd_layernorm_bwd_dropout).  g_bf16, colsum and the dropout arguments as there.
extern "C" int vitamd_layernorm_bwd_keep(const void* dy_bf16, const void* x_or_y, const float* mean, const float* rstd, const float* g_res,
                                         float* g_out, void* g_bf16, float* colsum, int B, int seq, int keep, int D, int use_xhat,
                                         float dropout_p, unsigned long long seed, void* stream) {
  if (B <= 0 || seq <= 0 || keep <= 0 || keep > seq || D <= 0 || D % 4) return VITAMD_ERR_SHAPE;
  if ((long long)B * seq > 2147483647LL) return VITAMD_ERR_SHAPE;
  if (use_xhat && !register_width(D)) return VITAMD_ERR_SHAPE;
  if (!dy_bf16 || !x_or_y || !rstd || !g_res || !g_out || (!use_xhat && !mean)) return VITAMD_ERR_ARG;
  const DropoutParams dp = dropout_params(dropout_p, seed);
  if (!dp.ok) return VITAMD_ERR_ARG;
  return ln_bwd_launch<true>(dy_bf16, x_or_y, mean, rstd, g_res, g_out, g_bf16, colsum, B * seq, D, use_xhat != 0, dp, seq, keep, stream);
}

// Forward with up to two bf16 addends and an optional stream store: s = fl(x_in + addend1), then s = fl(s + addend2) when addend2 is given;
// y, mean, rstd = LN(s); x_out = s when x_out is given.  The bits of vitamd_layernorm_fwd(x_in, addend1) followed by
// vitamd_layernorm_fwd(its x_out, addend2), in one pass over x_in.  addend1 is required.
extern "C" int vitamd_layernorm_fwd_add2(const float* x_in, const void* addend1_bf16, const void* addend2_bf16, float* x_out, void* y_bf16,
                                         float* mean, float* rstd, int M, int D, float eps, void* stream) {
  if (M <= 0 || D <= 0 || D % 4) return VITAMD_ERR_SHAPE;
  if (!x_in || !addend1_bf16 || !y_bf16 || !mean || !rstd) return VITAMD_ERR_ARG;
  return ln_fwd_launch<false>(x_in, addend1_bf16, addend2_bf16, x_out, y_bf16, mean, rstd, M, D, eps, 0, 0, stream);
}

// Its kept-row form: output row b*keep + t = LN(fl(fl(x_in[b*seq + t] + addend1[b*seq + t]) + addend2[b*keep + t])).  x_in and addend1 are
// full size [B*seq, D]; addend2 (required), x_out (optional), y, mean and rstd are compact [B*keep, ...].
extern "C" int vitamd_layernorm_fwd_keep_add2(const float* x_in, const void* addend1_bf16, const void* addend2_bf16, float* x_out, void* y_bf16,
                                              float* mean, float* rstd, int B, int seq, int keep, int D, float eps, void* stream) {
  if (B <= 0 || seq <= 0 || keep <= 0 || keep > seq || D <= 0 || D % 4) return VITAMD_ERR_SHAPE;
  if ((long long)B * seq > 2147483647LL) return VITAMD_ERR_SHAPE;
  if (!x_in || !addend1_bf16 || !addend2_bf16 || !y_bf16 || !mean || !rstd) return VITAMD_ERR_ARG;
  return ln_fwd_launch<true>(x_in, addend1_bf16, addend2_bf16, x_out, y_bf16, mean, rstd, B * keep, D, eps, seq, keep, stream);
}
