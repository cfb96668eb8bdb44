// Fused AdamW step (decoupled weight decay), the optimiser of the reference's loops
// (train_vit.py:82,105 `torch.optim.AdamW` through GradScaler.step; bf16 needs no scaler).
// HBM-bound: 16 B read + 12 B written per parameter, one pass, 16-B accesses.
//
// Two forms share one element function.  The per-tensor form is one launch per parameter tensor.  The multi-tensor form (DESIGN.md
// section 12) walks a row table in device memory, one row per tensor, so that the whole optimiser step is one launch; with gradient-norm
// clipping two launches come first: per-chunk sums of squares, then one workgroup that adds them in a fixed order and derives the clip
// coefficient, which the update (or an in-place scale of the gradients) reads from device memory.  No float atomics anywhere: which
// workgroup handled a chunk has no influence on any value, so the norm and the coefficient are the same bits on every call and every rank.
#include "common.h"
#include "../../include/vitamd.h"

namespace {

// One element of the update.  decay = 1 - lr * wd and step = lr / bc1 are formed once per tensor by adamw_scalars.
// omb1 = fp32(1 - beta1), omb2 = fp32(1 - beta2), rounded once from the caller's doubles on the host: 1.0f - b would carry the rounding of b
// into a number ten to a thousand times smaller (beta2 = 0.999: exp_avg_sq 1.3e-5 off torch's)
// Which products are fused into the following addition decides the last bit, and left to the compiler it is decided per call site: so the
// function says it itself (contraction off, fmaf where a product is fused).  The forms are those adamw_kernel has always been compiled to;
// VEC, for the elements in 16-byte pieces, fuses b2 * v and decay * p, the scalar tail of a tensor (n % 4 elements) rounds them first.
// Every kernel that calls this gives the same bits for the same element, which is what lets the multi-tensor form stand in for the other.
template <bool VEC>
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float decay, float step, float b1, float omb1, float b2,
                                           float omb2, float eps, float inv_sqrt_bc2) {
#pragma clang fp contract(off)
  m = __builtin_fmaf(omb1, g, b1 * m);
  const float gg = g * (omb2 * g);
  v = VEC ? __builtin_fmaf(b2, v, gg) : gg + b2 * v;
  const float q = step * m / __builtin_fmaf(inv_sqrt_bc2, sqrtf(v), eps);
  p = VEC ? __builtin_fmaf(decay, p, -q) : decay * p - q;
}
__device__ __forceinline__ void adamw_scalars(float lr, float wd, float inv_bc1, float& decay, float& step) {
  decay = __builtin_fmaf(-lr, wd, 1.0f);   // 1 - lr * wd
  step = lr * inv_bc1;
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, size_t n4, size_t n, float lr, float b1, float omb1,
                                                    float b2, float omb2, float eps, float wd, float inv_bc1, float inv_sqrt_bc2) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  float decay, step;
  adamw_scalars(lr, wd, inv_bc1, decay, step);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 pv = *(const f32x4*)(p + 4 * i);
    const f32x4 gv = *(const f32x4*)(g + 4 * i);
    f32x4 mv = *(const f32x4*)(m + 4 * i), vv = *(const f32x4*)(v + 4 * i);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float pc = pv[c], mc = mv[c], vc = vv[c];
      adamw_elem<true>(pc, gv[c], mc, vc, decay, step, b1, omb1, b2, omb2, eps, inv_sqrt_bc2);
      pv[c] = pc; mv[c] = mc; vv[c] = vc;
    }
    *(f32x4*)(p + 4 * i) = pv;
    *(f32x4*)(m + 4 * i) = mv;
    *(f32x4*)(v + 4 * i) = vv;
  }
  if (blockIdx.x == 0) {
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      float pv = p[i], mv = m[i], vv = v[i];
      adamw_elem<false>(pv, g[i], mv, vv, decay, step, b1, omb1, b2, omb2, eps, inv_sqrt_bc2);
      p[i] = pv; m[i] = mv; v[i] = vv;
    }
  }
}

// ------------------------------------------------------------------------------------------------ multi-tensor form
// A tensor of n elements is cut into ceil(n / MT_CHUNK) chunks; chunk c of the table belongs to the row r with
// rows[r].first_chunk <= c < rows[r + 1].first_chunk and covers elements (c - first_chunk) * MT_CHUNK ... of it.  MT_CHUNK is a multiple
// of 4, so every chunk of a 16-byte aligned tensor starts on a 16-byte boundary, and only the last chunk of a tensor has a scalar tail.
// One workgroup per chunk; the grid is capped and the workgroups stride over the chunks.
constexpr int MT_CHUNK = 8192;        // floats: 8 x 16 B per lane of a 256-lane workgroup
constexpr int MT_GRID_CAP = 2048;     // 8 workgroups per CU
constexpr int MT_THREADS = 256;
constexpr int MT_FINISH_THREADS = 1024;
typedef vitamd_mt_row MtRow;
static_assert(sizeof(MtRow) == 80 && MT_CHUNK % 4 == 0, "the row layout is part of the ABI");

// the row of a chunk: the last r with first_chunk <= chunk (rows[0].first_chunk == 0).  Wave-uniform, so the loads are scalar loads.
__device__ __forceinline__ int mt_find_row(const MtRow* __restrict__ rows, int n_rows, int chunk) {
  int lo = 0, hi = n_rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// element offset of the chunk inside its tensor, and how many elements of the tensor it holds
__device__ __forceinline__ void mt_span(const MtRow& row, int chunk, long long& off, int& len) {
  off = (long long)(chunk - row.first_chunk) * MT_CHUNK;
  const long long rest = row.n - off;
  len = rest < MT_CHUNK ? (int)rest : MT_CHUNK;
}

// partials[chunk] = sum of g^2 over the chunk, fp32: a lane adds its 16-byte pieces in ascending order (then, in the last chunk of a
// tensor, lanes 0 .. n % 4 - 1 one tail element each), the 64 lanes of a wave are merged by the xor butterfly, the four waves in order.
__global__ __launch_bounds__(MT_THREADS) void mt_sumsq_kernel(const MtRow* __restrict__ rows, int n_rows, int total_chunks,
                                                              float* __restrict__ partials) {
  __shared__ float red[MT_THREADS / 64];
  const int t = threadIdx.x;
  for (int chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
    const MtRow& row = rows[mt_find_row(rows, n_rows, chunk)];
    long long off;
    int len;
    mt_span(row, chunk, off, len);
    const float* g = row.g + off;
    const int n4 = len >> 2;
    float acc = 0.f;
#pragma unroll 4
    for (int i = t; i < n4; i += MT_THREADS) {
      const f32x4 gv = *(const f32x4*)(g + 4 * i);
      acc += gv[0] * gv[0];
      acc += gv[1] * gv[1];
      acc += gv[2] * gv[2];
      acc += gv[3] * gv[3];
    }
    if (t < (len & 3)) { const float x = g[4 * n4 + t]; acc += x * x; }
    acc = wave_sum(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) partials[chunk] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();                        // red is rewritten by the next chunk
  }
}

// out[0] = norm = fp32(sqrt(sum of the partials)), out[1] = the clip coefficient.  One workgroup: lane t adds partials t, t + 1024, ...
// in ascending order in fp64, then the 1024 sums are halved ten times in LDS; the order depends on total_chunks alone.
// coef as torch.nn.utils.clip_grad_norm_ forms it in fp32: max_norm / (norm + 1e-6) is evaluated there as reciprocal(norm + 1e-6) *
// max_norm, then clamped to at most 1 (a NaN stays a NaN).  max_norm <= 0: no clipping was asked for, coef = 1.
__global__ __launch_bounds__(MT_FINISH_THREADS) void mt_finish_kernel(const float* __restrict__ partials, int total_chunks, float max_norm,
                                                                      float* __restrict__ out) {
  __shared__ double red[MT_FINISH_THREADS];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < total_chunks; i += MT_FINISH_THREADS) s += (double)partials[i];
  red[t] = s;
  __syncthreads();
  for (int h = MT_FINISH_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) {
    const float norm = (float)sqrt(red[0]);
    float coef = 1.0f;
    if (max_norm > 0.f) {
      const float c = (1.0f / (norm + 1e-6f)) * max_norm;
      coef = c > 1.0f ? 1.0f : c;
    }
    out[0] = norm;
    out[1] = coef;
  }
}

// the update over the table; SCALED: the gradient is multiplied by *coef first (rounded to fp32, as an in-place clip would leave it)
template <bool SCALED>
__global__ __launch_bounds__(MT_THREADS) void mt_adamw_kernel(const MtRow* __restrict__ rows, int n_rows, int total_chunks,
                                                              const float* __restrict__ coef_ptr) {
  const int t = threadIdx.x;
  float coef = 1.0f;
  if constexpr (SCALED) coef = *coef_ptr;
  for (int chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
    const MtRow& row = rows[mt_find_row(rows, n_rows, chunk)];
    long long off;
    int len;
    mt_span(row, chunk, off, len);
    float* __restrict__ p = row.p + off;
    const float* __restrict__ g = row.g + off;
    float* __restrict__ m = row.m + off;
    float* __restrict__ v = row.v + off;
    const float b1 = row.beta1, omb1 = row.one_minus_beta1, b2 = row.beta2, omb2 = row.one_minus_beta2, eps = row.eps,
                inv_sqrt_bc2 = row.inv_sqrt_bc2;
    float decay, step;
    adamw_scalars(row.lr, row.weight_decay, row.inv_bc1, decay, step);
    const int n4 = len >> 2;
#pragma unroll 2
    for (int i = t; i < n4; i += MT_THREADS) {
      f32x4 pv = *(const f32x4*)(p + 4 * i);
      const f32x4 gv = *(const f32x4*)(g + 4 * i);
      f32x4 mv = *(const f32x4*)(m + 4 * i), vv = *(const f32x4*)(v + 4 * i);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float pc = pv[c], gc = gv[c], mc = mv[c], vc = vv[c];
        if constexpr (SCALED) gc *= coef;
        adamw_elem<true>(pc, gc, mc, vc, decay, step, b1, omb1, b2, omb2, eps, inv_sqrt_bc2);
        pv[c] = pc; mv[c] = mc; vv[c] = vc;
      }
      *(f32x4*)(p + 4 * i) = pv;
      *(f32x4*)(m + 4 * i) = mv;
      *(f32x4*)(v + 4 * i) = vv;
    }
    if (t < (len & 3)) {
      const int i = 4 * n4 + t;
      float pv = p[i], gv = g[i], mv = m[i], vv = v[i];
      if constexpr (SCALED) gv *= coef;
      adamw_elem<false>(pv, gv, mv, vv, decay, step, b1, omb1, b2, omb2, eps, inv_sqrt_bc2);
      p[i] = pv; m[i] = mv; v[i] = vv;
    }
  }
}

// g *= *coef in place; nothing is stored when the coefficient is exactly 1
__global__ __launch_bounds__(MT_THREADS) void mt_scale_kernel(const MtRow* __restrict__ rows, int n_rows, int total_chunks,
                                                              const float* __restrict__ coef_ptr) {
  const float coef = *coef_ptr;
  if (coef == 1.0f) return;
  const int t = threadIdx.x;
  for (int chunk = blockIdx.x; chunk < total_chunks; chunk += gridDim.x) {
    const MtRow& row = rows[mt_find_row(rows, n_rows, chunk)];
    long long off;
    int len;
    mt_span(row, chunk, off, len);
    float* g = const_cast<float*>(row.g) + off;
    const int n4 = len >> 2;
#pragma unroll 4
    for (int i = t; i < n4; i += MT_THREADS) {
      f32x4 gv = *(const f32x4*)(g + 4 * i);
#pragma unroll
      for (int c = 0; c < 4; ++c) gv[c] *= coef;
      *(f32x4*)(g + 4 * i) = gv;
    }
    if (t < (len & 3)) g[4 * n4 + t] *= coef;
  }
}

// The step-dependent floats of every row, derived on the device from the row's schedule entry: one thread per
// row advances the two counters and rewrites lr, inv_bc1 and inv_sqrt_bc2, so that a table which stays in device memory - and a graph
// that recorded the launches over it - sees every step's values without the host.  fp64 throughout, each result rounded to fp32 once: the
// bias corrections in the order vitamd_adamw_step_d forms them, the factor in the order of utils.lr_factor (contraction off: Python fuses
// nothing).  Every store is an ordinary per-lane store to the lane's own row.
typedef vitamd_sched_row MtSched;
static_assert(sizeof(MtSched) == 64, "the schedule entry is part of the ABI");
constexpr int MT_ADVANCE_THREADS = 256;

__device__ __forceinline__ double mt_lr_factor(long long t, long long warmup, long long train, double min_ratio) {
#pragma clang fp contract(off)
  if (train == 0) return 1.0;                                   // no schedule: constant base_lr
  if (t < warmup) {
    const double f = (double)t / (double)warmup;
    return f < 1.0 ? f : 1.0;
  }
  if (t < train) {
    const double tt = (double)(t - warmup);                     // the cosine counts from the warm-up milestone
    return min_ratio + (1.0 - min_ratio) * (1.0 + cos(3.14159265358979323846 * tt / (double)train)) / 2.0;
  }
  return 1.0;                                                   // from train_steps on: back at base_lr
}

__global__ __launch_bounds__(MT_ADVANCE_THREADS) void mt_advance_kernel(MtRow* __restrict__ rows, MtSched* __restrict__ sched, int n_rows) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * MT_ADVANCE_THREADS + threadIdx.x;
  if (r >= n_rows) return;
  const MtSched s = sched[r];
  const long long k = s.step + 1, t = s.sched_t;
  sched[r].step = k;
  sched[r].sched_t = t + 1;
  const double bc1 = 1.0 - pow(s.beta1, (double)k), bc2 = 1.0 - pow(s.beta2, (double)k);
  rows[r].inv_bc1 = (float)(1.0 / bc1);
  rows[r].inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  rows[r].lr = (float)(s.base_lr * mt_lr_factor(t, s.warmup_steps, s.train_steps, s.min_ratio));
}

// The host's copy of the table is what the entry points check: the chunk plan (first_chunk is the running sum of ceil(n / MT_CHUNK), the
// total is total_chunks, so no chunk index can reach past a tensor) and every tensor pointer, before anything is launched.
int mt_check(const MtRow* rows, int n_rows, int total_chunks, bool with_state) {
  if (n_rows < 1 || total_chunks < 1) return VITAMD_ERR_SHAPE;
  if (!rows) return VITAMD_ERR_ARG;
  long long next = 0;
  for (int r = 0; r < n_rows; ++r) {
    if (rows[r].n < 1 || rows[r].first_chunk != next) return VITAMD_ERR_SHAPE;
    next += (rows[r].n + MT_CHUNK - 1) / MT_CHUNK;
    if (next > 0x7fffffffLL) return VITAMD_ERR_SHAPE;
  }
  if (next != total_chunks) return VITAMD_ERR_SHAPE;
  for (int r = 0; r < n_rows; ++r) {
    if (!rows[r].g || ((uintptr_t)rows[r].g & 15)) return VITAMD_ERR_ARG;
    if (!with_state) continue;
    if (!rows[r].p || !rows[r].m || !rows[r].v) return VITAMD_ERR_ARG;
    if (((uintptr_t)rows[r].p | (uintptr_t)rows[r].m | (uintptr_t)rows[r].v) & 15) return VITAMD_ERR_ARG;
  }
  return VITAMD_OK;
}

inline int mt_grid(int total_chunks) { return total_chunks < MT_GRID_CAP ? total_chunks : MT_GRID_CAP; }

}  // namespace

// beta1 / beta2 as the caller's doubles (torch.optim.AdamW holds them as Python floats): the kernel's four coefficients beta and 1 - beta are
// each rounded to fp32 once, and the bias corrections use the same doubles.
extern "C" int vitamd_adamw_step_d(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2,
                                   float eps, float weight_decay, int step, void* stream) {
  if (n < 0 || step < 1) return VITAMD_ERR_SHAPE;
  if (n == 0) return VITAMD_OK;
  if (!p || !g || !m || !v) return VITAMD_ERR_ARG;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) return VITAMD_ERR_ARG;
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  const size_t n4 = (size_t)n / 4;
  int grid = (int)((n4 + 255) / 256);
  grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4, (size_t)n, lr, (float)beta1, (float)(1.0 - beta1),
                     (float)beta2, (float)(1.0 - beta2), eps, weight_decay, (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)));
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

// the same with fp32 betas (1 - beta is then exact in fp32: the arithmetic this entry point has always had)
extern "C" int vitamd_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, int step, void* stream) {
  return vitamd_adamw_step_d(p, g, m, v, n, lr, (double)beta1, (double)beta2, eps, weight_decay, step, stream);
}

extern "C" long vitamd_mt_row_bytes(void) { return (long)sizeof(MtRow); }
extern "C" int vitamd_mt_chunk_elems(void) { return MT_CHUNK; }
extern "C" int vitamd_mt_grid_cap(void) { return MT_GRID_CAP; }

extern "C" int vitamd_mt_sumsq(const vitamd_mt_row* rows_host, const void* rows_dev, int n_rows, int total_chunks, float* partials,
                               float* norm_coef, float max_norm, void* stream) {
  const int rc = mt_check(rows_host, n_rows, total_chunks, false);
  if (rc != VITAMD_OK) return rc;
  if (!rows_dev || !partials || !norm_coef) return VITAMD_ERR_ARG;
  hipLaunchKernelGGL(mt_sumsq_kernel, dim3(mt_grid(total_chunks)), dim3(MT_THREADS), 0, (hipStream_t)stream, (const MtRow*)rows_dev, n_rows,
                     total_chunks, partials);
  hipLaunchKernelGGL(mt_finish_kernel, dim3(1), dim3(MT_FINISH_THREADS), 0, (hipStream_t)stream, (const float*)partials, total_chunks, max_norm,
                     norm_coef);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_mt_adamw(const vitamd_mt_row* rows_host, const void* rows_dev, int n_rows, int total_chunks, const float* coef,
                               void* stream) {
  const int rc = mt_check(rows_host, n_rows, total_chunks, true);
  if (rc != VITAMD_OK) return rc;
  if (!rows_dev) return VITAMD_ERR_ARG;
  const dim3 grid(mt_grid(total_chunks)), block(MT_THREADS);
  if (coef) hipLaunchKernelGGL(mt_adamw_kernel<true>, grid, block, 0, (hipStream_t)stream, (const MtRow*)rows_dev, n_rows, total_chunks, coef);
  else hipLaunchKernelGGL(mt_adamw_kernel<false>, grid, block, 0, (hipStream_t)stream, (const MtRow*)rows_dev, n_rows, total_chunks, coef);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" long vitamd_sched_row_bytes(void) { return (long)sizeof(MtSched); }

extern "C" int vitamd_sched_advance(void* rows_dev, void* sched_dev, int n_rows, void* stream) {
  if (n_rows < 1) return VITAMD_ERR_SHAPE;
  if (!rows_dev || !sched_dev || (((uintptr_t)rows_dev | (uintptr_t)sched_dev) & 7)) return VITAMD_ERR_ARG;
  const int grid = (int)(((long long)n_rows + MT_ADVANCE_THREADS - 1) / MT_ADVANCE_THREADS);      // n_rows <= 2^31 - 1: at most 2^23 workgroups
  hipLaunchKernelGGL(mt_advance_kernel, dim3(grid), dim3(MT_ADVANCE_THREADS), 0, (hipStream_t)stream, (MtRow*)rows_dev, (MtSched*)sched_dev, n_rows);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_mt_scale(const vitamd_mt_row* rows_host, const void* rows_dev, int n_rows, int total_chunks, const float* coef,
                               void* stream) {
  const int rc = mt_check(rows_host, n_rows, total_chunks, false);
  if (rc != VITAMD_OK) return rc;
  if (!rows_dev || !coef) return VITAMD_ERR_ARG;
  hipLaunchKernelGGL(mt_scale_kernel, dim3(mt_grid(total_chunks)), dim3(MT_THREADS), 0, (hipStream_t)stream, (const MtRow*)rows_dev, n_rows,
                     total_chunks, coef);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
