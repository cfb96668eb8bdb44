// Training of the causal stack: mean cross-entropy over rows of logits, forward and backward, and the token +
// position embedding, forward and backward.  The two halves share no code.
//
// Cross-entropy.  All arithmetic is fp32 on the logits as stored (fp32 or bf16).  A row is owned by one wave (V <= 4096) or by the four
// waves of a workgroup (longer rows); every lane walks its 16-byte pieces of the row once, keeping a running maximum m and the sum s of
// exp(x - m) (the online form: a piece with a larger maximum rescales s), lanes and waves are merged in a fixed order, and
// lse = m + ln(s).  exp and ln are the hardware's base-2 operations with the log2(e) / ln(2) factor applied to the DIFFERENCE x - m
// (exact for neighbouring values), never to x itself.  -inf logits add exp2(-inf) = 0.  The mean is formed by a second, single-workgroup
// launch that sums the per-row losses in a fixed order and counts the rows with an integer: no float atomics, the same bits every call.
// The backward is one pass: dlogits = (exp(x - lse) - onehot) * (*grad_out / count), each lane writing the piece it has just read, so
// it may run in place.  Rows whose target is ignore_index (or outside [0, V)) are written as zeros without being read.
// The soft-target pair (Mixup / CutMix / label smoothing) is the SOFT form of the same two kernels: the row walk
// also carries the plain sum of the row, and the one-hot becomes (1-e) (l [ya] + (1-l) [yb]) + e / V.
// Evaluation (at the end of the file) is the RANK form of the forward kernel - the same walk also counts the
// columns that rank above the target - and a single-workgroup launch that adds loss, rows, top-1 and top-k hits to device counters.
#include "common.h"
#include "../../include/vitamd.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr float NEG_BIG = -3.0e38f;   // running maximum before the first element: finite, so that exp2 of (NEG_BIG - NEG_BIG) is 1 and never NaN
constexpr int CE_MAX_V = VITAMD_CE_MAX_V;
constexpr int CE_WIDE_V = 4096;       // longer rows: the four waves of a workgroup share one row
constexpr int CE_GRID_CAP = 2048;     // workgroups per launch; further rows are reached by the row-stride loop
constexpr int EMB_GRID_CAP = 8192;

template <bool BF16> struct Elem { typedef float type; };
template <> struct Elem<true> { typedef __bf16 type; };

template <bool BF16>
__device__ __forceinline__ float load_one(const void* row, int c) {
  if constexpr (BF16) return bf2f(((const __bf16*)row)[c]);
  else return ((const float*)row)[c];
}
template <bool BF16>
__device__ __forceinline__ void store_one(void* row, int c, float v) {
  if constexpr (BF16) ((__bf16*)row)[c] = f2bf(v);
  else ((float*)row)[c] = v;
}
// piece i of a row: W consecutive elements from column i * W, in 16-byte accesses (bf16: W == 8)
template <bool BF16, int W>
__device__ __forceinline__ void load_piece(const void* row, int i, float (&f)[W]) {
  if constexpr (BF16) {
    static_assert(W == 8, "a bf16 piece is 8 elements");
    const u32x4 v = *(const u32x4*)((const __bf16*)row + (size_t)i * 8);
#pragma unroll
    for (int c = 0; c < 4; ++c) { f[2 * c] = bf16lo(v[c]); f[2 * c + 1] = bf16hi(v[c]); }
  } else {
#pragma unroll
    for (int k = 0; k < W / 4; ++k) {
      const f32x4 v = *(const f32x4*)((const float*)row + (size_t)i * W + 4 * k);
#pragma unroll
      for (int c = 0; c < 4; ++c) f[4 * k + c] = v[c];
    }
  }
}
template <bool BF16, int W>
__device__ __forceinline__ void store_piece(void* row, int i, const float (&f)[W]) {
  if constexpr (BF16) {
    static_assert(W == 8, "a bf16 piece is 8 elements");
    *(u32x4*)((__bf16*)row + (size_t)i * 8) =
        (u32x4){pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
  } else {
#pragma unroll
    for (int k = 0; k < W / 4; ++k)
      *(f32x4*)((float*)row + (size_t)i * W + 4 * k) = (f32x4){f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]};
  }
}

__device__ __forceinline__ float ex2(float d) { return __builtin_amdgcn_exp2f(d * LOG2E); }   // exp(d)

// (m, s) <- (m, s) merged with (m2, s2): s counts exp(x - m).  FUSED = false leaves the contraction of s * e + s2 * e2 to the compiler,
// as the training forms always have (their bits stay what they were): in the plain form it fuses the first product and rounds the
// second everywhere.  FUSED = true spells exactly that out.  The evaluation form needs it: left to the compiler, the vectoriser packed
// its last lane merge into two rounded products and an add, one rounding away from the plain form's loss.
template <bool FUSED = false>
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if constexpr (FUSED) s = __builtin_fmaf(s, ex2(m - mn), s2 * ex2(m2 - mn));
  else s = s * ex2(m - mn) + s2 * ex2(m2 - mn);
  m = mn;
}

// ------------------------------------------------------------------------------------------------ cross-entropy forward
// The soft target of vitamd_soft_cross_entropy_fwd / _bwd: t[v] = (1-e) (l [v == ya] + (1-l) [v == yb]) + e / V, ya = the kernels'
// `target`.  lam == nullptr: l = 1 and target_b is not looked at.
struct Soft { const long long* target_b; const float* lam; float smoothing; };

// VEC: base and row stride allow 16-byte loads; the V % W columns after the last whole piece are read one by one.  WIDE: one row per
// workgroup (256 lanes) instead of one per wave.  SOFT: the same walk also carries the plain sum of the row (the smoothing term), merged
// over lanes and waves beside (m, s), and the row's loss is the soft-target one; no row is ignored.  RANK (the evaluation form,
// vitamd_classify_metrics; never with SOFT): every lane first loads the target's logit x_t, the walk also counts the columns that rank
// above the target (rank_above), the count is merged by integer adds and written to rank_out; a row whose target is ignore_index is
// not read (rank -1, loss 0) and no lse is written.  Its (m, s) arithmetic rounds as the plain form's does (merge<true>), so the
// two losses of a row are the same bits.
__device__ __forceinline__ int rank_above(float x, int c, float xt, int tcol) {
  return (c != tcol && !(x < xt || (x == xt && c > tcol))) ? 1 : 0;      // a NaN compares false: it ranks above, a NaN target below all
}

template <bool BF16, bool VEC, bool WIDE, bool SOFT, bool RANK = false>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const void* logits, const long long* __restrict__ target, float* __restrict__ loss_row,
                                                    float* __restrict__ lse_out, int M, int V, int ld, long long ignore_index, Soft soft,
                                                    int* __restrict__ rank_out = nullptr) {
  static_assert(!(SOFT && RANK), "the evaluation form has hard targets");
  constexpr int W = BF16 ? 8 : 4;
  constexpr int TPR = WIDE ? 256 : 64;      // lanes per row
  constexpr int RPW = 256 / TPR;            // rows per workgroup
  typedef typename Elem<BF16>::type T;
  __shared__ float red[3][4];
  __shared__ int redn[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = WIDE ? (int)threadIdx.x : lane;
  for (long row0 = (long)blockIdx.x * RPW; row0 < M; row0 += (long)gridDim.x * RPW) {
    const long row = row0 + (WIDE ? 0 : w);
    if (row >= M) continue;                 // wave-uniform (never taken when WIDE: no barrier is skipped)
    const T* xr = (const T*)logits + (size_t)row * ld;
    float m = NEG_BIG, s = 0.f, sx = 0.f;     // sx: the sum of the row's logits (SOFT)
    float xt = 0.f;                           // RANK: the target's logit (NaN for a target outside [0, V): no address is formed)
    int tcol = -1, above = 0;
    if constexpr (RANK) {
      const long long tg = target[row];       // uniform over the lanes that share the row
      if (tg == ignore_index) {               // not read; WIDE: the whole workgroup leaves, no barrier is skipped by a part of it
        if (t == 0) { loss_row[row] = 0.f; rank_out[row] = -1; }
        continue;
      }
      const bool in_range = tg >= 0 && tg < V;
      tcol = in_range ? (int)tg : -1;
      xt = in_range ? load_one<BF16>(xr, tcol) : __builtin_nanf("");
    }
    if constexpr (VEC) {
      const int nvec = V / W;
#pragma unroll 2
      for (int i = t; i < nvec; i += TPR) {
        float f[W];
        load_piece<BF16, W>(xr, i, f);
        if constexpr (SOFT) {
#pragma unroll
          for (int j = 0; j < W; ++j) sx += f[j];
        }
        if constexpr (RANK) {
#pragma unroll
          for (int j = 0; j < W; ++j) above += rank_above(f[j], i * W + j, xt, tcol);
        }
        float vm = f[0];
#pragma unroll
        for (int j = 1; j < W; ++j) vm = fmaxf(vm, f[j]);
        const float mn = fmaxf(m, vm);
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < W; ++j) a += ex2(f[j] - mn);
        if constexpr (RANK) s = __builtin_fmaf(s, ex2(m - mn), a);      // as merge<true>: what the plain form's contraction gives
        else s = s * ex2(m - mn) + a;
        m = mn;
      }
      const int c = nvec * W + t;
      if (c < V) {
        const float x = load_one<BF16>(xr, c);
        merge<RANK>(m, s, x, 1.f);
        if constexpr (SOFT) sx += x;
        if constexpr (RANK) above += rank_above(x, c, xt, tcol);
      }
    } else {
      for (int c = t; c < V; c += TPR) {
        const float x = load_one<BF16>(xr, c);
        merge<RANK>(m, s, x, 1.f);
        if constexpr (SOFT) sx += x;
        if constexpr (RANK) above += rank_above(x, c, xt, tcol);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      merge<RANK>(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
      if constexpr (SOFT) sx += __shfl_xor(sx, o, 64);
      if constexpr (RANK) above += __shfl_xor(above, o, 64);
    }
    if constexpr (WIDE) {
      if (lane == 0) {
        red[0][w] = m; red[1][w] = s; red[2][w] = sx;
        if constexpr (RANK) redn[w] = above;
      }
      __syncthreads();
      m = red[0][0]; s = red[1][0]; sx = red[2][0];
#pragma unroll
      for (int i = 1; i < 4; ++i) { merge<RANK>(m, s, red[0][i], red[1][i]); sx += red[2][i]; }
      if constexpr (RANK) above = (redn[0] + redn[1]) + (redn[2] + redn[3]);
      __syncthreads();                      // red is rewritten by the next row
    }
    if (t == 0) {
      const float lse = RANK ? __builtin_fmaf(__builtin_amdgcn_logf(s), LN2, m) : m + __builtin_amdgcn_logf(s) * LN2;
      if constexpr (RANK) {                   // xt is the value the plain form loads below: the same subtraction, the same bits
        loss_row[row] = tcol >= 0 ? lse - xt : __builtin_nanf("");
        rank_out[row] = above;
        continue;
      }
      const long long tg = target[row];
      float loss = 0.f;
      if constexpr (SOFT) {
        const float e = soft.smoothing, l = soft.lam ? soft.lam[row] : 1.f;
        const long long tb = soft.lam ? soft.target_b[row] : tg;
        if (tg >= 0 && tg < V && tb >= 0 && tb < V) {
          float hard = load_one<BF16>(xr, (int)tg);                 // lam == nullptr: x[ya] itself, so that e == 0 gives lse - x[ya]
          if (soft.lam) {
            const float lb = 1.f - l;                               // a zero weight forms no term: its logit may be -inf
            hard = (l != 0.f ? l * hard : 0.f) + (lb != 0.f ? lb * load_one<BF16>(xr, (int)tb) : 0.f);
          }
          float inner = (1.f - e) * hard;
          if (e != 0.f) inner += e / (float)V * sx;
          loss = lse - inner;
        } else {
          loss = __builtin_nanf("");
        }
      } else {
        if (tg != ignore_index) loss = (tg >= 0 && tg < V) ? lse - load_one<BF16>(xr, (int)tg) : __builtin_nanf("");
      }
      lse_out[row] = lse;
      loss_row[row] = loss;
    }
  }
}

// stats = {sum(loss_row) / count, 1 / count}, count = the rows whose target is not ignore_index (target == nullptr: every row): one
// workgroup, a fixed order
__global__ __launch_bounds__(1024) void ce_mean_kernel(const float* __restrict__ loss_row, const long long* __restrict__ target,
                                                      float* __restrict__ stats, int M, long long ignore_index) {
  __shared__ float ssum[16];
  __shared__ int scnt[16];
  float a = 0.f;
  int n = 0;
  for (int i = threadIdx.x; i < M; i += 1024) {
    a += loss_row[i];
    n += !target || target[i] != ignore_index ? 1 : 0;
  }
  a = wave_sum(a);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) { ssum[threadIdx.x >> 6] = a; scnt[threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  a = 0.f; n = 0;
  for (int i = 0; i < 16; ++i) { a += ssum[i]; n += scnt[i]; }
  stats[0] = a / (float)n;                  // every row ignored: 0 / 0 = NaN, as the framework's mean
  stats[1] = 1.f / (float)n;
}

// ------------------------------------------------------------------------------------------------ cross-entropy backward
// tpr = lanes per row (64 or 256).  logits and dlogits may be the same buffer: a lane writes the piece it has just read.
// What is subtracted from the softmax at column c is hot_weight(c): 1 at the target's column, or the soft target (SOFT).
struct Hot {
  int a, b;                 // the columns of ya and yb (-1: none)
  float wa, wb, u;          // (1-e) l, (1-e) (1-l), e / V
  template <bool SOFT>
  __device__ __forceinline__ float weight(int c) const {
    if constexpr (SOFT) return (c == a ? wa : 0.f) + (c == b ? wb : 0.f) + u;
    else return c == a ? 1.f : 0.f;
  }
};

template <bool IN_BF16, bool OUT_BF16, bool VEC, bool SOFT>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const void* logits, const long long* __restrict__ target, const float* __restrict__ lse,
                                                    const float* __restrict__ stats, const float* __restrict__ grad_out, void* dlogits, int M,
                                                    int V, int ld, int ldo, long long ignore_index, int tpr, Soft soft) {
  constexpr int W = (IN_BF16 || OUT_BF16) ? 8 : 4;
  typedef typename Elem<IN_BF16>::type TI;
  typedef typename Elem<OUT_BF16>::type TO;
  const int rpw = 256 / tpr, t = threadIdx.x % tpr, r = threadIdx.x / tpr;
  const float scale = (grad_out ? *grad_out : 1.f) * stats[1];
  for (long row = (long)blockIdx.x * rpw + r; row < M; row += (long)gridDim.x * rpw) {
    const long long tg = target[row];
    bool live = tg >= 0 && tg < V;
    Hot hot = {live ? (int)tg : -1, -1, 1.f, 0.f, 0.f};
    if constexpr (SOFT) {
      const float e = soft.smoothing;
      hot.wa = 1.f - e;
      hot.u = e / (float)V;
      if (soft.lam) {
        const long long tb = soft.target_b[row];
        const float lm = soft.lam[row];
        live = live && tb >= 0 && tb < V;
        hot.b = live ? (int)tb : -1;
        hot.wa = (1.f - e) * lm;
        hot.wb = (1.f - e) * (1.f - lm);
      }
    } else {
      live = live && tg != ignore_index;
    }
    const float l = lse[row];
    const TI* xr = (const TI*)logits + (size_t)row * ld;
    TO* dr = (TO*)dlogits + (size_t)row * ldo;
    if constexpr (VEC) {
      const int nvec = V / W;
#pragma unroll 2
      for (int i = t; i < nvec; i += tpr) {
        float f[W];
        if (live) {
          load_piece<IN_BF16, W>(xr, i, f);
#pragma unroll
          for (int j = 0; j < W; ++j) f[j] = (ex2(f[j] - l) - hot.weight<SOFT>(i * W + j)) * scale;
        } else {
#pragma unroll
          for (int j = 0; j < W; ++j) f[j] = 0.f;
        }
        store_piece<OUT_BF16, W>(dr, i, f);
      }
      const int c = nvec * W + t;
      if (c < V) store_one<OUT_BF16>(dr, c, live ? (ex2(load_one<IN_BF16>(xr, c) - l) - hot.weight<SOFT>(c)) * scale : 0.f);
    } else {
      for (int c = t; c < V; c += tpr)
        store_one<OUT_BF16>(dr, c, live ? (ex2(load_one<IN_BF16>(xr, c) - l) - hot.weight<SOFT>(c)) * scale : 0.f);
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int ce_grid(int M, int rows_per_wg) {
  const long g = ((long)M + rows_per_wg - 1) / rows_per_wg;
  return (int)(g < CE_GRID_CAP ? g : CE_GRID_CAP);
}

template <bool BF16, bool VEC, bool SOFT, bool RANK = false>
void launch_ce_fwd(const void* logits, const long long* target, float* loss_row, float* lse, int M, int V, int ld, long long ignore_index,
                   Soft soft, hipStream_t s, int* rank = nullptr) {
  if (V > CE_WIDE_V)
    hipLaunchKernelGGL((ce_fwd_kernel<BF16, VEC, true, SOFT, RANK>), dim3(ce_grid(M, 1)), dim3(256), 0, s, logits, target, loss_row, lse, M, V,
                       ld, ignore_index, soft, rank);
  else
    hipLaunchKernelGGL((ce_fwd_kernel<BF16, VEC, false, SOFT, RANK>), dim3(ce_grid(M, 4)), dim3(256), 0, s, logits, target, loss_row, lse, M, V,
                       ld, ignore_index, soft, rank);
}

template <bool IN_BF16, bool OUT_BF16, bool SOFT>
void launch_ce_bwd(bool vec, const void* logits, const long long* target, const float* lse, const float* stats, const float* grad_out,
                   void* dlogits, int M, int V, int ld, int ldo, long long ignore_index, Soft soft, hipStream_t s) {
  const int tpr = V > CE_WIDE_V ? 256 : 64;
  const dim3 grid(ce_grid(M, 256 / tpr));
  if (vec)
    hipLaunchKernelGGL((ce_bwd_kernel<IN_BF16, OUT_BF16, true, SOFT>), grid, dim3(256), 0, s, logits, target, lse, stats, grad_out, dlogits, M, V,
                       ld, ldo, ignore_index, tpr, soft);
  else
    hipLaunchKernelGGL((ce_bwd_kernel<IN_BF16, OUT_BF16, false, SOFT>), grid, dim3(256), 0, s, logits, target, lse, stats, grad_out, dlogits, M, V,
                       ld, ldo, ignore_index, tpr, soft);
}

// the soft target's own argument rules (after the shape check): smoothing in [0, 1], target_b wherever lam is given
inline bool soft_ok(const Soft& soft) { return soft.smoothing >= 0.f && soft.smoothing <= 1.f && (!soft.lam || soft.target_b); }

// the bodies of the two pairs of entries; SOFT: the mean is over every row (no target is handed to the mean kernel)
template <bool SOFT>
int ce_fwd(const void* logits, int logits_bf16, const long long* target, float* loss_row, float* lse, float* stats, int M, int V, int ld,
           long long ignore_index, Soft soft, void* stream) {
  if (M < 1 || V < 2 || V > CE_MAX_V || ld < V) return VITAMD_ERR_SHAPE;
  if (!logits || !target || !loss_row || !lse || !stats || (SOFT && !soft_ok(soft))) return VITAMD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = aligned16(logits) && ld % (logits_bf16 ? 8 : 4) == 0;
  if (logits_bf16) {
    if (vec) launch_ce_fwd<true, true, SOFT>(logits, target, loss_row, lse, M, V, ld, ignore_index, soft, s);
    else launch_ce_fwd<true, false, SOFT>(logits, target, loss_row, lse, M, V, ld, ignore_index, soft, s);
  } else {
    if (vec) launch_ce_fwd<false, true, SOFT>(logits, target, loss_row, lse, M, V, ld, ignore_index, soft, s);
    else launch_ce_fwd<false, false, SOFT>(logits, target, loss_row, lse, M, V, ld, ignore_index, soft, s);
  }
  hipLaunchKernelGGL(ce_mean_kernel, dim3(1), dim3(1024), 0, s, (const float*)loss_row, SOFT ? nullptr : target, stats, M, ignore_index);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

template <bool SOFT>
int ce_bwd(const void* logits, int logits_bf16, const long long* target, const float* lse, const float* stats, const float* grad_out,
           void* dlogits, int dlogits_bf16, int M, int V, int ld, int ldo, long long ignore_index, Soft soft, void* stream) {
  if (M < 1 || V < 2 || V > CE_MAX_V || ld < V || ldo < V) return VITAMD_ERR_SHAPE;
  if (!logits || !target || !lse || !stats || !dlogits || (SOFT && !soft_ok(soft))) return VITAMD_ERR_ARG;
  if (logits == dlogits && (!logits_bf16 != !dlogits_bf16 || ld != ldo)) return VITAMD_ERR_ARG;   // in place: same type and stride only
  hipStream_t s = (hipStream_t)stream;
  // a piece is 8 elements when either side is bf16, else 4: fp32 rows then need a stride that keeps both 16-byte halves aligned
  const bool vec = aligned16(logits) && aligned16(dlogits) && ld % (logits_bf16 ? 8 : 4) == 0 && ldo % (dlogits_bf16 ? 8 : 4) == 0;
  if (logits_bf16) {
    if (dlogits_bf16) launch_ce_bwd<true, true, SOFT>(vec, logits, target, lse, stats, grad_out, dlogits, M, V, ld, ldo, ignore_index, soft, s);
    else launch_ce_bwd<true, false, SOFT>(vec, logits, target, lse, stats, grad_out, dlogits, M, V, ld, ldo, ignore_index, soft, s);
  } else {
    if (dlogits_bf16) launch_ce_bwd<false, true, SOFT>(vec, logits, target, lse, stats, grad_out, dlogits, M, V, ld, ldo, ignore_index, soft, s);
    else launch_ce_bwd<false, false, SOFT>(vec, logits, target, lse, stats, grad_out, dlogits, M, V, ld, ldo, ignore_index, soft, s);
  }
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ token + position embedding
// x[r, :] = tok[ids[r], :] + pos[r % S, :], one lane per 4 columns.  An id outside the table: the row is left alone.
__global__ __launch_bounds__(256) void embed_tokens_fwd_kernel(const float* __restrict__ tok, const float* __restrict__ pos,
                                                              const long long* __restrict__ ids, float* __restrict__ x, long n4, int S, int D,
                                                              int tok_rows) {
  const int dq = D / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long r = i / dq;
    const int c = (int)(i - r * dq) * 4;
    const long long id = ids[r];
    if (id < 0 || id >= tok_rows) continue;
    const int s = (int)(r % S);
    const f32x4 a = *(const f32x4*)(tok + (size_t)id * D + c);
    const f32x4 e = *(const f32x4*)(pos + (size_t)s * D + c);
    *(f32x4*)(x + (size_t)r * D + c) = a + e;
  }
}

// Workgroup (s, column block): lane = one column c.  It reads g[b*S + s, c] for b = 0 .. B-1 once: the running sum, in ascending b, goes
// to dpos[s, c], which no other lane touches (no atomics, reproducible); each value is also added to dtok[ids[b*S + s], c] by an fp32
// atomic - a wave-instruction adds 64 contiguous floats of one table row.
__global__ __launch_bounds__(256) void embed_tokens_bwd_kernel(const float* __restrict__ g, const long long* __restrict__ ids,
                                                              float* __restrict__ dtok, float* __restrict__ dpos, int B, int S, int D,
                                                              int tok_rows) {
  const int s = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
  if (c >= D) return;
  float acc = 0.f;
#pragma unroll 4
  for (int b = 0; b < B; ++b) {
    const size_t r = (size_t)b * S + s;
    const float v = g[r * D + c];
    acc += v;
    const long long id = ids[r];
    if (id >= 0 && id < tok_rows) atomicAdd(dtok + (size_t)id * D + c, v);
  }
  dpos[(size_t)s * D + c] += acc;
}

}  // namespace

extern "C" int vitamd_cross_entropy_grid_rows(int V) {
  if (V < 2 || V > CE_MAX_V) return -VITAMD_ERR_SHAPE;
  return CE_GRID_CAP * (V > CE_WIDE_V ? 1 : 4);
}

extern "C" int vitamd_cross_entropy_fwd(const void* logits, int logits_bf16, const long long* target, float* loss_row, float* lse, float* stats,
                                        int M, int V, int ld, long long ignore_index, void* stream) {
  return ce_fwd<false>(logits, logits_bf16, target, loss_row, lse, stats, M, V, ld, ignore_index, Soft{nullptr, nullptr, 0.f}, stream);
}

extern "C" int vitamd_cross_entropy_bwd(const void* logits, int logits_bf16, const long long* target, const float* lse, const float* stats,
                                        const float* grad_out, void* dlogits, int dlogits_bf16, int M, int V, int ld, int ldo,
                                        long long ignore_index, void* stream) {
  return ce_bwd<false>(logits, logits_bf16, target, lse, stats, grad_out, dlogits, dlogits_bf16, M, V, ld, ldo, ignore_index,
                       Soft{nullptr, nullptr, 0.f}, stream);
}

extern "C" int vitamd_soft_cross_entropy_fwd(const void* logits, int logits_bf16, const long long* target_a, const long long* target_b,
                                             const float* lam, float smoothing, float* loss_row, float* lse, float* stats, int M, int V,
                                             int ld, void* stream) {
  return ce_fwd<true>(logits, logits_bf16, target_a, loss_row, lse, stats, M, V, ld, 0, Soft{target_b, lam, smoothing}, stream);
}

extern "C" int vitamd_soft_cross_entropy_bwd(const void* logits, int logits_bf16, const long long* target_a, const long long* target_b,
                                             const float* lam, float smoothing, const float* lse, const float* stats, const float* grad_out,
                                             void* dlogits, int dlogits_bf16, int M, int V, int ld, int ldo, void* stream) {
  return ce_bwd<true>(logits, logits_bf16, target_a, lse, stats, grad_out, dlogits, dlogits_bf16, M, V, ld, ldo, 0,
                      Soft{target_b, lam, smoothing}, stream);
}

extern "C" int vitamd_embed_tokens_fwd(const float* tok_table, const float* pos_table, const long long* ids, float* x, int B, int S, int D,
                                       int tok_rows, int pos_rows, void* stream) {
  if (B < 1 || S < 1 || D < 4 || D % 4 != 0 || tok_rows < 1 || pos_rows < 1 || S > pos_rows) return VITAMD_ERR_SHAPE;
  if (!tok_table || !pos_table || !ids || !x) return VITAMD_ERR_ARG;
  const long n4 = (long)B * S * (D / 4);
  const long wgs = (n4 + 255) / 256;
  hipLaunchKernelGGL(embed_tokens_fwd_kernel, dim3((unsigned)(wgs < EMB_GRID_CAP ? wgs : EMB_GRID_CAP)), dim3(256), 0, (hipStream_t)stream,
                     tok_table, pos_table, ids, x, n4, S, D, tok_rows);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_embed_tokens_bwd(const float* g, const long long* ids, float* dtok, float* dpos, int B, int S, int D, int tok_rows,
                                       void* stream) {
  if (B < 1 || S < 1 || D < 4 || D % 4 != 0 || tok_rows < 1 || (D + 255) / 256 > 65535) return VITAMD_ERR_SHAPE;
  if (!g || !ids || !dtok || !dpos) return VITAMD_ERR_ARG;
  hipLaunchKernelGGL(embed_tokens_bwd_kernel, dim3(S, (D + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, ids, dtok, dpos, B, S, D,
                     tok_rows);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ evaluation
namespace {

// The second launch of vitamd_classify_metrics: one workgroup, a fixed order.  Over the counted rows (rank >= 0) of this call: the fp64
// sum of loss_row, the rows, the rows of rank 0 and the rows of rank < topk; thread 0 then ADDS the four to the caller's accumulators
// with ordinary loads and stores (launches on one stream are ordered: no atomics).
__global__ __launch_bounds__(1024) void metrics_sum_kernel(const float* __restrict__ loss_row, const int* __restrict__ rank,
                                                          double* __restrict__ loss_sum, long long* __restrict__ counts, int M, int topk) {
  __shared__ double ssum[16];
  __shared__ int scnt[3][16];
  double a = 0.0;
  int n = 0, n1 = 0, nk = 0;
  for (int i = threadIdx.x; i < M; i += 1024) {
    const int r = rank[i];
    if (r < 0) continue;
    a += (double)loss_row[i];
    n += 1;
    n1 += r == 0 ? 1 : 0;
    nk += r < topk ? 1 : 0;
  }
  a = wave_sum(a);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    n1 += __shfl_xor(n1, o, 64);
    nk += __shfl_xor(nk, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { ssum[w] = a; scnt[0][w] = n; scnt[1][w] = n1; scnt[2][w] = nk; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  a = 0.0; n = 0; n1 = 0; nk = 0;
  for (int i = 0; i < 16; ++i) { a += ssum[i]; n += scnt[0][i]; n1 += scnt[1][i]; nk += scnt[2][i]; }
  loss_sum[0] += a;
  counts[0] += n;
  counts[1] += n1;
  counts[2] += nk;
}

}  // namespace

extern "C" int vitamd_classify_metrics(const void* logits, int logits_bf16, const long long* target, float* loss_row, int* rank,
                                       double* loss_sum, long long* counts, long M, int V, long ld, int topk, long long ignore_index,
                                       void* stream) {
  if (M < 1 || M > 0x7fffffffL || V < 2 || V > CE_MAX_V || ld < V || ld > 0x7fffffffL) return VITAMD_ERR_SHAPE;
  if (!logits || !target || !loss_row || !rank || !loss_sum || !counts || topk < 1 || topk > V) return VITAMD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int m = (int)M, l = (int)ld;
  const Soft none{nullptr, nullptr, 0.f};
  const bool vec = aligned16(logits) && l % (logits_bf16 ? 8 : 4) == 0;
  if (logits_bf16) {
    if (vec) launch_ce_fwd<true, true, false, true>(logits, target, loss_row, nullptr, m, V, l, ignore_index, none, s, rank);
    else launch_ce_fwd<true, false, false, true>(logits, target, loss_row, nullptr, m, V, l, ignore_index, none, s, rank);
  } else {
    if (vec) launch_ce_fwd<false, true, false, true>(logits, target, loss_row, nullptr, m, V, l, ignore_index, none, s, rank);
    else launch_ce_fwd<false, false, false, true>(logits, target, loss_row, nullptr, m, V, l, ignore_index, none, s, rank);
  }
  hipLaunchKernelGGL(metrics_sum_kernel, dim3(1), dim3(1024), 0, s, (const float*)loss_row, (const int*)rank, loss_sum, counts, m, topk);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
