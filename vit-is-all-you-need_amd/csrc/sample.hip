// Sampled generation: temperature -> top-k -> top-p -> draw on one row of fp32 logits per workgroup, one launch.
//
// Everything that decides the result is integer arithmetic, so a call gives the same bits every time, whatever order the lanes arrive in:
//   - the order of the logits is the order of their uint32 images (key()), taken from x itself, not from x / T: T > 0 keeps the order, and
//     a division in fp32 could merge two neighbouring logits into one tie;
//   - the softmax weight of a logit is the 2^-40 fixed-point image of exp2((x - max) * log2(e) / T), at least one unit for a finite logit
//     and zero for -inf (mass()).  Sums of these are 64-bit integer sums (at most 2^16 terms of at most 2^40): associative, so the LDS
//     histograms may use integer atomics and no sum depends on an order.  A weight is off by at most 2^-41 of the largest one.
// The two thresholds are found by a radix select over the keys, 8 bits per pass and 256 bins: per bin a count (top-k) or a mass (top-p);
// the bins are walked from the top to the one where the count reaches k, resp. the mass reaches top_p * total, and the next pass descends
// into it.  Four passes fix a threshold exactly; ties with it are all kept.  The draw is a prefix sum of the kept masses in index order.
#include "common.h"
#include "vitamd_internal.h"
#include "../../include/vitamd.h"

namespace {

typedef unsigned long long u64;

constexpr int MAX_V = VITAMD_SAMPLE_MAX_V;
constexpr int LDS_ROW_MAX_V = 32768;       // the row stays in LDS up to here (128 KiB); longer rows are re-read through L2
constexpr int REP = 8;                     // copies of each histogram bin, picked by lane: logits crowd into few exponent bins on the first pass
constexpr unsigned KEY_NINF = 0x007fffffu; // key(-inf): everything finite is above it
constexpr int HIST = REP * 257;
constexpr float FIX_ONE = 1099511627776.f; // 2^40

// order-preserving image: a < b  <=>  key(a) < key(b) (-0 is folded into +0 first)
__device__ __forceinline__ unsigned key(float x) {
  const unsigned b = __builtin_bit_cast(unsigned, x + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unkey(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// fixed-point softmax weight; the ONE expression every pass uses
__device__ __forceinline__ u64 mass(float x, float xmax, float c) {
  if (x == -__builtin_inff()) return 0;
  const u64 m = (u64)__builtin_rintf(__builtin_amdgcn_exp2f((x - xmax) * c) * FIX_ONE);
  return m ? m : 1;
}

// v + (the DPP-selected lane's v, or 0 where the control selects none): both halves moved by the same control, then one 64-bit add
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 dpp_add(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROW_MASK, 0xf, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xf, true);
  return v + (((u64)hi << 32) | lo);
}
// inclusive prefix sum over the 64 lanes (all active) in registers: shifts by 1, 2, 4, 8 inside each row of 16 lanes, then lane 15 of
// rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3.  A __shfl_up chain costs twelve dependent LDS round trips per 64-bit scan.
__device__ __forceinline__ u64 wave_incl_scan(u64 v) {
  v = dpp_add<0x111, 0xf>(v);     // row_shr:1
  v = dpp_add<0x112, 0xf>(v);     // row_shr:2
  v = dpp_add<0x114, 0xf>(v);     // row_shr:4
  v = dpp_add<0x118, 0xf>(v);     // row_shr:8
  v = dpp_add<0x142, 0xa>(v);     // row_bcast:15 -> rows 1, 3
  v = dpp_add<0x143, 0xc>(v);     // row_bcast:31 -> rows 2, 3
  return v;
}
__device__ __forceinline__ u64 wave_last(u64 v) {
  return ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Philox4x32-10 (common.h), first output word
__device__ __forceinline__ unsigned philox_first(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
  return philox4x32_10(c0, c1, c2, c3, k0, k1)[0];
}

struct SampleArgs {
  const float* logits;
  long long* token;
  float* info;              // [B, 4] or null
  const float* u;           // [B] or null (Philox)
  const u64* step;          // device counter or null (= 0)
  int V, ld, top_k;
  float c;                  // log2(e) / temperature
  float top_p;
  u64 seed;
};

struct Shared {
  u64 hist[HIST];           // [copy][bin], 257 bins apart: a bin's copies lie on different banks, a copy's bins side by side
  u64 wsum[16];
  u64 wall[16];
  unsigned wcnt[16];
  unsigned wmin[16];
  u64 sel_rem;
  int sel_bin;
};

// One radix pass over the elements whose key matches `prefix` above bit shift + 8 and is >= lo: histogram of bits shift .. shift+7
// (counts, or masses when MASS), then the bin, from the top, where the running sum reaches the target.  first: a MASS pass derives the
// target from the total, ceil(top_p * total).  Returns false when the total is below the target (fewer finite logits than k).
template <int NT, bool MASS>
__device__ __forceinline__ bool radix_pass(Shared& sh, const float* row, const SampleArgs& p, float xmax, int shift, unsigned prefix, unsigned lo,
                                           bool first, u64& target, unsigned& bin_out) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int rep = lane & (REP - 1);              // the histogram is zero on entry: the kernel's prologue and every pass's readers clear it
  for (int i = tid; i < p.V; i += NT) {
    const float x = row[i];
    const unsigned k = key(x);
    if (k >= lo && (shift == 24 || (k >> (shift + 8)) == prefix)) {
      const int slot = rep * 257 + (int)((k >> shift) & 255u);
      if constexpr (MASS) atomicAdd(&sh.hist[slot], mass(x, xmax, p.c));
      else atomicAdd(&sh.hist[slot], (u64)1);
    }
  }
  __syncthreads();
  u64 v = 0, incl = 0;
  if (tid < 256) {                          // thread t owns bin 255 - t: a prefix scan over t walks the bins from the top
#pragma unroll
    for (int r = 0; r < REP; ++r) {
      v += sh.hist[r * 257 + 255 - tid];
      sh.hist[r * 257 + 255 - tid] = 0;
    }
    incl = wave_incl_scan(v);
    if (lane == 63) sh.wsum[w] = incl;
  }
  __syncthreads();
  const u64 s0 = sh.wsum[0], s1 = sh.wsum[1], s2 = sh.wsum[2], s3 = sh.wsum[3];
  const u64 total = s0 + s1 + s2 + s3;
  if (first) {
    if constexpr (MASS) {
      u64 t = (u64)__builtin_ceil((double)p.top_p * (double)total);
      target = t < 1 ? 1 : (t > total ? total : t);
    }
  }
  if (total < target) {                      // uniform; only a first count pass can get here: fewer finite logits than k
    __syncthreads();                         // wsum is rewritten by what follows
    return false;
  }
  if (tid < 256) {
    incl += (w > 0 ? s0 : 0) + (w > 1 ? s1 : 0) + (w > 2 ? s2 : 0);
    if (incl >= target && incl - v < target) {
      sh.sel_bin = 255 - tid;
      sh.sel_rem = target - (incl - v);
    }
  }
  __syncthreads();
  bin_out = (unsigned)sh.sel_bin;
  target = sh.sel_rem;
  return true;
}

template <int NT, bool LDSROW>
__global__ __launch_bounds__(NT) void sample_kernel(const SampleArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ Shared sh;
  constexpr int NW = NT / 64;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x, V = p.V;
  const float* xg = p.logits + (size_t)b * p.ld;
  const float* row = LDSROW ? (const float*)smem : xg;

  // ---- pass 0: the row into LDS, its maximum
  unsigned kmax = 0;
  for (int i = tid; i < HIST; i += NT) sh.hist[i] = 0;
  for (int i = tid; i < V; i += NT) {
    const float x = xg[i];
    if constexpr (LDSROW) ((float*)smem)[i] = x;
    kmax = max(kmax, key(x));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
  if (lane == 0) sh.wmin[w] = kmax;
  __syncthreads();
  kmax = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) kmax = max(kmax, sh.wmin[i]);
  const float xmax = unkey(kmax);
  __syncthreads();                          // wmin is written again below

  // ---- top-k, then top-p over what it kept: thr = the smallest kept key
  unsigned thr = KEY_NINF + 1;              // -inf is never kept
  if (p.top_k > 0) {
    u64 target = (u64)p.top_k;
    unsigned prefix = 0, bin = 0;
    bool ok = true;
#pragma unroll 1
    for (int shift = 24; shift >= 0 && ok; shift -= 8) {
      ok = radix_pass<NT, false>(sh, row, p, xmax, shift, prefix, KEY_NINF + 1, shift == 24, target, bin);
      prefix = (prefix << 8) | bin;
    }
    if (ok) thr = max(prefix, KEY_NINF + 1);
  }
  if (p.top_p < 1.f) {
    u64 target = 0;
    unsigned prefix = 0, bin = 0;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
      radix_pass<NT, true>(sh, row, p, xmax, shift, prefix, thr, shift == 24, target, bin);   // always finds: 1 <= target <= total
      prefix = (prefix << 8) | bin;
    }
    thr = max(prefix, thr);
  }

  // ---- draw.  Wave w owns the indices [w * seg, (w + 1) * seg): kept mass per wave, the wave where the running sum passes u * kept
  // mass, then that wave alone scans its segment 64 indices at a time.
  const int seg = ((V + NW - 1) / NW + 63) & ~63;
  const int i0 = w * seg, i1 = min(V, i0 + seg);
  u64 ms = 0, mall = 0;
  unsigned cnt = 0, kmin = 0xffffffffu;
  for (int i = i0 + lane; i < i1; i += 64) {
    const float x = row[i];
    const unsigned k = key(x);
    const u64 m = mass(x, xmax, p.c);
    mall += m;
    if (k >= thr) { ms += m; ++cnt; kmin = min(kmin, k); }
  }
  ms = wave_sum_u64(ms);
  mall = wave_sum_u64(mall);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += (unsigned)__shfl_xor((int)cnt, o, 64);
    kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64));
  }
  if (lane == 0) { sh.wsum[w] = ms; sh.wall[w] = mall; sh.wcnt[w] = cnt; sh.wmin[w] = kmin; }
  __syncthreads();
  u64 kept = 0, all = 0;
  cnt = 0; kmin = 0xffffffffu;
#pragma unroll
  for (int i = 0; i < NW; ++i) { kept += sh.wsum[i]; all += sh.wall[i]; cnt += sh.wcnt[i]; kmin = min(kmin, sh.wmin[i]); }
  float u;
  if (p.u) {
    u = p.u[b];
  } else {
    const u64 st = p.step ? *p.step : 0;
    u = (float)(philox_first((unsigned)b, 0u, (unsigned)st, (unsigned)(st >> 32), (unsigned)p.seed, (unsigned)(p.seed >> 32)) >> 8) * 0x1p-24f;
  }
  u = fminf(fmaxf(u, 0.f), 1.f);
  u64 ut = (u64)__builtin_floor((double)u * (double)kept);     // running > u * kept  <=>  running > floor(u * kept): the sums are integers
  if (ut >= kept) ut = kept - 1;                          // kept >= 2^40 (the maximum is always kept), so a crossing exists
  u64 run = 0;
  int wstar = NW - 1;
#pragma unroll
  for (int i = NW - 1; i >= 0; --i) {
    u64 before = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) before += j < i ? sh.wsum[j] : 0;
    if (before <= ut && before + sh.wsum[i] > ut) { wstar = i; run = before; }
  }
  if (w != wstar) return;
  for (int c = i0; c < i1; c += 64) {                     // wave-uniform trip count
    const int i = c + lane;
    u64 m = 0;
    if (i < i1) {
      const float x = row[i];
      if (key(x) >= thr) m = mass(x, xmax, p.c);
    }
    const u64 incl = wave_incl_scan(m);
    const unsigned long long hit = __ballot(run + incl > ut);
    if (hit) {
      if (lane == __builtin_ctzll(hit)) {
        p.token[b] = i;
        if (p.info) {
          float* o = p.info + (size_t)b * 4;
          o[0] = unkey(kmin);
          o[1] = (float)cnt;
          o[2] = (float)((double)kept / (double)all);
          o[3] = (float)((double)m / (double)kept);
        }
      }
      return;
    }
    run += wave_last(incl);
  }
}

template <int NT, bool LDSROW>
int launch_sample(const SampleArgs& p, int B, hipStream_t stream) {
  auto kern = sample_kernel<NT, LDSROW>;
  const int lds = LDSROW ? p.V * 4 : 0;
  if (lds > 32768)
    if (int e = set_lds(kern, lds)) return e;
  hipLaunchKernelGGL(kern, dim3(B), dim3(NT), lds, stream, p);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

}  // namespace

extern "C" int vitamd_sample_logits(const float* logits, long long* token, float* info, const float* u, const unsigned long long* step, int B,
                                    int V, int ld, float temperature, int top_k, float top_p, unsigned long long seed, void* stream) {
  if (B < 1 || V < 2 || V > MAX_V || ld < V) return VITAMD_ERR_SHAPE;
  if (!(temperature > 0.f) || !(temperature < __builtin_inff()) || top_k < 0 || !(top_p > 0.f) || !(top_p <= 1.f)) return VITAMD_ERR_ARG;
  if (!logits || !token) return VITAMD_ERR_ARG;
  SampleArgs p{logits, token, info, u, step, V, ld, top_k < V ? top_k : 0, 1.4426950408889634f / temperature, top_p, seed};
  hipStream_t s = (hipStream_t)stream;
  if (V > LDS_ROW_MAX_V) return launch_sample<1024, false>(p, B, s);
  if (V > 4096) return launch_sample<1024, true>(p, B, s);
  return launch_sample<256, true>(p, B, s);
}
