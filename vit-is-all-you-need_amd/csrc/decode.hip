// Kernels of KV-cached autoregressive decoding: the K/V append, single-query attention over the cache
// (flash-decoding split + deterministic combine), the skinny-M GEMM that streams a Linear's weights once across the chip, its QKV form
// that appends K/V from the epilogue, and the embedding of a decoded token at the device-resident position.
// The current length is read from a device int32 (never a host integer), so a decode step enqueues without host synchronisation;
// grids are sized from the cache capacity Lmax and work past the length exits early.
#include "common.h"
#include "vitamd_internal.h"
#include "gemm_nt_epilogue.h"
#include "../../include/vitamd.h"

namespace {

constexpr int DH = 64;              // head dim (the library's only one)
constexpr int MAX_LEN = VITAMD_DECODE_MAX_LEN;
constexpr float NEG_BIG = -1e30f;   // running max before the first key (finite: exp2 of a difference of two of these is 1, never NaN)

int dec_cus() {
  static int cus[16] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return 256; }
  if (!cus[dev]) {
    int n = 0;
    cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cus[dev];
}

__device__ __forceinline__ void unpack8(const u32x4& v, float (&f)[8]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) { f[2 * c] = bf16lo(v[c]); f[2 * c + 1] = bf16hi(v[c]); }
}

// ------------------------------------------------------------------------------------------------ a. K/V append
// one thread per 16-B piece (b, t, h, k|v, segment of 8 elements): qkv row b*T+t, columns (1|2)*D + h*64 + 8*seg -> cache row *len + t
__global__ __launch_bounds__(256) void kv_append_kernel(const __bf16* __restrict__ qkv, __bf16* __restrict__ kc, __bf16* __restrict__ vc,
                                                       const int* __restrict__ len, int B, int T, int H, int Lmax) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * T * H * 16) return;
  const int seg = (int)(i & 7), kv = (int)((i >> 3) & 1);
  long r = i >> 4;
  const int h = (int)(r % H);
  r /= H;
  const int t = (int)(r % T), b = (int)(r / T);
  const int pos = *len + t;
  if (pos < 0 || pos >= Lmax) return;                 // the binding refuses len + T > Lmax; never write outside the cache
  const int D = H * DH;
  const u32x4 v = *(const u32x4*)(qkv + (size_t)(b * T + t) * 3 * D + (1 + kv) * D + h * DH + seg * 8);
  *(u32x4*)((kv ? vc : kc) + (((size_t)b * H + h) * Lmax + pos) * DH + seg * 8) = v;
}

// ------------------------------------------------------------------------------------------------ b. decode attention
// Split of the keys: chunks of `chunk` keys (a multiple of 128), about 4 workgroups per CU at full length (B*H workgroups alone leave
// most CUs idle at batch 1-4, and 1.5 rounds of 256 CUs at B*H = 384).  nch == 1: the workgroup normalises and writes o itself.
struct DecPlan { int chunk, nch; };
DecPlan dec_plan(int B, int H, int Lmax) {
  const int bh = B * H, target = 4 * dec_cus();
  int nch = (target + bh - 1) / bh;
  const int maxch = (Lmax + 127) / 128;
  nch = nch < 1 ? 1 : (nch > maxch ? maxch : nch);
  const int chunk = ((Lmax + nch - 1) / nch + 127) / 128 * 128;
  return {chunk, (Lmax + chunk - 1) / chunk};
}
long dec_ws_bytes(const DecPlan& pl, int B, int H) { return pl.nch > 1 ? (long)B * H * pl.nch * (DH + 2) * 4 : 0; }

// Workgroup (chunk c, b*H + h), 4 waves.  Lane = 8 key slots x 8 segments: a wave-instruction reads 8 whole 128-B key rows straight into
// VGPRs (no LDS), U = 4 of them per K and per V in flight per lane.  Each slot keeps its own online softmax (fp32, base-2 exponent with
// scale 1/8 * log2 e folded into q); slots, then waves, are merged in a fixed order.  Keys past *len + 1 are masked (p = 0).
template <bool SPLIT>
__global__ __launch_bounds__(256) void decode_attn_kernel(const __bf16* __restrict__ qkv, const __bf16* __restrict__ kc,
                                                         const __bf16* __restrict__ vc, __bf16* __restrict__ o, const int* __restrict__ len,
                                                         int H, int Lmax, int chunk, int nch, float* __restrict__ ws) {
  __shared__ float red[4][8][DH / 8 + 2];
  const int c = blockIdx.x, bh = blockIdx.y;
  const int n = *len + 1;                              // keys 0 .. *len: the query's own K/V were appended at *len
  const int k0 = c * chunk;
  if (k0 >= n) return;                                 // whole workgroup: past the current length
  const int k1 = min(min(k0 + chunk, n), Lmax);
  const int b = bh / H, h = bh - b * H, D = H * DH;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, slot = lane >> 3, seg = lane & 7;
  float q[8];
  unpack8(*(const u32x4*)(qkv + (size_t)b * 3 * D + h * DH + seg * 8), q);
  constexpr float QS = 0.125f * 1.4426950408889634f;
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] *= QS;
  const __bf16* kb = kc + (size_t)bh * Lmax * DH + seg * 8;
  const __bf16* vb = vc + (size_t)bh * Lmax * DH + seg * 8;
  float m = NEG_BIG, l = 0.f, acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  constexpr int U = 4;
  for (int base = k0 + w * 8 * U; base < k1; base += 4 * 8 * U) {     // wave-uniform trip count
    u32x4 kr[U], vr[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = base + u * 8 + slot;
      ok[u] = key < k1;
      kr[u] = ok[u] ? *(const u32x4*)(kb + (size_t)key * DH) : (u32x4){0u, 0u, 0u, 0u};
      vr[u] = ok[u] ? *(const u32x4*)(vb + (size_t)key * DH) : (u32x4){0u, 0u, 0u, 0u};
    }
    float s[U], mx = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8], d = 0.f;
      unpack8(kr[u], kf);
#pragma unroll
      for (int j = 0; j < 8; ++j) d = fmaf(q[j], kf[j], d);
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      d += __shfl_xor(d, 4);
      s[u] = ok[u] ? d : NEG_BIG;
      mx = fmaxf(mx, s[u]);
    }
    const float sc = exp2f(m - mx);
    l *= sc;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= sc;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = ok[u] ? exp2f(s[u] - mx) : 0.f;
      float vf[8];
      unpack8(vr[u], vf);
      l += p;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(p, vf[j], acc[j]);
    }
    m = mx;
  }
  // merge the 8 slots of each segment (lanes seg, seg+8, ..., seg+56)
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
    const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off);
    const float mm = fmaxf(m, m2), a = exp2f(m - mm), a2 = exp2f(m2 - mm);
    l = l * a + l2 * a2;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] * a + __shfl_xor(acc[j], off) * a2;
    m = mm;
  }
  if (slot == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[w][seg][j] = acc[j];
    red[w][seg][8] = m;
    red[w][seg][9] = l;
  }
  __syncthreads();
  if (threadIdx.x >= 8) return;
  float mm = NEG_BIG;
#pragma unroll
  for (int ww = 0; ww < 4; ++ww) mm = fmaxf(mm, red[ww][seg][8]);
  float L = 0.f, A[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) A[j] = 0.f;
#pragma unroll
  for (int ww = 0; ww < 4; ++ww) {
    const float a = exp2f(red[ww][seg][8] - mm);
    L += red[ww][seg][9] * a;
#pragma unroll
    for (int j = 0; j < 8; ++j) A[j] += red[ww][seg][j] * a;
  }
  if constexpr (SPLIT) {
    float* pa = ws + ((size_t)bh * nch + c) * DH + seg * 8;
    *(f32x4*)pa = (f32x4){A[0], A[1], A[2], A[3]};
    *(f32x4*)(pa + 4) = (f32x4){A[4], A[5], A[6], A[7]};
    if (seg == 0) {
      float* pm = ws + (size_t)gridDim.y * nch * DH + ((size_t)bh * nch + c) * 2;
      pm[0] = mm;
      pm[1] = L;
    }
  } else {
    const float r = 1.f / L;
    const u32x4 ov = {pack_bf16x2(A[0] * r, A[1] * r), pack_bf16x2(A[2] * r, A[3] * r), pack_bf16x2(A[4] * r, A[5] * r),
                      pack_bf16x2(A[6] * r, A[7] * r)};
    *(u32x4*)(o + (size_t)b * D + h * DH + seg * 8) = ov;
  }
}

// one wave per (b, h), lane = output dim: the chunk partials below the current length, merged in chunk order (deterministic)
__global__ __launch_bounds__(64) void decode_attn_combine_kernel(__bf16* __restrict__ o, const int* __restrict__ len, int H, int chunk, int nch,
                                                                const float* __restrict__ ws) {
  const int bh = blockIdx.x, d = threadIdx.x;
  const int n = *len + 1;
  const int nv = min((n + chunk - 1) / chunk, nch);
  if (nv <= 0) return;                                // *len < 0: no chunk lies below the length, o stays as it is (as in the unsplit form)
  const float* pm = ws + (size_t)gridDim.x * nch * DH + (size_t)bh * nch * 2;
  const float* pa = ws + (size_t)bh * nch * DH + d;
  float mm = NEG_BIG;
  for (int c = 0; c < nv; ++c) mm = fmaxf(mm, pm[2 * c]);
  float L = 0.f, A = 0.f;
  for (int c = 0; c < nv; ++c) {
    const float a = exp2f(pm[2 * c] - mm);
    L += pm[2 * c + 1] * a;
    A += pa[(size_t)c * DH] * a;
  }
  const int b = bh / H, h = bh - b * H;
  o[(size_t)b * H * DH + h * DH + d] = f2bf(A / L);
}

// ------------------------------------------------------------------------------------------------ a2. decoded-token embedding
// x[b, :] = tok[token[b], :] + pos[*len, :], one thread per 4 columns.  A token or a position outside its table: the row is left alone.
__global__ __launch_bounds__(256) void decode_embed_kernel(const float* __restrict__ tok, const float* __restrict__ pos,
                                                          const long long* __restrict__ token, const int* __restrict__ len,
                                                          float* __restrict__ x, int B, int D, int tok_rows, int pos_rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int dq = D / 4;
  if (i >= B * dq) return;
  const int b = i / dq, c = (i - b * dq) * 4;
  const long long t = token[b];
  const int l = *len;
  if (t < 0 || t >= tok_rows || l < 0 || l >= pos_rows) return;
  const f32x4 a = *(const f32x4*)(tok + (size_t)t * D + c);
  const f32x4 e = *(const f32x4*)(pos + (size_t)l * D + c);
  *(f32x4*)(x + (size_t)b * D + c) = a + e;
}

// ------------------------------------------------------------------------------------------------ c. skinny-M GEMM
// out = epi(A[M,K] . W[N,K]^T), 1 <= M <= 64.  Workgroup = 64 output columns (4 waves x 16) x one K range of `ks`; the A slice is staged
// in LDS once per workgroup (rows padded with zeros to 16*MT, 16-B row pad), each wave streams its 16 weight rows straight into VGPRs
// (lane = row n0 + lane%16, 32 contiguous bytes per 64-K step; U = 4 steps in flight) and runs 16x16x32 MFMAs with W as the first
// operand, so a lane ends up holding 4 consecutive columns of one row.  The K permutation (k-group g of a lane covers g*16 .. g*16+15
// of each 64-K step) is the same for both operands, so the sum is unchanged.
struct SkinnyArgs {
  const __bf16* A;
  const __bf16* W;
  void* out;
  void* out2;
  const float* bias;
  const float* aux;
  float* ws;                 // [splits][M][N] fp32 partials (splits > 1)
  const unsigned* gelu_tab;
  int M, N, K, ks, splits;
  __bf16* kc;                // EPI_QKV_APPEND only: k / v cache [M][H][Lmax][64], the device length, H and Lmax
  __bf16* vc;
  const int* len;
  int H, Lmax;
};
constexpr int EPI_QKV_APPEND = 100;     // internal: EPI_BIAS_BF16 whose K and V column ranges also go to row *len of the caches
struct SkinnyPlan { int splits, ks; };
// split K until the N tiles cover the CUs, keeping >= 128 K per split and the LDS image of A under ~65 KiB (ks <= 512)
SkinnyPlan skinny_plan(int M, int N, int K) {
  (void)M;
  const int tn = (N + 63) / 64;
  int splits = (dec_cus() + tn - 1) / tn;
  const int lo = (K + 511) / 512, hi = K / 128 > 0 ? K / 128 : 1;
  splits = splits < lo ? lo : (splits > hi ? hi : splits);
  if (splits < 1) splits = 1;
  const int ks = ((K + splits - 1) / splits + 63) / 64 * 64;
  return {(K + ks - 1) / ks, ks};
}
long skinny_ws_bytes(const SkinnyPlan& pl, int M, int N) { return pl.splits > 1 ? (long)pl.splits * M * N * 4 : 0; }

// the epilogue on 4 consecutive columns n..n+3 of row m (semantics of gemm_nt_epilogue.h, plus a bias on the fp32 form)
template <int EPI>
__device__ __forceinline__ void skinny_store(const SkinnyArgs& p, int m, int n, f32x4 v) {
  if (p.bias) {
    const f32x4 b = *(const f32x4*)(p.bias + n);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += round_bf16(b[r]);       // autocast casts the bias to bf16
  }
  const size_t at = (size_t)m * p.N + n;
  if constexpr (EPI == EPI_BIAS_BF16) {
    *(u32x2*)((__bf16*)p.out + at) = (u32x2){pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
  } else if constexpr (EPI == EPI_QKV_APPEND) {
    const u32x2 pk = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    *(u32x2*)((__bf16*)p.out + at) = pk;
    const int D = p.H * DH, which = n / D;              // 0 = q, 1 = k, 2 = v; n % 4 == 0 and D % 64 == 0: the 4 columns share a head
    const int pos = *p.len;
    if (which >= 1 && pos >= 0 && pos < p.Lmax) {       // kv_append_kernel's guard: never write outside the cache
      const int c = n - which * D, h = c / DH, d = c - h * DH;
      *(u32x2*)((which == 1 ? p.kc : p.vc) + (((size_t)m * p.H + h) * p.Lmax + pos) * DH + d) = pk;
    }
  } else if constexpr (EPI == EPI_GELU) {
    const u32x2 pz = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    u32x2 g, unused = pz;
    gelu_lookup<u32x2>(pz, (const char*)p.gelu_tab, false, g, unused);
    *(u32x2*)((__bf16*)p.out + at) = pz;
    *(u32x2*)((__bf16*)p.out2 + at) = g;
  } else if constexpr (EPI == EPI_RESID_F32) {
    const f32x4 res = *(const f32x4*)(p.aux + at);
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = res[r] + round_bf16(v[r]);
    *(f32x4*)((float*)p.out + at) = o;
  } else {
    *(f32x4*)((float*)p.out + at) = v;
  }
}

template <int MT, int EPI, bool SPLIT>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const SkinnyArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* As = (__bf16*)smem;
  const int kb = blockIdx.y * p.ks;
  const int kl = min(p.ks, p.K - kb);                 // > 0: splits = ceil(K / ks)
  const int lda = p.ks + 8;
  const int per_row = kl / 8;
  for (int i = threadIdx.x; i < MT * 16 * per_row; i += 256) {
    const int r = i / per_row, c = (i - r * per_row) * 8;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (r < p.M) v = *(const u32x4*)(p.A + (size_t)r * p.K + kb + c);
    *(u32x4*)(As + r * lda + c) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 64 + w * 16;
  if (n0 >= p.N) return;                              // no barrier below
  const int g = lane >> 4, nrow = min(n0 + (lane & 15), p.N - 1);     // rows past N read row N-1; their columns are not stored
  const __bf16* wp = p.W + (size_t)nrow * p.K + kb + g * 16;
  const __bf16* ap = As + (lane & 15) * lda + g * 16;
  f32x4 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nsteps = kl / 64;
  constexpr int U = 4;
  for (int s = 0; s < nsteps; s += U) {
    u32x4 wr[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s + u < nsteps) {
        wr[u][0] = *(const u32x4*)(wp + (s + u) * 64);
        wr[u][1] = *(const u32x4*)(wp + (s + u) * 64 + 8);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s + u < nsteps) {                           // wave-uniform
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bf16x8 bw = __builtin_bit_cast(bf16x8, wr[u][j]);
#pragma unroll
          for (int i = 0; i < MT; ++i) {
            const bf16x8 af = *(const bf16x8*)(ap + i * 16 * lda + (s + u) * 64 + j * 8);
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw, af, acc[i], 0, 0, 0);
          }
        }
      }
    }
  }
  const int n = n0 + 4 * g;
  if (n >= p.N) return;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = i * 16 + (lane & 15);
    if (m >= p.M) continue;
    if constexpr (SPLIT) *(f32x4*)(p.ws + ((size_t)blockIdx.y * p.M + m) * p.N + n) = acc[i];
    else skinny_store<EPI>(p, m, n, acc[i]);
  }
}

// split-K partials summed in split order (bit-reproducible), then the epilogue; one thread per 4 columns of a row
template <int EPI>
__global__ __launch_bounds__(256) void gemm_skinny_reduce_kernel(const SkinnyArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int nq = p.N / 4;
  if (i >= p.M * nq) return;
  const int m = i / nq, n = (i - m * nq) * 4;
  f32x4 v = *(const f32x4*)(p.ws + (size_t)m * p.N + n);
  for (int s = 1; s < p.splits; ++s) v += *(const f32x4*)(p.ws + ((size_t)s * p.M + m) * p.N + n);
  skinny_store<EPI>(p, m, n, v);
}

template <int MT, int EPI>
int launch_skinny(const SkinnyArgs& p, hipStream_t stream) {
  const int lds = MT * 16 * (p.ks + 8) * 2;
  const dim3 grid((p.N + 63) / 64, p.splits);
  if (p.splits > 1) {
    auto kern = gemm_skinny_kernel<MT, EPI, true>;
    if (int e = set_lds(kern, lds)) return e;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, p);
    hipLaunchKernelGGL(gemm_skinny_reduce_kernel<EPI>, dim3((p.M * (p.N / 4) + 255) / 256), dim3(256), 0, stream, p);
  } else {
    auto kern = gemm_skinny_kernel<MT, EPI, false>;
    if (int e = set_lds(kern, lds)) return e;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, p);
  }
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

template <int EPI>
int launch_skinny_mt(const SkinnyArgs& p, hipStream_t stream) {
  switch ((p.M + 15) / 16) {
    case 1: return launch_skinny<1, EPI>(p, stream);
    case 2: return launch_skinny<2, EPI>(p, stream);
    case 3: return launch_skinny<3, EPI>(p, stream);
    default: return launch_skinny<4, EPI>(p, stream);
  }
}

}  // namespace

extern "C" int vitamd_kv_append(const void* qkv, void* k_cache, void* v_cache, const int* len, int B, int T, int H, int head_dim, int Lmax,
                                void* stream) {
  if (!qkv || !k_cache || !v_cache || !len) return VITAMD_ERR_ARG;
  if (head_dim != DH || B <= 0 || T <= 0 || H <= 0 || Lmax <= 0 || Lmax > MAX_LEN || T > Lmax) return VITAMD_ERR_SHAPE;
  const long threads = (long)B * T * H * 16;
  hipLaunchKernelGGL(kv_append_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const __bf16*)qkv,
                     (__bf16*)k_cache, (__bf16*)v_cache, len, B, T, H, Lmax);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" long vitamd_decode_attention_ws_bytes(int B, int H, int Lmax) {
  if (B <= 0 || H <= 0 || Lmax <= 0 || Lmax > MAX_LEN) return -VITAMD_ERR_SHAPE;
  return dec_ws_bytes(dec_plan(B, H, Lmax), B, H);
}

extern "C" int vitamd_decode_attention(const void* qkv, const void* k_cache, const void* v_cache, void* o, const int* len, int B, int H,
                                       int head_dim, int Lmax, float* ws, long ws_bytes, void* stream) {
  if (!qkv || !k_cache || !v_cache || !o || !len) return VITAMD_ERR_ARG;
  if (head_dim != DH || B <= 0 || H <= 0 || Lmax <= 0 || Lmax > MAX_LEN || (long)B * H > 65535) return VITAMD_ERR_SHAPE;
  const DecPlan pl = dec_plan(B, H, Lmax);
  const long need = dec_ws_bytes(pl, B, H);
  if (need > 0 && (!ws || ws_bytes < need)) return VITAMD_ERR_ARG;
  const dim3 grid(pl.nch, B * H);
  hipStream_t s = (hipStream_t)stream;
  if (pl.nch > 1) {
    hipLaunchKernelGGL(decode_attn_kernel<true>, grid, dim3(256), 0, s, (const __bf16*)qkv, (const __bf16*)k_cache, (const __bf16*)v_cache,
                       (__bf16*)o, len, H, Lmax, pl.chunk, pl.nch, ws);
    hipLaunchKernelGGL(decode_attn_combine_kernel, dim3(B * H), dim3(64), 0, s, (__bf16*)o, len, H, pl.chunk, pl.nch, (const float*)ws);
  } else {
    hipLaunchKernelGGL(decode_attn_kernel<false>, grid, dim3(256), 0, s, (const __bf16*)qkv, (const __bf16*)k_cache, (const __bf16*)v_cache,
                       (__bf16*)o, len, H, Lmax, pl.chunk, pl.nch, ws);
  }
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

static bool skinny_shape_ok(int M, int N, int K) { return M >= 1 && M <= 64 && N >= 4 && N % 4 == 0 && K >= 64 && K % 64 == 0; }

extern "C" long vitamd_gemm_skinny_ws_bytes(int M, int N, int K) {
  if (!skinny_shape_ok(M, N, K)) return -VITAMD_ERR_SHAPE;
  return skinny_ws_bytes(skinny_plan(M, N, K), M, N);
}

extern "C" int vitamd_gemm_skinny_bf16(const void* A, const void* W, void* out, void* out2, const float* bias, const float* aux, int M, int N,
                                       int K, int epi, float* ws, long ws_bytes, void* stream) {
  if (!A || !W || !out) return VITAMD_ERR_ARG;
  if (epi != EPI_BIAS_BF16 && epi != EPI_GELU && epi != EPI_RESID_F32 && epi != EPI_F32) return VITAMD_ERR_ARG;
  if ((epi == EPI_GELU && !out2) || (epi == EPI_RESID_F32 && !aux)) return VITAMD_ERR_ARG;
  if (!skinny_shape_ok(M, N, K)) return VITAMD_ERR_SHAPE;
  const SkinnyPlan pl = skinny_plan(M, N, K);
  const long need = skinny_ws_bytes(pl, M, N);
  if (need > 0 && (!ws || ws_bytes < need)) return VITAMD_ERR_ARG;
  SkinnyArgs p{(const __bf16*)A, (const __bf16*)W, out, out2, bias, aux, ws, nullptr, M, N, K, pl.ks, pl.splits, nullptr, nullptr, nullptr, 0, 0};
  if (epi == EPI_GELU) {
    p.gelu_tab = vitamd_gelu_table();
    if (!p.gelu_tab) return VITAMD_ERR_INIT;
  }
  hipStream_t s = (hipStream_t)stream;
  switch (epi) {
    case EPI_BIAS_BF16: return launch_skinny_mt<EPI_BIAS_BF16>(p, s);
    case EPI_GELU: return launch_skinny_mt<EPI_GELU>(p, s);
    case EPI_RESID_F32: return launch_skinny_mt<EPI_RESID_F32>(p, s);
    default: return launch_skinny_mt<EPI_F32>(p, s);
  }
}

extern "C" int vitamd_gemm_skinny_qkv_append(const void* A, const void* W, void* qkv, const float* bias, void* k_cache, void* v_cache,
                                             const int* len, int M, int H, int K, int head_dim, int Lmax, float* ws, long ws_bytes,
                                             void* stream) {
  if (!A || !W || !qkv || !k_cache || !v_cache || !len) return VITAMD_ERR_ARG;
  if (head_dim != DH || H <= 0 || H > 1024 || Lmax <= 0 || Lmax > MAX_LEN) return VITAMD_ERR_SHAPE;
  const int N = 3 * H * DH;
  if (!skinny_shape_ok(M, N, K)) return VITAMD_ERR_SHAPE;
  const SkinnyPlan pl = skinny_plan(M, N, K);
  const long need = skinny_ws_bytes(pl, M, N);
  if (need > 0 && (!ws || ws_bytes < need)) return VITAMD_ERR_ARG;
  const SkinnyArgs p{(const __bf16*)A, (const __bf16*)W, qkv, nullptr, bias, nullptr, ws, nullptr, M, N, K, pl.ks, pl.splits,
                     (__bf16*)k_cache, (__bf16*)v_cache, len, H, Lmax};
  return launch_skinny_mt<EPI_QKV_APPEND>(p, (hipStream_t)stream);
}

extern "C" int vitamd_decode_embed(const float* tok_table, const float* pos_table, const long long* token, const int* len, float* x, int B,
                                   int D, int tok_rows, int pos_rows, void* stream) {
  if (!tok_table || !pos_table || !token || !len || !x) return VITAMD_ERR_ARG;
  if (B <= 0 || D < 4 || D % 4 != 0 || tok_rows <= 0 || pos_rows <= 0 || (long)B * (D / 4) > 0x7fffffffL) return VITAMD_ERR_SHAPE;
  const long threads = (long)B * (D / 4);
  hipLaunchKernelGGL(decode_embed_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tok_table, pos_table,
                     token, len, x, B, D, tok_rows, pos_rows);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
