// Training of the two image tokenizers: the cosine-similarity VQ quantiser of train_titok.Quantizer, forward and
// backward, and the reconstruction loss mse_loss(pixel_shuffle(tokens), images) taken on the tokens as the head GEMM wrote them, forward
// and backward.  The two halves share the final fixed-order sum and nothing else.
//
// Quantiser.  All arithmetic is fp32.  u = x / max(|x|, eps) and e^_k = e_k / max(|e_k|, eps), both norms summed over ascending c;
// the unit codebook is staged once per call in the workspace.  The search is vq_nearest's (csrc/misc.hip): one thread per row, 256 codes
// per workgroup in LDS, sum over ascending c of (u_c - e^_kc)^2, strict <, and (distance bits << 32 | index) folded into the row's slot
// of the index buffer by a 64-bit atomicMin - the first minimum whatever order the chunks arrive in.  A second pass gathers the RAW row,
// writes q = u + (p - u) and the row's sum of (p - u)^2; per-workgroup partials and one fixed-order sum give the loss: no float atomics,
// the same bits on every call.  The backward is one thread per row; rows of a workgroup that picked the same code are summed on chip in
// ascending row order before ONE fp32 atomic per (code, column) leaves the workgroup, so dcodebook depends on arrival order only where
// a code is shared between workgroups.
//
// Reconstruction loss.  A workgroup owns a strip of whole tokens of one grid row (b, gh): it stages them in LDS in 16-byte pieces, then
// walks the matching image rows (one run of contiguous floats per (channel, p1)) with 16-byte loads, reading the token element of each
// pixel from LDS.  The backward writes the gradient over the staged tokens in LDS and the strip back in 16-byte pieces, so it may run in
// place.  Columns between F and the row stride are never touched.
#include <type_traits>

#include "common.h"
#include "../../include/vitamd.h"

namespace {

constexpr float VQ_EPS = 1e-12f;              // F.normalize
constexpr float VQ_RNORM_CLAMPED = 1.0f / VQ_EPS;   // rnorm of a row whose norm was below eps: the backward's mark for dx = du / eps
constexpr int VQ_MAX_D = 64;
constexpr int RECON_LDS_BYTES = 48 * 1024;    // the staged strip; three workgroups per CU
constexpr int SUM_THREADS = 1024;

// out[0] = scale * sum(partials[0 .. n)), one workgroup: every thread sums its strided share in fp64, then lanes, then waves, in a fixed order
__global__ __launch_bounds__(SUM_THREADS) void sum_partials_kernel(const float* __restrict__ partials, float* __restrict__ out, long n, double scale) {
  __shared__ double part[SUM_THREADS / 64];
  double a = 0.0;
  for (long i = threadIdx.x; i < n; i += SUM_THREADS) a += (double)partials[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  a = 0.0;
  for (int i = 0; i < SUM_THREADS / 64; ++i) a += part[i];
  out[0] = (float)(a * scale);
}

// sum of the four waves' values in wave order, returned to thread 0 (red: 4 floats of LDS)
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------------ quantiser forward
// thread i: unit row i of the codebook (i < K) and the empty slot of row i of the packed index buffer (i < M)
__global__ __launch_bounds__(256) void vq_prepare_kernel(const float* __restrict__ e, float* __restrict__ eunit, unsigned long long* __restrict__ packed,
                                                         int M, int K, int d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < M) packed[i] = ~0ull;
  if (i >= K) return;
  const float* er = e + (size_t)i * d;
  float ss = 0.f;
  for (int c = 0; c < d; ++c) ss += er[c] * er[c];
  const float den = fmaxf(sqrtf(ss), VQ_EPS);
  for (int c = 0; c < d; ++c) eunit[(size_t)i * d + c] = er[c] / den;
}

// grid = (row blocks) x (256-code chunks).  Every workgroup normalises its rows again (d flops a row); chunk 0 writes unit and rnorm.
template <int DMAX>
__global__ __launch_bounds__(256) void vq_search_kernel(const float* __restrict__ x, const float* __restrict__ eunit, float* __restrict__ unit,
                                                        float* __restrict__ rnorm, unsigned long long* __restrict__ packed, int M, int K, int d) {
  __shared__ float ce[256 * DMAX];
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int k0 = blockIdx.y * 256, nk = min(256, K - k0);
  float xr[DMAX];
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < DMAX; ++c) {
    xr[c] = (m < M && c < d) ? x[(size_t)m * d + c] : 0.f;
    ss += xr[c] * xr[c];
  }
  const float nrm = sqrtf(ss);
  const float den = fmaxf(nrm, VQ_EPS);
#pragma unroll
  for (int c = 0; c < DMAX; ++c) xr[c] = xr[c] / den;
  if (blockIdx.y == 0 && m < M) {
#pragma unroll
    for (int c = 0; c < DMAX; ++c)
      if (c < d) unit[(size_t)m * d + c] = xr[c];
    // exactly 1 / eps is the mark of a clamped row; a norm of exactly eps keeps the projection form (torch's mask is norm >= eps)
    rnorm[m] = nrm < VQ_EPS ? VQ_RNORM_CLAMPED : fminf(1.0f / nrm, __builtin_bit_cast(float, __builtin_bit_cast(unsigned, VQ_RNORM_CLAMPED) - 1u));
  }
  for (int i = threadIdx.x; i < nk * d; i += 256) ce[(i / d) * DMAX + (i % d)] = eunit[(size_t)k0 * d + i];
  __syncthreads();
  float best = 3.0e38f;
  int besti = k0;
  for (int k = 0; k < nk; ++k) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DMAX; ++c) {
      if (c < d) { const float t = xr[c] - ce[k * DMAX + c]; s += t * t; }
    }
    if (s < best) { best = s; besti = k0 + k; }
  }
  if (m < M) atomicMin(packed + m, ((unsigned long long)__builtin_bit_cast(unsigned, best) << 32) | (unsigned)besti);
}

// idx = the low half of the packed word; q = u + (p - u) on the raw row p; partials[workgroup] = sum over its rows of (p - u)^2
__global__ __launch_bounds__(256) void vq_gather_kernel(const float* __restrict__ e, const float* __restrict__ unit, unsigned long long* __restrict__ packed,
                                                        float* __restrict__ q, float* __restrict__ partials, int M, int K, int d) {
  __shared__ float red[4];
  const int m = blockIdx.x * 256 + threadIdx.x;
  float a = 0.f;
  if (m < M) {
    unsigned long long id = packed[m] & 0xffffffffull;
    if (id >= (unsigned long long)K) id = 0;            // every distance NaN (a NaN input row): no slot was ever taken
    packed[m] = id;
    const float* p = e + (size_t)id * d;
    const float* u = unit + (size_t)m * d;
    for (int c = 0; c < d; ++c) {
      const float t = p[c] - u[c];
      q[(size_t)m * d + c] = u[c] + t;
      a += t * t;
    }
  }
  a = block_sum_256(a, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

// ------------------------------------------------------------------------------------------------ quantiser backward
// k_commit = 0.5 s / (M d), k_code = 2 s / (M d), s = *g_loss (0 when absent)
__global__ __launch_bounds__(256) void vq_bwd_kernel(const float* __restrict__ g_q, const float* __restrict__ g_loss, const float* __restrict__ unit,
                                                     const float* __restrict__ rnorm, const long long* __restrict__ idx, const float* __restrict__ e,
                                                     float* __restrict__ dx, float* __restrict__ dcode, int M, int K, int d, float inv_md) {
  __shared__ int ids[256];
  const int m = blockIdx.x * 256 + threadIdx.x;
  const float s = g_loss ? *g_loss : 0.f;
  const float k_commit = 0.5f * s * inv_md, k_code = 2.0f * s * inv_md;
  long long id64 = m < M ? idx[m] : -1;
  if (id64 < 0 || id64 >= K) id64 = -1;                            // an index outside the codebook adds nothing and reads nothing
  const int id = (int)id64;
  ids[threadIdx.x] = id;
  if (id >= 0) {
    const float* u = unit + (size_t)m * d;
    const float* p = e + (size_t)id * d;
    const float* g = g_q ? g_q + (size_t)m * d : nullptr;
    float dot = 0.f;
    for (int c = 0; c < d; ++c) {
      const float du = (g ? g[c] : 0.f) + k_commit * (u[c] - p[c]);
      dot += u[c] * du;
    }
    const float rn = rnorm[m];
    const bool clamped = rn == VQ_RNORM_CLAMPED;
    for (int c = 0; c < d; ++c) {
      const float du = (g ? g[c] : 0.f) + k_commit * (u[c] - p[c]);
      dx[(size_t)m * d + c] = clamped ? du / VQ_EPS : (du - u[c] * dot) * rn;
    }
  } else if (m < M) {
    for (int c = 0; c < d; ++c) dx[(size_t)m * d + c] = 0.f;
  }
  __syncthreads();
  if (id < 0 || dcode == nullptr) return;
  for (int j = 0; j < (int)threadIdx.x; ++j)
    if (ids[j] == id) return;                           // an earlier row of this workgroup leads this code
  const int row0 = blockIdx.x * 256;
  const float* p = e + (size_t)id * d;
  for (int c0 = 0; c0 < d; c0 += 16) {
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.f;
    for (int j = threadIdx.x; j < 256; ++j) {
      if (ids[j] != id) continue;
      const float* u = unit + (size_t)(row0 + j) * d;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c0 + c < d) acc[c] += p[c0 + c] - u[c0 + c];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (c0 + c < d) atomicAdd(dcode + (size_t)id * d + c0 + c, k_code * acc[c]);
  }
}

// ------------------------------------------------------------------------------------------------ reconstruction loss
// Strip s of the grid: (b, gh) = s / chunks, tokens gw0 .. gw0 + nt of that grid row.  LDS: the strip, compact ([token][F]), then 4 floats.
// Image items: VEC_IMG (p % 4 == 0, aligned image): 4 consecutive pixels of one image row, which lie in one token; else single pixels.
template <bool BF16>
__device__ __forceinline__ float lds_elem(const char* strip, int i) {
  if constexpr (BF16) return bf2f(((const __bf16*)strip)[i]);
  else return ((const float*)strip)[i];
}
template <bool BF16>
__device__ __forceinline__ void lds_store(char* strip, int i, float v) {
  if constexpr (BF16) ((__bf16*)strip)[i] = f2bf(v);
  else ((float*)strip)[i] = v;
}

template <bool BF16, bool BWD, bool VEC_IMG>
__global__ __launch_bounds__(256) void recon_mse_kernel(const void* y, const float* __restrict__ img, const float* __restrict__ grad_out, void* dy,
                                                        float* __restrict__ partials, int G, int p, int c, int ld, int ldo, int nt_max, int chunks,
                                                        float inv_e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = BF16 ? 2 : 4;
  constexpr int W = 16 / ES;                            // elements per 16-byte piece
  typedef typename std::conditional<BF16, __bf16, float>::type T;
  const int F = p * p * c;
  const long strip = blockIdx.x;
  const long bg = strip / chunks;                       // b * G + gh
  const int gw0 = (int)(strip - bg * chunks) * nt_max;
  const int nt = min(nt_max, G - gw0);
  const long b = bg / G;
  const int gh = (int)(bg - b * G);
  const size_t row0 = (size_t)bg * G + gw0;             // first token row of the strip
  char* strip_lds = smem;
  float* red = (float*)(smem + (size_t)nt_max * F * ES);   // F * ES is a multiple of 16

  const int ppr = F / W;                                // pieces per token
  const int npieces = nt * ppr;
  for (int i = threadIdx.x; i < npieces; i += 256) {
    const int t = i / ppr, j = i - t * ppr;
    *(u32x4*)(strip_lds + (size_t)i * 16) = *(const u32x4*)((const T*)y + (row0 + t) * (size_t)ld + (size_t)j * W);
  }
  __syncthreads();

  const int Wimg = G * p;
  const float* img_b = img + (size_t)b * c * Wimg * Wimg;
  const float scale = BWD ? 2.0f * (grad_out ? *grad_out : 1.f) * inv_e : 0.f;
  const int run = nt * p;                               // pixels of one image row inside the strip
  float a = 0.f;
  if constexpr (VEC_IMG) {
    const int qpr = run / 4;
    const int nitems = c * p * qpr;
    for (int i = threadIdx.x; i < nitems; i += 256) {
      const int r = i / qpr, xq = (i - r * qpr) * 4;    // r = ch * p + p1
      const int ch = r / p, p1 = r - ch * p;
      const int t = xq / p, p2 = xq - t * p;
      const f32x4 v = *(const f32x4*)(img_b + ((size_t)ch * Wimg + (size_t)gh * p + p1) * Wimg + (size_t)gw0 * p + xq);
      const int e0 = t * F + (p1 * p + p2) * c + ch;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float df = lds_elem<BF16>(strip_lds, e0 + k * c) - v[k];
        if constexpr (BWD) lds_store<BF16>(strip_lds, e0 + k * c, df * scale);
        else a += df * df;
      }
    }
  } else {
    const int nitems = c * p * run;
    for (int i = threadIdx.x; i < nitems; i += 256) {
      const int r = i / run, xp = i - r * run;
      const int ch = r / p, p1 = r - ch * p;
      const int t = xp / p, p2 = xp - t * p;
      const float v = img_b[((size_t)ch * Wimg + (size_t)gh * p + p1) * Wimg + (size_t)gw0 * p + xp];
      const int e0 = t * F + (p1 * p + p2) * c + ch;
      const float df = lds_elem<BF16>(strip_lds, e0) - v;
      if constexpr (BWD) lds_store<BF16>(strip_lds, e0, df * scale);
      else a += df * df;
    }
  }
  if constexpr (BWD) {
    __syncthreads();
    for (int i = threadIdx.x; i < npieces; i += 256) {
      const int t = i / ppr, j = i - t * ppr;
      *(u32x4*)((T*)dy + (row0 + t) * (size_t)ldo + (size_t)j * W) = *(const u32x4*)(strip_lds + (size_t)i * 16);
    }
  } else {
    a = block_sum_256(a, red);
    if (threadIdx.x == 0) partials[strip] = a;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct ReconPlan { int nt, chunks; long strips; size_t lds; };

// shape rules shared by the forward, the backward and the workspace query; false = VITAMD_ERR_SHAPE
inline bool recon_plan(int B, int G, int p, int c, int bf16, ReconPlan& pl) {
  if (B < 1 || G < 1 || p < 1 || c < 1) return false;
  const long F = (long)p * p * c;
  const int es = bf16 ? 2 : 4;
  if (F % (16 / es) != 0 || F * es > RECON_LDS_BYTES) return false;
  if ((long)G * p > 46340 || (long)B * G * G > 0x7fffffffL) return false;      // image plane and token rows within int
  pl.nt = (int)(RECON_LDS_BYTES / (F * es));
  if (pl.nt > G) pl.nt = G;
  pl.chunks = (G + pl.nt - 1) / pl.nt;
  pl.strips = (long)B * G * pl.chunks;
  if (pl.strips > 0x7fffffffL) return false;
  pl.lds = (size_t)pl.nt * F * es + 16;
  return true;
}

template <bool BF16, bool BWD, bool VEC_IMG>
int launch_recon_form(const ReconPlan& pl, const void* y, const float* img, const float* grad_out, void* dy, float* partials, int G, int p, int c,
                      int ld, int ldo, float inv_e, hipStream_t s) {
  if (int e = set_lds(recon_mse_kernel<BF16, BWD, VEC_IMG>, (int)pl.lds)) return e;
  hipLaunchKernelGGL((recon_mse_kernel<BF16, BWD, VEC_IMG>), dim3((unsigned)pl.strips), dim3(256), pl.lds, s, y, img, grad_out, dy, partials, G, p, c, ld,
                     ldo, pl.nt, pl.chunks, inv_e);
  return VITAMD_OK;
}

template <bool BF16, bool BWD>
int launch_recon(bool vec_img, const ReconPlan& pl, const void* y, const float* img, const float* grad_out, void* dy, float* partials, int G, int p,
                 int c, int ld, int ldo, float inv_e, hipStream_t s) {
  return vec_img ? launch_recon_form<BF16, BWD, true>(pl, y, img, grad_out, dy, partials, G, p, c, ld, ldo, inv_e, s)
                 : launch_recon_form<BF16, BWD, false>(pl, y, img, grad_out, dy, partials, G, p, c, ld, ldo, inv_e, s);
}

inline long vq_blocks(int M) { return ((long)M + 255) / 256; }

}  // namespace

extern "C" long vitamd_vq_quantize_ws_bytes(int M, int K, int d) {
  if (M < 1 || K < 1 || d < 1 || d > VQ_MAX_D) return -VITAMD_ERR_SHAPE;
  return ((long)K * d + vq_blocks(M)) * (long)sizeof(float);
}

extern "C" int vitamd_vq_quantize_fwd(const float* x, const float* codebook, float* unit, float* rnorm, float* q, long long* idx, float* loss,
                                      float* ws, int M, int K, int d, void* stream) {
  if (M < 1 || K < 1 || d < 1 || d > VQ_MAX_D || (long)M * d > 0x7fffffffL || (long)K * d > 0x7fffffffL) return VITAMD_ERR_SHAPE;
  if (!x || !codebook || !unit || !rnorm || !q || !idx || !loss || !ws) return VITAMD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* eunit = ws;
  float* partials = ws + (size_t)K * d;
  const int blocks = (int)vq_blocks(M);
  const int prep = (int)vq_blocks(M > K ? M : K);
  unsigned long long* packed = (unsigned long long*)idx;
  hipLaunchKernelGGL(vq_prepare_kernel, dim3(prep), dim3(256), 0, s, codebook, eunit, packed, M, K, d);
  const dim3 g2(blocks, (K + 255) / 256);
  if (g2.y > 65535) return VITAMD_ERR_SHAPE;
  if (d <= 16) hipLaunchKernelGGL(vq_search_kernel<16>, g2, dim3(256), 0, s, x, (const float*)eunit, unit, rnorm, packed, M, K, d);
  else hipLaunchKernelGGL(vq_search_kernel<64>, g2, dim3(256), 0, s, x, (const float*)eunit, unit, rnorm, packed, M, K, d);
  hipLaunchKernelGGL(vq_gather_kernel, dim3(blocks), dim3(256), 0, s, codebook, (const float*)unit, packed, q, partials, M, K, d);
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(SUM_THREADS), 0, s, (const float*)partials, loss, (long)blocks, 1.25 / ((double)M * d));
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_vq_quantize_bwd(const float* g_q, const float* g_loss, const float* unit, const float* rnorm, const long long* idx,
                                      const float* codebook, float* dx, float* dcodebook, int M, int K, int d, void* stream) {
  if (M < 1 || K < 1 || d < 1 || d > VQ_MAX_D || (long)M * d > 0x7fffffffL || (long)K * d > 0x7fffffffL) return VITAMD_ERR_SHAPE;
  if (!unit || !rnorm || !idx || !codebook || !dx || !dcodebook) return VITAMD_ERR_ARG;
  hipLaunchKernelGGL(vq_bwd_kernel, dim3((int)vq_blocks(M)), dim3(256), 0, (hipStream_t)stream, g_q, g_loss, unit, rnorm, idx, codebook, dx, dcodebook,
                     M, K, d, (float)(1.0 / ((double)M * d)));
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" long vitamd_recon_mse_ws_bytes(int B, int G, int p, int c, int y_bf16) {
  ReconPlan pl;
  if (!recon_plan(B, G, p, c, y_bf16, pl)) return -VITAMD_ERR_SHAPE;
  return pl.strips * (long)sizeof(float);
}

extern "C" int vitamd_recon_mse_fwd(const void* y, int y_bf16, const float* img, float* loss, float* ws, int B, int G, int p, int c, int ld,
                                    void* stream) {
  ReconPlan pl;
  if (!recon_plan(B, G, p, c, y_bf16, pl)) return VITAMD_ERR_SHAPE;
  const int W = y_bf16 ? 8 : 4;
  if (ld < p * p * c || ld % W != 0) return VITAMD_ERR_SHAPE;
  if (!y || !img || !loss || !ws) return VITAMD_ERR_ARG;
  if (!aligned16(y)) return VITAMD_ERR_SHAPE;           // the 16-byte path alone exists: the caller falls back
  hipStream_t s = (hipStream_t)stream;
  const bool vec_img = p % 4 == 0 && aligned16(img);
  const double E = (double)B * c * G * p * G * p;
  if (int e = y_bf16 ? launch_recon<true, false>(vec_img, pl, y, img, nullptr, nullptr, ws, G, p, c, ld, ld, 0.f, s)
                     : launch_recon<false, false>(vec_img, pl, y, img, nullptr, nullptr, ws, G, p, c, ld, ld, 0.f, s))
    return e;
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(SUM_THREADS), 0, s, (const float*)ws, loss, pl.strips, 1.0 / E);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_recon_mse_bwd(const void* y, int y_bf16, const float* img, const float* grad_out, void* dy, int B, int G, int p, int c, int ld,
                                    int ld_dy, void* stream) {
  ReconPlan pl;
  if (!recon_plan(B, G, p, c, y_bf16, pl)) return VITAMD_ERR_SHAPE;
  const int W = y_bf16 ? 8 : 4;
  if (ld < p * p * c || ld % W != 0 || ld_dy < p * p * c || ld_dy % W != 0) return VITAMD_ERR_SHAPE;
  if (!y || !img || !dy) return VITAMD_ERR_ARG;
  if (y == dy && ld != ld_dy) return VITAMD_ERR_ARG;    // in place: the tokens' own stride only
  if (!aligned16(y) || !aligned16(dy)) return VITAMD_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const bool vec_img = p % 4 == 0 && aligned16(img);
  const float inv_e = (float)(1.0 / ((double)B * c * G * p * G * p));
  if (int e = y_bf16 ? launch_recon<true, true>(vec_img, pl, y, img, grad_out, dy, nullptr, G, p, c, ld, ld_dy, inv_e, s)
                     : launch_recon<false, true>(vec_img, pl, y, img, grad_out, dy, nullptr, G, p, c, ld, ld_dy, inv_e, s))
    return e;
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
