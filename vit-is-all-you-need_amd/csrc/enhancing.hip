// The three streaming kernels of the Enhancing ViT-VQGAN tokenizer (train_enhancing_vitvqgan.py); everything else of
// that model runs on kernels that exist already.
//
// tanh between the two MLP GEMMs, forward and backward, on bf16 rows as the fc1 GEMM wrote them: 16-byte pieces (8 elements) per lane in
// a grid-stride loop under a grid cap, the elements in front of the first 16-byte boundary and behind the last whole piece one by one.
// Every element is read and written by the same lane, a piece as a whole before it is stored: both kernels may run in place.
//
// The L1 pixel tail: mean |depatchify(tokens) - images| on the tokens as the head GEMM wrote them, in the feature order of
// nn.ConvTranspose2d(dim, c, kernel = stride = p), (c p1 p2).  The structure is recon_mse_kernel's (csrc/tokenizer.hip): a workgroup owns
// a strip of whole tokens of one grid row, stages it in LDS in 16-byte pieces and walks the matching image rows; in this feature order
// the four pixels of a 16-byte image load are four CONSECUTIVE token elements.  The forward also writes the image when asked to; the
// backward writes g sign(diff) / N + g_image over the staged tokens and the strip back in 16-byte pieces, so it may run in place.
// Per-thread sums, then lanes, waves, workgroups in a fixed order: no float atomics, the same bits on every call.
#include <type_traits>

#include "common.h"
#include "../../include/vitamd.h"

namespace {

constexpr int TANH_GRID_CAP = 2048;           // workgroups per launch (8 per CU); further pieces are reached by the stride loop
constexpr int RECON_LDS_BYTES = 48 * 1024;    // the staged strip; three workgroups per CU
constexpr int SUM_THREADS = 1024;

// tanh in fp32, |error| well inside half a bf16 ulp of the result for every bf16 input:
//   |x| <  1/16: x (1 - x^2/3 + 2 x^4/15), the series (next term 17 x^6 / 315 < 4e-9 relative); +-0 and tiny values keep sign and value
//   |x| >= 1/16: 1 - 2 / (exp(2 |x|) + 1) with |x| clamped to 20, where the quotient is below 2^-56: exactly 1, and exp never overflows
// (no inf / inf).  A NaN stays a NaN.
__device__ __forceinline__ float tanh_f32(float x) {
  const float ax = __builtin_fabsf(x);
  const float x2 = x * x;
  const float small = x * fmaf(x2, fmaf(x2, 0.13333333333f, -0.33333333333f), 1.0f);
  const float e = __expf(2.0f * fminf(ax, 20.0f));
  const float big = __builtin_copysignf(1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f), x);
  const float r = ax < 0.0625f ? small : big;
  return x != x ? x : r;
}

// dh (1 - t^2): t^2 is exact in fp32 for a bf16 t, the fma rounds 1 - t^2 once; t = +-1 gives exactly 0
__device__ __forceinline__ float tanh_bwd_f32(float dh, float t) { return dh * fmaf(-t, t, 1.0f); }

// elements [0, head) and [head + 8 n8, n) one by one, the n8 pieces between them as 16-byte vectors; a + head is 16-byte aligned in every
// operand (the host checks).  BWD: a = dh, t = the saved output; else a = the pre-activation, t unused.
template <bool BWD>
__global__ __launch_bounds__(256) void tanh_kernel(const __bf16* a, const __bf16* t, __bf16* out, size_t head, size_t n8, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n8; i += stride) {
    const u32x4 va = *(const u32x4*)(a + head + i * 8);
    u32x4 vt = va, o;
    if constexpr (BWD) vt = *(const u32x4*)(t + head + i * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (BWD) o[j] = pack_bf16x2(tanh_bwd_f32(bf16lo(va[j]), bf16lo(vt[j])), tanh_bwd_f32(bf16hi(va[j]), bf16hi(vt[j])));
      else o[j] = pack_bf16x2(tanh_f32(bf16lo(va[j])), tanh_f32(bf16hi(va[j])));
    }
    *(u32x4*)(out + head + i * 8) = o;
  }
  const size_t tail0 = head + n8 * 8, nedge = head + (n - tail0);
  for (size_t k = tid; k < nedge; k += stride) {
    const size_t i = k < head ? k : tail0 + (k - head);
    if constexpr (BWD) out[i] = f2bf(tanh_bwd_f32(bf2f(a[i]), bf2f(t[i])));
    else out[i] = f2bf(tanh_f32(bf2f(a[i])));
  }
}

template <bool BWD>
int launch_tanh(const void* a, const void* t, void* out, long n, void* stream) {
  if (n < 1) return VITAMD_ERR_SHAPE;
  if (!a || !out || (BWD && !t)) return VITAMD_ERR_ARG;
  const uintptr_t ma = (uintptr_t)a & 15, mo = (uintptr_t)out & 15, mt = BWD ? ((uintptr_t)t & 15) : ma;
  if ((ma | mo | mt) & 1) return VITAMD_ERR_ARG;          // a bf16 element is 2-byte aligned
  // the vector body needs one 16-byte phase for every operand; operands out of phase with each other go element by element
  size_t head = (size_t)n, n8 = 0;
  if (ma == mo && ma == mt) {
    head = ((16 - ma) & 15) / 2;
    if (head > (size_t)n) head = (size_t)n;
    n8 = ((size_t)n - head) / 8;
  }
  const size_t edge = (size_t)n - n8 * 8;
  size_t work = n8 > edge ? n8 : edge;
  size_t wgs = (work + 255) / 256;
  if (wgs < 1) wgs = 1;
  if (wgs > (size_t)TANH_GRID_CAP) wgs = TANH_GRID_CAP;
  hipLaunchKernelGGL(tanh_kernel<BWD>, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, (const __bf16*)a, (const __bf16*)t, (__bf16*)out, head, n8,
                     (size_t)n);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

// out[0] = scale * sum(partials[0 .. n)), one workgroup: every thread sums its strided share in fp64, then lanes, then waves, in a fixed order
__global__ __launch_bounds__(SUM_THREADS) void l1_sum_partials_kernel(const float* __restrict__ partials, float* __restrict__ out, long n, double scale) {
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

// one element of the backward: sign(df) * scale + g_image, summed in fp64 and rounded once; sign(0) = 0, so a tie gives g_image itself
__device__ __forceinline__ float l1_grad(float df, double scale, float gi) {
  const double s = (double)((df > 0.f) - (df < 0.f));
  return (float)(s * scale + (double)gi);
}

// Strip s of the grid: (b, gh) = s / chunks, tokens gw0 .. gw0 + nt of that grid row.  LDS: the strip, compact ([token][F]), then 4 floats.
// Image items: VEC_IMG (p % 4 == 0, aligned image buffers): 4 consecutive pixels of one image row = 4 consecutive elements of one token;
// else single pixels.  Token element of pixel (ch, p1, p2): ch p^2 + p1 p + p2.
template <bool BF16, bool BWD, bool VEC_IMG>
__global__ __launch_bounds__(256) void recon_l1_kernel(const void* y, const float* __restrict__ img, const float* __restrict__ g_loss,
                                                       const float* __restrict__ g_img, void* dy, float* __restrict__ recon,
                                                       float* __restrict__ partials, int G, int p, int c, int ld, int ldo, int nt_max, int chunks,
                                                       double inv_e) {
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

  const int Wimg = G * p, pp = p * p;
  const size_t img_b = (size_t)b * c * Wimg * Wimg;
  const double scale = BWD ? (double)(g_loss ? *g_loss : 1.f) * inv_e : 0.0;
  const int run = nt * p;                               // pixels of one image row inside the strip
  float a = 0.f;
  if constexpr (VEC_IMG) {
    const int qpr = run / 4;
    const int nitems = c * p * qpr;
    for (int i = threadIdx.x; i < nitems; i += 256) {
      const int r = i / qpr, xq = (i - r * qpr) * 4;    // r = ch * p + p1
      const int ch = r / p, p1 = r - ch * p;
      const int t = xq / p, p2 = xq - t * p;
      const size_t at = img_b + ((size_t)ch * Wimg + (size_t)gh * p + p1) * Wimg + (size_t)gw0 * p + xq;
      const f32x4 v = *(const f32x4*)(img + at);
      const int e0 = t * F + ch * pp + p1 * p + p2;
      if constexpr (BWD) {
        f32x4 gi = {0.f, 0.f, 0.f, 0.f};
        if (g_img) gi = *(const f32x4*)(g_img + at);
#pragma unroll
        for (int k = 0; k < 4; ++k) lds_store<BF16>(strip_lds, e0 + k, l1_grad(lds_elem<BF16>(strip_lds, e0 + k) - v[k], scale, gi[k]));
      } else {
        f32x4 rv;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          rv[k] = lds_elem<BF16>(strip_lds, e0 + k);
          a += __builtin_fabsf(rv[k] - v[k]);
        }
        if (recon) *(f32x4*)(recon + at) = rv;
      }
    }
  } else {
    const int nitems = c * p * run;
    for (int i = threadIdx.x; i < nitems; i += 256) {
      const int r = i / run, xp = i - r * run;
      const int ch = r / p, p1 = r - ch * p;
      const int t = xp / p, p2 = xp - t * p;
      const size_t at = img_b + ((size_t)ch * Wimg + (size_t)gh * p + p1) * Wimg + (size_t)gw0 * p + xp;
      const int e0 = t * F + ch * pp + p1 * p + p2;
      const float rv = lds_elem<BF16>(strip_lds, e0);
      const float df = rv - img[at];
      if constexpr (BWD) {
        lds_store<BF16>(strip_lds, e0, l1_grad(df, scale, g_img ? g_img[at] : 0.f));
      } else {
        a += __builtin_fabsf(df);
        if (recon) recon[at] = rv;
      }
    }
  }
  if constexpr (BWD) {
    __syncthreads();
    for (int i = threadIdx.x; i < npieces; i += 256) {
      const int t = i / ppr, j = i - t * ppr;
      *(u32x4*)((T*)dy + (row0 + t) * (size_t)ldo + (size_t)j * W) = *(const u32x4*)(strip_lds + (size_t)i * 16);
    }
  } else {
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) partials[strip] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct L1Plan { int nt, chunks; long strips; size_t lds; };

// shape rules shared by the forward and the backward (those of vitamd_recon_mse_*: the workspace is the same size); false = VITAMD_ERR_SHAPE
inline bool l1_plan(int B, int G, int p, int c, int bf16, L1Plan& pl) {
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
int launch_l1_form(const L1Plan& pl, const void* y, const float* img, const float* g_loss, const float* g_img, void* dy, float* recon, float* partials,
                   int G, int p, int c, int ld, int ldo, double inv_e, hipStream_t s) {
  if (int e = set_lds(recon_l1_kernel<BF16, BWD, VEC_IMG>, (int)pl.lds)) return e;
  hipLaunchKernelGGL((recon_l1_kernel<BF16, BWD, VEC_IMG>), dim3((unsigned)pl.strips), dim3(256), pl.lds, s, y, img, g_loss, g_img, dy, recon, partials, G,
                     p, c, ld, ldo, pl.nt, pl.chunks, inv_e);
  return VITAMD_OK;
}

template <bool BWD>
int launch_l1(bool bf16, bool vec_img, const L1Plan& pl, const void* y, const float* img, const float* g_loss, const float* g_img, void* dy, float* recon,
              float* partials, int G, int p, int c, int ld, int ldo, double inv_e, hipStream_t s) {
  if (bf16)
    return vec_img ? launch_l1_form<true, BWD, true>(pl, y, img, g_loss, g_img, dy, recon, partials, G, p, c, ld, ldo, inv_e, s)
                   : launch_l1_form<true, BWD, false>(pl, y, img, g_loss, g_img, dy, recon, partials, G, p, c, ld, ldo, inv_e, s);
  return vec_img ? launch_l1_form<false, BWD, true>(pl, y, img, g_loss, g_img, dy, recon, partials, G, p, c, ld, ldo, inv_e, s)
                 : launch_l1_form<false, BWD, false>(pl, y, img, g_loss, g_img, dy, recon, partials, G, p, c, ld, ldo, inv_e, s);
}

}  // namespace

extern "C" int vitamd_tanh_bf16(const void* pre, void* out, long n, void* stream) { return launch_tanh<false>(pre, nullptr, out, n, stream); }

extern "C" int vitamd_tanh_bwd_bf16(const void* dh, const void* t, void* dpre, long n, void* stream) {
  return launch_tanh<true>(dh, t, dpre, n, stream);
}

extern "C" int vitamd_recon_l1_fwd(const void* y, int y_bf16, const float* img, float* loss, float* recon, float* ws, long ws_bytes, int B, int G,
                                   int p, int c, int ld, void* stream) {
  L1Plan pl;
  if (!l1_plan(B, G, p, c, y_bf16, pl)) return VITAMD_ERR_SHAPE;
  const int W = y_bf16 ? 8 : 4;
  if (ld < p * p * c || ld % W != 0) return VITAMD_ERR_SHAPE;
  if (!y || !img || !loss || !ws || ws_bytes < pl.strips * (long)sizeof(float)) return VITAMD_ERR_ARG;
  if (!aligned16(y)) return VITAMD_ERR_SHAPE;           // the 16-byte path alone exists: the caller falls back
  hipStream_t s = (hipStream_t)stream;
  const bool vec_img = p % 4 == 0 && aligned16(img) && aligned16(recon);
  const double E = (double)B * c * G * p * G * p;
  if (int e = launch_l1<false>(y_bf16 != 0, vec_img, pl, y, img, nullptr, nullptr, nullptr, recon, ws, G, p, c, ld, ld, 0.0, s)) return e;
  hipLaunchKernelGGL(l1_sum_partials_kernel, dim3(1), dim3(SUM_THREADS), 0, s, (const float*)ws, loss, pl.strips, 1.0 / E);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_recon_l1_bwd(const void* y, int y_bf16, const float* img, const float* g_loss, const float* g_recon, void* dy, int B, int G,
                                   int p, int c, int ld, int ld_dy, void* stream) {
  L1Plan pl;
  if (!l1_plan(B, G, p, c, y_bf16, pl)) return VITAMD_ERR_SHAPE;
  const int W = y_bf16 ? 8 : 4;
  if (ld < p * p * c || ld % W != 0 || ld_dy < p * p * c || ld_dy % W != 0) return VITAMD_ERR_SHAPE;
  if (!y || !img || !dy) return VITAMD_ERR_ARG;
  if (y == dy && ld != ld_dy) return VITAMD_ERR_ARG;    // in place: the tokens' own stride only
  if (!aligned16(y) || !aligned16(dy)) return VITAMD_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const bool vec_img = p % 4 == 0 && aligned16(img) && aligned16(g_recon);
  const double inv_e = 1.0 / ((double)B * c * G * p * G * p);
  if (int e = launch_l1<true>(y_bf16 != 0, vec_img, pl, y, img, g_loss, g_recon, dy, nullptr, nullptr, G, p, c, ld, ld_dy, inv_e, s)) return e;
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
