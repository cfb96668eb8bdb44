// The three streaming kernels of the Enhancing ViT-VQGAN tokenizer (train_enhancing_vitvqgan.py); everything else of
// that model runs on kernels that exist already.
//
// tanh between the two MLP GEMMs, forward and backward, on bf16 rows as the fc1 GEMM wrote them: 16-byte pieces (8 elements) per lane in
// a grid-stride loop under a grid cap, the elements in front of the first 16-byte boundary and behind the last whole piece one by one.
// Every element is read and written by the same lane, a piece as a whole before it is stored: both kernels may run in place.
//
// The L1 pixel tail: mean |depatchify(tokens) - images| on the tokens as the head GEMM wrote them, in the feature order of
// nn.ConvTranspose2d(dim, c, kernel = stride = p), (c p1 p2).  It is the strip kernel of csrc/recon_strip.h with L1Term below: in this
// feature order the four pixels of a 16-byte image load are four CONSECUTIVE token elements.  The forward also writes the image when asked
// to; the backward writes g sign(diff) / N + g_image over the staged tokens, so it may run in place.
#include "common.h"
#include "recon_strip.h"
#include "../../include/vitamd.h"

namespace {

constexpr int TANH_GRID_CAP = 2048;           // workgroups per launch (8 per CU); further pieces are reached by the stride loop

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

// one element of the backward: sign(df) * scale + g_image, summed in fp64 and rounded once; sign(0) = 0, so a tie gives g_image itself
__device__ __forceinline__ float l1_grad(float df, double scale, float gi) {
  const double s = (double)((df > 0.f) - (df < 0.f));
  return (float)(s * scale + (double)gi);
}

// The absolute-error term of recon_strip_kernel; the backward's scale is a double (l1_grad)
struct L1Term {
  typedef double Scale;
  static constexpr bool IMG_GRAD = true, IMG_OUT = true;
  static __device__ __forceinline__ int elem(int t, int ch, int p1, int p2, int F, int pp, int p, int) { return t * F + ch * pp + p1 * p + p2; }
  static __device__ __forceinline__ int step(int) { return 1; }
  static __device__ __forceinline__ double scale(float g, double inv_e) { return (double)g * inv_e; }
  static __device__ __forceinline__ float fwd(float df) { return __builtin_fabsf(df); }
  static __device__ __forceinline__ float bwd(float df, double scale, float gi) { return l1_grad(df, scale, gi); }
};

}  // namespace

extern "C" int vitamd_tanh_bf16(const void* pre, void* out, long n, void* stream) { return launch_tanh<false>(pre, nullptr, out, n, stream); }

extern "C" int vitamd_tanh_bwd_bf16(const void* dh, const void* t, void* dpre, long n, void* stream) {
  return launch_tanh<true>(dh, t, dpre, n, stream);
}

extern "C" int vitamd_recon_l1_fwd(const void* y, int y_bf16, const float* img, float* loss, float* recon, float* ws, long ws_bytes, int B, int G,
                                   int p, int c, int ld, void* stream) {
  ReconPlan pl;
  if (!recon_plan(B, G, p, c, y_bf16, pl)) return VITAMD_ERR_SHAPE;
  const int W = y_bf16 ? 8 : 4;
  if (ld < p * p * c || ld % W != 0) return VITAMD_ERR_SHAPE;
  if (!y || !img || !loss || !ws || ws_bytes < pl.strips * (long)sizeof(float)) return VITAMD_ERR_ARG;
  if (!aligned16(y)) return VITAMD_ERR_SHAPE;           // the 16-byte path alone exists: the caller falls back
  hipStream_t s = (hipStream_t)stream;
  const bool vec_img = p % 4 == 0 && aligned16(img) && aligned16(recon);
  const double E = (double)B * c * G * p * G * p;
  if (int e = launch_recon_strip<L1Term>(y_bf16 != 0, false, vec_img, pl, y, img, nullptr, nullptr, nullptr, recon, ws, G, p, c, ld, ld, 0.0, s)) return e;
  launch_sum_partials(ws, loss, pl.strips, 1.0 / E, s);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_recon_l1_bwd(const void* y, int y_bf16, const float* img, const float* g_loss, const float* g_recon, void* dy, int B, int G,
                                   int p, int c, int ld, int ld_dy, void* stream) {
  ReconPlan pl;
  if (!recon_plan(B, G, p, c, y_bf16, pl)) return VITAMD_ERR_SHAPE;
  const int W = y_bf16 ? 8 : 4;
  if (ld < p * p * c || ld % W != 0 || ld_dy < p * p * c || ld_dy % W != 0) return VITAMD_ERR_SHAPE;
  if (!y || !img || !dy) return VITAMD_ERR_ARG;
  if (y == dy && ld != ld_dy) return VITAMD_ERR_ARG;    // in place: the tokens' own stride only
  if (!aligned16(y) || !aligned16(dy)) return VITAMD_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const bool vec_img = p % 4 == 0 && aligned16(img) && aligned16(g_recon);
  const double inv_e = 1.0 / ((double)B * c * G * p * G * p);
  if (int e = launch_recon_strip<L1Term>(y_bf16 != 0, true, vec_img, pl, y, img, g_loss, g_recon, dy, nullptr, nullptr, G, p, c, ld, ld_dy, inv_e, s))
    return e;
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
