// The strip kernel of the two reconstruction tails (DESIGN.md sections 13 and 19): mean of a per-pixel term between the image a token matrix
// stands for and the target image, taken on the tokens as the head GEMM wrote them, forward and backward.  A workgroup owns a strip of whole
// tokens of one grid row (b, gh): it stages them in LDS in 16-byte pieces, then walks the matching image rows (one run of contiguous floats
// per (channel, p1)), reading the token element of each pixel from LDS.  The backward writes the gradient over the staged tokens in LDS and
// the strip back in 16-byte pieces, so it may run in place.  Columns between F and the row stride are never touched.  Per-thread sums, then
// lanes, waves, workgroups (sum_partials_kernel) in a fixed order: no float atomics, the same bits on every call.
//
// What differs between the tails is a compile-time policy struct, Term (MseTerm: csrc/tokenizer.hip, L1Term: csrc/enhancing.hip):
//   typedef ... Scale;                        type of 1 / E and of the backward's scale
//   static constexpr bool IMG_GRAD, IMG_OUT;  the backward adds an image-shaped gradient (when given); the forward writes the image (when asked)
//   elem(t, ch, p1, p2, F, pp, p, c)          element of the strip that holds pixel (ch, p1, p2) of token t; F = pp c, pp = p p
//   step(c)                                   element stride between the four pixels of a vector item (consecutive p2)
//   scale(g, inv_e)                           the backward's scale from the upstream gradient g (1 when absent)
//   fwd(df)                                   the forward term of df = token - image
//   bwd(df, scale, gi)                        the backward value; gi: the image gradient, 0 without one
#pragma once
#include <type_traits>

#include "common.h"

namespace {

constexpr int RECON_LDS_BYTES = 48 * 1024;    // the staged strip; three workgroups per CU

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

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

// Strip s of the grid: (b, gh) = s / chunks, tokens gw0 .. gw0 + nt of that grid row.  LDS: the strip, compact ([token][F]), then 4 floats.
// Image items: VEC_IMG (p % 4 == 0, aligned image buffers): 4 consecutive pixels of one image row, which lie in one token; else single pixels.
template <typename Term, bool BF16, bool BWD, bool VEC_IMG>
__global__ __launch_bounds__(256) void recon_strip_kernel(const void* y, const float* __restrict__ img, const float* __restrict__ g_loss,
                                                          const float* __restrict__ g_img, void* dy, float* __restrict__ recon,
                                                          float* __restrict__ partials, int G, int p, int c, int ld, int ldo, int nt_max,
                                                          int chunks, typename Term::Scale inv_e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = BF16 ? 2 : 4;
  constexpr int W = 16 / ES;                            // elements per 16-byte piece
  typedef typename std::conditional<BF16, __bf16, float>::type T;
  typedef typename Term::Scale Scale;
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
  // the image of batch element b: with one image-shaped operand its offset goes into the pointer, with several into the index they share
  constexpr bool ONE_IMG = !Term::IMG_GRAD && !Term::IMG_OUT;
  const size_t img_off = (size_t)b * c * Wimg * Wimg;
  const float* img_b = ONE_IMG ? img + img_off : img;
  const size_t at_b = ONE_IMG ? 0 : img_off;
  const Scale scale = BWD ? Term::scale(g_loss ? *g_loss : 1.f, inv_e) : Scale(0);
  const int run = nt * p;                               // pixels of one image row inside the strip
  float a = 0.f;
  if constexpr (VEC_IMG) {
    const int qpr = run / 4;
    const int nitems = c * p * qpr;
    for (int i = threadIdx.x; i < nitems; i += 256) {
      const int r = i / qpr, xq = (i - r * qpr) * 4;    // r = ch * p + p1
      const int ch = r / p, p1 = r - ch * p;
      const int t = xq / p, p2 = xq - t * p;
      const size_t at = at_b + ((size_t)ch * Wimg + (size_t)gh * p + p1) * Wimg + (size_t)gw0 * p + xq;
      const f32x4 v = *(const f32x4*)(img_b + at);
      const int e0 = Term::elem(t, ch, p1, p2, F, pp, p, c), es = Term::step(c);
      f32x4 gi = {0.f, 0.f, 0.f, 0.f}, rv;
      if constexpr (BWD && Term::IMG_GRAD)
        if (g_img) gi = *(const f32x4*)(g_img + at);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        rv[k] = lds_elem<BF16>(strip_lds, e0 + k * es);
        if constexpr (BWD) lds_store<BF16>(strip_lds, e0 + k * es, Term::bwd(rv[k] - v[k], scale, gi[k]));
        else a += Term::fwd(rv[k] - v[k]);
      }
      if constexpr (!BWD && Term::IMG_OUT)
        if (recon) *(f32x4*)(recon + at) = rv;
    }
  } else {
    const int nitems = c * p * run;
    for (int i = threadIdx.x; i < nitems; i += 256) {
      const int r = i / run, xp = i - r * run;
      const int ch = r / p, p1 = r - ch * p;
      const int t = xp / p, p2 = xp - t * p;
      const size_t at = at_b + ((size_t)ch * Wimg + (size_t)gh * p + p1) * Wimg + (size_t)gw0 * p + xp;
      const int e0 = Term::elem(t, ch, p1, p2, F, pp, p, c);
      const float rv = lds_elem<BF16>(strip_lds, e0);
      const float df = rv - img_b[at];
      if constexpr (BWD) {
        float gi = 0.f;
        if constexpr (Term::IMG_GRAD) gi = g_img ? g_img[at] : 0.f;
        lds_store<BF16>(strip_lds, e0, Term::bwd(df, scale, gi));
      } else {
        a += Term::fwd(df);
        if constexpr (Term::IMG_OUT)
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
    a = block_sum_256(a, red);
    if (threadIdx.x == 0) partials[strip] = a;
  }
}

struct ReconPlan { int nt, chunks; long strips; size_t lds; };

// shape rules shared by the forwards, the backwards and the workspace query; false = VITAMD_ERR_SHAPE
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

// one launch of the strip kernel: the instantiation for (bf16, bwd, vec_img); g_loss, g_img, dy belong to the backward, recon and partials to
// the forward, and the other direction's are null
template <typename Term>
int launch_recon_strip(bool bf16, bool bwd, bool vec_img, const ReconPlan& pl, const void* y, const float* img, const float* g_loss,
                       const float* g_img, void* dy, float* recon, float* partials, int G, int p, int c, int ld, int ldo,
                       typename Term::Scale inv_e, hipStream_t s) {
  auto form = [&](auto BF, auto BW) {
    constexpr bool B16 = decltype(BF)::value, BWD = decltype(BW)::value;
    const dim3 grid((unsigned)pl.strips), block(256);
    return vec_img ? launch<recon_strip_kernel<Term, B16, BWD, true>>(grid, block, (int)pl.lds, s, y, img, g_loss, g_img, dy, recon, partials, G, p, c, ld,
                                                                     ldo, pl.nt, pl.chunks, inv_e)
                   : launch<recon_strip_kernel<Term, B16, BWD, false>>(grid, block, (int)pl.lds, s, y, img, g_loss, g_img, dy, recon, partials, G, p, c, ld,
                                                                      ldo, pl.nt, pl.chunks, inv_e);
  };
  if (bf16) return bwd ? form(std::true_type{}, std::true_type{}) : form(std::true_type{}, std::false_type{});
  return bwd ? form(std::false_type{}, std::true_type{}) : form(std::false_type{}, std::false_type{});
}

}  // namespace
