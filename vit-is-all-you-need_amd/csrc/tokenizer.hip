// Training of the two image tokenizers: the cosine-similarity VQ quantiser of train_titok.Quantizer, forward and
// backward, and the reconstruction loss mse_loss(pixel_shuffle(tokens), images) taken on the tokens as the head GEMM wrote them, forward
// and backward.  The two halves share the final fixed-order sum (sum_partials_kernel, csrc/common.h) and nothing else.
//
// Quantiser.  All arithmetic is fp32.  u = x / max(|x|, eps) and e^_k = e_k / max(|e_k|, eps), both norms summed over ascending c;
// the unit codebook is staged once per call in the workspace.  The search is vq_nearest's (csrc/vq_scan.h): one thread per row, 256 codes
// per workgroup in LDS, sum over ascending c of (u_c - e^_kc)^2, strict <, and (distance bits << 32 | index) folded into the row's slot
// of the index buffer by a 64-bit atomicMin - the first minimum whatever order the chunks arrive in.  A second pass gathers the RAW row,
// writes q = u + (p - u) and the row's sum of (p - u)^2; per-workgroup partials and one fixed-order sum give the loss: no float atomics,
// the same bits on every call.  The backward is one thread per row; rows of a workgroup that picked the same code are summed on chip in
// ascending row order before ONE fp32 atomic per (code, column) leaves the workgroup, so dcodebook depends on arrival order only where
// a code is shared between workgroups.
//
// Reconstruction loss.  The strip kernel of csrc/recon_strip.h with the squared-error term, MseTerm; the entry points are here.
#include "common.h"
#include "recon_strip.h"
#include "vq_scan.h"
#include "../../include/vitamd.h"

namespace {

constexpr float VQ_EPS = 1e-12f;              // F.normalize
constexpr float VQ_RNORM_CLAMPED = 1.0f / VQ_EPS;   // rnorm of a row whose norm was below eps: the backward's mark for dx = du / eps
constexpr int VQ_MAX_D = VITAMD_VQ_MAX_D;

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
  const VqBest best = vq_scan_chunk<DMAX>(ce, xr, eunit, k0, nk, d, VqBest{3.0e38f, k0});
  if (m < M) atomicMin(packed + m, ((unsigned long long)__builtin_bit_cast(unsigned, best.dist) << 32) | (unsigned)best.index);
}

// idx = the low half of the packed word; q = u + (p - u) on the raw row p; partials[workgroup] = sum over its rows of (p - u)^2.
// UNIT (blocks.VectorQuantizer(use_l2_norm=True)): the caller passes the unit codebook as e, so p is the normalised row.
template <bool UNIT>
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
// k_commit = 0.5 s / (M d), k_code = 2 s / (M d), s = *g_loss (0 when absent).
// UNIT: p is the normalised code row e / max(|e|, eps) (the prepare kernel's arithmetic) and the per-code sum T of a workgroup goes through
// the normalisation before it leaves: (T - e^ (e^ . T)) / |e|, or T / eps for a row whose norm was below eps (F.normalize's clamp).
template <bool UNIT>
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
  float den = 1.f, enorm = 1.f;                                    // UNIT: p = e / den
  if (id >= 0) {
    const float* u = unit + (size_t)m * d;
    const float* p = e + (size_t)id * d;
    if constexpr (UNIT) {
      float ss = 0.f;
      for (int c = 0; c < d; ++c) ss += p[c] * p[c];
      enorm = sqrtf(ss);
      den = fmaxf(enorm, VQ_EPS);
    }
    const float* g = g_q ? g_q + (size_t)m * d : nullptr;
    float dot = 0.f;
    for (int c = 0; c < d; ++c) {
      const float pc = UNIT ? p[c] / den : p[c];
      const float du = (g ? g[c] : 0.f) + k_commit * (u[c] - pc);
      dot += u[c] * du;
    }
    const float rn = rnorm[m];
    const bool clamped = rn == VQ_RNORM_CLAMPED;
    for (int c = 0; c < d; ++c) {
      const float pc = UNIT ? p[c] / den : p[c];
      const float du = (g ? g[c] : 0.f) + k_commit * (u[c] - pc);
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
  // UNIT, first pass: e^ . T over all columns (T in units of k_code), by the same chunked sums the second pass repeats
  float edot = 0.f;
  if constexpr (UNIT) {
    if (enorm >= VQ_EPS) {
      for (int c0 = 0; c0 < d; c0 += 16) {
        float acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[c] = 0.f;
        for (int j = threadIdx.x; j < 256; ++j) {
          if (ids[j] != id) continue;
          const float* u = unit + (size_t)(row0 + j) * d;
#pragma unroll
          for (int c = 0; c < 16; ++c)
            if (c0 + c < d) acc[c] += p[c0 + c] / den - u[c0 + c];
        }
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if (c0 + c < d) edot += (p[c0 + c] / den) * acc[c];
      }
    }
  }
  for (int c0 = 0; c0 < d; c0 += 16) {
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.f;
    for (int j = threadIdx.x; j < 256; ++j) {
      if (ids[j] != id) continue;
      const float* u = unit + (size_t)(row0 + j) * d;
#pragma unroll
      for (int c = 0; c < 16; ++c)
        if (c0 + c < d) acc[c] += (UNIT ? p[c0 + c] / den : p[c0 + c]) - u[c0 + c];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      if (c0 + c >= d) continue;
      float t = acc[c];
      if constexpr (UNIT) t = enorm >= VQ_EPS ? (t - (p[c0 + c] / den) * edot) / den : t / VQ_EPS;
      atomicAdd(dcode + (size_t)id * d + c0 + c, k_code * t);
    }
  }
}

// ------------------------------------------------------------------------------------------------ reconstruction loss
// The squared-error term of recon_strip_kernel (csrc/recon_strip.h): tokens in the feature order of pixel_shuffle, (p1 p2 c), so the four
// pixels of a vector item lie c elements apart; all arithmetic in fp32.
struct MseTerm {
  typedef float Scale;
  static constexpr bool IMG_GRAD = false, IMG_OUT = false;
  static __device__ __forceinline__ int elem(int t, int ch, int p1, int p2, int F, int, int p, int c) { return t * F + (p1 * p + p2) * c + ch; }
  static __device__ __forceinline__ int step(int c) { return c; }
  static __device__ __forceinline__ float scale(float g, float inv_e) { return 2.0f * g * inv_e; }
  static __device__ __forceinline__ float fwd(float df) { return df * df; }
  static __device__ __forceinline__ float bwd(float df, float scale, float) { return df * scale; }
};

inline long vq_blocks(int M) { return ((long)M + 255) / 256; }

}  // namespace

extern "C" long vitamd_vq_quantize_ws_bytes(int M, int K, int d) {
  if (M < 1 || K < 1 || d < 1 || d > VQ_MAX_D) return -VITAMD_ERR_SHAPE;
  return ((long)K * d + vq_blocks(M)) * (long)sizeof(float);
}

namespace {

template <bool UNIT>
int vq_fwd(const float* x, const float* codebook, float* unit, float* rnorm, float* q, long long* idx, float* loss, float* ws, int M, int K, int d,
           void* stream) {
  if (M < 1 || K < 1 || d < 1 || d > VQ_MAX_D || (long)M * d > 0x7fffffffL || (long)K * d > 0x7fffffffL) return VITAMD_ERR_SHAPE;
  if (!x || !codebook || !unit || !rnorm || !q || !idx || !loss || !ws) return VITAMD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* eunit = ws;
  float* partials = ws + (size_t)K * d;
  const int blocks = (int)vq_blocks(M);
  const int prep = (int)vq_blocks(M > K ? M : K);
  unsigned long long* packed = (unsigned long long*)idx;
  const dim3 g2(blocks, (K + 255) / 256);
  if (g2.y > 65535) return VITAMD_ERR_SHAPE;
  hipLaunchKernelGGL(vq_prepare_kernel, dim3(prep), dim3(256), 0, s, codebook, eunit, packed, M, K, d);
  if (d <= 16) hipLaunchKernelGGL(vq_search_kernel<16>, g2, dim3(256), 0, s, x, (const float*)eunit, unit, rnorm, packed, M, K, d);
  else hipLaunchKernelGGL(vq_search_kernel<64>, g2, dim3(256), 0, s, x, (const float*)eunit, unit, rnorm, packed, M, K, d);
  hipLaunchKernelGGL(vq_gather_kernel<UNIT>, dim3(blocks), dim3(256), 0, s, UNIT ? (const float*)eunit : codebook, (const float*)unit, packed, q, partials,
                     M, K, d);
  launch_sum_partials(partials, loss, blocks, 1.25 / ((double)M * d), s);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

template <bool UNIT>
int vq_bwd(const float* g_q, const float* g_loss, const float* unit, const float* rnorm, const long long* idx, const float* codebook, float* dx,
           float* dcodebook, int M, int K, int d, void* stream) {
  if (M < 1 || K < 1 || d < 1 || d > VQ_MAX_D || (long)M * d > 0x7fffffffL || (long)K * d > 0x7fffffffL) return VITAMD_ERR_SHAPE;
  if (!unit || !rnorm || !idx || !codebook || !dx || !dcodebook) return VITAMD_ERR_ARG;
  hipLaunchKernelGGL(vq_bwd_kernel<UNIT>, dim3((int)vq_blocks(M)), dim3(256), 0, (hipStream_t)stream, g_q, g_loss, unit, rnorm, idx, codebook, dx,
                     dcodebook, M, K, d, (float)(1.0 / ((double)M * d)));
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

}  // namespace

extern "C" int vitamd_vq_quantize_fwd(const float* x, const float* codebook, float* unit, float* rnorm, float* q, long long* idx, float* loss,
                                      float* ws, int M, int K, int d, void* stream) {
  return vq_fwd<false>(x, codebook, unit, rnorm, q, idx, loss, ws, M, K, d, stream);
}

extern "C" int vitamd_vq_quantize_bwd(const float* g_q, const float* g_loss, const float* unit, const float* rnorm, const long long* idx,
                                      const float* codebook, float* dx, float* dcodebook, int M, int K, int d, void* stream) {
  return vq_bwd<false>(g_q, g_loss, unit, rnorm, idx, codebook, dx, dcodebook, M, K, d, stream);
}

extern "C" int vitamd_vq_quantize_unit_fwd(const float* x, const float* codebook, float* unit, float* rnorm, float* q, long long* idx, float* loss,
                                           float* ws, int M, int K, int d, void* stream) {
  return vq_fwd<true>(x, codebook, unit, rnorm, q, idx, loss, ws, M, K, d, stream);
}

extern "C" int vitamd_vq_quantize_unit_bwd(const float* g_q, const float* g_loss, const float* unit, const float* rnorm, const long long* idx,
                                           const float* codebook, float* dx, float* dcodebook, int M, int K, int d, void* stream) {
  return vq_bwd<true>(g_q, g_loss, unit, rnorm, idx, codebook, dx, dcodebook, M, K, d, stream);
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
  if (int e = launch_recon_strip<MseTerm>(y_bf16 != 0, false, vec_img, pl, y, img, nullptr, nullptr, nullptr, nullptr, ws, G, p, c, ld, ld, 0.f, s)) return e;
  launch_sum_partials(ws, loss, pl.strips, 1.0 / E, s);
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
  if (int e = launch_recon_strip<MseTerm>(y_bf16 != 0, true, vec_img, pl, y, img, grad_out, nullptr, dy, nullptr, nullptr, G, p, c, ld, ld_dy, inv_e, s))
    return e;
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------ pixel tail: conv_out on the tokens + loss
// The tail of blocks.TiTokDecoder: r = conv3x3(pixel_shuffle(tokens), w, zero padding 1) + bias, loss = mean((r - img)^2), c = 3.  The
// shuffled image is never formed.  Row y of image b is a line of 3 * Wimg elements, L = 3 x + ch, that lies in the token matrix in runs of
// 3 p elements: token (gh, gw = L / 3p), columns p1 * 3p + L % 3p.  With p % 8 == 0 (bf16) / p % 4 == 0 (fp32) every run is whole 16-byte
// pieces, so a workgroup stages the lines of its 32 x 32 pixel tile and their halo piece by piece, as fp32, zero outside the image (rows
// of another image of the batch are never read: a tile belongs to one b).  Forward: halo 1.  Backward: halo 2 - it recomputes r on the
// tile + 1, forms e there (zero outside the image), and from e in LDS takes the input gradient (flipped taps) and, on the tile's own
// pixels only, the weight and bias gradients.  Every sum is per thread, then lanes, waves, workgroups in a fixed order: no float atomics.
namespace {

constexpr int CT = 32;                 // tile side, pixels
constexpr int CT_L0 = 8;               // staged line element of (tile column 0, channel 0): the line starts 8 elements (whole pieces) before the tile
constexpr int CT_LROW = 112;           // staged elements per row: 8 before, 96 of the tile, 8 after; the 2-pixel halo needs 6 on either side
constexpr int CT_ER = CT + 2;          // side of the region e is formed on
constexpr int CT_NW = 84;              // 81 weight + 3 bias gradients

struct ConvTile { long b; int y0, x0; };

__device__ __forceinline__ ConvTile conv_tile(long tile, int side) {
  ConvTile t;
  const long per = (long)side * side;
  t.b = tile / per;
  const int r = (int)(tile - t.b * per);
  t.y0 = (r / side) * CT;
  t.x0 = (r - (r / side) * side) * CT;
  return t;
}

// rows y0 - R .. y0 + CT + R of image b into S[(CT + 2R) x CT_LROW] as fp32; element l of a row is line element 3 x0 - CT_L0 + l
template <bool BF16, int R>
__device__ __forceinline__ void stage_lines(float* S, const void* tok, long b, int y0, int x0, int G, int p, int ld) {
  constexpr int W = BF16 ? 8 : 4;
  constexpr int PPR = CT_LROW / W;
  const int Himg = G * p, seg = 3 * p, Lend = 3 * Himg;
  for (int i = threadIdx.x; i < (CT + 2 * R) * PPR; i += 256) {
    const int row = i / PPR, k = i - row * PPR;
    const int y = y0 - R + row;
    const int L = 3 * x0 - CT_L0 + k * W;               // a multiple of W, as Lend and seg are: a piece is inside one run or outside the image
    float v[W];
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = 0.f;
    if (y >= 0 && y < Himg && L >= 0 && L < Lend) {
      const int gh = y / p, p1 = y - gh * p, gw = L / seg, off = L - gw * seg;
      const size_t e = ((size_t)b * G * G + (size_t)gh * G + gw) * (size_t)ld + (size_t)p1 * seg + off;
      if constexpr (BF16) {
        const u32x4 raw = *(const u32x4*)((const __bf16*)tok + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[2 * j] = bf16lo(raw[j]); v[2 * j + 1] = bf16hi(raw[j]); }
      } else {
        const f32x4 raw = *(const f32x4*)((const float*)tok + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = raw[j];
      }
    }
    float* dst = S + row * CT_LROW + k * W;
#pragma unroll
    for (int j = 0; j < W; j += 4) *(f32x4*)(dst + j) = f32x4{v[j], v[j + 1], v[j + 2], v[j + 3]};
  }
}

// r[co] = bias[co] + sum over ci, kh, kw of w[co, ci, kh, kw] * yimg[ci](y + kh - 1, x + kw - 1); (row, l): the pixel's channel 0 in S
__device__ __forceinline__ void conv_at(const float* S, int row, int l, const float* __restrict__ w, const float* __restrict__ bias, float r[3]) {
#pragma unroll
  for (int co = 0; co < 3; ++co) r[co] = bias[co];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {
        const float v = S[(row + kh - 1) * CT_LROW + l + 3 * (kw - 1) + ci];
#pragma unroll
        for (int co = 0; co < 3; ++co) r[co] = fmaf(w[((co * 3 + ci) * 3 + kh) * 3 + kw], v, r[co]);
      }
}

// The wave's sum in lane 63, on the VALU's lane-crossing (DPP) paths: pairs and quads, row_shr 4 and 8 (lane 15 of a 16-lane row then holds
// the row), row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3.  A fixed order, and no LDS traffic - the backward kernel
// reduces 84 values per workgroup, which as ds_bpermute shuffles were more LDS instructions than the rest of the kernel issues.
#define CT_DPP_ADD(v, ctrl, rows) \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, rows, 0xf, false))
__device__ __forceinline__ float wave_sum_lane63(float v) {
  CT_DPP_ADD(v, 0xB1, 0xf);            // quad_perm [1, 0, 3, 2]
  CT_DPP_ADD(v, 0x4E, 0xf);            // quad_perm [2, 3, 0, 1]
  CT_DPP_ADD(v, 0x114, 0xf);           // row_shr 4
  CT_DPP_ADD(v, 0x118, 0xf);           // row_shr 8
  CT_DPP_ADD(v, 0x142, 0xa);           // row_bcast 15
  CT_DPP_ADD(v, 0x143, 0xc);           // row_bcast 31
  return v;
}
#undef CT_DPP_ADD

// thread t: column t % 32 of rows t / 32 + 8 i, i = 0 .. 3
template <bool BF16>
__global__ __launch_bounds__(256) void conv_recon_fwd_kernel(const void* tok, const float* __restrict__ w, const float* __restrict__ bias,
                                                             const float* __restrict__ img, float* __restrict__ recon, float* __restrict__ partials,
                                                             int G, int p, int ld, int side) {
  __shared__ __attribute__((aligned(16))) float S[(CT + 2) * CT_LROW];
  __shared__ float red[4];
  const ConvTile t = conv_tile(blockIdx.x, side);
  const int Himg = G * p;
  stage_lines<BF16, 1>(S, tok, t.b, t.y0, t.x0, G, p, ld);
  __syncthreads();
  const int tx = threadIdx.x & 31, x = t.x0 + tx;
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ty = (threadIdx.x >> 5) + 8 * i, y = t.y0 + ty;
    if (x >= Himg || y >= Himg) continue;
    float r[3];
    conv_at(S, ty + 1, CT_L0 + 3 * tx, w, bias, r);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const size_t at = (((size_t)t.b * 3 + ch) * Himg + y) * Himg + x;
      const float df = r[ch] - img[at];
      a += df * df;
      if (recon) recon[at] = r[ch];
    }
  }
  a = block_sum_256(a, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

// wpart[j * ntiles + tile]: this tile's share of gradient j (dw in [co][ci][kh][kw] order, then db)
template <bool BF16>
__global__ __launch_bounds__(256) void conv_recon_bwd_kernel(const void* tok, const float* __restrict__ w, const float* __restrict__ bias,
                                                             const float* __restrict__ img, const float* __restrict__ g_loss,
                                                             const float* __restrict__ g_recon, void* dtok, float* __restrict__ wpart, int G, int p,
                                                             int ld, int ldo, int side, long ntiles, float inv_n) {
  typedef typename std::conditional<BF16, __bf16, float>::type T;
  constexpr int W = BF16 ? 8 : 4;
  __shared__ __attribute__((aligned(16))) float S[(CT + 4) * CT_LROW];
  __shared__ float E[3 * CT_ER * CT_ER];
  __shared__ float wred[4 * CT_NW];
  const ConvTile t = conv_tile(blockIdx.x, side);
  const int Himg = G * p;
  stage_lines<BF16, 2>(S, tok, t.b, t.y0, t.x0, G, p, ld);
  __syncthreads();
  const float scale = 2.0f * (g_loss ? *g_loss : 1.f) * inv_n;
  for (int i = threadIdx.x; i < CT_ER * CT_ER; i += 256) {
    const int ey = i / CT_ER, ex = i - ey * CT_ER;
    const int y = t.y0 - 1 + ey, x = t.x0 - 1 + ex;
    float e[3] = {0.f, 0.f, 0.f};
    if (y >= 0 && y < Himg && x >= 0 && x < Himg) {
      float r[3];
      conv_at(S, ey + 1, CT_L0 + 3 * (ex - 1), w, bias, r);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const size_t at = (((size_t)t.b * 3 + ch) * Himg + y) * Himg + x;
        e[ch] = scale * (r[ch] - img[at]) + (g_recon ? g_recon[at] : 0.f);
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) E[ch * CT_ER * CT_ER + i] = e[ch];
  }
  __syncthreads();
  const int tx = threadIdx.x & 31, x = t.x0 + tx;
  float acc[CT_NW];
#pragma unroll
  for (int j = 0; j < CT_NW; ++j) acc[j] = 0.f;
  float dx[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ty = (threadIdx.x >> 5) + 8 * i, y = t.y0 + ty;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) dx[i][ci] = 0.f;
    if (x >= Himg || y >= Himg) continue;
    float e[3];
#pragma unroll
    for (int co = 0; co < 3; ++co) e[co] = E[co * CT_ER * CT_ER + (ty + 1) * CT_ER + tx + 1];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const float v = S[(ty + 2 + kh - 1) * CT_LROW + CT_L0 + 3 * tx + 3 * (kw - 1) + ci];
#pragma unroll
          for (int co = 0; co < 3; ++co) acc[((co * 3 + ci) * 3 + kh) * 3 + kw] = fmaf(e[co], v, acc[((co * 3 + ci) * 3 + kh) * 3 + kw]);
        }
        // the input gradient: tap (kh, kw) of output pixel (y + 1 - kh, x + 1 - kw) reaches this pixel
#pragma unroll
        for (int co = 0; co < 3; ++co) {
          const float eo = E[co * CT_ER * CT_ER + (ty + 1 - (kh - 1)) * CT_ER + tx + 1 - (kw - 1)];
#pragma unroll
          for (int ci = 0; ci < 3; ++ci) dx[i][ci] = fmaf(w[((co * 3 + ci) * 3 + kh) * 3 + kw], eo, dx[i][ci]);
        }
      }
#pragma unroll
    for (int co = 0; co < 3; ++co) acc[81 + co] += e[co];
  }
  __syncthreads();                                       // every read of S is done: the tile's gradient takes its place, [CT][96] of T
  T* out = (T*)S;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ty = (threadIdx.x >> 5) + 8 * i;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
      if constexpr (BF16) out[ty * (3 * CT) + 3 * tx + ci] = f2bf(dx[i][ci]);
      else out[ty * (3 * CT) + 3 * tx + ci] = dx[i][ci];
    }
  }
#pragma unroll
  for (int j = 0; j < CT_NW; ++j) {
    const float v = wave_sum_lane63(acc[j]);
    if ((threadIdx.x & 63) == 63) wred[(threadIdx.x >> 6) * CT_NW + j] = v;
  }
  __syncthreads();
  constexpr int PPR = 3 * CT / W;
  const int seg = 3 * p, Lend = 3 * Himg;
  for (int i = threadIdx.x; i < CT * PPR; i += 256) {
    const int ty = i / PPR, k = i - ty * PPR;
    const int y = t.y0 + ty, L = 3 * t.x0 + k * W;
    if (y >= Himg || L >= Lend) continue;
    const int gh = y / p, p1 = y - gh * p, gw = L / seg, off = L - gw * seg;
    const size_t at = ((size_t)t.b * G * G + (size_t)gh * G + gw) * (size_t)ldo + (size_t)p1 * seg + off;
    *(u32x4*)((T*)dtok + at) = *(const u32x4*)(out + ty * (3 * CT) + k * W);
  }
  if (threadIdx.x < CT_NW) {
    const int j = threadIdx.x;
    wpart[(size_t)j * ntiles + blockIdx.x] = (wred[j] + wred[CT_NW + j]) + (wred[2 * CT_NW + j] + wred[3 * CT_NW + j]);
  }
}

// workgroup j: gradient j = the sum of its ntiles partials, strided shares in fp64, then lanes, then waves
__global__ __launch_bounds__(256) void conv_wgrad_sum_kernel(const float* __restrict__ wpart, float* __restrict__ dw, float* __restrict__ db, long ntiles) {
  __shared__ double part[4];
  const int j = blockIdx.x;
  const float* src = wpart + (size_t)j * ntiles;
  double a = 0.0;
  for (long i = threadIdx.x; i < ntiles; i += 256) a += (double)src[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float v = (float)((part[0] + part[1]) + (part[2] + part[3]));
  if (j < 81) dw[j] = v;
  else db[j - 81] = v;
}

// shape rules of both directions; false = VITAMD_ERR_SHAPE.  side: tiles along one image side
inline bool conv_recon_plan(int B, int G, int p, int bf16, int& side, long& ntiles) {
  if (B < 1 || G < 1 || p < 1 || p % (bf16 ? 8 : 4) != 0) return false;
  if ((long)G * p > 46340 || (long)B * G * G > 0x7fffffffL || (long)p * p * 3 > 0x7fffffffL) return false;
  side = (G * p + CT - 1) / CT;
  ntiles = (long)B * side * side;
  return ntiles <= 0x7fffffffL;
}

inline bool conv_recon_ld_ok(int ld, int p, int bf16) { return (long)ld >= (long)p * p * 3 && ld % (bf16 ? 8 : 4) == 0; }

}  // namespace

extern "C" long vitamd_conv_recon_mse_ws_bytes(int B, int G, int p, int y_bf16, int backward) {
  int side;
  long ntiles;
  if (!conv_recon_plan(B, G, p, y_bf16, side, ntiles)) return -VITAMD_ERR_SHAPE;
  return ntiles * (backward ? CT_NW : 1) * (long)sizeof(float);
}

extern "C" int vitamd_conv_recon_mse_fwd(const void* y, int y_bf16, const float* w, const float* bias, const float* img, float* loss, float* recon,
                                         float* ws, int B, int G, int p, int ld, void* stream) {
  int side;
  long ntiles;
  if (!conv_recon_plan(B, G, p, y_bf16, side, ntiles) || !conv_recon_ld_ok(ld, p, y_bf16)) return VITAMD_ERR_SHAPE;
  if (!y || !w || !bias || !img || !loss || !ws) return VITAMD_ERR_ARG;
  if (!aligned16(y)) return VITAMD_ERR_SHAPE;           // the 16-byte path alone exists: the caller falls back
  hipStream_t s = (hipStream_t)stream;
  if (y_bf16) hipLaunchKernelGGL(conv_recon_fwd_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, s, y, w, bias, img, recon, ws, G, p, ld, side);
  else hipLaunchKernelGGL(conv_recon_fwd_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, s, y, w, bias, img, recon, ws, G, p, ld, side);
  const double E = (double)B * 3 * G * p * G * p;
  launch_sum_partials(ws, loss, ntiles, 1.0 / E, s);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_conv_recon_mse_bwd(const void* y, int y_bf16, const float* w, const float* bias, const float* img, const float* g_loss,
                                         const float* g_recon, void* dy, float* dw, float* db, float* ws, int B, int G, int p, int ld, int ld_dy,
                                         void* stream) {
  int side;
  long ntiles;
  if (!conv_recon_plan(B, G, p, y_bf16, side, ntiles) || !conv_recon_ld_ok(ld, p, y_bf16) || !conv_recon_ld_ok(ld_dy, p, y_bf16)) return VITAMD_ERR_SHAPE;
  if (!y || !w || !bias || !img || !dy || !dw || !db || !ws) return VITAMD_ERR_ARG;
  if (y == dy) return VITAMD_ERR_ARG;                   // never in place: a tile reads its neighbours' tokens
  if (!aligned16(y) || !aligned16(dy)) return VITAMD_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const float inv_n = (float)(1.0 / ((double)B * 3 * G * p * G * p));
  if (y_bf16)
    hipLaunchKernelGGL(conv_recon_bwd_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, s, y, w, bias, img, g_loss, g_recon, dy, ws, G, p, ld, ld_dy,
                       side, ntiles, inv_n);
  else
    hipLaunchKernelGGL(conv_recon_bwd_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, s, y, w, bias, img, g_loss, g_recon, dy, ws, G, p, ld, ld_dy,
                       side, ntiles, inv_n);
  hipLaunchKernelGGL(conv_wgrad_sum_kernel, dim3(CT_NW), dim3(256), 0, s, (const float*)ws, dw, db, ntiles);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
