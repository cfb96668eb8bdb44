// Random Erasing on the finished batch of the device input feed: a post-pass over the outputs of the four frame
// kernels (input.hip, resize.hip) that rewrites ONLY the erased boxes, in place, through the one statement of where a pixel lives
// (frames_out.h).  rec int32 [B, K, 5] = (mode, yl, yh, xl, xh) names up to K boxes per sample; mode 1 writes fill[b, k, c], mode 2 an
// N(0, 1) value per pixel and channel that is a pure function of (seed, step, b, c, y, x).
//
// Work is proportional to the erased area: a workgroup is given (sample, box, strip of the box) and walks only the aligned groups of 4
// pixels that meet its box; a (sample, box) without a box costs its workgroups one record read each.  SINGLE WRITER: a pixel covered by
// several boxes of its sample is written by the box with the largest k alone - box k skips every pixel a later box covers - so no
// element has two writers, nothing is read back, and the bits do not depend on the order the workgroups run in.
// Every device-side value is clamped before it forms an address: yl, yh into [0, H], xl, xh into [0, W].
#include "common.h"
#include "frames_out.h"

namespace {

constexpr int ERASE_GRID_CAP = 2048;                 // workgroups per launch (8 per CU); further (sample, box, strip) units by the stride loop
constexpr int ERASE_STRIPS = 32;                     // workgroups that share one box: a lane of the recipe's largest box (a third of 224 x 224) has 2 groups
constexpr int ERASE_MAX_K = VITAMD_ERASE_MAX_BOXES;

struct EraseBox { int mode, yl, yh, xl, xh; };

// box `bk` (= b * K + k) of the record, clamped; an empty box and a mode outside {1, 2} are mode 0
__device__ __forceinline__ EraseBox erase_box(const int* __restrict__ rec, size_t bk, int H, int W) {
  const int* r = rec + bk * 5;
  EraseBox bx = {r[0], min(max(r[1], 0), H), min(max(r[2], 0), H), min(max(r[3], 0), W), min(max(r[4], 0), W)};
  if ((bx.mode != 1 && bx.mode != 2) || bx.yl >= bx.yh || bx.xl >= bx.xh) bx.mode = 0;
  return bx;
}

// the four N(0, 1) values of pixels 4 * (x >> 2) .. + 3 of row y, channel c, sample b: one Philox call, two Box-Muller pairs
__device__ __forceinline__ f32x4 erase_noise4(unsigned c0, unsigned c1, unsigned s0, unsigned s1, unsigned k0, unsigned k1) {
  const u32x4 w = philox4x32_10(c0, c1, s0, s1, k0, k1);
  f32x4 z;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float u1 = (float)((w[2 * i] >> 8) + 1u) * 0x1p-24f;      // (0, 1]: integers up to 2^24 and the power of two are exact
    const float u2 = (float)(w[2 * i + 1] >> 8) * 0x1p-24f;         // [0, 1)
    const float r = sqrtf(-2.f * logf(u1));
    float s, c;
    sincospif(2.f * u2, &s, &c);
    z[2 * i] = r * c;
    z[2 * i + 1] = r * s;
  }
  return z;
}

// FAST: W % 4 == 0, p % 4 == 0 where patch rows are written, image 16-byte and patches 8-byte aligned - a group wholly its box's goes
// out through store4.  Otherwise, and for the groups a box edge or a later box cuts, store1 per pixel.
template <bool FAST>
__global__ __launch_bounds__(256) void frames_erase_kernel(__bf16* __restrict__ patches, float* __restrict__ image, int B, int C, int H, int W,
                                                           int p, const int* __restrict__ rec, const float* __restrict__ fill, int K, unsigned k0,
                                                           unsigned k1, unsigned s0, unsigned s1) {
  const FramesOut out = {patches, image, H, W, C, p, patches ? H / p : 0, patches ? W / p : 0, C * p * p};
  const unsigned w4 = (unsigned)(((long long)W + 3) / 4);
  const size_t units = (size_t)B * K * ERASE_STRIPS;
  for (size_t u = blockIdx.x; u < units; u += gridDim.x) {            // u, and with it everything up to the item loop, is workgroup-uniform
    const int strip = (int)(u % ERASE_STRIPS);
    const size_t bk = u / ERASE_STRIPS;
    const int b = (int)(bk / (unsigned)K), k = (int)(bk - (size_t)b * K);
    const EraseBox bx = erase_box(rec, bk, H, W);
    if (bx.mode == 0) continue;
    const int g0 = bx.xl >> 2, ng = ((bx.xh + 3) >> 2) - g0, h = bx.yh - bx.yl;
    const size_t items = (size_t)C * h * ng;                         // aligned groups of 4 pixels that meet the box, per channel and row
    for (size_t t = (size_t)strip * 256 + threadIdx.x; t < items; t += (size_t)ERASE_STRIPS * 256) {
      // t < items <= C * H * ceil(W / 4) <= 2^32 (the entry's refusal): 32-bit divisions inside the box
      const unsigned cr = (unsigned)t / (unsigned)ng, g = (unsigned)t - cr * (unsigned)ng;
      const int c = (int)(cr / (unsigned)h), y = bx.yl + (int)(cr - (unsigned)c * (unsigned)h), x0 = (g0 + (int)g) * 4;
      unsigned mine = 0;                                             // bit j: pixel x0 + j is this box's to write
#pragma unroll
      for (int j = 0; j < 4; ++j) mine |= (unsigned)(x0 + j >= bx.xl && x0 + j < bx.xh) << j;
      for (int l = k + 1; l < K; ++l) {                              // a later box of the sample wins its pixels
        const EraseBox lb = erase_box(rec, (size_t)b * K + l, H, W);
        if (lb.mode == 0 || y < lb.yl || y >= lb.yh) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j >= lb.xl && x0 + j < lb.xh) mine &= ~(1u << j);
      }
      if (mine == 0) continue;
      f32x4 v;
      if (bx.mode == 1) {
        const float f = fill ? fill[bk * 4 + c] : 0.f;
        v = f32x4{f, f, f, f};
      } else {
        v = erase_noise4((unsigned)(((size_t)c * H + y) * w4 + (unsigned)(x0 >> 2)), ((unsigned)b << 2) | 2u, s0, s1, k0, k1);
      }
      if (FAST && mine == 15u) {
        out.store4(b, c, y, x0, v);
      } else {
        const size_t i0 = (((size_t)b * C + c) * H + y) * W + x0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (mine & (1u << j)) out.store1(i0 + j, b, c, y, x0 + j, v[j]);
      }
    }
  }
}

}  // namespace

extern "C" int vitamd_frames_erase_grid_cap(void) { return ERASE_GRID_CAP; }

extern "C" int vitamd_frames_erase(void* patches_bf16, float* image, int B, int C, int H, int W, int p, const int* rec, const float* fill, int K,
                                   unsigned long long seed, unsigned long long step, void* stream) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || C > 4 || K < 1 || K > ERASE_MAX_K) return VITAMD_ERR_SHAPE;
  if (patches_bf16 && (p < 1 || H % p != 0 || W % p != 0)) return VITAMD_ERR_SHAPE;
  // B * C * H * W: every index of the outputs; B << 2 and (c * H + y) * ceil(W / 4) + (x >> 2): the two counter words of the noise
  if (count(B, C, H, W) < 0 || B >= (1 << 30) || (long long)C * H * (((long long)W + 3) / 4) > (1ll << 32)) return VITAMD_ERR_SHAPE;
  if (!rec || (!patches_bf16 && !image)) return VITAMD_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid = capped_grid((size_t)B * K * ERASE_STRIPS, 1, ERASE_GRID_CAP);
  const bool fast = W % 4 == 0 && (!patches_bf16 || p % 4 == 0) && ((uintptr_t)image & 15) == 0 && ((uintptr_t)patches_bf16 & 7) == 0;
  if (fast)
    hipLaunchKernelGGL(frames_erase_kernel<true>, grid, dim3(256), 0, st, (__bf16*)patches_bf16, image, B, C, H, W, p, rec, fill, K, (unsigned)seed,
                       (unsigned)(seed >> 32), (unsigned)step, (unsigned)(step >> 32));
  else
    hipLaunchKernelGGL(frames_erase_kernel<false>, grid, dim3(256), 0, st, (__bf16*)patches_bf16, image, B, C, H, W, p, rec, fill, K, (unsigned)seed,
                       (unsigned)(seed >> 32), (unsigned)step, (unsigned)(step >> 32));
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
