// What the frame kernels of the input feed (input.hip, resize.hip) share besides mix_row.h: the shape checks of their entries, the grid
// cap, the clamped source frame of a sample and - stated once, so the feeds cannot drift apart - WHERE a pixel is stored.
#pragma once
#include "common.h"
#include "../../include/vitamd.h"

constexpr long long MAX_ELEMS = 1ll << 40;           // per tensor: keeps every product of the index arithmetic inside 64 bits
// the element count of a tensor, or -1 beyond MAX_ELEMS (checked factor by factor: four ints can overflow 64 bits)
static inline long long count(int a, int b, int c, int d) {
  long long n = a;
  for (const int f : {b, c, d}) {
    n *= f;
    if (n > MAX_ELEMS) return -1;
  }
  return n;
}

// the shape rules every frame entry has, ahead of its pointer checks -> VITAMD_OK and the two element counts, or VITAMD_ERR_SHAPE
static inline int frames_shape(bool want_patches, bool has_index, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p, long long* n_src, long long* n_out) {
  if (B < 1 || Nsrc < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || C < 1 || C > 4) return VITAMD_ERR_SHAPE;
  if ((want_patches && (p < 1 || H % p != 0 || W % p != 0)) || (!has_index && Nsrc < B)) return VITAMD_ERR_SHAPE;
  *n_src = count(Nsrc, Hs, Ws, C), *n_out = count(B, C, H, W);
  return *n_src < 0 || *n_out < 0 ? VITAMD_ERR_SHAPE : VITAMD_OK;
}

// workgroups for `items` of work at `per_wg` each, at most `cap`: what lies beyond is reached by the kernels' stride loops
static inline dim3 capped_grid(size_t items, size_t per_wg, int cap) {
  return dim3((unsigned)std::min((items + per_wg - 1) / per_wg, (size_t)cap));
}

// the source frame of output sample b: index[b] (b itself without an index), clamped into [0, Nsrc)
__device__ __forceinline__ const unsigned char* source_frame(const unsigned char* src, const long long* index, int b, int Nsrc, int Hs, int Ws, int C) {
  long long f = index ? index[b] : b;
  f = f < 0 ? 0 : (f > Nsrc - 1 ? Nsrc - 1 : f);
  return src + (size_t)f * Hs * Ws * C;
}

// The outputs of a frame kernel, either of which may be NULL: image fp32 [B, C, H, W] and patches bf16 [B*gh*gw, pd = C*p*p], the rows
// ops.im2col makes of that image.  A kernel fills it as {patches, image, H, W, C, p, patches ? H / p : 0, patches ? W / p : 0, C * p * p}.
struct FramesOut {
  __bf16* patches; float* image; int H, W, C, p, gh, gw, pd;
  __device__ __forceinline__ __bf16* row_at(int b, int c, int y, int x) const {
    const int ph = y / p, kh = y - ph * p, pw = x / p, kw = x - pw * p;
    return patches + (((size_t)b * gh + ph) * gw + pw) * pd + (c * p + kh) * p + kw;
  }
  // the fast forms: pixels x .. x + 3 of a row (x, W and p multiples of 4, aligned bases) as one 16-byte fp32 and one 8-byte bf16 store
  __device__ __forceinline__ void store4(int b, int c, int y, int x, f32x4 v) const {
    if (image) *(f32x4*)(image + (((size_t)b * C + c) * H + y) * W + x) = v;
    if (patches) *(u32x2*)row_at(b, c, y, x) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
  }
  // the generic forms: one element, i = its index in the image, (((b * C + c) * H + y) * W + x), which these kernels walk
  __device__ __forceinline__ void store1(size_t i, int b, int c, int y, int x, float v) const {
    if (image) image[i] = v;
    if (patches) *row_at(b, c, y, x) = f2bf(v);
  }
};
