// The device input pipeline: raw uint8 frames [Nsrc, Hs, Ws, C] (channels last, as decoders and video sets hand
// them over) -> the patch-embed GEMM's bf16 operand AND the fp32 NCHW image the tokenizers' losses take as their target, in one pass that
// reads every source byte once.  Frame gather (index), crop and horizontal flip (geom) are an index map; ToTensor + Normalize are a
// 256-entry table per channel, so the arithmetic of the reference's CPU transform is reproduced bit for bit by a lookup.
//
// A pure HBM stream: per pixel and channel 1 byte in, 4 (fp32) + 2 (bf16) bytes out.
// Fast form (C == 3, W % 4 == 0, p % 4 == 0 when patches are wanted): a lane owns 4 consecutive output pixels of one image row and all
// three channels - 12 contiguous source bytes (in reverse pixel order under a flip), one 16-byte fp32 store and one 8-byte bf16 store
// per channel.  Consecutive lanes walk an image row, as in im2col_kernel, when only the image is wanted, and (kw, 4 image rows, pw)
// when patch rows are: see the loop.  Source addresses are byte-aligned only (x0, Ws * 3 and the
// flip make every offset possible): the 12 bytes are taken from the four ALIGNED dwords that enclose them where src itself is 4-byte
// aligned and that window lies inside src, and by twelve byte loads otherwise (the last lanes of the last frame, an odd base pointer).
// Generic form: one lane per output element.
// Every device-side value is clamped before it forms an address: index into [0, Nsrc), y0 into [0, Hs-H], x0 into [0, Ws-W].
#include "common.h"
#include "frames_out.h"
#include "mix_row.h"

namespace {

constexpr int PREP_GRID_CAP = 2048;                  // workgroups per launch (8 per CU); further work is reached by the stride loop

struct Placement { const unsigned char* frame; int y0, x0, flip; };

// where output sample b reads: its (clamped) source frame and crop origin
__device__ __forceinline__ Placement place(const unsigned char* src, const long long* index, const int* geom, int b, int Nsrc, int Hs, int Ws,
                                           int C, int H, int W) {
  Placement pl = {source_frame(src, index, b, Nsrc, Hs, Ws, C), 0, 0, 0};
  if (geom) {
    const int* g = geom + (size_t)b * 3;
    pl.y0 = min(max(g[0], 0), Hs - H);
    pl.x0 = min(max(g[1], 0), Ws - W);
    pl.flip = g[2] != 0;
  }
  return pl;
}

// the 12 source bytes behind the 4 output pixels from column x of row y of a placed sample, as three little-endian words: the four
// ALIGNED dwords that enclose them where the window lies inside src (DWORDS: src itself is 4-byte aligned), twelve byte loads otherwise.
// The 4 source pixels are neighbours either way; under a flip output pixel j takes source pixel 3 - j.
template <bool DWORDS>
__device__ __forceinline__ void fetch12(const unsigned char* src, const Placement& pl, int y, int x, int Ws, int W, size_t src_bytes,
                                        unsigned (&w)[3]) {
  const int sx = pl.x0 + (pl.flip ? W - 4 - x : x);
  const unsigned char* s = pl.frame + ((size_t)(pl.y0 + y) * Ws + sx) * 3;
  const size_t off = (size_t)(s - src);
  if (DWORDS && (off & ~(size_t)3) + 16 <= src_bytes) {
    const unsigned* q = (const unsigned*)(src + (off & ~(size_t)3));
    const unsigned d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
    const unsigned sh = (unsigned)(off & 3) * 8;
    w[0] = (unsigned)((((uint64_t)d1 << 32) | d0) >> sh);
    w[1] = (unsigned)((((uint64_t)d2 << 32) | d1) >> sh);
    w[2] = (unsigned)((((uint64_t)d3 << 32) | d2) >> sh);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = s[4 * k] | (s[4 * k + 1] << 8) | (s[4 * k + 2] << 16) | ((unsigned)s[4 * k + 3] << 24);
  }
}

// channel c of those 4 pixels, in OUTPUT order
__device__ __forceinline__ f32x4 lookup4(const float* tab, const unsigned (&w)[3], int c, int flip) {
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 3 * j + c;                                       // byte of source pixel j, channel c
    const float val = tab[c * 256 + ((w[k >> 2] >> (8 * (k & 3))) & 0xffu)];
    if (flip) v[3 - j] = val; else v[j] = val;
  }
  return v;
}

// MIX: vitamd_frames_prep_mix.  The partner's 12 bytes are fetched only by the lanes one of whose pixels takes them (every lane of a
// mode-1 sample, the lanes whose 4 pixels meet the box of a mode-2 sample); a sample's mode is uniform over its lanes.
template <bool DWORDS, bool MIX>
__global__ __launch_bounds__(256) void frames_prep_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ index,
                                                          const int* __restrict__ geom, const float* __restrict__ table,
                                                          __bf16* __restrict__ patches, float* __restrict__ image, int B, int Nsrc, int Hs,
                                                          int Ws, int H, int W, int p, size_t src_bytes, const int* __restrict__ rec,
                                                          const float* __restrict__ lam) {
  __shared__ float tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = table[i];
  __syncthreads();
  const int w4 = W / 4;
  const unsigned per_sample = (unsigned)H * w4;
  const size_t total = (size_t)B * per_sample;
  const FramesOut out = {patches, image, H, W, 3, p, patches ? H / p : 0, patches ? W / p : 0, 3 * p * p};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    // one 64-bit division per item (the sample), 32-bit arithmetic inside the sample: the host keeps H * W / 4 below 2^31
    const int b = (int)(i / per_sample);
    unsigned t = (unsigned)(i - (size_t)b * per_sample);
    int x, y;
    if (patches) {
      // consecutive lanes walk (kw, 4 image rows, pw): the 4 rows of one patch are neighbours in its patch vector, so a bf16 store
      // instruction writes pieces of 4 * p * 2 bytes (whole 128-byte lines at p = 16) where a row-major walk writes p * 2, and
      // the fp32 stores still cover runs of whole patches of each row
      const unsigned p4 = p / 4;
      const int kw4 = (int)(t % p4); t /= p4;
      const int r = (int)(t & 3); t >>= 2;
      const int pw = (int)(t % (unsigned)out.gw); t /= (unsigned)out.gw;
      x = pw * p + kw4 * 4;
      y = (int)t * 4 + r;                                           // H % p == 0 and p % 4 == 0: rows come in fours
    } else {
      x = (int)(t % (unsigned)w4) * 4;
      y = (int)(t / (unsigned)w4);
    }
    const Placement pl = place(src, index, geom, b, Nsrc, Hs, Ws, 3, H, W);
    unsigned w[3];
    fetch12<DWORDS>(src, pl, y, x, Ws, W, src_bytes, w);
    MixRow mr = {};
    Placement plq = pl;
    unsigned wq[3] = {0u, 0u, 0u};
    bool take[4] = {false, false, false, false};                    // mode 2: which of the 4 pixels lie in the box
    if constexpr (MIX) {
      mr = mix_row(rec, lam, b, B, H, W);
      bool any = mr.mode == 1;
      if (mr.mode == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          take[j] = y >= mr.yl && y < mr.yh && x + j >= mr.xl && x + j < mr.xh;
          any |= take[j];
        }
      }
      if (any) {
        plq = place(src, index, geom, mr.q, Nsrc, Hs, Ws, 3, H, W);
        fetch12<DWORDS>(src, plq, y, x, Ws, W, src_bytes, wq);
      } else {
        mr.mode = 0;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4 v = lookup4(tab, w, c, pl.flip);
      if constexpr (MIX) {
        if (mr.mode != 0) {
          const f32x4 u = lookup4(tab, wq, c, plq.flip);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = mr.mode == 1 ? blend(v[j], u[j], mr.l, mr.m) : (take[j] ? u[j] : v[j]);
        }
      }
      out.store4(b, c, y, x, v);
    }
  }
}

// one table value: element (c, y, x) of a placed sample
__device__ __forceinline__ float fetch1(const float* tab, const Placement& pl, int c, int y, int x, int Ws, int C, int W) {
  const int sx = pl.x0 + (pl.flip ? W - 1 - x : x);
  return tab[c * 256 + pl.frame[((size_t)(pl.y0 + y) * Ws + sx) * C + c]];
}

template <bool MIX>
__global__ __launch_bounds__(256) void frames_prep_generic_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ index,
                                                                  const int* __restrict__ geom, const float* __restrict__ table,
                                                                  __bf16* __restrict__ patches, float* __restrict__ image, int B, int Nsrc,
                                                                  int Hs, int Ws, int C, int H, int W, int p, const int* __restrict__ rec,
                                                                  const float* __restrict__ lam) {
  __shared__ float tab[4 * 256];
  for (int i = threadIdx.x; i < C * 256; i += 256) tab[i] = table[i];
  __syncthreads();
  const size_t total = (size_t)B * C * H * W;
  const FramesOut out = {patches, image, H, W, C, p, patches ? H / p : 0, patches ? W / p : 0, C * p * p};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {      // i = the element of image
    size_t t = i;
    const int x = (int)(t % W); t /= W;
    const int y = (int)(t % H); t /= H;
    const int c = (int)(t % C);
    const int b = (int)(t / C);
    float v = fetch1(tab, place(src, index, geom, b, Nsrc, Hs, Ws, C, H, W), c, y, x, Ws, C, W);
    if constexpr (MIX) {
      const MixRow mr = mix_row(rec, lam, b, B, H, W);
      if (mr.mode == 1 || (mr.mode == 2 && y >= mr.yl && y < mr.yh && x >= mr.xl && x < mr.xh)) {
        const float u = fetch1(tab, place(src, index, geom, mr.q, Nsrc, Hs, Ws, C, H, W), c, y, x, Ws, C, W);
        v = mr.mode == 1 ? blend(v, u, mr.l, mr.m) : u;
      }
    }
    out.store1(i, b, c, y, x, v);
  }
}

// one lane per sample: (y0, x0, flip) from three words of Philox4x32-10, key = seed, counter = (b, 1, step)
__global__ __launch_bounds__(256) void crop_flip_draw_kernel(int* __restrict__ geom, int B, unsigned ny, unsigned nx, int flip, unsigned k0,
                                                             unsigned k1, unsigned s0, unsigned s1) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const u32x4 r = philox4x32_10((unsigned)b, 1u, s0, s1, k0, k1);
  geom[b * 3 + 0] = (int)(((uint64_t)r[0] * ny) >> 32);
  geom[b * 3 + 1] = (int)(((uint64_t)r[1] * nx) >> 32);
  geom[b * 3 + 2] = flip ? (int)(r[2] >> 31) : 0;
}

// rint(clamp(v, 0, 1) * 255), NaN -> 0 (fmaxf returns its other operand)
__device__ __forceinline__ unsigned to_u8(float v) { return (unsigned)__builtin_rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

// fp32 [B, C, H, W] -> uint8 [B, H, W, C].  A lane owns 4 neighbouring pixels: one 16-byte load per channel plane, and its 4 * C output
// bytes are C whole dwords at a 4-byte-aligned offset.
template <int C>
__global__ __launch_bounds__(256) void frames_to_u8_kernel(const float* __restrict__ img, unsigned* __restrict__ out, size_t groups, size_t hw4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
    const size_t b = i / hw4, g = i - b * hw4;
    unsigned bytes[4 * C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const f32x4 v = *(const f32x4*)(img + ((b * C + c) * hw4 + g) * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) bytes[j * C + c] = to_u8(v[j]);
    }
#pragma unroll
    for (int d = 0; d < C; ++d)
      out[i * C + d] = bytes[4 * d] | (bytes[4 * d + 1] << 8) | (bytes[4 * d + 2] << 16) | (bytes[4 * d + 3] << 24);
  }
}

__global__ __launch_bounds__(256) void frames_to_u8_generic_kernel(const float* __restrict__ img, unsigned char* __restrict__ out, size_t total,
                                                                   int C, size_t hw) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {       // i = the element of out
    const int c = (int)(i % C);
    const size_t px = i / C, b = px / hw, yx = px - b * hw;
    out[i] = (unsigned char)to_u8(img[(b * C + c) * hw + yx]);
  }
}

// the two entries: rec == nullptr launches the plain kernels
template <bool MIX>
int frames_prep(const unsigned char* src, const long long* index, const int* geom, const float* table, void* patches_bf16, float* image, int B,
                int Nsrc, int Hs, int Ws, int C, int H, int W, int p, const int* rec, const float* lam, void* stream) {
  long long n_src, n_out;
  if (H > Hs || W > Ws || frames_shape(patches_bf16 != nullptr, index != nullptr, B, Nsrc, Hs, Ws, C, H, W, p, &n_src, &n_out)) return VITAMD_ERR_SHAPE;
  if (!src || !table || (!patches_bf16 && !image) || (MIX && !rec)) return VITAMD_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const bool aligned = ((uintptr_t)image & 15) == 0 && ((uintptr_t)patches_bf16 & 7) == 0;      // of the 16- and 8-byte stores
  if (C == 3 && W % 4 == 0 && (!patches_bf16 || p % 4 == 0) && aligned && (long long)H * W / 4 < 0x7fffffffll) {
    const dim3 grid = capped_grid((size_t)n_out / 12, 256, PREP_GRID_CAP);
    if (((uintptr_t)src & 3) == 0)
      hipLaunchKernelGGL((frames_prep_kernel<true, MIX>), grid, dim3(256), 0, st, src, index, geom, table, (__bf16*)patches_bf16, image, B, Nsrc,
                         Hs, Ws, H, W, p, (size_t)n_src, rec, lam);
    else
      hipLaunchKernelGGL((frames_prep_kernel<false, MIX>), grid, dim3(256), 0, st, src, index, geom, table, (__bf16*)patches_bf16, image, B, Nsrc,
                         Hs, Ws, H, W, p, (size_t)n_src, rec, lam);
  } else {
    hipLaunchKernelGGL(frames_prep_generic_kernel<MIX>, capped_grid((size_t)n_out, 256, PREP_GRID_CAP), dim3(256), 0, st, src, index, geom, table,
                       (__bf16*)patches_bf16, image, B, Nsrc, Hs, Ws, C, H, W, p, rec, lam);
  }
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

}  // namespace

extern "C" int vitamd_frames_prep_grid_cap(void) { return PREP_GRID_CAP; }

extern "C" int vitamd_frames_prep(const unsigned char* src, const long long* index, const int* geom, const float* table, void* patches_bf16,
                                  float* image, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p, void* stream) {
  return frames_prep<false>(src, index, geom, table, patches_bf16, image, B, Nsrc, Hs, Ws, C, H, W, p, nullptr, nullptr, stream);
}

extern "C" int vitamd_frames_prep_mix(const unsigned char* src, const long long* index, const int* geom, const float* table,
                                      void* patches_bf16, float* image, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p,
                                      const int* rec, const float* lam, void* stream) {
  return frames_prep<true>(src, index, geom, table, patches_bf16, image, B, Nsrc, Hs, Ws, C, H, W, p, rec, lam, stream);
}

extern "C" int vitamd_crop_flip_draw(int* geom, int B, int Hs, int Ws, int H, int W, int flip, unsigned long long seed, unsigned long long step,
                                     void* stream) {
  if (B < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || H > Hs || W > Ws || B > 0x7fffffff / 3) return VITAMD_ERR_SHAPE;
  if (!geom) return VITAMD_ERR_ARG;
  hipLaunchKernelGGL(crop_flip_draw_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, geom, B, (unsigned)(Hs - H + 1),
                     (unsigned)(Ws - W + 1), flip, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)step, (unsigned)(step >> 32));
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_frames_to_u8(const float* img, unsigned char* out, int B, int C, int H, int W, void* stream) {
  if (B < 1 || C < 1 || C > 4 || H < 1 || W < 1) return VITAMD_ERR_SHAPE;
  const long long n = count(B, C, H, W);
  if (n < 0) return VITAMD_ERR_SHAPE;
  if (!img || !out) return VITAMD_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const size_t hw = (size_t)H * W;
  if (hw % 4 == 0 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 3) == 0) {
    const size_t groups = (size_t)B * (hw / 4);
    const dim3 grid = capped_grid(groups, 256, PREP_GRID_CAP);
    unsigned* o = (unsigned*)out;
    if (C == 1) hipLaunchKernelGGL(frames_to_u8_kernel<1>, grid, dim3(256), 0, st, img, o, groups, hw / 4);
    else if (C == 2) hipLaunchKernelGGL(frames_to_u8_kernel<2>, grid, dim3(256), 0, st, img, o, groups, hw / 4);
    else if (C == 3) hipLaunchKernelGGL(frames_to_u8_kernel<3>, grid, dim3(256), 0, st, img, o, groups, hw / 4);
    else hipLaunchKernelGGL(frames_to_u8_kernel<4>, grid, dim3(256), 0, st, img, o, groups, hw / 4);
  } else {
    hipLaunchKernelGGL(frames_to_u8_generic_kernel, capped_grid((size_t)n, 256, PREP_GRID_CAP), dim3(256), 0, st, img, out, (size_t)n, C, hw);
  }
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
