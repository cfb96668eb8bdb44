// The kernels of the ConvNeXt-S perceptual loss (reference perceptual_loss.py) that are not a GEMM or a row LayerNorm:
//
//  * the depthwise 7x7 convolution of a ConvNeXt block (stride 1, zero padding 3) on CHANNELS-LAST rows [B*H*W, C], forward and input
//    gradient from one body (FLIP, as conv3x3.hip).  49 FMAs per output and no reuse across channels: VALU work, not a GEMM.  Lanes run
//    along channels (16 lanes x 4 channels = 256 contiguous bytes of a pixel), a thread owns DW_TW output pixels of one image row and walks
//    the DW_TW + 6 input pixels under them once per kernel row: every value loaded feeds up to 7 FMAs per channel from registers.  The
//    [C,49] weights of the workgroup's 64 channels (reversed for FLIP, so both directions run the same correlation) and the bias are staged
//    in LDS once.  The network is frozen: there is no weight gradient.
//  * the antialiased bilinear resize + ImageNet normalisation in front of the network, forward and backward.  The resize is separable,
//    out = Wh . img . Ww^T per channel, and each row of Wh / Ww holds a few contiguous non-zero taps; the host builds the band tables
//    (first tap index + T weights per output index, zero-padded) once per (n_in, n_out) and both kernels are the same band product on
//    different tables and layouts: the backward takes the tables of the TRANSPOSED matrices.  No atomics: every result is reproducible.
//    The forward writes the operand of the 4x4 stride-4 stem convolution directly: bf16 patch rows [B*(S/4)^2, 64], column
//    c*16 + kh*4 + kw (the contraction order of the Conv2d weight), columns 48..63 zero (the GEMM wants K % 64 == 0).
#include "common.h"
#include "vitamd_internal.h"
#include "../../include/vitamd.h"

namespace {

constexpr int DW_TW = 8;     // output pixels along W per thread
constexpr int DW_CT = 64;    // channels per workgroup: 16 lanes x 4
constexpr int DW_SEGS = 16;  // W-segments (of DW_TW pixels) per 256-thread workgroup

__device__ __forceinline__ f32x4 load4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 load4(const __bf16* p) {
  const u32x2 u = *(const u32x2*)p;
  return f32x4{bf16lo(u[0]), __builtin_bit_cast(float, u[0] & 0xffff0000u), bf16lo(u[1]), __builtin_bit_cast(float, u[1] & 0xffff0000u)};
}

template <typename TIN, bool FLIP>
__global__ __launch_bounds__(256, 3) void dwconv7_kernel(const TIN* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ add, float* __restrict__ y, int B, int H, int W, int C) {
  // FLIP = false: y[b,h,w,c] = bias[c] + sum_kh,kw w[c,kh,kw] * x[b,h+kh-3,w+kw-3,c]
  // FLIP = true : y[b,h,w,c] = add[b,h,w,c] + sum_kh,kw w[c,kh,kw] * x[b,h+3-kh,w+3-kw,c]   (input gradient; x = dy) - the same
  //               correlation with the 49 taps stored in reverse order
  __shared__ float ws[49 * DW_CT];   // [tap][channel]
  __shared__ float bs[DW_CT];
  const int c0 = blockIdx.y * DW_CT;
  for (int i = threadIdx.x; i < 49 * DW_CT; i += 256) {
    const int c = i / 49, k = i - c * 49;
    ws[(FLIP ? 48 - k : k) * DW_CT + c] = (c0 + c < C) ? w[(size_t)(c0 + c) * 49 + k] : 0.f;
  }
  if (threadIdx.x < DW_CT) bs[threadIdx.x] = (bias && c0 + (int)threadIdx.x < C) ? bias[c0 + threadIdx.x] : 0.f;
  __syncthreads();
  const int cg = threadIdx.x & 15;
  const int c = c0 + cg * 4;
  const int segs_w = (W + DW_TW - 1) / DW_TW;
  const long long seg = (long long)blockIdx.x * DW_SEGS + (threadIdx.x >> 4);
  if (c >= C || seg >= (long long)B * H * segs_w) return;
  const int sw = (int)(seg % segs_w);
  const long long bh = seg / segs_w;          // = b * H + h
  const int h = (int)(bh % H);
  const int w0 = sw * DW_TW;
  f32x4 acc[DW_TW];
  const f32x4 b4 = *(const f32x4*)(bs + cg * 4);
#pragma unroll
  for (int t = 0; t < DW_TW; ++t) acc[t] = b4;
#pragma unroll 1
  for (int kh = 0; kh < 7; ++kh) {
    const int hh = h + kh - 3;
    if (hh >= 0 && hh < H) {
      f32x4 wk[7];
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) wk[kw] = *(const f32x4*)(ws + (kh * 7 + kw) * DW_CT + cg * 4);
      const TIN* row = x + ((size_t)(bh + (kh - 3)) * W) * C + c;
      // straight-line body: a pixel outside the row is loaded from a clamped (valid) address and replaced by zero
#pragma unroll
      for (int j = 0; j < DW_TW + 6; ++j) {
        const int iw = w0 + j - 3;
        const bool ok = iw >= 0 && iw < W;
        f32x4 v = load4(row + (size_t)(ok ? iw : w0) * C);
        if (!ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < DW_TW; ++t) {
          const int kw = j - t;                 // input pixel w0+j-3 = (w0+t) + kw - 3
          if (kw >= 0 && kw < 7) acc[t] += wk[kw] * v;
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < DW_TW; ++t) {
    const int ow = w0 + t;
    if (ow < W) {
      const size_t o = ((size_t)bh * W + ow) * C + c;
      f32x4 r = acc[t];
      if (add) r += *(const f32x4*)(add + o);
      *(f32x4*)(y + o) = r;
    }
  }
}

template <typename TIN, bool FLIP>
int launch_dwconv7(const void* x, const float* w, const float* bias, const float* add, float* y, int B, int H, int W, int C, hipStream_t s) {
  const long long segs = (long long)B * H * ((W + DW_TW - 1) / DW_TW);
  const long long gx = (segs + DW_SEGS - 1) / DW_SEGS;
  const int gy = (C + DW_CT - 1) / DW_CT;
  if (gx > 0x7fffffffLL || gy > 65535) return VITAMD_ERR_SHAPE;
  hipLaunchKernelGGL((dwconv7_kernel<TIN, FLIP>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, (const TIN*)x, w, bias, add, y, B, H, W, C);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

int dwconv7_check(const void* x, const float* w, const float* y, int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 != 0) return VITAMD_ERR_SHAPE;
  if ((unsigned long long)B * H * W * C >= (1ull << 40)) return VITAMD_ERR_SHAPE;
  if (!x || !w || !y) return VITAMD_ERR_ARG;
  return VITAMD_OK;
}

// ---- resize + normalise ------------------------------------------------------------------------------------------------------------
// patch-row coordinates of element (c, oh, ow) of image b of the S x S normalised image: row b*(S/4)^2 + (oh/4)*(S/4) + ow/4,
// column c*16 + (oh%4)*4 + ow%4
__device__ __forceinline__ size_t patch_index(int b, int c, int oh, int ow, int S, int ld) {
  const int P = S >> 2;
  return ((size_t)b * P * P + (size_t)(oh >> 2) * P + (ow >> 2)) * ld + c * 16 + (oh & 3) * 4 + (ow & 3);
}

__global__ __launch_bounds__(256) void resize_norm_fwd_kernel(const float* __restrict__ img, const int* __restrict__ sh, const float* __restrict__ wh,
                                                              int Th, const int* __restrict__ sw, const float* __restrict__ ww, int Tw,
                                                              const float* __restrict__ mean, const float* __restrict__ stdv,
                                                              __bf16* __restrict__ rows, float* __restrict__ nchw, int B, int Hin, int Win, int S) {
  // one thread per element of the patch rows [B*(S/4)^2, 64]; columns >= 48 are the zero padding
  const int P = S >> 2;
  const size_t total = (size_t)B * P * P * 64;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i & 63);
    if (k >= 48) {
      if (rows) rows[i] = (__bf16)0.f;
      continue;
    }
    const size_t m = i >> 6;
    const int b = (int)(m / ((size_t)P * P));
    const int pr = (int)(m - (size_t)b * P * P);
    const int c = k >> 4, oh = (pr / P) * 4 + ((k >> 2) & 3), ow = (pr % P) * 4 + (k & 3);
    const float* src = img + ((size_t)b * 3 + c) * Hin * Win + (size_t)sh[oh] * Win + sw[ow];
    const float* wr = wh + (size_t)oh * Th;
    const float* wc = ww + (size_t)ow * Tw;
    float acc = 0.f;
    for (int a = 0; a < Th; ++a) {
      float r = 0.f;
      for (int t = 0; t < Tw; ++t) r += wc[t] * src[(size_t)a * Win + t];
      acc += wr[a] * r;
    }
    const float v = (acc - mean[c]) / stdv[c];
    if (rows) rows[i] = (__bf16)v;
    if (nchw) nchw[(((size_t)b * 3 + c) * S + oh) * S + ow] = v;
  }
}

__global__ __launch_bounds__(256) void resize_norm_bwd_kernel(const float* __restrict__ g, int ldg, const int* __restrict__ sh,
                                                              const float* __restrict__ wh, int Th, const int* __restrict__ sw,
                                                              const float* __restrict__ ww, int Tw, const float* __restrict__ stdv,
                                                              float* __restrict__ dimg, int B, int Hin, int Win, int S) {
  // one thread per input pixel: dimg[b,c,ih,iw] = (1/std[c]) sum_a sum_t WhT[ih,a] WwT[iw,t] g[b,c,sh[ih]+a,sw[iw]+t] (g in patch-row layout)
  const size_t hw = (size_t)Hin * Win, total = (size_t)B * 3 * hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int bc = (int)(i / hw);
    const int r = (int)(i - (size_t)bc * hw);
    const int b = bc / 3, c = bc - b * 3;
    const int ih = r / Win, iw = r - ih * Win;
    const int oh0 = sh[ih], ow0 = sw[iw];
    const float* wr = wh + (size_t)ih * Th;
    const float* wc = ww + (size_t)iw * Tw;
    float acc = 0.f;
    for (int a = 0; a < Th; ++a) {
      float s = 0.f;
      for (int t = 0; t < Tw; ++t) s += wc[t] * g[patch_index(b, c, oh0 + a, ow0 + t, S, ldg)];
      acc += wr[a] * s;
    }
    dimg[i] = acc / stdv[c];
  }
}

int grid_for(size_t total) {
  size_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

int resize_check(int B, int C, int Hin, int Win, int S, int Th, int Tw, int n_h, int n_w) {
  if (B <= 0 || C != 3 || Hin <= 0 || Win <= 0 || S <= 0 || S % 4 != 0) return VITAMD_ERR_SHAPE;
  if (Th <= 0 || Tw <= 0 || Th > n_h || Tw > n_w) return VITAMD_ERR_SHAPE;      // a band of T taps starting at index <= n - T stays inside
  if ((unsigned long long)B * 3 * Hin * Win >= (1ull << 40) || (unsigned long long)B * S * S * 16 >= (1ull << 40)) return VITAMD_ERR_SHAPE;
  return VITAMD_OK;
}

}  // namespace

extern "C" int vitamd_dwconv7_fwd(const void* x, int x_bf16, const float* w, const float* bias, float* y, int B, int H, int W, int C, void* stream) {
  if (int e = dwconv7_check(x, w, y, B, H, W, C)) return e;
  hipStream_t s = (hipStream_t)stream;
  return x_bf16 ? launch_dwconv7<__bf16, false>(x, w, bias, nullptr, y, B, H, W, C, s) : launch_dwconv7<float, false>(x, w, bias, nullptr, y, B, H, W, C, s);
}

extern "C" int vitamd_dwconv7_bwd(const void* dy, int dy_bf16, const float* w, const float* add, float* dx, int B, int H, int W, int C, void* stream) {
  if (int e = dwconv7_check(dy, w, dx, B, H, W, C)) return e;
  if (add && (const void*)add == (const void*)dy) return VITAMD_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  return dy_bf16 ? launch_dwconv7<__bf16, true>(dy, w, nullptr, add, dx, B, H, W, C, s) : launch_dwconv7<float, true>(dy, w, nullptr, add, dx, B, H, W, C, s);
}

extern "C" int vitamd_resize_norm_fwd(const float* img, const int* start_h, const float* taps_h, int Th, const int* start_w, const float* taps_w, int Tw,
                                      const float* mean, const float* stdv, void* rows_bf16, float* nchw, int B, int C, int Hin, int Win, int S,
                                      void* stream) {
  if (int e = resize_check(B, C, Hin, Win, S, Th, Tw, Hin, Win)) return e;
  if (!img || !start_h || !taps_h || !start_w || !taps_w || !mean || !stdv || (!rows_bf16 && !nchw)) return VITAMD_ERR_ARG;
  hipLaunchKernelGGL(resize_norm_fwd_kernel, dim3(grid_for((size_t)B * S * S * 4)), dim3(256), 0, (hipStream_t)stream, img, start_h, taps_h, Th, start_w,
                     taps_w, Tw, mean, stdv, (__bf16*)rows_bf16, nchw, B, Hin, Win, S);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_resize_norm_bwd(const float* g_rows, int ldg, const int* start_h, const float* taps_h, int Th, const int* start_w,
                                      const float* taps_w, int Tw, const float* stdv, float* dimg, int B, int C, int Hin, int Win, int S, void* stream) {
  if (int e = resize_check(B, C, Hin, Win, S, Th, Tw, S, S)) return e;
  if (ldg < 48) return VITAMD_ERR_SHAPE;
  if (!g_rows || !start_h || !taps_h || !start_w || !taps_w || !stdv || !dimg) return VITAMD_ERR_ARG;
  hipLaunchKernelGGL(resize_norm_bwd_kernel, dim3(grid_for((size_t)B * 3 * Hin * Win)), dim3(256), 0, (hipStream_t)stream, g_rows, ldg, start_h, taps_h, Th,
                     start_w, taps_w, Tw, stdv, dimg, B, Hin, Win, S);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
