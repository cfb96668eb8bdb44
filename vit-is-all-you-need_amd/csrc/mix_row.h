// The mix record of the mixing input feeds (vitamd_frames_prep_mix in input.hip, vitamd_frames_prep_resize_mix in resize.hip) and the
// blend both apply: one statement of the clamps and of the three roundings, so the two feeds cannot drift apart.
#pragma once
#include "common.h"

// The mix record of output sample b (vitamd_frames_prep_mix), clamped: partner into [0, B), the box into the image, a mode outside
// {1, 2} or a sample that is its own partner = mode 0.  lam is read for mode 1 only (NULL: l = 1).
struct MixRow { int q, mode, yl, yh, xl, xh; float l, m; };

__device__ __forceinline__ MixRow mix_row(const int* rec, const float* lam, int b, int B, int H, int W) {
  const int* r = rec + (size_t)b * 6;
  MixRow mr;
  mr.q = min(max(r[0], 0), B - 1);
  const int mode = r[1];
  mr.mode = (mode == 1 || mode == 2) && mr.q != b ? mode : 0;
  mr.yl = min(max(r[2], 0), H);
  mr.yh = min(max(r[3], 0), H);
  mr.xl = min(max(r[4], 0), W);
  mr.xh = min(max(r[5], 0), W);
  mr.l = mr.mode == 1 && lam ? lam[b] : 1.f;
  mr.m = __fsub_rn(1.f, mr.l);
  return mr;
}

// fl(fl(a * l) + fl(p * m)): three roundings, the bits of torch's a.mul(l).add(p.mul(m)).  hipcc would contract a * l + p * m into a
// fused multiply-add (one rounding fewer), also through __fmul_rn / __fadd_rn, which are the plain operators: the empty asm statements
// make each product a value of its own before the sum.
__device__ __forceinline__ float blend(float a, float p, float l, float m) {
  float al = __fmul_rn(a, l), pm = __fmul_rn(p, m);
  asm volatile("" : "+v"(al), "+v"(pm));
  return __fadd_rn(al, pm);
}
