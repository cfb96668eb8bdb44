// The narrow nearest-code scan (code width d <= DMAX <= 64) of vq_nearest_kernel, vq_nearest_chunk_kernel (csrc/misc.hip) and
// vq_search_kernel (csrc/tokenizer.hip): the three give the same index for the same rows because they run this one loop.
#pragma once
#include "common.h"

struct VqBest { float dist; int index; };     // the smallest distance so far and the FIRST code that has it

// One chunk of nk <= 256 codes, e[k0 .. k0 + nk): the workgroup (256 threads, every one of them calls) stages it in ce[256 * DMAX],
// synchronises, and each thread scans it for its row xr - sum over ascending c of (xr_c - e_kc)^2, strict <, so an earlier code keeps a
// tie.  The caller synchronises before ce is staged again.  The state goes in and out by value: passed by reference it costs the
// kernels a compare, two selects and more SGPR spills (profiles/tokenizer_shared_source/README.md).
template <int DMAX>
__device__ __forceinline__ VqBest vq_scan_chunk(float* ce, const float (&xr)[DMAX], const float* __restrict__ e, int k0, int nk, int d, VqBest b) {
  for (int i = threadIdx.x; i < nk * d; i += 256) ce[(i / d) * DMAX + (i % d)] = e[(size_t)k0 * d + i];
  __syncthreads();
  for (int k = 0; k < nk; ++k) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DMAX; ++c) {
      if (c < d) { const float t = xr[c] - ce[k * DMAX + c]; s += t * t; }
    }
    if (s < b.dist) { b.dist = s; b.index = k0 + k; }
  }
  return b;
}
