// Sequence assembly of the code-id TiTok: E learned rows in front of S rows that each get their position added,
// forward and backward.  x fp32 [B, E+S, D]: x[b, e] = prefix[e] (e < E), x[b, E+t] = src(b, t) + pos[t], src either a row of a token
// table picked by an id (gather mode) or a row of a dense body [B, S, D] (dense mode).  Both kernels are one pass over x / its gradient
// in 16-byte accesses, with capped grids and a stride loop beyond the cap.
//
// Forward: one lane per 4 columns, one fp32 add per element (the bits of the framework's gather / add / cat).  An id outside the table
// leaves its row alone; no table is read out of bounds.
// Backward: a wave owns (position p, 256 columns) and walks the batch in ascending order, 8 rows of loads in flight: the running sum
// goes to dprefix[p] or dpos[p - E], which no other wave touches - no atomics, the same bits every call.  In gather mode each row is
// also added to dtok[id] by fp32 atomics.  A lane holds 4 neighbouring columns, which as they stand would make every atomic
// wave-instruction 64 pieces of 4 bytes at a 16-byte stride; the wave passes its 1-KiB row piece through a slab of LDS of its own
// instead and adds it as four instructions of 64 contiguous floats, the shape the memory side takes at full rate.
#include "common.h"
#include "../../include/vitamd.h"

namespace {

constexpr int ASM_GRID_CAP = 2048;    // workgroups per launch (8 per CU); further work is reached by the stride loop
constexpr int ASM_ROWS = 8;           // batch rows a backward wave has in flight

template <bool GATHER>
__global__ __launch_bounds__(256) void assemble_tokens_fwd_kernel(const float* __restrict__ prefix, const float* __restrict__ pos,
                                                                 const float* __restrict__ tok, const long long* __restrict__ ids,
                                                                 const float* __restrict__ body, float* __restrict__ x, long n4, int E, int S,
                                                                 int D, int tok_rows) {
  const int dq = D / 4, T = E + S;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long r = i / dq;                      // row of x: b * T + p
    const int c = (int)(i - r * dq) * 4;
    const long b = r / T;
    const int p = (int)(r - b * T);
    f32x4 v;
    if (p < E) {
      v = *(const f32x4*)(prefix + (size_t)p * D + c);
    } else {
      const int t = p - E;
      const size_t br = (size_t)b * S + t;      // row of ids / body
      f32x4 a;
      if constexpr (GATHER) {
        const long long id = ids[br];
        if (id < 0 || id >= tok_rows) continue;
        a = *(const f32x4*)(tok + (size_t)id * D + c);
      } else {
        a = *(const f32x4*)(body + br * D + c);
      }
      v = a + *(const f32x4*)(pos + (size_t)t * D + c);
    }
    *(f32x4*)(x + (size_t)r * D + c) = v;
  }
}

template <bool GATHER>
__global__ __launch_bounds__(256) void assemble_tokens_bwd_kernel(const float* __restrict__ g, const long long* __restrict__ ids,
                                                                 float* __restrict__ dprefix, float* __restrict__ dpos, float* __restrict__ dtok,
                                                                 int B, int E, int S, int D, int tok_rows, long items, int cblocks) {
  __shared__ float slab[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* mine = slab[w];
  const size_t T = (size_t)(E + S);
  for (long it = (long)blockIdx.x * 4 + w; it < items; it += (long)gridDim.x * 4) {     // wave-uniform
    const int p = (int)(it / cblocks);
    const int c0 = (int)(it - (long)p * cblocks) * 256;
    const int c = c0 + lane * 4;
    const bool live = c < D;
    const float* gp = g + (size_t)p * D + c;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += ASM_ROWS) {
      f32x4 v[ASM_ROWS];
      long long id[ASM_ROWS];
#pragma unroll
      for (int k = 0; k < ASM_ROWS; ++k) {
        v[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        id[k] = -1;
        if (b0 + k < B) {
          if (live) v[k] = *(const f32x4*)(gp + (size_t)(b0 + k) * T * D);
          if (GATHER && p >= E) id[k] = ids[(size_t)(b0 + k) * S + (p - E)];
        }
      }
#pragma unroll
      for (int k = 0; k < ASM_ROWS; ++k) {
        if (b0 + k >= B) break;
        acc += v[k];
        if (GATHER && id[k] >= 0 && id[k] < tok_rows) {                                  // wave-uniform: ids[] is read at a uniform index
          if (live) *(f32x4*)(mine + lane * 4) = v[k];
          __builtin_amdgcn_wave_barrier();
          float* drow = dtok + (size_t)id[k] * D + c0;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + 64 * j + lane < D) atomicAdd(drow + 64 * j + lane, mine[64 * j + lane]);
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
    if (live) {
      float* dst = p < E ? dprefix + (size_t)p * D + c : dpos + (size_t)(p - E) * D + c;
      *(f32x4*)dst = *(const f32x4*)dst + acc;
    }
  }
}

inline bool assemble_shape_ok(int B, int E, int S, int D, int pos_rows) {
  return B >= 1 && E >= 0 && S >= 1 && D >= 4 && D % 4 == 0 && pos_rows >= S && (long)E + S <= 0x7fffffffL;
}

}  // namespace

extern "C" int vitamd_assemble_tokens_grid_cap(void) { return ASM_GRID_CAP; }

extern "C" int vitamd_assemble_tokens_fwd(const float* prefix, const float* pos, const float* tok_table, const long long* ids,
                                          const float* body, float* x, int B, int E, int S, int D, int tok_rows, int pos_rows, void* stream) {
  if (!assemble_shape_ok(B, E, S, D, pos_rows)) return VITAMD_ERR_SHAPE;
  const bool gather = tok_table != nullptr || ids != nullptr;
  if (gather && tok_rows < 1) return VITAMD_ERR_SHAPE;
  if (!pos || !x || (E > 0 && !prefix)) return VITAMD_ERR_ARG;
  if (gather ? (!tok_table || !ids || body) : !body) return VITAMD_ERR_ARG;           // exactly one source
  const long n4 = (long)B * (E + S) * (D / 4);
  const long wgs = (n4 + 255) / 256;
  const dim3 grid((unsigned)(wgs < ASM_GRID_CAP ? wgs : ASM_GRID_CAP));
  if (gather)
    hipLaunchKernelGGL(assemble_tokens_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, prefix, pos, tok_table, ids, body, x, n4, E, S,
                       D, tok_rows);
  else
    hipLaunchKernelGGL(assemble_tokens_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, prefix, pos, tok_table, ids, body, x, n4, E, S,
                       D, tok_rows);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

extern "C" int vitamd_assemble_tokens_bwd(const float* g, const long long* ids, float* dprefix, float* dpos, float* dtok, int B, int E, int S,
                                          int D, int tok_rows, int pos_rows, void* stream) {
  if (!assemble_shape_ok(B, E, S, D, pos_rows)) return VITAMD_ERR_SHAPE;
  const bool gather = ids != nullptr || dtok != nullptr;
  if (gather && tok_rows < 1) return VITAMD_ERR_SHAPE;
  if (!g || !dpos || (E > 0 && !dprefix)) return VITAMD_ERR_ARG;
  if (gather && (!ids || !dtok)) return VITAMD_ERR_ARG;
  const int cblocks = (D + 255) / 256;
  const long items = (long)(E + S) * cblocks;
  const long wgs = (items + 3) / 4;
  const dim3 grid((unsigned)(wgs < ASM_GRID_CAP ? wgs : ASM_GRID_CAP));
  if (gather)
    hipLaunchKernelGGL(assemble_tokens_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g, ids, dprefix, dpos, dtok, B, E, S, D,
                       tok_rows, items, cblocks);
  else
    hipLaunchKernelGGL(assemble_tokens_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g, ids, dprefix, dpos, dtok, B, E, S, D,
                       tok_rows, items, cblocks);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
