// What the NT GEMM kernels on 256-column tiles share.  For the two (32 MT) x 256 x 64 ping-pong kernels (gemm_nt_pp_kernel in gemm_nt.hip,
// gemm_nt_seam_kernel in gemm_nt_seam.h): the request schedule (NtSchedule), the LDS-DMA source offsets (pp_offsets) and the two-barrier K-tile body
// (pp_ktile).  For those two and gemm_nt_ld_kernel (gemm_nt_ld.h): the tile walk (nt_tile), the fragment-read bases (frag_bases) and the launch
// helper (launch_tiles).  NOT shared: the wave-private staged epilogue, which gemm_nt_seam_kernel and gemm_nt_ld_kernel each keep a copy of (marked
// TWIN in both files; as one function it changed the code of gemm_nt_ld_kernel<3, false, 1>: DESIGN.md section 4).
#pragma once
#include "gemm_nt_epilogue.h"

namespace {

// ---- tile walk: workgroup ti of ntiles (XCD remap, grouped order on wide problems) -> first row / column of its BM x 256 tile
struct NtTile { int m0, n0; };
template <int BM>
__device__ __forceinline__ NtTile nt_tile(int ti, int tiles_m, int tiles_n) {
  int tm, tn;
  tile_coords(xcd_remap(ti, tiles_m * tiles_n), tiles_m, tiles_n, tiles_n >= 6, tm, tn);
  return NtTile{tm * BM, tn * 256};
}

// ---- fragment reads: 16-row tile at LDS row rb: lane -> row rb + (lane & 15), chunk ((lane >> 4) + 4 ks) ^ (row & 7); k-substep (K-half) 1 flips
// chunk bit 2 = XOR 64 on the swizzled offset, hence one base pointer per substep
__device__ __forceinline__ void frag_bases(const char* base, int lane, const char* (&rd)[2]) {
  const int frag_off = (lane & 15) * 128 + ((((lane >> 4) ^ (lane & 7)) & 7) << 4);
  rd[0] = base + frag_off;
  rd[1] = base + (frag_off ^ 64);
}

// ---- request schedule of the ping-pong kernels.  A K-tile is cut into NP = MT/2 A-parts and four 64-row B pieces (gemm_nt.hip, at
// gemm_nt_pp_kernel).  Phase ph of K-tile t requests, in program order: A-part (ph + LA) % NP of K-tile t + (ph + LA) / NP, then every B piece q
// whose lead 6 - q ends on a K-tile boundary (the B block is first read in phase 0), of K-tile t + (ph + 6 - q) / NP.
// (A request-placement experiment of round 3 - the B request, or both requests, issued from inside the matrix section - measured slower everywhere
// and was removed in round 4: profiles/r03/request_placement_experiment.log.)  Both requests of a phase are issued in its read section, ahead of the
// phase's counted wait.
template <int MT, int LA>
struct NtSchedule {
  static constexpr int NP = MT / 2;
  static constexpr int LB = 6;                       // lead of B piece 0; piece q leads by LB - q
  static_assert(MT % 2 == 0 && NP >= 4 && NP <= 5, "tile height");
  static_assert(LA >= 2 && LA <= 2 * NP - 2, "A lead");
  static constexpr int blead(int q) { return LB - q; }
  static constexpr int lookback = LA > LB ? LA : LB;            // phases before the first whose requests the prologue replays
  static constexpr int phase_of(int P) { return ((P % NP) + NP) % NP; }       // P = NP * tile_of(P) + phase_of(P), also for P < 0
  static constexpr int tile_of(int P) { return (P - phase_of(P)) / NP; }
  static constexpr int prologue_requests() {       // LDS-DMA instructions per wave in one tile's prologue (the replayed lookback phases)
    int n = 0;
    for (int P = -lookback; P < 0; ++P) {
      ++n;
      for (int q = 0; q < 4; ++q) n += b_here(phase_of(P), q) ? 1 : 0;
    }
    return n;
  }
  static constexpr int a_part(int ph) { return (ph + LA) % NP; }
  static constexpr int a_tile(int ph) { return (ph + LA) / NP; }
  static constexpr bool b_here(int ph, int q) { return (ph + blead(q)) % NP == 0; }
  static constexpr int b_tile(int ph, int q) { return (ph + blead(q)) / NP; }
  // operations allowed outstanding after phase ph's requests so that everything first read in phase ph + 1 has landed.  E: operations the
  // epilogue of the previous tile put between that tile's requests and this tile's phase 0 (seam kernel, first K-tile behind a seam only): they
  // are younger than any request issued before the seam, so a wait for such a request leaves them outstanding too.
  static constexpr int wait(int ph, int E = 0) {
    int allowed = 0;
    for (int d = 0; d < 4 * NP; ++d) {
      const int f = ((ph - d) % NP + NP) % NP;
      // reverse program order inside phase ph - d: its wait | [B requests] [A request]
      for (int q = 3; q >= 0; --q)
        if (b_here(f, q)) {
          if (d + 1 >= blead(q)) return allowed + (d > ph ? E : 0);
          ++allowed;
        }
      if (d + 1 >= LA) return allowed + (d > ph ? E : 0);
      ++allowed;
    }
    return allowed;
  }
  // the requests of phase ph of K-tile kt.  The prologue of a tile replays those of the `lookback` phases before its phase 0:
  //     for (int P = -lookback; P < 0; ++P) requests(tile_of(P), phase_of(P), request_a, request_b);
  // (K-tiles < 0 are requested out of range: the queue then looks exactly as in steady state and the same counted waits apply from the first phase
  // on.)  That loop stays in the kernels: as a member function here taking the two lambdas it reordered the epilogues of gemm_nt_pp_kernel.
  template <class ReqA, class ReqB>
  static __device__ __forceinline__ void requests(int kt, int ph, ReqA request_a, ReqB request_b) {
    request_a(kt + a_tile(ph), a_part(ph));
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (b_here(ph, q)) request_b(kt + b_tile(ph, q), q);
  }
};

// (a macro: the count must reach the "n" constraint as an expression that folds after unrolling; #undef'd at the end of gemm_nt.hip's kernels)
#define VITAMD_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")

// ---- this wave's LDS-DMA source offsets.  Its piece of A-part j: LDS rows 8 wave + (lane >> 3) of the part = rows 32 j + (lr & 31) of wave row
// lr >> 5; its piece q of the B block: rows 64 q + lr.  16-B chunk lane & 7, XOR (row & 7) on the SOURCE side.  Rows past M / N are clamped (never
// stored).  MUL32 (seam kernel, whose offsets are recomputed at every seam): keeps each product a 32-bit v_mul_lo - hipcc otherwise forms
// v_mad_u64_u32 there, a register PAIR per offset.
template <int MT, bool MUL32>
__device__ __forceinline__ void pp_offsets(const GemmNtArgs& p, NtTile t, int wave, int lane, unsigned (&voffA)[MT / 2], unsigned (&voffB)[4]) {
  const int lr = 8 * wave + (lane >> 3);
  const unsigned chunk = (unsigned)(((lane & 7) ^ (lr & 7)) * 16);
#pragma unroll
  for (int j = 0; j < MT / 2; ++j) {
    unsigned o = (unsigned)min(t.m0 + (lr >> 5) * (16 * MT) + j * 32 + (lr & 31), p.M - 1) * (unsigned)(p.K * 2);
    if constexpr (MUL32) asm volatile("" : "+v"(o));
    voffA[j] = o + chunk;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned o = (unsigned)min(t.n0 + 64 * q + lr, p.N - 1) * (unsigned)(p.K * 2);
    if constexpr (MUL32) asm volatile("" : "+v"(o));
    voffB[q] = o + chunk;
  }
}

// ---- one K-tile of the two-barrier ping-pong loop: NP phases of [ds_reads | DMA requests | counted wait] s_barrier [16 MFMAs, s_setprio 1]
// s_barrier.  Phase ph multiplies A-part ph (pa0 / pa1: the wave's fragment bases in the K-tile's A buffer, k-substep 0 / 1) with the whole B block
// (pb0 / pb1), whose fragments are read once, in phase 0.  request(ph) issues the phase's LDS-DMA requests, wait(ph) its counted wait (ph is a
// compile-time constant after unrolling: the count folds into the instruction).  Call it from a lambda of the kernel (`ktile`), as both kernels do:
// called straight from the seam kernel's K loop it made hipcc compile that kernel's dGELU epilogue differently (scalar instead of packed fp32 math).
template <int MT, int PART, class Request, class Wait>
__device__ __forceinline__ void pp_ktile(f32x4 (&acc)[MT][4], const char* pa0, const char* pa1, const char* pb0, const char* pb1, Request request, Wait wait) {
  bf16x8 bq[4][2], af[2][2];
#pragma unroll
  for (int ph = 0; ph < MT / 2; ++ph) {
    // ---- read section
    if (ph == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bq[j][0] = *(const bf16x8*)(pb0 + j * 2048);
        bq[j][1] = *(const bf16x8*)(pb1 + j * 2048);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      af[i][0] = *(const bf16x8*)(pa0 + ph * PART + i * 2048);
      af[i][1] = *(const bf16x8*)(pa1 + ph * PART + i * 2048);
    }
    request(ph);
    wait(ph);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // ---- matrix section: A-part ph x the whole B block
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[2 * ph + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[j][ks], af[i][ks], acc[2 * ph + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
}

// ---- launch on BM x 256 tiles with at most max_wgs workgroups.  Persistent forms pass the CU count (one workgroup per CU, each walking a strided
// list of tiles); INT_MAX gives one workgroup per tile (gemm_nt_pp_kernel with PERS = false).
template <class Kern>
int launch_tiles(Kern kern, const GemmNtArgs& p, hipStream_t stream, int BM, int threads, int lds, int max_wgs) {
  if (int e = set_lds(kern, lds)) return e;
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + 255) / 256);
  hipLaunchKernelGGL(kern, dim3(tiles > max_wgs ? max_wgs : tiles), dim3(threads), lds, stream, p);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

}  // namespace
