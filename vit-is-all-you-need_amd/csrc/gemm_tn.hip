// out[P,Q] (fp32) += sum_r L[r,p] * Rm[r,q]   — the weight-gradient GEMM of every Linear on the path:
//   dW[out,in] = dY[M,out]^T . X[M,in]   (reduction over the M = batch*tokens rows; the backward of
//   reference transformer.py:21,37,39 and of the patch-embed conv train_vit.py:34).
//
// Both operands are stored with the REDUCTION index as the slow (row) dimension, so neither is
// MFMA-fragment shaped in memory.  gfx950 answer: stage whole 512-B rows of [r][256 cols] tiles by LDS-DMA (zero-fill past the last
// row through the buffer descriptor's range check) and read the fragments with the hardware transpose read ds_read_b64_tr_b16.
// The 16-B chunk index of row r is XOR-ed with (r&3)<<2 (on the global source side) which makes every transposed read
// bank-conflict-free (tools/lds_banks.py).  mfma_f32_32x32x16_bf16 so one accumulator register of a wave = two 128-B row segments:
// the shape float atomics run at full rate with.  Split over the reduction dimension (grid = tiles x splits): partial tiles go to a
// workspace with plain stores and a reduce pass sums them (bitwise reproducible), or fp32 atomics straight into `out`.
// One kernel template, gemm_tn_kernel<LD, WS, CS>, in two forms that share every line but the LDS-DMA requests: eight waves that fetch for
// themselves (LD = false, GemmTnArgs::form = 0) or the same eight waves fed by four loader waves (LD = true, form = 1).  WS: partial tiles to
// the workspace (false: atomics, without loader waves only); CS: column sums of L beside the GEMM.  splitk_reduce_kernel is the reduce pass.
#include "common.h"
#include "vitamd_internal.h"

namespace {

constexpr int BR = 64;    // reduction rows per stage
constexpr int BP = 256, BQ = 256;
constexpr int WP = 2, WQ = 4, NW = 8;
constexpr int MT = BP / WP / 32;  // 4 p-tiles per wave
constexpr int NT = BQ / WQ / 32;  // 2 q-tiles per wave

typedef LDS_AS bf16x4* lds_bf16x4_ptr;

__device__ __forceinline__ bf16x8 tr_frag(const char* p) {
  // two transposed 4x16 reads: k = 0..3 and k = 4..7 of this lane's half (rows +4 = +2048 B)
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(p + 4 * 512));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Column sums of L beside the GEMM (GemmTnArgs::colsum: the bias gradient of the Linear whose weight gradient this is).  An A fragment holds,
// in lane l, the 8 reduction rows 8 (l >> 5) .. + 7 of column l & 31 of its 32-column p-tile: their sum is 4 v_dot2c_f32_bf16 against (1, 1)
// into ONE fp32 register per lane, issued in the shadow of the phase's MFMAs; lanes l and l + 32 are combined once behind the main loop.
// The four waves of a wave row hold the same four fragments, so wave column wq sums p-tile wq alone - and, so that this is the SAME register in
// every wave (no selects), the CS kernels walk their p-tiles rotated by wq: fragment i of wave column wq is p-tile (i + wq) & 3 (frag_pairsum below).  Every
// accumulator still sees its own k-steps in the same order, so `out` is bit-identical to the kernels without the flag.
// Every workgroup of a CS launch sums (four VALU instructions per phase; a second copy of the main loop for the others would cost more in
// code than it saves) but only those of the first column tile store: their 256 partial sums go to the workspace behind the partial tiles, [split][row tile][256], and the reduce pass adds them in split order: no atomics, bitwise reproducible.
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
__device__ __forceinline__ float frag_pairsum(bf16x8 f, int c, float s) {      // s + f[2 c] + f[2 c + 1]
  const bf16x2 ones = {(__bf16)1.0f, (__bf16)1.0f};
  return __builtin_amdgcn_fdot2_f32_bf16((bf16x2){f[2 * c], f[2 * c + 1]}, ones, s, false);
}

// ---------------------------------------------------------------------------------------------
// The schedule (ping-pong, the production kernel since round 2).  A kernel with one vmcnt(0) + barrier per 64-row stage drains the load queue
// every microsecond: MFMA pipe 28 % busy, waves parked on s_waitcnt / s_barrier 57 % of their cycles (profiles/r02/a_baseline_pmc_mfma.json).
// Here nothing ever drains:
//   * the reduction rows are the slow dimension of BOTH operands, so a 64-row stage splits into four 16-row QUARTERS of whole
//     512-B rows (16 KiB: 8 KiB of L, 8 KiB of Rm) and one 32x32x16 k-step consumes exactly one quarter: a quarter's LDS slot is
//     free again as soon as its k-step is read, long before the rest of the stage;
//   * LDS is a ring of NQ quarter slots filled by LDS-DMA (2 one-KiB pieces per wave per quarter) D quarters ahead of the reads,
//     behind a COUNTED s_waitcnt vmcnt(2(D-1)) - never 0 inside the loop;
//   * one PHASE per quarter: [transposed reads of the quarter's fragments | 2 DMA pieces | counted wait] s_barrier
//     [8 MFMAs = 256 matrix-pipe cycles] s_barrier, and the waves of the second wave row (wave >= 4: the second wave of every
//     SIMD) run ONE barrier behind the first: while one wave of a SIMD issues its MFMAs its partner reads LDS and issues DMA.
// Ordering (cdna_hip_programming.md section 5, "Read a staged buffer one phase AFTER the wait that retires it"): quarter q is
// read in phase q by both groups; every wave retires ITS pieces of quarter q by the counted wait of phase q-1, which precedes
// a barrier both groups pass before any phase-q read (RAW); the slot of quarter q is refilled with quarter q+NQ in phase
// q+NQ-D >= q+2, two barriers after the later group's reads of it have been waited for (WAR)  =>  D <= NQ-2.
// Past-the-end quarters are still "loaded" (range-checked to zeros, no traffic) so the vmcnt arithmetic is uniform.
//
// Loader-wave form (LD; round 3): the same ring, phases and MFMA order (bit-identical results), but the LDS-DMA requests move out of the eight
// compute waves into FOUR loader waves (waves 8-11, one per SIMD).  A compute wave's read section is then the 12 transposed reads alone; without
// loaders it also issues 2 DMA pieces whose issue costs 60-185 cycles each beside the partner wave's 256 cycles of MFMAs.  Loader l issues the
// four pieces the compute waves l (L operand) and l + 4 (R operand) would have issued, waits for them with the same counted vmcnt arithmetic
// (4 pieces per quarter instead of 2) and takes part in every barrier on the first wave row's timeline.
// 12 waves x 168 registers = 3 x 168 per SIMD lane: fits the 512-register file only because this kernel needs <= 168 - and fills it: nothing
// can share the CU with such a workgroup, where the 8-wave form leaves 176 registers per lane for e.g. LayerNorm waves of the other stream.
// Measured (tools/bench_tn.py, profiles/r03/tn_loader_waves.log): alone 171 / 214 / 216 us against 201 / 247 / 258 for the three ViT-B weight
// gradients (-15 %); inside the step it wins where the launch runs beside kernels that fill their CUs anyway (the fc2 weight gradient, beside
// the two input-gradient GEMMs: -0.1 ... -0.36 ms per step) and loses where the 8-wave form shared CUs with LayerNorm (all launches: +0.46 ms).
// Round 4 (from the NT loader kernel where it was worth 5-14 %): the loaders issue half of a quarter's four requests behind the phase's first
// barrier instead of all four in front of it, and run at priority 3 - a loader that is late for a barrier holds up all twelve waves.
constexpr int NQ = 8, D = 4;          // quarter slots in the ring (= two 64-row stages), prefetch distance in quarters
constexpr int QSLOT = 16 * 512 * 2;   // bytes of one quarter slot
constexpr int LDS_BYTES = NQ * QSLOT;
static_assert(D >= 2 && D <= NQ - 2, "prefetch distance: WAR rule");
static_assert(D <= 8, "add a vmcnt literal");
#define VITAMD_WAIT_VM(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")

template <bool LD, bool WS, bool CS = false>
__global__ __launch_bounds__(LD ? 768 : NW * 64) void gemm_tn_kernel(const GemmTnArgs a, int tiles_p, int tiles_q, int splits) {
  static_assert(!LD || WS, "the loader form stores partial tiles only");
  static_assert(!CS || WS, "column sums go through the workspace");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // wp, wq: a compute wave's row and column in the tile.  Formed here without loader waves and behind the loaders' branch with them: the two
  // places at which hipcc emits, instruction for instruction, the scalar code the two forms had as separate kernels.
  int wp, wq;
  if constexpr (!LD) { wp = wave / WQ; wq = wave % WQ; }

  const int ntile = tiles_p * tiles_q;
  const int id = xcd_remap(blockIdx.x, ntile * splits);
  const int split = id / ntile, tile = id % ntile;
  const int p0 = (tile / tiles_q) * BP, q0 = (tile % tiles_q) * BQ;
  const int nsteps = (a.R + BR - 1) / BR;
  const int s_lo = (int)((long)nsteps * split / splits), s_hi = (int)((long)nsteps * (split + 1) / splits);
  if (s_lo >= s_hi) return;
  const int g_lo = 4 * s_lo, g_hi = 4 * s_hi;      // quarters (16 reduction rows each)

  if constexpr (LD) {
    if (wave >= NW) {
      const int l = wave - NW;                         // pieces of compute-wave identities (wave & 3) == l, both operands
      const srd_t srdL = make_srd(a.L, (size_t)a.R * a.ldl * 2), srdR = make_srd(a.Rm, (size_t)a.R * a.ldr * 2);
      unsigned voffL[2], voffR[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = (l * 2 + i) * 2 + (lane >> 5);
        const int logical = (lane & 31) ^ ((row & 3) << 2);
        voffL[i] = (p0 + logical * 8 < a.P) ? (unsigned)(((size_t)row * a.ldl + p0 + logical * 8) * 2) : 0x80000000u;
        voffR[i] = (q0 + logical * 8 < a.Q) ? (unsigned)(((size_t)row * a.ldr + q0 + logical * 8) * 2) : 0x80000000u;
      }
      const unsigned qbL = (unsigned)16 * a.ldl * 2, qbR = (unsigned)16 * a.ldr * 2;
      const unsigned dstL = lds_addr(smem) + l * 2048, dstR = dstL + 8192;
      unsigned soL = (unsigned)g_lo * qbL, soR = (unsigned)g_lo * qbR;
      int slot_w = 0;
      auto issue_l = [&]() {
        const unsigned o = slot_w * QSLOT;
        asm_glds16(srdL, dstL + o, voffL[0], soL);
        asm_glds16(srdL, dstL + o + 1024, voffL[1], soL);
      };
      auto issue_r = [&]() {
        const unsigned o = slot_w * QSLOT;
        asm_glds16(srdR, dstR + o, voffR[0], soR);
        asm_glds16(srdR, dstR + o + 1024, voffR[1], soR);
        soL += qbL; soR += qbR;
        slot_w = slot_w + 1 == NQ ? 0 : slot_w + 1;
      };
      auto issue = [&]() { issue_l(); issue_r(); };
      __builtin_amdgcn_s_setprio(3);
#pragma unroll
      for (int d = 0; d < D; ++d) issue();
      VITAMD_WAIT_VM(4 * (D - 1));
      __builtin_amdgcn_s_barrier();
      for (int g = g_lo; g < g_hi; ++g) {
        issue_l();
        __builtin_amdgcn_s_barrier();
        issue_r();
        // quarter g + 1 is first read by the first wave row BEHIND the second barrier of this iteration, so the wait may sit here rather than in
        // front of the first barrier (one more interval for the requests to land).  Measured equal (164 / 212 / 215 us either way).
        VITAMD_WAIT_VM(4 * (D - 1));
        __builtin_amdgcn_s_barrier();
      }
      __builtin_amdgcn_s_barrier();                   // the first wave row's balancing barrier
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      return;
    }
    wp = wave / WQ; wq = wave % WQ;
  }

  // !LD: this wave's own requests (none of this is left in the loader form)
  const bool isL = wave < NW / 2;
  const int ld = isL ? a.ldl : a.ldr;
  const int c0 = isL ? p0 : q0;
  const int ncols = isL ? a.P : a.Q;
  const srd_t srd = isL ? make_srd(a.L, (size_t)a.R * a.ldl * 2) : make_srd(a.Rm, (size_t)a.R * a.ldr * 2);
  // this wave's two pieces of a quarter: rows 4*(wave&3) + 2*i + (lane>>5) of its operand, chunk = lane&31 (swizzled)
  unsigned voff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = ((wave & 3) * 2 + i) * 2 + (lane >> 5);
    const int logical = (lane & 31) ^ ((row & 3) << 2);
    const int col = c0 + logical * 8;
    voff[i] = (col < ncols) ? (unsigned)(((size_t)row * ld + col) * 2) : 0x80000000u;
  }
  const unsigned qbytes = (unsigned)16 * ld * 2;             // global bytes per quarter
  const unsigned dst0 = lds_addr(smem) + (isL ? 0 : 8192) + (wave & 3) * 2048;  // this wave's pieces inside slot 0
  int slot_w = 0;                                   // slot the next issued quarter goes to
  unsigned soff = (unsigned)g_lo * qbytes;
  auto issue = [&]() {
    const unsigned dst = dst0 + slot_w * QSLOT;
    asm_glds16(srd, dst, voff[0], soff);
    asm_glds16(srd, dst + 1024, voff[1], soff);
    soff += qbytes;
    slot_w = slot_w + 1 == NQ ? 0 : slot_w + 1;
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int h = lane >> 5, colhalf = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
  const int rowpart = (8 * h + qq) * 512 + (pp & 1) * 8;
  int offA[MT], offB[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int ip = CS ? (i + wq) & (MT - 1) : i;     // CS: p-tiles rotated by wq (frag_pairsum)
    const int chunk = (wp * (BP / WP) + ip * 32) / 8 + 2 * colhalf + (pp >> 1);
    offA[i] = rowpart + ((chunk ^ (qq << 2)) << 4);
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int chunk = (wq * (BQ / WQ) + j * 32) / 8 + 2 * colhalf + (pp >> 1);
    offB[j] = 8192 + rowpart + ((chunk ^ (qq << 2)) << 4);
  }

  if constexpr (!LD) {                              // prologue: quarters g_lo .. g_lo+D-1
#pragma unroll
    for (int d = 0; d < D; ++d) issue();
    VITAMD_WAIT_VM(2 * (D - 1));                    // quarter g_lo landed (this wave's pieces)
  }
  __builtin_amdgcn_s_barrier();                     // ... and everyone's (LD: the loaders waited for it)
  asm volatile("" ::: "memory");
  if (wp == 1) __builtin_amdgcn_s_barrier();        // second wave row runs one barrier behind from here on
  int slot_r = 0;
  float csum = 0.f;                                 // CS: this lane's column of p-tile wq over its half of every quarter's rows
  for (int g = g_lo; g < g_hi; ++g) {
    // ---- read section
    const char* q = smem + slot_r * QSLOT;
    bf16x8 af[MT], bfr[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bfr[j] = tr_frag(q + offB[j]);
#pragma unroll
    for (int i = 0; i < MT; ++i) af[i] = tr_frag(q + offA[i]);
    if constexpr (!LD) {
      issue();
      VITAMD_WAIT_VM(2 * (D - 1));                  // my pieces of quarter g+1 have landed
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // ---- matrix section
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        if constexpr (CS) { if (i * NT + j < 4) csum = frag_pairsum(af[0], i * NT + j, csum); }     // one dot product behind each of the first four MFMAs
      }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    slot_r = slot_r + 1 == NQ ? 0 : slot_r + 1;
  }
  if (wp == 0) __builtin_amdgcn_s_barrier();        // balance the stagger
  if constexpr (!LD) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the past-the-end pieces (zeros) must not outlive the workgroup's LDS
  int rot = wq;                                     // the p-tile rotation again, opaque: store addresses that depend on it are formed here, behind the
  if constexpr (CS) asm volatile("" : "+s"(rot));   // main loop, not hoisted above it into registers the loop has none to spare of
  if constexpr (CS) {
    if (tile % tiles_q == 0) {                      // one set of column sums per row tile: the first column tile's
      csum += __shfl_xor(csum, 32, 64);
      float* wc = a.ws + (size_t)splits * ntile * (BP * BQ) + ((size_t)split * tiles_p + tile / tiles_q) * BP;
      if (lane < 32) wc[wp * (BP / WP) + rot * 32 + lane] = csum;
    }
  }

  if constexpr (WS) {
    float* wt = a.ws + ((size_t)split * ntile + tile) * (BP * BQ);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int ql = wq * (BQ / WQ) + j * 32 + (lane & 31);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if constexpr (CS) {
          float* const wti = wt + ((i + rot) & (MT - 1)) * (32 * BQ);             // p-tile of fragment i: a wave-uniform step
          const int pl = wp * (BP / WP) + 4 * (lane >> 5);
#pragma unroll
          for (int r = 0; r < 16; ++r) wti[(pl + (r & 3) + 8 * (r >> 2)) * BQ + ql] = acc[i][j][r];
          continue;
        }
        const int pl = wp * (BP / WP) + i * 32 + 4 * (lane >> 5);
#pragma unroll
        for (int r = 0; r < 16; ++r) wt[(pl + (r & 3) + 8 * (r >> 2)) * BQ + ql] = acc[i][j][r];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int q = q0 + wq * (BQ / WQ) + j * 32 + (lane & 31);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int pbase = p0 + wp * (BP / WP) + i * 32 + 4 * (lane >> 5);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int p = pbase + (r & 3) + 8 * (r >> 2);
          if (p < a.P && q < a.Q) atomicAdd(a.out + (size_t)p * a.ldo + q, acc[i][j][r]);
        }
      }
    }
  }
}
#undef VITAMD_WAIT_VM

// out[p][q] (+)= sum_s ws[s][tile][p_local][q_local]; RPT float4 per thread
constexpr int RPT = 1;      // 4 is faster back to back (9.2 vs ~12 us) but slower inside the step (13.9 vs 12.0 us)
// colsum: blocks blockIdx.y >= ntile (one per row tile, launched only with a colsum) add the splits' column-sum partials of L, in split order
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int P, int Q, int ldo,
                                                            int tiles_q, int ntile, int splits, int accumulate, float* __restrict__ colsum) {
  if ((int)blockIdx.y >= ntile) {
    static_assert(BP == 256, "one thread per column of a row tile");
    const int tiles_p = ntile / tiles_q, tp = (int)blockIdx.y - ntile, p = tp * BP + (int)threadIdx.x;
    if (blockIdx.x != 0 || p >= P) return;
    const float* part = ws + (size_t)splits * ntile * (BP * BQ) + tp * BP + threadIdx.x;
    float s = part[0];
    for (int s2 = 1; s2 < splits; ++s2) s += part[(size_t)s2 * tiles_p * BP];
    colsum[p] += s;
    return;
  }
  const int tile = blockIdx.y;
  const int p0 = (tile / tiles_q) * BP, q0 = (tile % tiles_q) * BQ;
  f32x4 sum[RPT];
  const float* src[RPT];
  bool ok[RPT];
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    const int idx = (blockIdx.x * RPT + k) * 256 + threadIdx.x;   // float4 index inside the tile: 64 per row
    const int pl = idx >> 6, ql = (idx & 63) * 4;
    ok[k] = p0 + pl < P && q0 + ql < Q;
    src[k] = ws + (size_t)tile * (BP * BQ) + pl * BQ + ql;
    sum[k] = ok[k] ? *(const f32x4*)src[k] : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  for (int s2 = 1; s2 < splits; ++s2) {
#pragma unroll
    for (int k = 0; k < RPT; ++k)
      if (ok[k]) sum[k] += *(const f32x4*)(src[k] + (size_t)s2 * ntile * (BP * BQ));
  }
#pragma unroll
  for (int k = 0; k < RPT; ++k) {
    if (!ok[k]) continue;
    const int idx = (blockIdx.x * RPT + k) * 256 + threadIdx.x;
    const int p = p0 + (idx >> 6), q = q0 + (idx & 63) * 4;
    float* dst = out + (size_t)p * ldo + q;
    if (q + 3 < Q && (ldo & 3) == 0) {
      if (accumulate) sum[k] += *(const f32x4*)dst;
      *(f32x4*)dst = sum[k];
    } else {
      for (int c = 0; c < 4 && q + c < Q; ++c) dst[c] = accumulate ? dst[c] + sum[k][c] : sum[k][c];
    }
  }
}

}  // namespace

static int auto_splits(int R, int P, int Q, int requested) {
  const int ntile = ((P + BP - 1) / BP) * ((Q + BQ - 1) / BQ);
  const int nsteps = (R + BR - 1) / BR;
  int splits = requested;
  if (splits <= 0) splits = ntile >= 256 ? 1 : 256 / ntile;
  if (splits > nsteps) splits = nsteps;
  return splits;
}

extern "C" long vitamd_gemm_tn_ws_bytes(int R, int P, int Q, int splits) {
  if (R <= 0 || P <= 0 || Q <= 0) return 0;
  const long ntile = (long)((P + BP - 1) / BP) * ((Q + BQ - 1) / BQ);
  const long tiles_p = (P + BP - 1) / BP;
  // partial tiles, then the column-sum partials of L (256 floats per split and row tile; used by launches with a colsum)
  return (long)auto_splits(R, P, Q, splits) * (ntile * BP * BQ + tiles_p * BP) * (long)sizeof(float);
}

int vitamd_gemm_tn_impl(const GemmTnArgs& a, hipStream_t stream) {
  if (a.R <= 0 || a.P <= 0 || a.Q <= 0 || a.ldl % 8 || a.ldr % 8 || a.ldl < a.P || a.ldr < a.Q || a.ldo < a.Q) return VITAMD_ERR_SHAPE;
  if ((size_t)(a.R + BR) * a.ldl * 2 >= 0x80000000ull || (size_t)(a.R + BR) * a.ldr * 2 >= 0x80000000ull) return VITAMD_ERR_SHAPE;
  if (!a.L || !a.Rm || !a.out) return VITAMD_ERR_ARG;
  const int tiles_p = (a.P + BP - 1) / BP, tiles_q = (a.Q + BQ - 1) / BQ;
  const int ntile = tiles_p * tiles_q;
  const int splits = auto_splits(a.R, a.P, a.Q, a.splits);
  const size_t cs_bytes = a.colsum ? (size_t)splits * tiles_p * BP * sizeof(float) : 0;
  const bool use_ws = a.ws != nullptr && a.ws_bytes >= (size_t)splits * ntile * BP * BQ * sizeof(float) + cs_bytes;
  if (!use_ws && !a.accumulate) return VITAMD_ERR_ARG;      // overwrite mode needs the workspace: the atomic form can only add to `out`
  if (!use_ws && a.colsum) return VITAMD_ERR_ARG;           // ... and so do the column sums (their partials are summed by the reduce pass)
  const bool loaders = use_ws && a.form == 1, cs = a.colsum != nullptr;
  const dim3 grid(ntile * splits), block(loaders ? 768 : NW * 64);
  int e;
  if (!use_ws)      e = launch<gemm_tn_kernel<false, false>>(grid, block, LDS_BYTES, stream, a, tiles_p, tiles_q, splits);
  else if (loaders) e = cs ? launch<gemm_tn_kernel<true, true, true>>(grid, block, LDS_BYTES, stream, a, tiles_p, tiles_q, splits)
                           : launch<gemm_tn_kernel<true, true>>(grid, block, LDS_BYTES, stream, a, tiles_p, tiles_q, splits);
  else              e = cs ? launch<gemm_tn_kernel<false, true, true>>(grid, block, LDS_BYTES, stream, a, tiles_p, tiles_q, splits)
                           : launch<gemm_tn_kernel<false, true>>(grid, block, LDS_BYTES, stream, a, tiles_p, tiles_q, splits);
  if (e) return e;
  if (use_ws)
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(BP * BQ / 4 / 256 / RPT, ntile + (cs ? tiles_p : 0)), dim3(256), 0, stream, a.ws, a.out, a.P, a.Q, a.ldo,
                       tiles_q, ntile, splits, a.accumulate, a.colsum);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}
