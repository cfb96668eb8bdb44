// C[M,N] = A[M,K] . B[N,K]^T  (both operands K-contiguous, bf16, fp32 accumulate) with fused
// epilogues.  This is the one kernel behind every forward Linear and every dgrad of the hot path:
//   forward  y = x W^T + b      : A = x [M,K],  B = W  [N,K]           (reference transformer.py:21,37,39)
//   dgrad    dx = dy W          : A = dy [M,N'], B = W^T [K',N'] (the host keeps a bf16 transposed copy)
//
// Kernels:
//   gemm_nt_pp_kernel   (32 MT) x 256 x 64 ping-pong kernel, MT = 8 (256 rows) or 10 (320 rows): LDS-DMA that never drains, one wave of
//                       every SIMD in its matrix section while its partner reads LDS and issues DMA.  Every large GEMM of the step.
//   gemm_nt_seam_kernel persistent ping-pong kernel that requests the next tile's pipeline fill before the epilogue (gemm_nt_seam.h).
//   gemm_nt_ld_kernel   eight compute waves fed by four loader waves, 256-row tiles (gemm_nt_ld.h).
//   (gemm_nt_pp.h: request schedule, operand offsets and K-tile body of the first two; tile walk, fragment bases and launch helper of all three.)
//   gemm_nt_kernel      128 x 128 x 64 plain double-buffered kernel for small problems (classifier head, tiny models).
// Epilogues (gemm_nt_epilogue.h): gemm_epilogue_rows (LDS-transposed, row-major 16-B accesses), gemm_epilogue (direct; small tiles, fp32).
// plan_single below picks the form.  The measured alternatives of rounds 1-4 were removed; DESIGN.md section 4 holds their numbers.
#include <type_traits>
#include <mutex>
#include <atomic>
#include <cmath>
#include <cstring>
#include <climits>
#include "gemm_nt_ld.h"      // and through it gemm_nt_seam.h, gemm_nt_pp.h, gemm_nt_epilogue.h

namespace {

// SPLIT (split-K form, for launches with fewer tiles than CUs: launch_splitk below): the grid is tiles x splits; a workgroup takes one tile and the
// K-tiles [split * nkt / splits, (split + 1) * nkt / splits) and stores its fp32 accumulators to `ws` with plain stores, in the accumulator
// layout ([split][tile][i * NT + j][thread] f32x4: 1 KiB per wave-instruction); gemm_nt_splitk_reduce sums them and runs the epilogue.  EPI is unused.
template <int BM, int BN, int WM, int WN, int EPI, bool SPLIT = false>
__global__ __launch_bounds__(WM * WN * 64) void gemm_nt_kernel(const GemmNtArgs p, float* __restrict__ ws = nullptr, int splits = 1) {
  constexpr int NW = WM * WN;
  constexpr int WTM = BM / WM, WTN = BN / WN;   // wave tile
  constexpr int MT = WTM / 16, NT = WTN / 16;   // 16x16 accumulator tiles per wave
  constexpr int PIECES = (BM + BN) / 8;         // 1-KiB LDS-DMA pieces (8 rows x 128 B) per K-tile
  constexpr int PPW = PIECES / NW;
  static_assert(PIECES % NW == 0, "pieces must divide over waves");
  constexpr int BUF_BYTES = (BM + BN) * 128;

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  const int tiles_n = (p.N + BN - 1) / BN;
  const int tiles_m = (p.M + BM - 1) / BM;
  int bid = blockIdx.x, split = 0;
  if constexpr (SPLIT) {
    split = bid / (tiles_m * tiles_n);
    bid -= split * (tiles_m * tiles_n);
  }
  const int tile = xcd_remap(bid, tiles_m * tiles_n);
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;

  const __bf16* __restrict__ A = (const __bf16*)p.A;
  const __bf16* __restrict__ B = (const __bf16*)p.B;
  const int K = p.K;

  // per-lane source pointers of this wave's pieces (row clamped: out-of-range rows re-read the
  // last valid row; their results are never stored)
  const __bf16* src[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int piece = wave * PPW + i;
    const int row = piece * 8 + (lane >> 3);
    const int logical = (lane & 7) ^ (row & 7);
    if (piece < BM / 8) {
      const int g = min(m0 + row, p.M - 1);
      src[i] = A + (size_t)g * K + logical * 8;
    } else {
      const int g = min(n0 + row - BM, p.N - 1);
      src[i] = B + (size_t)g * K + logical * 8;
    }
  }

  auto stage = [&](int kt, int buf) {
    char* base = smem + buf * BUF_BYTES + wave * PPW * 1024;
#pragma unroll
    for (int i = 0; i < PPW; ++i) glds16(src[i] + kt * BK, base + i * 1024);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment read offsets inside a buffer (ks = 1 flips chunk bit 2 -> byte ^ 64)
  const int frag_off = (lane & 15) * 128 + ((((lane >> 4) ^ (lane & 7)) & 7) << 4);
  const int a_off = wm * WTM * 128 + frag_off;
  const int b_off = BM * 128 + wn * WTN * 128 + frag_off;

  const int nkt = K / BK;
  int kt0 = 0, kt1 = nkt;
  if constexpr (SPLIT) {
    kt0 = (int)((long)split * nkt / splits);
    kt1 = (int)((long)(split + 1) * nkt / splits);
  }
  stage(kt0, 0);
  for (int kt = kt0; kt < kt1; ++kt) {
    const int cur = (kt - kt0) & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile kt landed for everyone; everyone finished reading buffer cur^1
    if (kt + 1 < kt1) stage(kt + 1, cur ^ 1);
    const char* buf = smem + cur * BUF_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[MT], bfr[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) bfr[j] = *(const bf16x8*)(buf + ((b_off + j * 16 * 128) ^ (ks * 64)));
#pragma unroll
      for (int i = 0; i < MT; ++i) af[i] = *(const bf16x8*)(buf + ((a_off + i * 16 * 128) ^ (ks * 64)));
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
  }
  if constexpr (SPLIT) {
    float* w = ws + ((size_t)split * (tiles_m * tiles_n) + tile) * (BM * BN) + tid * 4;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) *(f32x4*)(w + (i * NT + j) * (NW * 64 * 4)) = acc[i][j];
    return;
  }
  if constexpr (BM == 256 && BN == 256 && WM == 2 && WN == 4 && EPI != EPI_F32) {
    if (p.N % 8 == 0 && p.ldo % 8 == 0) {
      gemm_epilogue_rows<EPI>(p, acc, m0, n0, wm, wn, lane, tid, wave, smem);
      return;
    }
  }
  gemm_epilogue<BN, WM, WN, WTM, WTN, MT, NT, EPI>(p, acc, m0, n0, wm, wn, lane, tid, smem);
}

// The reduce pass of the split-K form of gemm_nt_kernel<128, 128, 2, 2>: one workgroup per 16 x 16-per-wave unit (i, j) of a tile - 16 per tile, so
// the pass has 16 times the GEMM's tile count in workgroups - sums that unit's partials in split order (the same bits in every run, no atomics)
// and runs gemm_epilogue on it as a 1 x 1 accumulator tile whose origin is moved by (16 i, 16 j).  A thread reads one f32x4 per split, 4 KiB
// contiguous per workgroup.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_nt_splitk_reduce(const GemmNtArgs p, const float* __restrict__ ws, int splits) {
  constexpr int BM = 128, BN = 128, WM = 2, WN = 2, WTM = BM / WM, WTN = BN / WN, MT = WTM / 16, NT = WTN / 16;
  __shared__ float red[WM * BN];              // gemm_epilogue's column-sum scratch (EPI_DGELU with colsum)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
  const int tile = blockIdx.x / (MT * NT), unit = blockIdx.x % (MT * NT);
  const int m0 = (tile / tiles_n) * BM + (unit / NT) * 16;
  const int n0 = (tile % tiles_n) * BN + (unit % NT) * 16;
  const float* w = ws + ((size_t)tile * (MT * NT) + unit) * (256 * 4) + tid * 4;
  const size_t stride = (size_t)tiles_m * tiles_n * (BM * BN);
  f32x4 acc[1][1];
  acc[0][0] = *(const f32x4*)w;
  int s = 1;
  for (; s + 4 <= splits; s += 4) {           // four loads in flight; added in split order
    const f32x4 a = *(const f32x4*)(w + s * stride), b = *(const f32x4*)(w + (s + 1) * stride);
    const f32x4 c = *(const f32x4*)(w + (s + 2) * stride), d = *(const f32x4*)(w + (s + 3) * stride);
    acc[0][0] += a; acc[0][0] += b; acc[0][0] += c; acc[0][0] += d;
  }
  for (; s < splits; ++s) acc[0][0] += *(const f32x4*)(w + s * stride);
  if constexpr (EPI == EPI_DGELU) {
    // column sums (the path with BIAS_FROM_WGRAD off): gemm_epilogue fills the 2 x 16 columns of this unit in `red` and adds all 128 to colsum
    // with atomics - the others must be zeros (an atomic add of 0.0 to a column another unit sums)
    if (p.colsum) {
      for (int c = tid; c < WM * BN; c += 256) red[c] = 0.f;
      __syncthreads();
    }
  }
  gemm_epilogue<BN, WM, WN, WTM, WTN, 1, 1, EPI>(p, acc, m0, n0, wm, wn, lane, tid, (char*)red);
}

// ---------------------------------------------------------------------------------------------
// Ping-pong kernel (round 2): (32 MT) x 256 x 64 tile (MT = 8: 256 rows, MT = 10: 320 rows), 8 waves (2 x 4, wave tile 16 MT x 64),
// two K-tile buffers, LDS-DMA that never drains.  PMC on the pipe kernel above (profiles/r02/a_baseline_pmc_mfma.json): MFMA
// pipe 32-50 % busy, waves parked on s_waitcnt / s_barrier 35-42 % of their cycles - its vmcnt(0) + barrier per K-tile empties
// the load queue every microsecond.  Here:
//   * a K-tile is cut into NP = MT/2 A-PARTS (the 32 rows [32 j, 32 j + 32) of BOTH wave rows: 64 rows x 128 B = 8 KiB, one
//     1-KiB DMA piece per wave) and the B block (256 rows, 4 pieces per wave).  PHASE j of a K-tile multiplies A-part j with the
//     whole B block (2 x 4 tiles x 2 k-substeps = 16 MFMAs); B's fragments are read once, in phase 0, and stay in registers.  So
//     every LDS region is read in ONE known phase and is free long before the K-tile ends.
//   * every phase requests one A piece LA phases ahead of its use and (most phases) one B piece LB phases ahead, into the region
//     the same part of two K-tiles earlier left.  Waits are COUNTED (never 0 in the loop): the count per phase is computed at
//     compile time from the request schedule (gemm_nt_pp.h::NtSchedule).
//   * phase = [ds_reads | DMA requests | counted wait] s_barrier [16 MFMAs, s_setprio 1] s_barrier; the second wave row (waves 4-7,
//     the second wave of every SIMD) runs ONE barrier behind the first, so on every SIMD one wave feeds the matrix pipe while its
//     partner reads LDS and issues DMA (cdna_hip_programming.md section 5, the 8-phase template).
// Ordering: a region first read in phase n is retired by every wave (its own pieces) in phase n-1, before a barrier that both
// groups pass ahead of any phase-n read (RAW); a region is refilled >= 2 phases after its only read (WAR)  =>  LA, LB <= 2 NP - 2.
// Requests for K-tiles that do not exist (before the first, past the last) are issued out of range (zero fill, no traffic) so the
// counts are the same in every phase.  The DMA is issued from inline asm (common.h::asm_glds16): hipcc would otherwise put
// vmcnt(0) in front of every ds_read.
template <int EPI, int MT, int LA, int LB, bool PERS = false>     // PERS: one workgroup per CU walks a strided list of tiles (the automatic choice for large problems)
__global__ __launch_bounds__(512) void gemm_nt_pp_kernel(const GemmNtArgs p) {
  using S = NtSchedule<MT, LA>;
  static_assert(LB == S::LB, "the B lead the shared schedule implements");
  constexpr int NP = S::NP;
  constexpr int BM = 32 * MT, BN = 256, WN = 4, NT = 4;
  constexpr int PART = 64 * 128;                  // bytes of an A-part
  constexpr int BUFB = NP * PART + 256 * 128;     // one K-tile buffer: A-parts, then the B block

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
  const int ntiles = tiles_m * tiles_n;
  const int K = p.K;
  const int nkt = K / 64;
  const srd_t srdA = make_srd(p.A, (size_t)p.M * K * 2);
  const srd_t srdB = make_srd(p.B, (size_t)p.N * K * 2);
  for (int ti = blockIdx.x; ti < ntiles; ti += PERS ? (int)gridDim.x : ntiles) {
  const NtTile t = nt_tile<BM>(ti, tiles_m, tiles_n);
  const int m0 = t.m0, n0 = t.n0;
  unsigned voffA[NP], voffB[4];
  pp_offsets<MT, false>(p, t, wave, lane, voffA, voffB);
  const unsigned lds0 = lds_addr(smem) + wave * 1024;
  constexpr unsigned OOB = 0x80000000u;
  auto request_a = [&](int kt, int j) {
    const bool live = kt >= 0 && kt < nkt;
    asm_glds16(srdA, lds0 + (kt & 1) * BUFB + j * PART, live ? voffA[j] : OOB, live ? (unsigned)kt * 128u : 0u);
  };
  auto request_b = [&](int kt, int q) {
    const bool live = kt >= 0 && kt < nkt;
    asm_glds16(srdB, lds0 + (kt & 1) * BUFB + NP * PART + q * 8192, live ? voffB[q] : OOB, live ? (unsigned)kt * 128u : 0u);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const char *rdA[2], *rdB[2];
  frag_bases(smem + wm * 32 * 128, lane, rdA);                  // + part*PART + i*2048 (+ buffer)
  frag_bases(smem + NP * PART + wn * 64 * 128, lane, rdB);      // + j*2048 (+ buffer)

#pragma unroll
  for (int P = -S::lookback; P < 0; ++P) S::requests(S::tile_of(P), S::phase_of(P), request_a, request_b);
  VITAMD_WAIT_VM(S::wait(NP - 1));
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (wm == 1) __builtin_amdgcn_s_barrier();        // second wave row: one barrier behind from here on

  auto ktile = [&](int kt, auto bufc) {
    constexpr int BUF = decltype(bufc)::value;                  // the buffer is a compile-time constant of the twice-unrolled loop
    pp_ktile<MT, PART>(acc, rdA[0] + BUF * BUFB, rdA[1] + BUF * BUFB, rdB[0] + BUF * BUFB, rdB[1] + BUF * BUFB,
                       [&](int ph) { S::requests(kt, ph, request_a, request_b); }, [&](int ph) { VITAMD_WAIT_VM(S::wait(ph)); });
  };
  int kt = 0;
  for (; kt + 1 < nkt; kt += 2) {
    ktile(kt, std::integral_constant<int, 0>{});
    ktile(kt + 1, std::integral_constant<int, 1>{});
  }
  if (kt < nkt) ktile(kt, std::integral_constant<int, 0>{});
  if (wm == 0) __builtin_amdgcn_s_barrier();        // balance the stagger
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // past-the-end requests (zeros) land before the epilogue reuses LDS
  if constexpr (EPI == EPI_F32) gemm_epilogue<BN, 2, WN, 16 * MT, 64, MT, NT, EPI>(p, acc, m0, n0, wm, wn, lane, tid, smem);
  else if (p.N % 8 == 0 && p.ldo % 8 == 0) gemm_epilogue_rows<EPI, MT>(p, acc, m0, n0, wm, wn, lane, tid, wave, smem);
  else gemm_epilogue<BN, 2, WN, 16 * MT, 64, MT, NT, EPI>(p, acc, m0, n0, wm, wn, lane, tid, smem);
  if constexpr (PERS) __syncthreads();              // every wave is done with its epilogue image before the next tile's DMA lands
  }
}

static int device_cus() {          // CU count of the current device (persistent launches: one workgroup per CU)
  static int cus[16] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  if (!cus[dev]) {
    int n = 0;
    cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }
  return cus[dev];
}

template <int EPI, int MT, int LA, int LB, bool PERS = false>
int launch_pp(const GemmNtArgs& p, hipStream_t stream) {
  constexpr int ops_b = 2 * ((MT / 2) * 8192 + 32768), epi_b = 8 * MT * 2048;     // operand buffers / epilogue images
  return launch_tiles(gemm_nt_pp_kernel<EPI, MT, LA, LB, PERS>, p, stream, 32 * MT, 512, ops_b > epi_b ? ops_b : epi_b, PERS ? device_cus() : INT_MAX);
}
#undef VITAMD_WAIT_VM

template <int BM, int BN, int WM, int WN, int EPI>
int launch(const GemmNtArgs& p, hipStream_t stream) {
  constexpr int lds = 2 * (BM + BN) * 128;
  auto kern = gemm_nt_kernel<BM, BN, WM, WN, EPI>;
  if (int e = set_lds(kern, lds)) return e;
  const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(WM * WN * 64), lds, stream, p, (float*)nullptr, 1);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

// Split-K form of the 128 x 128 kernel + its reduce pass: splits * tiles * 64 KiB of `ws`.
constexpr size_t NT_SPLITK_TILE_BYTES = 128 * 128 * 4;
template <int EPI>
int launch_splitk(const GemmNtArgs& p, float* ws, int splits, hipStream_t stream) {
  constexpr int lds = 2 * (128 + 128) * 128;
  auto kern = gemm_nt_kernel<128, 128, 2, 2, EPI_F32, true>;
  if (int e = set_lds(kern, lds)) return e;
  const int tiles = ((p.M + 127) / 128) * ((p.N + 127) / 128);
  hipLaunchKernelGGL(kern, dim3(tiles * splits), dim3(256), lds, stream, p, ws, splits);
  hipLaunchKernelGGL(gemm_nt_splitk_reduce<EPI>, dim3(tiles * 16), dim3(256), 0, stream, p, (const float*)ws, splits);
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

// 320-row tiles instead of 256-row ones when that does not need more (rounds of 256 CUs) x (rows per tile): at M = 50 432,
// N = 768 outputs take 591 tiles = 3 rounds of 256 rows but 474 tiles = 2 rounds of 320 rows (-0.6 ms/step); N = 3072 is a tie
// (10 x 256 = 8 x 320), N = 2304 stays on 256 (7 x 256 < 6 x 320; forcing 320 there measured equal).  A 384-row tile would need
// 192 accumulator registers (compiles to 256 VGPRs) and a two-pass epilogue, and quantises worse at this M.
static bool prefer_tall(const GemmNtArgs& p) {
  if (p.N % 8 != 0 || p.ldo % 8 != 0 || p.K % 64 != 0) return false;
  if (p.epi != EPI_BIAS_BF16 && p.epi != EPI_RESID_F32 && p.epi != EPI_GELU && p.epi != EPI_DGELU) return false;
  const long tn = (p.N + 255) / 256;
  const long r256 = (((p.M + 255) / 256) * tn + 255) / 256, r320 = (((p.M + 319) / 320) * tn + 255) / 256;
  return r320 * 320 <= r256 * 256;     // ties go to the tall tile: 142 instead of 128 FLOP per staged byte (whole-step A/B: -0.5 ms on the N = 3072 GEMMs alone)
}

// bf16 nearest-even of a double, decided on exact distances (no float intermediate rounding)
static unsigned short bf16_rne_d(double v) {
  auto val = [](unsigned short b) { const unsigned w = (unsigned)b << 16; float g; memcpy(&g, &w, 4); return (double)g; };
  const float f = (float)v;
  unsigned u;
  memcpy(&u, &f, 4);
  unsigned short best = (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  double bd = fabs(val(best) - v);
  const unsigned short first = best;
  for (int dl = -1; dl <= 1; dl += 2) {
    const unsigned short n = (unsigned short)(first + dl);
    const double dd = fabs(val(n) - v);
    if (dd < bd || (dd == bd && !(n & 1) && (best & 1))) { best = n; bd = dd; }
  }
  return best;
}

// Device image of the erf-GELU table every GELU epilogue reads (gemm_nt_epilogue.h::gelu_lookup): entry sign x 2048 + (|bits| - 0x3900) for
// bf16 inputs 2^-13 <= |x| < 8 holds bf16(x Phi(x)) | bf16(Phi(x) + x phi(x)) << 16, from double (erfc for the tail).  One 16-KiB allocation per
// device, made by vitamd_init - the ONLY place this library allocates or synchronises; the launch functions read the pointer and nothing else.
static std::atomic<const unsigned*> g_gelu_tab[64];

static const unsigned* gelu_table() {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return nullptr; }
  return g_gelu_tab[dev].load(std::memory_order_acquire);
}

}  // namespace

const unsigned* vitamd_gelu_table() { return gelu_table(); }

int vitamd_init_impl(int device, hipStream_t stream) {
  static std::mutex mu;
  static unsigned host[4096];
  static bool built = false;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); return VITAMD_ERR_LAUNCH; }
  if (device < 0) device = cur;
  if (device >= 64) return VITAMD_ERR_ARG;
  std::lock_guard<std::mutex> lock(mu);
  if (g_gelu_tab[device].load(std::memory_order_acquire)) return VITAMD_OK;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return VITAMD_ERR_ARG; }   // never inside a capture
  if (!built) {
    for (int sg = 0; sg < 2; ++sg)
      for (int i = 0; i < 2048; ++i) {
        const unsigned w = (unsigned)(0x3900 + i) << 16;
        float ax;
        memcpy(&ax, &w, 4);
        const double x = sg ? -(double)ax : (double)ax;
        const double cdf = 0.5 * erfc(-x * 0.70710678118654752440);
        const double pdf = 0.39894228040143267794 * exp(-0.5 * x * x);
        host[sg * 2048 + i] = (unsigned)bf16_rne_d(x * cdf) | ((unsigned)bf16_rne_d(cdf + x * pdf) << 16);
      }
    built = true;
  }
  if (device != cur && hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return VITAMD_ERR_ARG; }
  void* d = nullptr;
  bool ok = hipMalloc(&d, sizeof(host)) == hipSuccess;
  ok = ok && hipMemcpy(d, host, sizeof(host), hipMemcpyHostToDevice) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();                // a failed HIP call must not surface as a later launch's error
    if (d) (void)hipFree(d);
  }
  if (device != cur) (void)hipSetDevice(cur);
  if (!ok) return VITAMD_ERR_LAUNCH;
  g_gelu_tab[device].store((const unsigned*)d, std::memory_order_release);
  return VITAMD_OK;
}

namespace {

// ---- which kernel a launch takes (one place: the dispatcher below executes the plan, vitamd_gemm_nt_plan reports it) -------------------------
// the tile selector of the C ABI: NtTileCode (vitamd_internal.h)
enum NtForm { NT_FORM_SMALL = 1, NT_FORM_PP = 2, NT_FORM_PP_PERSISTENT = 3, NT_FORM_SEAM = 4, NT_FORM_LOADER = 5, NT_FORM_SPLITK = 6 };
struct NtPlan { int form, rows, err; };

static NtPlan plan_single(const GemmNtArgs& p) {
  int tile = p.tile;
  const int epi = p.epi;
  const bool seam_epi = epi == EPI_BIAS_BF16 || epi == EPI_GELU || epi == EPI_DGELU;
  const bool tall_epi = seam_epi || epi == EPI_RESID_F32;
  if (tile == NT_TILE_LOADER) return (seam_epi && ld_ok(p)) ? NtPlan{NT_FORM_LOADER, 256, VITAMD_OK} : NtPlan{0, 0, VITAMD_ERR_SHAPE};
  if (tile == NT_TILE_SEAM) return (seam_epi && seam_ok(p)) ? NtPlan{NT_FORM_SEAM, 256, VITAMD_OK} : NtPlan{0, 0, VITAMD_ERR_SHAPE};
  const bool no_seam = tile == NT_TILE_AUTO_NO_SEAM;      // the automatic choice with persistent launches but WITHOUT the seam / loader forms (A/B and start-up probe: ops.seam_probe)
  if (no_seam) tile = NT_TILE_AUTO;
  const long big_tiles = (long)((p.M + 255) / 256) * ((p.N + 255) / 256);
  const bool pp_ok = (size_t)p.M * p.K * 2 < 0xf0000000ull && (size_t)p.N * p.K * 2 < 0xf0000000ull && p.K % 64 == 0;
  const bool big = p.N >= 256 && big_tiles >= 192 && pp_ok;
  const bool tall = tall_epi && prefer_tall(p);
  // Automatic choice, more tiles than CUs: the PERSISTENT form (one workgroup per CU walking a strided tile list; same kernel, same
  // results).  Alone it is as fast as one workgroup per tile; inside the training step, next to the weight-gradient GEMMs of the
  // second stream, it is faster: -0.45 / -0.04 / -0.34 / -0.45 ms per step on four boxes.  The explicit
  // tile codes 256 / 320 keep the one-workgroup-per-tile launch.
  if (tile == NT_TILE_AUTO_NO_PERSISTENT) tile = NT_TILE_AUTO;              // the automatic choice WITHOUT persistent launches (one workgroup per tile)
  else if (tile == NT_TILE_AUTO && big) {
    const int cus = device_cus();
    // Short K loops with several tiles per CU: the SEAM form of the persistent kernel (gemm_nt_seam.h: the next tile's pipeline fill is requested
    // before the epilogue, the epilogue runs beside the operand buffers).  Measured on the ViT-B launches (tools/bench_seam.py): QKV 172 -> 163 us,
    // fc1+GELU 316 -> 298 (265-276 with the GELU table, which needs the 256-row ring), dgrad-fc2 298 -> 268 (K = 768, 7-10 tiles per CU); equal or
    // 4 % slower where a CU sees only two tiles of a long K loop (dgrad-fc1 K = 3072, dgrad-QKV K = 2304), which therefore stay on the form
    // below.  Bit-identical results.
    if (seam_epi && !no_seam && seam_ok(p) && p.K <= 1536) {
      if (epi == EPI_BIAS_BF16 && tall && (long)((p.M + 319) / 320) * ((p.N + 255) / 256) >= 3L * cus) return NtPlan{NT_FORM_SEAM, 320, VITAMD_OK};
      // 256-row tiles: the loader-wave form (gemm_nt_ld.h) where it applies (an even number of K-tiles), else the seam kernel.  Measured (DESIGN.md
      // section 4.7; profiles/r04/ab_nt_loader_whole_step*.log, two boxes, bit-identical losses): in place of the 256-row seam kernel on the three
      // K = 768 launch classes of a layer (QKV, fc1 + GELU, dgrad-fc2 x gelu') the whole step gains 0.11 / 0.26 ms; on the N = 768 GEMMs (K = 2304 /
      // 3072) it loses - 591 tiles of 256 rows are three rounds of the 256 CUs where gemm_nt_pp_kernel runs two rounds of 320-row tiles, and twelve
      // waves at <= 168 registers cannot hold a 320-row accumulator tile - so those stay.
      if (big_tiles >= 3L * cus) return NtPlan{ld_ok(p) ? NT_FORM_LOADER : NT_FORM_SEAM, 256, VITAMD_OK};
    }
    return NtPlan{NT_FORM_PP_PERSISTENT, tall ? 320 : 256, VITAMD_OK};
  }
  if (tile == NT_TILE_AUTO) tile = big ? (tall ? NT_TILE_320 : NT_TILE_256) : NT_TILE_128;
  if (tile == NT_TILE_320) return (tall_epi && pp_ok) ? NtPlan{NT_FORM_PP, 320, VITAMD_OK} : NtPlan{0, 0, VITAMD_ERR_SHAPE};
  if (tile == NT_TILE_256) return pp_ok ? NtPlan{NT_FORM_PP, 256, VITAMD_OK} : NtPlan{0, 0, VITAMD_ERR_SHAPE};
  if (tile != NT_TILE_128) return NtPlan{0, 0, VITAMD_ERR_ARG};
  return p.K % BK == 0 ? NtPlan{NT_FORM_SMALL, 128, VITAMD_OK} : NtPlan{0, 0, VITAMD_ERR_SHAPE};
}

template <int EPI>
int dispatch_tile(const GemmNtArgs& p, hipStream_t stream) {
  constexpr bool seam_epi = EPI == EPI_BIAS_BF16 || EPI == EPI_GELU || EPI == EPI_DGELU;
  constexpr bool tall_epi = seam_epi || EPI == EPI_RESID_F32;
  const NtPlan pl = plan_single(p);
  if (pl.err) return pl.err;
  switch (pl.form) {
    case NT_FORM_LOADER:
      if constexpr (EPI == EPI_DGELU) { if (!p.colsum) return launch_ld<EPI_DGELU_NOCS>(p, stream, device_cus()); }
      if constexpr (seam_epi) return launch_ld<EPI, EPI == EPI_GELU>(p, stream, device_cus());
      break;
    case NT_FORM_SEAM:
      if constexpr (EPI == EPI_DGELU) { if (!p.colsum) return launch_seam<EPI_DGELU_NOCS, 8>(p, stream, device_cus()); }
      if constexpr (EPI == EPI_BIAS_BF16) { if (pl.rows == 320) return launch_seam<EPI, 10>(p, stream, device_cus()); }
      if constexpr (seam_epi) return launch_seam<EPI, 8, EPI == EPI_GELU>(p, stream, device_cus());
      break;
    case NT_FORM_PP_PERSISTENT:
      if constexpr (tall_epi) { if (pl.rows == 320) return launch_pp<EPI, 10, 4, 6, true>(p, stream); }
      return launch_pp<EPI, 8, 4, 6, true>(p, stream);
    case NT_FORM_PP:
      if constexpr (tall_epi) { if (pl.rows == 320) return launch_pp<EPI, 10, 4, 6>(p, stream); }
      return launch_pp<EPI, 8, 4, 6>(p, stream);
    case NT_FORM_SMALL:
      return launch<128, 128, 2, 2, EPI>(p, stream);
  }
  return VITAMD_ERR_SHAPE;
}

}  // namespace

static int dispatch_epi(const GemmNtArgs& p, hipStream_t stream) {
  switch (p.epi) {
    case EPI_BIAS_BF16: return dispatch_tile<EPI_BIAS_BF16>(p, stream);
    case EPI_GELU: return dispatch_tile<EPI_GELU>(p, stream);
    case EPI_RESID_F32: return dispatch_tile<EPI_RESID_F32>(p, stream);
    case EPI_DGELU: return dispatch_tile<EPI_DGELU>(p, stream);
    case EPI_PATCH_F32: return dispatch_tile<EPI_PATCH_F32>(p, stream);
    case EPI_F32: return dispatch_tile<EPI_F32>(p, stream);
    default: return VITAMD_ERR_ARG;
  }
}

// One big-tile workgroup per CU means a launch runs in whole rounds of 256 tiles; a last round that is mostly empty idles most of
// the chip for a full tile time.  Two remedies: the tile height (prefer_tall) and the tail split decided here.
// Tail split: the last, mostly empty round of big tiles is re-cut into 128x128 tiles.  Only ever paid for the fused-residual fc2 FORWARD GEMM
// on 256-row tiles (591 tiles = 2.31 rounds; -0.2 ms/step), which the 320-row tile has since replaced (474 tiles = 1.85 rounds:
// no split).  Everywhere else it loses on the whole step: +0.9 ms forced on every GEMM because the weight-gradient GEMMs
// of the side stream already fill the backward tails, +0.2 ms on fc1+GELU at 7.4 rounds of 320-row tiles (the 128x128 kernel's
// direct-store GELU epilogue costs more than the 0.6 idle round).
static int tail_split_rows(const GemmNtArgs& p, bool& tall) {       // rows of the head part, 0 = no split
  const int CUS = device_cus();
  tall = is_auto(p.tile) && prefer_tall(p);
  const int bm = tall ? 320 : 256;
  const int tiles_m = (p.M + bm - 1) / bm, tiles_n = (p.N + 255) / 256;
  const long big_tiles = (long)tiles_m * tiles_n;
  const long rem = big_tiles % CUS;
  const bool split_on = p.epi == EPI_RESID_F32 && !tall;
  if (!(is_auto(p.tile) && split_on && p.epi != EPI_PATCH_F32 && p.N >= 256 && p.K % 64 == 0 && big_tiles > 2 * CUS && rem != 0 && rem * 10 < CUS * 6))
    return 0;
  const int rows_a = (int)((big_tiles - rem) / tiles_n) * bm;       // M-panels whose tiles fill whole rounds
  return rows_a > 0 && rows_a < p.M ? rows_a : 0;
}

static int check_args(const GemmNtArgs& p) {
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.K % 32 != 0 || p.N % 4 != 0 || p.ldo % 4 != 0) return VITAMD_ERR_SHAPE;
  if (!p.A || !p.B || !p.out) return VITAMD_ERR_ARG;
  if (p.epi == EPI_GELU && !p.out2) return VITAMD_ERR_ARG;
  if ((p.epi == EPI_RESID_F32 || p.epi == EPI_DGELU) && !p.aux) return VITAMD_ERR_ARG;
  if (p.epi == EPI_PATCH_F32 && (!p.aux || p.n_patches <= 0)) return VITAMD_ERR_ARG;
  if (p.epi < EPI_BIAS_BF16 || p.epi > EPI_F32) return VITAMD_ERR_ARG;
  return VITAMD_OK;
}

// ---- operand sizes.  The 256-column kernels address A, B, out, out2 and aux through buffer descriptors: 32-bit byte offsets from the start of
// the operand, a 32-bit num_records, and masked requests / stores sent to offset 2^31 (OOB in the kernels), which is out of range only while the
// operand is shorter than that.  So no launch ever sees an operand of 2^31 bytes or more: vitamd_gemm_nt_impl cuts M into ROW PANELS with
// re-based A, out, out2 and aux pointers (and row0, the dropout index of the panel's first row) such that rows x K x 2 and rows x ldo x (bytes per
// output element) both stay below NT_SPAN.  Panels are whole multiples of NT_PANEL_ROWS = lcm(256, 320) rows, so every tile of every panel
// but the last is a tile of the unsplit launch and the full-height panels (close to 2^31 bytes of A or out each) take the form the whole would
// have: results are bit-identical (all forms are), colsum is added to by every panel.  What a row split cannot shrink is refused: B of NT_SPAN
// bytes or more, and the patch epilogue past the limit (its output row is a function of the global m).  The size tests of plan_single / seam_ok
// (written when one launch had to carry the whole operand) stay as a second line behind this.
constexpr size_t NT_SPAN = 0x80000000ull;
constexpr int NT_PANEL_ROWS = 1280;

static size_t out_esz(const GemmNtArgs& p) { return (p.epi == EPI_RESID_F32 || p.epi == EPI_PATCH_F32 || p.epi == EPI_F32) ? 4 : 2; }

// rows per panel (>= M: the call is one launch), or 0: VITAMD_ERR_SHAPE
static int panel_rows(const GemmNtArgs& p) {
  if ((size_t)p.N * p.K * 2 >= NT_SPAN) return 0;
  const size_t kb = (size_t)p.K * 2, ob = (size_t)p.ldo * out_esz(p), row_bytes = kb > ob ? kb : ob;      // out2 and a per-row aux are no wider than out
  if ((size_t)p.M * row_bytes < NT_SPAN) return p.M;
  if (p.epi == EPI_PATCH_F32) return 0;
  return (int)((NT_SPAN - 1) / row_bytes / NT_PANEL_ROWS) * NT_PANEL_ROWS;
}

// rows [r0, r0 + rows) of a launch as a launch of its own
static GemmNtArgs rows_of(const GemmNtArgs& p, int r0, int rows) {
  GemmNtArgs q = p;
  q.M = rows;
  q.A = (const char*)p.A + (size_t)r0 * p.K * 2;
  q.out = (char*)p.out + (size_t)r0 * p.ldo * out_esz(p);
  if (p.out2) q.out2 = (char*)p.out2 + (size_t)r0 * p.ldo * 2;
  if (p.aux && p.epi != EPI_PATCH_F32) q.aux = (const char*)p.aux + (size_t)r0 * p.ldo * (p.epi == EPI_RESID_F32 ? 4 : 2);
  q.row0 = p.row0 + r0;
  return q;
}

// the head part of a tail-split launch, or the launch itself (rows_a = 0)
static GemmNtArgs head_of(const GemmNtArgs& p, int rows_a, bool tall) {
  GemmNtArgs a = p;
  if (rows_a) {
    a.M = rows_a;
    a.tile = tall ? p.tile : NT_TILE_256;                                   // (auto picks the 320-row form again for the head part)
  }
  return a;
}

// one launch (or head + 128x128 tail) over operands below NT_SPAN
static int launch_rows(const GemmNtArgs& p, hipStream_t stream) {
  bool tall = false;
  const int rows_a = tail_split_rows(p, tall);
  if (int e = dispatch_epi(head_of(p, rows_a, tall), stream)) return e;
  if (!rows_a) return VITAMD_OK;
  GemmNtArgs b = rows_of(p, rows_a, p.M - rows_a);
  b.tile = NT_TILE_128;
  return dispatch_epi(b, stream);
}

// form | rows << 8 (| 0x80: head of whole rounds in that form and a tail on 128x128 tiles) of what launch_rows would do, or -VITAMD_ERR_*
static int plan_rows(const GemmNtArgs& p) {
  bool tall = false;
  const int rows_a = tail_split_rows(p, tall);
  const NtPlan pl = plan_single(head_of(p, rows_a, tall));
  if (pl.err) return -pl.err;
  return pl.form | (pl.rows << 8) | (rows_a ? 0x80 : 0);
}

// ---- split-K for launches that leave most of the chip idle (the kept-row layer and the classifier head: M = 256 rows are 2 x N/128 tiles, each
// walking up to 48 K-tiles alone).  Only the automatic tile codes, only launches plan_single sends to the 128 x 128 kernel as ONE launch (no row
// panels, no tail split), only the epilogues the reduce pass serves (all but the patch embedding).  Whether the caller asks for column sums does not
// enter: the launch with and the launch without them must give the same `out` (tests/test_gpu_tn_colsum.py holds BIAS_FROM_WGRAD on against off).
// The rule (want = 0): launches of at most 256 rows - two tile rows - and the split count a function of N, K and the device ALONE: as many as
// keep 2 x N/128 tiles x splits within the CU count, every split at least 2 K-tiles (its double buffer fills once).  The K ranges, and with them
// the order in which a row's products are summed, then do not depend on how many rows the launch has: a sample's result is the same bits in a
// batch of 32 and in a batch of 256 (tests/test_gpu_parity.py::test_full_size_properties holds the step to that), at the price of half the
// chip for M <= 128.  `want` > 0 asks for that many splits (still at least 2 K-tiles each) whatever the shape.  1 = the launch stays what it is.
static int splitk_count(const GemmNtArgs& p, int want) {
  if (want < 0 || !is_auto(p.tile) || p.epi == EPI_PATCH_F32) return 1;
  if (panel_rows(p) < p.M) return 1;
  bool tall = false;
  if (tail_split_rows(p, tall)) return 1;
  const NtPlan pl = plan_single(p);
  if (pl.err || pl.form != NT_FORM_SMALL) return 1;
  const int cap = p.K / BK / 2;
  long s = want;
  if (want == 0) {
    const long tiles = 2L * ((p.N + 127) / 128);
    const int cus = device_cus();
    if (p.M > 256 || tiles >= cus) return 1;
    s = cus / tiles;
  }
  if (s > cap) s = cap;
  return s < 1 ? 1 : (int)s;
}

// bytes of workspace vitamd_gemm_nt_ws_impl needs for this call (0: it does not split), or -VITAMD_ERR_*
long vitamd_gemm_nt_ws_bytes_impl(const GemmNtArgs& p, int splits) {
  if (int e = check_args(p)) return -e;
  const int s = splitk_count(p, splits);
  return s <= 1 ? 0 : (long)(s * (size_t)((p.M + 127) / 128) * ((p.N + 127) / 128) * NT_SPLITK_TILE_BYTES);
}

// form | rows << 8 | splits << 16 of what vitamd_gemm_nt_ws_impl would do with a large enough workspace
int vitamd_gemm_nt_ws_plan_impl(const GemmNtArgs& p, int splits) {
  const int plain = vitamd_gemm_nt_plan_impl(p);
  if (plain < 0) return plain;
  const int s = splitk_count(p, splits);
  return s <= 1 ? plain : (NT_FORM_SPLITK | (128 << 8) | (s << 16));
}

// vitamd_gemm_nt_impl with a caller's workspace: the split-K form where splitk_count says so and `ws` is given, the plain launch otherwise
int vitamd_gemm_nt_ws_impl(const GemmNtArgs& p0, int splits, float* ws, size_t ws_bytes, hipStream_t stream) {
  if (int e = check_args(p0)) return e;
  if (splits < 0) return VITAMD_ERR_ARG;
  const int s = ws ? splitk_count(p0, splits) : 1;
  if (s <= 1) return vitamd_gemm_nt_impl(p0, stream);
  if ((size_t)s * ((p0.M + 127) / 128) * ((p0.N + 127) / 128) * NT_SPLITK_TILE_BYTES > ws_bytes) return VITAMD_ERR_ARG;
  GemmNtArgs p = p0;
  if (p.epi == EPI_GELU) {
    p.gelu_tab = gelu_table();
    if (!p.gelu_tab) return VITAMD_ERR_INIT;
  }
  switch (p.epi) {
    case EPI_BIAS_BF16: return launch_splitk<EPI_BIAS_BF16>(p, ws, s, stream);
    case EPI_GELU: return launch_splitk<EPI_GELU>(p, ws, s, stream);
    case EPI_RESID_F32: return launch_splitk<EPI_RESID_F32>(p, ws, s, stream);
    case EPI_DGELU: return launch_splitk<EPI_DGELU>(p, ws, s, stream);
    case EPI_F32: return launch_splitk<EPI_F32>(p, ws, s, stream);
    default: return VITAMD_ERR_ARG;
  }
}

int vitamd_gemm_nt_impl(const GemmNtArgs& p0, hipStream_t stream) {
  if (int e = check_args(p0)) return e;
  const int rows = panel_rows(p0);
  if (!rows) return VITAMD_ERR_SHAPE;
  GemmNtArgs p = p0;
  if (p.epi == EPI_GELU) {                 // ONE rounding of GELU whatever kernel the launch takes: every GELU epilogue reads the table
    p.gelu_tab = gelu_table();
    if (!p.gelu_tab) return VITAMD_ERR_INIT;
  }
  if (rows >= p.M) return launch_rows(p, stream);
  const int last = (p.M - 1) / rows * rows;                                  // every refusal comes before the first launch: the two panel heights
  if (int e = plan_rows(rows_of(p, 0, rows)); e < 0) return -e;
  if (int e = plan_rows(rows_of(p, last, p.M - last)); e < 0) return -e;
  for (int r0 = 0; r0 < p.M; r0 += rows)
    if (int e = launch_rows(rows_of(p, r0, p.M - r0 < rows ? p.M - r0 : rows), stream)) return e;
  return VITAMD_OK;
}

// vitamd_gemm_nt_plan: the kernel form vitamd_gemm_nt_bf16 would launch for these arguments on the current device, without launching:
// form | rows << 8 (| 0x80: the launch is cut into a head of whole rounds in that form and a tail on 128x128 tiles), or -VITAMD_ERR_*.  A call
// that is cut into row panels answers for its full-height panels (the last, shorter one may take another form).
int vitamd_gemm_nt_plan_impl(const GemmNtArgs& p0) {
  if (int e = check_args(p0)) return -e;
  const int rows = panel_rows(p0);
  if (!rows) return -VITAMD_ERR_SHAPE;
  if (rows >= p0.M) return plan_rows(p0);
  const int last = (p0.M - 1) / rows * rows;
  if (int e = plan_rows(rows_of(p0, last, p0.M - last)); e < 0) return e;
  return plan_rows(rows_of(p0, 0, rows));
}
