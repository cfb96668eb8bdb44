// Scaled-dot-product attention forward / backward for the packed fused-QKV layout of the
// reference (transformer.py:26-29): qkv [B, N, 3, H, 64] bf16 straight out of the QKV GEMM,
// output o [B, N, H*64] bf16 — the einops split/merge copies of transformer.py:27,29 never exist.
// softmax(q k^T / sqrt(dh) [+ causal -inf mask, transformer.py:22-25]) v ; dh = 64 ; N <= 512 in one LDS-resident
// chunk per head, longer sequences (to 16 384) through the two-sided tiling of the *_long_kernel forms.
//
// gfx950 design.  One workgroup (4 waves) per (batch, head); the whole K/V (or Q/dO) of the head
// sits in LDS as [N][64] bf16 tiles (128-B rows, LDS-DMA staged, chunk index XOR-swizzled so BOTH
// the row reads (ds_read_b128) and the transposed reads (ds_read_b64_tr_b16) are conflict-free:
// tools/lds_banks.py).  Each wave owns 32-row blocks of the "lane side" matrix and keeps its
// fragments in registers.  mfma_f32_32x32x16_bf16 with the reduction-side index on the accumulator
// ROWS, so an accumulator tile converts in place into the B operand of the next MFMA
// (cdna guide section 3, "accumulator tile as the next MFMA's operand") — softmax never leaves registers.
//
//   forward : lane = query.  S^T = K.Q^T ; online softmax ; O^T += V^T.P^T
//   bwd dQ  : lane = query.  S^T = K.Q^T ; dP^T = V.dO^T ; dS^T = P^T o (dP^T - delta) ; dQ^T += K^T.dS^T
//   bwd dKV : lane = key.    S = Q.K^T ; dP = dO.V^T ; dV^T += dO^T.P ; dK^T += Q^T.dS
// Scores are recomputed from Q, K and the forward's log-sum-exp (flash-attention backward).
//
// Shared pieces: the staged output store store_rows_T_img (4-KiB / 2-KiB image, residual add, column sums), zero(), head_addr / stat_index, and on
// the host make_args, launch and with_tiles / with_flag.  NOT shared, marked TWIN where they stand: the tile bodies of the plain kernels and their
// *_long_kernel forms and the lane-side set-up of dQ (as __forceinline__ functions they changed registers and waits of those kernels), and the
// local zeroing loops / addressing lines of the kernels whose code the helpers changed (profiles/attention_shared_source/README.md).
#include "common.h"
#include "vitamd_internal.h"
#include <type_traits>

namespace {

constexpr int DH = 64;
constexpr int MAX_N = 512;        // single-chunk kernels; longer sequences (up to MAX_N_LONG) take the *_long_kernel forms
constexpr int MAX_N_LONG = VITAMD_DECODE_MAX_LEN;
constexpr float NEG_BIG = -1.0e30f;

typedef LDS_AS bf16x4* lds_bf16x4_ptr;

__device__ __forceinline__ int swz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 3) & 3); }

// Stage rows [0, npad) of a [N][64]-per-head matrix (row stride ld elements) into an LDS tile.
// Rows >= N re-read row N-1 (finite data; masked by the callers).
__device__ __forceinline__ void stage_tile(const __bf16* __restrict__ g, int ld, int N, int npad, char* lds, int wave, int lane, int nwaves = 4) {
  const int pieces = npad / 8;
  for (int pc = wave; pc < pieces; pc += nwaves) {
    const int row = pc * 8 + (lane >> 3);
    const int logical = (lane & 7) ^ swz(row);
    const int grow = min(row, N - 1);
    glds16(g + (size_t)grow * ld + logical * 8, lds + pc * 1024);
  }
}

// A-operand fragment by ROW read: element j = Y[32T + (lane&31)][16kk + 8(lane>>5) + j]
__device__ __forceinline__ bf16x8 row_frag(const char* tile, int T, int kk, int lane) {
  const int rr = lane & 31;
  const int chunk = (2 * kk + (lane >> 5)) ^ swz(rr);
  return *(const bf16x8*)(tile + T * 4096 + rr * 128 + (chunk << 4));
}

// A-operand fragment by TRANSPOSED read, in the k order of an accumulator-derived B operand:
// element j = Y[32T + 16s + 8(j>>2) + 4(lane>>5) + (j&3)][32dt + (lane&31)]
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int T, int s, int dt, int lane) {
  const int h = lane >> 5, colhalf = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
  const int chunk = 4 * dt + 2 * colhalf + (pp >> 1);
  bf16x4 part[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int rloc = 16 * s + 8 * u + 4 * h + qq;  // row inside the 32-row tile
    const int f = (((qq >> 1) & 1) << 2) | (2 * s + u);
    part[u] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(tile + T * 4096 + rloc * 128 + ((chunk ^ f) << 4) + (pp & 1) * 8));
  }
  return __builtin_shufflevector(part[0], part[1], 0, 1, 2, 3, 4, 5, 6, 7);
}

// registers 8s..8s+7 of a 32x32 accumulator -> bf16 B-operand fragment of k-step s
__device__ __forceinline__ bf16x8 acc_to_frag(const f32x16& x, int s) {
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (__bf16)x[8 * s + j];
  return f;
}

// clear one accumulator tile / a 64x32 pair (three kernels keep their own loops, noted there: the call changed their code)
__device__ __forceinline__ void zero(f32x16& x) {
#pragma unroll
  for (int r = 0; r < 16; ++r) x[r] = 0.f;
}
__device__ __forceinline__ void zero(f32x16 (&x)[2]) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) zero(x[dt]);
}

// lane-side fragments of a 32-row block: element j = X[r0 + (lane&31)][16kk + 8(lane>>5) + j]
__device__ __forceinline__ void load_lane_frags(const __bf16* __restrict__ g, int ld, int N, int r0, int lane, bf16x8 (&f)[4]) {
  const int row = min(r0 + (lane & 31), N - 1);
  const __bf16* p = g + (size_t)row * ld + 8 * (lane >> 5);
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) f[kk] = *(const bf16x8*)(p + 16 * kk);
}

__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }  // bare v_exp_f32 (inputs <= 0 or masked)
__device__ __forceinline__ float max16(const f32x16& v) {
  float a = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), b = fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7]));
  float c = fmaxf(fmaxf(v[8], v[9]), fmaxf(v[10], v[11])), d = fmaxf(fmaxf(v[12], v[13]), fmaxf(v[14], v[15]));
  return fmaxf(fmaxf(a, b), fmaxf(c, d));
}

// store a transposed 64x32 accumulator pair  acc[dt][reg] = X^T[d][row]  as X[row][d] bf16, scaled
__device__ __forceinline__ void store_rows_T(__bf16* __restrict__ g, int ld, int N, int r0, int lane, const f32x16 (&acc)[2], float scale) {
  const int row = r0 + (lane & 31);
  if (row >= N) return;
  __bf16* p = g + (size_t)row * ld + 4 * (lane >> 5);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      u32x2 o = {pack_bf16x2(acc[dt][4 * u] * scale, acc[dt][4 * u + 1] * scale),
                 pack_bf16x2(acc[dt][4 * u + 2] * scale, acc[dt][4 * u + 3] * scale)};
      *(u32x2*)(p + 32 * dt + 8 * u) = o;
    }
}

// Same, but transposed through a wave-private LDS image first so that every lane stores 16 B and a wave-instruction covers 8 whole
// 128-B head rows (4 store instructions instead of 16 scattered 8-B ones: the output tail was store-issue bound).
//   ROWS = 32: a 4-KiB image, one pass.  colacc: the column sums of the stored bf16 rows are added to it (lane = column).
//   ROWS = 16: a 2-KiB image, 16 rows per pass, two passes: the 8-wave kernels keep the LDS of a workgroup at 2 x npad x 128 + 8 x 2 KiB,
//              the footprint of the 4-wave ones, so that two workgroups - now 16 waves - still share a CU.
//   RES: plus the residual add of the fp32 stream, xo[row][d] = xi[row][d] + bf16(acc) for the same 32 rows x 64 columns (row stride ldx).
template <int ROWS = 32, bool RES = false>
__device__ __forceinline__ void store_rows_T_img(__bf16* __restrict__ g, int ld, int N, int r0, int lane, const f32x16 (&acc)[2], float scale, char* img,
                                                 float* colacc = nullptr, const float* __restrict__ xi = nullptr, float* __restrict__ xo = nullptr,
                                                 int ldx = 0) {
  const int rr = lane & 31, h = lane >> 5;
  constexpr int ITS = ROWS / 8;
  int pass = 0;
#pragma unroll
  do {                                         // a do-while: around the single pass of ROWS = 32 it leaves no loop at all (a one-trip for loop changes how hipcc schedules the callers)
    f32x4 r[ITS][2];
    if constexpr (RES) {                       // residual loads first: their latency overlaps the LDS round trip
#pragma unroll
      for (int it = 0; it < ITS; ++it) {
        const int row = (lane >> 3) + 8 * it, pc = lane & 7;
        const float* px = xi + (size_t)min(r0 + ROWS * pass + row, N - 1) * ldx + 8 * (pc ^ (row & 7));
        r[it][0] = *(const f32x4*)px;
        r[it][1] = *(const f32x4*)(px + 4);
      }
    }
    if (ROWS == 32 || (rr >> 4) == pass) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          u32x2 o = {pack_bf16x2(acc[dt][4 * u] * scale, acc[dt][4 * u + 1] * scale),
                     pack_bf16x2(acc[dt][4 * u + 2] * scale, acc[dt][4 * u + 3] * scale)};
          // element columns 32dt + 8u + 4h .. +3  -> 16-B chunk 4dt + u, half h ; chunk XOR (row & 7)
          *(u32x2*)(img + (rr & (ROWS - 1)) * 128 + (((4 * dt + u) ^ (rr & 7)) << 4) + h * 8) = o;
        }
    }
    // wave-private image: the same wave reads it back (the compiler orders LDS accesses of one wave)
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      const int row = (lane >> 3) + 8 * it, pc = lane & 7;                  // image row = block row ROWS pass + row
      const u32x4 v = *(const u32x4*)(img + row * 128 + pc * 16);
      const int grow = r0 + ROWS * pass + row;
      if (grow < N) {
        const int col = 8 * (pc ^ (row & 7));
        *(u32x4*)(g + (size_t)grow * ld + col) = v;
        if constexpr (RES) {
          f32x4 o0 = {r[it][0][0] + bf16lo(v[0]), r[it][0][1] + bf16hi(v[0]), r[it][0][2] + bf16lo(v[1]), r[it][0][3] + bf16hi(v[1])};
          f32x4 o1 = {r[it][1][0] + bf16lo(v[2]), r[it][1][1] + bf16hi(v[2]), r[it][1][2] + bf16lo(v[3]), r[it][1][3] + bf16hi(v[3])};
          float* po = xo + (size_t)grow * ldx + col;
          *(f32x4*)po = o0;
          *(f32x4*)(po + 4) = o1;
        }
      }
    }
  } while (ROWS == 16 && ++pass < 2);
  if constexpr (ROWS == 32) {
    if (colacc) {
      // column sums of the stored bf16 rows (the bias gradient of the QKV Linear): lane = column
      const int chunk = lane >> 3, within = (lane & 7) * 2;
      const int nrows = min(32, N - r0);
      float sacc = 0.f;
      for (int row = 0; row < nrows; ++row)
        sacc += bf2f(*(const __bf16*)(img + row * 128 + ((chunk ^ (row & 7)) << 4) + within));
      *colacc += sacc;
    }
  }
}

struct AttnArgs {
  const __bf16* qkv;   // [B, N, 3, H, 64]
  __bf16* o;           // fwd out / bwd in  [B, N, H*64]
  float* lse2;         // [B, H, N] log2-domain log-sum-exp of the scaled scores
  const __bf16* d_o;   // bwd: [B, N, H*64]
  __bf16* dqkv;        // bwd: [B, N, 3, H, 64]
  float* delta;        // bwd: [B, H, N] rowsum(dO o O)
  float* dbias;        // bwd: optional [3*H*64] fp32, column sums of dqkv are ADDED (QKV bias gradient)
  int B, N, H;
  int causal;
  float scale_log2e;   // (1/sqrt(dh)) * log2(e)
  float scale;         // 1/sqrt(dh)
  // dropout on the softmax probabilities (reference transformer.py:28 dropout_p); thresh = p * 2^32, 0 = off
  unsigned drop_thresh;
  float drop_scale;
  unsigned seed_lo, seed_hi;
  // forward only, optional: fp32 residual stream [B*N, H*64]; with both set the kernel also writes resid_out = resid_in + bf16(o)
  // (transformer.py:44 `x = x + attn(...)`), so the LayerNorm that follows reads x once instead of x and o and writing x
  const float* resid_in;
  float* resid_out;
  // kept-query forms only (KEEP / LIM template arguments): queries >= nq are not computed (forward) / carry no gradient (backward).
  // o and d_o are then COMPACT [B*nq, H*64] (row b*nq + t); lse2 and delta keep the [B, H, N] layout, entries of queries >= nq untouched.
  int nq;
};

// Per-head addressing, the same in every kernel: batch b, head hh, sequence length N, the row strides D3 (qkv, dqkv) and D (o, d_o, the residual
// stream) and the head's Q rows (its K rows at + D, its V rows at + 2 D).  Arguments by value: the kernels read AttnArgs themselves.
struct HeadAddr {
  int b, hh, N, D3, D;
  const __bf16* qbase;
};
template <typename Idx>   // the index type of the caller's own division: blockIdx.x is unsigned, the unrolled kernels divide their int head
__device__ __forceinline__ HeadAddr head_addr(const __bf16* qkv, int N, int H, Idx head) {
  const int b = head / H, hh = head % H, D3 = 3 * H * DH, D = H * DH;
  return {b, hh, N, D3, D, qkv + (size_t)b * N * D3 + hh * DH};
}
// index of (b, hh, row) in the [B, H, N] statistics lse2 and delta
__device__ __forceinline__ size_t stat_index(int b, int H, int hh, int N, int row) { return ((size_t)b * H + hh) * N + row; }

// keep-scale of probability (b, head, query, key): 1/(1-p) or 0
__device__ __forceinline__ float attn_keep(const AttnArgs& a, int bh, int query, int key) {
  const unsigned long long idx = ((unsigned long long)bh * a.N + query) * a.N + key;
  return dropout_keep(idx, a.seed_lo, a.seed_hi, a.drop_thresh, a.drop_scale);
}

// ------------------------------------------------------------------------------------------ forward
template <bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, blockIdx.x);
  const int nt = (N + 31) / 32, npad = nt * 32;
  char* ktile = smem;
  char* vtile = smem + npad * 128;
  stage_tile(qbase + D, D3, N, npad, ktile, wave, lane);
  stage_tile(qbase + 2 * D, D3, N, npad, vtile, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const float c = a.scale_log2e;
  for (int qb = wave; qb < nt; qb += 4) {
    const int q0 = qb * 32;
    const int qrow = q0 + (lane & 31);
    bf16x8 qf[4];
    load_lane_frags(qbase, D3, N, q0, lane, qf);
    f32x16 oacc[2];
    zero(oacc);
    float m = NEG_BIG, l = 0.f;
    const int t_end = a.causal ? min(nt, qb + 1) : nt;  // key tiles above the diagonal contribute nothing
    for (int T = 0; T < t_end; ++T) {     // TWIN of the key-tile body of attn_fwd_long_kernel (there: key0 for 32 * T): a change to one belongs in the other
      f32x16 s;
      zero(s);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(ktile, T, kk, lane), qf[kk], s, 0, 0, 0);
      if (32 * T + 32 > N || (a.causal && T == qb)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = 32 * T + acc_row(r, lane);
          if (!(key < N && (!a.causal || key <= qrow))) s[r] = NEG_BIG;
        }
      }
      float tmax = max16(s);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * c;
      const float mnew = fmaxf(m, tmax);
      const float alpha = fast_exp2(m - mnew);
      m = mnew;
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = fast_exp2(__builtin_fmaf(s[r], c, -mnew));
        psum += s[r];
        if constexpr (DROP) s[r] *= attn_keep(a, blockIdx.x, min(qrow, N - 1), min(32 * T + acc_row(r, lane), N - 1));
      }
      l = l * alpha + psum;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 pf = acc_to_frag(s, sidx);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(vtile, T, sidx, dt, lane), pf, oacc[dt], 0, 0, 0);
      }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    store_rows_T(a.o + (size_t)b * N * D + hh * DH, D, N, q0, lane, oacc, inv);
    if (lane < 32 && qrow < N) a.lse2[stat_index(b, a.H, hh, N, qrow)] = m + log2f(l);
  }
}

// ------------------------------------------------------------------------------------------ forward, N <= 256
// The whole score row of a query fits in registers (NKT tiles x 16 fp32), so there is no online
// rescaling: S for every key tile, one row maximum, exp2, then P.V.  Per element the VALU work is
// fma + v_exp + add + cvt (the kernel is VALU-bound at dh = 64, not MFMA-bound).
template <int NKT, bool DROP, bool CAUSAL, bool RES = false>
__global__ __launch_bounds__(256, 2) void attn_fwd_small_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int head = blockIdx.x;     // one workgroup per (batch, head); a persistent two-per-CU grid walking the heads is slower (backward 276 against 256 us)
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, head);
  constexpr int nt = NKT, npad = NKT * 32;
  char* ktile = smem;
  char* vtile = smem + npad * 128;
  char* oimg = smem + 2 * npad * 128 + wave * 4096;
  stage_tile(qbase + D, D3, N, npad, ktile, wave, lane);
  stage_tile(qbase + 2 * D, D3, N, npad, vtile, wave, lane);
  const int wrot = (wave + head) & 3;   // rotate which wave gets the short list of query blocks
  // the Q rows of both of this wave's query blocks ride the same wait as the K/V staging (one memory round trip per head, not three)
  bf16x8 qf[4], qf2[4];
  load_lane_frags(qbase, D3, N, wrot * 32, lane, qf);
  if (wrot + 4 < nt) load_lane_frags(qbase, D3, N, wrot * 32 + 128, lane, qf2);
  else {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf2[kk] = qf[kk];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) asm volatile("" : "+v"(qf[kk]), "+v"(qf2[kk]));   // pins the loads above the wait (hipcc sinks plain loads to their first use)
  __syncthreads();

  const float c = a.scale_log2e;
  for (int qb = wrot; qb < nt; qb += 4) {
    const int q0 = qb * 32;
    const int qrow = q0 + (lane & 31);
    if (qb != wrot) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) qf[kk] = qf2[kk];
    }
    const int t_end = CAUSAL ? qb + 1 : nt;
    f32x16 s[NKT];
    float mx = NEG_BIG;
#pragma unroll
    for (int T = 0; T < NKT; ++T) {
      if (T < t_end) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[T][r] = 0.f;      // (zeroing loops local in this kernel: with zero() the NKT = 1 dropout form changes its waits)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) s[T] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(ktile, T, kk, lane), qf[kk], s[T], 0, 0, 0);
        if (32 * T + 32 > N || (CAUSAL && T == qb)) {   // only boundary tiles need masking (wave-uniform)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = 32 * T + acc_row(r, lane);
            if (!(key < N && (!CAUSAL || key <= qrow))) s[T][r] = NEG_BIG;
          }
        }
        mx = fmaxf(mx, max16(s[T]));
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = mx * c;
    float l = 0.f;
    f32x16 oacc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
#pragma unroll
    for (int T = 0; T < NKT; ++T) {
      if (T < t_end) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float pexp = fast_exp2(__builtin_fmaf(s[T][r], c, -mc));
          l += pexp;
          if constexpr (DROP) pexp *= attn_keep(a, head, min(qrow, N - 1), min(32 * T + acc_row(r, lane), N - 1));
          s[T][r] = pexp;
        }
#pragma unroll
        for (int sidx = 0; sidx < 2; ++sidx) {
          const bf16x8 pf = acc_to_frag(s[T], sidx);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
            oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(vtile, T, sidx, dt, lane), pf, oacc[dt], 0, 0, 0);
        }
      }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    if constexpr (RES)
      store_rows_T_img<32, true>(a.o + (size_t)b * N * D + hh * DH, D, N, q0, lane, oacc, inv, oimg, nullptr, a.resid_in + (size_t)b * N * D + hh * DH,
                                 a.resid_out + (size_t)b * N * D + hh * DH, D);
    else
      store_rows_T_img(a.o + (size_t)b * N * D + hh * DH, D, N, q0, lane, oacc, inv, oimg);
    if (lane < 32 && qrow < N) a.lse2[stat_index(b, a.H, hh, N, qrow)] = mc + log2f(l);
  }
}

// ------------------------------------------------------------------------------------------ forward, 129 <= N <= 256, EIGHT waves (round 3)
// attn_fwd_small_kernel gives each of its 4 waves up to two 32-row query blocks, needs 229 registers for the register-resident score row and is
// bound by memory round trips at 2 workgroups x 4 waves per CU (DESIGN.md sections 4.2, 4.4).  Here a workgroup has EIGHT waves - one query block
// each - that share the staged K / V, and the softmax is ONLINE over a rolled key-tile loop, so a wave needs 102 registers: two workgroups
// = 16 waves share a CU at the LDS footprint of the 4-wave kernel (2 x npad x 128 + 8 x 2 KiB).  93 against 103 us at B = 256, N = 197, H = 12.
// Non-causal, no dropout; RES: also writes resid_out = resid_in + bf16(o) (the 4-wave kernel's fused residual form).
// KEEP: only the queries < a.nq are wanted (the last layer of a stack whose caller keeps a prefix of the tokens).  Every wave still helps stage
// K / V - all keys are needed - and the waves whose query block starts at or beyond nq stop there; o is written compact [B*nq, H*64], lse2 at
// its usual [B, H, N] position.  A query's arithmetic does not depend on the other lanes of its block, so the kept rows are bit-identical.
// ------------------------------------------------------------------------------------------
template <int NKT, bool RES, bool KEEP = false>
__global__ __launch_bounds__(512, 4) void attn_fwd_small8_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int head = blockIdx.x;
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, head);
  constexpr int nt = NKT, npad = NKT * 32;
  char* ktile = smem;
  char* vtile = smem + npad * 128;
  char* oimg = smem + 2 * npad * 128 + wave * 2048;
  stage_tile(qbase + D, D3, N, npad, ktile, wave, lane, 8);
  stage_tile(qbase + 2 * D, D3, N, npad, vtile, wave, lane, 8);
  const int qb = (wave + head) & 7;            // rotate which waves sit out when the head has fewer than 8 query blocks
  bool active = qb < nt;
  if constexpr (KEEP) active = qb * 32 < a.nq;
  bf16x8 qf[4];
  load_lane_frags(qbase, D3, N, (active ? qb : 0) * 32, lane, qf);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) asm volatile("" : "+v"(qf[kk]));
  __syncthreads();
  if (!active) return;
  const float c = a.scale_log2e;
  const int q0 = qb * 32;
  const int qrow = q0 + (lane & 31);
  // ONLINE softmax (one key tile of scores in registers at a time): the register-resident score row of attn_fwd_small_kernel (NKT x 16 registers)
  // does not fit the 128 registers that 16 waves per CU leave a wave
  float m = NEG_BIG, l = 0.f;
  f32x16 oacc[2];
  zero(oacc);
#pragma unroll 1
  for (int T = 0; T < NKT; ++T) {
    f32x16 st;
    zero(st);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(ktile, T, kk, lane), qf[kk], st, 0, 0, 0);
    if (32 * T + 32 > N) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (!(32 * T + acc_row(r, lane) < N)) st[r] = NEG_BIG;
    }
    float mt = max16(st);
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);
    const float alpha = fast_exp2((m - mn) * c);        // first tile: exp2(-huge) = 0 on zero accumulators
    m = mn;
    const float mc = mn * c;
    float lt = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float pexp = fast_exp2(__builtin_fmaf(st[r], c, -mc));
      lt += pexp;
      st[r] = pexp;
    }
    l = l * alpha + lt;
    if (T > 0) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
    }
#pragma unroll
    for (int sidx = 0; sidx < 2; ++sidx) {
      const bf16x8 pf = acc_to_frag(st, sidx);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(vtile, T, sidx, dt, lane), pf, oacc[dt], 0, 0, 0);
    }
  }
  l += __shfl_xor(l, 32, 64);
  const float mc = m * c;
  const float inv = 1.0f / l;
  if constexpr (KEEP) {
    store_rows_T_img<16>(a.o + (size_t)b * a.nq * D + hh * DH, D, a.nq, q0, lane, oacc, inv, oimg);
    if (lane < 32 && qrow < a.nq) a.lse2[stat_index(b, a.H, hh, N, qrow)] = mc + log2f(l);
    return;
  }
  if constexpr (RES)
    store_rows_T_img<16, true>(a.o + (size_t)b * N * D + hh * DH, D, N, q0, lane, oacc, inv, oimg, nullptr, a.resid_in + (size_t)b * N * D + hh * DH,
                               a.resid_out + (size_t)b * N * D + hh * DH, D);
  else
    store_rows_T_img<16>(a.o + (size_t)b * N * D + hh * DH, D, N, q0, lane, oacc, inv, oimg);
  if (lane < 32 && qrow < N) a.lse2[stat_index(b, a.H, hh, N, qrow)] = mc + log2f(l);
}

// ------------------------------------------------------------------------------------------ backward, dQ
template <bool DROP, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, blockIdx.x);
  const int nt = (N + 31) / 32, npad = nt * 32;
  char* ktile = smem;
  char* vtile = smem + npad * 128;
  char* oimg = smem + 2 * npad * 128 + wave * 4096;
  stage_tile(qbase + D, D3, N, npad, ktile, wave, lane);
  stage_tile(qbase + 2 * D, D3, N, npad, vtile, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const float c = a.scale_log2e;
  const __bf16* obase = a.o + (size_t)b * N * D + hh * DH;
  const __bf16* dobase = a.d_o + (size_t)b * N * D + hh * DH;
  float csum_q = 0.f;
  for (int qb = (wave + blockIdx.x) & 3; qb < nt; qb += 4) {
    const int q0 = qb * 32;
    const int qrow = q0 + (lane & 31);
    bf16x8 qf[4], dof[4], of[4];           // TWIN (to "write delta") of the set-up in attn_bwd_dq_long_kernel and, with the LIM changes, attn_bwd_dq_pipe_kernel
    load_lane_frags(qbase, D3, N, q0, lane, qf);
    load_lane_frags(dobase, D, N, q0, lane, dof);
    load_lane_frags(obase, D, N, q0, lane, of);
    float delta = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int j = 0; j < 8; ++j) delta += (float)dof[kk][j] * (float)of[kk][j];
    delta += __shfl_xor(delta, 32, 64);
    const size_t stat = stat_index(b, a.H, hh, N, min(qrow, N - 1));
    const float lse2 = a.lse2[stat];
    if (lane < 32 && qrow < N) a.delta[stat] = delta;

    f32x16 dq[2];
    zero(dq);
    const int t_end = CAUSAL ? min(nt, qb + 1) : nt;
    for (int T = 0; T < t_end; ++T) {     // TWIN of the key-tile body of attn_bwd_dq_long_kernel (there: key0 for 32 * T, a.causal for CAUSAL)
      f32x16 s, dp;
      zero(s);
      zero(dp);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(ktile, T, kk, lane), qf[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(vtile, T, kk, lane), dof[kk], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pexp = fast_exp2(__builtin_fmaf(s[r], c, -lse2));
        float dpr = dp[r];
        if constexpr (DROP) dpr *= attn_keep(a, blockIdx.x, min(qrow, N - 1), min(32 * T + acc_row(r, lane), N - 1));
        s[r] = pexp * (dpr - delta);  // dS^T (the 1/sqrt(dh) factor is applied once at the end)
      }
      if (32 * T + 32 > N || (CAUSAL && T == qb)) {   // boundary tiles: zero the masked keys
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = 32 * T + acc_row(r, lane);
          if (!(key < N && (!CAUSAL || key <= qrow))) s[r] = 0.f;
        }
      }
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 dsf = acc_to_frag(s, sidx);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(ktile, T, sidx, dt, lane), dsf, dq[dt], 0, 0, 0);
      }
    }
    store_rows_T_img(a.dqkv + (size_t)b * N * D3 + hh * DH, D3, N, q0, lane, dq, a.scale, oimg, a.dbias ? &csum_q : nullptr);
  }
  if (a.dbias) atomicAdd(a.dbias + hh * DH + lane, csum_q);   // 256 contiguous bytes per wave
}

// ------------------------------------------------------------------------------------------ backward, dQ: software-pipelined form
// The loop above leaves the schedule to hipcc, which reads every LDS fragment right in front of the MFMA that consumes it and
// keeps the three stages of a key tile (S/dP products, exp + dS on the VALU, dQ products) strictly one after the other: the phase
// probe showed 1 660 cycles per tile against ~400 of matrix-pipe and ~300 of VALU work.  Here the tile count
// is a template parameter, the loop is unrolled and the stages of neighbouring tiles overlap by construction:
//   iteration T:  request K/V row fragments of tile T+2 and the transposed K fragments of tile T
//                 S, dP products of tile T+1 (fragments requested one iteration earlier)   } one scheduling region: hipcc interleaves
//                 exp, dS of tile T on the VALU                                            } the independent MFMA and VALU streams
//                 dQ += K^T.dS of tile T
// Same arithmetic in the same order as attn_bwd_dq_kernel (bit-identical results); non-causal, no dropout.
// LIM (kept-query form, NQT = ceil(nq / 32) <= NT): o and d_o are compact [B*nq, H*64] and the queries >= nq carry no gradient.  Query blocks
// < NQT are computed as usual - a lane whose query is >= nq takes dO = 0 and lse = +1e30, so its P, delta, dS and dQ are exact zeros - and the
// blocks >= NQT only write zero rows into the Q part of dqkv (the dense dgrad-qkv / dW-qkv GEMMs read them).  delta is written for queries < nq.
template <int NT, int NQT = NT, bool LIM = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_pipe_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int head = blockIdx.x;     // one workgroup per (batch, head); a persistent two-per-CU grid walking the heads is slower (backward 276 against 256 us)
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, head);
  constexpr int nt = NT, npad = NT * 32;
  char* ktile = smem;
  char* vtile = smem + npad * 128;
  char* oimg = smem + 2 * npad * 128 + wave * 4096;
  stage_tile(qbase + D, D3, N, npad, ktile, wave, lane);
  stage_tile(qbase + 2 * D, D3, N, npad, vtile, wave, lane);
  int nq = N;                      // rows of o / d_o per sequence
  if constexpr (LIM) nq = a.nq;
  const __bf16* obase = a.o + (size_t)b * nq * D + hh * DH;
  const __bf16* dobase = a.d_o + (size_t)b * nq * D + hh * DH;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const float c = a.scale_log2e;
  float csum_q = 0.f;
  // (requesting the first block's Q, dO, O rows together with the K/V staging makes this kernel slower, 272 against 259 us per
  // backward: more requests in flight only queue longer - the forward, with a third of the lane-side traffic, gains 5 % from it)
  for (int qb = (wave + head) & 3; qb < nt; qb += 4) {
    const int q0 = qb * 32;
    const int qrow = q0 + (lane & 31);
    if constexpr (LIM) {
      if (qb >= NQT) {               // no gradient reaches these queries: zero rows (8 lanes x 16 B = one 128-B head row)
        __bf16* zp = a.dqkv + (size_t)b * N * D3 + hh * DH + 8 * (lane & 7);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          const int row = q0 + (lane >> 3) + 8 * it;
          if (row < N) *(u32x4*)(zp + (size_t)row * D3) = (u32x4){0u, 0u, 0u, 0u};
        }
        continue;
      }
    }
    bf16x8 qf[4], dof[4];
    float delta = 0.f;
    {
      bf16x8 of[4];
      load_lane_frags(qbase, D3, N, q0, lane, qf);
      load_lane_frags(dobase, D, nq, q0, lane, dof);
      load_lane_frags(obase, D, nq, q0, lane, of);
      if constexpr (LIM) {
        if (qrow >= nq) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int j = 0; j < 8; ++j) dof[kk][j] = (__bf16)0.f;
        }
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) delta += (float)dof[kk][j] * (float)of[kk][j];
    }
    delta += __shfl_xor(delta, 32, 64);
    const size_t stat = stat_index(b, a.H, hh, N, min(qrow, nq - 1));
    float lse2 = a.lse2[stat];
    if constexpr (LIM) lse2 = qrow < nq ? lse2 : 1.0e30f;      // exp2(s - 1e30) = 0 exactly
    if (lane < 32 && qrow < nq) a.delta[stat] = delta;

    f32x16 dq[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
    bf16x8 kr[2][4], vr[2][4];      // row fragments of K and V, two tiles in flight
    f32x16 sb[2], dpb[2];           // S^T and dP^T of the tile on the VALU and of the next one in the matrix pipe
    auto products = [&](int buf) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { sb[buf][r] = 0.f; dpb[buf][r] = 0.f; }     // (zeroing loops local in this kernel: with zero() hipcc packs its dS arithmetic differently)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        sb[buf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kr[buf][kk], qf[kk], sb[buf], 0, 0, 0);
        dpb[buf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vr[buf][kk], dof[kk], dpb[buf], 0, 0, 0);
      }
    };
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { kr[0][kk] = row_frag(ktile, 0, kk, lane); vr[0][kk] = row_frag(vtile, 0, kk, lane); }
    if (NT > 1) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) { kr[1][kk] = row_frag(ktile, 1, kk, lane); vr[1][kk] = row_frag(vtile, 1, kk, lane); }
    }
    products(0);
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      const int cur = T & 1, nxt = cur ^ 1;
      bf16x8 ktr[2][2];
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) ktr[sidx][dt] = tr_frag(ktile, T, sidx, dt, lane);
      __builtin_amdgcn_sched_barrier(0);
      if (T + 1 < NT) products(nxt);
      if (T + 2 < NT) {             // tile T's row fragments were consumed by the products issued one iteration ago
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) { kr[cur][kk] = row_frag(ktile, T + 2, kk, lane); vr[cur][kk] = row_frag(vtile, T + 2, kk, lane); }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pexp = fast_exp2(__builtin_fmaf(sb[cur][r], c, -lse2));
        sb[cur][r] = pexp * (dpb[cur][r] - delta);  // dS^T (the 1/sqrt(dh) factor is applied once at the end)
      }
      if (T == NT - 1 && 32 * T + 32 > N) {         // boundary tile: zero the masked keys
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!(32 * T + acc_row(r, lane) < N)) sb[cur][r] = 0.f;
      }
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 dsf = acc_to_frag(sb[cur], sidx);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[sidx][dt], dsf, dq[dt], 0, 0, 0);
      }
    }
    store_rows_T_img(a.dqkv + (size_t)b * N * D3 + hh * DH, D3, N, q0, lane, dq, a.scale, oimg, a.dbias ? &csum_q : nullptr);
  }
  if (a.dbias) atomicAdd(a.dbias + hh * DH + lane, csum_q);   // 256 contiguous bytes per wave
}

// ------------------------------------------------------------------------------------------ backward, dK and dV
template <bool DROP, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, blockIdx.x);
  const int nt = (N + 31) / 32, npad = nt * 32;
  char* qtile = smem;
  char* dotile = smem + npad * 128;
  float* lse_s = (float*)(smem + 2 * npad * 128);
  float* delta_s = lse_s + npad;
  char* oimg = smem + 2 * npad * 128 + 2 * npad * 4 + wave * 4096;
  const __bf16* dobase = a.d_o + (size_t)b * N * D + hh * DH;
  stage_tile(qbase, D3, N, npad, qtile, wave, lane);
  stage_tile(dobase, D, N, npad, dotile, wave, lane);
  for (int i = threadIdx.x; i < npad; i += 256) {
    const size_t stat = stat_index(b, a.H, hh, N, min(i, N - 1));
    lse_s[i] = a.lse2[stat];
    delta_s[i] = a.delta[stat];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const float c = a.scale_log2e;
  float csum_k = 0.f, csum_v = 0.f;
  for (int kb = (wave + blockIdx.x) & 3; kb < nt; kb += 4) {
    const int k0 = kb * 32;
    const int krow = k0 + (lane & 31);
    bf16x8 kf[4], vf[4];
    load_lane_frags(qbase + D, D3, N, k0, lane, kf);
    load_lane_frags(qbase + 2 * D, D3, N, k0, lane, vf);
    f32x16 dk[2], dv[2];
    zero(dk);
    zero(dv);
    const int t_beg = CAUSAL ? kb : 0;  // queries before the key block never attend to it
    for (int T = t_beg; T < nt; ++T) {    // TWIN of the query-tile body of attn_bwd_dkv_long_kernel (there: rows r0 + ... of the staged chunk, a.causal for CAUSAL)
      f32x16 s, dp;
      zero(s);
      zero(dp);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(qtile, T, kk, lane), kf[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(dotile, T, kk, lane), vf[kk], dp, 0, 0, 0);
      }
      f32x16 pmat;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int qr = 32 * T + 8 * u + 4 * (lane >> 5);
        const f32x4 lse4 = *(const f32x4*)(lse_s + qr);
        const f32x4 del4 = *(const f32x4*)(delta_s + qr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * u + i;
          const float pexp = fast_exp2(__builtin_fmaf(s[r], c, -lse4[i]));
          float keep = 1.0f;
          if constexpr (DROP) keep = attn_keep(a, blockIdx.x, min(qr + i, N - 1), min(krow, N - 1));
          pmat[r] = pexp * keep;
          s[r] = pexp * (dp[r] * keep - del4[i]);
        }
        if (32 * T + 32 > N || k0 + 32 > N || (CAUSAL && T == kb)) {   // boundary tiles only (wave-uniform)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * u + i, query = qr + i;
            if (!(query < N && krow < N && (!CAUSAL || krow <= query))) { pmat[r] = 0.f; s[r] = 0.f; }
          }
        }
      }
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 pf = acc_to_frag(pmat, sidx);
        const bf16x8 dsf = acc_to_frag(s, sidx);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(dotile, T, sidx, dt, lane), pf, dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(qtile, T, sidx, dt, lane), dsf, dk[dt], 0, 0, 0);
        }
      }
    }
    __bf16* dbase = a.dqkv + (size_t)b * N * D3 + hh * DH;
    store_rows_T_img(dbase + D, D3, N, k0, lane, dk, a.scale, oimg, a.dbias ? &csum_k : nullptr);
    store_rows_T_img(dbase + 2 * D, D3, N, k0, lane, dv, 1.0f, oimg, a.dbias ? &csum_v : nullptr);
  }
  if (a.dbias) {
    atomicAdd(a.dbias + D + hh * DH + lane, csum_k);
    atomicAdd(a.dbias + 2 * D + hh * DH + lane, csum_v);
  }
}

// ------------------------------------------------------------------------------------------ backward, dK and dV: software-pipelined form
// Same restructuring as attn_bwd_dq_pipe_kernel (tile count a template parameter, unrolled, LDS fragments requested a stage
// ahead, the S/dP products of query tile T+1 issued before the VALU work of tile T).  Padded query rows need no masking here:
// their lse is staged as +1e30, so P and dS are exactly 0 for them; padded key lanes are never stored.  Bit-identical to
// attn_bwd_dkv_kernel; non-causal, no dropout.
// LIM (kept-query form): d_o is compact [B*nq, H*64]; only NQT = ceil(nq / 32) query tiles of Q and dO are staged and swept, the queries
// nq .. 32 NQT - 1 of the last tile are padded queries in the sense above (lse +1e30).  The tiles left out would have added exact zeros.
template <int NT, int NQT = NT, bool LIM = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_pipe_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int head = blockIdx.x;     // one workgroup per (batch, head); a persistent two-per-CU grid walking the heads is slower (backward 276 against 256 us)
  // (head_addr() spelled out in this kernel: through the helper NT = 7 spills 80 instead of 84 bytes and reorders its waits - not the parent's code)
  const int b = head / a.H, hh = head % a.H;
  const int N = a.N, D3 = 3 * a.H * DH, D = a.H * DH;
  constexpr int nt = NT, npad = NQT * 32;           // npad: staged QUERY rows
  int nq = N;
  if constexpr (LIM) nq = a.nq;
  char* qtile = smem;
  char* dotile = smem + npad * 128;
  float* lse_s = (float*)(smem + 2 * npad * 128);
  float* delta_s = lse_s + npad;
  char* oimg = smem + 2 * npad * 128 + 2 * npad * 4 + wave * 4096;
  const __bf16* qbase = a.qkv + (size_t)b * N * D3 + hh * DH;
  const __bf16* dobase = a.d_o + (size_t)b * nq * D + hh * DH;
  stage_tile(qbase, D3, N, npad, qtile, wave, lane);
  stage_tile(dobase, D, nq, npad, dotile, wave, lane);
  for (int i = threadIdx.x; i < npad; i += 256) {
    const size_t stat = ((size_t)b * a.H + hh) * N + min(i, nq - 1);
    lse_s[i] = i < nq ? a.lse2[stat] : 1.0e30f;       // padded queries: exp2(s - 1e30) = 0 exactly
    delta_s[i] = a.delta[stat];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const float c = a.scale_log2e;
  float csum_k = 0.f, csum_v = 0.f;
  for (int kb = (wave + head) & 3; kb < nt; kb += 4) {
    const int k0 = kb * 32;
    bf16x8 kf[4], vf[4];
    load_lane_frags(qbase + D, D3, N, k0, lane, kf);
    load_lane_frags(qbase + 2 * D, D3, N, k0, lane, vf);
    f32x16 dk[2], dv[2];
    zero(dk);
    zero(dv);
    bf16x8 qr[4], dor[4];           // row fragments of Q and dO of the tile whose products are issued next
    f32x16 sb, dpb;                 // (one set: 256 registers do not hold a second one next to dK, dV and the fragments)
    auto products = [&]() {
      zero(sb);
      zero(dpb);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        sb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qr[kk], kf[kk], sb, 0, 0, 0);
        dpb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dor[kk], vf[kk], dpb, 0, 0, 0);
      }
    };
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { qr[kk] = row_frag(qtile, 0, kk, lane); dor[kk] = row_frag(dotile, 0, kk, lane); }
    products();
    if (NQT > 1) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) { qr[kk] = row_frag(qtile, 1, kk, lane); dor[kk] = row_frag(dotile, 1, kk, lane); }
    }
#pragma unroll
    for (int T = 0; T < NQT; ++T) {
      bf16x8 dotr[2][2], qtr[2][2];
      f32x4 lse4[4], del4[4];
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) { dotr[sidx][dt] = tr_frag(dotile, T, sidx, dt, lane); qtr[sidx][dt] = tr_frag(qtile, T, sidx, dt, lane); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int qr0 = 32 * T + 8 * u + 4 * (lane >> 5);
        lse4[u] = *(const f32x4*)(lse_s + qr0);
        del4[u] = *(const f32x4*)(delta_s + qr0);
      }
      f32x16 pmat;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * u + i;
          const float pexp = fast_exp2(__builtin_fmaf(sb[r], c, -lse4[u][i]));
          pmat[r] = pexp;
          sb[r] = pexp * (dpb[r] - del4[u][i]);
        }
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 pf = acc_to_frag(pmat, sidx);
        const bf16x8 dsf = acc_to_frag(sb, sidx);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotr[sidx][dt], pf, dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtr[sidx][dt], dsf, dk[dt], 0, 0, 0);
        }
      }
      if (T + 1 < NQT) products();     // S, dP of the next tile queue up behind this tile's dV, dK products
      if (T + 2 < NQT) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) { qr[kk] = row_frag(qtile, T + 2, kk, lane); dor[kk] = row_frag(dotile, T + 2, kk, lane); }
      }
    }
    __bf16* dbase = a.dqkv + (size_t)b * N * D3 + hh * DH;
    store_rows_T_img(dbase + D, D3, N, k0, lane, dk, a.scale, oimg, a.dbias ? &csum_k : nullptr);
    store_rows_T_img(dbase + 2 * D, D3, N, k0, lane, dv, 1.0f, oimg, a.dbias ? &csum_v : nullptr);
  }
  if (a.dbias) {
    atomicAdd(a.dbias + D + hh * DH + lane, csum_k);
    atomicAdd(a.dbias + 2 * D + hh * DH + lane, csum_v);
  }
}

// ------------------------------------------------------------------------------------------ long sequences (N > 512)
// Same three algorithms with both sides tiled: the grid gets a second dimension over blocks of 128 "lane-side" rows
// (one 32-row block per wave: queries in forward / dQ, keys in dK-dV) and the kernel loops over LDS-staged chunks of
// CH = 512 rows of the other side (K,V or Q,dO + lse/delta), re-staging between two barriers.  The per-wave state
// (online-softmax m, l and the O accumulator; dQ; dK and dV) lives in registers across chunks.  K/V (Q/dO) are read
// ceil(N/128) times, from L2 after the first.
constexpr int CH = 512;

template <bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_long_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, blockIdx.x);
  const int nt = (N + 31) / 32;
  char* ktile = smem;
  char* vtile = smem + CH * 128;
  const int qb = blockIdx.y * 4 + wave;
  const bool active = qb < nt;                       // idle waves still stage and synchronise
  const int q0 = qb * 32, qrow = q0 + (lane & 31);
  const float c = a.scale_log2e;
  bf16x8 qf[4];
  if (active) load_lane_frags(qbase, D3, N, q0, lane, qf);
  f32x16 oacc[2];
  zero(oacc);
  float m = NEG_BIG, l = 0.f;
  const int t_end = a.causal ? min(nt, qb + 1) : nt;  // global key-tile bound
  for (int k0 = 0; k0 < N; k0 += CH) {
    const int rows = min(CH, N - k0), ntc = (rows + 31) / 32;
    __syncthreads();                                   // everyone is done with the previous chunk
    stage_tile(qbase + D + (size_t)k0 * D3, D3, rows, ntc * 32, ktile, wave, lane);
    stage_tile(qbase + 2 * D + (size_t)k0 * D3, D3, rows, ntc * 32, vtile, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    for (int T = 0; T < ntc && k0 / 32 + T < t_end; ++T) {
      const int key0 = k0 + 32 * T;        // TWIN of the key-tile body of attn_fwd_kernel
      f32x16 s;
      zero(s);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(ktile, T, kk, lane), qf[kk], s, 0, 0, 0);
      if (key0 + 32 > N || (a.causal && key0 / 32 == qb)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + acc_row(r, lane);
          if (!(key < N && (!a.causal || key <= qrow))) s[r] = NEG_BIG;
        }
      }
      float tmax = max16(s);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * c;
      const float mnew = fmaxf(m, tmax);
      const float alpha = fast_exp2(m - mnew);
      m = mnew;
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = fast_exp2(__builtin_fmaf(s[r], c, -mnew));
        psum += s[r];
        if constexpr (DROP) s[r] *= attn_keep(a, blockIdx.x, min(qrow, N - 1), min(key0 + acc_row(r, lane), N - 1));
      }
      l = l * alpha + psum;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 pf = acc_to_frag(s, sidx);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(vtile, T, sidx, dt, lane), pf, oacc[dt], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.0f / l;
  store_rows_T(a.o + (size_t)b * N * D + hh * DH, D, N, q0, lane, oacc, inv);
  if (lane < 32 && qrow < N) a.lse2[stat_index(b, a.H, hh, N, qrow)] = m + log2f(l);
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dq_long_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, blockIdx.x);
  const int nt = (N + 31) / 32;
  char* ktile = smem;
  char* vtile = smem + CH * 128;
  char* oimg = smem + 2 * CH * 128 + wave * 4096;
  const __bf16* obase = a.o + (size_t)b * N * D + hh * DH;
  const __bf16* dobase = a.d_o + (size_t)b * N * D + hh * DH;
  const int qb = blockIdx.y * 4 + wave;
  const bool active = qb < nt;
  const int q0 = qb * 32, qrow = q0 + (lane & 31);
  const float c = a.scale_log2e;
  bf16x8 qf[4], dof[4];
  float delta = 0.f, lse2 = 0.f;
  if (active) {
    bf16x8 of[4];
    load_lane_frags(qbase, D3, N, q0, lane, qf);
    load_lane_frags(dobase, D, N, q0, lane, dof);
    load_lane_frags(obase, D, N, q0, lane, of);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int j = 0; j < 8; ++j) delta += (float)dof[kk][j] * (float)of[kk][j];
    delta += __shfl_xor(delta, 32, 64);
    const size_t stat = stat_index(b, a.H, hh, N, min(qrow, N - 1));
    lse2 = a.lse2[stat];
    if (lane < 32 && qrow < N) a.delta[stat] = delta;
  }
  f32x16 dq[2];
  zero(dq);
  const int t_end = a.causal ? min(nt, qb + 1) : nt;
  for (int k0 = 0; k0 < N; k0 += CH) {
    const int rows = min(CH, N - k0), ntc = (rows + 31) / 32;
    __syncthreads();
    stage_tile(qbase + D + (size_t)k0 * D3, D3, rows, ntc * 32, ktile, wave, lane);
    stage_tile(qbase + 2 * D + (size_t)k0 * D3, D3, rows, ntc * 32, vtile, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    for (int T = 0; T < ntc && k0 / 32 + T < t_end; ++T) {
      const int key0 = k0 + 32 * T;        // TWIN of the key-tile body of attn_bwd_dq_kernel
      f32x16 s, dp;
      zero(s);
      zero(dp);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(ktile, T, kk, lane), qf[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(vtile, T, kk, lane), dof[kk], dp, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float pexp = fast_exp2(__builtin_fmaf(s[r], c, -lse2));
        float dpr = dp[r];
        if constexpr (DROP) dpr *= attn_keep(a, blockIdx.x, min(qrow, N - 1), min(key0 + acc_row(r, lane), N - 1));
        s[r] = pexp * (dpr - delta);
      }
      if (key0 + 32 > N || (a.causal && key0 / 32 == qb)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + acc_row(r, lane);
          if (!(key < N && (!a.causal || key <= qrow))) s[r] = 0.f;
        }
      }
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 dsf = acc_to_frag(s, sidx);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(ktile, T, sidx, dt, lane), dsf, dq[dt], 0, 0, 0);
      }
    }
  }
  float csum_q = 0.f;
  if (active) store_rows_T_img(a.dqkv + (size_t)b * N * D3 + hh * DH, D3, N, q0, lane, dq, a.scale, oimg, a.dbias ? &csum_q : nullptr);
  if (a.dbias && active) atomicAdd(a.dbias + hh * DH + lane, csum_q);
}

template <bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_long_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const auto [b, hh, N, D3, D, qbase] = head_addr(a.qkv, a.N, a.H, blockIdx.x);
  const int nt = (N + 31) / 32;
  char* qtile = smem;
  char* dotile = smem + CH * 128;
  float* lse_s = (float*)(smem + 2 * CH * 128);
  float* delta_s = lse_s + CH;
  char* oimg = smem + 2 * CH * 128 + 2 * CH * 4 + wave * 4096;
  const __bf16* dobase = a.d_o + (size_t)b * N * D + hh * DH;
  const int kb = blockIdx.y * 4 + wave;
  const bool active = kb < nt;
  const int k0 = kb * 32, krow = k0 + (lane & 31);
  const float c = a.scale_log2e;
  bf16x8 kf[4], vf[4];
  if (active) {
    load_lane_frags(qbase + D, D3, N, k0, lane, kf);
    load_lane_frags(qbase + 2 * D, D3, N, k0, lane, vf);
  }
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[dt][r] = 0.f; dv[dt][r] = 0.f; }
  const int t_beg = a.causal ? kb : 0;                 // global query-tile bound: earlier queries never see this key block
  for (int r0 = 0; r0 < N; r0 += CH) {
    const int rows = min(CH, N - r0), ntc = (rows + 31) / 32;
    __syncthreads();
    stage_tile(qbase + (size_t)r0 * D3, D3, rows, ntc * 32, qtile, wave, lane);
    stage_tile(dobase + (size_t)r0 * D, D, rows, ntc * 32, dotile, wave, lane);
    for (int i = threadIdx.x; i < ntc * 32; i += 256) {
      const size_t stat = stat_index(b, a.H, hh, N, min(r0 + i, N - 1));
      lse_s[i] = a.lse2[stat];
      delta_s[i] = a.delta[stat];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) continue;
    for (int T = 0; T < ntc; ++T) {
      const int Tg = r0 / 32 + T;
      if (Tg < t_beg) continue;            // TWIN of the query-tile body of attn_bwd_dkv_kernel; zeroing loops local (zero() costs this kernel 16 v_mov fewer: not the parent's code)
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(qtile, T, kk, lane), kf[kk], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag(dotile, T, kk, lane), vf[kk], dp, 0, 0, 0);
      }
      f32x16 pmat;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ql = 32 * T + 8 * u + 4 * (lane >> 5);        // row inside the staged chunk
        const f32x4 lse4 = *(const f32x4*)(lse_s + ql);
        const f32x4 del4 = *(const f32x4*)(delta_s + ql);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * u + i;
          const float pexp = fast_exp2(__builtin_fmaf(s[r], c, -lse4[i]));
          float keep = 1.0f;
          if constexpr (DROP) keep = attn_keep(a, blockIdx.x, min(r0 + ql + i, N - 1), min(krow, N - 1));
          pmat[r] = pexp * keep;
          s[r] = pexp * (dp[r] * keep - del4[i]);
        }
        if (r0 + 32 * T + 32 > N || k0 + 32 > N || (a.causal && Tg == kb)) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 4 * u + i, query = r0 + ql + i;
            if (!(query < N && krow < N && (!a.causal || krow <= query))) { pmat[r] = 0.f; s[r] = 0.f; }
          }
        }
      }
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const bf16x8 pf = acc_to_frag(pmat, sidx);
        const bf16x8 dsf = acc_to_frag(s, sidx);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(dotile, T, sidx, dt, lane), pf, dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(qtile, T, sidx, dt, lane), dsf, dk[dt], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  float csum_k = 0.f, csum_v = 0.f;
  __bf16* dbase = a.dqkv + (size_t)b * N * D3 + hh * DH;
  store_rows_T_img(dbase + D, D3, N, k0, lane, dk, a.scale, oimg, a.dbias ? &csum_k : nullptr);
  store_rows_T_img(dbase + 2 * D, D3, N, k0, lane, dv, 1.0f, oimg, a.dbias ? &csum_v : nullptr);
  if (a.dbias) {
    atomicAdd(a.dbias + D + hh * DH + lane, csum_k);
    atomicAdd(a.dbias + 2 * D + hh * DH + lane, csum_v);
  }
}

// ------------------------------------------------------------------------------------------ host side
// Fills AttnArgs and validates what every entry point validates, in this order: head_dim and the shape -> VITAMD_ERR_SHAPE, then a null
// pointer or a dropout probability outside [0, 1) -> VITAMD_ERR_ARG.  bwd: d_o, dqkv and delta are required as well.
int make_args(AttnArgs& out, bool bwd, const void* qkv, const void* o, const float* lse2, const void* d_o, void* dqkv, float* delta, float* dbias, int B,
              int N, int H, int head_dim, int causal, float p, unsigned long long seed, int nq = 0) {
  if (head_dim != DH || B <= 0 || N <= 0 || H <= 0 || N > MAX_N_LONG) return VITAMD_ERR_SHAPE;
  if (!qkv || !o || !lse2 || (bwd && (!d_o || !dqkv || !delta))) return VITAMD_ERR_ARG;
  const DropoutParams d = dropout_params(p, seed);
  if (!d.ok) return VITAMD_ERR_ARG;
  AttnArgs a{};
  a.qkv = (const __bf16*)qkv;
  a.o = (__bf16*)o;
  a.lse2 = (float*)lse2;
  a.d_o = (const __bf16*)d_o;
  a.dqkv = (__bf16*)dqkv;
  a.delta = delta;
  a.dbias = dbias;
  a.B = B;
  a.N = N;
  a.H = H;
  a.causal = causal;
  a.scale = 0.125f;                                  // 1 / sqrt(64)
  a.scale_log2e = 0.125f * 1.4426950408889634f;
  a.drop_thresh = d.thresh;
  a.drop_scale = d.scale;
  a.seed_lo = d.seed_lo;
  a.seed_hi = d.seed_hi;
  a.nq = nq;
  out = a;
  return VITAMD_OK;
}

int launched(int e) { return e ? e : hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH; }

// A runtime value as a template argument: f is a generic lambda that gets a std::integral_constant and reads decltype(arg)::value.
// with_tiles: v in [LO, HI], VITAMD_ERR_SHAPE outside (only the listed counts are instantiated).
template <int LO, int HI, typename F>
int with_tiles(int v, F f) {
  if constexpr (LO > HI) return VITAMD_ERR_SHAPE;
  else return v == LO ? f(std::integral_constant<int, LO>{}) : with_tiles<LO + 1, HI>(v, f);
}
template <typename F>
int with_flag(bool v, F f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
#define CONST_OF(arg) decltype(arg)::value

// the two pipelined backward kernels (dQ also writes delta); NQT <= NT query tiles; LIM: the kept-query form
template <int NT, int NQT, bool LIM>
int launch_bwd_pipe(const AttnArgs& a, hipStream_t stream) {
  if constexpr (NQT > NT) return VITAMD_ERR_SHAPE;
  else {
    const dim3 grid(a.B * a.H), block(256);
    if (int e = launch<attn_bwd_dq_pipe_kernel<NT, NQT, LIM>>(grid, block, 2 * NT * 32 * 128 + 4 * 4096, stream, a)) return e;
    return launch<attn_bwd_dkv_pipe_kernel<NT, NQT, LIM>>(grid, block, 2 * NQT * 32 * 128 + 2 * NQT * 32 * 4 + 4 * 4096, stream, a);
  }
}

// ------------------------------------------------------------------------------------------ the form a call takes
// THE dispatch rule: which kernel family a call launches and the template arguments it is instantiated with.  Every entry point below
// launches what this function answers (launch_fwd / launch_bwd switch on it) and vitamd_attention_form returns the same answer as a code,
// so the query cannot disagree with the launcher.  A template argument a family does not have stays 0 / false (attn_fwd_kernel and the
// long kernels read causal at run time), so two calls have equal forms exactly when they launch the same instantiations.
// (the numbers are part of the C ABI: include/vitamd.h VITAMD_ATTN_*, held equal by tests/test_attention_forms_host.py)
enum AttnFamily { ATTN_FWD_SMALL = 1, ATTN_FWD_SMALL8 = 2, ATTN_FWD_LOOP = 3, ATTN_FWD_LONG = 4, ATTN_BWD_PIPE = 5, ATTN_BWD_LOOP = 6, ATTN_BWD_LONG = 7 };
enum AttnFlag { ATTN_DROP = 0x1000, ATTN_CAUSAL = 0x2000, ATTN_RES = 0x4000, ATTN_KEEP = 0x8000 };
struct AttnForm {
  int family = 0;            // AttnFamily
  int nt = 0, nqt = 0;       // key tiles / query tiles of the instantiation; 0 where the family is not templated on them
  bool drop = false, causal = false, res = false, keep = false;      // DROP, CAUSAL, RES, KEEP (forward) or LIM (backward)
  int code() const {
    return family | nt << 4 | nqt << 8 | (drop ? ATTN_DROP : 0) | (causal ? ATTN_CAUSAL : 0) | (res ? ATTN_RES : 0) |
           (keep ? ATTN_KEEP : 0);
  }
};

// Only shapes are refused here (VITAMD_ERR_SHAPE), and the use of a kept-query form with a mask or the residual epilogue
// (VITAMD_ERR_ARG); the probability itself is make_args' to judge.  res: the forward's residual epilogue (the backward has none: ignored).
// nq = 0: the ordinary entry points; nq > 0: the kept-query ones.
int attention_form(AttnForm& out, int N, bool causal, bool drop, bool res, int nq, bool bwd) {
  if (N <= 0 || N > MAX_N_LONG || nq < 0 || nq > N) return VITAMD_ERR_SHAPE;
  if (!bwd && res && N > 256) return VITAMD_ERR_SHAPE;   // the residual epilogue lives in the register-resident-softmax kernels only
  const int nkt = (N + 31) / 32;
  AttnForm f;
  if (nq > 0) {                                           // kept-query forms: non-causal, no dropout, no residual epilogue
    f.keep = true;
    if (!bwd) {                                           // the eight-wave kernel: 129 <= N <= 256
      if (nkt < 5 || nkt > 8) return VITAMD_ERR_SHAPE;
      f.family = ATTN_FWD_SMALL8;
      f.nt = nkt;
    } else {                                              // the pipelined kernels: 33 <= N <= 224; up to 4 query tiles are instantiated
      if (nkt < 2 || nkt > 7 || nq > 128) return VITAMD_ERR_SHAPE;
      f.family = ATTN_BWD_PIPE;
      f.nt = nkt;
      f.nqt = (nq + 31) / 32;
    }
    if (causal || drop || res) return VITAMD_ERR_ARG;
  } else if (!bwd) {
    if (N > MAX_N) {
      f.family = ATTN_FWD_LONG;
      f.drop = drop;
    } else if (nkt >= 5 && nkt <= 8 && !drop && !causal) {   // eight waves, one query block each
      f.family = ATTN_FWD_SMALL8;
      f.nt = nkt;
      f.res = res;
    } else if (nkt <= 8) {                                // causal / not: compile-time (fewer scalar registers: no runtime mask branches per tile)
      f.family = ATTN_FWD_SMALL;
      f.nt = nkt;
      f.drop = drop;
      f.causal = causal;
      f.res = res;
    } else {
      f.family = ATTN_FWD_LOOP;
      f.drop = drop;
    }
  } else {
    if (N > MAX_N) {
      f.family = ATTN_BWD_LONG;
      f.drop = drop;
    } else if (!drop && !causal && nkt >= 2 && nkt <= 7) {   // the ViT shapes: pipelined forms.  (Round 4, DESIGN.md section 8: with 8 / 9 key tiles - 256 tokens: ViT-VQGAN, 288: TiTok - the fully unrolled kernels LOSE to the plain loops, 604 against 402 us at B 256, N 256, H 12 and 597 against 440 at N 288; 2-7 tiles: equal to 13 % faster)
      f.family = ATTN_BWD_PIPE;
      f.nt = f.nqt = nkt;
    } else {
      f.family = ATTN_BWD_LOOP;
      f.drop = drop;
      f.causal = causal;
    }
  }
  out = f;
  return VITAMD_OK;
}

int launch_fwd(const AttnForm& f, const AttnArgs& a, hipStream_t stream) {
  const int nkt = (a.N + 31) / 32, npad = nkt * 32;
  const dim3 heads(a.B * a.H);
  switch (f.family) {
    case ATTN_FWD_LONG:
      return with_flag(f.drop, [&](auto DR) {
        return launch<attn_fwd_long_kernel<CONST_OF(DR)>>(dim3(a.B * a.H, (nkt + 3) / 4), dim3(256), 2 * CH * 128, stream, a);
      });
    case ATTN_FWD_SMALL8:
      return with_tiles<5, 8>(f.nt, [&](auto K) {
        if (f.keep) return launch<attn_fwd_small8_kernel<CONST_OF(K), false, true>>(heads, dim3(512), 2 * npad * 128 + 8 * 2048, stream, a);
        return with_flag(f.res, [&](auto RES) {
          return launch<attn_fwd_small8_kernel<CONST_OF(K), CONST_OF(RES)>>(heads, dim3(512), 2 * npad * 128 + 8 * 2048, stream, a);
        });
      });
    case ATTN_FWD_SMALL:
      return with_tiles<1, 8>(f.nt, [&](auto K) {
        return with_flag(f.drop, [&](auto DR) {
          return with_flag(f.causal, [&](auto CAUSAL) {
            return with_flag(f.res, [&](auto RES) {
              return launch<attn_fwd_small_kernel<CONST_OF(K), CONST_OF(DR), CONST_OF(CAUSAL), CONST_OF(RES)>>(heads, dim3(256), 2 * npad * 128 + 4 * 4096,
                                                                                                           stream, a);
            });
          });
        });
      });
    case ATTN_FWD_LOOP:
      return with_flag(f.drop, [&](auto DR) { return launch<attn_fwd_kernel<CONST_OF(DR)>>(heads, dim3(256), 2 * npad * 128, stream, a); });
  }
  return VITAMD_ERR_SHAPE;
}

int launch_bwd(const AttnForm& f, const AttnArgs& a, hipStream_t stream) {
  const int nkt = (a.N + 31) / 32, npad = nkt * 32;
  const dim3 block(256);
  switch (f.family) {
    case ATTN_BWD_LONG:
      return with_flag(f.drop, [&](auto DR) {
        const dim3 grid(a.B * a.H, (nkt + 3) / 4);
        if (int el = launch<attn_bwd_dq_long_kernel<CONST_OF(DR)>>(grid, block, 2 * CH * 128 + 4 * 4096, stream, a)) return el;   // also writes delta
        return launch<attn_bwd_dkv_long_kernel<CONST_OF(DR)>>(grid, block, 2 * CH * 128 + 2 * CH * 4 + 4 * 4096, stream, a);
      });
    case ATTN_BWD_PIPE:
      if (f.keep)
        return with_tiles<2, 7>(f.nt, [&](auto K) {
          return with_tiles<1, 4>(f.nqt, [&](auto Q) { return launch_bwd_pipe<CONST_OF(K), CONST_OF(Q), true>(a, stream); });
        });
      return with_tiles<2, 7>(f.nt, [&](auto K) { return launch_bwd_pipe<CONST_OF(K), CONST_OF(K), false>(a, stream); });
    case ATTN_BWD_LOOP:
      return with_flag(f.drop, [&](auto DR) {
        return with_flag(f.causal, [&](auto CAUSAL) {
          const dim3 grid(a.B * a.H);
          if (int el = launch<attn_bwd_dq_kernel<CONST_OF(DR), CONST_OF(CAUSAL)>>(grid, block, 2 * npad * 128 + 4 * 4096, stream, a)) return el;   // also writes delta
          return launch<attn_bwd_dkv_kernel<CONST_OF(DR), CONST_OF(CAUSAL)>>(grid, block, 2 * npad * 128 + 2 * npad * 4 + 4 * 4096, stream, a);
        });
      });
  }
  return VITAMD_ERR_SHAPE;
}

int attention_fwd_impl(const void* qkv, void* o, float* lse2, const float* resid_in, float* resid_out, int B, int N, int H, int head_dim, int causal,
                       float dropout_p, unsigned long long seed, void* stream_) {
  AttnArgs a;
  if (int e = make_args(a, false, qkv, o, lse2, nullptr, nullptr, nullptr, nullptr, B, N, H, head_dim, causal, dropout_p, seed)) return e;
  a.resid_in = resid_in;
  a.resid_out = resid_out;
  AttnForm f;
  if (int e = attention_form(f, N, causal != 0, a.drop_thresh != 0u, resid_in != nullptr, 0, false)) return e;
  return launched(launch_fwd(f, a, (hipStream_t)stream_));
}

}  // namespace

// Which kernels a call would launch (nothing is launched, no pointer is needed): AttnForm::code(), or -VITAMD_ERR_* where the matching
// entry point refuses - the shape first, then the probability, as make_args orders them.
extern "C" int vitamd_attention_form(int N, int causal, float dropout_p, int resid, int nq, int backward) {
  AttnForm f;
  const DropoutParams d = dropout_params(dropout_p, 0ull);
  if (int e = attention_form(f, N, causal != 0, d.ok ? d.thresh != 0u : dropout_p != 0.f, resid != 0, nq, backward != 0)) return -e;
  if (!d.ok) return -VITAMD_ERR_ARG;
  return f.code();
}

extern "C" int vitamd_attention_fwd(const void* qkv, void* o, float* lse2, int B, int N, int H, int head_dim, int causal,
                                    float dropout_p, unsigned long long seed, void* stream_) {
  return attention_fwd_impl(qkv, o, lse2, nullptr, nullptr, B, N, H, head_dim, causal, dropout_p, seed, stream_);
}

// forward + the residual add that follows it in the layer: resid_out = resid_in + o  (fp32 [B*N, H*64]); N <= 256 only
extern "C" int vitamd_attention_fwd_resid(const void* qkv, void* o, float* lse2, const float* resid_in, float* resid_out, int B, int N,
                                          int H, int head_dim, int causal, float dropout_p, unsigned long long seed, void* stream_) {
  if (!resid_in || !resid_out) return VITAMD_ERR_ARG;
  AttnForm f;
  if (int e = attention_form(f, N, false, false, true, 0, false)) return e;      // N <= 256: answered before make_args' pointers and probability
  return attention_fwd_impl(qkv, o, lse2, resid_in, resid_out, B, N, H, head_dim, causal, dropout_p, seed, stream_);
}

extern "C" int vitamd_attention_bwd(const void* qkv, const void* o, const float* lse2, const void* d_o, void* dqkv, float* delta,
                                    float* dbias, int B, int N, int H, int head_dim, int causal, float dropout_p,
                                    unsigned long long seed, void* stream_) {
  AttnArgs a;
  if (int e = make_args(a, true, qkv, o, lse2, d_o, dqkv, delta, dbias, B, N, H, head_dim, causal, dropout_p, seed)) return e;
  AttnForm f;
  if (int e = attention_form(f, N, causal != 0, a.drop_thresh != 0u, false, 0, true)) return e;
  return launched(launch_bwd(f, a, (hipStream_t)stream_));
}

// ------------------------------------------------------------------------------------------ kept-query forms
// The last layer of a stack whose caller keeps the first nq tokens of every sequence (functions.layer_forward, keep=): attention output
// and its gradient exist for the queries < nq only, K and V for every token.  o and d_o are COMPACT [B*nq, H*64] (row b*nq + t); lse2 and
// delta keep the [B, H, N] layout and only the entries of queries < nq are written / read.  Non-causal, no dropout.  Shapes: the forward
// needs the eight-wave kernel (129 <= N <= 256), the backward the pipelined kernels (33 <= N <= 224) and nq <= 128;
// vitamd_attention_keep_forms tells.
extern "C" int vitamd_attention_keep_forms(int N, int nq) {
  if (nq <= 0) return 0;                                  // (nq = 0 names the ordinary forms in attention_form)
  AttnForm f;
  return (attention_form(f, N, false, false, false, nq, false) == VITAMD_OK ? 1 : 0) |
         (attention_form(f, N, false, false, false, nq, true) == VITAMD_OK ? 2 : 0);
}

extern "C" int vitamd_attention_fwd_keep(const void* qkv, void* o, float* lse2, int B, int N, int H, int head_dim, int nq, void* stream_) {
  AttnArgs a;
  if (int e = make_args(a, false, qkv, o, lse2, nullptr, nullptr, nullptr, nullptr, B, N, H, head_dim, 0, 0.f, 0ull, nq)) return e;
  AttnForm f;
  if (nq <= 0) return VITAMD_ERR_SHAPE;
  if (int e = attention_form(f, N, false, false, false, nq, false)) return e;
  return launched(launch_fwd(f, a, (hipStream_t)stream_));
}

extern "C" int vitamd_attention_bwd_keep(const void* qkv, const void* o, const float* lse2, const void* d_o, void* dqkv, float* delta,
                                         float* dbias, int B, int N, int H, int head_dim, int nq, void* stream_) {
  AttnArgs a;
  if (int e = make_args(a, true, qkv, o, lse2, d_o, dqkv, delta, dbias, B, N, H, head_dim, 0, 0.f, 0ull, nq)) return e;
  AttnForm f;
  if (nq <= 0) return VITAMD_ERR_SHAPE;
  if (int e = attention_form(f, N, false, false, false, nq, true)) return e;
  return launched(launch_bwd(f, a, (hipStream_t)stream_));
}
