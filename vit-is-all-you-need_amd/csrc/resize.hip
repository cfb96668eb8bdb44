// Resize in the device input pipeline: vitamd_frames_prep with an antialiased bilinear resize in front of the
// crop.  Per output sample an int32 record (y0, h, Hv, oy, x0, w, Wv, ox, flip, 0): the box [y0, y0+h) x [x0, x0+w) of frame index[b] is
// resized to a virtual Hv x Wv image, of which the output is the H x W window at (oy, ox), mirrored under a flip.  The weights are
// defined in integers (include/vitamd.h): per axis S = max(h, Hv), u = 2 (o + oy) + 1, n_j = max(0, 2S - |(2j+1) Hv - u h|),
// w_j = n_j / sum n: every n_j and their sum are exact in fp32, so a weight carries one rounding.
//
// Fast form (C == 3, W % 4 == 0, p % 4 == 0 when patch rows are wanted): separable through LDS.  A workgroup owns a TH x TW output tile
// of one sample.  It computes the tile's x- and y-taps once (first tap, count, normalised weights) into LDS; the horizontal pass then
// turns the source rows the tile needs, STRIP_ROWS at a time, into an fp32 strip [row][channel][tile column] (a lane owns one tile
// column - its taps are neighbouring source bytes - and walks rows); the vertical pass adds a lane's 4 neighbouring output pixels x 3
// channels up from the strip with 16-byte LDS reads, in ascending tap order across the chunks, and stores them as the plain prep's
// fast form does (one 16-byte fp32 and one 8-byte bf16 store per channel).  The flip is applied where the x-taps are computed (tile
// column x reads window column W-1-x), so nothing after that knows of it.
// LDS: strip 80 x 3 x 32 x 4 = 30 720 B + taps 4 608 B: four workgroups per CU.  At the 8x cap a 32-row tile needs (32 + 1) x 8 = 264
// source rows = four chunks; at the 1.1 - 2.3x of a training crop one.
// Generic form (any other C, W, p or alignment): one lane per output element, both tap loops in the lane.
// Mixing (vitamd_frames_prep_resize_mix): the same kernels with MIX = true.  In the fast form the workgroup that
// owns a tile of sample b runs the separable pass for b and, where the tile takes pixels of the partner q (Mixup: always; CutMix: where
// the tile meets the box), a second time with q's record - its own taps and strip chunks on the SAME LDS, behind the barrier at the head
// of tile_pass - then normalises both accumulators and blends or selects per pixel.  A pass keeps its order of additions, so both
// images carry the bits of a stand-alone launch.  The generic form evaluates the partner's taps only where the pixel takes them.
// No atomics and a fixed order of additions: the same bits on every call.
// Every device-side value is clamped before it forms an address (box_of), and no tap loop runs past MAX_TAPS.
#include "common.h"
#include "frames_out.h"
#include "mix_row.h"

namespace {

constexpr int RESIZE_GRID_CAP = 1024;                // workgroups per launch (4 per CU: what the LDS admits); a stride loop beyond
constexpr int MAX_SIZE = VITAMD_FRAMES_MAX_SIZE;                       // of Hs, Ws, H, W and the virtual sizes: u * h and (2j+1) * Hv stay below 2^31
constexpr int MAX_TAPS = 16;                         // per axis: 2 * max(h / Hv, 1) at the 8x down-scaling cap
constexpr int TH = 32, TW = 32;                      // the output tile of a workgroup
constexpr int STRIP_ROWS = 80;                       // source rows of one horizontal pass

struct Box { const unsigned char* frame; int y0, h, Hv, oy, x0, w, Wv, ox, flip; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the record of output sample b, clamped: index into [0, Nsrc); y0 into [0, Hs-1], h into [1, Hs-y0], Hv into [max(H, ceil(h/8)), 8192],
// oy into [0, Hv-H]; x alike.  After this the box lies inside the frame, the window inside the virtual image, and an axis has at most
// MAX_TAPS taps.
__device__ __forceinline__ Box box_of(const unsigned char* src, const long long* index, const int* box, int b, int Nsrc, int Hs, int Ws, int C,
                                      int H, int W) {
  const int* r = box + (size_t)b * 10;
  Box bx;
  bx.frame = source_frame(src, index, b, Nsrc, Hs, Ws, C);
  bx.y0 = clampi(r[0], 0, Hs - 1);
  bx.h = clampi(r[1], 1, Hs - bx.y0);
  bx.Hv = clampi(r[2], max(H, (bx.h + 7) / 8), MAX_SIZE);
  bx.oy = clampi(r[3], 0, bx.Hv - H);
  bx.x0 = clampi(r[4], 0, Ws - 1);
  bx.w = clampi(r[5], 1, Ws - bx.x0);
  bx.Wv = clampi(r[6], max(W, (bx.w + 7) / 8), MAX_SIZE);
  bx.ox = clampi(r[7], 0, bx.Wv - W);
  bx.flip = r[8] != 0;
  return bx;
}

// The taps of position v of the virtual axis (v = o + oy; n source taps resized to nv): the first box-relative tap j0, their number
// nt <= MAX_TAPS, S and u * n for numer().  The non-zero n_j are those with |(2j+1) nv - u n| < 2S, clipped to [0, n).
struct Taps { int j0, nt, twoS, un, nv; };

__device__ __forceinline__ Taps taps_of(int v, int n, int nv) {
  Taps t;
  t.nv = nv;
  t.twoS = 2 * max(n, nv);
  t.un = (2 * v + 1) * n;
  const int d = 2 * nv;
  const int lo = t.un - t.twoS - nv;                 // 2j nv > lo
  const int hi = t.un + t.twoS - nv;                 // 2j nv < hi; hi > 0
  const int first = (lo >= 0 ? lo / d : -((-lo + d - 1) / d)) + 1;
  const int last = (hi + d - 1) / d - 1;
  t.j0 = max(first, 0);
  t.nt = clampi(min(last, n - 1) - t.j0 + 1, 0, MAX_TAPS);
  return t;
}

// n_j of tap j0 + k, as an exact fp32 integer
__device__ __forceinline__ float numer(const Taps& t, int k) {
  const int a = (2 * (t.j0 + k) + 1) * t.nv - t.un;
  return (float)max(0, t.twoS - (a < 0 ? -a : a));
}

__device__ __forceinline__ float numer_sum(const Taps& t) {
  float s = 0.f;                                     // integers below 16 * 16384: every partial sum is exact
  for (int k = 0; k < t.nt; ++k) s += numer(t, k);
  return s;
}

// fl(fl(fl(r / 255) - mean) / std): three separately rounded operations with true division, as data.norm_table builds its entries
// (a subtraction feeding a division leaves nothing to contract); without mean / std fl(r / 255)
__device__ __forceinline__ float finish(float r, bool norm, float mean, float std) {
  float v = __fdiv_rn(r, 255.f);
  if (norm) v = __fdiv_rn(__fsub_rn(v, mean), std);
  return v;
}

// The horizontal pass of one strip chunk for tile column hx: source rows cs + hr, cs + hr + 8, ... below ce -> strip[row - cs][c][hx].
// NT = the most taps a column of this sample can have, rounded up to 4 or 8: the lane keeps its NT weights in registers (zero past
// its own nx taps) and takes the NT * 3 source bytes behind them from the ALIGNED dwords that enclose them, as input.hip's fetch12 does,
// where src itself is 4-byte aligned and that window lies inside src; bytes past the lane's taps meet a zero weight.  Otherwise (the
// last lanes of the last frame, an odd base pointer) it loads its own nx * 3 bytes one by one.  Both are one chain of fused
// multiply-adds in ascending tap order (written as such: left to the compiler, one path was contracted and the other was not) and a
// zero weight adds +0: the same bits either way.  Issuing the loads of several rows before the first use was measured and brought
// nothing (profiles/resize/gpu_visit.md).
template <int NT>
__device__ __forceinline__ void hpass(const unsigned char* __restrict__ src, const unsigned char* col, size_t src_bytes, bool dwords, int Ws,
                                      int cs, int ce, int hr, int hx, int nx, const float (&wx)[MAX_TAPS][TW], float (&strip)[STRIP_ROWS][3][TW]) {
  constexpr int NW = NT * 3 / 4;                     // dwords of tap bytes; the aligned window has one more
  float wr[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) wr[k] = wx[k][hx];
  for (int r = cs + hr; r < ce; r += 256 / TW) {
    const unsigned char* s = col + (size_t)r * Ws * 3;
    const size_t off = (size_t)(s - src);
    float a[3] = {0.f, 0.f, 0.f};
    if (dwords && (off & ~(size_t)3) + 4 * (NW + 1) <= src_bytes) {
      const unsigned* q = (const unsigned*)(src + (off & ~(size_t)3));
      unsigned d[NW + 1];
#pragma unroll
      for (int i = 0; i <= NW; ++i) d[i] = q[i];
      const unsigned sh = (unsigned)(off & 3) * 8;
#pragma unroll
      for (int k = 0; k < NT; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int m = 3 * k + c;                   // byte of tap k, channel c
          const unsigned word = (unsigned)((((uint64_t)d[(m >> 2) + 1] << 32) | d[m >> 2]) >> sh);
          a[c] = __builtin_fmaf(wr[k], (float)((word >> (8 * (m & 3))) & 0xffu), a[c]);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        if (k < nx) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a[c] = __builtin_fmaf(wr[k], (float)s[3 * k + c], a[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) strip[r - cs][c][hx] = a[c];
  }
}

// the same pass for samples scaled down by more than 4x (9 - 16 taps, 27 - 48 bytes a lane): the weights from LDS, the bytes one by one
__device__ __forceinline__ void hpass_bytes(const unsigned char* col, int Ws, int cs, int ce, int hr, int hx, int nx,
                                            const float (&wx)[MAX_TAPS][TW], float (&strip)[STRIP_ROWS][3][TW]) {
  for (int r = cs + hr; r < ce; r += 256 / TW) {
    const unsigned char* s = col + (size_t)r * Ws * 3;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = 0; k < nx; ++k) {
      const float wgt = wx[k][hx];
      a0 = __builtin_fmaf(wgt, (float)s[3 * k], a0);
      a1 = __builtin_fmaf(wgt, (float)s[3 * k + 1], a1);
      a2 = __builtin_fmaf(wgt, (float)s[3 * k + 2], a2);
    }
    strip[r - cs][0][hx] = a0;
    strip[r - cs][1][hx] = a1;
    strip[r - cs][2][hx] = a2;
  }
}

// One separable pass: tile (ty, tx) of the sample cut with record bx -> acc, the lane's 4 neighbouring pixels x 3 channels on the
// 0..255 scale.  Called by every lane of the workgroup (it holds barriers).  The FIRST barrier is the one that lets a pass follow
// another on the same LDS: the taps and the strip are rewritten only once every lane has left the previous pass's last vertical
// accumulation (the previous tile's, or - in the mixing kernel - the receiver's pass of this tile).  After it, taps -> barrier ->
// per chunk (barrier between chunks) horizontal pass -> barrier -> vertical accumulation, in ascending tap order across the chunks.
__device__ __forceinline__ void tile_pass(const unsigned char* __restrict__ src, const Box bx, size_t src_bytes, bool dwords, int Ws, int H, int W,
                                          int ty, int tx, float (&strip)[STRIP_ROWS][3][TW], float (&wx)[MAX_TAPS][TW], float (&wy)[MAX_TAPS][TH],
                                          int (&xj0)[TW], int (&xnt)[TW], int (&yj0)[TH], int (&ynt)[TH], f32x4 (&acc)[3]) {
  const int tid = threadIdx.x;
  const int hx = tid % TW, hr = tid / TW;            // horizontal pass: tile column, first row of the walk
  const int vo = tid / (TW / 4), vg = tid % (TW / 4);   // vertical pass: tile row, group of 4 columns
  __syncthreads();                                   // the previous pass's readers of the taps and the strip are done
  if (tid < TW) {                                    // wave 0: the x-taps of tile column tid
    const int x = tx * TW + tid;
    Taps tp = {0, 0, 0, 0, 1};
    if (x < W) tp = taps_of((bx.flip ? W - 1 - x : x) + bx.ox, bx.w, bx.Wv);
    const float sum = numer_sum(tp);
    for (int k = 0; k < MAX_TAPS; ++k) wx[k][tid] = k < tp.nt ? __fdiv_rn(numer(tp, k), sum) : 0.f;
    xj0[tid] = tp.j0;
    xnt[tid] = tp.nt;
  } else if (tid >= 64 && tid < 64 + TH) {           // wave 1: the y-taps of tile row tid - 64
    const int r = tid - 64, y = ty * TH + r;
    Taps tp = {0, 0, 0, 0, 1};
    if (y < H) tp = taps_of(y + bx.oy, bx.h, bx.Hv);
    const float sum = numer_sum(tp);
    for (int k = 0; k < MAX_TAPS; ++k) wy[k][r] = k < tp.nt ? __fdiv_rn(numer(tp, k), sum) : 0.f;
    yj0[r] = tp.j0;
    ynt[r] = tp.nt;
  }
  __syncthreads();
  const int rows = min(TH, H - ty * TH);             // first and last tap are monotone in the output row
  const int ylo = yj0[0], yhi = yj0[rows - 1] + ynt[rows - 1];
  const int nx = xnt[hx], my_j0 = yj0[vo], my_nt = ynt[vo];
  const int nt_max = (2 * max(bx.w, bx.Wv) + bx.Wv - 1) / bx.Wv;       // ceil(2S / Wv): no column of this sample has more taps
  const unsigned char* col = bx.frame + ((size_t)bx.y0 * Ws + bx.x0 + xj0[hx]) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int cs = ylo; cs < yhi; cs += STRIP_ROWS) {
    const int ce = min(cs + STRIP_ROWS, yhi);
    if (cs != ylo) __syncthreads();                  // the previous chunk's vertical pass is done with the strip
    if (nt_max <= 4) hpass<4>(src, col, src_bytes, dwords, Ws, cs, ce, hr, hx, nx, wx, strip);
    else if (nt_max <= 8) hpass<8>(src, col, src_bytes, dwords, Ws, cs, ce, hr, hx, nx, wx, strip);
    else hpass_bytes(col, Ws, cs, ce, hr, hx, nx, wx, strip);
    __syncthreads();
    const int k0 = max(cs - my_j0, 0), k1 = min(ce - my_j0, my_nt);
    for (int k = k0; k < k1; ++k) {
      const float wgt = wy[k][vo];
      const int r = my_j0 + k - cs;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += wgt * *(const f32x4*)&strip[r][c][4 * vg];
    }
  }
}

// MIX: vitamd_frames_prep_resize_mix.  The workgroup runs the pass for the receiver b and, where the tile takes any of the partner's
// pixels (every tile of a mode-1 sample, the tiles of a mode-2 sample that meet its box), a second pass with q's record on the SAME
// LDS - its own taps, nt_max and strip chunks; tile_pass's first barrier keeps it off the first pass's readers.  A mode-2 tile that
// lies wholly inside the box takes nothing of b and skips the receiver's pass.  Which passes run depends on the sample's record and
// the tile alone, so every lane of the workgroup reaches the same barriers.  Both accumulators are finished (normalised) before they
// are blended or selected per pixel.  The plain kernel is the MIX = false instantiation: one pass, nothing else compiled in.
template <bool MIX>
__global__ __launch_bounds__(256) void frames_prep_resize_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ index,
                                                                 const int* __restrict__ box, const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv, __bf16* __restrict__ patches,
                                                                 float* __restrict__ image, int B, int Nsrc, int Hs, int Ws, int H, int W,
                                                                 int p, size_t src_bytes, bool dwords, const int* __restrict__ rec,
                                                                 const float* __restrict__ lam) {
  __shared__ __attribute__((aligned(16))) float strip[STRIP_ROWS][3][TW];
  __shared__ float wx[MAX_TAPS][TW], wy[MAX_TAPS][TH];
  __shared__ int xj0[TW], xnt[TW], yj0[TH], ynt[TH];
  const int tid = threadIdx.x;
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const unsigned per_sample = (unsigned)tiles_x * tiles_y;
  const size_t total = (size_t)B * per_sample;
  const FramesOut out = {patches, image, H, W, 3, p, patches ? H / p : 0, patches ? W / p : 0, 3 * p * p};
  const bool norm = mean != nullptr;
  const int vo = tid / (TW / 4), vg = tid % (TW / 4);   // the lane's tile row and group of 4 columns (tile_pass's vertical pass)
  for (size_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const int b = (int)(tile / per_sample);
    const unsigned t = (unsigned)(tile - (size_t)b * per_sample);
    const int ty = (int)(t / (unsigned)tiles_x), tx = (int)(t - (unsigned)ty * tiles_x);
    f32x4 acc[3] = {}, accq[3] = {};                 // a pass that is skipped leaves zeros, which no pixel then takes
    MixRow mr = {};
    bool pass_b = true, pass_q = false;
    if constexpr (MIX) {
      mr = mix_row(rec, lam, b, B, H, W);
      const int y0 = ty * TH, y1 = min(y0 + TH, H), x0 = tx * TW, x1 = min(x0 + TW, W);      // the tile's pixels: [y0, y1) x [x0, x1)
      if (mr.mode == 1) {
        pass_q = true;
      } else if (mr.mode == 2) {
        pass_q = mr.yl < mr.yh && mr.xl < mr.xh && mr.yl < y1 && mr.yh > y0 && mr.xl < x1 && mr.xh > x0;      // the box meets the tile
        pass_b = !(mr.yl <= y0 && mr.yh >= y1 && mr.xl <= x0 && mr.xh >= x1);                                 // and does not cover it
      }
    }
    if (pass_b) tile_pass(src, box_of(src, index, box, b, Nsrc, Hs, Ws, 3, H, W), src_bytes, dwords, Ws, H, W, ty, tx, strip, wx, wy, xj0, xnt, yj0, ynt, acc);
    if constexpr (MIX) {
      if (pass_q) tile_pass(src, box_of(src, index, box, mr.q, Nsrc, Hs, Ws, 3, H, W), src_bytes, dwords, Ws, H, W, ty, tx, strip, wx, wy, xj0, xnt, yj0, ynt, accq);
    }
    const int y = ty * TH + vo, x = tx * TW + 4 * vg;
    if (y < H && x < W) {                            // W % 4 == 0: a group of 4 columns is inside or outside as a whole
      const bool in_rows = MIX && mr.mode == 2 && y >= mr.yl && y < mr.yh;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float m = norm ? mean[c] : 0.f, sd = norm ? stdv[c] : 1.f;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if constexpr (MIX) {
            const bool take = in_rows && x + j >= mr.xl && x + j < mr.xh;      // a pixel outside the box never reads accq, one inside never acc
            if (mr.mode == 1) v[j] = blend(finish(acc[c][j], norm, m, sd), finish(accq[c][j], norm, m, sd), mr.l, mr.m);
            else v[j] = finish(take ? accq[c][j] : acc[c][j], norm, m, sd);
          } else {
            v[j] = finish(acc[c][j], norm, m, sd);
          }
        }
        out.store4(b, c, y, x, v);
      }
    }
  }
}

// element (c, y, x) of the sample cut with record bx, on the 0..255 scale: both tap loops in the lane
__device__ __forceinline__ float resize_elem(const Box bx, int c, int y, int x, int Ws, int C, int W) {
  const Taps tx = taps_of((bx.flip ? W - 1 - x : x) + bx.ox, bx.w, bx.Wv), ty = taps_of(y + bx.oy, bx.h, bx.Hv);
  const float sx = numer_sum(tx), sy = numer_sum(ty);
  const unsigned char* s = bx.frame + ((size_t)(bx.y0 + ty.j0) * Ws + bx.x0 + tx.j0) * C + c;
  float r = 0.f;
  for (int ky = 0; ky < ty.nt; ++ky) {
    float row = 0.f;
    for (int kx = 0; kx < tx.nt; ++kx) row += __fdiv_rn(numer(tx, kx), sx) * (float)s[((size_t)ky * Ws + kx) * C];
    r += __fdiv_rn(numer(ty, ky), sy) * row;
  }
  return r;
}

// MIX: the partner's taps are evaluated only where the pixel takes them (every pixel of a mode-1 sample, the box of a mode-2 one); a
// pixel inside the box evaluates the partner's alone
template <bool MIX>
__global__ __launch_bounds__(256) void frames_prep_resize_generic_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ index,
                                                                         const int* __restrict__ box, const float* __restrict__ mean,
                                                                         const float* __restrict__ stdv, __bf16* __restrict__ patches,
                                                                         float* __restrict__ image, int B, int Nsrc, int Hs, int Ws, int C, int H,
                                                                         int W, int p, const int* __restrict__ rec, const float* __restrict__ lam) {
  const size_t total = (size_t)B * C * H * W;
  const FramesOut out = {patches, image, H, W, C, p, patches ? H / p : 0, patches ? W / p : 0, C * p * p};
  const bool norm = mean != nullptr;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {      // i = the element of image
    size_t t = i;
    const int x = (int)(t % W); t /= W;
    const int y = (int)(t % H); t /= H;
    const int c = (int)(t % C);
    const int b = (int)(t / C);
    int from = b;
    MixRow mr = {};
    if constexpr (MIX) {
      mr = mix_row(rec, lam, b, B, H, W);
      if (mr.mode == 2 && y >= mr.yl && y < mr.yh && x >= mr.xl && x < mr.xh) from = mr.q;
    }
    const float r = resize_elem(box_of(src, index, box, from, Nsrc, Hs, Ws, C, H, W), c, y, x, Ws, C, W);
    float v = finish(r, norm, norm ? mean[c] : 0.f, norm ? stdv[c] : 1.f);
    if constexpr (MIX) {
      if (mr.mode == 1) {
        const float rq = resize_elem(box_of(src, index, box, mr.q, Nsrc, Hs, Ws, C, H, W), c, y, x, Ws, C, W);
        v = blend(v, finish(rq, norm, norm ? mean[c] : 0.f, norm ? stdv[c] : 1.f), mr.l, mr.m);
      }
    }
    out.store1(i, b, c, y, x, v);
  }
}

// the two entries: rec == nullptr launches the plain kernels
template <bool MIX>
int frames_prep_resize(const unsigned char* src, const long long* index, const int* box, const float* mean, const float* std, void* patches_bf16,
                       float* image, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p, const int* rec, const float* lam,
                       void* stream) {
  long long n_src, n_out;
  if (std::max({Hs, Ws, H, W}) > MAX_SIZE || frames_shape(patches_bf16 != nullptr, index != nullptr, B, Nsrc, Hs, Ws, C, H, W, p, &n_src, &n_out)) return VITAMD_ERR_SHAPE;
  if (!src || !box || (mean == nullptr) != (std == nullptr) || (!patches_bf16 && !image) || (MIX && !rec)) return VITAMD_ERR_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const bool aligned = ((uintptr_t)image & 15) == 0 && ((uintptr_t)patches_bf16 & 7) == 0;      // of the 16- and 8-byte stores
  if (C == 3 && W % 4 == 0 && (!patches_bf16 || p % 4 == 0) && aligned) {
    const size_t tiles = (size_t)B * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
    hipLaunchKernelGGL(frames_prep_resize_kernel<MIX>, capped_grid(tiles, 1, RESIZE_GRID_CAP), dim3(256), 0, st, src, index, box, mean, std, (__bf16*)patches_bf16, image, B, Nsrc,
                       Hs, Ws, H, W, p, (size_t)n_src, ((uintptr_t)src & 3) == 0, rec, lam);
  } else {
    hipLaunchKernelGGL(frames_prep_resize_generic_kernel<MIX>, capped_grid((size_t)n_out, 256, RESIZE_GRID_CAP), dim3(256), 0, st, src, index, box, mean, std, (__bf16*)patches_bf16, image,
                       B, Nsrc, Hs, Ws, C, H, W, p, rec, lam);
  }
  return hipGetLastError() == hipSuccess ? VITAMD_OK : VITAMD_ERR_LAUNCH;
}

}  // namespace

extern "C" int vitamd_frames_prep_resize_grid_cap(void) { return RESIZE_GRID_CAP; }

extern "C" int vitamd_frames_prep_resize(const unsigned char* src, const long long* index, const int* box, const float* mean, const float* std,
                                         void* patches_bf16, float* image, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p,
                                         void* stream) {
  return frames_prep_resize<false>(src, index, box, mean, std, patches_bf16, image, B, Nsrc, Hs, Ws, C, H, W, p, nullptr, nullptr, stream);
}

extern "C" int vitamd_frames_prep_resize_mix(const unsigned char* src, const long long* index, const int* box, const float* mean,
                                             const float* std, void* patches_bf16, float* image, int B, int Nsrc, int Hs, int Ws, int C, int H,
                                             int W, int p, const int* rec, const float* lam, void* stream) {
  return frames_prep_resize<true>(src, index, box, mean, std, patches_bf16, image, B, Nsrc, Hs, Ws, C, H, W, p, rec, lam, stream);
}
