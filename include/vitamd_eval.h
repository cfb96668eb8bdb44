/* vitamd_eval.h - the tokenizer-evaluation entry points of libvitamd.so: per-image MSE / MAE / PSNR / SSIM of a
 * reconstruction against its target, and the code-usage histogram of a quantiser's ids, both added to accumulators that stay on the
 * device.  The conventions are those of vitamd.h (device pointers, `stream` a hipStream_t passed as void*, VITAMD_OK or a VITAMD_ERR_*
 * code, nothing launched on error, only enqueues: safe under HIP-graph capture; the caller owns all memory).
 *
 * These entry points are an addition to ABI 9 of vitamd.h, which they leave as it is: vitamd_abi_version() stays 9 and no declaration
 * of vitamd.h changes.  They are declared here, not there, because the table of vitamd.h's declarations is pinned entry by entry
 * (tests/test_abi_parser_host.py) until the ABI number next changes; the binding (vitamd/lib.py) reads both headers the same way.
 */
#ifndef VITAMD_EVAL_H
#define VITAMD_EVAL_H

#include "vitamd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Image-pair metrics of a reconstruction against its target, per image, added to accumulators that stay on the device.
 * recon: [B, C, H, W] contiguous, fp32 or bf16 (recon_bf16); target: fp32 [B, C, H, W].  Neither needs 16-byte alignment: rows are read
 * in 16-byte pieces when both bases are aligned and W is a multiple of 4 (fp32 recon) or 8 (bf16 recon), element by element otherwise.
 * The contract.  Values are taken as fp32; with clamp != 0, recon (not target) is first limited to [0, R], R = data_range, by comparisons
 * that a NaN fails, so a NaN stays a NaN.  For image b:
 *   mse_b  = mean over C*H*W of (r - t)^2          mae_b = mean over C*H*W of |r - t|
 *   psnr_b = 10 log10(R^2 / mse_b)                 (+inf where mse_b == 0)
 *   ssim_b = the SSIM of Wang et al. (2004) per channel on the values as they are (no luma conversion): window 11 x 11 Gaussian,
 *            sigma 1.5, normalised to sum 1 (the kernel holds the 11 taps of the separable form as the fp64-normalised values rounded to
 *            fp32 once); only the (H-10) x (W-10) windows that lie wholly inside the image (no padding); K1 = 0.01, K2 = 0.03,
 *            C1 = (K1 R)^2, C2 = (K2 R)^2; biased weighted moments; map
 *            ((2 mu_x mu_y + C1)(2 sigma_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(sigma_x^2 + sigma_y^2 + C2));
 *            ssim_b = the plain mean of the map over channels and windows.  Identical images give exactly 1.
 * A NaN anywhere in an image makes its four values NaN, and the running sums with them; other images of the batch are untouched.
 * ssim == 0 skips the windows: H, W >= 1 suffices and ssim_b is NaN (and so is its running sum).
 * Launch one: a workgroup per vitamd_recon_metrics_tile()-square tile of one channel of one image (at most vitamd_recon_metrics_grid_cap()
 * workgroups, which loop over further tiles); every pixel and every window belongs to exactly one tile; three fp32 partial sums per tile
 * go to `ws` with plain stores (no float atomics), each an fp32 summation of depth vitamd_recon_metrics_sum_depth() at most, in a fixed
 * order.  Launch two (one workgroup, a fixed order): per image the fp64 sum of its partials in ascending tile order per lane, the four
 * values formed in fp64 and written to per_image (fp64 [B, 4] = mse, mae, psnr, ssim); then the batch is ADDED, with ordinary loads and
 * stores, to sums (fp64 [4] = the sums of mse_b, mae_b, psnr_b, ssim_b) and count (int64 [1] += B).  Zero both for a fresh evaluation;
 * the same inputs from the same state give the same bits.  Only enqueues on `stream`.  ws, per_image: written before they are read.
 * VITAMD_ERR_SHAPE: B or C < 1; H or W < 11 with ssim (< 1 without) or above VITAMD_RECON_METRICS_MAX_DIM (offsets inside one channel
 * are 32-bit); more than VITAMD_RECON_METRICS_MAX_TILES tiles in all; ws_bytes below vitamd_recon_metrics_ws_bytes(B, C, H, W, ssim).
 * VITAMD_ERR_ARG, after the shape check: data_range not a finite number above 0 (or beyond fp32), a missing pointer.  Nothing is
 * launched in either case.  vitamd_recon_metrics_ws_bytes: the bytes of `ws` (12 per tile), or -VITAMD_ERR_SHAPE.
 * replaces the l1_loss / codebook_usage lines the reference tokenizer loops log (train_titok.py:155,168 and its siblings). */
#define VITAMD_RECON_METRICS_MAX_DIM 32768
#define VITAMD_RECON_METRICS_MAX_TILES 0x7fffffff
int vitamd_recon_metrics(const void* recon, int recon_bf16, const float* target, double* per_image, double* sums, long long* count, void* ws,
                         long ws_bytes, long B, int C, int H, int W, double data_range, int clamp, int ssim, void* stream);
long vitamd_recon_metrics_ws_bytes(long B, int C, int H, int W, int ssim);
int vitamd_recon_metrics_grid_cap(void);
int vitamd_recon_metrics_tile(void);
int vitamd_recon_metrics_sum_depth(void);
/* Code-usage histogram: hist[id] += 1 for every id of ids (int64 [M]) in [0, K); bad[0] += the number of ids outside that range, which
 * form no address.  hist: int64 [K], bad: int64 [1], both ACCUMULATED into.  Integer atomics only: exact in any order, so the result is
 * reproducible.  K <= vitamd_code_hist_lds_max_k(): each workgroup counts its ids into an int32 histogram in LDS and flushes the
 * non-zero bins with one 64-bit global atomic each; above: global atomics directly.  At most vitamd_code_hist_grid_cap() workgroups,
 * which loop.  M outside 1 .. VITAMD_CODE_HIST_MAX_M or K outside 2 .. VITAMD_CODE_HIST_MAX_K: VITAMD_ERR_SHAPE; a missing pointer:
 * VITAMD_ERR_ARG (after the shape check); nothing is launched in either case.  Usage, dead codes, entropy and perplexity are formed by
 * the caller from hist.  replaces codebook_usage[indices] = 1 (train_titok.py:165 and its siblings). */
#define VITAMD_CODE_HIST_MAX_K 65536
#define VITAMD_CODE_HIST_MAX_M 0x7fffffff
int vitamd_code_hist(const long long* ids, long M, int K, long long* hist, long long* bad, void* stream);
int vitamd_code_hist_lds_max_k(void);
int vitamd_code_hist_grid_cap(void);

#ifdef __cplusplus
}
#endif
#endif /* VITAMD_EVAL_H */
