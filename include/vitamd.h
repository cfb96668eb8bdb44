/* vitamd.h — C ABI of libvitamd.so, the MI355X (gfx950) kernels behind the ViT training hot path
 * (the KV-cached decoding of the causal stack, and the loss and embedding kernels of its training step).
 *
 * The reference (SnakeOnex/vit-is-all-you-need) has no FFI layer: its hot path is a handful of
 * PyTorch ATen calls made from transformer.py and train_vit.py.  Each entry point below replaces
 * one (or a fused group) of those call sites; the citation after "replaces" is the reference
 * file:line.  A maintainer binds them with ctypes; the build's own
 * `vit-is-all-you-need_amd/vitamd/lib.py` is exactly that binding.
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HBM), row-major, 16-byte aligned.  "bf16" buffers are
 *     passed as void*; fp32 buffers as float*.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Every entry point except vitamd_init only enqueues work:
 *     no allocation, no synchronisation, safe under HIP-graph capture.
 *   - vitamd_init(device, stream) is called once per device before the first GEMM with a GELU epilogue: it is the ONLY function that
 *     allocates (one 16-KiB table image per device) and synchronises.  A GELU launch on a device without it returns VITAMD_ERR_INIT.
 *   - Every function returns VITAMD_OK (0) or a VITAMD_ERR_* code and launches nothing on error.
 *   - The caller owns all memory.  Kernels never allocate.
 *   - ONE HIP runtime per process: load this library after the framework that owns the streams and pointers you pass in (PyTorch bundles
 *     its own libamdhip64; a second copy pulled in by an earlier dlopen of this library fails the first launch) - see INTEGRATION.md.
 */
#ifndef VITAMD_H
#define VITAMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define VITAMD_OK 0
#define VITAMD_ERR_SHAPE 1   /* unsupported / inconsistent dimensions */
#define VITAMD_ERR_ARG 2     /* missing pointer or bad enum */
#define VITAMD_ERR_LAUNCH 3  /* HIP reported a launch error */
#define VITAMD_ERR_INIT 4    /* vitamd_init has not run for the current device (GELU epilogues need its table) */

/* ABI version of this header (bumped on any signature change): 9 (the KV-cached decoding entry points; the cross-entropy and token-embedding
 * entry points, the multi-tensor optimiser entry points vitamd_mt_* and the table advance vitamd_sched_*, were added to 9 without changing
 * an existing signature; so was the evaluation entry point vitamd_classify_metrics). */
int vitamd_abi_version(void);

/* Per-device set-up, once per device and process (idempotent; device < 0 = the current device; never inside a stream capture): builds the
 * 4 096-entry table {bf16(gelu(x)), bf16(gelu'(x))} of every bf16 input 2^-13 <= |x| < 8, correctly rounded from float64, that all GELU
 * epilogues read (replaces the erf of nn.GELU(), transformer.py:38, exactly).  The only entry point that allocates or synchronises. */
int vitamd_init(int device, void* stream);

/* ---- Linear layers: C[M,N] = A[M,K] . B[N,K]^T, bf16 operands, fp32 accumulation (MFMA) ------
 * epilogue selectors (argument `epi`):                                                          */
#define VITAMD_EPI_BIAS_BF16 0 /* out bf16 = bf16(acc + bias)                      replaces transformer.py:21,27 (qkv Linear) */
#define VITAMD_EPI_GELU 1      /* out bf16 = pre-activation, out2 bf16 = erf-GELU  replaces transformer.py:37-38 (Linear + nn.GELU) */
#define VITAMD_EPI_RESID_F32 2 /* out f32 = aux_f32 + bf16(acc + bias)             replaces transformer.py:39-40,44 (Linear + Dropout(0) + residual add) */
#define VITAMD_EPI_DGELU 3     /* out bf16 = bf16(acc) * gelu'(aux_bf16); colsum += column sums   (backward of transformer.py:38-39) */
#define VITAMD_EPI_PATCH_F32 4 /* out f32[b*seq+extra+p] = bf16(acc+bias) + aux_f32[p]  replaces train_vit.py:39-41 (Conv2d patchify + rearrange + pos_emb) */
#define VITAMD_EPI_F32 5       /* out f32 = acc */
#define VITAMD_EPI_GELU_DG 6   /* as GELU, but out bf16 = gelu'(pre-activation): the derivative is evaluated here, where its exp is
                                  shared with the erf and the VALU work hides under the output stores */
#define VITAMD_EPI_DMUL 7      /* as DGELU, but aux_bf16 already holds gelu'(pre) (written by GELU_DG): out = bf16(bf16(acc) * aux) */

/* Requirements: K % 64 == 0 (whatever the first argument check lets through: K = 96 is VITAMD_ERR_SHAPE from every tile code, nothing
 * written), N % 4 == 0, ldo % 4 == 0, ldo >= N.  `ldo` (elements) is the row stride of `out` AND of `out2`, of the RESID / DGELU / DMUL `aux`
 * and of the PATCH position table aux_f32[n_patches][ldo]; A and B are dense (row stride K), bias and colsum hold N elements.  Columns
 * N .. ldo-1 of every row, and the rows a PATCH launch skips, are neither read nor written.  N % 8 != 0 or ldo % 8 != 0 takes the
 * direct-store epilogue inside the 256- / 320-row kernels (4-column pieces per lane instead of 8-column row segments): same results, bit for
 * bit.  The loader-wave and seam forms (2048 / 4096) exist for N % 8 == 0 and ldo % 8 == 0 only, their dGELU-multiply epilogue for
 * N % 256 == 0 only: VITAMD_ERR_SHAPE otherwise.  bias may be NULL.  `tile`: 0 = auto; 128 = the 128x128 small-problem
 * kernel; 256 / 320 = the ping-pong kernel on 256- / 320-row tiles (320: bias, GELU, residual and dGELU epilogues only),
 * one workgroup per tile.  Auto launches problems with more tiles than CUs PERSISTENT (one workgroup per CU walking a strided tile
 * list: faster next to a second stream's kernels, but sensitive to CUs held by other long-running kernels, e.g. collectives; with a
 * short reduction dim (K <= 1536) and >= 3 tiles per CU in the form that requests the next tile's operands before the epilogue);
 * 512 = auto without persistent launches; 1024 = auto with persistent launches but without the seam / loader forms; 2048 = the
 * loader-wave form (256-row tiles, twelve waves per workgroup, four of them only issue the operand requests; bias / GELU / dGELU-multiply
 * epilogues, K % 128 == 0; VITAMD_ERR_SHAPE where it does not apply); 4096 = the seam form on 256-row tiles (the same epilogues, K % 64 == 0,
 * K >= 128; VITAMD_ERR_SHAPE where it does not apply).  All forms give bit-identical results.  With VITAMD_EPI_DMUL, colsum may be NULL:
 * the seam and loader forms then run without the column sums in their epilogue (the bias gradient can come from
 * vitamd_gemm_tn_bf16_ws_colsum instead); `out` is bit-identical either way.
 * Sizes: A, out, out2 and aux may be of any size.  The kernels on 256-column tiles address their operands with 32-bit byte offsets, so a
 * call whose A (M x K x 2 bytes) or out (M x ldo x 2, or x 4 for the fp32 outputs) reaches 2^31 bytes is run as several launches over ROW
 * PANELS of M, each below 2^31 bytes in both, with re-based pointers (and dropout indices that stay global); panel heights are multiples
 * of 1280 rows, so every panel but the last is cut into the tiles of one big launch: same results, bit for bit, and colsum is added to by
 * every panel.  What a row split cannot shrink is VITAMD_ERR_SHAPE with nothing written: B (N x K x 2 bytes) of 2^31 bytes or more, a row
 * so wide that 1280 of them do not fit, and VITAMD_EPI_PATCH_F32 with M x K x 2 or M x ldo x 4 of 2^31 bytes or more (its output row
 * depends on the global row index).  No case was given up to refusal beyond these.
 * Forward of nn.Linear (x W^T + b): A = x, B = W.  Input gradient (dy W): A = dy, B = W^T. */
int vitamd_gemm_nt_bf16(const void* A, const void* B, void* out, void* out2, const float* bias, const void* aux,
                        float* colsum, int M, int N, int K, int ldo, int epi, int n_patches, int seq, int extra,
                        int tile, void* stream);

/* Which kernel the call above would launch for these arguments on the current device (nothing is launched, no pointer is needed):
 * VITAMD_NT_FORM_* | tile rows << 8, | VITAMD_NT_FORM_TAIL_SPLIT when the launch is cut into a head of whole rounds in that form and a
 * tail on 128x128 tiles; a negative value is -VITAMD_ERR_*.  For a call that is cut into row panels (above) the answer is that of its
 * full-height panels; the last, shorter panel may take another form. */
#define VITAMD_NT_FORM_SMALL 1          /* 128x128 tiles, 4 waves */
#define VITAMD_NT_FORM_PP 2             /* ping-pong kernel, one workgroup per tile */
#define VITAMD_NT_FORM_PP_PERSISTENT 3  /* ping-pong kernel, one workgroup per CU walking a tile list */
#define VITAMD_NT_FORM_SEAM 4           /* persistent, the next tile's fill requested before the epilogue */
#define VITAMD_NT_FORM_LOADER 5         /* persistent, 8 compute waves + 4 loader waves */
#define VITAMD_NT_FORM_TAIL_SPLIT 0x80
int vitamd_gemm_nt_plan(int M, int N, int K, int ldo, int epi, int tile);

/* vitamd_gemm_nt_bf16 with a caller's workspace (added to ABI 9: no signature changed).  A launch that would take the 128x128 kernel on fewer
 * tiles than the device has CUs - a few hundred rows against a whole weight: the kept-row layer, the classifier head - leaves most of the chip
 * idle while each workgroup walks the whole K loop alone.  With `ws` it runs the SPLIT-K form instead: tiles x splits workgroups, each one tile
 * and one K range, storing fp32 partial tiles to `ws` with plain stores, then a reduce pass that sums them in split order and applies the
 * epilogue.  No atomics, no waiting between workgroups: the same inputs give the same bits, which differ from the unsplit kernel's by fp32
 * summation order only.  Split: `tile` one of the automatic codes (0, 512, 1024; explicit codes keep their meaning), one 128x128-kernel launch
 * (no row panels, no tail split), epilogue not VITAMD_EPI_PATCH_F32 (colsum, where given, is added to by the reduce pass).  splits = 0: the rule - M <= 256 (two tile rows) and
 * floor(CUs / (2 N/128)) splits, every split at least 2 K-tiles of 64: a function of N, K and the device alone, so that a row's sum does not
 * depend on how many rows the launch has; splits = n > 0: n splits whatever the shape (capped at K / 128); 1: never split.  Everything else,
 * and ws == NULL, is vitamd_gemm_nt_bf16 unchanged.  vitamd_gemm_nt_ws_bytes: the bytes of `ws` the call needs (0: it does not split;
 * negative: -VITAMD_ERR_*; a shorter ws_bytes is VITAMD_ERR_ARG).  vitamd_gemm_nt_ws_plan: vitamd_gemm_nt_plan's
 * answer for the call, or VITAMD_NT_FORM_SPLITK | 128 << 8 | splits << 16.  (vitamd_gemm_nt_plan keeps describing vitamd_gemm_nt_bf16, which
 * has no workspace and never splits.) */
#define VITAMD_NT_FORM_SPLITK 6         /* 128x128 tiles, split-K partials + reduce pass (vitamd_gemm_nt_bf16_ws only) */
int vitamd_gemm_nt_bf16_ws(const void* A, const void* B, void* out, void* out2, const float* bias, const void* aux,
                           float* colsum, int M, int N, int K, int ldo, int epi, int n_patches, int seq, int extra,
                           int tile, int splits, float* ws, long ws_bytes, void* stream);
long vitamd_gemm_nt_ws_bytes(int M, int N, int K, int ldo, int epi, int tile, int splits);
int vitamd_gemm_nt_ws_plan(int M, int N, int K, int ldo, int epi, int tile, int splits);

/* fc2 with dropout: out f32 = resid + dropout_p(bf16(A.B^T + bias)), mask = hash(seed, row*N+col).
 * replaces transformer.py:39-40,44 (Linear + nn.Dropout(p) + residual add) in training mode.  `tile` as for vitamd_gemm_nt_bf16 (0, 128,
 * 256, 320, 512, 1024), and so are the size rules: out and resid (M x N x 4 bytes) of 2^31 bytes or more are served in row panels whose
 * mask indices stay row*N+col of the whole call; B of 2^31 bytes or more is VITAMD_ERR_SHAPE. */
int vitamd_linear_dropout_resid_bf16(const void* A, const void* B, float* out, const float* bias, const float* resid,
                                     int M, int N, int K, float dropout_p, unsigned long long seed, int tile, void* stream);

/* Weight gradient: out[P,Q] (fp32) += sum_r L[r,p] * Rm[r,q]   (dW = dY^T X).  Accumulates with
 * fp32 atomics, so `out` must hold the running gradient (zeros for a fresh one).
 * replaces the autograd backward of transformer.py:21,37,39 and train_vit.py:34.
 * Requirements: ldl % 8 == 0, ldr % 8 == 0.  `splits` 0 = auto.
 * Sizes (all three vitamd_gemm_tn_bf16* entry points): L and Rm are addressed with 32-bit byte offsets from their first element, the
 * zero-filled stage past the last row included: (R + 64) x ldl x 2 and (R + 64) x ldr x 2 must both be below 2^31, VITAMD_ERR_SHAPE with
 * nothing written otherwise (cut R and accumulate).  `out`, `ws` and colsum are addressed with 64-bit pointers. */
int vitamd_gemm_tn_bf16(const void* L, const void* Rm, float* out, int R, int P, int Q, int ldl, int ldr, int ldo,
                        int splits, void* stream);

/* Same GEMM with a caller-provided split-K workspace (>= splits * ceil(P/256) * ceil(Q/256) * 256 KiB;
 * vitamd_gemm_tn_ws_bytes tells, and adds the 1 KiB per split and row tile that vitamd_gemm_tn_bf16_ws_colsum needs): partial tiles are written with plain stores and summed by a second
 * pass (bitwise reproducible, ~4x the rate of the atomic form).  accumulate = 0 overwrites `out`.
 * `form` picks the kernel (same results): which one is faster depends on what runs beside the launch. */
#define VITAMD_TN_FORM_SHARED 0    /* 8 waves per workgroup, 2/3 of the register file: waves of other kernels (LayerNorm) can share the CU */
#define VITAMD_TN_FORM_EXCLUSIVE 1 /* 12 waves (4 of them only issue the LDS-DMA requests): 15 % faster alone, fills the CU; bit-identical */
int vitamd_gemm_tn_bf16_ws(const void* L, const void* Rm, float* out, int R, int P, int Q, int ldl, int ldr, int ldo,
                           int splits, float* ws, long ws_bytes, int accumulate, int form, void* stream);
long vitamd_gemm_tn_ws_bytes(int R, int P, int Q, int splits);

/* The workspace form that also sums the columns of L: colsum[p] += sum_r float(L[r,p]) for p < P (fp32 [P], caller-zeroed or holding a
 * running sum) - the bias gradient of the Linear whose weight gradient the call forms, taken from the operand tiles the GEMM stages anyway.
 * The sums are formed by the workgroups of the first column tile beside their MFMAs; their partials (256 floats per split and row tile)
 * lie behind the partial tiles in `ws` - vitamd_gemm_tn_ws_bytes counts them - and the reduce pass adds them in split order: no atomics,
 * bitwise reproducible.  `out` is bit-identical to vitamd_gemm_tn_bf16_ws's.  colsum == NULL is that call; a workspace that is missing
 * or too small is VITAMD_ERR_ARG (the atomic form has no reduce pass to sum in). */
int vitamd_gemm_tn_bf16_ws_colsum(const void* L, const void* Rm, float* out, float* colsum, int R, int P, int Q, int ldl, int ldr,
                                  int ldo, int splits, float* ws, long ws_bytes, int accumulate, int form, void* stream);

/* ---- LayerNorm (no affine, eps as given) on the fp32 residual stream -------------------------
 * forward: x = x_in (+ addend_bf16 -> also written to x_out); y = bf16(LN(x)); mean/rstd saved.
 * replaces transformer.py:43-44 `F.layer_norm(x, (n_embd,))` and the residual add of :43. */
int vitamd_layernorm_fwd(const float* x_in, const void* addend_bf16, float* x_out, void* y_bf16, float* mean,
                         float* rstd, int M, int D, float eps, void* stream);
/* backward: g_out = (g_res ? g_res : 0) + LN'(dy_bf16); optional bf16 copy of g_out and its column sums. */
int vitamd_layernorm_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                         const float* g_res, float* g_out, void* g_bf16, float* colsum, int M, int D, void* stream);
/* same; the bf16 copy additionally carries the dropout mask (p, seed; element index row*D+col) of the
 * Linear output whose gradient it is (backward of the nn.Dropout of transformer.py:40). */
int vitamd_layernorm_bwd_dropout(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                 const float* g_res, float* g_out, void* g_bf16, float* colsum, int M, int D,
                                 float dropout_p, unsigned long long seed, void* stream);
/* Same backward with xhat read back from the forward's bf16 output y_bf16 (for this non-affine LayerNorm y IS xhat, and it is
 * saved anyway as the operand of the following Linear's weight gradient) instead of recomputed from x: 14 instead of 16 B per
 * element of an HBM-bound kernel; D in {256, 512, 768, 1024}; dropout_p = 0 for no mask on the bf16 copy. */
int vitamd_layernorm_bwd_xhat(const void* dy_bf16, const void* y_bf16, const float* rstd, const float* g_res, float* g_out,
                              void* g_bf16, float* colsum, int M, int D, float dropout_p, unsigned long long seed, void* stream);
/* Kept-row forms, for the LAST layer of a stack whose caller keeps the first `keep` tokens of every `seq` (0 < keep <= seq).
 * forward: B*keep output rows; row b*keep + t = LN(x_in[b*seq + t] + addend[b*keep + t]).  x_in is the full fp32 stream [B*seq, D];
 * addend (bf16, required: the kept-query attention output), x_out, y, mean and rstd are compact [B*keep, ...].  Per-row arithmetic
 * as vitamd_layernorm_fwd. */
int vitamd_layernorm_fwd_keep(const float* x_in, const void* addend_bf16, float* x_out, void* y_bf16, float* mean, float* rstd,
                              int B, int seq, int keep, int D, float eps, void* stream);
/* backward over all B*seq rows with a COMPACT g_res fp32 [B*keep, D] (required): row b*seq + t adds g_res[b*keep + t] when t < keep
 * and nothing otherwise (those rows of the dense g_res would be zeros and are never read).  use_xhat != 0: x_or_y is the forward's
 * bf16 output as in vitamd_layernorm_bwd_xhat (D in {256, 512, 768, 1024}; mean may be NULL); 0: the fp32 input with mean / rstd as
 * in vitamd_layernorm_bwd_dropout.  g_bf16, colsum, dropout_p, seed as there. */
int vitamd_layernorm_bwd_keep(const void* dy_bf16, const void* x_or_y, const float* mean, const float* rstd, const float* g_res,
                              float* g_out, void* g_bf16, float* colsum, int B, int seq, int keep, int D, int use_xhat,
                              float dropout_p, unsigned long long seed, void* stream);
/* Forward with up to two bf16 addends and an optional stream store (added to ABI 9: no signature changed): s = fl(x_in + addend1), then
 * s = fl(s + addend2) when addend2_bf16 is given; y, mean, rstd = LN(s); x_out = s when x_out is given (NULL: no stream store).  The bits of
 * vitamd_layernorm_fwd(x_in, addend1) followed by vitamd_layernorm_fwd(its x_out, addend2), in one pass over x_in: a caller that needs the
 * intermediate sum only as the second LayerNorm's input does not store it.  addend1_bf16 is required; any D % 4 == 0. */
int vitamd_layernorm_fwd_add2(const float* x_in, const void* addend1_bf16, const void* addend2_bf16, float* x_out, void* y_bf16, float* mean,
                              float* rstd, int M, int D, float eps, void* stream);
/* Its kept-row form: output row b*keep + t = LN(fl(fl(x_in[b*seq + t] + addend1[b*seq + t]) + addend2[b*keep + t])).  x_in and addend1 are
 * full size [B*seq, D]; addend2 (required), x_out (optional), y, mean and rstd are compact [B*keep, ...]. */
int vitamd_layernorm_fwd_keep_add2(const float* x_in, const void* addend1_bf16, const void* addend2_bf16, float* x_out, void* y_bf16,
                                   float* mean, float* rstd, int B, int seq, int keep, int D, float eps, void* stream);

/* Affine LayerNorm (nn.LayerNorm weight/bias) for the `blocks.py` surface (blocks.py:43,48,179,184).
 * forward: y = bf16(LN(x) * gamma + beta).  backward: g_out = (g_res or 0) + dLN/dx; dgamma, dbeta are
 * ACCUMULATED into (zero them first); optional bf16 copy of g_out and its column sums as above. */
int vitamd_layernorm_affine_fwd(const float* x, const float* gamma, const float* beta, void* y_bf16, float* mean,
                                float* rstd, int M, int D, float eps, void* stream);
int vitamd_layernorm_affine_bwd(const void* dy_bf16, const float* x, const float* mean, const float* rstd,
                                const float* gamma, const float* g_res, float* g_out, void* g_bf16, float* colsum,
                                float* dgamma, float* dbeta, int M, int D, void* stream);
/* fp32-in / fp32-out forms for a LayerNorm that is NOT followed by a GEMM: the tokenizers' ln_pre / ln_post
 * (blocks.py:247,253 / :320,326), whose output stays in the fp32 token stream.  dgamma / dbeta accumulated into. */
int vitamd_layernorm_affine_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                                    float* rstd, int M, int D, float eps, void* stream);
int vitamd_layernorm_affine_bwd_f32(const float* dy, const float* x, const float* mean, const float* rstd,
                                    const float* gamma, float* g_out, float* dgamma, float* dbeta, int M, int D, void* stream);

/* ---- Attention on the packed fused-QKV layout ------------------------------------------------
 * qkv bf16 [B,N,3,H,64] (output-channel order (qkv, head, dh) of transformer.py:27), o bf16 [B,N,H*64],
 * lse2 fp32 [B,H,N].  head_dim must be 64, N <= 16384 (N <= 512: one LDS-resident chunk per head; longer: both sides tiled).  causal != 0 applies the strictly-upper -inf
 * mask of transformer.py:22-25.   replaces transformer.py:27-29 (rearrange + SDPA + rearrange).
 * dropout_p in [0,1): dropout on the softmax probabilities (SDPA's dropout_p); the mask is a stateless
 * hash of (seed, batch, head, query, key), so the backward call regenerates it from the same seed. */
int vitamd_attention_fwd(const void* qkv, void* o, float* lse2, int B, int N, int H, int head_dim, int causal,
                         float dropout_p, unsigned long long seed, void* stream);
/* Forward fused with the residual add that follows it in the layer (transformer.py:44 `x = x + attn(LN(x))`):
 * resid_out fp32 [B*N, H*64] = resid_in + o (o as rounded to bf16), written by the same workgroup that produces o, so the next
 * LayerNorm reads the stream once (6 instead of 12 B per element).  N <= 256 (the register-resident-softmax kernel). */
#define VITAMD_ATTN_RESID_MAX_N 256
int vitamd_attention_fwd_resid(const void* qkv, void* o, float* lse2, const float* resid_in, float* resid_out, int B, int N, int H,
                               int head_dim, int causal, float dropout_p, unsigned long long seed, void* stream);
/* dqkv bf16 [B,N,3,H,64]; delta fp32 [B,H,N] is scratch written by the call; dbias (may be NULL) fp32
 * [3*H*64]: the column sums of dqkv (= gradient of the QKV bias, transformer.py:21) are ADDED to it. */
int vitamd_attention_bwd(const void* qkv, const void* o, const float* lse2, const void* d_o, void* dqkv,
                         float* delta, float* dbias, int B, int N, int H, int head_dim, int causal, float dropout_p,
                         unsigned long long seed, void* stream);
/* Kept-query forms (non-causal, no dropout), for the last layer of a stack whose caller keeps the first nq tokens (0 < nq <= N): the
 * attention output and its gradient exist for the queries < nq only, K and V for every token.
 *   o, d_o : COMPACT bf16 [B*nq, H*64], row b*nq + t.
 *   lse2, delta : the usual fp32 [B, H, N] buffers; only the entries of queries < nq are written / read, the rest is left untouched.
 *   dqkv : dense bf16 [B,N,3,H,64]; its Q rows >= nq are written as zeros; dbias as in vitamd_attention_bwd.
 * The kept rows are bit-identical to vitamd_attention_fwd, and dqkv to vitamd_attention_bwd given d_o zero-padded to N rows (up to the
 * sign of zeros).  vitamd_attention_keep_forms(N, nq) returns a bit mask of the shapes served: 1 = forward (129 <= N <= 256, the
 * eight-wave kernel), 2 = backward (33 <= N <= 224 and nq <= 128, the pipelined kernels); the calls return VITAMD_ERR_SHAPE elsewhere and the caller
 * runs the full-size forms (vitamd/functions.py does). */
#define VITAMD_ATTN_KEEP_FWD 1
#define VITAMD_ATTN_KEEP_BWD 2
int vitamd_attention_keep_forms(int N, int nq);
int vitamd_attention_fwd_keep(const void* qkv, void* o, float* lse2, int B, int N, int H, int head_dim, int nq, void* stream);
int vitamd_attention_bwd_keep(const void* qkv, const void* o, const float* lse2, const void* d_o, void* dqkv, float* delta,
                              float* dbias, int B, int N, int H, int head_dim, int nq, void* stream);

/* Which kernels an attention call would launch (nothing is launched, no pointer is needed).  The launchers switch on the same host
 * function that answers here, so the two cannot disagree.  nq = 0: vitamd_attention_fwd / _fwd_resid (resid != 0) / _bwd (backward != 0;
 * the backward has no residual form, resid is ignored); nq > 0: vitamd_attention_fwd_keep / _bwd_keep, for which causal, dropout_p and
 * resid must be 0 (-VITAMD_ERR_ARG).
 * The answer is  family | key tiles << 4 | query tiles << 8 | flags : the kernel family and the template arguments of the
 * instantiation(s) launched, so two calls get the same code if and only if they launch the same machine code.  A field the family is
 * not templated on is 0: the tile counts of VITAMD_ATTN_FWD_LOOP, _FWD_LONG, _BWD_LOOP and _BWD_LONG, the query tiles of every forward
 * family, VITAMD_ATTN_CAUSAL where causal is read at run time (_FWD_LOOP and the long families).  VITAMD_ATTN_BWD_PIPE without
 * VITAMD_ATTN_KEEP has query tiles = key tiles.
 * A negative value is -VITAMD_ERR_* exactly where the entry point refuses: N <= 0, N > 16384, resid with N > 256 and a kept form that
 * vitamd_attention_keep_forms does not serve are -VITAMD_ERR_SHAPE, and answer before a dropout_p outside [0, 1): -VITAMD_ERR_ARG. */
#define VITAMD_ATTN_FWD_SMALL 1    /* attn_fwd_small_kernel<tiles 1..8, DROP, CAUSAL, RES>: 4 waves, register-resident score row */
#define VITAMD_ATTN_FWD_SMALL8 2   /* attn_fwd_small8_kernel<tiles 5..8, RES, KEEP>: 8 waves; non-causal, no dropout */
#define VITAMD_ATTN_FWD_LOOP 3     /* attn_fwd_kernel<DROP>: online softmax over 9..16 tiles */
#define VITAMD_ATTN_FWD_LONG 4     /* attn_fwd_long_kernel<DROP>: N > 512 */
#define VITAMD_ATTN_BWD_PIPE 5     /* attn_bwd_dq_pipe_kernel + attn_bwd_dkv_pipe_kernel<tiles 2..7, query tiles, LIM = KEEP> */
#define VITAMD_ATTN_BWD_LOOP 6     /* attn_bwd_dq_kernel + attn_bwd_dkv_kernel<DROP, CAUSAL> */
#define VITAMD_ATTN_BWD_LONG 7     /* attn_bwd_dq_long_kernel + attn_bwd_dkv_long_kernel<DROP>: N > 512 */
#define VITAMD_ATTN_FAMILY(code) ((code) & 0xf)
#define VITAMD_ATTN_TILES(code) ((code) >> 4 & 0xf)
#define VITAMD_ATTN_QTILES(code) ((code) >> 8 & 0xf)
#define VITAMD_ATTN_DROP 0x1000
#define VITAMD_ATTN_CAUSAL 0x2000
#define VITAMD_ATTN_RES 0x4000
#define VITAMD_ATTN_KEEP 0x8000    /* KEEP of the eight-wave forward, LIM of the pipelined backward */
int vitamd_attention_form(int N, int causal, float dropout_p, int resid, int nq, int backward);

/* ---- KV-cached decoding (autoregressive generation on a causal stack) ---------------------------------
 * The reference has no cache: VideoGPT.generate (train_videogpt.py:56-65) re-runs the whole stack over the whole prefix for every new
 * token.  These entry points run one token per sequence per call against a per-layer cache instead.
 * Cache layout (per layer): k_cache, v_cache bf16 [B][H][Lmax][64].  `len` is a DEVICE int32: the number of positions already held
 * (the grids are sized from Lmax, work past the length exits early, so a decode step needs no host synchronisation).
 * head_dim must be 64 and 1 <= Lmax <= 16384, else VITAMD_ERR_SHAPE.  The caller advances *len after a token's layers have run.
 *
 * Append: copies the k and v slices of T rows of a packed QKV GEMM output qkv bf16 [B*T, 3*H*64] (the layout vitamd_attention_fwd
 * reads) to cache positions *len .. *len+T-1.  T = 1 decodes, T = prompt length prefills.  T > Lmax: VITAMD_ERR_SHAPE; rows whose
 * position would reach Lmax are not written (the host binding refuses len + T > Lmax against its own copy of the length).
 * replaces the K/V half of transformer.py:27 for the cached path (the reference recomputes it for the whole prefix). */
#define VITAMD_DECODE_MAX_LEN 16384   /* of Lmax, and of N in the attention entry points above */
int vitamd_kv_append(const void* qkv, void* k_cache, void* v_cache, const int* len, int B, int T, int H, int head_dim, int Lmax,
                     void* stream);
/* Single-query attention: for each (b, h) the query row of qkv bf16 [B, 3*H*64] (one new token per sequence, already appended at
 * position *len) against cache positions 0 .. *len, scale 1/8, fp32 softmax -> o bf16 [B, H*64] (vitamd_attention_fwd's layout).
 * Long caches are split across workgroups (flash-decoding); the partials go to `ws` (vitamd_decode_attention_ws_bytes(B, H, Lmax)
 * bytes, may be NULL when that is 0) and are merged in a fixed order: results are bit-reproducible.  B*H <= 65535.
 * *len >= Lmax is clamped to the last position (the cache is never read outside [0, Lmax)); with *len < 0 no key lies below the length and
 * o is left untouched, whether the cache is split or not.
 * replaces transformer.py:28-29 (causal SDPA) for the last query row. */
long vitamd_decode_attention_ws_bytes(int B, int H, int Lmax);
int vitamd_decode_attention(const void* qkv, const void* k_cache, const void* v_cache, void* o, const int* len, int B, int H,
                            int head_dim, int Lmax, float* ws, long ws_bytes, void* stream);
/* Skinny-M GEMM: out = epi(A[M,K] . W[N,K]^T), bf16 operands, fp32 accumulation, 1 <= M <= 64 (VITAMD_ERR_SHAPE otherwise), K % 64 == 0,
 * N % 4 == 0.  The weights are streamed once, split over N and, where N alone leaves CUs idle, over K; split-K partials go to `ws`
 * (vitamd_gemm_skinny_ws_bytes(M, N, K) bytes, may be NULL when that is 0) and are summed in a fixed order (bit-reproducible).
 * epi: VITAMD_EPI_BIAS_BF16, VITAMD_EPI_GELU (out = pre-activation, out2 = erf-GELU from the vitamd_init table: the same rounding as
 * every GELU epilogue of vitamd_gemm_nt_bf16), VITAMD_EPI_RESID_F32 (aux fp32 [M,N]) or VITAMD_EPI_F32 (out f32 = acc + bias), with
 * the semantics of vitamd_gemm_nt_bf16; bias (fp32 [N], rounded to bf16 as autocast does) may be NULL.  Rows are dense (ld = K / N).
 * replaces transformer.py:21,27,37-39,44 and train_videogpt.py:43,53 (the Linears) at one row per sequence. */
#define VITAMD_SKINNY_MAX_M 64
long vitamd_gemm_skinny_ws_bytes(int M, int N, int K);
int vitamd_gemm_skinny_bf16(const void* A, const void* W, void* out, void* out2, const float* bias, const float* aux, int M, int N,
                            int K, int epi, float* ws, long ws_bytes, void* stream);

/* The QKV Linear of a decode step with the K/V append in its epilogue: qkv bf16 [M, 3*H*64] = bf16(A[M,K] . W[3*H*64,K]^T + bias), bit-equal
 * to vitamd_gemm_skinny_bf16(..., VITAMD_EPI_BIAS_BF16) (same plan, K split and summation order; ws of vitamd_gemm_skinny_ws_bytes(M, 3*H*64, K)),
 * and the store step of the K and V column ranges also writes the same packed values to row *len of k_cache / v_cache bf16 [M][H][Lmax][64]
 * (row m of the GEMM is sequence m): the caches end up bit-equal to vitamd_kv_append(T = 1) on that output, one launch fewer per layer.
 * Nothing is written to the caches when *len is outside [0, Lmax).  head_dim must be 64, 1 <= M <= 64, 1 <= Lmax <= 16384, K % 64 == 0. */
int vitamd_gemm_skinny_qkv_append(const void* A, const void* W, void* qkv, const float* bias, void* k_cache, void* v_cache, const int* len,
                                  int M, int H, int K, int head_dim, int Lmax, float* ws, long ws_bytes, void* stream);
/* Embedding of one decoded token per sequence at the device-resident position: x fp32 [B, D] with x[b, :] = tok_table[token[b], :] +
 * pos_table[*len, :] (one fp32 add: bit-equal to the framework's gather-and-add).  Tables fp32 [tok_rows, D] / [pos_rows, D], token int64 [B]
 * on the device, len the DEVICE int32 the cache kernels read, D % 4 == 0.  A token outside [0, tok_rows) or a *len outside [0, pos_rows)
 * leaves that row of x untouched; no table is ever read out of bounds.  With it a decode step holds no host value and can be captured
 * into a graph.  replaces train_videogpt.py:59 (tok_embed + pos_embed) for the one new position of a cached step. */
int vitamd_decode_embed(const float* tok_table, const float* pos_table, const long long* token, const int* len, float* x, int B, int D,
                        int tok_rows, int pos_rows, void* stream);

/* Sampled generation: one token per row of fp32 logits [B, V] (row stride ld >= V elements, 2 <= V <= 65536, else VITAMD_ERR_SHAPE), in one
 * launch, one workgroup per row, in the order of the usual logits processors:
 *   1. z = x / temperature (temperature > 0);
 *   2. top-k: K = { i : z_i >= the k-th largest z } when 0 < top_k < V, else every i; ties with the k-th value are all kept;
 *   3. top-p (0 < top_p <= 1): q = softmax of z over K, t = the largest value v with sum_{i in K, z_i >= v} q_i >= top_p,
 *      S = { i in K : z_i >= t } (ties with t all kept, never empty); top_p = 1: S = K;
 *   4. draw: the first i of S, in ascending index order, whose running sum of q over S exceeds u * sum_S q.
 * -inf logits are legal (never kept, zero mass); a row holds at least one finite logit; NaN / +inf are the caller's error.
 * u fp32 [B] in [0, 1), or NULL: then u = (first word of Philox4x32-10 >> 8) * 2^-24 with key = seed (low word, high word) and counter =
 * (row, 0, *step low, *step high); step is a DEVICE uint64 read by the kernel (NULL = 0) that the caller advances between calls, so a draw
 * never needs the host and a captured decode step replays with fresh numbers.
 * token int64 [B]; info (may be NULL) fp32 [B, 4] = (the smallest kept logit, |S|, sum_S / sum_all of the temperature softmax, q(token)
 * renormalised over S).  Logits are compared as they are (never after the division) and the softmax weights are summed as 2^-40
 * fixed-point integers: no result depends on an order of summation, every call gives the same bits.
 * temperature, top_k or top_p out of range, or a missing pointer: VITAMD_ERR_ARG (after the shape check).
 * replaces the `torch.argmax` of train_videogpt.py:63 where a sampled continuation is wanted (the reference has no sampler). */
#define VITAMD_SAMPLE_MAX_V 65536
int vitamd_sample_logits(const float* logits, long long* token, float* info, const float* u, const unsigned long long* step, int B, int V,
                         int ld, float temperature, int top_k, float top_p, unsigned long long seed, void* stream);

/* ---- Training the causal stack: cross-entropy over the vocabulary and the token + position embedding ----
 * Mean cross-entropy over the rows whose target != ignore_index: F.cross_entropy(logits.float(), target) with mean reduction, all
 * arithmetic in fp32 on the logits as stored.  logits fp32 or bf16 (logits_bf16 != 0) [M, V], row stride ld >= V elements; target
 * int64 [M].  Writes loss_row fp32 [M] (0 for ignored rows), lse fp32 [M] (natural log, every row), stats fp32 [2] = {mean loss, 1 / count}.
 * -inf logits are legal (zero probability, zero gradient); a row holds at least one finite logit.  Every row ignored: stats[0] is NaN.
 * A target outside [0, V) that is not ignore_index is the caller's error: nothing is read for it, its loss_row is NaN (so the mean is
 * NaN and the error shows without a host synchronise) and its gradient row is zeros.  Two launches: the rows (16-byte loads where the
 * base is 16-byte aligned and ld % 8 == 0 (bf16) / ld % 4 == 0 (fp32), element loads otherwise), then one workgroup that sums loss_row
 * in a fixed order and counts with an integer: no float atomics, every result is bit-reproducible.
 * M >= 1, 2 <= V <= 65536, ld >= V, else VITAMD_ERR_SHAPE; a missing pointer VITAMD_ERR_ARG (after the shape check).
 * replaces train_videogpt.py:52-53 and train_vit.py:101-103 (F.cross_entropy under autocast). */
#define VITAMD_CE_MAX_V 65536
int vitamd_cross_entropy_fwd(const void* logits, int logits_bf16, const long long* target, float* loss_row, float* lse, float* stats,
                             int M, int V, int ld, long long ignore_index, void* stream);
/* The rows one sweep of the (capped) cross-entropy grid covers at this V; an M above it makes workgroups loop over further rows.  For
 * tests that have to cross the cap.  V outside 2 .. 65536: -VITAMD_ERR_SHAPE. */
int vitamd_cross_entropy_grid_rows(int V);
/* dlogits[m, v] = (exp(x[m,v] - lse[m]) - [v == target[m]]) * (*grad_out) * stats[1]; ignored rows (and rows with a target outside
 * [0, V)) are written as zeros, never multiplied.  grad_out: DEVICE fp32 scalar (NULL = 1).  dlogits fp32 or bf16 (round to nearest even
 * of the fp32 value), row stride ldo >= V; columns V .. ldo-1 are not touched.  dlogits == logits (same type and stride, else
 * VITAMD_ERR_ARG) is allowed: every element is read once and written once by the same lane.
 * replaces the autograd backward of the same lines. */
int vitamd_cross_entropy_bwd(const void* logits, int logits_bf16, const long long* target, const float* lse, const float* stats,
                             const float* grad_out, void* dlogits, int dlogits_bf16, int M, int V, int ld, int ldo,
                             long long ignore_index, void* stream);
/* Soft-target cross-entropy: the loss of Mixup / CutMix and label smoothing, timm's SoftTargetCrossEntropy on
 * the target t[m, v] = (1-e) (l [v == ya] + (1-l) [v == yb]) + e / V, with ya = target_a[m], yb = target_b[m], l = lam[m] and
 * e = smoothing, without the [M, V] target ever existing:
 *   loss_row[m] = lse[m] - ( (1-e) (l x[m, ya] + (1-l) x[m, yb]) + (e / V) sum_v x[m, v] )
 *   stats = {sum_m loss_row[m] / M, 1 / M}: the mean is over ALL M rows, there is no ignore_index.
 * lam fp32 [M] on the device, NULL: l = 1 and target_b is not looked at (it may be NULL); with lam, target_b is required
 * (VITAMD_ERR_ARG).  ya == yb adds the two weights.  A target term whose weight l or 1-l is zero is not formed (its logit may be -inf).
 * e == 0 forms no sum_v term, so -inf logits stay legal as in vitamd_cross_entropy_fwd; with e > 0 every logit must be finite (the
 * caller's contract: inf or NaN comes out, never a fault).  sum_v x is carried by the single pass over the row that keeps the running
 * maximum and sum, lanes and waves are merged in the same fixed order, the mean is taken by the same single-workgroup launch: no
 * float atomics, the same bits on every call.  A target outside [0, V) (ya always, yb when lam is given): nothing is read for it, its
 * loss_row is NaN (so is the mean), its gradient row is zeros.  With smoothing == 0 and lam == NULL every output has the bits
 * vitamd_cross_entropy_fwd gives when no row is ignored (the same row walk).  logits, ld, the 16-byte rule and the shape refusals as
 * vitamd_cross_entropy_fwd; smoothing outside [0, 1] (or NaN) or a missing pointer: VITAMD_ERR_ARG (after the shape check).
 * replaces timm's Mixup target + SoftTargetCrossEntropy / LabelSmoothingCrossEntropy of the DeiT recipe (the reference trains without). */
int vitamd_soft_cross_entropy_fwd(const void* logits, int logits_bf16, const long long* target_a, const long long* target_b,
                                  const float* lam, float smoothing, float* loss_row, float* lse, float* stats, int M, int V, int ld,
                                  void* stream);
/* dlogits[m, v] = (exp(x[m,v] - lse[m]) - t[m, v]) * (*grad_out) * stats[1] with t as above; a row with a target outside [0, V) is
 * written as zeros.  grad_out, dlogits, ldo, the in-place rule and the refusals as vitamd_cross_entropy_bwd; target_b, lam and
 * smoothing as the forward's.  With smoothing == 0 and lam == NULL: the bits of vitamd_cross_entropy_bwd. */
int vitamd_soft_cross_entropy_bwd(const void* logits, int logits_bf16, const long long* target_a, const long long* target_b,
                                  const float* lam, float smoothing, const float* lse, const float* stats, const float* grad_out,
                                  void* dlogits, int dlogits_bf16, int M, int V, int ld, int ldo, void* stream);
/* Evaluation: per-row loss and rank of the target, added to counters that stay on the device.  logits, ld, the
 * 16-byte rule and target as vitamd_cross_entropy_fwd (M and ld are long here and must fit an int).  Launch one is the RANK form of that
 * entry's row walk, one pass over each row:
 *   loss_row[m] = lse[m] - x[m, t]: the bits vitamd_cross_entropy_fwd writes for the same input;
 *   rank[m] int32 = the number of columns v != t that rank above the target, where v ranks above t unless x[m, v] < x[m, t], or
 *                   x[m, v] == x[m, t] and v > t.  Compared as fp32 (exact for bf16); an integer count merged by integer adds.
 * rank == 0 is logits.argmax(-1) == t (the first maximal index) and rank < k is top-k membership.  A NaN compares false: a NaN in
 * another column ranks above the target, a NaN at the target ranks below every column (rank V - 1), so a NaN never makes a row top-1.
 * A row with t == ignore_index is not read: rank -1, loss_row 0.  A target outside [0, V) that is not ignore_index forms no address:
 * it is a counted row of rank V (wrong for every k) and NaN loss, so the error shows in the result without a synchronise.
 * Launch two (one workgroup, a fixed order) ADDS to the caller's accumulators, with ordinary loads and stores (no atomics):
 *   loss_sum[0] (fp64) += the fp64 sum of loss_row over the counted rows (rank >= 0);
 *   counts[0..2] (int64) += the counted rows, the rows with rank == 0, the rows with rank < topk.
 * Zero both for a fresh evaluation; the same inputs from the same state give the same bits.  Only enqueues on `stream`.
 * M < 1, V outside 2 .. 65536, ld < V (or M, ld >= 2^31): VITAMD_ERR_SHAPE; a missing pointer or topk outside 1 .. V: VITAMD_ERR_ARG
 * (after the shape check); nothing is launched in either case.
 * replaces train_vit.py:114-128 (the validation loop's F.cross_entropy, argmax == labels and their .item()s). */
int vitamd_classify_metrics(const void* logits, int logits_bf16, const long long* target, float* loss_row, int* rank, double* loss_sum,
                            long long* counts, long M, int V, long ld, int topk, long long ignore_index, void* stream);
/* x fp32 [B*S, D]: x[b*S+s, :] = tok_table[ids[b*S+s], :] + pos_table[s, :] (one fp32 add: bit-equal to the framework's gather-and-add).
 * D % 4 == 0, 1 <= S <= pos_rows, else VITAMD_ERR_SHAPE.  An id outside [0, tok_rows) leaves that row of x untouched; no table is read
 * out of bounds.  replaces train_videogpt.py:49 (tok_embed(x) + pos_embed(arange)). */
int vitamd_embed_tokens_fwd(const float* tok_table, const float* pos_table, const long long* ids, float* x, int B, int S, int D,
                            int tok_rows, int pos_rows, void* stream);
/* Its backward.  g fp32 [B*S, D] is read ONCE.  dpos fp32 [S, D] += sum over b in ascending order, by the one workgroup that owns
 * (position s, column block): no atomics, reproducible.  dtok fp32 [tok_rows, D] += the g rows by fp32 atomics (order-dependent in the
 * last bits, as vitamd_embed_bwd's outputs are), each wave-instruction adding 64 contiguous floats of one row.  Both are ACCUMULATED
 * into: zero them for a fresh gradient.  Ids out of range add nothing to dtok.  D % 4 == 0. */
int vitamd_embed_tokens_bwd(const float* g, const long long* ids, float* dtok, float* dpos, int B, int S, int D, int tok_rows, void* stream);
/* Sequence assembly of the code-id TiTok: x fp32 [B, E+S, D], x[b, e, :] = prefix[e, :] for e < E and
 * x[b, E+t, :] = src(b, t) + pos[t, :], one fp32 add per element (bit-equal to the framework's embedding / add / expand / cat).
 * Gather mode (tok_table and ids given, body NULL): src(b, t) = tok_table[ids[b*S+t], :], ids int64 [B, S]; an id outside [0, tok_rows)
 * leaves that row of x untouched and no table is read out of bounds (as vitamd_embed_tokens_fwd).  Dense mode (body given, tok_table and
 * ids NULL): src(b, t) = body[b*S+t, :], body fp32 [B*S, D].  prefix fp32 [E, D] (NULL allowed when E == 0), pos fp32 [pos_rows, D].
 * B >= 1, E >= 0, S >= 1, D % 4 == 0, pos_rows >= S, tok_rows >= 1 in gather mode, else VITAMD_ERR_SHAPE; a missing pointer, both
 * sources or neither: VITAMD_ERR_ARG (after the shape check, before any launch).  16-byte accesses; the grid is capped at
 * vitamd_assemble_tokens_grid_cap() workgroups with a stride loop beyond.  Only enqueues on `stream`.
 * replaces train_llamagen_titok.py:43-46 (tok_emb(x) + pos_emb, extra_emb in front) and :80-82 (quant_proj(z) + pos_emb, mask_tokens in front). */
int vitamd_assemble_tokens_fwd(const float* prefix, const float* pos, const float* tok_table, const long long* ids, const float* body,
                               float* x, int B, int E, int S, int D, int tok_rows, int pos_rows, void* stream);
/* Its backward.  g fp32 [B, E+S, D] is read ONCE.  dprefix fp32 [E, D] += sum over b of g[b, e]; dpos fp32 [pos_rows, D]: rows t < S +=
 * sum over b of g[b, E+t]; both sums are taken in ascending b by the one wave that owns (position, 256 columns): no atomics, reproducible
 * bits.  Gather mode (ids and dtok given): dtok fp32 [tok_rows, D] += g[b, E+t] at row ids[b*S+t] by fp32 atomics (order-dependent in
 * the last bits), each wave-instruction adding 64 contiguous floats; ids out of range add nothing.  Dense mode (ids and dtok NULL): the
 * body's gradient is the view g[:, E:], nothing is written for it.  All three outputs are ACCUMULATED into.  Shapes, errors, grid cap
 * and stream rule as the forward's (dprefix may be NULL when E == 0; one of ids / dtok without the other: VITAMD_ERR_ARG). */
int vitamd_assemble_tokens_bwd(const float* g, const long long* ids, float* dprefix, float* dpos, float* dtok, int B, int E, int S, int D,
                               int tok_rows, int pos_rows, void* stream);
/* Workgroups per launch of the two assembly kernels (the cap of their grids), for tests that have to cross it: the forward needs
 * B * (E+S) * D / 4 / 256 workgroups, the backward (E+S) * ceil(D / 256) / 4. */
int vitamd_assemble_tokens_grid_cap(void);

/* ---- device input pipeline: uint8 frames -> patch rows and images ------
 * src uint8 [Nsrc, Hs, Ws, C], channels last and contiguous (byte alignment is enough).  For output sample b < B:
 *   image[b, c, y, x] = table[c][ src[index[b], y0 + y, x0 + (flip ? W-1-x : x), c] ]          fp32 [B, C, H, W]
 *   patches_bf16[(b*gh + ph)*gw + pw, (c*p + kh)*p + kw] = bf16 (round to nearest even) of image[b, c, ph*p + kh, pw*p + kw]
 * the latter bit for bit the rows vitamd_im2col_bf16 makes of `image`.  index int64 [B] on the device names each sample's source
 * frame (NULL: sample b reads frame b, which needs Nsrc >= B): the frame gather of ImagesFromVideoDataset (datasets.py) and the window
 * videos[:, offset:offset+T] in one.  geom int32 [B, 3] on the device holds (y0, x0, flip) per sample (NULL: (0, 0, 0)): RandomCrop /
 * CenterCrop and RandomHorizontalFlip.  table fp32 [C, 256] on the device: ToTensor + Normalize per byte value.  Either output may be
 * NULL, not both; image must be 16-byte and patches_bf16 8-byte aligned for the fast form (C == 3, W % 4 == 0, p % 4 == 0), anything
 * else takes the generic one.
 * CLAMPS: the kernel clamps index[b] into [0, Nsrc), y0 into [0, Hs-H] and x0 into [0, Ws-W] before they form an address, and any
 * non-zero flip counts as 1: no device-side value can make it read outside src.
 * VITAMD_ERR_SHAPE (answered first): B, Nsrc, Hs, Ws, H, W < 1; C outside 1..4; H > Hs or W > Ws; NULL index with Nsrc < B; with
 * patches_bf16 given p < 1, H % p != 0 or W % p != 0; Nsrc*Hs*Ws*C or B*C*H*W beyond 2^40 elements.  VITAMD_ERR_ARG: NULL src, NULL
 * table, both outputs NULL.  Nothing is launched in either case.  The grid is capped at vitamd_frames_prep_grid_cap() workgroups of
 * 256 lanes with a stride loop beyond (a lane owns 4 pixels x 3 channels in the fast form, one element in the generic one).
 * Only enqueues on `stream`; no backward (a uint8 input takes no gradient).
 * replaces the CPU-side transforms of the reference's loaders (datasets.py: ToTensor, Normalize, crop, flip; with a Resize in
 * front: vitamd_frames_prep_resize) and vitamd_im2col_bf16's read of the fp32 image. */
int vitamd_frames_prep(const unsigned char* src, const long long* index, const int* geom, const float* table, void* patches_bf16,
                       float* image, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p, void* stream);
int vitamd_frames_prep_grid_cap(void);
/* vitamd_frames_prep with Mixup / CutMix applied on the way: every argument of vitamd_frames_prep, then
 * rec int32 [B, 6] = (partner, mode, yl, yh, xl, xh) per output sample and lam fp32 [B], both on the device.  With
 *   img_j[c, y, x] = table[c][ src[index[j], y0_j + y, x0_j + (flip_j ? W-1-x : x), c] ]
 * (each sample cut with ITS OWN index and geom rows), output sample b with q = partner[b] is
 *   mode 0, or q == b:  img_b                                              (the bits of vitamd_frames_prep)
 *   mode 1 (Mixup):     fl(fl(img_b * l) + fl(img_q * m)),  l = lam[b], m = fl(1 - l)     three separately rounded fp32 operations,
 *                       never a fused multiply-add: bit-equal to torch's CPU a.mul(l).add(p.mul(1 - l))
 *   mode 2 (CutMix):    img_q where yl <= y < yh and xl <= x < xh, else img_b; lam is not read (the box decides per pixel, also
 *                       inside the 4 pixels a lane of the fast form owns)
 * image holds that fp32 value, patches_bf16 its round-to-nearest-even in vitamd_im2col_bf16's layout: the bits that kernel makes of
 * the mixed image.  Either output may be NULL, not both.  The forms, lane ownership, LDS table, grid cap and source fetch are those of
 * vitamd_frames_prep (one fetch for b and, where a pixel of the lane needs it, one for q).
 * CLAMPS, before any address forms: those of vitamd_frames_prep for both samples; partner into [0, B); yl, yh into [0, H] and
 * xl, xh into [0, W]; a mode outside {1, 2} counts as 0.
 * lam may be NULL only if the caller promises that no row has mode 1: a NULL lam is taken as l = 1.
 * Refusals as vitamd_frames_prep; NULL rec: VITAMD_ERR_ARG.  No backward.
 * replaces timm's Mixup (mixup_alpha / cutmix_alpha, partner = the batch reversed) on the fp32 batch and the im2col behind it. */
int vitamd_frames_prep_mix(const unsigned char* src, const long long* index, const int* geom, const float* table, void* patches_bf16,
                           float* image, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p, const int* rec, const float* lam,
                           void* stream);
/* vitamd_frames_prep with an antialiased bilinear resize in front of the crop.  src, index, the two outputs and
 * their layouts as vitamd_frames_prep.  box int32 [B, 10] on the device holds per output sample
 *   (y0, h, Hv, oy,  x0, w, Wv, ox,  flip, 0)
 * The rectangle [y0, y0+h) x [x0, x0+w) of frame index[b] is resized (bilinear, antialiased, align_corners = false) to a virtual
 * image Hv x Wv; the output H x W is the window of that image at (oy, ox), mirrored under a flip (out[x] = window[W-1-x]).
 * RandomResizedCrop: the box is the drawn crop, Hv = H, Wv = W, oy = ox = 0.  Resize(S) + crop: the box is the frame (its valid
 * extent inside a padded canvas), (Hv, Wv) the resized size, (oy, ox) the crop offset.
 * WEIGHTS, in integers, per axis (y shown): S = max(h, Hv); for output row o, u = 2 (o + oy) + 1; for box-relative tap j in [0, h)
 *   n_j = max(0, 2S - |(2j+1) Hv - u h|),   wy_j = n_j / sum_j n_j
 * the triangle filter of support max(h / Hv, 1) about (o + oy + 0.5) h / Hv, clipped to the box and renormalised: the weights of
 * F.interpolate(mode="bilinear", antialias=True, align_corners=False) on the cropped box.  n_j and their sum are exact in fp32.
 * VALUES: r = sum_j wy_j sum_i wx_i src[index[b], y0+j, x0+i, c] in fp32 (0..255), then
 *   image = fl(fl(fl(r / 255) - mean[c]) / std[c])       three separately rounded fp32 operations with true division
 * mean, std fp32 [C] on the device, both or neither (NULL: image = fl(r / 255)).  patches_bf16 is the round-to-nearest-even of image
 * in vitamd_im2col_bf16's layout.  A record with h = Hv = H and w = Wv = W has one tap of weight 1 per value: the bits of
 * vitamd_frames_prep with geom (y0 + oy, x0 + ox, flip) and the table of those mean and std.
 * Down-scaling is limited to 8x per axis (at most 16 taps); up-scaling is not limited.  Either output may be NULL, not both; the fast
 * form (separable through LDS, a 32 x 32 output tile per workgroup) needs C == 3, W % 4 == 0, p % 4 == 0 and the alignments of
 * vitamd_frames_prep, anything else takes one lane per output element.  No atomics: the same bits on every call.
 * CLAMPS, before any address forms: index into [0, Nsrc); y0 into [0, Hs-1] and h into [1, Hs-y0]; Hv into [max(H, ceil(h / 8)), 8192];
 * oy into [0, Hv-H]; x0, w, Wv, ox alike; any non-zero flip counts as 1.  No device-side value can make the kernel read outside src
 * or run more than 16 taps per axis.
 * VITAMD_ERR_SHAPE (answered first): B, Nsrc, Hs, Ws, H, W < 1; C outside 1..4; Hs, Ws, H or W > 8192; NULL index with Nsrc < B; with
 * patches_bf16 given p < 1, H % p != 0 or W % p != 0; Nsrc*Hs*Ws*C or B*C*H*W beyond 2^40 elements.  VITAMD_ERR_ARG: NULL src, NULL
 * box, one of mean / std without the other, both outputs NULL.  Nothing is launched in either case.  H > Hs and W > Ws are legal.
 * The grid is capped at vitamd_frames_prep_resize_grid_cap() workgroups with a stride loop beyond (over tiles, or over elements).
 * Only enqueues on `stream`; no backward.
 * replaces the Resize / RandomResizedCrop of the reference's loaders (datasets.py: Resize(image_size) in front of RandomCrop; timm's
 * RandomResizedCrop in the DeiT recipe) on the CPU workers, and the host-side scaling of raw video frames to the tokenizer's size. */
#define VITAMD_FRAMES_MAX_SIZE 8192   /* of Hs, Ws, H, W and the virtual sizes Hv, Wv */
int vitamd_frames_prep_resize(const unsigned char* src, const long long* index, const int* box, const float* mean, const float* std,
                              void* patches_bf16, float* image, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p, void* stream);
int vitamd_frames_prep_resize_grid_cap(void);
/* vitamd_frames_prep_resize with Mixup / CutMix applied on the way: every argument of vitamd_frames_prep_resize,
 * then rec int32 [B, 6] = (partner, mode, yl, yh, xl, xh) per output sample and lam fp32 [B] as vitamd_frames_prep_mix takes them.
 * With R_j the fp32 image vitamd_frames_prep_resize gives for sample j - cut with ITS OWN index[j] and box[j] (crop, scale, flip) and
 * already normalised - output sample b with q = partner[b] is
 *   mode 0, q == b, or a mode outside {1, 2}:  R_b                          (the bits of vitamd_frames_prep_resize)
 *   mode 1 (Mixup):     fl(fl(R_b * l) + fl(R_q * m)),  l = lam[b], m = fl(1 - l)       three separately rounded fp32 operations,
 *                       never a fused multiply-add: bit-equal to torch's CPU a.mul(l).add(p.mul(1 - l)) of the two stand-alone images
 *   mode 2 (CutMix):    R_q where yl <= y < yh and xl <= x < xh, else R_b; lam is not read
 * image holds that fp32 value, patches_bf16 its round-to-nearest-even in vitamd_im2col_bf16's layout.  Either output may be NULL, not both.
 * Fast form (the conditions of vitamd_frames_prep_resize's): the workgroup of a 32 x 32 tile of sample b runs the separable pass for b
 * and, where the tile takes pixels of q (every tile under mode 1; the tiles that meet the box under mode 2), a second pass with q's
 * record on the same LDS; a mode-2 tile wholly inside the box runs q's pass alone.  Each pass adds in the order of the plain kernel, so
 * R_b and R_q carry the bits of a stand-alone launch.  Generic form: one lane per element, the partner's taps only where the pixel
 * takes them.  No atomics: the same bits on every call.
 * CLAMPS, before any address forms: those of vitamd_frames_prep_resize on both samples' records; partner into [0, B); yl, yh into
 * [0, H] and xl, xh into [0, W].  lam may be NULL only if the caller promises that no row has mode 1: a NULL lam is taken as l = 1.
 * Refusals as vitamd_frames_prep_resize; NULL rec: VITAMD_ERR_ARG.  Nothing is launched on a refusal.  Grid cap:
 * vitamd_frames_prep_resize_grid_cap().  Only enqueues on `stream`; no backward.
 * replaces timm's RandomResizedCrop on the CPU workers followed by its Mixup on the fp32 batch and the im2col behind it (the DeiT recipe). */
int vitamd_frames_prep_resize_mix(const unsigned char* src, const long long* index, const int* box, const float* mean, const float* std,
                                  void* patches_bf16, float* image, int B, int Nsrc, int Hs, int Ws, int C, int H, int W, int p,
                                  const int* rec, const float* lam, void* stream);
/* Fills geom int32 [B, 3] on the device for vitamd_frames_prep.  Sample b takes the words w0, w1, w2 of Philox4x32-10 with key
 * (seed low, seed high) and counter (b, 1, step low, step high) - c1 = 1 keeps it off vitamd_sample_logits' stream, which uses c1 = 0:
 *   y0 = (w0 * (Hs-H+1)) >> 32     x0 = (w1 * (Ws-W+1)) >> 32     flip = flip_enabled ? w2 >> 31 : 0       (64-bit products)
 * seed and step are passed by value: no host synchronisation, and the same (seed, step) gives the same crops on any device.
 * B, Hs, Ws, H, W < 1, H > Hs or W > Ws: VITAMD_ERR_SHAPE; NULL geom: VITAMD_ERR_ARG. */
int vitamd_crop_flip_draw(int* geom, int B, int Hs, int Ws, int H, int W, int flip_enabled, unsigned long long seed,
                          unsigned long long step, void* stream);
/* The way back, for frames that leave the tokenizers: img fp32 [B, C, H, W] -> out uint8 [B, H, W, C] = rint(clamp(v, 0, 1) * 255)
 * (ties to even), NaN -> 0: bit-equal to (x.clamp(0, 1) * 255).round().to(uint8) for finite input.  C in 1..4, all sizes >= 1,
 * at most 2^40 elements, else VITAMD_ERR_SHAPE; a NULL pointer: VITAMD_ERR_ARG.  Grid cap as vitamd_frames_prep. */
int vitamd_frames_to_u8(const float* img, unsigned char* out, int B, int C, int H, int W, void* stream);
/* Random Erasing on the finished batch: rewrites boxes of the two outputs of a vitamd_frames_prep* launch IN
 * PLACE - image fp32 [B, C, H, W] and patches_bf16 [B*gh*gw, C*p*p], either of which may be NULL, not both - and touches nothing else.
 * rec int32 [B, K, 5] on the device holds (mode, yl, yh, xl, xh) for box k of sample b, 1 <= K <= 8; fill fp32 [B, K, 4] on the
 * device (NULL: zeros).  For yl <= y < yh and xl <= x < xh and every channel c:
 *   mode 1:  image[b, c, y, x] = fill[b, k, c]
 *   mode 2:  image[b, c, y, x] = z(seed, step, b, c, y, x), an N(0, 1) value (below)
 * mode 0, any other mode and an empty box write nothing.  patches_bf16 gets the round-to-nearest-even of exactly the fp32 value image
 * gets, in vitamd_im2col_bf16's layout: erasing both outputs keeps patches_bf16 the bits vitamd_im2col_bf16 makes of image.
 * OVERLAP: a pixel covered by several boxes of its sample takes the value of the box with the largest k, decided per pixel, so every
 * element has at most one writer: no read-modify-write, no atomics, the same bits on every call.  A pixel outside every box is
 * neither read nor written.
 * NOISE: z depends on (seed, step, b, c, y, x) alone - not on the box, k, p, B, K or which output is present.  One Philox4x32-10 call
 * per four neighbouring pixels of a row: key (seed low, seed high), counter
 *   ((c*H + y) * ceil(W/4) + (x >> 2),  (b << 2) | 2,  step low,  step high)
 * (the low two bits of the second word keep it off vitamd_sample_logits' stream, 0, and vitamd_crop_flip_draw's, 1).  From its words
 * w0..w3, in fp32 with the full-precision math functions:
 *   u1 = ((w0 >> 8) + 1) * 2^-24   u2 = (w1 >> 8) * 2^-24   r = sqrtf(-2 logf(u1))   z0 = r cospif(2 u2)   z1 = r sinpif(2 u2)
 * z2, z3 alike from (w2, w3); pixel x takes z[x & 3].  |z| <= sqrt(48 ln 2).
 * CLAMPS, before any address forms: yl, yh into [0, H]; xl, xh into [0, W].
 * Work is proportional to the erased area: workgroups are given (sample, box, one of 32 strips of the box), and one without a box ends
 * after its record read.  Aligned groups of 4 pixels that are wholly their box's go out as one 16-byte fp32 and one 8-byte bf16 store where
 * W % 4 == 0, p % 4 == 0 (with patches_bf16), image is 16-byte and patches_bf16 8-byte aligned; box edges and everything else one
 * element at a time.  The grid is capped at vitamd_frames_erase_grid_cap() workgroups of 256 lanes with a stride loop beyond.
 * VITAMD_ERR_SHAPE (answered first): B, H, W < 1; C outside 1..4; K outside 1..8; with patches_bf16 given p < 1, H % p != 0 or
 * W % p != 0; B*C*H*W beyond 2^40 elements; B >= 2^30; C*H*ceil(W/4) beyond 2^32.  VITAMD_ERR_ARG: NULL rec, both outputs NULL.
 * Nothing is launched in either case.  Only enqueues on `stream`; no backward.
 * replaces timm's RandomErasing (--reprob, --remode const / rand / pixel) on the normalised fp32 device batch, and the im2col a
 * caller of the fused feed would have to run again behind it. */
#define VITAMD_ERASE_MAX_BOXES 8
int vitamd_frames_erase(void* patches_bf16, float* image, int B, int C, int H, int W, int p, const int* rec, const float* fill, int K,
                        unsigned long long seed, unsigned long long step, void* stream);
int vitamd_frames_erase_grid_cap(void);

/* ---- helpers around the GEMMs ---------------------------------------------------------------- */
/* fp32 -> bf16 (autocast's per-step weight / activation cast, train_vit.py:100). */
int vitamd_cast_f32_bf16(const float* in, void* out_bf16, long n, void* stream);
/* bf16(x) * dropout mask (p, seed; element index) — the top layer's fc2 output gradient under dropout. */
int vitamd_cast_f32_bf16_dropout(const float* in, void* out_bf16, long n, float dropout_p, unsigned long long seed, void* stream);
/* out[i] = in[i] * keep(seed, i / group): nn.Dropout (group = 1; reference blocks.py:118 proj_drop, :168-170 Mlp.drop) and DropPath
 * (group = elements per sample; blocks.py:124-152) in training mode.  keep = 1/(1-p) or 0 from the stateless (seed, index) hash;
 * the backward is the same call on the gradient.  In place (out == in) is allowed. */
int vitamd_dropout_bf16(const void* in, void* out, long n, long group, float dropout_p, unsigned long long seed, void* stream);
int vitamd_dropout_f32(const float* in, float* out, long n, long group, float dropout_p, unsigned long long seed, void* stream);
/* W fp32 [N,K] -> bf16 [N,K] (wb, may be NULL) and transposed bf16 [K,N] (wbt, may be NULL). */
int vitamd_cast_transpose_weight(const float* w, void* wb, void* wbt, int N, int K, void* stream);
/* The same for n weights in ONE launch.  desc_dev: device array of n vitamd_cast_desc records,
 * first_tile = running sum of ceil(N/64)*ceil(K/64), tiles_k = ceil(K/64); total_tiles = the final sum. */
typedef struct vitamd_cast_desc {
  const float* w;          /* fp32 [N,K] */
  void* wb;                /* bf16 [N,K], may be NULL */
  void* wbt;               /* bf16 [K,N], may be NULL */
  int N, K, first_tile, tiles_k;
} vitamd_cast_desc;        /* 40 bytes, 8-byte aligned */
int vitamd_cast_transpose_batched(const void* desc_dev, int n, int total_tiles, void* stream);
/* images fp32 [B,C,H,W] -> patches bf16 [B*(H/p)*(W/p), C*p*p], vector order (c,kh,kw): the
 * contraction order of Conv2d(kernel=stride=p), train_vit.py:34,39. */
int vitamd_im2col_bf16(const float* img, void* out_bf16, int B, int C, int H, int W, int p, void* stream);
/* out[n] += sum_m X[m,n]  (bias gradients). */
int vitamd_colsum_bf16(const void* x_bf16, float* out, int M, int N, int ld, void* stream);
/* Backward of the token assembly train_vit.py:41-44: g fp32 [B,seq,D] -> dpos [seq-extra,D],
 * dextra [extra,D], compact bf16 patch rows dyp [B*(seq-extra),D], dbias[D] = their column sums.
 * dpos, dextra and dbias are ACCUMULATED into (atomics): zero them for a fresh gradient.
 * dbias_rows: zeroed scratch [seq-extra, D] (per-position partials of dbias, summed by a second pass). */
int vitamd_embed_bwd(const float* g, float* dpos, float* dextra, void* dyp_bf16, float* dbias, float* dbias_rows, int B,
                     int seq, int extra, int D, void* stream);

/* ---- VQ quantiser (TiTok / ViT-VQGAN) --------------------------------------
 * idx[m] = argmin_k ||x[m,:] - codebook[k,:]||^2, first minimum, fp32; d <= 1024; idx is int64.
 * replaces train_titok.py:53 / train_vit_vqgan.py:52 `torch.cdist(x, embedding).argmin(dim=-1)` and the
 * expanded-distance argmin of blocks.py:442-446 (blocks.VectorQuantizer). */
int vitamd_vq_nearest(const float* x, const float* codebook, long long* idx, int M, int K, int d, void* stream);

/* ---- 3x3 smoothing convolution of the pixel decoders (blocks.py surface) ----
 * NCHW fp32, stride 1, zero padding 1, Cin = Cout = 3 (anything else: VITAMD_ERR_SHAPE).
 * w [Cout,Cin,3,3], bias [Cout] or null.  replaces `self.conv_out = nn.Conv2d(3, 3, 3, padding=1)`
 * (blocks.py:333, applied at :355 and :402).
 * bwd: dx (or null) = input gradient, overwritten; dw [Cout,Cin,3,3] (or null) and db [Cout] (or null) are
 * ACCUMULATED into (atomics): zero them for a fresh gradient. */
int vitamd_conv3x3_fwd(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                       void* stream);
int vitamd_conv3x3_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int B, int Cin,
                       int Cout, int H, int W, void* stream);

/* ---- optimiser -------------------------------------------------------------------------------
 * One fused AdamW update (decoupled weight decay, bias correction for 1-based `step`) of n fp32
 * parameters in place; m, v are the optimiser state.  replaces train_vit.py:82,105 (torch.optim.AdamW). */
int vitamd_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, void* stream);
/* The same with beta1 / beta2 in double, as torch.optim.AdamW holds them: the coefficients beta and 1 - beta are each rounded to fp32 once
 * (with fp32 betas, 1 - beta inherits the rounding of beta: 1.3e-5 relative on exp_avg_sq at beta2 = 0.999).  vitamd.optim.AdamW calls this one. */
int vitamd_adamw_step_d(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2,
                        float eps, float weight_decay, int step, void* stream);

/* ---- multi-tensor optimiser step with on-device gradient-norm clipping ----
 * The whole step after backward() in one to three launches over a ROW TABLE: one row per tensor that has a gradient this step.  Every
 * per-step and per-group value lives in the row, so parameter groups, and parameters whose step count lags, share one launch.
 * replaces train_titok.py / train_vit_vqgan.py / train_tatitok.py `clip_grad_norm_(model.parameters(), 1.0)` + `optim.step()`. */
typedef struct vitamd_mt_row {
  float* p;                /* parameter, updated in place (may be NULL for vitamd_mt_sumsq / vitamd_mt_scale) */
  const float* g;          /* gradient; read by all three calls, written by vitamd_mt_scale alone */
  float* m;                /* exp_avg (as p) */
  float* v;                /* exp_avg_sq (as p) */
  long long n;             /* elements, >= 1 */
  int first_chunk;         /* running sum of ceil(n / vitamd_mt_chunk_elems()) over the rows before this one */
  float lr, weight_decay;
  float beta1, one_minus_beta1, beta2, one_minus_beta2; /* each rounded to fp32 once from the double, as vitamd_adamw_step_d does */
  float eps;
  float inv_bc1;           /* fp32(1 / (1 - beta1^step)) of THIS tensor's 1-based step */
  float inv_sqrt_bc2;      /* fp32(1 / sqrt(1 - beta2^step)) */
} vitamd_mt_row;           /* 80 bytes, 8-byte aligned */
/* Queries: sizeof(vitamd_mt_row) as this library was compiled; the elements per chunk (a multiple of 4); the workgroups per launch, above
 * which workgroups stride over further chunks.  For bindings that build the table, and for tests that have to cross the cap. */
long vitamd_mt_row_bytes(void);
int vitamd_mt_chunk_elems(void);
int vitamd_mt_grid_cap(void);
/* All three calls take the table twice: rows_host, the caller's HOST copy, is read before anything is launched - n_rows >= 1, every
 * n >= 1, first_chunk the running sum above and total_chunks its final value (else VITAMD_ERR_SHAPE), every tensor pointer the call uses
 * present and 16-byte aligned (else VITAMD_ERR_ARG, nothing launched, nothing touched) - and rows_dev, the same bytes in device memory
 * (uploaded by the caller on `stream`), is what the kernels walk.  A missing buffer is VITAMD_ERR_ARG.
 *
 * Global gradient norm: partials fp32 [total_chunks] (scratch, every entry written) receives one sum of squares per chunk; a second,
 * single-workgroup launch adds them in a fixed order in fp64 and writes norm_coef fp32 [2] = {norm, coef} with
 * coef = min(1, max_norm / (norm + 1e-6)) evaluated in fp32 as torch.nn.utils.clip_grad_norm_ does; max_norm <= 0: coef = 1.
 * No float atomics: the same gradients give the same bits on every call, whatever the grid.  Uses g alone. */
int vitamd_mt_sumsq(const vitamd_mt_row* rows_host, const void* rows_dev, int n_rows, int total_chunks, float* partials, float* norm_coef,
                    float max_norm, void* stream);
/* AdamW over the table, arithmetic of vitamd_adamw_step_d element for element.  coef: DEVICE fp32 scalar (norm_coef + 1) by which the
 * gradient is multiplied before the update, read by the kernel (no host synchronisation); NULL = not multiplied.  g is not written. */
int vitamd_mt_adamw(const vitamd_mt_row* rows_host, const void* rows_dev, int n_rows, int total_chunks, const float* coef, void* stream);
/* g *= *coef in place (coef required); stores nothing when *coef == 1.  Uses g alone.  For clipping in front of another optimiser. */
int vitamd_mt_scale(const vitamd_mt_row* rows_host, const void* rows_dev, int n_rows, int total_chunks, const float* coef, void* stream);

/* ---- the step-dependent floats of the table, advanced on the device ----
 * A table that stays in device memory from step to step, so that the optimiser step can be recorded in a graph: one schedule entry per
 * row holds the counters and the doubles from which lr, inv_bc1 and inv_sqrt_bc2 of that row follow. */
typedef struct vitamd_sched_row {
  long long step;          /* optimiser steps this tensor has taken (0 before the first) */
  long long sched_t;       /* position in the learning-rate schedule (0 before the first step) */
  double base_lr;          /* the group's base learning rate */
  double beta1, beta2;     /* the doubles torch.optim.AdamW holds */
  double min_ratio;        /* min_lr / base_lr: where the cosine phase ends */
  long long warmup_steps;  /* linear warm-up over this many steps */
  long long train_steps;   /* cosine period and the milestone from which the factor is 1 again; 0 = constant base_lr */
} vitamd_sched_row;        /* 64 bytes, 8-byte aligned */
long vitamd_sched_row_bytes(void);
/* One launch, one thread per row r, any n_rows >= 1:  k = ++sched[r].step, t = sched[r].sched_t++;  in fp64
 *   rows[r].inv_bc1 = fp32(1 / (1 - beta1^k)), rows[r].inv_sqrt_bc2 = fp32(1 / sqrt(1 - beta2^k))   (as vitamd_adamw_step_d forms them)
 *   rows[r].lr = fp32(base_lr * factor(t)), factor = min(1, t / warmup_steps) for t < warmup_steps, else
 *   min_ratio + (1 - min_ratio) * (1 + cos(pi * (t - warmup_steps) / train_steps)) / 2 for t < train_steps, else 1
 * (the reference's SequentialLR, utils.lr_factor: the cosine counts from the warm-up milestone and the rate returns to base_lr at
 * train_steps).  No other byte of a row is written.  Both arrays are DEVICE memory, 8-byte aligned (else VITAMD_ERR_ARG; n_rows < 1:
 * VITAMD_ERR_SHAPE); nothing is read from or allocated on the host, so the call can be recorded in a graph in front of
 * vitamd_mt_sumsq / vitamd_mt_adamw, which then find this step's values in the table. */
int vitamd_sched_advance(void* rows_dev, void* sched_dev, int n_rows, void* stream);

/* ---- training the image tokenizers -------------------------------------
 * Every call only enqueues on `stream`; none allocates or synchronises; scalars are read from and written to device memory.
 *
 * The cosine-similarity quantiser of train_titok.py:50-59 / train_vit_vqgan.py:49-58, narrow codes (1 <= d <= 64, K >= 1; anything else
 * VITAMD_ERR_SHAPE), fp32 throughout, eps = 1e-12 as F.normalize:
 *   unit[m,:] = u = x / max(|x|, eps), rnorm[m] = 1 / max(|x|, eps) (exactly 1/eps marks a clamped row);
 *   idx[m]    = first argmin_k |u - e^_k|^2 over e^_k = e_k / max(|e_k|, eps), by the arithmetic and tie-break of vitamd_vq_nearest;
 *   q[m,:]    = u + (p - u) with p = codebook[idx[m],:], the RAW row;  *loss = 1.25 * mean over M*d of (p - u)^2.
 * ws: vitamd_vq_quantize_ws_bytes(M, K, d) bytes of scratch (negative: the shape error).  Its first K*d floats hold e^ after the call.
 * The loss is summed from per-workgroup partials in a fixed order: the same inputs give the same bits. */
#define VITAMD_VQ_MAX_D 64
long vitamd_vq_quantize_ws_bytes(int M, int K, int d);
int vitamd_vq_quantize_fwd(const float* x, const float* codebook, float* unit, float* rnorm, float* q, long long* idx, float* loss, float* ws,
                           int M, int K, int d, void* stream);
/* g_q fp32 [M,d] or NULL (the gradient of q), g_loss DEVICE fp32 or NULL (the gradient of the loss, s; NULL = 0):
 *   du = g_q + 0.5 s (u - p) / (M d);  dx = (du - u (u . du)) * rnorm, or du / eps for a clamped row (overwritten);
 *   dcodebook[idx[m],:] += 2 s (p - u) / (M d)   (ACCUMULATED into: zero it for a fresh gradient; nothing from g_q).
 * Rows of one workgroup that share a code are summed on chip in row order, then added by one fp32 atomic per element: dcodebook depends
 * on arrival order in its last bits where a code is picked in more than one 256-row block; dx never does.
 * An idx outside [0, K): that row's dx is zero and it adds nothing. */
int vitamd_vq_quantize_bwd(const float* g_q, const float* g_loss, const float* unit, const float* rnorm, const long long* idx,
                           const float* codebook, float* dx, float* dcodebook, int M, int K, int d, void* stream);

/* mse_loss(pixel_shuffle(y), img) without the image-shaped copy of y: y = tokens [B*G*G, F = p*p*c] with row stride ld (elements; columns
 * F .. ld are never read or written), bf16 (y_bf16 != 0) or fp32; img fp32 [B, c, G*p, G*p] contiguous;
 *   *loss = mean over b, ch, gh, p1, gw, p2 of (float(y[b*G*G + gh*G + gw, (p1*p + p2)*c + ch]) - img[b, ch, gh*p + p1, gw*p + p2])^2
 * (the index map of 'b (h w) (p1 p2 c) -> b c (h p1) (w p2)', train_titok.py:73-75).  Only a 16-byte path exists: y 16-byte aligned, ld and
 * F multiples of 8 (bf16) or 4 (fp32), one token within 48 KiB - anything else VITAMD_ERR_SHAPE, for the caller to take another route.
 * ws: vitamd_recon_mse_ws_bytes(...) bytes (negative: the shape error); one partial per workgroup, summed in a fixed order (reproducible). */
long vitamd_recon_mse_ws_bytes(int B, int G, int p, int c, int y_bf16);
int vitamd_recon_mse_fwd(const void* y, int y_bf16, const float* img, float* loss, float* ws, int B, int G, int p, int c, int ld, void* stream);
/* dy = 2 (float(y) - img) * (*grad_out) / (B c H W) in token layout and in y's type (bf16: one round-to-nearest-even), row stride ld_dy;
 * grad_out: DEVICE fp32 or NULL (= 1).  dy == y (with ld_dy == ld) overwrites the tokens in place. */
int vitamd_recon_mse_bwd(const void* y, int y_bf16, const float* img, const float* grad_out, void* dy, int B, int G, int p, int c, int ld,
                         int ld_dy, void* stream);

/* The quantiser of blocks.VectorQuantizer(use_l2_norm=True, commitment_cost=0.25): the two calls above with UNIT codes.
 * Same arguments, shapes, search, workspace and error rules; the differences:
 *   forward   p = e^_idx = e_idx / max(|e_idx|, eps), the NORMALISED row: q = u + (p - u), *loss = 1.25 * mean over M*d of (p - u)^2;
 *   backward  du and dx as above with that p; the per-code sum T_k = sum over the rows m with idx[m] = k of 2 s (p - u) / (M d) goes through
 *             the normalisation before it is added: dcodebook[k,:] += (T_k - e^_k (e^_k . T_k)) / |e_k|, or T_k / eps where |e_k| < eps.
 * The projection is linear, so it is applied to each workgroup's on-chip sum; the atomics and their order dependence are those of
 * vitamd_vq_quantize_bwd.  `codebook` is the RAW codebook in both calls. */
int vitamd_vq_quantize_unit_fwd(const float* x, const float* codebook, float* unit, float* rnorm, float* q, long long* idx, float* loss, float* ws,
                                int M, int K, int d, void* stream);
int vitamd_vq_quantize_unit_bwd(const float* g_q, const float* g_loss, const float* unit, const float* rnorm, const long long* idx,
                                const float* codebook, float* dx, float* dcodebook, int M, int K, int d, void* stream);

/* The pixel tail of blocks.TiTokDecoder on the tokens of its head GEMM, c = 3:
 *   yimg = pixel_shuffle(y) (the index map of vitamd_recon_mse_fwd), r = conv3x3(yimg, w[3,3,3,3], stride 1, zero padding 1) + bias[3],
 *   *loss = mean over B*3*H*W of (r - img)^2, H = W = G*p.
 * y = tokens [B*G*G, 3*p*p], bf16 (y_bf16 != 0) or fp32, read as stored, row stride ld >= 3*p*p; all arithmetic fp32; yimg is never formed.
 * recon: fp32 [B,3,H,W] that receives r, or NULL.  One workgroup per 32 x 32 pixel tile of one image, the tile index in blockIdx.x alone
 * (no grid cap); a halo never reads another image of the batch: outside the image yimg is zero.
 * Only a 16-byte path exists: p % 8 == 0 (bf16) / p % 4 == 0 (fp32), ld a multiple of 8 / 4, y 16-byte aligned - anything else
 * VITAMD_ERR_SHAPE, for the caller to take another route.  ws: vitamd_conv_recon_mse_ws_bytes(B, G, p, y_bf16, backward) bytes
 * (negative: the shape error): one loss partial per tile (forward), 84 gradient partials per tile (backward), summed in a fixed order. */
long vitamd_conv_recon_mse_ws_bytes(int B, int G, int p, int y_bf16, int backward);
int vitamd_conv_recon_mse_fwd(const void* y, int y_bf16, const float* w, const float* bias, const float* img, float* loss, float* recon, float* ws,
                              int B, int G, int p, int ld, void* stream);
/* e = (*g_loss) * 2 (r - img) / (B*3*H*W) + g_recon, r recomputed; g_loss: DEVICE fp32 or NULL (= 1); g_recon: fp32 [B,3,H,W] or NULL (= 0);
 * e is zero outside the image.
 *   dy = the input gradient of the convolution at e, in token layout and in y's type (bf16: one round-to-nearest-even), row stride ld_dy,
 *        columns 3*p*p .. ld_dy untouched.  dy == y is VITAMD_ERR_ARG: a tile reads its neighbours' tokens, so this call is never in place.
 *   dw[co,ci,kh,kw] = sum over b, y, x of e[b,co,y,x] * yimg[b,ci,y+kh-1,x+kw-1],  db[co] = sum of e[b,co,y,x]   (both OVERWRITTEN)
 * Each pixel's e is counted once (by the tile that owns it); per-thread sums, then lanes, waves and tiles in a fixed order, no float
 * atomics: the same inputs give the same bits in dy, dw and db. */
int vitamd_conv_recon_mse_bwd(const void* y, int y_bf16, const float* w, const float* bias, const float* img, const float* g_loss,
                              const float* g_recon, void* dy, float* dw, float* db, float* ws, int B, int G, int p, int ld, int ld_dy,
                              void* stream);

/* ---- the ConvNeXt-S perceptual loss of the tokenizers ---------------------
 * The frozen network of perceptual_loss.py:41 runs on channels-last activation rows [B*H*W, C]: its Linears, LayerNorms and strided
 * convolutions are vitamd_gemm_nt_bf16 / vitamd_layernorm_affine_* calls; the entry points below are the rest.  Every call only enqueues
 * on `stream`; none allocates or synchronises; no atomics: the same inputs give the same bits.  (Added to ABI 9: no signature changed.)
 *
 * Depthwise 7x7 convolution, stride 1, zero padding 3 (the first layer of a torchvision CNBlock, `nn.Conv2d(dim, dim, 7, padding=3,
 * groups=dim)`, reached from perceptual_loss.py:63-64), on rows:
 *   y[b,h,w,c] = bias[c] + sum_{kh,kw} w[c,kh,kw] * x[b,h+kh-3,w+kw-3,c]       x, y: [B,H,W,C], w fp32 [C,7,7], bias fp32 [C] or NULL.
 * x is fp32, or bf16 when x_bf16 != 0; y is fp32; accumulation is fp32 in the order kh, then input column.  C % 4 == 0, B, H, W >= 1 (maps
 * smaller than the window are fine), fewer than 2^40 elements, else VITAMD_ERR_SHAPE; a missing pointer VITAMD_ERR_ARG. */
int vitamd_dwconv7_fwd(const void* x, int x_bf16, const float* w, const float* bias, float* y, int B, int H, int W, int C, void* stream);
/* Its input gradient, the same kernel body on the reversed taps:
 *   dx[b,h,w,c] = (add ? add[b,h,w,c] : 0) + sum_{kh,kw} w[c,kh,kw] * dy[b,h+3-kh,w+3-kw,c]
 * add (fp32 rows, may be NULL, must not be dy): the gradient that reaches the block's input along the residual branch, added in the
 * store.  dx may not alias dy.  The network is frozen: there is no weight gradient.  replaces the autograd backward of that Conv2d. */
int vitamd_dwconv7_bwd(const void* dy, int dy_bf16, const float* w, const float* add, float* dx, int B, int H, int W, int C, void* stream);

/* `F.interpolate(img, size=S, mode="bilinear", align_corners=False, antialias=True)` followed by `(x - mean) / std`
 * (perceptual_loss.py:61-64) on img fp32 [B,3,Hin,Win] (C != 3: VITAMD_ERR_SHAPE), S % 4 == 0.  The resize is the separable product
 * Wh . img . Ww^T; the caller passes each matrix as a BAND TABLE built once per (n_in, n_out): for output index o, start[o] (int32) is
 * the first input index and taps[o*T .. o*T+T-1] (fp32) the weights of T consecutive inputs, zero-padded, with start[o] + T <= n_in
 * (the kernels trust this; T > n_in is VITAMD_ERR_SHAPE).  Weights: scale = n_in/n_out, support = max(scale, 1), centre = (o + 0.5) scale,
 * inputs j in [max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n_in)), weight max(0, 1 - |(j - centre + 0.5) / support|)
 * normalised to sum 1.  Sums are fp32: along W first, then along H.
 * Outputs (either may be NULL, not both): rows_bf16 [B*(S/4)^2, 64], the operand of the 4x4 stride-4 stem convolution - row
 * b*(S/4)^2 + (oh/4)*(S/4) + ow/4, column c*16 + (oh%4)*4 + ow%4, columns 48..63 written as zeros; nchw fp32 [B,3,S,S]. */
#define VITAMD_RESIZE_ROW_LD 64   /* columns of a rows_bf16 row: 3 * 4 * 4 = 48 patch values, zero-padded */
int vitamd_resize_norm_fwd(const float* img, const int* start_h, const float* taps_h, int Th, const int* start_w, const float* taps_w, int Tw,
                           const float* mean, const float* stdv, void* rows_bf16, float* nchw, int B, int C, int Hin, int Win, int S,
                           void* stream);
/* Its backward: dimg fp32 [B,3,Hin,Win] = Wh^T . g . Ww / std, overwritten, from g fp32 in the patch-row layout above with row stride
 * ldg >= 48 (the gradient of the stem GEMM's operand).  The tables are those of the TRANSPOSED matrices: index = input pixel, start =
 * first output index, start + T <= S.  replaces the autograd backward of perceptual_loss.py:61,63. */
int vitamd_resize_norm_bwd(const float* g_rows, int ldg, const int* start_h, const float* taps_h, int Th, const int* start_w,
                           const float* taps_w, int Tw, const float* stdv, float* dimg, int B, int C, int Hin, int Win, int S, void* stream);

/* ---- the Enhancing ViT-VQGAN tokenizer -------------------------------------
 * The model of train_enhancing_vitvqgan.py runs on the GEMM, attention, LayerNorm and quantiser entry points above; the entry points below
 * are the rest.  Every call only enqueues on `stream`; none allocates or synchronises; no atomics: the same inputs give the same bits.
 * (Added to ABI 9: no signature changed.)
 *
 * nn.Tanh between the two Linears of FeedForward (train_enhancing_vitvqgan.py:117-121) on n bf16 elements:
 *   out[i] = bf16(tanh(float(pre[i])))
 * computed in fp32 (within one bf16 ulp of the exact value for every bf16 input; |x| >= 20 gives exactly +-1, +-0 gives +-0, NaN stays NaN).
 * The fc1 bias is already in `pre` (VITAMD_EPI_BIAS_BF16).  out == pre runs in place; any other overlap is not allowed.  n >= 1 (else
 * VITAMD_ERR_SHAPE); the pointers need 2-byte alignment only (else VITAMD_ERR_ARG): elements in front of the first 16-byte boundary and
 * behind the last whole 16-byte piece are handled one by one, and operands that sit at different offsets within 16 bytes are handled
 * one by one throughout.  At most 2048 workgroups of 256 threads, 8 elements per thread and sweep: 4 194 304 elements per sweep of the
 * grid-stride loop. */
int vitamd_tanh_bf16(const void* pre, void* out, long n, void* stream);
/* Its backward from the SAVED OUTPUT t = tanh(pre), not from the pre-activation:
 *   dpre[i] = bf16(float(dh[i]) * (1 - float(t[i])^2))          (t^2 is exact in fp32; exactly 0 where t = +-1)
 * dpre == dh runs in place.  The fc1 bias gradient is the column sum of dpre (vitamd_gemm_tn_bf16_ws_colsum).  Arguments and errors as
 * above. */
int vitamd_tanh_bwd_bf16(const void* dh, const void* t, void* dpre, long n, void* stream);

/* mean |depatchify(y) - img| for the tokens of a Linear that stands for nn.ConvTranspose2d(dim, c, kernel_size = stride = p)
 * (train_enhancing_vitvqgan.py:221-224): the arguments of vitamd_recon_mse_fwd with the feature order (c p1 p2) of that layer's weight
 * [dim, c, p, p],
 *   *loss = mean over b, ch, gh, p1, gw, p2 of |float(y[b*G*G + gh*G + gw, ch*p*p + p1*p + p2]) - img[b, ch, gh*p + p1, gw*p + p2]|
 * recon: fp32 [B, c, G*p, G*p] that receives float(y) in image layout, or NULL.  ws: ws_bytes >= vitamd_recon_mse_ws_bytes(B, G, p, c, y_bf16)
 * bytes (the same plan: one partial per workgroup, summed in a fixed order; a smaller one is VITAMD_ERR_ARG).  Shape and alignment
 * rules, and their errors, are those of vitamd_recon_mse_fwd (a token row that is not whole 16-byte pieces, e.g. p = 2 in bf16, is
 * VITAMD_ERR_SHAPE, for the caller to take another route). */
int vitamd_recon_l1_fwd(const void* y, int y_bf16, const float* img, float* loss, float* recon, float* ws, long ws_bytes, int B, int G, int p,
                        int c, int ld, void* stream);
/* dy = (*g_loss) * sign(float(y) - img) / (B c H W) + g_recon in token layout and in y's type (the sum is formed in fp64 and rounded once
 * to fp32, then once to bf16), row stride ld_dy.  sign(0) = 0: at a tie dy is g_recon itself.  g_loss: DEVICE fp32 or NULL (= 1);
 * g_recon: fp32 [B, c, G*p, G*p], the gradient that arrived on `recon`, or NULL (= 0).  dy == y (with ld_dy == ld) overwrites the tokens
 * in place. */
int vitamd_recon_l1_bwd(const void* y, int y_bf16, const float* img, const float* g_loss, const float* g_recon, void* dy, int B, int G, int p,
                        int c, int ld, int ld_dy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VITAMD_H */
