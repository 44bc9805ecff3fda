/* C-ABI of libvlmo_hip.so: the MI355X (gfx950) engine under the VLMo
 * pretraining forward/backward path of fanzhongyi/ExploreMultiModal.
 *
 * The reference has no native/FFI boundary for this path (it is a Python
 * nn.Module contract: models/build.py:4-12, models/vlmo/vlmo_module.py:395-436,
 * models/vlmo/vlmo.py:357-414); these entry points are what a binding of that
 * path to this engine calls.  Each one cites the reference code it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; every buffer (including workspaces) is
 *    owned by the caller and lives in device memory unless stated otherwise;
 *  - every function only ENQUEUES work on `stream` (asynchronous, graph-capturable,
 *    no allocation, no synchronisation) and returns 0 on success, <0 for an
 *    argument error, >0 for a hipError_t; vlmo_last_error() gives the message;
 *  - token-major activations: row m of an [M, d] matrix is one token; rows are
 *    "packed" (all text tokens of the batch, then all image tokens) and attention
 *    finds its keys through per-sequence segment descriptors, so the reference's
 *    torch.cat([txt, img], dim=1) (vlmo.py:406) never materialises;
 *  - dropout masks come from a counter-based generator keyed by (seed, element),
 *    so backward regenerates them; prob = thresh/65536, thresh 0 = disabled.
 */
#ifndef VLMO_HIP_H
#define VLMO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

enum { VLMO_BF16 = 0, VLMO_F16 = 1, VLMO_F32 = 2 };

/* GEMM epilogues (fused into the accumulator write-back) */
enum {
    VLMO_EPI_BIAS = 0,      /* out[T]   = acc + bias            (relu optional)             */
    VLMO_EPI_BIAS_GELU = 1, /* out[T]   = u = acc + bias ; out2[T] = dropout(gelu_erf(u))    */
    VLMO_EPI_RESID = 2,     /* zd = dropout(acc + bias); out2[T] = zd;                        */
                            /* out[f32] = resid + gamma * zd * row_scale[m]                   */
    VLMO_EPI_DGELU = 3,     /* out[T]   = dropout_mask(acc) * gelu_erf'(aux[m,n])            */
    VLMO_EPI_F32 = 4,       /* out[f32] = acc + bias + beta * out                             */
    VLMO_EPI_DUAL = 5,      /* v = resid[T] + beta*(acc + bias); out[T] = v; out2[T] = relu(v)  */
    VLMO_EPI_ARGMAX = 6,    /* out = partial (max, argmax) of acc + bias per row and 64-column   */
                            /* chunk: float/int32 pairs [M, ldo, 2]; finish with vlmo_argmax_reduce */
    VLMO_EPI_CE = 7,        /* fused cross-entropy forward of a vocabulary head (heads.py:86-112,    */
                            /* objectives.py:57-68,571-582): out = partial {max, sum exp(x - max),    */
                            /* argmax, logit of label row_index[m]} per row and 64-column chunk,      */
                            /* floats [M, ldo, 4]; finish with vlmo_ce_reduce.  No logits in HBM.     */
    VLMO_EPI_CE_BWD = 8     /* out[T] = (exp(acc + bias - lse[m]) - [n == label[m]]) * row_scale[m]:  */
                            /* d loss / d logits recomputed; resid = lse [M] (1-D!), row_index = labels */
};

typedef struct VlmoEpilogue {
    void* out;              /* [M, ldo]                                     */
    void* out2;             /* [M, ld2] (see epilogue table), may be NULL   */
    const float* bias;      /* [N] or NULL                                  */
    const float* gamma;     /* [N] layer-scale or NULL (=1)                 */
    const float* resid;     /* [M, ldo] fp32 residual stream                */
    const float* row_scale; /* drop-path scale: per token [M], or per group */
                            /* when row_index is set (scale[row_index[m]])  */
    const int32_t* row_index; /* [M] token -> scale group, or NULL          */
    const void* aux;        /* [M, ld2] pre-activation for VLMO_EPI_DGELU   */
    int32_t ldo, ld2;
    int32_t relu;           /* bit 0: ReLU on the output (VLMO_EPI_BIAS); bit 1: ReLU on the INPUT activations (vlmo_conv2d_nhwc, f16);
                             * bit 2: VLMO_EPI_BIAS_GELU writes d h / d u = GELU'(u) * dropout mask / (1 - p) to `out` (not u),
                             * and VLMO_EPI_DGELU takes exactly that as `aux`: out = acc * aux, no erf / hash in the backward */
    uint32_t drop_thresh;   /* round(p * 65536); 0 disables dropout         */
    float inv_keep;         /* 1 / (1 - p)                                  */
    float beta;
    uint64_t seed;
    float* colpart;         /* VLMO_EPI_DGELU: [ceil(M/16), N] fp32 or NULL: column-sum partials of   */
                            /* the values written to out; EVERY row is written (an epilogue pass     */
                            /* puts the sums of its 16 or 32 output rows into the row of its first   */
                            /* 16-row block and zeros into the other) -- the fc1 bias gradient is    */
                            /* the fold of these rows (vlmo_colwork_multi kind 0); plain stores      */
} VlmoEpilogue;

const char* vlmo_last_error(void);
/* Version of the struct layouts and signatures below; raised whenever one of them changes
 * (exploremultimodal_amd/hip.py mirrors it as ABI_VERSION and refuses any other). */
#define VLMO_ABI_VERSION 17
int vlmo_abi_version(void);     /* = VLMO_ABI_VERSION of the header the library was built from */

/* C[M,N] = A[M,K] . B[N,K]^T with a fused epilogue.  tile: -1 = pick by shape, 0 = 128x128x64
 * (two workgroups per CU), 3 = 256x256x64 with the two-wave-group ping-pong schedule (one per CU),
 * 4 = 256x128x32 (two per CU; bf16 with the bias / bias+GELU epilogues, else it falls back to 0),
 * 8 = 192x256x64 ping-pong (bf16 with the bias / bias+GELU / residual / GELU-derivative epilogues, else 3): picked when its tile count
 * needs fewer dispatch rounds than 256x256 (VLMo-Large at 32 pairs per GPU),
 * 309..320 = (16 * (tile - 300)) x 256 x 64 ping-pong on v_mfma_f32_16x16x32 (144 .. 320 rows in 16-row steps; bf16, the
 * same four epilogues; 106..110 = the even heights 32 * (tile - 100)): tile height chosen per (M, N) so that the tiles
 * fill whole dispatch rounds of 256 CUs.
 * Replaces nn.functional.linear at vlmo.py:76-78 (qkv), vlmo.py:96 (proj), timm
 * Mlp fc1/fc2 (vlmo.py:141-157, 195-196), the PatchEmbed conv (vlmo.py:304) and,
 * with pre-transposed weights, their input gradients. K % 64 == 0, N % 4 == 0. */
int vlmo_gemm_nt(int epi, int dtype, int tile, const void* A, int lda, const void* B, int ldb,
                 int M, int N, int K, const VlmoEpilogue* e, hipStream_t stream);
/* C = epilogue((seg_scale * A[:, :k1] . B[:, :k1]^T) + A2[:, :K-k1] . B[:, k1:]^T): the reduction runs over two activation
 * matrices with the same rows (own leading dimensions) against ONE weight matrix [N, K].  dall_e EncoderBlock tail
 * (dall_e/encoder.py:45-46): id_path(x) + post_gain * res_path(x) with a convolutional id_path = one GEMM over
 * [conv_3 output | x] against [conv_4.w | id_path.w]; output convolution with the fp32 weight split [w_hi | w_lo]:
 * A2 = A (the activations are read twice instead of being concatenated in HBM).  k1 % 64 == 0; dtype VLMO_F16 only. */
int vlmo_gemm_nt_2src(int epi, int dtype, int tile, const void* A, int lda, int k1, float seg_scale, const void* A2,
                      int lda2, const void* B, int ldb, int M, int N, int K, const VlmoEpilogue* e,
                      hipStream_t stream);
/* 1..4 problems C_g[M_g,N] = A_g[M_g,K] . B_g[N,K]^T with the same N, K, leading dimensions and epilogue kind
 * in ONE launch: the per-modality expert FFNs of a Block below the fusion layer (mlp['l'] on the text rows,
 * mlp['v'] on the image rows: vlmo.py:141-157, 195-196).  e[g] is group g's epilogue (its own outputs, bias,
 * dropout seed).  A launch takes at least one tile time however few tiles it has, so two half-empty launches
 * cost twice one. */
int vlmo_gemm_nt_grouped(int epi, int dtype, int tile, int ngroups, const void* const* A, int lda,
                         const void* const* B, int ldb, const int32_t* M, int N, int K,
                         const VlmoEpilogue* e, hipStream_t stream);

/* C[N1,N2] += alpha * A[M,N1]^T . B[M,N2]  (weight gradients of the linears above, i.e. autograd of
 * vlmo.py:76-78,96,195-196).  The token dimension is split over workgroups; partial products go through
 * the caller's workspace `ws` (>= vlmo_gemm_tn_ws_bytes(M,N1,N2)) and one reduction pass, or, with
 * ws = NULL, straight into C with fp32 atomics. */
int64_t vlmo_gemm_tn_ws_bytes(int M, int N1, int N2);
int vlmo_gemm_tn(int dtype, const void* A, int lda, const void* B, int ldb, float* C, int ldc,
                 int M, int N1, int N2, float alpha, int splits, float* ws, int64_t ws_bytes,
                 hipStream_t stream);

/* Several weight gradients C_q[N1,N2] (+)= alpha * A_q[M,N1]^T . B_q[M,N2] in launches of 256x256 tiles: the
 * qkv / proj / fc1 / fc2 gradients of one or two transformer blocks (autograd of vlmo.py:76-78,96,195-196).
 * accumulate != 0: C += ..., else C = ...  No workspace.  A launch takes the next problems in the given order,
 * at most 16 and at most 960 tiles together (a first problem is always taken).  From 192 tiles on (two VLMo-Base
 * blocks have 216) the launch fills the chip as it is: every tile has one owner that stores or accumulates in place,
 * no partial slabs, no reduction pass, bitwise reproducible.  Below 192 tiles the token dimension of every problem
 * is split over up to 256 / tiles workgroups, which add into C with fp32 atomics (summation order varies); a
 * non-accumulating output is zeroed first (a memset on `stream`).  Every argument of every problem is checked before
 * anything is enqueued: after an argument error (< 0) no output has been touched. */
typedef struct VlmoTnProblem {
    const void* A;
    const void* B;
    float* C;
    int32_t lda, ldb, ldc;
    int32_t M, N1, N2;
    float alpha;
    int32_t accumulate;
} VlmoTnProblem;
int vlmo_gemm_tn_multi(int dtype, const VlmoTnProblem* probs, int n, hipStream_t stream);
/* What vlmo_gemm_tn_multi does with `probs`, from the one planner it executes.  A host function: no device, no stream;
 * reads M, N1, N2 and accumulate of a problem and never its pointers or leading dimensions.  Launch k of *n_launches
 * (<= n) takes the problems [launch_q0[k], launch_q0[k + 1]) and has grid[k] workgroups; workgroup b of it runs
 * order[k * 1024 + b] = (problem index inside the launch << 12) | (workgroup index inside the problem: split * tiles +
 * tile), or nothing (0xFFFF); b % 8 is the XCD.  Caller arrays: launch_q0 [n + 1], prob [n], grid [n], order [n * 1024]
 * (entries past a launch's grid are not written).  Returns 0, or < 0 with nothing meaningful written when the call
 * cannot be planned: vlmo_gemm_tn_multi then fails with the same message before it enqueues anything. */
typedef struct VlmoTnProblemPlan {
    int32_t tiles;          /* 256x256 output tiles                                                          */
    int32_t splits;         /* workgroups per tile, each reducing kt_per_split 64-token K-tiles (the last: the rest) */
    int32_t kt_per_split;
    int32_t mode;           /* 0 = fp32 atomics into C (splits > 1), 1 = C += alpha * acc, 2 = C = alpha * acc */
    int32_t zero_first;     /* C is zeroed before the launch (atomics into a non-accumulating output)        */
} VlmoTnProblemPlan;
int vlmo_gemm_tn_multi_plan(const VlmoTnProblem* probs, int n, int32_t* n_launches, int32_t* launch_q0,
                            VlmoTnProblemPlan* prob, int32_t* grid, uint16_t* order);

/* LayerNorm over the last dim (eps = 1e-12 in VLMo: vlmo_module.py:21-23; vlmo.py:188,192,413).
 * x fp32 [M,d] -> y (bf16, or fp32 when out_f32) at row rowmap[m] (or m), + mean/rstd [M]. */
int vlmo_ln_fwd(const float* x, const float* w, const float* b, void* y, int out_f32,
                float* mean, float* rstd, const int32_t* rowmap, int M, int d, float eps,
                hipStream_t stream);
/* Workspace (bytes) the column-reducing kernels below need for `ncols` reduced columns
 * (ln_bwd and resid_bwd reduce 2*d columns, colsum N).  Caller-owned, reusable across calls
 * on one stream. */
int64_t vlmo_reduce_ws_bytes(int ncols);

/* dx = dres + LN'(dy);  dw += sum dy*xhat;  db += sum dy  (dres may be NULL). */
int vlmo_ln_bwd(const void* dy, int dy_f32, const int32_t* rowmap, const float* x, const float* w,
                const float* mean, const float* rstd, const float* dres, float* dx, float* dw,
                float* db, int M, int d, float* ws, int64_t ws_bytes, hipStream_t stream);

/* vlmo_ln_bwd (dy bf16, no row map) fused with the vlmo_resid_bwd of the residual branch that the LayerNorm's
 * input gradient feeds next (Block backward: norm2, then the attention branch x1 = x + gamma_1 * rs * zd):
 * dz = dropout_mask * dx * gamma * rs, dgamma += sum dx * rs * zd, dbias += sum dz, where dx is the value this
 * call writes.  Saves re-reading dx (fp32 [M, d]) and one launch.  ws: vlmo_reduce_ws_bytes(4 * d). */
int vlmo_ln_resid_bwd(const void* dy, const float* x, const float* w, const float* mean, const float* rstd,
                      const float* dres, float* dx, float* dw, float* db, const void* zd, const float* gamma,
                      const float* row_scale, const int32_t* row_index, void* dz, float* dgamma, float* dbias,
                      uint32_t drop_thresh, float inv_keep, uint64_t seed, int M, int d, float* ws,
                      int64_t ws_bytes, hipStream_t stream);

/* Fused softmax attention over packed rows (vlmo.py:79-95).
 * qkv [M, 3*d] (q | k | v, head-major inside each third), ctx [M, d].
 * seg[s] = {rowA, lenA, rowB, lenB}: sequence s = rows [rowA,rowA+lenA) ++ [rowB,rowB+lenB).
 * keymask [M] int32 (0 = padded key, vlmo.py:89-91) or NULL.  lse [S, heads, NPAD] fp32 (natural log, row stride
 * lse_stride >= max_len).  max_len (the longest sequence of the launch) may be up to 1024; it picks the kernels:
 * <= 512 resident K / V, 513 - 1024 streamed.  Longer launches are refused.
 * Attention dropout (vlmo.py:93) is a counter hash of (seed, mask_seq0 + s, head, query, key) with the counter
 * query * S + key, S = 512 for a sequence of <= 512 tokens and 1024 above -- chosen by the sequence's own length, not
 * by max_len: a backward launch over the sequences [s0, s0 + n) of a forward launch passes mask_seq0 = s0 and the
 * forward's seed to regenerate its mask, whatever its own max_len. */
int vlmo_attn_fwd(const void* qkv, const int32_t* seg, int num_seq, const int32_t* keymask,
                  void* ctx, float* lse, int lse_stride, int heads, int d, int max_len,
                  float scale, uint32_t drop_thresh, float inv_keep, uint64_t seed, int mask_seq0,
                  hipStream_t stream);
/* qv_colsum (optional, [num_seq][2 d] fp32, written): per sequence the column sums of its tokens' dq | dv rows -- the
 * q_bias / v_bias gradient (vlmo.py:71-75) is their sum over the sequences, so nobody re-reads dqkv for it.
 * max_len up to 1024: <= 288 the resident kernels, 289 - 1024 a dK/dV and a dQ streaming kernel back to back (no
 * workspace, no global atomics: dqkv is bitwise reproducible). */
int vlmo_attn_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse,
                  int lse_stride, const int32_t* seg, int num_seq, const int32_t* keymask,
                  void* dqkv, float* qv_colsum, int heads, int d, int max_len, float scale,
                  uint32_t drop_thresh, float inv_keep, uint64_t seed, int mask_seq0, hipStream_t stream);

/* Attention maps: P = softmax((q k^T) * scale + keymask(-inf)) over packed rows (vlmo.py:88-92), written to HBM -- the
 * tensor the reference's Attention / Block return as `attn` and the fused kernels above never form.  Read-only
 * diagnostics: pre-dropout, no backward.
 * qkv, seg, keymask: exactly as vlmo_attn_fwd.  probs fp32, contiguous [num_seq, head_mean ? 1 : heads, nq, seq_len]:
 * query rows [q0, q0 + nq) of every sequence against all keys.  seq_len = key dimension of the output, >= every
 * sequence's length (longer ones are clamped to it), <= 1024.
 * A masked key gets exactly 0; a padded QUERY position is a row like any other (only keys are masked); key columns and
 * query rows past a sequence's own length are 0; a row whose keys are all masked is 0 (the reference has NaN there).
 * head_mean: the arithmetic mean over the heads, summed in head order by one workgroup (no atomics, no workspace):
 * two runs are bitwise equal.  Refused (negative status): d / heads != 64, seq_len outside [1, 1024], q0 < 0, nq < 1,
 * q0 + nq > seq_len, num_seq < 1, null qkv / seg / probs. */
int vlmo_attn_probs(const void* qkv, const int32_t* seg, int num_seq, const int32_t* keymask, float* probs,
                    int heads, int d, int seq_len, int q0, int nq, int head_mean, float scale, hipStream_t stream);

/* Gradient-weighted attention maps (Grad-CAM on `attn`).  With P of vlmo_attn_probs taken as a free variable of
 * ctx = P v, the gradient of a score with respect to P is G[i, j] = sum_c dctx[row_i, 64 h + c] * v[row_j, 64 h + c]
 * per head (bf16 products, fp32 accumulation); dctx is the bf16 [M, d] gradient of the attention context on the packed
 * rows, head-major like ctx.  kind selects what is written to out (fp32, the shape and window of vlmo_attn_probs):
 *   VLMO_GRADCAM_CAM P * max(G, 0)    VLMO_GRADCAM_ATTN_GRAD P * G    VLMO_GRADCAM_GRAD G
 * The zero rules of vlmo_attn_probs hold for every kind, GRAD included: a masked key, key columns and query rows past
 * a sequence's length and a row whose keys are all masked are exactly 0.  head_mean: the mean over heads of the
 * per-head output (of the products, not the product of the means), summed in head order: bitwise reproducible.
 * Up to 512 tokens K and V of a head are resident in LDS; 513 - 1024 K is resident and V is streamed.  Read-only.
 * Refused (negative status, nothing written): whatever vlmo_attn_probs refuses, a null dctx, an unknown kind. */
#define VLMO_GRADCAM_CAM 0
#define VLMO_GRADCAM_ATTN_GRAD 1
#define VLMO_GRADCAM_GRAD 2
int vlmo_attn_gradcam(const void* qkv, const void* dctx, const int32_t* seg, int num_seq, const int32_t* keymask,
                      float* out, int heads, int d, int seq_len, int q0, int nq, int kind, int head_mean, float scale,
                      hipStream_t stream);

/* One step of the relevance propagation over the depth (Chefer et al.'s rule R <- R + Abar R and attention rollout
 * R <- (0.5 I + 0.5 Abar) R, carried as rows from the top layer downward); csrc/relevance.hip.  For every sequence s:
 *   x_out[s, r, c0 + j] = alpha * x_in[s, r, c0 + j] + beta * sum_{k < n} x_in[s, r, c0 + k] * A[s, k, j]
 * A fp32 contiguous [num_seq, n, n] (a head-mean map of the two entry points above); x_in, x_out fp32 contiguous
 * [num_seq, nq, width]; columns outside [c0, c0 + n) of x_out are NOT written: a block-diagonal layer (text and image
 * attended separately) is two calls that tile the width.  fp32 operands and fp32 accumulation on the fp32 MFMA; an
 * element is one chain over k in ascending groups of 16 whatever the grid, with no atomics and no workspace: two runs are
 * bitwise equal.  Every access is guarded: nq, n, width and c0 need not be multiples of anything.
 * Refused (negative status, nothing written): a null pointer; x_out overlapping x_in or A; num_seq < 1; nq < 1; n < 1;
 * n > 1024; width > 1024; c0 < 0; c0 + n > width; non-finite alpha or beta. */
int vlmo_relevance_step(const float* A, const float* x_in, float* x_out, int num_seq, int nq, int width, int c0, int n,
                        float alpha, float beta, hipStream_t stream);

/* Residual-branch backward (vlmo.py:194-196): dz = dx * gamma * row_scale * dropmask/(1-p);
 * dgamma += sum_m dx * row_scale * zd;  dbias += sum_m dz. */
int vlmo_resid_bwd(const float* dx, const void* zd, const float* gamma, const float* row_scale,
                   const int32_t* row_index, void* dz, float* dgamma, float* dbias, int M, int d,
                   uint32_t drop_thresh,
                   float inv_keep, uint64_t seed, float* ws, int64_t ws_bytes, hipStream_t stream);

/* out[c] += sum_m x[m, c]  (bias gradients), x is bf16/f16 [M, ld]. */
int vlmo_colsum(int dtype, const void* x, int ld, float* out, int M, int N, float* ws,
                int64_t ws_bytes, hipStream_t stream);

/* Column work of several producers in ONE launch (the bias / layer-scale / LayerNorm-weight gradients of one or
 * two transformer blocks):  kind 0 folds fp32 partial rows ws[rows, ld] (the column partials the kernels behind
 * vlmo_ln_bwd / vlmo_ln_resid_bwd / vlmo_resid_bwd, the VLMO_EPI_DGELU epilogue and vlmo_attn_bwd's qv_colsum leave
 * behind), kind 1 sums the columns of a bf16/f16 matrix x[rows, ld].
 * Column c goes to out[c / n0][c % n0] += sum (out[k] may be NULL). */
typedef struct VlmoColJob {
    int32_t kind, ld;
    const void* src;
    int32_t rows, ncols;
    float* out[4];
    int32_t n0, pad_;
} VlmoColJob;
int vlmo_colwork_multi(int dtype, const VlmoColJob* jobs, int n, hipStream_t stream);

/* fp32 -> bf16/f16 weight shadow copies: dst = cast(src), dstT = cast(src)^T (either may be NULL). */
int vlmo_cast_weight(int dtype, const float* src, int rows, int cols, void* dst, void* dstT,
                     hipStream_t stream);
/* n weights in one launch (every weight of the model is stale after an optimizer step): job q casts src[q] [rows[q], cols[q]]
 * fp32 into dst[q] (same layout, may be NULL) and dstT[q] (transposed, may be NULL). */
int vlmo_cast_weight_multi(int dtype, int n, const float* const* src, const int32_t* rows, const int32_t* cols,
                           void* const* dst, void* const* dstT, hipStream_t stream);

/* Image embedding (vlmo.py:298-319, timm PatchEmbed):
 *  patchify: image f32 [B,C,H,W] -> bf16 [B*gh*gw, C*p*p] rows ordered (b, py, px), cols (c, ky, kx)
 *  finish:   x[b,0] = cls + pos[0] + type;  x[b,1+i] = (masked? mask_token : proj[b,i]) + pos[1+i] + type */
int vlmo_patchify(const float* img, void* out, int B, int C, int H, int W, int patch,
                  hipStream_t stream);
int vlmo_embed_img_finish(const void* proj, const float* cls_tok, const float* mask_tok,
                          const float* pos, const float* type_row, const uint8_t* masked_pos,
                          float* x, int B, int npatch, int d, uint32_t drop_thresh,
                          float inv_keep, uint64_t seed, hipStream_t stream);
/* backward of finish: dproj[b,i] = masked? 0 : g; dcls += ; dmask += ; dpos += ; dtype_row += */
int vlmo_embed_img_bwd(const float* dx, const uint8_t* masked_pos, void* dproj, float* dcls,
                       float* dmask, float* dpos, float* dtype_row, int B, int npatch, int d,
                       uint32_t drop_thresh, float inv_keep, uint64_t seed, hipStream_t stream);

/* Text embedding (vlmo.py:321-324 + transformers BertEmbeddings):
 *  e = word[ids] + btype0 + pos[t];  x = LN_eps(e) (+dropout) + type0 */
int vlmo_embed_txt_fwd(const int64_t* ids, const float* word, const float* pos, const float* btype0,
                       const float* ln_w, const float* ln_b, const float* type0, float* x,
                       float* xhat, float* rstd, int B, int T, int d, float eps,
                       uint32_t drop_thresh, float inv_keep, uint64_t seed, hipStream_t stream);
int vlmo_embed_txt_bwd(const float* dx, const int64_t* ids, const float* xhat, const float* rstd,
                       const float* ln_w, float* dword, float* dpos, float* dbtype0, float* dln_w,
                       float* dln_b, float* dtype0, int B, int T, int d, uint32_t drop_thresh,
                       float inv_keep, uint64_t seed, hipStream_t stream);
/* Row-table form of the text embedding, for batches whose texts have different row counts: sample b keeps its first
 * len_b positions (1 <= len_b <= T) in packed rows off[b] .. off[b] + len_b - 1; the others are in no row.  Same
 * arithmetic per row as the pair above; the dropout stream is indexed by the packed row.
 *  fwd: src int32 [nrows], src[m] = b * T + t of packed row m; x / xhat [nrows, d], rstd [nrows].
 *  bwd: off int32 [B + 1] = prefix sums of len_b, maxlen = max len_b (host value, <= T).  dpos, dbtype0, dln_w, dln_b
 *       and dtype0 (each may be NULL) get += sums taken in a fixed order over a workspace of
 *       vlmo_embed_txt_rows_ws_bytes(B, maxlen, d) bytes (a host function): two runs give the same bits.  dword is
 *       scatter-added with float atomics as in vlmo_embed_txt_bwd; row 0 (padding_idx) gets nothing. */
int vlmo_embed_txt_rows_fwd(const int64_t* ids, const int32_t* src, const float* word, const float* pos,
                            const float* btype0, const float* ln_w, const float* ln_b, const float* type0,
                            float* x, float* xhat, float* rstd, int nrows, int T, int d, float eps,
                            uint32_t drop_thresh, float inv_keep, uint64_t seed, hipStream_t stream);
int64_t vlmo_embed_txt_rows_ws_bytes(int B, int maxlen, int d);
int vlmo_embed_txt_rows_bwd(const float* dx, const int64_t* ids, const int32_t* off, const float* xhat,
                            const float* rstd, const float* ln_w, float* dword, float* dpos, float* dbtype0,
                            float* dln_w, float* dln_b, float* dtype0, float* ws, int64_t ws_bytes, int B, int T,
                            int maxlen, int d, uint32_t drop_thresh, float inv_keep, uint64_t seed,
                            hipStream_t stream);

/* Optional timing of the GEMM launches with HIP event pairs on their launch stream (bench.py's roofline).
 * stop() sums per tag: tag = epilogue id (+16 for the 256x256 tile, +48 for the 256x128 tile) for vlmo_gemm_nt, 32 + epilogue for
 * vlmo_conv2d_nhwc, 64 / 72 for vlmo_gemm_tn (128x128 / 256x256 tiles), 73 for vlmo_gemm_tn_multi; returns the number of recorded launches. Synchronise first. */
int vlmo_profile_start(int max_records);
int vlmo_profile_stop(int ntags, double* ms, double* flops, int64_t* launches);

/* ---- optimizer step ---------------------------------------------------------------
 * Multi-tensor Adam / AdamW over a list of fp32 tensors, replacing apex FusedAdam(adam_w_mode=True)
 * (utils/optim_factory.py:185-186) and the unscale + clip_grad_norm_ of NativeScalerWithGradNormCount
 * (utils/utils.py:343-364).  All tables are DEVICE arrays owned by the caller: per tensor the device
 * addresses of parameter / gradient / exp_avg / exp_avg_sq, its element count, learning rate and weight
 * decay; the work list is cut into chunks of `chunk` elements (chunk_tensor[c], chunk_start[c]). */
typedef struct {
    const int64_t* p;
    const int64_t* g;
    const int64_t* m;
    const int64_t* v;
    const int64_t* numel;
    const float* lr;
    const float* wd;
    const int32_t* chunk_tensor;
    const int64_t* chunk_start;
    int32_t n_chunks, chunk;
} VlmoTensorList;

typedef struct {
    float beta1, beta2, eps;
    float inv_bc1, inv_bc2;     /* 1 / (1 - beta^step), or 1 without bias correction */
    int32_t adam_w_mode;        /* 1: decoupled weight decay (AdamW); 0: L2 (decay added to the gradient) */
} VlmoAdamArgs;

/* out[0] = || inv_scale * g ||_2 over every tensor of the list, out[1] = the factor to apply to the raw
 * gradients = inv_scale * min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; max_norm <= 0:
 * no clipping), out[2] = 1 if the norm is not finite.  partial: n_chunks floats of scratch.  Deterministic, and
 * summed in double: another order of the same tensors, or another alignment, changes the sum below 1e-13 of it, so
 * the fp32 result is the same but for a tie in the final roundings. */
int vlmo_mt_grad_norm(const VlmoTensorList* tl, float inv_scale, float max_norm, float* partial, float* out,
                      hipStream_t stream);
/* One Adam step on every tensor.  ctl = the 3 floats of vlmo_mt_grad_norm (gradients are multiplied by
 * ctl[1]; the whole step is skipped when ctl[2] != 0, like GradScaler.step) or NULL. */
int vlmo_mt_adam(const VlmoTensorList* tl, const VlmoAdamArgs* a, const float* ctl, hipStream_t stream);
/* Weight average (the reference's model_ema, timm ModelEmaV2; conf/config.yaml:140-141), fp32:
 *   e <- e + w (p - e),  w = 1 - decay in [0, 1],
 * computed as fmaf(w, p - e, e), and from w = 0.5 on from p's side, fmaf(w - 1, p - e, p), as torch.lerp does.  e == p is an
 * exact fixed point, w = 0 leaves e and w = 1 copies p bit for bit.
 * Standalone over a list: tl->p[t] = the average (written in place), tl->g[t] = the tensor it follows; numel and the chunk
 * tables as for vlmo_mt_adam, the other tables unused. */
int vlmo_mt_ema(const VlmoTensorList* tl, float w, hipStream_t stream);
/* vlmo_mt_adam with the average of the NEW parameter value folded into the same pass (8 more bytes of traffic per
 * element instead of 12 and a launch).  ema = DEVICE table parallel to tl->p with the address of each tensor's average, or 0
 * for a tensor without one.  Element for element the result of vlmo_mt_adam followed by vlmo_mt_ema; when ctl[2] != 0 the
 * parameters and moments stay untouched and the averages still move toward the unchanged parameters. */
int vlmo_mt_adam_ema(const VlmoTensorList* tl, const VlmoAdamArgs* a, const float* ctl, const void* const* ema, float w,
                     hipStream_t stream);

/* The stream vlmo_stack_bwd's deferred parameter-gradient work runs on (VlmoStackDesc.side_stream).  It has the
 * whole step of slack while the activation-gradient chain on the caller's stream is the critical
 * path, so it is created with the LOWEST dispatch priority of the device (low_priority != 0), and/or
 * confined to the compute units of cu_mask (cu_mask_words 32-bit words; NULL/0 = all CUs). */
int vlmo_side_stream_create(int low_priority, const uint32_t* cu_mask, int cu_mask_words, hipStream_t* out);

/* ---- one transformer Block of a stack (vlmo.py:187-197 and its autograd) ---------------------
 * norm1 -> qkv -> attention -> proj(+gamma_1, residual) -> norm2 -> expert FFN(s) (+gamma_2,
 * residual), resp. the whole backward of that.  Expert e works on rows [exp_row0[e], +exp_rows[e]);
 * attention launch a on seg[a] (sequences of at most maxlen[a] tokens).  All buffers caller-owned. */
typedef struct VlmoBlockDesc {
    int32_t M, d, hidden, heads;
    int32_t n_experts, exp_row0[2], exp_rows[2];   /* 1..2 experts */
    int32_t n_attn, nseq[2], maxlen[2], lse_stride[2];
    int32_t attn_seed_idx[2], attn_seq0[2];         /* dropout mask of launch a: seed + 11 + attn_seed_idx[a], first sequence attn_seq0[a]
                                                     * (a backward launch split off a shared forward launch keeps the forward's mask) */
    const int32_t* seg[2];
    const int32_t* keymask;
    float eps;
    uint32_t drop_thresh, attn_drop_thresh;
    float inv_keep, attn_inv_keep;
    uint64_t seed;
    const float* rs1;           /* drop-path scales of the two residual branches: per row, or per */
    const float* rs2;           /* group when row_index is set                                     */
    const int32_t* row_index;
    int32_t tile, need_bwd;
    /* parameters: fp32 vectors, bf16 shadow matrices W [out,in] and W^T [in,out] */
    const float *g1, *g2, *n1w, *n1b, *n2w, *n2b, *qkv_bias, *proj_b;
    const void *qkv_w, *qkv_wT, *proj_w, *proj_wT;
    const float *b1[2], *b2[2];
    const void *w1[2], *w1T[2], *w2[2], *w2T[2];
    /* forward activations (saved for backward).  fp32 [M, d]: x (input), x1 (after the attention branch), x2 (output).
     * bf16: y1, ctx, zd1, y2, zd2 [M, d]; qkv [M, 3 d]; u, h [M, hidden] (pre- / post-GELU).
     * fp32: mean1, rstd1, mean2, rstd2 [M]; lse[a] [nseq[a] * heads, lse_stride[a]]. */
    const float* x;
    float *x1, *x2;
    void *y1, *qkv, *ctx, *zd1, *y2, *u, *h, *zd2;
    float *mean1, *rstd1, *mean2, *rstd2, *lse[2];
    /* backward.  fp32 [M, d]: dx2 (incoming), dx1, dx0 (outgoing).
     * bf16: dz2, dy2, dz1, dctx, dy1 [M, d]; du [M, hidden]; dqkv [M, 3 d].  dctx may be the buffer of dy2. */
    const float* dx2;
    float *dx1, *dx0;
    void *dz2, *du, *dy2, *dz1, *dctx, *dqkv, *dy1;
    float *dg1, *dg2, *dn1w, *dn1b, *dn2w, *dn2b, *dqkv_w, *dqkv_b, *dproj_w, *dproj_b;
    float *dw1[2], *db1[2], *dw2[2], *db2[2];
    float* ws_main;             /* column-reduction scratch (see vlmo_stack_bwd)                         */
    int64_t ws_bytes;
} VlmoBlockDesc;

/* ---- all blocks of one backbone pass in ONE call per direction (the loops at vlmo.py:402-411) -------------
 * blocks[] are in forward order; block i's x2 is block i+1's x.  vlmo_stack_fwd runs the blocks' forwards in order.
 * vlmo_stack_bwd runs the activation-gradient chains of all blocks back to back on `stream` and defers the
 * parameter-gradient work (weight-gradient GEMMs, bias / layer-scale / LayerNorm column sums) to
 * `side_stream` in batches of `wgrad_batch` blocks, one vlmo_gemm_tn_multi + one vlmo_colwork_multi launch
 * per batch (parameter gradients are ACCUMULATED: zero or pre-load them; with wgrad_store only the vector ones).  Because that work runs later than
 * the block's own chain, the caller gives the k-th block in backward order its own backward temporaries
 * (dz2, du, dz1, dqkv) and column workspace ws_main of ws_bytes >= vlmo_stack_bwd_ws_bytes(M, d, hidden, sequences of
 * the block's attention launches) bytes, rotating over n_tmp_sets > wgrad_batch sets (set k % n_tmp_sets).  A block
 * with a smaller workspace is an argument error, found before anything is enqueued (up to ABI 12 such a block ran with
 * extra passes over du and dqkv and without the fusion across blocks).  The call waits for a set's deferred readers
 * before reusing it and joins the side stream before it returns control of the buffers.  grad_ready (optional,
 * [n_blocks] hipEvent_t handles from vlmo_event_create): event i is recorded when block i's parameter gradients
 * are complete, so a gradient all-reduce on another stream can start per block (vlmo_stream_wait_event). */
typedef struct VlmoStackDesc {
    int32_t n_blocks, wgrad_batch, n_tmp_sets;
    int32_t wgrad_store;        /* != 0: weight-gradient MATRICES are written (C = ...), not accumulated: no zero-fill, no
                                 * read of C.  The vector gradients (biases, LayerNorm, layer-scale) always accumulate. */
    const VlmoBlockDesc* blocks;
    hipStream_t side_stream;
    void* const* grad_ready;
} VlmoStackDesc;
/* Bytes of VlmoBlockDesc.ws_main for a block of M rows and at most max_seqs attention sequences: the partial rows of the
 * LayerNorm / residual-branch folds, the fc1-bias column partials and the per-sequence q / v bias sums, sized for two
 * experts and the fusion with the block below whatever the block has.  Monotone in every argument. */
int64_t vlmo_stack_bwd_ws_bytes(int M, int d, int hidden, int max_seqs);
int vlmo_stack_fwd(const VlmoStackDesc* s, hipStream_t stream);
int vlmo_stack_bwd(const VlmoStackDesc* s, hipStream_t stream);
int vlmo_event_create(void** out);
int vlmo_event_destroy(void* ev);
int vlmo_stream_wait_event(hipStream_t stream, void* ev);

/* ---- gradient exchange (replaces torch DDP / DeepSpeed ZeRO-2 over NCCL, train/pretrain/multimodal.py:61-95,
 * conf/ds_stage/l2.yaml) ----
 * RCCL over xGMI, one communicator per process, collectives enqueued on the caller's stream, sum reduction.  RCCL is
 * resolved at run time (the copy already in the process, else librccl.so); without it every entry returns -1 (an argument
 * error, message in vlmo_last_error); RCCL's own failures come back as 1000 + ncclResult_t.
 * Bootstrap: rank 0 calls vlmo_comm_unique_id and hands the 128 bytes to the other ranks by any means (the Python host
 * uses the torch.distributed store); every rank then calls vlmo_comm_init (blocks until all ranks arrived). */
#define VLMO_COMM_ID_BYTES 128
int vlmo_comm_available(void);
int vlmo_comm_unique_id(void* id128);
int vlmo_comm_init(void** comm, const void* id128, int rank, int world);
/* waits for the device to drain (every collective enqueued through the communicator has finished), then frees it */
int vlmo_comm_destroy(void* comm);
/* the size of the communicator as RCCL reports it (ncclCommCount) and this process' rank in it (rank may be NULL) */
int vlmo_comm_count(void* comm, int* ranks, int* rank);
int vlmo_comm_all_reduce(void* comm, const void* send, void* recv, int64_t count, int dtype, hipStream_t stream);
/* send [world * recv_count] -> recv [recv_count] = this rank's slice of the sum (ZeRO-2 gradient partition) */
int vlmo_comm_reduce_scatter(void* comm, const void* send, void* recv, int64_t recv_count, int dtype,
                             hipStream_t stream);
/* send [send_count] -> recv [world * send_count]; send may be recv + rank * send_count (in place) */
int vlmo_comm_all_gather(void* comm, const void* send, void* recv, int64_t send_count, int dtype,
                         hipStream_t stream);
/* the reducer's two passes over a gradient arena: dst bf16 = src * scale (1 / world), and back.  16-B aligned. */
int vlmo_grad_pack(const float* src, void* dst_bf16, int64_t n, float scale, hipStream_t stream);
int vlmo_grad_unpack(const void* src_bf16, float* dst, int64_t n, hipStream_t stream);

/* ---- dall_e dVAE encoder (dall_e/encoder.py:49-133) and decoder (dall_e/decoder.py:49-136), fp16 NHWC activations
 * [B*H*W, C] ---- */

/* Conv2d, stride 1, same padding (kw-1)/2 (dall_e/utils.py:37-48) as implicit GEMM:
 * x [B*H*W, Cin], w [Cout, kw*kw*Cin] (tap-major, channel-minor), zero_page = >= 128 zero bytes.
 * Epilogues: VLMO_EPI_BIAS (relu flag), VLMO_EPI_DUAL (block tail id + post_gain * res, encoder.py:45-46 and
 * decoder.py:45-46: resid = the identity path's rows in the activation type, [M, ldo]; out2 may be NULL), VLMO_EPI_F32. */
int vlmo_conv2d_nhwc(int epi, int dtype, const void* x, int B, int H, int W, int Cin, int kw,
                     const void* w, int Cout, const void* zero_page, const VlmoEpilogue* e,
                     hipStream_t stream);
/* stem input: image f32 NCHW -> f16 [B*H*W, Kpad] patches, column = c*kw*kw + ky*kw + kx. */
int vlmo_dvae_im2col(const float* x, void* out, int B, int C, int H, int W, int kw, int Kpad,
                     hipStream_t stream);
/* MaxPool2d(2) (encoder.py:85,95,105): raw pooled map + relu of it (relu may be NULL). */
int vlmo_maxpool2_nhwc(const void* x, void* raw, void* relu, int B, int H, int W, int C,
                       hipStream_t stream);
/* Decoder input convolution on a one-hot map (decoder.py:77-78 after modeling_discrete_vae.py:241-243) as a row gather:
 * out f16 [M, n_init] = fp16(table[ids[m]] + bias), table = the fp32 weight transposed to [vocab, n_init].  n_init % 8 == 0.
 * ids must lie in [0, vocab): the caller checks them (an id outside is clamped, never dereferenced outside the table). */
int vlmo_dvae_embed(const int64_t* ids, const float* table, const float* bias, void* out, int M, int vocab,
                    int n_init, hipStream_t stream);
/* nn.Upsample(scale_factor=2, mode='nearest') (decoder.py:85,95,105): x f16 [B*H*W, C] -> out f16 [B*2H*2W, C]. C % 8 == 0. */
int vlmo_upsample2_nhwc(const void* x, void* out, int B, int H, int W, int C, hipStream_t stream);
/* Decoder output head (decoder.py:116-123): out f32 NCHW [B, Cout, H, W] = conv1x1(relu(x)) + bias for x f16 [B*H*W, C],
 * w f16 [Cout, C], 1 <= Cout <= 8, C % 8 == 0, C <= 1024. */
int vlmo_dvae_out_head(const void* x, const void* w, const float* bias, float* out, int B, int H, int W, int C,
                       int Cout, hipStream_t stream);
/* ---- BEiT-style DiscreteVAE (models/modeling_discrete_vae.py:81-221), fp16 NHWC activations; its 3x3 / 1x1 layers,
 * the arg-max and the codebook lookup run on the entry points above ---- */

/* Conv2d(Cin, Cout, 4, stride=2, padding=1) as implicit GEMM: x f16 [B*H*W, Cin] -> e->out f16 [B*(H/2)*(W/2), ldo];
 * output pixel (oy, ox) reads input (2 oy - 1 + ky, 2 ox - 1 + kx), taps outside the image read zero_page (>= 128 zero
 * bytes).  w f16 [Cout, 16*Cin], tap-major (4 ky + kx), channel-minor.  Epilogue: e->bias (may be NULL), e->relu bit 0.
 * dtype VLMO_F16; H, W even; Cin % 64 == 0; Cout % 8 == 0; ldo % 8 == 0. */
int vlmo_conv4s2_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, const void* w, int Cout,
                      const void* zero_page, const VlmoEpilogue* e, hipStream_t stream);
/* ConvTranspose2d(Cin, Cout, 4, stride=2, padding=1): x f16 [B*H*W, Cin] -> e->out f16 [B*2H*2W, ldo]; the four output
 * parities (oy & 1, ox & 1) are four 2x2 convolutions of one launch (no zero-stuffed input).  w f16 [4][Cout, 4*Cin]:
 * quarter p = 2 py + px, column (2 a + b) * Cin + c holds weight[c, n, 1 - py + 2 a, 1 - px + 2 b] of the PyTorch layout
 * [Cin, Cout, 4, 4], met by input pixel (y + py - a, x + px - b) for output pixel (2 y + py, 2 x + px).  Epilogue and
 * limits as vlmo_conv4s2_nhwc (no parity condition on H, W). */
int vlmo_convt4s2_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, const void* w, int Cout,
                       const void* zero_page, const VlmoEpilogue* e, hipStream_t stream);
/* stem input of the 4x4 stride-2 convolution: image f32 NCHW -> f16 [B*(H/2)*(W/2), Kpad] patches, column = c*16 + ky*4 + kx
 * (zero outside the image and beyond C*16).  H, W even; Kpad % 8 == 0, Kpad >= 16 C. */
int vlmo_dvae_patch4s2(const float* x, void* out, int B, int C, int H, int W, int Kpad, hipStream_t stream);
/* vlmo_dvae_out_head without the ReLU: out f32 NCHW [B, Cout, H, W] = conv1x1(x) + bias (modeling_discrete_vae.py:135).
 * Same limits. */
int vlmo_dvae_out_head_linear(const void* x, const void* w, const float* bias, float* out, int B, int H, int W, int C,
                              int Cout, hipStream_t stream);

/* finish of VLMO_EPI_CE: partial [M, nchunk, 4] -> lse [M], loss [M] (lse - label logit; 0 where
 * labels[m] == ignore_index; may be NULL), pred [M] (arg-max, first maximum wins; may be NULL). */
int vlmo_ce_reduce(const float* partial, int nchunk, const int32_t* labels, int ignore_index, float* lse,
                   float* loss, int32_t* pred, int M, hipStream_t stream);
/* final step of Dalle_VAE.get_codebook_indices (modeling_discrete_vae.py:246-248):
 * partial [M, nchunk, 2] from VLMO_EPI_ARGMAX -> ids int64 [M] (first maximum wins). */
int vlmo_argmax_reduce(const float* partial, int nchunk, int64_t* ids, int M, hipStream_t stream);

/* ---- VQA classifier head (vlmo_module.py:85-93, objectives.py:12-21, 317-353) ---- */

/* h [M, ldh] bf16 = GELU_erf(LayerNorm(x) * w + b), eps as given (1e-12), fp32 statistics -> mean, rstd [M].
 * x fp32 [M, ldx]; 0 < d <= 2048, d % 4 == 0; ldx, ldh multiples of 4; columns [d, ldh) of h are written as 0
 * (the zero pad of the next GEMM's reduction dimension). */
int vlmo_ln_gelu_fwd(const float* x, int ldx, const float* w, const float* b, void* h, int ldh, float* mean,
                     float* rstd, int M, int d, float eps, hipStream_t stream);
/* Backward of vlmo_ln_gelu_fwd from dh = d loss / d h (fp32 [M, lddh]): recomputes the LayerNorm output, applies
 * GELU', then the LayerNorm backward.  dx fp32 [M, lddx] and / or dxb bf16 [M, lddxb] (pad columns [d, lddxb) = 0);
 * dw, db (LayerNorm weight / bias) and dbias (= column sums of dx: the bias gradient of the Linear that produced x)
 * are OVERWRITTEN, each may be NULL.  Column sums are deterministic: fixed-order partial rows in ws, folded in order,
 * no atomics.  ws: min(M, 128) * 3 * d floats. */
int vlmo_ln_gelu_bwd(const float* dh, int lddh, const float* x, int ldx, const float* w, const float* b,
                     const float* mean, const float* rstd, float* dx, int lddx, void* dxb, int lddxb, float* dw,
                     float* db, float* dbias, int M, int d, float* ws, int64_t ws_bytes, hipStream_t stream);
/* Per row of the fp32 logits z [B, ldz] (first V columns) against targets y fp32 [B, ldy]:
 *   row_loss[r]  = sum_n max(z,0) - z*y + log1p(exp(-|z|))      (binary cross-entropy with logits, summed)
 *   row_arg[r]   = arg-max of z[r, :V]; the FIRST maximum wins (smallest column among equal values)
 *   row_score[r] = y[r, row_arg[r]]
 * each output may be NULL; y may be NULL when row_loss and row_score are.  Backward mode (dz != NULL): also writes
 * dz bf16 [B, lddz] = (sigmoid(z) - y) * alpha * (*dscale) (+ dadd fp32 [B, ldadd] when given), with the pad columns
 * [V, lddz) = 0; lddz a multiple of 64.  dscale: device scalar (NULL = 1); y NULL = no loss term. */
int vlmo_vqa_bce(const float* z, int ldz, const float* y, int ldy, int B, int V, float* row_loss, int32_t* row_arg,
                 float* row_score, const float* dscale, float alpha, const float* dadd, int ldadd, void* dz, int lddz,
                 hipStream_t stream);

/* ---- ISDA of the VQA classifier's last Linear (heads.py:6-83, objectives.py:325-344); csrc/isda.hip ---- */

/* Estimator update, in place, and the arg-max class of every target row.  Features f [B, A] fp32: with ln_w given,
 * f = GELU_erf(LayerNorm(u) * ln_w + ln_b) recomputed from the pre-LayerNorm rows u [B, ldu] and the statistics
 * mean, rstd [B] of vlmo_ln_gelu_fwd; with ln_w NULL, f = u.  Targets y fp32 [B, ldy] (first V columns).  For each
 * class c with n_c = #{n : y[n, c] != 0} > 0: ave, var = mean and population variance of its member rows (ascending
 * n), w = n_c / (n_c + count[c]), cov[c] = cov[c](1 - w) + var w + w(1 - w)(emean[c] - ave)^2,
 * emean[c] = emean[c](1 - w) + ave w, count[c] += n_c; classes with n_c = 0 are not written.  count [V],
 * emean, cov [V, A] fp32 contiguous.  k int32 [B] = first arg-max of each target row (0 for an all-zero row).
 * 0 < A <= 2048, A % 4 == 0, ldu % 4 == 0. */
int vlmo_isda_update(const float* u, int ldu, const float* mean, const float* rstd, const float* ln_w,
                     const float* ln_b, const float* y, int ldy, int B, int V, int A, float* count, float* emean,
                     float* cov, int32_t* k, hipStream_t stream);
/* Bytes of the workspace of vlmo_isda_aug_fwd / vlmo_isda_aug_bwd for (B, V, A). */
int64_t vlmo_isda_ws_bytes(int B, int V, int A);
/* z[n, j] += scale * sum_a (W[j, a] - W[k[n], a])^2 * ck[n, a] for n < B, j < V (columns >= V untouched).
 * W fp32 [V, ldw], k int32 [B] with values in [0, V), ck fp32 [B, ldc] (the covariance rows cov[k[n]]), z fp32
 * [B, ldz].  fp32 arithmetic; fixed-order partial sums over A in ws: bitwise reproducible. */
int vlmo_isda_aug_fwd(const float* W, int ldw, const int32_t* k, const float* ck, int ldc, int B, int V, int A,
                      float scale, float* z, int ldz, float* ws, int64_t ws_bytes, hipStream_t stream);
/* Weight gradient of the augmentation for G = d loss / d z_aug (bf16 [B, ldg]) and r = 2 * scale:
 *   dw[j, a] += r * sum_n G[n, j] (W[j, a] - W[k_n, a]) ck[n, a]
 *             - r * sum_{n: k_n = j} ck[n, a] * sum_j' G[n, j'] (W[j', a] - W[j, a])
 * dw fp32 [V, lddw] (an accumulator; rows >= V untouched).  No atomics, fixed summation order. */
int vlmo_isda_aug_bwd(const void* G, int ldg, const float* W, int ldw, const int32_t* k, const float* ck, int ldc,
                      int B, int V, int A, float r, float* dw, int lddw, float* ws, int64_t ws_bytes,
                      hipStream_t stream);

/* ---- retrieval ranking (zero-shot / fine-tuned image-text retrieval on the ITC features); csrc/retrieval.hip ---- */

/* For every query row q < Nq the K best gallery rows under score(q, g) = scale * sum_d Q[q, d] * G[g, d], best first, in
 * out_val fp32 / out_idx int32, both [Nq, K] contiguous.  The order is total: higher score first, and among equal scores
 * the lower gallery index first.  With Ng < K the tail of a row is idx = -1, val = -inf.  Q [Nq, ldq], G [Ng, ldg] fp32;
 * fp32 MFMA operands and accumulation; the [Nq, Ng] score matrix never reaches memory.  Inputs are assumed finite.
 * Limits: 1 <= K <= 16; 4 <= D <= 1024, D % 4 == 0; ldq, ldg >= D; scale > 0; Nq, Ng >= 1.
 * The gallery is cut into `splits` contiguous slices (0 = chosen by the library so that a small query count still fills
 * the chip; never more slices than 128-row steps of the gallery); with more than one slice the per-slice lists go through
 * ws (>= vlmo_sim_topk_ws_bytes of the same Nq, Ng, K, splits; 0 bytes for one slice) and a merge kernel.  No atomics; a
 * score is one fixed-order chain over D whatever the tile or split: the same bits from run to run and for every splits. */
int64_t vlmo_sim_topk_ws_bytes(int Nq, int Ng, int K, int splits);
int vlmo_sim_topk(const float* Q, int ldq, const float* G, int ldg, int Nq, int Ng, int D, int K, float scale, int splits,
                  void* ws, size_t ws_bytes, float* out_val, int32_t* out_idx, hipStream_t stream);

/* ---- input preparation: the two image views of a sample from decoded pixels; csrc/augment.hip ---- */

/* One source image of the packed byte buffer: uint8 [H, W, 3] starting `offset` bytes into it (any alignment). */
typedef struct {
    int64_t offset;
    int32_t H, W;
} VlmoImage;

enum { VLMO_FILTER_BICUBIC = 0, VLMO_FILTER_LANCZOS = 1 };          /* Keys a = -0.5, radius 2; Lanczos, radius 3 */
enum { VLMO_FINISH_NORMALIZE = 0, VLMO_FINISH_MAP_PIXELS = 1 };     /* (v / 255 - mean) / std; (1 - 2 eps) v / 255 + eps */
#define VLMO_CROP_MAX_SIZE 1024     /* output side S */
#define VLMO_CROP_MAX_SIDE 8192     /* crop box side */
#define VLMO_CROP_MAX_JOBS 65536    /* jobs per call */

/* One output view: crop box (top, left, h, w) of image `image`, resampled to S x S with `filter`, mirrored when flip = 1,
 * finished with `finish`, written to out fp32 [3, S, S].  tmp_off: where the job's fp32 intermediate [h, S, 3] starts in
 * the workspace, in floats: the sum of h * S * 3 over the jobs before it. */
typedef struct {
    int32_t image, top, left, h, w;
    int32_t flip, S, filter, finish, pad_;
    int64_t tmp_off;
    float* out;
} VlmoCropJob;

/* Every job of a batch in two launches, whatever their number (data/utils/transforms.py:8-138 + the flip, ToTensor and
 * Normalize / map_pixels of data/base_dataset.py, which the reference runs on the CPU with PIL).  Per job: crop first
 * (pixels outside the box do not exist for the filter), then a separable resampling, horizontal pass then vertical, with
 * PIL's windows: per axis of input length n, scale = n / S, fs = max(scale, 1), support = R * fs, output o has centre
 * (o + 0.5) * scale and taps k in [max(0, int(centre - support + 0.5)), min(n, int(centre + support + 0.5))) with weight
 * f((k + 0.5 - centre) / fs) divided by the sum of the output's weights.  Weights are computed on the device (fp64, rounded
 * to fp32); values stay fp32 between the passes and at the end, unclamped (PIL rounds to uint8 after each pass).
 * src: device bytes, 4-byte aligned, src_bytes a multiple of 4 (pad the tail).  images / jobs: HOST tables, checked here;
 * images_dev / jobs_dev: the same tables in device memory, read by the kernels.  mean, std: 3 host floats each.
 * pixel_eps: the eps of VLMO_FINISH_MAP_PIXELS.  ws: device workspace of at least 4 * sum(h * S * 3) bytes.
 * Limits: 3 channels; 1 <= S <= VLMO_CROP_MAX_SIZE; 1 <= h, w <= VLMO_CROP_MAX_SIDE; the box inside its image; 1 <= n_jobs
 * <= VLMO_CROP_MAX_JOBS.  No atomics, fixed summation order: the same bits from run to run and for any order of the jobs. */
int vlmo_crop_resample(const uint8_t* src, int64_t src_bytes, const VlmoImage* images, const VlmoImage* images_dev,
                       int n_images, const VlmoCropJob* jobs, const VlmoCropJob* jobs_dev, int n_jobs, const float* mean,
                       const float* std, float pixel_eps, float* ws, int64_t ws_bytes, hipStream_t stream);

/* ---- RandAugment on the packed sources, in front of the crop (data/utils/randaugment.py); csrc/randaug.hip ---- */

enum {
    VLMO_AUG_SKIP = -1,         /* the slot was not kept: a copy */
    VLMO_AUG_IDENTITY = 0,
    VLMO_AUG_AUTOCONTRAST = 1,  /* table ops: 1, 2, 3 and 10 .. 12 */
    VLMO_AUG_EQUALIZE = 2,
    VLMO_AUG_BRIGHTNESS = 3,    /* a = factor */
    VLMO_AUG_SHARPNESS = 4,     /* a = factor */
    VLMO_AUG_SHEAR_X = 5,       /* a = shear factor */
    VLMO_AUG_SHEAR_Y = 6,
    VLMO_AUG_TRANSLATE_X = 7,   /* a = offset in pixels */
    VLMO_AUG_TRANSLATE_Y = 8,
    VLMO_AUG_ROTATE = 9,        /* a = cos, b = sin of the counter-clockwise angle */
    VLMO_AUG_SOLARIZE = 10,     /* a = threshold */
    VLMO_AUG_POSTERIZE = 11,    /* a = bits kept, an integer in [0, 8] */
    VLMO_AUG_CONTRAST = 12      /* a = factor */
};
#define VLMO_AUG_MAX_SLOTS 4        /* operations per image */
#define VLMO_AUG_MAX_IMAGES 65536   /* images per call */
#define VLMO_AUG_MAX_SHIFT 1000000  /* |shear factor|, |translate offset| */

/* One operation of one image; unused arguments are 0. */
typedef struct {
    int32_t op, pad_;
    double a, b;
} VlmoAugSlot;

/* Bytes of the workspace of vlmo_randaug for n_images: 32-bit histograms and byte tables, [n_images][3][256] each. */
int64_t vlmo_randaug_ws_bytes(int n_images);
/* Applies slots[i * n_slots + s], s = 0 .. n_slots - 1 in order, to image i of the packed buffer src; every operation keeps
 * H x W, so the result has src's layout.  The result is in `out` after the call; `scratch` (NULL allowed for n_slots = 1)
 * takes the intermediate batches, because a warp and the 3 x 3 filter cannot run in place; src is only read.  The three
 * buffers are nbytes long each, 4-byte aligned, nbytes a multiple of 4, and do not overlap; only the bytes of the images
 * are written.  DESIGN.md 4i defines every operation: table look-ups (tables built on the device from 32-bit integer
 * histograms; fp64, Brightness fp32, no fused multiply-add), PIL's Sharpness (borders copied, result clamped), affine warps
 * with fp64 bilinear sampling where a tap outside the image reads `fill`.
 * images / slots: HOST tables, checked here; images_dev / slots_dev: the same tables in device memory.  ws: device
 * workspace, 16-byte aligned, at least vlmo_randaug_ws_bytes(n_images) bytes.
 * Launches per call depend on n_slots alone (at most a memset and three kernels per slot); no device-to-host read.
 * Limits: 3 channels; 1 <= H, W <= VLMO_CROP_MAX_SIDE; images do not overlap; 1 <= n_images <= VLMO_AUG_MAX_IMAGES;
 * 1 <= n_slots <= VLMO_AUG_MAX_SLOTS; 0 <= fill <= 255; arguments finite.  Integer histogram sums and no arithmetic that
 * depends on the position of an image in the table: the same bits from run to run and for any order of the images. */
int vlmo_randaug(const uint8_t* src, uint8_t* out, uint8_t* scratch, int64_t nbytes, const VlmoImage* images,
                 const VlmoImage* images_dev, int n_images, const VlmoAugSlot* slots, const VlmoAugSlot* slots_dev,
                 int n_slots, int fill, void* ws, int64_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VLMO_HIP_H */
