// Fused multi-head softmax attention for VLMo on gfx950 (head_dim 64).
// Reference: Attention.forward, vlmo.py:79-95:
//   attn = softmax((q k^T) * dh^-0.5 + keymask(-inf)) ; dropout ; ctx = attn v
// At 224 px VLMo sequences are short (64 / 197 / 261 tokens), so a whole head's
// K and V sit in LDS (<= 36 KB each) and the scores of a 32-query tile never
// leave registers: no N x N tensor in HBM (the reference materialises [B,h,N,N]
// several times).  Forward: attn_fwd1_kernel (one wave per query tile, key
// tiles one at a time with a lazily rescaled running maximum; up to 256 tokens
// as it is, 257 - 288 in its FRINGE form: eight waves for the eight full query
// tiles, the fringe queries split over them by key tile) and attn_fwd_kernel
// (128-key chunks with an exact running maximum; up to 512).  Backward: attn_bwd1_kernel (single pass; up to 256
// tokens as it is, 257 - 288 in its FRINGE form: eight full tiles + one
// fringe tile).
// Higher resolutions (384 / 480 px: 577 / 901 image tokens, up to 965 fused)
// take the streaming kernels: attn_fwd_long_kernel for launches of 513 - 1024
// tokens, attn_dkdv_long_kernel + attn_dq_long_kernel for 289 - 1024; K / V
// (or Q / dO) pass through a two-slot LDS ring instead of staying resident.
// The launch's max_len picks the kernels; nothing else does.
// attn_map_kernel writes the probabilities themselves to HBM for inspection, beside this path (vlmo_attn_probs), or
// their gradient-weighted form (vlmo_attn_gradcam).
//
// Orientation: scores are computed TRANSPOSED, S^T[key][query] = K . Q^T, so a
// lane owns one query column (softmax reductions are in-register + one
// cross-half shuffle) and the fp32 accumulator tile is directly the B operand
// of the next MFMA (O^T = V^T . P^T) after a bf16 pack; V^T fragments come from
// ds_read_b64_tr_b16.  All four operand images use one dual-use swizzle that
// is bank-conflict free for row reads and transposed reads (tests/ldssim.py).
//
// Packed rows: sequence s = rows [rowA,rowA+lenA) ++ [rowB,rowB+lenB) of the
// [M, 3d] qkv matrix, so text+image fusion needs no concatenated copy.
#include "common.h"
#include "vlmo_hip.h"

namespace {

struct AttnArgs {
    const bf16* qkv;
    const bf16* ctx;      // bwd: forward output
    const bf16* dctx;     // bwd: grad of ctx
    bf16* out;            // fwd: ctx ; bwd: dqkv
    float* lse;
    float* qvsum;        // bwd, optional: [num_seq][2 d] column sums of dq | dv over each sequence's tokens
    const int32_t* seg;
    const int32_t* keymask;
    int lse_stride, heads, d;
    float scale, scale_log2e;
    uint32_t drop_thresh, drop_cmp;     // drop_cmp = thresh << 16: keep <=> att_mix(...) >= drop_cmp
    float inv_keep;
    uint64_t seed;
    int bh0;             // dropout-mask index of the launch's first (sequence, head): a backward launch over a SUFFIX of the
                         // forward launch's sequences regenerates the forward's mask (vlmo.py:93 has one mask per call)
};

#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f

__device__ __forceinline__ int att_off(int row, int ch) {
    return 1024 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

// stage rows [0, NPAD) x 64 columns starting at column `col0` of qkv-like matrix
// into a dual-use image by LDS-DMA (one wave-instruction = 8 rows = 1 KiB)
template <int NWAVES>
__device__ __forceinline__ void stage_image(const bf16* base, int ld, int col0, const int* rowidx, char* img, int ninstr,
                                            int wave, int lane) {
    const int chhi = lane >> 5, rowlo = (lane >> 2) & 7, pc = lane & 3;
    for (int ii = wave; ii < ninstr; ii += NWAVES) {
        const int row = ii * 8 + rowlo;
        const int ch = chhi * 4 + (pc ^ ((row >> 2) & 3));
        glds16(base + (size_t)rowidx[row] * ld + col0 + ch * 8, img + ii * 1024);
    }
}

// ---- attention dropout (vlmo.py:93): counter-based, regenerated in the backward -------------------------------
// keep(seq*heads + head, q, key) <=> top 16 bits of att_mix(c * G + att_key) >= thresh, c = q * 512 + key for a
// sequence of <= 512 tokens (every sequence these resident kernels take; the streaming kernels use q * 1024 + key
// above 512 tokens, see att_stride).  The soft-max arithmetic of these kernels is bound by VALU ISSUE (one wave alone on a SIMD issues
// a vector instruction every 4 cycles; the single-pass backward spends ~2/3 of a step in it), so the hash is as short
// as its use allows: the counter is affine in q and in key (either orientation advances it with ONE add of a
// compile-time constant), one xor-shift + one multiply mix it, and only the TOP half of the product is used -- the
// best-mixed bits, compared as a whole word against thresh << 16 (no field extraction).  5 instructions per element.
#define ATT_G 0x9E3779B1u
#define ATT_G512 ((uint32_t)(512ull * ATT_G))
__device__ __forceinline__ uint32_t att_key(uint64_t seed, int bh) {
    return hash32((uint32_t)seed ^ ((uint32_t)bh * 0x9E3779B9u)) + (uint32_t)(seed >> 32);
}
__device__ __forceinline__ uint32_t att_mix(uint32_t x) {
    x ^= x >> 15;
    x *= 0x7feb352du;
    return x;
}

// B/A operand by row read: rows row_base + (lane&31), features 16*ks + 8*(lane>>5) ..+7
__device__ __forceinline__ bf16x8 row_frag(const char* img, int row_base, int ks, int lane) {
    return *(const bf16x8*)(img + att_off(row_base + (lane & 31), 2 * ks + (lane >> 5)));
}
// A operand by transposed read: operand rows = features cb + (lane&31), k = image rows in
// accumulator order rb + 8*(j>>2) + 4*(lane>>5) + (j&3)
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int rb, int cb, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3, h = lane >> 5;
    const int col = cb + 16 * (g & 1) + 4 * pp;
    const int r0 = rb + 4 * h + q;
    const bf16x4 lo = lds_tr4<bf16>(img + att_off(r0, col >> 3) + (col & 7) * 2);
    const bf16x4 hi = lds_tr4<bf16>(img + att_off(r0 + 8, col >> 3) + (col & 7) * 2);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// Token of a sequence -> row of the packed matrix (the four words of seg: rowA, lenA, rowB, lenB)
struct SeqRows {
    int rowA, lenA, rowB, N;
    __device__ __forceinline__ SeqRows(const int32_t* seg, int sidx)
        : rowA(seg[4 * sidx + 0]), lenA(seg[4 * sidx + 1]), rowB(seg[4 * sidx + 2]), N(seg[4 * sidx + 1] + seg[4 * sidx + 3]) {}
    // lengths clamped to [0, cap] tokens in all; an empty sequence reads row 0 (row(i) = rowA + min(i, -1))
    __device__ __forceinline__ SeqRows(const int32_t* seg, int sidx, int cap)
        : rowA(seg[4 * sidx + 0]), lenA(min(max(seg[4 * sidx + 1], 0), cap)), rowB(seg[4 * sidx + 2]),
          N(lenA + min(max(seg[4 * sidx + 3], 0), cap - lenA)) {
        if (N == 0) rowA = 1;
    }
    __device__ __forceinline__ int row(int tok) const {        // padded tokens read the last real row
        tok = min(tok, N - 1);
        return tok < lenA ? rowA + tok : rowB + (tok - lenA);
    }
};

// additive score bias of key i of a sequence of N tokens, `row` its packed row: -inf on padded and masked keys
__device__ __forceinline__ float key_bias(const int32_t* keymask, int row, int i, int N) {
    return (i < N && (!keymask || keymask[row] != 0)) ? 0.f : -INFINITY;
}

// row table and key bias of the padded tokens [0, npad) of a sequence, in LDS
__device__ __forceinline__ void setup_rows(const SeqRows& sr, const int32_t* keymask, int npad, int* rowidx, float* kbias) {
    for (int i = threadIdx.x; i < npad; i += blockDim.x) {
        const int row = sr.row(i);
        rowidx[i] = row;
        kbias[i] = key_bias(keymask, row, i, sr.N);
    }
}

// zero the dropped scores of an S^T tile; rk = dropout counter base of the lane's first key of the tile.  The tile goes
// in and out by value: written through a reference, hipcc turns the 16 selects into compare chains and a branch.
__device__ __forceinline__ f32x16 drop_tile(f32x16 S, uint32_t rk, uint32_t drop_cmp) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (att_mix(rk + (uint32_t)(8 * g4 + e) * ATT_G) < drop_cmp) S[4 * g4 + e] = 0.f;
    return S;
}

// epilogue of the forwards: the O^T accumulators of query qi (packed row qrow) over the row sum l, as bf16 ctx, and
// the row's log-sum-exp (the kernels keep their reference maximum in different units, so they pass the finished value).
// `a` by value: it names the kernel's own argument block either way, and attn_fwd1_kernel keeps its 112 registers.
__device__ __forceinline__ void store_ctx(const AttnArgs a, const f32x16 (&O)[2], float l, float lse, int bh, int hd,
                                          int qi, int qrow, int h) {
    const float inv = a.inv_keep / l;
    bf16* op = a.out + (size_t)qrow * a.d + hd * 64 + 4 * h;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            bf16x4 o = {(bf16)(O[dt][4 * g4 + 0] * inv), (bf16)(O[dt][4 * g4 + 1] * inv),
                        (bf16)(O[dt][4 * g4 + 2] * inv), (bf16)(O[dt][4 * g4 + 3] * inv)};
            *(bf16x4*)(op + dt * 32 + 8 * g4) = o;
        }
    if (h == 0 && a.lse) a.lse[(size_t)bh * a.lse_stride + qi] = lse;
}

// Keys are swept in chunks of CK*32 = 128 with an exact running max (the chunk's
// scores live in 64 accumulator registers; O is rescaled at most once per chunk).
#define ATT_CK 4
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const AttnArgs a, const int NPAD) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kimg = smem;
    char* Vimg = smem + NPAD * 128;
    float* kbias = (float*)(smem + 2 * NPAD * 128);
    int* rowidx = (int*)(kbias + NPAD);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bh = blockIdx.x, sidx = bh / a.heads, hd = bh % a.heads;
    const int ld = 3 * a.d;
    const SeqRows sr(a.seg, sidx);
    const int N = sr.N;
    setup_rows(sr, a.keymask, NPAD, rowidx, kbias);
    __syncthreads();
    const int nq = (N + 31) >> 5;
    stage_image<4>(a.qkv, ld, a.d + hd * 64, rowidx, Kimg, nq * 4, wave, lane);
    stage_image<4>(a.qkv, ld, 2 * a.d + hd * 64, rowidx, Vimg, nq * 4, wave, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const int l31 = lane & 31, h = lane >> 5;
    const uint32_t akey = att_key(a.seed, bh + a.bh0);
    for (int qt = wave; qt < nq; qt += 4) {
        const int qi = qt * 32 + l31;
        const int qrow = rowidx[qi];
        const uint32_t rq = ((uint32_t)qi * 512u + 4u * h) * ATT_G + akey;     // dropout counter base of this lane
        const bf16* qp = a.qkv + (size_t)qrow * ld + hd * 64 + 8 * h;
        bf16x8 qf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);

        float m_run = -INFINITY, l_run = 0.f;
        f32x16 O[2] = {zero16(), zero16()};
        for (int c0 = 0; c0 < nq; c0 += ATT_CK) {
            f32x16 S[ATT_CK];
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < ATT_CK; ++c) {
                S[c] = zero16();
                const int kt = c0 + c;
                if (kt < nq) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) S[c] = Elem<bf16>::mfma(row_frag(Kimg, kt * 32, s, lane), qf[s], S[c]);
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        const f32x4 kb = *(const f32x4*)(kbias + kt * 32 + 8 * g4 + 4 * h);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float t = S[c][4 * g4 + e] * a.scale_log2e + kb[e];
                            S[c][4 * g4 + e] = t;
                            mx = fmaxf(mx, t);
                        }
                    }
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run, mx);
            const bool dead = (m_new == -INFINITY);            // every key so far is masked
            const float alpha = dead ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);
            float lsum = 0.f;
#pragma unroll
            for (int c = 0; c < ATT_CK; ++c) {
                if (c0 + c < nq) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float p = dead ? 0.f : __builtin_amdgcn_exp2f(S[c][i] - m_new);
                        S[c][i] = p;
                        lsum += p;
                    }
                }
            }
            lsum += __shfl_xor(lsum, 32, 64);
            l_run = l_run * alpha + lsum;
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) O[dt][i] *= alpha;
#pragma unroll
            for (int c = 0; c < ATT_CK; ++c) {
                const int kt = c0 + c;
                if (kt < nq) {
                    if (a.drop_thresh) S[c] = drop_tile(S[c], rq + (uint32_t)(kt * 32) * ATT_G, a.drop_cmp);
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        bf16x8 pf;
#pragma unroll
                        for (int j = 0; j < 8; ++j) pf[j] = (bf16)S[c][8 * s2 + j];
#pragma unroll
                        for (int dt = 0; dt < 2; ++dt)
                            O[dt] = Elem<bf16>::mfma(tr_frag(Vimg, kt * 32 + 16 * s2, dt * 32, lane), pf, O[dt]);
                    }
                }
            }
        }
        if (qi < N) store_ctx(a, O, l_run, (m_run + log2f(l_run)) * LN2, bh, hd, qi, qrow, h);
    }
}

// ---- forward, one wave per query tile (sequences of <= 9 tiles = 288 tokens) ------------------------------------
// The chunked kernel above gives a wave several query tiles in turn (7 tiles over 4 waves at 197 tokens: the last round
// runs one wave short, each tile starts with an exposed global load of its Q rows) and carries 64 score registers per
// chunk, i.e. two waves per SIMD.  Here a workgroup has one wave per query tile (right-sized: 7 waves at 197 tokens,
// 2 at 64; waves past the sequence's last tile of a mixed launch leave after the staging barrier), the Q fragments are
// loaded from global memory before the K / V images are staged, and the key tiles are walked one at a time:
//   * the accumulator of the S^T MFMAs starts at the key bias (0 / -inf), so masking costs no vector instruction;
//   * the running maximum is lazy: the accumulators are rescaled only when some row's maximum grew by more than 2^8
//     since the last rescale (a wave-uniform branch, taken on the first tile and almost never again) -- exp2 arguments
//     stay <= 8, the final division by the row sum cancels the stale reference exactly as in the eager form;
//   * row sums are per half-wave partials, combined once at the end;
//   * the S^T product of tile t + 1 is issued before the soft-max arithmetic of tile t, whose P^T V products run under the
//     next tile's arithmetic: the matrix pipe works while the wave issues vector instructions.
// ~110 registers: four waves per SIMD, two workgroups per CU at 197 tokens.
//
// FRINGE form, launches of 257 - 288 tokens (the fused layers at 64 text tokens: 261).  Nine waves are 576 threads: three
// waves on one SIMD and one workgroup per CU.  Here EIGHT waves run the walk above for query tiles 0 - 7 over all nine
// key tiles, then share the <= 32 fringe queries (tokens 256 ..) by KEY tile:
//   * wave w forms S^T(key tile w, fringe queries), wave 0 key tile 8 as well; the row maxima of the nine tiles meet in
//     LDS (one barrier), so every wave forms p = exp2(c S - c m*) against the FINAL maximum: no rescale, the result is
//     a fixed function of the inputs; the row sums are written per key tile and added in key-tile order;
//   * after dropout (the counter q * 512 + key of the walk, so the backward regenerates the same mask) a lane's packed
//     P^T registers ARE the B operand a lane of the same index needs for O^T += V^T P^T, so they cross LDS lane-linear
//     (16 bytes per lane and half tile: conflict-free ds_write_b128 / ds_read_b128, no transposed layout);
//   * waves 6 and 7, one 32-feature half each, add the nine products in key-tile order.  The P^T tiles take turns in
//     three 2 KB slots (key tiles 0-2, 3-5, 6-8, a barrier pair per group): no fp32 partial O tiles in LDS.
// LDS: the K and V images hold NPAD = ceil(max_len / 8) * 8 rows, not 288; the 4 KB image of the fringe queries shares
// the bytes of the P slots (every wave has its Q fragments in registers before the barrier that precedes the first P
// write).  Key tile 8 reads 288 - NPAD rows past either image: past K lies V, past V lie the fringe Q rows and later
// the P tiles -- finite values of the head's own data under a key bias of -inf (S = -inf, p = 0 exactly).
// 2 * 128 NPAD + 6 KB slots + 3 * 1152 B (key bias, maxima, sums): 77 184 bytes at 261 tokens; two workgroups share a CU
// (163 840 bytes, 4 waves per SIMD at <= 128 registers) up to NPAD = 280, i.e. max_len <= 280; 281 - 288 run one per CU.
// Sequences of <= 256 tokens inside a FRINGE launch run the walk only, bit for bit what a 256-token launch gives them.
#define ATT_F1_SLOTS 6144
template <bool FRINGE>
__global__ __launch_bounds__(FRINGE ? 512 : 576) void attn_fwd1_kernel(const AttnArgs a, const int NPAD) {
    const int IMG = NPAD * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kimg = smem;
    char* Vimg = smem + IMG;
    char* Pbuf = smem + 2 * IMG;                                 // FRINGE: fringe Q image, then the P^T slots
    float* kbias = (float*)(smem + 2 * IMG + (FRINGE ? ATT_F1_SLOTS : 0));

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int bh = blockIdx.x, sidx = bh / a.heads, hd = bh % a.heads;
    const int ld = 3 * a.d;
    const SeqRows sr(a.seg, sidx);
    const int N = sr.N;
    const int nq = (N + 31) >> 5;
    const int l31 = lane & 31, h = lane >> 5;
    const bool active = w < nq;
    const int qi = w * 32 + l31;
    const int qrow = sr.row(qi);
    bf16x8 qf[4];
    if (active) {
        const bf16* qp = a.qkv + (size_t)qrow * ld + hd * 64 + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);
    }
    const int ninstr = FRINGE ? min(nq * 4, NPAD >> 3) : nq * 4;
    for (int ii = w; ii < ninstr; ii += nw) {
        const int chhi = lane >> 5, rowlo = (lane >> 2) & 7, pc = lane & 3;
        const int row = ii * 8 + rowlo;
        const int ch = chhi * 4 + (pc ^ ((row >> 2) & 3));
        const size_t r = (size_t)sr.row(row);
        glds16(a.qkv + r * ld + a.d + hd * 64 + ch * 8, Kimg + ii * 1024);
        glds16(a.qkv + r * ld + 2 * a.d + hd * 64 + ch * 8, Vimg + ii * 1024);
    }
    if (FRINGE && nq == 9 && w < 4) {        // the fringe queries' rows, same image layout (tokens past N: the last row)
        const int chhi = lane >> 5, rowlo = (lane >> 2) & 7, pc = lane & 3;
        const int row = w * 8 + rowlo;
        const int ch = chhi * 4 + (pc ^ ((row >> 2) & 3));
        glds16(a.qkv + (size_t)sr.row(256 + row) * ld + hd * 64 + ch * 8, Pbuf + w * 1024);
    }
    for (int i = threadIdx.x; i < (FRINGE ? 288 : NPAD); i += blockDim.x) {
        kbias[i] = key_bias(a.keymask, sr.row(i), i, N);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) return;

    // LDS addressing as in attn_bwd1_kernel: per-lane offsets once, tile bases as scalars / immediates
    const int xq = (l31 >> 2) & 3;
    const int rf0 = 1024 * (l31 >> 3) + 64 * (l31 & 7) + 16 * (h ^ xq);
    const int rf1 = 1024 * (l31 >> 3) + 64 * (l31 & 7) + 16 * ((2 + h) ^ xq);
    const int tg = (lane >> 4) & 1, tq = (lane >> 2) & 3, tp = lane & 3;
    const int trl = 64 * (4 * h + tq) + 16 * ((2 * tg + (tp >> 1)) ^ h) + 8 * (tp & 1);
    const int trh = 1024 + 64 * (4 * h + tq) + 16 * ((2 * tg + (tp >> 1)) ^ ((2 + h) & 3)) + 8 * (tp & 1);
    auto rfrag = [&](const char* img_rb, int s) -> bf16x8 {
        return *(const bf16x8*)(img_rb + 512 * (s >> 1) + ((s & 1) ? rf1 : rf0));
    };
    auto tfrag = [&](const char* img_rb, int dt) -> bf16x8 {
        const bf16x4 lo = lds_tr4<bf16>(img_rb + 512 * dt + trl);
        const bf16x4 hi = lds_tr4<bf16>(img_rb + 512 * dt + trh);
        return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    auto other_half = [&](float v) -> float {       // the value lane ^ 32 holds (v_permlane32_swap: no LDS round trip)
        const uint32_t u = __builtin_bit_cast(uint32_t, v);
        const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        return __builtin_bit_cast(float, h ? r[0] : r[1]);
    };
    // S^T tile of key tile kt: accumulator = key bias of the rows this lane holds (8 (i >> 2) + 4 h + (i & 3))
    auto s_tile = [&](int kt) -> f32x16 {
        f32x16 acc;
        const float* kb = kbias + kt * 32 + 4 * h;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 v = *(const f32x4*)(kb + 8 * g4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[4 * g4 + e] = v[e];
        }
        const char* kimg = Kimg + 4096 * kt;
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = Elem<bf16>::mfma(rfrag(kimg, s), qf[s], acc);
        return acc;
    };

    const uint32_t akey = att_key(a.seed, bh + a.bh0);
    const uint32_t rq = ((uint32_t)qi * 512u + 4u * h) * ATT_G + akey;
    const float c2 = a.scale_log2e;
    const float thr = 8.f / c2;             // lazy-rescale threshold in raw score units
    float m_run = -INFINITY;                // reference maximum in raw score units
    f32x2 l2 = {0.f, 0.f};                  // this half-wave's partial row sum, two interleaved accumulators (v_pk_add_f32)
    f32x16 O[2] = {zero16(), zero16()};
    // soft-max + dropout of one S^T tile in place, then its P^T V products
    auto consume = [&](f32x16& S, int kt) {
        float mx = fmaxf(fmaxf(S[0], S[1]), S[2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2) mx = fmaxf(fmaxf(mx, S[i]), S[i + 1]);
        mx = fmaxf(mx, S[15]);
        mx = fmaxf(mx, other_half(mx));
        if (__builtin_amdgcn_ballot_w64(mx - m_run > thr)) {
            asm volatile("" ::: "memory");      // a real branch: hipcc otherwise if-converts it into 17 packed multiplies per tile
            const float m_new = fmaxf(m_run, mx);
            const float alpha = (m_run == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f((m_run - m_new) * c2);
            l2 *= alpha;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) O[dt][i] *= alpha;
            m_run = m_new;
        }
        const float msub = (m_run == -INFINITY) ? 0.f : -m_run * c2;
        const f32x2 c2v = {c2, c2}, msv = {msub, msub};
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            const f32x2 t = f32x2{S[i], S[i + 1]} * c2v + msv;      // v_pk_fma_f32
            const f32x2 pr = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
            l2 += pr;
            S[i] = pr[0];
            S[i + 1] = pr[1];
        }
        if (a.drop_thresh) S = drop_tile(S, rq + (uint32_t)(kt * 32) * ATT_G, a.drop_cmp);
        const char* vimg = Vimg + 4096 * kt;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            bf16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (bf16)S[8 * s2 + j];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) O[dt] = Elem<bf16>::mfma(tfrag(vimg + 2048 * s2, dt), pf, O[dt]);
        }
    };
    // two tiles per trip, the S^T buffers alternate (no register copies): the product of the next tile is in flight
    // while the current one is consumed
    f32x16 S0 = s_tile(0), S1;
    for (int kt = 0; kt < nq; kt += 2) {
        if (kt + 1 < nq) S1 = s_tile(kt + 1);
        __builtin_amdgcn_sched_barrier(0);
        consume(S0, kt);
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nq) {
            if (kt + 2 < nq) S0 = s_tile(kt + 2);
            __builtin_amdgcn_sched_barrier(0);
            consume(S1, kt + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const float l_run = l2[0] + l2[1];
    const float l_tot = l_run + other_half(l_run);
    // the reference maximum is in raw score units here
    if (qi < N) store_ctx(a, O, l_tot, (m_run * c2 + log2f(l_tot)) * LN2, bh, hd, qi, qrow, h);

    if constexpr (FRINGE) {
        if (nq < 9) return;                 // the whole workgroup: N <= 256
        float* fmax = kbias + 288;          // [9][32] row maxima of the fringe queries per key tile, raw score units
        float* fsum = fmax + 288;           // [9][32] row sums per key tile
        bf16x8 qF[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) qF[s] = rfrag(Pbuf, s);
        auto s_fringe = [&](int kt) -> f32x16 {
            f32x16 acc;
            const float* kb = kbias + kt * 32 + 4 * h;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 v = *(const f32x4*)(kb + 8 * g4);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * g4 + e] = v[e];
            }
            const char* kimg = Kimg + 4096 * kt;
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = Elem<bf16>::mfma(rfrag(kimg, s), qF[s], acc);
            return acc;
        };
        auto tile_max = [&](const f32x16& S) -> float {
            float mx = S[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) mx = fmaxf(mx, S[i]);
            return fmaxf(mx, other_half(mx));
        };
        const bool two = (w == 0);          // wave 0 takes key tile 8 as well
        f32x16 SA = s_fringe(w), SB = SA;
        if (two) SB = s_fringe(8);
        {
            const float ma = tile_max(SA), mb = tile_max(SB);
            if (h == 0) {
                fmax[w * 32 + l31] = ma;
                if (two) fmax[8 * 32 + l31] = mb;
            }
        }
        __syncthreads();                    // the maxima are complete; every wave holds its fringe Q fragments
        float mstar = fmax[l31];
#pragma unroll
        for (int t = 1; t < 9; ++t) mstar = fmaxf(mstar, fmax[t * 32 + l31]);
        const float msubF = (mstar == -INFINITY) ? 0.f : -mstar * c2;
        const uint32_t rqF = ((uint32_t)(256 + l31) * 512u + 4u * h) * ATT_G + akey;
        // p = exp2(c S - c m*) in place, the tile's row sum to fsum, dropout, bf16 pack: the B operands of the tile
        auto soft_pack = [&](f32x16& S, int kt, bf16x8 (&pf)[2]) {
            float l = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                S[i] = __builtin_amdgcn_exp2f(fmaf(S[i], c2, msubF));
                l += S[i];
            }
            l += other_half(l);
            if (h == 0) fsum[kt * 32 + l31] = l;
            if (a.drop_thresh) S = drop_tile(S, rqF + (uint32_t)(kt * 32) * ATT_G, a.drop_cmp);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[s2][j] = (bf16)S[8 * s2 + j];
        };
        bf16x8 pA[2], pB[2];
        soft_pack(SA, w, pA);
        if (two) soft_pack(SB, 8, pB);
        const int dtF = w & 1;              // waves 6 / 7: features [0, 32) / [32, 64)
        f32x16 OF = zero16();
        for (int g = 0; g < 3; ++g) {
            if (w / 3 == g) {
                *(bf16x8*)(Pbuf + (w % 3) * 2048 + lane * 16) = pA[0];
                *(bf16x8*)(Pbuf + (w % 3) * 2048 + 1024 + lane * 16) = pA[1];
            }
            if (g == 2 && two) {
                *(bf16x8*)(Pbuf + 2 * 2048 + lane * 16) = pB[0];
                *(bf16x8*)(Pbuf + 2 * 2048 + 1024 + lane * 16) = pB[1];
            }
            __syncthreads();
            if (w >= 6) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        const bf16x8 pf = *(const bf16x8*)(Pbuf + j * 2048 + s2 * 1024 + lane * 16);
                        OF = Elem<bf16>::mfma(tfrag(Vimg + 4096 * (3 * g + j) + 2048 * s2, dtF), pf, OF);
                    }
            }
            if (g < 2) __syncthreads();     // the slots are free again
        }
        const int qiF = 256 + l31;
        if (w >= 6 && qiF < N) {
            float l = fsum[l31];
#pragma unroll
            for (int t = 1; t < 9; ++t) l += fsum[t * 32 + l31];
            const float inv = a.inv_keep / l;
            bf16* op = a.out + (size_t)sr.row(qiF) * a.d + hd * 64 + 4 * h + dtF * 32;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                bf16x4 o = {(bf16)(OF[4 * g4 + 0] * inv), (bf16)(OF[4 * g4 + 1] * inv), (bf16)(OF[4 * g4 + 2] * inv),
                            (bf16)(OF[4 * g4 + 3] * inv)};
                *(bf16x4*)(op + 8 * g4) = o;
            }
            if (w == 6 && h == 0 && a.lse) a.lse[(size_t)bh * a.lse_stride + qiF] = (mstar * c2 + log2f(l)) * LN2;
        }
    }
}

// ------------------------------------------------------------------ backward
// Column sums for the qkv-bias gradient (vlmo.py:71-75: q_bias / v_bias; the k third is a constant zero): t[dt][r] holds
// feature dt * 32 + (r & 3) + 8 (r >> 2) + 4 h of the token on lane & 31.  Sum over the wave's 32 tokens (butterfly inside
// each half-wave), scale, and add into acc[64] in LDS; tokens past the sequence carry weight 0.
// inclusive DPP scan over each 32-lane half (gfx9 row_shr / row_bcast15 sequence): lanes 31 and 63 end up with their
// half's total.  Six v_add_f32_dpp; the same sum through __shfl_xor is five ds_bpermute round trips per register and
// made the two reductions of a wave cost more than the 51 MB re-read of dqkv they replace.
__device__ __forceinline__ float half_wave_total(float v) {
    float s_ = v + dpp_mov<0x111, 0xf, 0xf>(v);         // row_shr:1 (lanes without a source read 0)
    s_ += dpp_mov<0x112, 0xf, 0xf>(v);                  // row_shr:2
    s_ += dpp_mov<0x113, 0xf, 0xf>(v);                  // row_shr:3  -> sums of 4
    s_ += dpp_mov<0x114, 0xf, 0xe>(s_);                 // row_shr:4, banks 1-3 -> sums of 8
    s_ += dpp_mov<0x118, 0xf, 0xc>(s_);                 // row_shr:8, banks 2-3 -> lane 15 of a row = the row's total
    s_ += dpp_mov<0x142, 0xa, 0xf>(s_);                 // row_bcast15 into rows 1 and 3 -> lanes 31 / 63 = half totals
    return s_;
}
__device__ __forceinline__ void colsum_tile(const f32x16& t, float w, float scale, float* acc, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = half_wave_total(t[r] * w);
        if ((lane & 31) == 31) atomicAdd(acc + (r & 3) + 8 * (r >> 2) + 4 * h, v * scale);
    }
}
__device__ __forceinline__ void colsum_tiles(const f32x16* t, float w, float scale, float* acc, int lane) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) colsum_tile(t[dt], w, scale, acc + dt * 32, lane);
}

// ------------------------------------------------------------------ backward, single pass
// One workgroup = one (sequence, head); wave w OWNS key tile w (32 keys: its K / V row fragments, dK^T and dV^T
// accumulators) AND the dQ^T accumulators of query tile w.  The nq x nq tile pairs are swept along the diagonals of a
// rotation: in step t wave w works on (query tile (w + t) mod nq, key tile w), so S, dP, P and dS of every pair are
// computed exactly ONCE (the two-phase kernel this one replaced, one item per key tile and one per query tile handed
// out to the waves, computed them in the dK/dV items and again in the dQ items: 28 MFMAs and two passes of soft-max /
// dropout arithmetic per pair instead of 20 and one; DESIGN.md section 5 keeps its numbers).  With the key on the lane
// (S = Q . K^T, rows = queries) the accumulator tiles P and dS are directly the B operands of dV^T += dO^T . P and
// dK^T += Q^T . dS; only dS crosses LDS, once: the wave stores its bf16 tile [key][query] into its slot and, after the
// step's barrier, the owner of that query tile reads it back transposed (ds_read_b64_tr_b16) as the B operand of
// dQ^T += K^T . dS^T.  Slots are double buffered: one barrier per step.
// Row constants ride in as INITIAL accumulators: S starts at -lse / scale and dP at -delta, so p = exp2(c * S' + keybias)
// and dS = p * dP' need no per-element subtraction (cdna guide, attention backward).
// LDS at 256 padded tokens (8 key tiles): Q, dO, K images 3 x 32 KB + 2 x 8 slots of 2 KB + row constants = 132 KB.
__device__ __forceinline__ int slot_off(int k, int q) {
    // [key][query] bf16 tile, 64-byte rows, 8-byte units XOR-swizzled by the key pair: conflict-free for the producer's
    // ds_write_b64 (16 consecutive keys, one unit) and for the consumer's transposed reads (4 keys x 8 units)
    return k * 64 + ((((q >> 2) ^ (k >> 1)) & 7) << 3) + (q & 3) * 2;
}
// One wave per key tile, at most 8 (two per SIMD, 251 registers): a ninth wave would put three on one SIMD, i.e. a
// 168-register budget against 96 accumulator registers + V fragments + the S / dP tiles -- hipcc spills 160-330
// registers there and the N = 261 backward takes 200-450 us instead of 120.  Sequences of 257-288 tokens (the fused
// layers at T = 64: 261) take the FRINGE instantiation instead: eight waves, the rotation over the eight full tiles as
// it is, then the 17 pairs that touch the ninth tile in two more steps whose extra accumulators replace dead values:
//   A  (fringe queries, key tile w) into the wave's own dK / dV, which are then final and stored; dS^T stays in the
//      wave's slot of ring buffer 0
//   B  (query tile w, fringe keys) into the wave's own dQ through its slot of buffer 1 (wave-local), and into PARTIAL
//      dK / dV of the fringe keys in the registers step A freed; wave 0 takes (fringe, fringe) as well
//   fringe dQ: waves 4 and 5, one 32-feature half each, from the nine dS^T slots of buffer 0 and the K image, key tiles
//      in order; fringe dK / dV: the eight partials summed through LDS (over the dead Q / dO images) in a fixed tree.
// Every sum has a fixed order: dq / dk / dv are bitwise reproducible in both forms.  Sequences of <= 256 tokens in a
// FRINGE launch run the rotation only.  LDS at 288 padded tokens: images 3 x 36 KB, 2 x 9 slots, row constants, column
// sums, the 4 KB V image of the fringe keys = 155 520 bytes.  The template keeps the <= 256-token kernel as it was.
// Measured (MI355X, B = 64, 12 heads, dropout 0.1; tools/attn_bench.py): N = 197 78 us (two-phase 94), N = 64 16 us (25).
// Per workgroup at N = 197 (s_memrealtime stamps): 7 us before the first product (165 KB through one CU's vector
// memory path at ~25 GB/s: images + V fragments + the ctx / dctx rows for delta), 13 us in the loop (1.9 us per step:
// the two waves of a SIMD spend it in ~180 + ~180 soft-max / dropout instructions, SQ_ACTIVE_INST_VALU is what bounds
// it, the 40 MFMAs of both hide under it), 2-3 us of stores; one workgroup per CU, so the three phases add.
template <bool FRINGE>
__global__ __launch_bounds__(512) void attn_bwd1_kernel(const AttnArgs a, const int NPAD) {
    const int IMG = NPAD * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qimg = smem;
    char* Dimg = smem + IMG;
    char* Kimg = smem + 2 * IMG;
    const int nt = NPAD >> 5;
    char* slots = smem + 3 * IMG;                           // [2][nt][2048]
    float* kbias = (float*)(slots + 2 * nt * 2048);
    float* nlq = kbias + NPAD;      // -lse / scale per query (-inf on padded queries)
    float* ndl = nlq + NPAD;        // -delta * keep_prob
    float* csum = ndl + NPAD;       // [2][64]: column sums of dq | dv of this (sequence, head)
    char* V8img = (char*)(csum + 128);                      // FRINGE: V of the fringe keys, one 4 KB tile

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int bh = blockIdx.x, sidx = bh / a.heads, hd = bh % a.heads;
    const int ld = 3 * a.d;
    // Prologue with ONE level of dependent loads: the packed row of a token is arithmetic on the sequence's four
    // descriptor words (scalar loads), so the LDS-DMA of the three images, the key mask, the rows of ctx / dctx for
    // delta, the log-sum-exp and this wave's V fragments are all issued together (a row table in LDS first costs two more
    // global round trips and a barrier: 6.4 of the 7.2 us a workgroup spent before its first product).
    const SeqRows sr(a.seg, sidx);
    const int N = sr.N;
    const int nq = (N + 31) >> 5;
    const int nc = FRINGE ? min(nq, 8) : nq;        // tiles of the rotation = waves at work
    for (int ii = w; ii < nq * 4; ii += nw) {
        const int chhi = lane >> 5, rowlo = (lane >> 2) & 7, pc = lane & 3;
        const int row = ii * 8 + rowlo;
        const int ch = chhi * 4 + (pc ^ ((row >> 2) & 3));
        const size_t r = (size_t)sr.row(row);
        glds16(a.qkv + r * ld + hd * 64 + ch * 8, Qimg + ii * 1024);
        glds16(a.qkv + r * ld + a.d + hd * 64 + ch * 8, Kimg + ii * 1024);
        glds16(a.dctx + r * a.d + hd * 64 + ch * 8, Dimg + ii * 1024);
    }
    if (FRINGE && nq > 8 && w >= 4) {       // waves 0-3 staged five rows of instructions above, these four
        const int chhi = lane >> 5, rowlo = (lane >> 2) & 7, pc = lane & 3;
        const int row = 256 + (w - 4) * 8 + rowlo;
        const int ch = chhi * 4 + (pc ^ ((row >> 2) & 3));
        glds16(a.qkv + (size_t)sr.row(row) * ld + 2 * a.d + hd * 64 + ch * 8, V8img + (w - 4) * 1024);
    }
    const int l31 = lane & 31, h = lane >> 5;
    const bool active = w < nc;
    const int ki = w * 32 + l31;
    const int krow = sr.row(ki);
    // row fragments (B operands) of this wave's keys straight from global memory: V has no LDS image at all
    // (K row fragments are re-read from the LDS image each step: held in 16 more registers they spill)
    bf16x8 vf[4];
    if (active) {
        const bf16* kp = a.qkv + (size_t)krow * ld + a.d + hd * 64 + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) vf[s] = *(const bf16x8*)(kp + a.d + 16 * s);
    }
    for (int i = threadIdx.x; i < 128; i += blockDim.x) csum[i] = 0.f;      // a one-tile launch has 64 threads
    const float keep_prob = 1.f / a.inv_keep;
    const float inv_scale = 1.f / a.scale;
    for (int i = threadIdx.x; i < NPAD; i += blockDim.x) {
        float dl = 0.f, lq = INFINITY;
        const int row = sr.row(i);
        const float kb = key_bias(a.keymask, row, i, N);
        if (i < N) {
            const size_t o = (size_t)row * a.d + hd * 64;
            bf16x8 x[8], y[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                x[c] = *(const bf16x8*)(a.ctx + o + 8 * c);
                y[c] = *(const bf16x8*)(a.dctx + o + 8 * c);
            }
            lq = a.lse[(size_t)bh * a.lse_stride + i];
#pragma unroll
            for (int c = 0; c < 8; ++c)
#pragma unroll
                for (int j = 0; j < 8; ++j) dl += (float)x[c][j] * (float)y[c][j];
        }
        kbias[i] = kb;
        ndl[i] = -dl * keep_prob;       // dS = scale * inv_keep * P * (keep * dP - delta * keep_prob)
        nlq[i] = -lq * inv_scale;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    const uint32_t akey = att_key(a.seed, bh + a.bh0);
    const float out_scale = a.scale * a.inv_keep;
    const float c_l2 = a.scale_log2e;
    const float kb_own = kbias[min(ki, NPAD - 1)];
    // dropout counter of (q, ki) = q * 512 + ki: affine in q, so a lane walks its 16 queries of a tile with
    // compile-time constant adds
    const uint32_t rl_own = (uint32_t)ki * ATT_G + akey + (uint32_t)(4 * h) * ATT_G512;
    f32x16 dK[2] = {zero16(), zero16()}, dV[2] = {zero16(), zero16()}, dQ[2] = {zero16(), zero16()};

    // LDS addressing with FOUR per-lane offsets for all image accesses (att_off spelled out for tile-aligned bases: the
    // row base enters as 128 * row (a scalar), the k-step / feature half as immediates), so that the loop does not
    // carry ~50 address registers:
    //   row fragment (rows rb + l31, 16-byte chunk 2 s + h):   img + 128 rb + 512 (s >> 1) + rf[s & 1]
    //   transposed fragment (rows rb + ..., features cb + ...): img + 128 rb + 512 (cb >> 5) + {trl | trh}
    const int xq = (l31 >> 2) & 3;
    const int rf0 = 1024 * (l31 >> 3) + 64 * (l31 & 7) + 16 * (h ^ xq);
    const int rf1 = 1024 * (l31 >> 3) + 64 * (l31 & 7) + 16 * ((2 + h) ^ xq);
    const int tg = (lane >> 4) & 1, tq = (lane >> 2) & 3, tp = lane & 3;
    const int trl = 64 * (4 * h + tq) + 16 * ((2 * tg + (tp >> 1)) ^ h) + 8 * (tp & 1);
    const int trh = 1024 + 64 * (4 * h + tq) + 16 * ((2 * tg + (tp >> 1)) ^ ((2 + h) & 3)) + 8 * (tp & 1);
    // (The lambdas of this kernel are always_inline: the FRINGE form calls the stages from five places, and left as
    // functions they take the accumulator arrays through scratch memory.)
    // img_rb = image + 128 * row base (wave-uniform)
    auto rfrag = [&](const char* img_rb, int s) __attribute__((always_inline)) -> bf16x8 {
        return *(const bf16x8*)(img_rb + 512 * (s >> 1) + ((s & 1) ? rf1 : rf0));
    };
    // img_rb = image + 128 * (row base of the 16-row k-step)
    auto tfrag = [&](const char* img_rb, int dt) __attribute__((always_inline)) -> bf16x8 {
        const bf16x4 lo = lds_tr4<bf16>(img_rb + 512 * dt + trl);
        const bf16x4 hi = lds_tr4<bf16>(img_rb + 512 * dt + trh);
        return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    // slot tile [key][query] (slot_off): the producer's two 8-byte stores per k-step, the consumer's transposed reads
    const int sw0 = slot_off(l31, 4 * h), sw1 = slot_off(l31, 8 + 4 * h);           // k-step 1: + 32 bytes XOR-wise
    const int srl = slot_off(4 * h + tq, 16 * tg + 4 * tp), srh = slot_off(8 + 4 * h + tq, 16 * tg + 4 * tp);
    auto sfrag = [&](const char* slot, int s2) __attribute__((always_inline)) -> bf16x8 {
        const bf16x4 lo = lds_tr4<bf16>(slot + 1024 * s2 + srl);
        const bf16x4 hi = lds_tr4<bf16>(slot + 1024 * s2 + srh);
        return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };

    // One step of a wave = four stages:
    //   sdp   S = Q K^T - lse / scale, dP = dO V^T                      8 MFMAs   (row fragments of Q, dO)
    //   valu  p = exp2(c S + keybias), dropout, dS = p (dP - delta)      ~15 VALU instructions per element; dS -> slot
    //   dvdk  dV^T += dO^T P, dK^T += Q^T dS                             8 MFMAs   (transposed fragments of dO, Q)
    //   dq    dQ^T += K^T dS^T for the query tile this wave owns         4 MFMAs   (behind the step's barrier)
    // Left alone, the compiler issues every LDS read right in front of the MFMA that uses it (the LDS latency is then
    // exposed 20 times per step): operands are fetched a stage ahead and __builtin_amdgcn_sched_barrier(0) keeps the
    // fetch groups where they are written.
    // The two waves of a SIMD (w and w + 4) run the stages in DIFFERENT orders between two barriers, so that one is in
    // its MFMA stages while the other does arithmetic (in lockstep every SIMD alternates between idle matrix pipe and
    // idle vector issue, and all waves queue on the LDS port together):
    //   w <  4:  | dq(t-1) sdp(t) valu(t) dvdk(t)          | barrier t
    //   w >= 4:  | valu(t) dvdk(t) dq(t-1) sdp(t+1)        | barrier t        (sdp(0) in front of the loop)
    // Legal because dq(t-1) only needs barrier t-1 behind it and the slot buffer it reads is rewritten after barrier t.
    bf16x8 qa[4], da[4], pf[2], sf[2];
    f32x16 S, dP;
    auto fetch_a = [&](int qt_) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qa[s] = rfrag(Qimg + qt_ * 4096, s);
            da[s] = rfrag(Dimg + qt_ * 4096, s);
        }
    };
    auto qtile = [&](int t_) __attribute__((always_inline)) {
        int q_ = w + t_;
        return q_ >= nc ? q_ - nc : q_;
    };
    // qa / da hold the fragments of query tile qt; ktile = the K image of the key tile, vfr its V row fragments
    auto stage_sdp = [&](int qt, const char* ktile, const bf16x8 (&vfr)[4]) __attribute__((always_inline)) {
        // the row constant -lse / scale as the initial accumulator of S (dP starts at zero: its row constant -delta
        // is needed as a value by the dropout select anyway, and a second set of initial registers spills)
        dP = zero16();
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 l4 = *(const f32x4*)(nlq + qt * 32 + 8 * g4 + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) S[4 * g4 + e] = l4[e];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            S = Elem<bf16>::mfma(qa[s], rfrag(ktile, s), S);
            dP = Elem<bf16>::mfma(da[s], vfr[s], dP);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // kb / rl: key bias and dropout counter base of the lane's key; dV / dK: the accumulators of that key tile
    auto stage_valu_dvdk = [&](int qt, char* myslot, float kb, uint32_t rl, f32x16 (&dV)[2],
                               f32x16 (&dK)[2]) __attribute__((always_inline)) {
        bf16x8 dtr[2], qtr[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            dtr[dt] = tfrag(Dimg + qt * 4096, dt);
            qtr[dt] = tfrag(Qimg + qt * 4096, dt);
        }
        __builtin_amdgcn_sched_barrier(0);
        // P (after dropout) and dS are packed to bf16 as they are produced: registers 8 s2 .. 8 s2 + 7 of a tile are
        // the fragment of k-step s2 of the products that follow
        if (a.drop_thresh) {
            const uint32_t rqt = rl + (uint32_t)(qt * 32) * ATT_G512;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 nd = *(const f32x4*)(ndl + qt * 32 + 8 * g4 + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g4 + e;
                    const float p = __builtin_amdgcn_exp2f(fmaf(S[i], c_l2, kb));
                    const bool keep = att_mix(rqt + (uint32_t)(8 * g4 + e) * ATT_G512) >= a.drop_cmp;
                    const float pd = keep ? p : 0.f;
                    pf[i >> 3][i & 7] = (bf16)pd;
                    sf[i >> 3][i & 7] = (bf16)fmaf(pd, dP[i], p * nd[e]);      // p * (keep * dP - delta)
                }
            }
        } else {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 nd = *(const f32x4*)(ndl + qt * 32 + 8 * g4 + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g4 + e;
                    const float p = __builtin_amdgcn_exp2f(fmaf(S[i], c_l2, kb));
                    pf[i >> 3][i & 7] = (bf16)p;
                    sf[i >> 3][i & 7] = (bf16)(p * (dP[i] + nd[e]));
                }
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            // dS^T tile for the owner of this query tile: registers 4g .. 4g+3 = queries 8g + 4h .. +3 of key l31
            *(bf16x4*)(myslot + (sw0 ^ (32 * s2))) = bf16x4{sf[s2][0], sf[s2][1], sf[s2][2], sf[s2][3]};
            *(bf16x4*)(myslot + (sw1 ^ (32 * s2))) = bf16x4{sf[s2][4], sf[s2][5], sf[s2][6], sf[s2][7]};
        }
        __builtin_amdgcn_sched_barrier(0);
        // the second k-step's fragments are fetched under the first one's products
        bf16x8 dtr1[2], qtr1[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            dtr1[dt] = tfrag(Dimg + qt * 4096 + 2048, dt);
            qtr1[dt] = tfrag(Qimg + qt * 4096 + 2048, dt);
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            dV[dt] = Elem<bf16>::mfma(dtr[dt], pf[0], dV[dt]);
            dK[dt] = Elem<bf16>::mfma(qtr[dt], sf[0], dK[dt]);
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            dV[dt] = Elem<bf16>::mfma(dtr1[dt], pf[1], dV[dt]);
            dK[dt] = Elem<bf16>::mfma(qtr1[dt], sf[1], dK[dt]);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // dq(t): the wave that worked on query tile w in step t owns key tile wp = (w - t) mod nq.  next_q >= 0: also fetch
    // the row fragments of that query tile (the following sdp stage) under these products
    auto stage_dq_at = [&](const char* slot, const char* ktile, int next_q) __attribute__((always_inline)) {
        bf16x8 ktr[2][2], sb[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            sb[s2] = sfrag(slot, s2);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) ktr[s2][dt] = tfrag(ktile + 2048 * s2, dt);
        }
        if (next_q >= 0) fetch_a(next_q);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) dQ[dt] = Elem<bf16>::mfma(ktr[s2][dt], sb[s2], dQ[dt]);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto stage_dq = [&](int t, int next_q) __attribute__((always_inline)) {
        int wp = w - t;
        if (wp < 0) wp += nc;
        stage_dq_at(slots + ((t & 1) * nt + wp) * 2048, Kimg + wp * 4096, next_q);
    };
    const char* kown = Kimg + w * 4096;
    auto core_sdp = [&](int qt) __attribute__((always_inline)) { stage_sdp(qt, kown, vf); };
    auto core_valu_dvdk = [&](int qt, int t) __attribute__((always_inline)) {
        stage_valu_dvdk(qt, slots + ((t & 1) * nt + w) * 2048, kb_own, rl_own, dV, dK);
    };
    // VALU issue is arbitrated by priority, then age: left alone the younger wave of a SIMD (w >= 4) gets the leftovers of
    // the older one's arithmetic stage and every barrier waits for it (interval 3 900 -> 3 540 cycles with this)
    if (w >= 4) __builtin_amdgcn_s_setprio(1);
    if (!active) {
        for (int t = 0; t < nc; ++t) __syncthreads();
    } else if (w < 4) {
        fetch_a(w);
        for (int t = 0; t < nc; ++t) {
            const int qt = qtile(t);
            core_sdp(qt);
            core_valu_dvdk(qt, t);
            __syncthreads();
            stage_dq(t, t + 1 < nc ? qtile(t + 1) : -1);
        }
    } else {
        fetch_a(w);
        core_sdp(w);
        for (int t = 0; t < nc; ++t) {
            core_valu_dvdk(qtile(t), t);
            if (t > 0) stage_dq(t - 1, -1);
            if (t + 1 < nc) {
                fetch_a(qtile(t + 1));
                core_sdp(qtile(t + 1));
            }
            __syncthreads();
        }
        stage_dq(nc - 1, -1);
    }
    if (FRINGE && nq > 8) {
        // Nine tiles: the rotation above covered the 8 x 8 core pairs with all eight waves; the 17 pairs that touch the
        // fringe tile (tokens 256 ..) follow in two more steps, every pair still computed once.
        // A tile of 32 tokens x 64 features, scaled, to columns col0 .. col0 + 63 of dqkv row `row`
        auto store_tile = [&](const f32x16 (&t)[2], float sc, int row, int col0) __attribute__((always_inline)) {
            bf16* op = a.out + (size_t)row * ld + col0 + hd * 64 + 4 * h;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *(bf16x4*)(op + dt * 32 + 8 * g4) =
                        bf16x4{(bf16)(t[dt][4 * g4 + 0] * sc), (bf16)(t[dt][4 * g4 + 1] * sc),
                               (bf16)(t[dt][4 * g4 + 2] * sc), (bf16)(t[dt][4 * g4 + 3] * sc)};
        };
        // ---- step A: (fringe queries, key tile w).  dS^T stays in slot w of ring buffer 0 (free since the last core
        // barrier) for the dQ of the fringe queries below.  dK / dV of key tile w are then final: out they go.
        fetch_a(8);
        stage_sdp(8, kown, vf);
        stage_valu_dvdk(8, slots + w * 2048, kb_own, rl_own, dV, dK);
        store_tile(dK, out_scale, krow, a.d);
        store_tile(dV, a.inv_keep, krow, 2 * a.d);
        if (a.qvsum) colsum_tiles(dV, 1.f, a.inv_keep, csum + 64, lane);
        dK[0] = zero16(), dK[1] = zero16(), dV[0] = zero16(), dV[1] = zero16();
        __syncthreads();        // ring buffer 1 has been read by the last core dq stage of every wave
        // ---- step B: (query tile w, fringe keys).  dK / dV now hold this wave's PARTIAL sums of the fringe keys; dS^T
        // goes through the wave's own slot of buffer 1 into its dQ (wave-local: LDS executes a wave's accesses in order).
        const int k8 = 256 + l31;
        const char* k8tile = Kimg + 8 * 4096;
        const float kb8 = kbias[k8];
        const uint32_t rl8 = (uint32_t)k8 * ATT_G + akey + (uint32_t)(4 * h) * ATT_G512;
#pragma unroll
        for (int s = 0; s < 4; ++s) vf[s] = rfrag(V8img, s);
        char* slot1 = slots + (nt + w) * 2048;
        fetch_a(w);
        stage_sdp(w, k8tile, vf);
        stage_valu_dvdk(w, slot1, kb8, rl8, dV, dK);
        stage_dq_at(slot1, k8tile, w == 0 ? 8 : -1);
        if (w == 0) {           // the pair (fringe, fringe): its dS^T into the ninth slot of buffer 0
            stage_sdp(8, k8tile, vf);
            stage_valu_dvdk(8, slots + 8 * 2048, kb8, rl8, dV, dK);
        }
        store_tile(dQ, out_scale, krow, 0);
        if (a.qvsum) colsum_tiles(dQ, 1.f, out_scale, csum, lane);
        __syncthreads();        // the Q and dO images are dead, buffer 0 holds dS^T of all nine (fringe query, key tile) pairs
        // ---- the fringe rows.  dK / dV: eight partial tiles summed through LDS in a fixed tree, ((0+4)+(1+5))+(2+6))+(3+7)
        // (16 KB regions over the dead images), wave 0 stores.  dQ: waves 4 and 5 each form one 32-feature half from the
        // nine dS^T slots and the K image, key tiles in order -- no partial sums at all.
        auto put = [&](int region) __attribute__((always_inline)) {
            f32x4* p = (f32x4*)(smem + region * 16384) + lane;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    p[(dt * 4 + g4) * 64] = f32x4{dK[dt][4 * g4], dK[dt][4 * g4 + 1], dK[dt][4 * g4 + 2], dK[dt][4 * g4 + 3]};
                    p[(8 + dt * 4 + g4) * 64] = f32x4{dV[dt][4 * g4], dV[dt][4 * g4 + 1], dV[dt][4 * g4 + 2], dV[dt][4 * g4 + 3]};
                }
        };
        auto add = [&](int region) __attribute__((always_inline)) {
            const f32x4* p = (const f32x4*)(smem + region * 16384) + lane;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const f32x4 uk = p[(dt * 4 + g4) * 64], uv = p[(8 + dt * 4 + g4) * 64];
#pragma unroll
                    for (int e = 0; e < 4; ++e) dK[dt][4 * g4 + e] += uk[e], dV[dt][4 * g4 + e] += uv[e];
                }
        };
        const int row8 = sr.row(k8);
        const float wt8 = k8 < N ? 1.f : 0.f;
        if (w >= 4) put(w - 4);
        if (w == 4 || w == 5) {
            const int dt = w - 4;
            f32x16 acc = zero16();
            for (int k = 0; k < 9; ++k) {
                const char* slot = slots + k * 2048;
                const bf16x8 s0 = sfrag(slot, 0), s1 = sfrag(slot, 1);
                const bf16x8 k0 = tfrag(Kimg + k * 4096, dt), k1 = tfrag(Kimg + k * 4096 + 2048, dt);
                acc = Elem<bf16>::mfma(k0, s0, acc);
                acc = Elem<bf16>::mfma(k1, s1, acc);
            }
            if (k8 < N) {
                bf16* op = a.out + (size_t)row8 * ld + hd * 64 + dt * 32 + 4 * h;
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *(bf16x4*)(op + 8 * g4) =
                        bf16x4{(bf16)(acc[4 * g4 + 0] * out_scale), (bf16)(acc[4 * g4 + 1] * out_scale),
                               (bf16)(acc[4 * g4 + 2] * out_scale), (bf16)(acc[4 * g4 + 3] * out_scale)};
            }
            if (a.qvsum) colsum_tile(acc, wt8, out_scale, csum + dt * 32, lane);
        }
        __syncthreads();
        if (w < 4) add(w);
        if (w >= 1 && w < 4) put(w);
        __syncthreads();
        if (w == 0) {
            add(1), add(2), add(3);
            if (k8 < N) {
                store_tile(dK, out_scale, row8, a.d);
                store_tile(dV, a.inv_keep, row8, 2 * a.d);
            }
            if (a.qvsum) colsum_tiles(dV, wt8, a.inv_keep, csum + 64, lane);
        }
    } else if (active && ki < N) {
        // ki doubles as the query index of the dQ tile this wave owns
        bf16* op = a.out + (size_t)krow * ld + hd * 64 + 4 * h;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                bf16x4 oq = {(bf16)(dQ[dt][4 * g4 + 0] * out_scale), (bf16)(dQ[dt][4 * g4 + 1] * out_scale),
                             (bf16)(dQ[dt][4 * g4 + 2] * out_scale), (bf16)(dQ[dt][4 * g4 + 3] * out_scale)};
                bf16x4 ok = {(bf16)(dK[dt][4 * g4 + 0] * out_scale), (bf16)(dK[dt][4 * g4 + 1] * out_scale),
                             (bf16)(dK[dt][4 * g4 + 2] * out_scale), (bf16)(dK[dt][4 * g4 + 3] * out_scale)};
                bf16x4 ov = {(bf16)(dV[dt][4 * g4 + 0] * a.inv_keep), (bf16)(dV[dt][4 * g4 + 1] * a.inv_keep),
                             (bf16)(dV[dt][4 * g4 + 2] * a.inv_keep), (bf16)(dV[dt][4 * g4 + 3] * a.inv_keep)};
                *(bf16x4*)(op + dt * 32 + 8 * g4) = oq;
                *(bf16x4*)(op + a.d + dt * 32 + 8 * g4) = ok;
                *(bf16x4*)(op + 2 * a.d + dt * 32 + 8 * g4) = ov;
            }
    }
    if (a.qvsum) {
        if (active && !(FRINGE && nq > 8)) {
            const float wt = ki < N ? 1.f : 0.f;
            colsum_tiles(dQ, wt, out_scale, csum, lane);
            colsum_tiles(dV, wt, a.inv_keep, csum + 64, lane);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 128; i += blockDim.x) {
            float* dst = a.qvsum + (size_t)sidx * 2 * a.d + (i >> 6) * a.d + hd * 64 + (i & 63);
            *dst = csum[i];
        }
    }
}

// ------------------------------------------------------------------ streaming kernels, 289 .. 1024 tokens
// The kernels above keep a whole head's operand images resident in LDS (256 B per token forward, ~512 B backward), which
// caps them at 576 / 288 tokens.  The three kernels below stream the swept operand through a two-slot LDS ring instead:
// a chunk = ATT_LCH tiles of 32 tokens x two images (K | V, or Q | dO) = 32 KiB, chunk j + 1 in flight (LDS-DMA) while
// chunk j is consumed, one barrier per chunk.  One workgroup per (sequence, head) of ATT_LW waves; wave w owns tile
// w + ATT_LW r in round r, so the number of rounds follows the sequence's OWN length (the short text sequences of a
// mixed launch take one round of one chunk).  The per-tile arithmetic is that of attn_fwd_kernel / attn_bwd1_kernel
// (scores transposed, key on the lane where the next MFMA wants it).
//   forward   attn_fwd_long_kernel   waves own query tiles, K / V chunks streamed; exact running maximum per chunk
//   backward  attn_dkdv_long_kernel  waves own key tiles, Q / dO chunks streamed: dK, dV, dv column sums
//             attn_dq_long_kernel    waves own query tiles, K / V chunks streamed: dQ, dq column sums
// The two backward kernels write disjoint columns of dqkv and recompute P from lse and delta = rowsum(dO . O) on their
// own: no workspace, no global atomics, and every output element is summed in a fixed order (bitwise reproducible).
// The column sums are folded per wave in registers -> one LDS slot per wave -> summed over the waves in wave order.
#define ATT_LW 8
#define ATT_LCH 4
#define ATT_LBUF (ATT_LCH * 4096)               // one image of one chunk
#define ATT_LMAX 1024                           // longest sequence of the streaming kernels
#define ATT_LDS_FWD (4 * ATT_LBUF + ATT_LMAX * 4)
#define ATT_LDS_BWD (4 * ATT_LBUF + 3 * ATT_LMAX * 4 + ATT_LW * 64 * 4)

// dropout counter stride of a sequence of N tokens: c = q * stride + key.  512 up to 512 tokens (the counter of the
// kernels above, bit for bit), 1024 beyond: collision-free up to 1024 tokens.  Chosen from the sequence's own length,
// not the launch's max_len, so that a backward launch over a subset of a forward launch's sequences regenerates its mask.
__device__ __forceinline__ uint32_t att_stride(int N) { return N > 512 ? 1024u : 512u; }

// LDS-DMA of tiles [t0, t0 + nt) of two 64-column operands into dual-use images ia / ib (tile-local rows: the swizzle of
// att_off depends on the row modulo 32 only)
__device__ __forceinline__ void stage_chunk(const bf16* pa, int lda, const bf16* pb, int ldb, const SeqRows& sr, int t0,
                                            int nt, char* ia, char* ib, int w, int lane) {
    const int chhi = lane >> 5, rowlo = (lane >> 2) & 7, pc = lane & 3;
    for (int ii = w; ii < nt * 4; ii += ATT_LW) {
        const int row = t0 * 32 + ii * 8 + rowlo;
        const int ch = chhi * 4 + (pc ^ ((row >> 2) & 3));
        const size_t r = (size_t)sr.row(row);
        glds16(pa + r * lda + ch * 8, ia + ii * 1024);
        glds16(pb + r * ldb + ch * 8, ib + ii * 1024);
    }
}

// per-wave column sums of 32 tokens x 64 features (t[dt][r] as in colsum_tiles, weight w per lane) added into this wave's
// LDS slot part[64]: one writer per slot, a fixed order of additions
__device__ __forceinline__ void colsum_wave(const f32x16* t, float wt, float* part, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = half_wave_total(t[dt][r] * wt);
            if ((lane & 31) == 31) part[dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] += v;
        }
}

// delta (x keep_prob) and the log2-domain LSE of every query of the sequence (+inf / 0 on padded queries), key bias
__device__ __forceinline__ void bwd_row_constants(const AttnArgs& a, const SeqRows& sr, int bh, int hd, int npad,
                                                  float* lseq, float* delta, float* kbias) {
    const float keep_prob = 1.f / a.inv_keep;
    for (int i = threadIdx.x; i < npad; i += blockDim.x) {
        float dl = 0.f, lq = INFINITY;
        const int row = sr.row(i);
        if (i < sr.N) {
            const size_t o = (size_t)row * a.d + hd * 64;
            bf16x8 x[8], y[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                x[c] = *(const bf16x8*)(a.ctx + o + 8 * c);
                y[c] = *(const bf16x8*)(a.dctx + o + 8 * c);
            }
            lq = a.lse[(size_t)bh * a.lse_stride + i] * LOG2E;
#pragma unroll
            for (int c = 0; c < 8; ++c)
#pragma unroll
                for (int j = 0; j < 8; ++j) dl += (float)x[c][j] * (float)y[c][j];
        }
        delta[i] = dl * keep_prob;
        lseq[i] = lq;
        if (kbias) kbias[i] = key_bias(a.keymask, row, i, sr.N);
    }
}

__global__ __launch_bounds__(512) void attn_fwd_long_kernel(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                  // [2][K | V]
    float* kbias = (float*)(smem + 4 * ATT_LBUF);

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bh = blockIdx.x, sidx = bh / a.heads, hd = bh % a.heads;
    const int ld = 3 * a.d;
    const SeqRows sr(a.seg, sidx);
    const int N = sr.N;
    if (N <= 0) return;
    const int nq = (N + 31) >> 5, nch = (nq + ATT_LCH - 1) / ATT_LCH, nrounds = (nq + ATT_LW - 1) / ATT_LW;
    const bf16* kb0 = a.qkv + a.d + hd * 64;
    const bf16* vb0 = a.qkv + 2 * a.d + hd * 64;
    stage_chunk(kb0, ld, vb0, ld, sr, 0, min(ATT_LCH, nq), ring, ring + ATT_LBUF, w, lane);
    for (int i = threadIdx.x; i < nq * 32; i += blockDim.x) kbias[i] = key_bias(a.keymask, sr.row(i), i, N);

    const int l31 = lane & 31, h = lane >> 5;
    const uint32_t akey = att_key(a.seed, bh + a.bh0);
    const uint32_t stride = att_stride(N);
    int qi = 0, qrow = 0;
    uint32_t rq = 0;
    bf16x8 qf[4];
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 O[2] = {zero16(), zero16()};
    const int nsteps = nrounds * nch;
    for (int j = 0; j < nsteps; ++j) {
        const int rd = j / nch, c = j - rd * nch;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                // chunk j landed; everybody is done with chunk j - 1's slot
        if (j + 1 < nsteps) {
            const int t0 = ((j + 1) % nch) * ATT_LCH;
            char* nb = ring + ((j + 1) & 1) * 2 * ATT_LBUF;
            stage_chunk(kb0, ld, vb0, ld, sr, t0, min(ATT_LCH, nq - t0), nb, nb + ATT_LBUF, w, lane);
        }
        const char* Kc = ring + (j & 1) * 2 * ATT_LBUF;
        const char* Vc = Kc + ATT_LBUF;
        const int qt = rd * ATT_LW + w;
        if (qt >= nq) continue;                         // wave-uniform: no query tile for this wave in this round
        if (c == 0) {
            qi = qt * 32 + l31;
            qrow = sr.row(qi);
            rq = ((uint32_t)qi * stride + 4u * h) * ATT_G + akey;
            const bf16* qp = a.qkv + (size_t)qrow * ld + hd * 64 + 8 * h;
#pragma unroll
            for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);
            m_run = -INFINITY, l_run = 0.f;
            O[0] = zero16(), O[1] = zero16();
        }
        const int c0 = c * ATT_LCH;
        f32x16 S[ATT_LCH];
        float mx = -INFINITY;
#pragma unroll
        for (int cc = 0; cc < ATT_LCH; ++cc) {
            S[cc] = zero16();
            const int kt = c0 + cc;
            if (kt < nq) {
#pragma unroll
                for (int s = 0; s < 4; ++s) S[cc] = Elem<bf16>::mfma(row_frag(Kc, cc * 32, s, lane), qf[s], S[cc]);
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const f32x4 kb = *(const f32x4*)(kbias + kt * 32 + 8 * g4 + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float t = S[cc][4 * g4 + e] * a.scale_log2e + kb[e];
                        S[cc][4 * g4 + e] = t;
                        mx = fmaxf(mx, t);
                    }
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const bool dead = (m_new == -INFINITY);
        const float alpha = dead ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);
        float lsum = 0.f;
#pragma unroll
        for (int cc = 0; cc < ATT_LCH; ++cc) {
            if (c0 + cc < nq) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = dead ? 0.f : __builtin_amdgcn_exp2f(S[cc][i] - m_new);
                    S[cc][i] = p;
                    lsum += p;
                }
            }
        }
        lsum += __shfl_xor(lsum, 32, 64);
        l_run = l_run * alpha + lsum;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) O[dt][i] *= alpha;
#pragma unroll
        for (int cc = 0; cc < ATT_LCH; ++cc) {
            const int kt = c0 + cc;
            if (kt < nq) {
                if (a.drop_thresh) S[cc] = drop_tile(S[cc], rq + (uint32_t)(kt * 32) * ATT_G, a.drop_cmp);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    bf16x8 pf;
#pragma unroll
                    for (int jj = 0; jj < 8; ++jj) pf[jj] = (bf16)S[cc][8 * s2 + jj];
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
                        O[dt] = Elem<bf16>::mfma(tr_frag(Vc, cc * 32 + 16 * s2, dt * 32, lane), pf, O[dt]);
                }
            }
        }
        if (c == nch - 1 && qi < N) store_ctx(a, O, l_run, (m_run + log2f(l_run)) * LN2, bh, hd, qi, qrow, h);
    }
}

// dQ^T[d][q] = sum_k K^T[d][k] dS^T[k][q]: waves own query tiles, K / V chunks streamed
__global__ __launch_bounds__(512) void attn_dq_long_kernel(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                  // [2][K | V]
    float* kbias = (float*)(smem + 4 * ATT_LBUF);
    float* lseq = kbias + ATT_LMAX;
    float* delta = lseq + ATT_LMAX;
    float* part = delta + ATT_LMAX;                     // [ATT_LW][64] column sums of dq

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bh = blockIdx.x, sidx = bh / a.heads, hd = bh % a.heads;
    const int ld = 3 * a.d;
    const SeqRows sr(a.seg, sidx);
    const int N = sr.N;
    if (N <= 0) {
        if (a.qvsum && threadIdx.x < 64) a.qvsum[(size_t)sidx * 2 * a.d + hd * 64 + threadIdx.x] = 0.f;
        return;
    }
    const int nq = (N + 31) >> 5, nch = (nq + ATT_LCH - 1) / ATT_LCH, nrounds = (nq + ATT_LW - 1) / ATT_LW;
    const bf16* kb0 = a.qkv + a.d + hd * 64;
    const bf16* vb0 = a.qkv + 2 * a.d + hd * 64;
    stage_chunk(kb0, ld, vb0, ld, sr, 0, min(ATT_LCH, nq), ring, ring + ATT_LBUF, w, lane);
    bwd_row_constants(a, sr, bh, hd, nq * 32, lseq, delta, kbias);
    for (int i = threadIdx.x; i < ATT_LW * 64; i += blockDim.x) part[i] = 0.f;

    const int l31 = lane & 31, h = lane >> 5;
    const uint32_t akey = att_key(a.seed, bh + a.bh0);
    const uint32_t stride = att_stride(N);
    const float out_scale = a.scale * a.inv_keep;
    int qi = 0;
    uint32_t rq = 0;
    float lq = 0.f, dl = 0.f;
    bf16x8 qf[4], df[4];
    f32x16 dQ[2] = {zero16(), zero16()};
    const int nsteps = nrounds * nch;
    for (int j = 0; j < nsteps; ++j) {
        const int rd = j / nch, c = j - rd * nch;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (j + 1 < nsteps) {
            const int t0 = ((j + 1) % nch) * ATT_LCH;
            char* nb = ring + ((j + 1) & 1) * 2 * ATT_LBUF;
            stage_chunk(kb0, ld, vb0, ld, sr, t0, min(ATT_LCH, nq - t0), nb, nb + ATT_LBUF, w, lane);
        }
        const char* Kc = ring + (j & 1) * 2 * ATT_LBUF;
        const char* Vc = Kc + ATT_LBUF;
        const int qt = rd * ATT_LW + w;
        if (qt >= nq) continue;
        if (c == 0) {
            qi = qt * 32 + l31;
            const size_t qrow = (size_t)sr.row(qi);
            const bf16* qp = a.qkv + qrow * ld + hd * 64 + 8 * h;
            const bf16* dp = a.dctx + qrow * a.d + hd * 64 + 8 * h;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                qf[s] = *(const bf16x8*)(qp + 16 * s);
                df[s] = *(const bf16x8*)(dp + 16 * s);
            }
            lq = lseq[qi], dl = delta[qi];
            rq = ((uint32_t)qi * stride + 4u * h) * ATT_G + akey;
            dQ[0] = zero16(), dQ[1] = zero16();
        }
        const int c0 = c * ATT_LCH;
#pragma unroll
        for (int cc = 0; cc < ATT_LCH; ++cc) {
            const int kt = c0 + cc;
            if (kt >= nq) break;
            f32x16 S = zero16(), dP = zero16();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                S = Elem<bf16>::mfma(row_frag(Kc, cc * 32, s, lane), qf[s], S);
                dP = Elem<bf16>::mfma(row_frag(Vc, cc * 32, s, lane), df[s], dP);
            }
            const uint32_t rk = rq + (uint32_t)(kt * 32) * ATT_G;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 kb = *(const f32x4*)(kbias + kt * 32 + 8 * g4 + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g4 + e;
                    const float p = __builtin_amdgcn_exp2f(S[i] * a.scale_log2e + (kb[e] - lq));
                    bool keep = true;
                    if (a.drop_thresh) keep = att_mix(rk + (uint32_t)(8 * g4 + e) * ATT_G) >= a.drop_cmp;
                    S[i] = p * ((keep ? dP[i] : 0.f) - dl);
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                bf16x8 sf;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) sf[jj] = (bf16)S[8 * s2 + jj];
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    dQ[dt] = Elem<bf16>::mfma(tr_frag(Kc, cc * 32 + 16 * s2, dt * 32, lane), sf, dQ[dt]);
            }
        }
        if (c == nch - 1) {
            if (a.qvsum) colsum_wave(dQ, qi < N ? 1.f : 0.f, part + 64 * w, lane);
            if (qi < N) {
                bf16* op = a.out + (size_t)sr.row(qi) * ld + hd * 64 + 4 * h;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        bf16x4 o = {(bf16)(dQ[dt][4 * g4 + 0] * out_scale), (bf16)(dQ[dt][4 * g4 + 1] * out_scale),
                                    (bf16)(dQ[dt][4 * g4 + 2] * out_scale), (bf16)(dQ[dt][4 * g4 + 3] * out_scale)};
                        *(bf16x4*)(op + dt * 32 + 8 * g4) = o;
                    }
            }
        }
    }
    if (a.qvsum) {
        __syncthreads();
        if (threadIdx.x < 64) {
            float s = 0.f;
            for (int ww = 0; ww < ATT_LW; ++ww) s += part[64 * ww + threadIdx.x];
            a.qvsum[(size_t)sidx * 2 * a.d + hd * 64 + threadIdx.x] = s * out_scale;
        }
    }
}

// dV^T[d][k] = sum_q dO^T[d][q] Pd[q][k], dK^T[d][k] = sum_q Q^T[d][q] dS[q][k]: waves own key tiles, Q / dO chunks
// streamed
__global__ __launch_bounds__(512) void attn_dkdv_long_kernel(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                  // [2][Q | dO]
    float* lseq = (float*)(smem + 4 * ATT_LBUF);
    float* delta = lseq + ATT_LMAX;
    float* part = delta + 2 * ATT_LMAX;                 // [ATT_LW][64] column sums of dv (same layout as the dQ kernel)

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bh = blockIdx.x, sidx = bh / a.heads, hd = bh % a.heads;
    const int ld = 3 * a.d;
    const SeqRows sr(a.seg, sidx);
    const int N = sr.N;
    if (N <= 0) {
        if (a.qvsum && threadIdx.x < 64) a.qvsum[(size_t)sidx * 2 * a.d + a.d + hd * 64 + threadIdx.x] = 0.f;
        return;
    }
    const int nq = (N + 31) >> 5, nch = (nq + ATT_LCH - 1) / ATT_LCH, nrounds = (nq + ATT_LW - 1) / ATT_LW;
    const bf16* qb0 = a.qkv + hd * 64;
    const bf16* db0 = a.dctx + hd * 64;
    stage_chunk(qb0, ld, db0, a.d, sr, 0, min(ATT_LCH, nq), ring, ring + ATT_LBUF, w, lane);
    bwd_row_constants(a, sr, bh, hd, nq * 32, lseq, delta, nullptr);
    for (int i = threadIdx.x; i < ATT_LW * 64; i += blockDim.x) part[i] = 0.f;

    const int l31 = lane & 31, h = lane >> 5;
    const uint32_t akey = att_key(a.seed, bh + a.bh0);
    const uint32_t gs = att_stride(N) * ATT_G;          // counter advance of one query
    const float out_scale = a.scale * a.inv_keep;
    int ki = 0;
    uint32_t rl = 0;
    float kb = 0.f;
    bf16x8 kf[4], vf[4];
    f32x16 dK[2] = {zero16(), zero16()}, dV[2] = {zero16(), zero16()};
    const int nsteps = nrounds * nch;
    for (int j = 0; j < nsteps; ++j) {
        const int rd = j / nch, c = j - rd * nch;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (j + 1 < nsteps) {
            const int t0 = ((j + 1) % nch) * ATT_LCH;
            char* nb = ring + ((j + 1) & 1) * 2 * ATT_LBUF;
            stage_chunk(qb0, ld, db0, a.d, sr, t0, min(ATT_LCH, nq - t0), nb, nb + ATT_LBUF, w, lane);
        }
        const char* Qc = ring + (j & 1) * 2 * ATT_LBUF;
        const char* Dc = Qc + ATT_LBUF;
        const int kt = rd * ATT_LW + w;
        if (kt >= nq) continue;
        if (c == 0) {
            ki = kt * 32 + l31;
            const int krow = sr.row(ki);
            const bf16* kp = a.qkv + (size_t)krow * ld + a.d + hd * 64 + 8 * h;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                kf[s] = *(const bf16x8*)(kp + 16 * s);
                vf[s] = *(const bf16x8*)(kp + a.d + 16 * s);
            }
            kb = key_bias(a.keymask, krow, ki, N);
            rl = (uint32_t)ki * ATT_G + akey + (uint32_t)(4 * h) * gs;
            dK[0] = zero16(), dK[1] = zero16(), dV[0] = zero16(), dV[1] = zero16();
        }
        const int c0 = c * ATT_LCH;
#pragma unroll
        for (int cc = 0; cc < ATT_LCH; ++cc) {
            const int qt = c0 + cc;
            if (qt >= nq) break;
            f32x16 S = zero16(), dP = zero16();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                S = Elem<bf16>::mfma(row_frag(Qc, cc * 32, s, lane), kf[s], S);
                dP = Elem<bf16>::mfma(row_frag(Dc, cc * 32, s, lane), vf[s], dP);
            }
            f32x16 Pd;
            const uint32_t rqt = rl + (uint32_t)(qt * 32) * gs;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int q0 = qt * 32 + 8 * g4 + 4 * h;
                const f32x4 lq = *(const f32x4*)(lseq + q0);
                const f32x4 dl = *(const f32x4*)(delta + q0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g4 + e;
                    const float p = __builtin_amdgcn_exp2f(S[i] * a.scale_log2e + (kb - lq[e]));
                    bool keep = true;
                    if (a.drop_thresh) keep = att_mix(rqt + (uint32_t)(8 * g4 + e) * gs) >= a.drop_cmp;
                    Pd[i] = keep ? p : 0.f;
                    S[i] = p * ((keep ? dP[i] : 0.f) - dl[e]);
                }
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                bf16x8 pf, sf;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    pf[jj] = (bf16)Pd[8 * s2 + jj];
                    sf[jj] = (bf16)S[8 * s2 + jj];
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    dV[dt] = Elem<bf16>::mfma(tr_frag(Dc, cc * 32 + 16 * s2, dt * 32, lane), pf, dV[dt]);
                    dK[dt] = Elem<bf16>::mfma(tr_frag(Qc, cc * 32 + 16 * s2, dt * 32, lane), sf, dK[dt]);
                }
            }
        }
        if (c == nch - 1) {
            if (a.qvsum) colsum_wave(dV, ki < N ? 1.f : 0.f, part + 64 * w, lane);
            if (ki < N) {
                bf16* op = a.out + (size_t)sr.row(ki) * ld + hd * 64 + 4 * h;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) {
                        bf16x4 ok = {(bf16)(dK[dt][4 * g4 + 0] * out_scale), (bf16)(dK[dt][4 * g4 + 1] * out_scale),
                                     (bf16)(dK[dt][4 * g4 + 2] * out_scale), (bf16)(dK[dt][4 * g4 + 3] * out_scale)};
                        bf16x4 ov = {(bf16)(dV[dt][4 * g4 + 0] * a.inv_keep), (bf16)(dV[dt][4 * g4 + 1] * a.inv_keep),
                                     (bf16)(dV[dt][4 * g4 + 2] * a.inv_keep), (bf16)(dV[dt][4 * g4 + 3] * a.inv_keep)};
                        *(bf16x4*)(op + a.d + dt * 32 + 8 * g4) = ok;
                        *(bf16x4*)(op + 2 * a.d + dt * 32 + 8 * g4) = ov;
                    }
            }
        }
    }
    if (a.qvsum) {
        __syncthreads();
        if (threadIdx.x < 64) {
            float s = 0.f;
            for (int ww = 0; ww < ATT_LW; ++ww) s += part[64 * ww + threadIdx.x];
            a.qvsum[(size_t)sidx * 2 * a.d + a.d + hd * 64 + threadIdx.x] = s * a.inv_keep;
        }
    }
}

// ------------------------------------------------------------------ attention maps (vlmo_attn_probs, vlmo_attn_gradcam)
// P = softmax(q k^T * scale + keymask) written to HBM as fp32 [num_seq, heads | 1, nq, seq_len]: the one tensor the
// kernels above exist to avoid, for looking at a trained model.  The kernel is bound by its OUTPUT (4 seq_len^2 bytes per
// sequence and head against 64 multiply-adds per element), so it is laid out for the stores:
//   * S = Q . K^T with the KEY on the lane (Q is the row operand, as in attn_bwd1_kernel): accumulator register i of a
//     lane holds query row 8 (i >> 2) + 4 h + (i & 3), key lane & 31.  One store instruction therefore writes two runs of
//     32 consecutive keys (128 B each) of two output rows.  The forward's transposed tile would scatter 4-byte pieces
//     over 32 rows.  Rows are only 4-byte aligned (seq_len = 261: 1044 B), so the stores are dwords.
//   * two sweeps over the keys instead of an nq x seq_len strip: the first keeps a running (maximum, sum) per lane and
//     register and folds the 32 lanes of a half-wave at the end; the second recomputes S (the same MFMAs, bit for bit)
//     and stores exp2(S c - m) / l.
//   * K of one head stays resident for every length: 1024 tokens x 128 B = 128 KB + 8 KB of key bias and row table of
//     the 160 KB LDS.  One workgroup = one (sequence, head) and a run of query tiles, one tile per wave and round.
//   * head_mean: the workgroup walks the heads in order, restaging K; a lane owns the same output elements for every
//     head, so the mean is a read-add-write of its own stores: no atomics, no workspace, a fixed order of additions.
// Zero rules: masked keys, keys and query rows past the sequence's own length, and rows whose keys are all masked
// (the reference has NaN there) are written as 0.  Lengths in seg are clamped to seq_len: nothing outside out is written.
//
// The two MAP_CAM modes write Grad-CAM on these maps instead: with P taken as a free variable, d score / d P[i, j] =
// G[i, j] = dctx[i, :] . v[j, :] per head (ctx = P v).  That is one more MFMA chain in the second sweep: the dctx rows of
// the query tile are a second row operand held in registers beside q, and V is a second key-row operand beside K, so G
// lands in the accumulator layout of S and the combination
//   kind GRAD: G      ATTN_GRAD: P * G      CAM: P * max(G, 0)
// is stored exactly as the maps are.  G is written only where the definition of P has a non-zero.
//   * MAP_CAM_VRES (seq_len <= 512): K and V of the head both resident, 2 x 64 KB + the 4 KB of key bias and row table.
//   * MAP_CAM_VSTREAM (513 - 1024): K alone takes 128 KB, so the V operand of a key tile (4 x 16 B per lane, the bytes
//     row_frag would read from an image) is streamed from global memory into registers, one tile ahead: the loads of
//     tile kt + 1 are issued before the stores of tile kt.  A wave reads 4 KB of V (L2 hits: the head's V is 128 KB) per
//     4 KB tile it stores, and the stores go to HBM.
struct MapArgs {
    const bf16* qkv;
    const bf16* dctx;       // MAP_CAM modes
    const int32_t* seg;
    const int32_t* keymask;
    float* out;
    int heads, d, seq_len, q0, nq, head_mean, tiles_per_block, kind;        // kind: MAP_CAM modes
    float scale_log2e;
};
enum { MAP_PROBS, MAP_CAM_VRES, MAP_CAM_VSTREAM };
#define ATT_PW 8

template <int MODE>
__global__ __launch_bounds__(64 * ATT_PW) void attn_map_kernel(const MapArgs a, const int NPAD) {
    constexpr bool CAM = MODE != MAP_PROBS, VRES = MODE == MAP_CAM_VRES, VSTREAM = MODE == MAP_CAM_VSTREAM;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kimg = smem;
    char* Vimg = smem + NPAD * 128;                 // VRES only
    float* kbias = (float*)(smem + (VRES ? 2 : 1) * NPAD * 128);
    int* rowidx = (int*)(kbias + NPAD);

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hout = a.head_mean ? 1 : a.heads;
    const int sidx = blockIdx.x / hout, hd0 = blockIdx.x % hout;
    const int nh = a.head_mean ? a.heads : 1;
    const int ld = 3 * a.d;
    const SeqRows sr(a.seg, sidx, a.seq_len);
    const int N = sr.N;
    setup_rows(sr, a.keymask, NPAD, rowidx, kbias);
    __syncthreads();

    const int l31 = lane & 31, h = lane >> 5;
    const int nkt = (N + 31) >> 5;                  // key tiles that hold keys of this sequence
    const int nkt_out = NPAD >> 5;                  // key tiles of the output rows
    const int ntq = (a.nq + 31) >> 5;
    const int t_begin = blockIdx.y * a.tiles_per_block, t_end = min(ntq, t_begin + a.tiles_per_block);
    const float c2 = a.scale_log2e;
    const float inv_heads = 1.f / (float)nh;
    const int kind = a.kind;
    float* out = a.out + (size_t)blockIdx.x * a.nq * a.seq_len;

    for (int hi = 0; hi < nh; ++hi) {
        const int hd = hd0 + hi;
        if (hi) __syncthreads();                    // every wave is done with the previous head's images
        stage_image<ATT_PW>(a.qkv, ld, a.d + hd * 64, rowidx, Kimg, nkt * 4, w, lane);
        if (VRES) stage_image<ATT_PW>(a.qkv, ld, 2 * a.d + hd * 64, rowidx, Vimg, nkt * 4, w, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // the V operand of key tile kt: row_frag of the image, or the same 16 bytes per lane and k-step from global memory
        auto v_frags = [&](int kt, bf16x8* vf) {
            if (VRES) {
#pragma unroll
                for (int s = 0; s < 4; ++s) vf[s] = row_frag(Vimg, kt * 32, s, lane);
            } else {
                const bf16* vp = a.qkv + (size_t)rowidx[kt * 32 + l31] * ld + 2 * a.d + hd * 64 + 8 * h;
#pragma unroll
                for (int s = 0; s < 4; ++s) vf[s] = *(const bf16x8*)(vp + 16 * s);
            }
        };

        for (int qt = t_begin + w; qt < t_end; qt += ATT_PW) {
            const int ql = qt * 32;                 // first row of the tile inside the query window
            const size_t qrow = (size_t)rowidx[min(a.q0 + ql + l31, NPAD - 1)];
            const bf16* qp = a.qkv + qrow * ld + hd * 64 + 8 * h;
            bf16x8 qf[4], df[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);
            if (CAM) {
                const bf16* dp = a.dctx + qrow * a.d + hd * 64 + 8 * h;
#pragma unroll
                for (int s = 0; s < 4; ++s) df[s] = *(const bf16x8*)(dp + 16 * s);
            }

            // sweep 1: running maximum and sum of every row over the keys this lane sees
            f32x16 m, l = zero16();
#pragma unroll
            for (int i = 0; i < 16; ++i) m[i] = -INFINITY;
            for (int kt = 0; kt < nkt; ++kt) {
                f32x16 S = zero16();
#pragma unroll
                for (int s = 0; s < 4; ++s) S = Elem<bf16>::mfma(qf[s], row_frag(Kimg, kt * 32, s, lane), S);
                const float kb = kbias[kt * 32 + l31];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float t = S[i] * c2 + kb;
                    const float mn = fmaxf(m[i], t);
                    const float ms = mn == -INFINITY ? 0.f : mn;
                    l[i] = l[i] * __builtin_amdgcn_exp2f(m[i] - ms) + __builtin_amdgcn_exp2f(t - ms);
                    m[i] = mn;
                }
            }
            // the 32 lanes of a half-wave hold the same 16 rows: fold them (fixed order)
#pragma unroll
            for (int off = 16; off > 0; off >>= 1)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float mo = __shfl_xor(m[i], off, 64), lo = __shfl_xor(l[i], off, 64);
                    const float mn = fmaxf(m[i], mo);
                    const float ms = mn == -INFINITY ? 0.f : mn;
                    l[i] = l[i] * __builtin_amdgcn_exp2f(m[i] - ms) + lo * __builtin_amdgcn_exp2f(mo - ms);
                    m[i] = mn;
                }
            // l becomes the factor of the row (0: the row is written as zeros, in every mode), m its finite reference
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int qi = a.q0 + ql + 8 * (i >> 2) + 4 * h + (i & 3);
                const bool zero = qi >= N || m[i] == -INFINITY;
                l[i] = zero ? 0.f : inv_heads / l[i];
                m[i] = zero ? 0.f : m[i];
            }

            // sweep 2: the same scores again (CAM: and G = dctx . v^T beside them), normalised, combined and stored
            const int rows_left = a.nq - ql - 4 * h;        // row 8 (i >> 2) + (i & 3) of this half is inside the window
            bf16x8 vf[4];
            if (VSTREAM && nkt > 0) v_frags(0, vf);
            for (int kt = 0; kt < nkt_out; ++kt) {
                const int key = kt * 32 + l31;
                const bool has_keys = kt < nkt;             // wave-uniform
                f32x16 S = zero16(), G = zero16();
                float kb = CAM ? -INFINITY : 0.f;
                if (has_keys) {
                    if (VRES) v_frags(kt, vf);
#pragma unroll
                    for (int s = 0; s < 4; ++s) S = Elem<bf16>::mfma(qf[s], row_frag(Kimg, kt * 32, s, lane), S);
                    if (CAM) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) G = Elem<bf16>::mfma(df[s], vf[s], G);
                    }
                    kb = kbias[key];
                    if (VSTREAM && kt + 1 < nkt) v_frags(kt + 1, vf);       // in flight during this tile's stores
                }
                if (key < a.seq_len) {
                    float* op = out + (size_t)(ql + 4 * h) * a.seq_len + key;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int r = 8 * (i >> 2) + (i & 3);
                        if (r < rows_left) {
                            // MAP_PROBS adds the key bias inside the exponent (fma(S, c, kb) - m: two roundings), the
                            // CAM modes test it instead (fma(S, c, -m): one).  Each keeps the bits it has always written.
                            float v = 0.f;
                            if (!CAM) {
                                if (has_keys && l[i] != 0.f) v = __builtin_amdgcn_exp2f(S[i] * c2 + kb - m[i]) * l[i];
                            } else if (kb == 0.f && l[i] != 0.f) {      // a key the definition gives a non-zero P, in a live row
                                const float g = kind == VLMO_GRADCAM_CAM ? fmaxf(G[i], 0.f) : G[i];
                                v = kind == VLMO_GRADCAM_GRAD ? g * inv_heads
                                                              : __builtin_amdgcn_exp2f(S[i] * c2 - m[i]) * l[i] * g;
                            }
                            float* p = op + (size_t)r * a.seq_len;
                            *p = hi ? *p + v : v;
                        }
                    }
                }
            }
        }
    }
}

// Launch with `lds` bytes of dynamic LDS.  Beyond the 64 KB default a kernel's limit has to be raised first, on every
// device it runs on (a process may drive several GPUs): mark[] is the limit set so far for this kernel, per device,
// raised atomically as DeviceOnce does it.
template <auto Kernel, class... Args>
void launch(dim3 grid, int threads, int lds, hipStream_t st, const Args&... args) {
    static int mark[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    int& set = mark[dev & 63];
    int old = __atomic_load_n(&set, __ATOMIC_RELAXED);
    while (lds > std::max(old, 65536))
        if (__atomic_compare_exchange_n(&set, &old, lds, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
            (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            break;
        }
    hipLaunchKernelGGL(Kernel, grid, dim3(threads), lds, st, args...);
}

void launch_map(const MapArgs& a, int gx, int gy, hipStream_t st) {
    const int npad = (a.seq_len + 31) / 32 * 32;
    if (!a.dctx) launch<attn_map_kernel<MAP_PROBS>>(dim3(gx, gy), 64 * ATT_PW, npad * 136, st, a, npad);
    else if (a.seq_len <= 512) launch<attn_map_kernel<MAP_CAM_VRES>>(dim3(gx, gy), 64 * ATT_PW, npad * 264, st, a, npad);
    else launch<attn_map_kernel<MAP_CAM_VSTREAM>>(dim3(gx, gy), 64 * ATT_PW, npad * 136, st, a, npad);
}
void launch_fwd_long(const AttnArgs& a, int nblocks, hipStream_t st) {
    launch<attn_fwd_long_kernel>(dim3(nblocks), 64 * ATT_LW, ATT_LDS_FWD, st, a);
}
void launch_bwd_long(const AttnArgs& a, int nblocks, hipStream_t st) {
    launch<attn_dkdv_long_kernel>(dim3(nblocks), 64 * ATT_LW, ATT_LDS_BWD, st, a);
    launch<attn_dq_long_kernel>(dim3(nblocks), 64 * ATT_LW, ATT_LDS_BWD, st, a);
}
void launch_fwd(const AttnArgs& a, int nt, int nblocks, hipStream_t st) {
    launch<attn_fwd_kernel>(dim3(nblocks), 256, nt * 32 * 256 + nt * 32 * 8, st, a, nt * 32);
}
void launch_fwd1(const AttnArgs& a, int nt, int nblocks, hipStream_t st) {
    launch<attn_fwd1_kernel<false>>(dim3(nblocks), nt * 64, nt * 32 * 256 + nt * 32 * 4, st, a, nt * 32);
}
// 257 - 288 tokens: eight waves, images of ceil(max_len / 8) * 8 rows (attn_fwd1_kernel, FRINGE form)
void launch_fwd1_fringe(const AttnArgs& a, int max_len, int nblocks, hipStream_t st) {
    const int rows = (max_len + 7) / 8 * 8;
    launch<attn_fwd1_kernel<true>>(dim3(nblocks), 512, rows * 256 + ATT_F1_SLOTS + 3 * 288 * 4, st, a, rows);
}
template <bool FRINGE>
int launch_bwd1(const AttnArgs& a, int nt, int nblocks, hipStream_t st) {
    // images Q | dO | K, two rings of nt dS^T slots, row constants, column sums; FRINGE: + the V tile of the fringe keys
    const int LDS = nt * 32 * 384 + 2 * nt * 2048 + nt * 32 * 12 + 512 + (FRINGE ? 4096 : 0);
    if (LDS > 160 * 1024) return -1;
    launch<attn_bwd1_kernel<FRINGE>>(dim3(nblocks), (FRINGE ? 8 : nt) * 64, LDS, st, a, nt * 32);
    return 0;
}

int check_common(const char* fn, const void* qkv, const int32_t* seg, int num_seq, int heads, int d, int max_len,
                 int cap) {
    VLMO_CHECK_ARG(qkv && seg, "%s: null pointer", fn);
    VLMO_CHECK_ARG(num_seq > 0 && heads > 0, "%s: empty problem", fn);
    VLMO_CHECK_ARG(d == heads * 64, "%s: head_dim must be 64 (d=%d, heads=%d)", fn, d, heads);
    VLMO_CHECK_ARG(max_len > 0 && max_len <= cap, "%s: sequence length %d exceeds this build's limit %d", fn, max_len, cap);
    return 0;
}

// the arguments vlmo_attn_fwd and vlmo_attn_bwd share; the tensors that differ are left to the caller
AttnArgs make_args(const void* qkv, const int32_t* seg, const int32_t* keymask, const float* lse, int lse_stride, int heads,
                   int d, float scale, uint32_t drop_thresh, float inv_keep, uint64_t seed, int mask_seq0) {
    AttnArgs a{};
    a.qkv = (const bf16*)qkv;
    a.lse = (float*)lse;
    a.seg = seg;
    a.keymask = keymask;
    a.lse_stride = lse_stride;
    a.heads = heads;
    a.d = d;
    a.scale = scale;
    a.scale_log2e = scale * LOG2E;
    a.drop_thresh = drop_thresh;
    a.drop_cmp = drop_thresh >= 65536u ? 0xFFFFFFFFu : drop_thresh << 16;
    a.inv_keep = drop_thresh ? inv_keep : 1.f;
    a.seed = seed;
    a.bh0 = mask_seq0 * heads;
    return a;
}

// vlmo_attn_probs (dctx null, kind unused) and vlmo_attn_gradcam, behind the checks of their own arguments
int run_map(const char* fn, const void* qkv, const void* dctx, const int32_t* seg, int num_seq, const int32_t* keymask,
            float* out, int heads, int d, int seq_len, int q0, int nq, int kind, int head_mean, float scale,
            hipStream_t stream) {
    if (int rc = check_common(fn, qkv, seg, num_seq, heads, d, seq_len, ATT_LMAX)) return rc;
    VLMO_CHECK_ARG(q0 >= 0 && nq >= 1 && q0 <= seq_len - nq, "%s: query rows [%d, %d + %d) outside [0, %d)", fn, q0, q0, nq,
                   seq_len);
    MapArgs a{};
    a.qkv = (const bf16*)qkv;
    a.dctx = (const bf16*)dctx;
    a.seg = seg;
    a.keymask = keymask;
    a.out = out;
    a.heads = heads;
    a.d = d;
    a.seq_len = seq_len;
    a.q0 = q0;
    a.nq = nq;
    a.kind = kind;
    a.head_mean = head_mean != 0;
    a.scale_log2e = scale * LOG2E;
    // one query tile per wave and round; the query tiles of a (sequence, head) are split over workgroups only while
    // that adds workgroups the chip has room for (each one stages the head's images again)
    const int gx = num_seq * (a.head_mean ? 1 : heads);
    const int rounds = ((nq + 31) / 32 + ATT_PW - 1) / ATT_PW;
    const int gy = std::min(rounds, std::max(1, (768 + gx - 1) / gx));
    a.tiles_per_block = ATT_PW * ((rounds + gy - 1) / gy);
    launch_map(a, gx, (rounds * ATT_PW + a.tiles_per_block - 1) / a.tiles_per_block, stream);
    VLMO_CHECK_LAUNCH(fn);
    return 0;
}

}  // namespace

extern "C" int vlmo_attn_fwd(const void* qkv, const int32_t* seg, int num_seq, const int32_t* keymask, void* ctx,
                             float* lse, int lse_stride, int heads, int d, int max_len, float scale,
                             uint32_t drop_thresh, float inv_keep, uint64_t seed, int mask_seq0, hipStream_t stream) {
    if (int rc = check_common("vlmo_attn_fwd", qkv, seg, num_seq, heads, d, max_len, 1024)) return rc;
    VLMO_CHECK_ARG(ctx, "vlmo_attn_fwd: null ctx");
    VLMO_CHECK_ARG(!lse || lse_stride >= max_len, "vlmo_attn_fwd: lse_stride too small");
    AttnArgs a = make_args(qkv, seg, keymask, lse, lse_stride, heads, d, scale, drop_thresh, inv_keep, seed, mask_seq0);
    a.out = (bf16*)ctx;
    const int nt = (max_len + 31) / 32, nb = num_seq * heads;
    if (max_len > 512) {        // 513 .. 1024 tokens: K / V streamed (the resident kernels' 512-token dropout counter ends here)
        launch_fwd_long(a, nb, stream);
        VLMO_CHECK_LAUNCH("vlmo_attn_fwd(long)");
        return 0;
    }
    if (nt == 9) launch_fwd1_fringe(a, max_len, nb, stream);
    else if (nt < 9) launch_fwd1(a, nt, nb, stream);
    else launch_fwd(a, nt, nb, stream);
    VLMO_CHECK_LAUNCH("vlmo_attn_fwd");
    return 0;
}

extern "C" int vlmo_attn_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, int lse_stride,
                             const int32_t* seg, int num_seq, const int32_t* keymask, void* dqkv, float* qv_colsum,
                             int heads, int d, int max_len, float scale, uint32_t drop_thresh, float inv_keep,
                             uint64_t seed, int mask_seq0, hipStream_t stream) {
    if (int rc = check_common("vlmo_attn_bwd", qkv, seg, num_seq, heads, d, max_len, 1024)) return rc;
    VLMO_CHECK_ARG(ctx && dctx && lse && dqkv, "vlmo_attn_bwd: null pointer");
    VLMO_CHECK_ARG(lse_stride >= max_len, "vlmo_attn_bwd: lse_stride too small");
    AttnArgs a = make_args(qkv, seg, keymask, lse, lse_stride, heads, d, scale, drop_thresh, inv_keep, seed, mask_seq0);
    a.ctx = (const bf16*)ctx;
    a.dctx = (const bf16*)dctx;
    a.out = (bf16*)dqkv;
    a.qvsum = qv_colsum;
    const int nt = (max_len + 31) / 32, nb = num_seq * heads;
    if (max_len > 288) {        // 289 .. 1024 tokens: the dK/dV and the dQ streaming kernels, back to back
        launch_bwd_long(a, nb, stream);
        VLMO_CHECK_LAUNCH("vlmo_attn_bwd(long)");
        return 0;
    }
    // 257 .. 288: eight owners + the fringe steps for the ninth tile
    const int rc = nt > 8 ? launch_bwd1<true>(a, nt, nb, stream) : launch_bwd1<false>(a, nt, nb, stream);
    VLMO_CHECK_ARG(rc == 0, "vlmo_attn_bwd: %d tokens do not fit the LDS of one CU", max_len);
    VLMO_CHECK_LAUNCH("vlmo_attn_bwd");
    return 0;
}

extern "C" int vlmo_attn_probs(const void* qkv, const int32_t* seg, int num_seq, const int32_t* keymask, float* probs,
                               int heads, int d, int seq_len, int q0, int nq, int head_mean, float scale,
                               hipStream_t stream) {
    VLMO_CHECK_ARG(probs, "vlmo_attn_probs: null probs");
    return run_map("vlmo_attn_probs", qkv, nullptr, seg, num_seq, keymask, probs, heads, d, seq_len, q0, nq, 0, head_mean,
                   scale, stream);
}

extern "C" int vlmo_attn_gradcam(const void* qkv, const void* dctx, const int32_t* seg, int num_seq, const int32_t* keymask,
                                 float* out, int heads, int d, int seq_len, int q0, int nq, int kind, int head_mean,
                                 float scale, hipStream_t stream) {
    VLMO_CHECK_ARG(dctx && out, "vlmo_attn_gradcam: null dctx or out");
    VLMO_CHECK_ARG(kind == VLMO_GRADCAM_CAM || kind == VLMO_GRADCAM_ATTN_GRAD || kind == VLMO_GRADCAM_GRAD,
                   "vlmo_attn_gradcam: unknown kind %d", kind);
    return run_map("vlmo_attn_gradcam", qkv, dctx, seg, num_seq, keymask, out, heads, d, seq_len, q0, nq, kind, head_mean,
                   scale, stream);
}
