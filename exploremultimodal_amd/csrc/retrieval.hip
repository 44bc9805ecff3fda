// Retrieval ranking: for every query row the K best gallery rows under score(q, g) = scale * <Q[q], G[g]>, without the
// [Nq, Ng] score matrix in HBM (what `(t_feat @ i_feat.t()).topk(k)` writes and reads back).  Entry point vlmo_sim_topk:
//   sim_topk_kernel   a workgroup (4 waves) owns 128 query rows and one contiguous slice of the gallery.  Per 128 gallery
//                     rows the score tile is built on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation) from
//                     16-column chunks of Q and G staged through LDS, double-buffered.  Gallery rows are the MFMA's A
//                     operand and query rows its B operand, so a lane holds 16 scores of ONE query per tile and keeps
//                     that query's running list of K (value, index) pairs in registers: a score is compared with the
//                     list's last value first and inserted only when it beats it.  The lists of the two lane halves and
//                     of the two waves that share a query are merged at the end of the slice.
//   sim_topk_merge_kernel   splits > 1: one thread per query folds the per-slice lists [Nq, splits, K] in split order.
// Order: higher score first, lower gallery index first among equal scores -- a total order, so the result does not depend
// on how the gallery is cut.  A score is one chain of MFMAs over D in a fixed order (columns 8t + m and 8t + 4 + m in
// step m of group t), whatever the tile or the split, and nothing is accumulated with atomics: the output has the same
// bits from run to run and for every split count.
#include <stddef.h>

#include "common.h"
#include "vlmo_hip.h"

namespace {

constexpr int TQ = 128;        // query rows per workgroup
constexpr int TG = 128;        // gallery rows per step
constexpr int DC = 16;         // columns of Q / G per LDS chunk
constexpr int PITCH = DC + 4;  // LDS row pitch in floats: 16 consecutive rows start on 16 different 16-byte slots
constexpr int TOPK_MAX = 16;
constexpr int D_MAX = 1024;
constexpr int TARGET_WG = 512;   // two workgroups per compute unit
constexpr int MAX_SPLITS = 32;

__device__ __forceinline__ bool ranks_before(float v, int32_t i, float lv, int32_t li) {
    return v > lv || (v == lv && (uint32_t)i < (uint32_t)li);     // an empty slot (index -1) ranks last
}

// K (value, index) pairs, best first, in registers (every index below is a compile-time constant)
template <int KT> struct TopList {
    float v[KT];
    int32_t i[KT];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            v[k] = -INFINITY;
            i[k] = -1;
        }
    }
    // STREAM: the candidate's index is above every index already in the list, so it enters only on a greater value
    template <bool STREAM> __device__ __forceinline__ void insert(float s, int32_t idx) {
        if (STREAM ? s > v[KT - 1] : ranks_before(s, idx, v[KT - 1], i[KT - 1])) {
            v[KT - 1] = s;
            i[KT - 1] = idx;
#pragma unroll
            for (int k = KT - 1; k > 0; --k) {
                const bool up = STREAM ? v[k] > v[k - 1] : ranks_before(v[k], i[k], v[k - 1], i[k - 1]);
                const float tv = v[k];
                const int32_t ti = i[k];
                v[k] = up ? v[k - 1] : tv;
                i[k] = up ? i[k - 1] : ti;
                v[k - 1] = up ? tv : v[k - 1];
                i[k - 1] = up ? ti : i[k - 1];
            }
        }
    }
};

// 4 columns [c, c + 4) of a row; zeros for a missing row or columns past D (D % 4 == 0: a group is all in or all out)
__device__ __forceinline__ f32x4 load4(const float* row, int c, int D, bool vec) {
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (row && c < D) {
        if (vec) {
            r = *(const f32x4*)(row + c);
        } else {
            r[0] = row[c];
            r[1] = row[c + 1];
            r[2] = row[c + 2];
            r[3] = row[c + 3];
        }
    }
    return r;
}

// out_val / out_idx: [Nq, nsplit, K]
template <int KT>
__global__ __launch_bounds__(256) void sim_topk_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ G,
                                                       int ldg, int Nq, int Ng, int D, int K, float scale, int slice_len,
                                                       int nsplit, int vecq, int vecg, float* __restrict__ out_val,
                                                       int32_t* __restrict__ out_idx) {
    // [buffer][0 = gallery, 1 = query][row][column of the chunk]; reused for the merge of the two gallery waves
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * 128 * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = wave >> 1, wq = wave & 1;          // this wave: gallery rows [64 wg, +64) x query rows [64 wq, +64) of a step
    const int l31 = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * TQ;
    const int split = blockIdx.y;
    const int g_beg = split * slice_len;
    const int g_end = min(Ng, g_beg + slice_len);
    const int nchunk = (D + DC - 1) / DC;
    const int nstep = (g_end - g_beg + TG - 1) / TG;
    const int total = nstep * nchunk;

    // loader: thread t stages rows t / 4 and 64 + t / 4 of both tiles, columns 4 (t % 4) .. + 3 of the chunk
    const int lr = tid >> 2, lc = (tid & 3) * 4;
    const float* qrow[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int q = q0 + lr + 64 * p;
        qrow[p] = q < Nq ? Q + (size_t)q * ldq : nullptr;
    }
    f32x4 stage[4];
    auto fetch = [&](int it) {
        const int step = it / nchunk, c = (it - step * nchunk) * DC + lc;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int g = g_beg + step * TG + lr + 64 * p;
            stage[p] = load4(g < g_end ? G + (size_t)g * ldg : nullptr, c, D, vecg);
            stage[2 + p] = load4(qrow[p], c, D, vecq);
        }
    };
    auto stash = [&](int buf) {
        float* b = lds + buf * (2 * 128 * PITCH);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            *(f32x4*)(b + (lr + 64 * p) * PITCH + lc) = stage[p];
            *(f32x4*)(b + (128 + lr + 64 * p) * PITCH + lc) = stage[2 + p];
        }
    };

    TopList<KT> top[2];
    top[0].init();
    top[1].init();
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    if (total > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    int chunk = 0, g0 = g_beg;
    for (int it = 0; it < total; ++it) {
        const bool more = it + 1 < total;
        if (more) fetch(it + 1);
        const float* gb = lds + (it & 1) * (2 * 128 * PITCH) + (wg * 64 + l31) * PITCH + 4 * h;
        const float* qb = lds + (it & 1) * (2 * 128 * PITCH) + (128 + wq * 64 + l31) * PITCH + 4 * h;
#pragma unroll
        for (int t = 0; t < DC / 8; ++t) {
            const f32x4 a0 = *(const f32x4*)(gb + 8 * t), a1 = *(const f32x4*)(gb + 32 * PITCH + 8 * t);
            const f32x4 b0 = *(const f32x4*)(qb + 8 * t), b1 = *(const f32x4*)(qb + 32 * PITCH + 8 * t);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[m], b0[m], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[m], b1[m], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[m], b0[m], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[m], b1[m], acc[1][1], 0, 0, 0);
            }
        }
        if (++chunk == nchunk) {
            // lane: query column l31 of query tile b; register r of gallery tile a is gallery row
            // g0 + 64 wg + 32 a + (r & 3) + 8 (r >> 2) + 4 h -- ascending in (a, r), as insert<true> needs
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int g = g0 + wg * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        const float s = g < g_end ? scale * acc[a][b][r] : -INFINITY;
                        top[b].template insert<true>(s, g);
                        acc[a][b][r] = 0.f;
                    }
            chunk = 0;
            g0 += TG;
        }
        if (more) stash((it + 1) & 1);
        __syncthreads();
    }

    // lanes l and l + 32 hold lists of the same query over different gallery rows: the upper half's go into the lower's
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const float ov = __shfl(top[b].v[k], l31 + 32, 64);
            const int32_t oi = __shfl(top[b].i[k], l31 + 32, 64);
            if (h == 0) top[b].template insert<false>(ov, oi);
        }
    // the wave of gallery rows [64, 128) hands its lists to the wave of rows [0, 64) through LDS: [k][query of the tile]
    float* mv = lds;
    int32_t* mi = (int32_t*)(lds + KT * TQ);
    if (wg == 1 && h == 0)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                mv[k * TQ + wq * 64 + b * 32 + l31] = top[b].v[k];
                mi[k * TQ + wq * 64 + b * 32 + l31] = top[b].i[k];
            }
    __syncthreads();
    if (wg == 0 && h == 0)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ql = wq * 64 + b * 32 + l31;
#pragma unroll
            for (int k = 0; k < KT; ++k) top[b].template insert<false>(mv[k * TQ + ql], mi[k * TQ + ql]);
            const int q = q0 + ql;
            if (q < Nq) {
                const size_t o = ((size_t)q * nsplit + split) * K;
#pragma unroll
                for (int k = 0; k < KT; ++k)
                    if (k < K) {
                        out_val[o + k] = top[b].v[k];
                        out_idx[o + k] = top[b].i[k];
                    }
            }
        }
}

// pv / pi [Nq, nsplit, K] -> out [Nq, K]; the lists of a query are folded in split order
template <int KT>
__global__ __launch_bounds__(256) void sim_topk_merge_kernel(const float* __restrict__ pv, const int32_t* __restrict__ pi,
                                                             int Nq, int nsplit, int K, float* __restrict__ out_val,
                                                             int32_t* __restrict__ out_idx) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Nq) return;
    TopList<KT> top;
    top.init();
    for (int s = 0; s < nsplit; ++s) {
        const size_t o = ((size_t)q * nsplit + s) * K;
        for (int k = 0; k < K; ++k) {
            const float v = pv[o + k];
            const int32_t i = pi[o + k];
            if (!ranks_before(v, i, top.v[KT - 1], top.i[KT - 1])) break;      // the rest of this list ranks lower still
            top.template insert<false>(v, i);
        }
    }
#pragma unroll
    for (int k = 0; k < KT; ++k)
        if (k < K) {
            out_val[(size_t)q * K + k] = top.v[k];
            out_idx[(size_t)q * K + k] = top.i[k];
        }
}

int cdiv(int a, int b) { return (a + b - 1) / b; }

// the gallery in slices of whole 128-row steps -> number of slices; splits <= 0: enough workgroups to fill the chip
int topk_slices(int Nq, int Ng, int splits, int* slice_len) {
    const int g_tiles = cdiv(Ng, TG);
    if (splits <= 0) {
        splits = cdiv(TARGET_WG, cdiv(Nq, TQ));
        splits = splits > MAX_SPLITS ? MAX_SPLITS : splits;
    }
    splits = splits > g_tiles ? g_tiles : splits;
    const int per = cdiv(g_tiles, splits);
    *slice_len = per * TG;
    return cdiv(g_tiles, per);
}

}  // namespace

extern "C" int64_t vlmo_sim_topk_ws_bytes(int Nq, int Ng, int K, int splits) {
    if (Nq < 1 || Ng < 1 || K < 1) return 0;
    int slice_len;
    const int n = topk_slices(Nq, Ng, splits, &slice_len);
    return n <= 1 ? 0 : (int64_t)Nq * n * K * 8;
}

extern "C" int vlmo_sim_topk(const float* Q, int ldq, const float* G, int ldg, int Nq, int Ng, int D, int K, float scale,
                             int splits, void* ws, size_t ws_bytes, float* out_val, int32_t* out_idx, hipStream_t stream) {
    VLMO_CHECK_ARG(Q && G && out_val && out_idx, "vlmo_sim_topk: null pointer");
    VLMO_CHECK_ARG(Nq >= 1 && Ng >= 1, "vlmo_sim_topk: need Nq, Ng >= 1 (Nq=%d Ng=%d)", Nq, Ng);
    VLMO_CHECK_ARG(K >= 1 && K <= TOPK_MAX, "vlmo_sim_topk: need 1 <= K <= %d (K=%d)", TOPK_MAX, K);
    VLMO_CHECK_ARG(D >= 4 && D <= D_MAX && D % 4 == 0, "vlmo_sim_topk: need 4 <= D <= %d, D %% 4 == 0 (D=%d)", D_MAX, D);
    VLMO_CHECK_ARG(ldq >= D && ldg >= D, "vlmo_sim_topk: leading dimensions %d / %d below D=%d", ldq, ldg, D);
    VLMO_CHECK_ARG(scale > 0.f, "vlmo_sim_topk: need scale > 0 (scale=%g)", (double)scale);
    VLMO_CHECK_ARG(splits >= 0, "vlmo_sim_topk: splits must be >= 0 (splits=%d)", splits);
    int slice_len;
    const int nsplit = topk_slices(Nq, Ng, splits, &slice_len);
    const size_t need = nsplit <= 1 ? 0 : (size_t)Nq * nsplit * K * 8;
    VLMO_CHECK_ARG(need == 0 || (ws && ws_bytes >= need), "vlmo_sim_topk: workspace too small (need %llu bytes, got %llu)",
                   (unsigned long long)need, (unsigned long long)(ws ? ws_bytes : 0));
    float* pv = nsplit > 1 ? (float*)ws : out_val;
    int32_t* pi = nsplit > 1 ? (int32_t*)ws + (size_t)Nq * nsplit * K : out_idx;
    // 16-byte loads need aligned rows; any other layout is read one float at a time
    const int vecq = ((uintptr_t)Q % 16 == 0 && ldq % 4 == 0) ? 1 : 0;
    const int vecg = ((uintptr_t)G % 16 == 0 && ldg % 4 == 0) ? 1 : 0;
    const dim3 grid(cdiv(Nq, TQ), nsplit);
    const int mblocks = cdiv(Nq, 256);
#define TOPK_RUN(KT)                                                                                                       \
    do {                                                                                                                   \
        hipLaunchKernelGGL((sim_topk_kernel<KT>), grid, dim3(256), 0, stream, Q, ldq, G, ldg, Nq, Ng, D, K, scale,         \
                           slice_len, nsplit, vecq, vecg, pv, pi);                                                         \
        VLMO_CHECK_LAUNCH("vlmo_sim_topk");                                                                                \
        if (nsplit > 1) {                                                                                                  \
            hipLaunchKernelGGL((sim_topk_merge_kernel<KT>), dim3(mblocks), dim3(256), 0, stream, pv, pi, Nq, nsplit, K,    \
                               out_val, out_idx);                                                                          \
            VLMO_CHECK_LAUNCH("vlmo_sim_topk(merge)");                                                                     \
        }                                                                                                                  \
    } while (0)
    if (K == 1)
        TOPK_RUN(1);
    else if (K <= 5)
        TOPK_RUN(5);
    else if (K <= 10)
        TOPK_RUN(10);
    else
        TOPK_RUN(16);
#undef TOPK_RUN
    return 0;
}
