// Relevance propagation over the depth (Chefer et al.'s rule and attention rollout, attnmap.py): one step of the row form
//   x_out[s, r, c0 + j] = alpha * x_in[s, r, c0 + j] + beta * sum_{k < n} x_in[s, r, c0 + k] * A[s, k, j]
// for every sequence s, with A the head-mean map [n, n] of a layer and x the nq relevance rows carried from the top layer
// downward.  Entry point vlmo_relevance_step:
//   relevance_step_kernel   a workgroup (4 waves) owns a 64 x 64 tile of x_out[s]; wave w the 32 x 32 quarter (w >> 1, w & 1)
//                           on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation).  Per 16 values of k a [64 rows x
//                           16 k] piece of x_in and a [16 k x 64 columns] piece of A are staged through LDS, double-buffered
//                           with the next piece's global loads in flight under the MFMAs.  Rows of x are the MFMA's A
//                           operand and columns of A its B operand, so register i of a lane is output row
//                           (i & 3) + 8 (i >> 2) + 4 (lane >> 5), column lane & 31: a register is stored as two 128-byte
//                           row segments.
// Summation order: an output element is ONE chain of MFMAs over k = 0 .. 16 ceil(n / 16) - 1 (k = 8 t + m and 8 t + 4 + m in
// step m of group t; k >= n contributes exact zeros), whatever the grid: no split over k, no atomics, no workspace -- two runs
// give the same bits.  Every global load is guarded by nq and n (a missing element is 0) and every store by nq and n:
// nothing past A + num_seq n^2 is read, nothing outside columns [c0, c0 + n) of rows [0, nq) is written.  Rows of x may
// start at any 4-byte boundary (width and c0 are arbitrary), so global accesses are one float per lane, 64 consecutive
// floats (A) or four 16-float row pieces (x) per wave instruction.
#include <cmath>
#include <stddef.h>

#include "common.h"
#include "vlmo_hip.h"

namespace {

constexpr int TR = 64;          // rows of x per workgroup
constexpr int TC = 64;          // columns of A per workgroup
constexpr int KC = 16;          // values of k per LDS piece
constexpr int XP = KC + 4;      // pitch of the x piece [TR][XP]: 16 consecutive rows start on 16 different 16-byte slots
constexpr int AP = TC + 8;      // pitch of the A piece [KC][AP]: rows k and k + 4 (the two lane halves) are 32 banks apart
constexpr int BUF = TR * XP + KC * AP;
constexpr int N_MAX = 1024;

__global__ __launch_bounds__(256) void relevance_step_kernel(const float* __restrict__ A, const float* __restrict__ x_in,
                                                             float* __restrict__ x_out, int num_seq, int nq, int width,
                                                             int c0, int n, float alpha, float beta) {
    __shared__ __attribute__((aligned(16))) float lds[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, h = lane >> 5;
    const int ctiles = (n + TC - 1) / TC;
    const int rt = blockIdx.x / ctiles, ct = blockIdx.x - rt * ctiles;
    const int r0 = rt * TR, j0 = ct * TC;
    const int nchunk = (n + KC - 1) / KC;
    // loader: element e of thread t is x row (t >> 4) + 16 e, k = t & 15 and A row k = (t >> 6) + 4 e, column t & 63
    const int xr = tid >> 4, xk = tid & 15;
    const int ak = tid >> 6, aj = tid & 63;

    for (int s = blockIdx.y; s < num_seq; s += gridDim.y) {
        const float* As = A + (size_t)s * n * n;
        const float* xs = x_in + (size_t)s * nq * width + c0;
        float* os = x_out + (size_t)s * nq * width + c0;
        float sx[4], sa[4];
        auto fetch = [&](int it) {
            const int k0 = it * KC;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = r0 + xr + 16 * e, k = k0 + xk;
                sx[e] = (r < nq && k < n) ? xs[(size_t)r * width + k] : 0.f;
                const int ka = k0 + ak + 4 * e, j = j0 + aj;
                sa[e] = (ka < n && j < n) ? As[(size_t)ka * n + j] : 0.f;
            }
        };
        auto stash = [&](int buf) {
            float* b = lds + buf * BUF;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                b[(xr + 16 * e) * XP + xk] = sx[e];
                b[TR * XP + (ak + 4 * e) * AP + aj] = sa[e];
            }
        };
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;

        fetch(0);
        stash(0);
        __syncthreads();
        for (int it = 0; it < nchunk; ++it) {
            const bool more = it + 1 < nchunk;
            if (more) fetch(it + 1);
            const float* xb = lds + (it & 1) * BUF + (wr * 32 + l31) * XP + 4 * h;
            const float* ab = lds + (it & 1) * BUF + TR * XP + 4 * h * AP + wc * 32 + l31;
#pragma unroll
            for (int t = 0; t < KC / 8; ++t) {
                const f32x4 xv = *(const f32x4*)(xb + 8 * t);        // x[row l31][k = 8 t + 4 h + m], m = 0 .. 3
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[m], ab[(8 * t + m) * AP], acc, 0, 0, 0);
            }
            if (more) stash((it + 1) & 1);
            __syncthreads();
        }
        // after the loop's last barrier nobody reads the buffers any more: the next sequence may stash at once
        const int j = j0 + wc * 32 + l31;
        if (j < n) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = r0 + wr * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (r < nq) {
                    const size_t o = (size_t)r * width + j;
                    os[o] = alpha * xs[o] + beta * acc[i];
                }
            }
        }
    }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" int vlmo_relevance_step(const float* A, const float* x_in, float* x_out, int num_seq, int nq, int width, int c0,
                                   int n, float alpha, float beta, hipStream_t stream) {
    VLMO_CHECK_ARG(A && x_in && x_out, "vlmo_relevance_step: null pointer");
    VLMO_CHECK_ARG(num_seq >= 1 && nq >= 1, "vlmo_relevance_step: need num_seq, nq >= 1 (num_seq=%d nq=%d)", num_seq, nq);
    VLMO_CHECK_ARG(n >= 1 && n <= N_MAX, "vlmo_relevance_step: need 1 <= n <= %d (n=%d)", N_MAX, n);
    VLMO_CHECK_ARG(width >= 1 && width <= N_MAX, "vlmo_relevance_step: need 1 <= width <= %d (width=%d)", N_MAX, width);
    VLMO_CHECK_ARG(c0 >= 0 && c0 <= width - n, "vlmo_relevance_step: columns [c0, c0 + n) are not inside the width "
                   "(c0=%d n=%d width=%d)", c0, n, width);
    VLMO_CHECK_ARG(std::isfinite(alpha) && std::isfinite(beta), "vlmo_relevance_step: alpha and beta must be finite (%g, %g)",
                   (double)alpha, (double)beta);
    const size_t xbytes = (size_t)num_seq * nq * width * 4, abytes = (size_t)num_seq * n * n * 4;
    VLMO_CHECK_ARG(!overlap(x_out, xbytes, x_in, xbytes), "vlmo_relevance_step: x_out overlaps x_in (not an in-place step)");
    VLMO_CHECK_ARG(!overlap(x_out, xbytes, A, abytes), "vlmo_relevance_step: x_out overlaps A");
    const int tiles = ((nq + TR - 1) / TR) * ((n + TC - 1) / TC);
    const dim3 grid(tiles, num_seq < 65535 ? num_seq : 65535);
    hipLaunchKernelGGL(relevance_step_kernel, grid, dim3(256), 0, stream, A, x_in, x_out, num_seq, nq, width, c0, n, alpha,
                       beta);
    VLMO_CHECK_LAUNCH("vlmo_relevance_step");
    return 0;
}
