// ISDA (implicit semantic data augmentation) of the VQA classifier's last Linear (models/vlmo/heads.py:6-83,
// objectives.py:325-344): a per-class diagonal-covariance estimator and the logit correction
//   z_aug[n, j] = z[n, j] + s * sum_a (W[j, a] - W[k_n, a])^2 * cov[k_n, a]            (s = ratio / 2)
// without the reference's [B, vs, A] intermediates.  Entry points:
//   isda_update    one wave per class: member rows (targets != 0) in ascending order, their mean and population variance
//                  over the features, the count-weighted blend into (count, mean, cov) in place; classes without a
//                  member leave at once (bitwise unchanged).  Extra waves give k_n = first arg-max of each target row.
//                  The features are recomputed from the pre-LayerNorm rows (the fp32 values of ln_gelu_fwd) or read as
//                  given.
//   isda_aug_fwd   fp32 tiles of 64 rows x 64 classes reduced over A in 16-wide LDS chunks, split over A into fixed
//                  segments (partial slabs), then folded in segment order into z (pad columns untouched)
//   isda_aug_bwd   R[n, a] = sum_j G[n, j] (W[j, a] - W[k_n, a]) in partial slabs over j; then per (j, a) of dW
//                  + r sum_n G[n, j] (W[j, a] - W[k_n, a]) ck[n, a] - r sum_{n: k_n = j} ck[n, a] R[n, a]
//                  added to the fp32 accumulator (each element owned by one thread; rows summed in ascending order)
// No float atomics anywhere: two runs give the same bits.
#include "common.h"
#include "vlmo_hip.h"

namespace {

constexpr int ISDA_MAX_A = 2048;
constexpr int T64 = 64;      // rows / classes / columns per tile edge
constexpr int KC = 16;       // reduction chunk staged in LDS
constexpr int LDT = T64 + 4; // LDS row pitch (floats): breaks the 256-byte row stride
constexpr int TARGET_WG = 512;

__device__ __forceinline__ float isda_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

// feature a of row n: GELU(LayerNorm(u[n]) * g + b) when g is given (the arithmetic of ln_gelu_fwd), else u[n, a]
__device__ __forceinline__ f32x4 isda_feat4(const float* __restrict__ u, int ldu, const float* __restrict__ mean,
                                            const float* __restrict__ rstd, const float* __restrict__ g,
                                            const float* __restrict__ b, int n, int i) {
    f32x4 v = ((const f32x4*)(u + (size_t)n * ldu))[i];
    if (g) {
        const float mu = mean[n], rs = rstd[n];
        const f32x4 ww = ((const f32x4*)g)[i], bb = ((const f32x4*)b)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = isda_gelu((v[k] - mu) * rs * ww[k] + bb[k]);
    }
    return v;
}

// waves [0, V): class c = wave; waves [V, V + B): arg-max of target row wave - V
template <int VPL>
__global__ __launch_bounds__(256) void isda_update_kernel(const float* __restrict__ u, int ldu, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ g,
                                                          const float* __restrict__ b, const float* __restrict__ y, int ldy,
                                                          int B, int V, int A, float* __restrict__ count,
                                                          float* __restrict__ emean, float* __restrict__ cov,
                                                          int32_t* __restrict__ kout) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= V + B) return;
    if (w >= V) {                                   // first maximum of the row (all-zero row -> 0)
        const int n = w - V;
        const float* yr = y + (size_t)n * ldy;
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = lane; c < V; c += 64) {
            const float v = yr[c];
            if (v > best) {
                best = v;
                bi = c;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if (lane == 0) kout[n] = bi < V ? bi : 0;
        return;
    }
    const int c = w;
    const int nv = A >> 2;
    f32x4 s[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int n0 = 0; n0 < B; n0 += 64) {
        const int n = n0 + lane;
        unsigned long long m = __ballot(n < B && y[(size_t)n * ldy + c] != 0.f);
        cnt += __popcll(m);
        while (m) {
            const int r = n0 + __ffsll((long long)m) - 1;
            m &= m - 1;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int i = lane + 64 * j;
                if (i < nv) s[j] += isda_feat4(u, ldu, mean, rstd, g, b, r, i);
            }
        }
    }
    if (cnt == 0) return;
    const float fn = (float)cnt;
#pragma unroll
    for (int j = 0; j < VPL; ++j) s[j] = s[j] / fn;          // class mean of this step
    f32x4 q[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) q[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < B; n0 += 64) {
        const int n = n0 + lane;
        unsigned long long m = __ballot(n < B && y[(size_t)n * ldy + c] != 0.f);
        while (m) {
            const int r = n0 + __ffsll((long long)m) - 1;
            m &= m - 1;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int i = lane + 64 * j;
                if (i < nv) {
                    const f32x4 d = isda_feat4(u, ldu, mean, rstd, g, b, r, i) - s[j];
                    q[j] += d * d;
                }
            }
        }
    }
    const float cold = count[c];
    const float wt = fn / (fn + cold);
    f32x4* mr = (f32x4*)(emean + (size_t)c * A);
    f32x4* cr = (f32x4*)(cov + (size_t)c * A);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = lane + 64 * j;
        if (i < nv) {
            const f32x4 mo = mr[i], co = cr[i];
            const f32x4 var = q[j] / fn;
            const f32x4 dm = mo - s[j];
            cr[i] = co * (1.f - wt) + var * wt + (wt * (1.f - wt)) * (dm * dm);
            mr[i] = mo * (1.f - wt) + s[j] * wt;
        }
    }
    if (lane == 0) count[c] = cold + fn;
}

// part[seg][n][j] = sum_{a in segment} (W[j, a] - W[k_n, a])^2 ck[n, a]; 256 threads = 16 (4 classes) x 16 (4 rows)
__global__ __launch_bounds__(256) void isda_aug_part_kernel(const float* __restrict__ W, int ldw, const int32_t* __restrict__ k,
                                                            const float* __restrict__ ck, int ldc, int B, int V, int A,
                                                            int seg_len, float* __restrict__ part, int ldp) {
    __shared__ __attribute__((aligned(16))) float wj_s[KC][LDT], wk_s[KC][LDT], ck_s[KC][LDT];
    const int tid = threadIdx.x, tj = tid & 15, tn = tid >> 4;
    const int j0 = blockIdx.x * T64, n0 = blockIdx.y * T64;
    const int a_beg = blockIdx.z * seg_len, a_end = min(A, a_beg + seg_len);
    const int lr = tid >> 2, lq = (tid & 3) * 4;          // loader: row lr of the tile, columns lq .. lq + 3 of the chunk
    const int jl = j0 + lr, nl = n0 + lr;
    const float* wrow = jl < V ? W + (size_t)jl * ldw : nullptr;
    const float* krow = nl < B ? W + (size_t)k[nl] * ldw : nullptr;
    const float* crow = nl < B ? ck + (size_t)nl * ldc : nullptr;
    float acc[4][4] = {};
    for (int a0 = a_beg; a0 < a_end; a0 += KC) {
        const int a = a0 + lq;
        const bool in = a < a_end;
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        const f32x4 vw = wrow && in ? *(const f32x4*)(wrow + a) : z4;
        const f32x4 vk = krow && in ? *(const f32x4*)(krow + a) : z4;
        const f32x4 vc = crow && in ? *(const f32x4*)(crow + a) : z4;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            wj_s[lq + q][lr] = vw[q];
            wk_s[lq + q][lr] = vk[q];
            ck_s[lq + q][lr] = vc[q];
        }
        __syncthreads();
#pragma unroll
        for (int aa = 0; aa < KC; ++aa) {
            const f32x4 wj = *(const f32x4*)&wj_s[aa][4 * tj];
            const f32x4 wk = *(const f32x4*)&wk_s[aa][4 * tn];
            const f32x4 cv = *(const f32x4*)&ck_s[aa][4 * tn];
#pragma unroll
            for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float d = wj[x] - wk[yy];
                    acc[yy][x] += d * d * cv[yy];
                }
        }
    }
    float* pp = part + (size_t)blockIdx.z * B * ldp;
#pragma unroll
    for (int yy = 0; yy < 4; ++yy) {
        const int n = n0 + 4 * tn + yy;
        if (n < B) *(f32x4*)(pp + (size_t)n * ldp + j0 + 4 * tj) = f32x4{acc[yy][0], acc[yy][1], acc[yy][2], acc[yy][3]};
    }
}

// z[n, j] += scale * sum_seg part[seg][n][j] for j < V, segments in order
__global__ __launch_bounds__(256) void isda_aug_fold_kernel(const float* __restrict__ part, int ldp, int nseg, int B, int V,
                                                            float scale, float* __restrict__ z, int ldz) {
    const int64_t total = (int64_t)B * V;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int n = (int)(e / V), j = (int)(e % V);
        float s = 0.f;
        for (int q = 0; q < nseg; ++q) s += part[((size_t)q * B + n) * ldp + j];
        z[(size_t)n * ldz + j] += scale * s;
    }
}

// rpart[seg][n][a] = sum_{j in segment} G[n, j] (W[j, a] - W[k_n, a]); 256 threads = 16 (4 columns) x 16 (4 rows)
__global__ __launch_bounds__(256) void isda_rows_part_kernel(const bf16* __restrict__ G, int ldg, const float* __restrict__ W,
                                                             int ldw, const int32_t* __restrict__ k, int B, int V, int A,
                                                             int seg_len, float* __restrict__ rpart) {
    __shared__ __attribute__((aligned(16))) float g_s[KC][LDT], w_s[KC][LDT];
    const int tid = threadIdx.x, ta = tid & 15, tn = tid >> 4;
    const int a0 = blockIdx.x * T64, n0 = blockIdx.y * T64;
    const int j_beg = blockIdx.z * seg_len, j_end = min(V, j_beg + seg_len);
    float wk[4][4];
#pragma unroll
    for (int yy = 0; yy < 4; ++yy) {
        const int n = n0 + 4 * tn + yy, a = a0 + 4 * ta;
        const f32x4 v = n < B && a < A ? *(const f32x4*)(W + (size_t)k[n] * ldw + a) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int x = 0; x < 4; ++x) wk[yy][x] = v[x];
    }
    // loaders: G[n0 + gr, j0 + gq .. + 3] (transposed into g_s[j][n]); W[j0 + wr, a0 + wq .. + 3] (wr < 16, wq < 64)
    const int gr = tid >> 2, gq = (tid & 3) * 4;
    const int wr = tid >> 4, wq = (tid & 15) * 4;
    float acc[4][4] = {};
    for (int j0 = j_beg; j0 < j_end; j0 += KC) {
        float gv[4];
        const int n = n0 + gr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + gq + q;
            gv[q] = n < B && j < j_end ? (float)G[(size_t)n * ldg + j] : 0.f;
        }
        const int jw = j0 + wr, aw = a0 + wq;
        const f32x4 vw = jw < j_end && aw < A ? *(const f32x4*)(W + (size_t)jw * ldw + aw) : f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) g_s[gq + q][gr] = gv[q];
        *(f32x4*)&w_s[wr][wq] = vw;
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < KC; ++jj) {
            const f32x4 gg = *(const f32x4*)&g_s[jj][4 * tn];
            const f32x4 ww = *(const f32x4*)&w_s[jj][4 * ta];
#pragma unroll
            for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                for (int x = 0; x < 4; ++x) acc[yy][x] += gg[yy] * (ww[x] - wk[yy][x]);
        }
    }
    float* rp = rpart + (size_t)blockIdx.z * B * A;
    const int a = a0 + 4 * ta;
    if (a < A)
#pragma unroll
        for (int yy = 0; yy < 4; ++yy) {
            const int n = n0 + 4 * tn + yy;
            if (n < B) *(f32x4*)(rp + (size_t)n * A + a) = f32x4{acc[yy][0], acc[yy][1], acc[yy][2], acc[yy][3]};
        }
}

// dW[j, a] += r * (sum_n G[n, j] (W[j, a] - W[k_n, a]) ck[n, a] - sum_{n: k_n = j} ck[n, a] R[n, a]);
// 256 threads = 16 (4 columns) x 16 (4 classes)
__global__ __launch_bounds__(256) void isda_dw_kernel(const bf16* __restrict__ G, int ldg, const float* __restrict__ W, int ldw,
                                                      const int32_t* __restrict__ k, const float* __restrict__ ck, int ldc,
                                                      const float* __restrict__ rpart, int nseg, int B, int V, int A,
                                                      float r, float* __restrict__ dw, int lddw) {
    __shared__ __attribute__((aligned(16))) float g_s[KC][LDT], wk_s[KC][LDT], ck_s[KC][LDT];
    const int tid = threadIdx.x, ta = tid & 15, tj = tid >> 4;
    const int a0 = blockIdx.x * T64, j0 = blockIdx.y * T64;
    const int a = a0 + 4 * ta;
    float wj[4][4];
#pragma unroll
    for (int yy = 0; yy < 4; ++yy) {
        const int j = j0 + 4 * tj + yy;
        const f32x4 v = j < V && a < A ? *(const f32x4*)(W + (size_t)j * ldw + a) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int x = 0; x < 4; ++x) wj[yy][x] = v[x];
    }
    // loaders: row nr < 16 of the chunk, columns q4 .. q4 + 3 of the 64-wide tile (G over classes, W[k] and ck over a)
    const int nr = tid >> 4, q4 = (tid & 15) * 4;
    float acc[4][4] = {};
    for (int n0 = 0; n0 < B; n0 += KC) {
        const int n = n0 + nr;
        float gv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + q4 + q;
            gv[q] = n < B && j < V ? (float)G[(size_t)n * ldg + j] : 0.f;
        }
        const bool in = n < B && a0 + q4 < A;
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        const f32x4 vk = in ? *(const f32x4*)(W + (size_t)k[n] * ldw + a0 + q4) : z4;
        const f32x4 vc = in ? *(const f32x4*)(ck + (size_t)n * ldc + a0 + q4) : z4;
        __syncthreads();
        *(f32x4*)&g_s[nr][q4] = f32x4{gv[0], gv[1], gv[2], gv[3]};
        *(f32x4*)&wk_s[nr][q4] = vk;
        *(f32x4*)&ck_s[nr][q4] = vc;
        __syncthreads();
#pragma unroll
        for (int nn = 0; nn < KC; ++nn) {
            const f32x4 gg = *(const f32x4*)&g_s[nn][4 * tj];
            const f32x4 wk = *(const f32x4*)&wk_s[nn][4 * ta];
            const f32x4 cv = *(const f32x4*)&ck_s[nn][4 * ta];
#pragma unroll
            for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                for (int x = 0; x < 4; ++x) acc[yy][x] += gg[yy] * ((wj[yy][x] - wk[x]) * cv[x]);
        }
    }
    if (a >= A) return;
    // rows whose arg-max class is one of this thread's 4 classes, ascending n; R folded over its segments in order
    const int jt = j0 + 4 * tj;
    f32x4 sub[4] = {};
    for (int n = 0; n < B; ++n) {
        const int kn = k[n] - jt;
        if (kn < 0 || kn > 3) continue;
        f32x4 rr = {0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < nseg; ++q) rr += *(const f32x4*)(rpart + ((size_t)q * B + n) * A + a);
        const f32x4 cv = *(const f32x4*)(ck + (size_t)n * ldc + a);
#pragma unroll
        for (int yy = 0; yy < 4; ++yy)
            if (kn == yy) sub[yy] += cv * rr;
    }
#pragma unroll
    for (int yy = 0; yy < 4; ++yy) {
        const int j = jt + yy;
        if (j < V) {
            f32x4* o = (f32x4*)(dw + (size_t)j * lddw + a);
            const f32x4 t = f32x4{acc[yy][0], acc[yy][1], acc[yy][2], acc[yy][3]} - sub[yy];
            *o = *o + r * t;
        }
    }
}

int isda_vpl(int A) {
    const int v = (A / 4 + 63) / 64;
    return v <= 1 ? 1 : (v <= 2 ? 2 : (v <= 4 ? 4 : 8));
}

int cdiv(int a, int b) { return (a + b - 1) / b; }

// segments of the split reduction: enough workgroups to fill the chip, in whole KC chunks, capped at `cap` segments
void isda_split(int tiles, int len, int cap, int* nseg, int* seg_len) {
    int s = cdiv(TARGET_WG, tiles);
    const int chunks = cdiv(len, KC);
    s = s < 1 ? 1 : (s > chunks ? chunks : s);
    s = s > cap ? cap : s;
    const int sl = cdiv(chunks, s) * KC;
    *seg_len = sl;
    *nseg = cdiv(len, sl);
}

constexpr int AUG_MAX_SEG = 16, ROWS_MAX_SEG = 32;

}  // namespace

extern "C" int64_t vlmo_isda_ws_bytes(int B, int V, int A) {
    int sa, la, sr, lr;
    isda_split(cdiv(V, T64) * cdiv(B, T64), A, AUG_MAX_SEG, &sa, &la);
    isda_split(cdiv(A, T64) * cdiv(B, T64), V, ROWS_MAX_SEG, &sr, &lr);
    const int64_t fwd = (int64_t)sa * B * cdiv(V, T64) * T64;
    const int64_t bwd = (int64_t)sr * B * A;
    return 4 * (fwd > bwd ? fwd : bwd);
}

extern "C" int vlmo_isda_update(const float* u, int ldu, const float* mean, const float* rstd, const float* ln_w,
                                const float* ln_b, const float* y, int ldy, int B, int V, int A, float* count,
                                float* emean, float* cov, int32_t* k, hipStream_t stream) {
    VLMO_CHECK_ARG(u && y && count && emean && cov && k, "vlmo_isda_update: null pointer");
    VLMO_CHECK_ARG(!ln_w || (ln_b && mean && rstd), "vlmo_isda_update: LayerNorm mode needs mean, rstd, ln_w and ln_b");
    VLMO_CHECK_ARG(B > 0 && V > 0 && A > 0 && A % 4 == 0 && A <= ISDA_MAX_A,
                   "vlmo_isda_update: need B, V > 0, 0 < A <= %d, A %% 4 == 0 (B=%d V=%d A=%d)", ISDA_MAX_A, B, V, A);
    VLMO_CHECK_ARG(ldu >= A && ldu % 4 == 0 && ldy >= V, "vlmo_isda_update: bad ldu/ldy %d/%d", ldu, ldy);
    const dim3 grid(cdiv(V + B, 4));
#define IUP(P) hipLaunchKernelGGL((isda_update_kernel<P>), grid, dim3(256), 0, stream, u, ldu, mean, rstd, ln_w, ln_b, y, ldy, B, V, A, count, emean, cov, k)
    switch (isda_vpl(A)) {
        case 1: IUP(1); break;
        case 2: IUP(2); break;
        case 4: IUP(4); break;
        default: IUP(8); break;
    }
#undef IUP
    VLMO_CHECK_LAUNCH("vlmo_isda_update");
    return 0;
}

extern "C" int vlmo_isda_aug_fwd(const float* W, int ldw, const int32_t* k, const float* ck, int ldc, int B, int V, int A,
                                 float scale, float* z, int ldz, float* ws, int64_t ws_bytes, hipStream_t stream) {
    VLMO_CHECK_ARG(W && k && ck && z && ws, "vlmo_isda_aug_fwd: null pointer");
    VLMO_CHECK_ARG(B > 0 && V > 0 && A > 0 && A % 4 == 0 && A <= ISDA_MAX_A,
                   "vlmo_isda_aug_fwd: need B, V > 0, 0 < A <= %d, A %% 4 == 0 (B=%d V=%d A=%d)", ISDA_MAX_A, B, V, A);
    VLMO_CHECK_ARG(ldw >= A && ldw % 4 == 0 && ldc >= A && ldc % 4 == 0 && ldz >= V,
                   "vlmo_isda_aug_fwd: bad leading dimensions %d/%d/%d", ldw, ldc, ldz);
    VLMO_CHECK_ARG(ws_bytes >= vlmo_isda_ws_bytes(B, V, A), "vlmo_isda_aug_fwd: workspace too small (need %lld bytes)",
                   (long long)vlmo_isda_ws_bytes(B, V, A));
    const int nj = cdiv(V, T64), nn = cdiv(B, T64);
    int nseg, seg_len;
    isda_split(nj * nn, A, AUG_MAX_SEG, &nseg, &seg_len);
    const int ldp = nj * T64;
    hipLaunchKernelGGL(isda_aug_part_kernel, dim3(nj, nn, nseg), dim3(256), 0, stream, W, ldw, k, ck, ldc, B, V, A, seg_len, ws, ldp);
    VLMO_CHECK_LAUNCH("vlmo_isda_aug_fwd(part)");
    const int64_t total = (int64_t)B * V;
    const int fb = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(isda_aug_fold_kernel, dim3(fb), dim3(256), 0, stream, ws, ldp, nseg, B, V, scale, z, ldz);
    VLMO_CHECK_LAUNCH("vlmo_isda_aug_fwd(fold)");
    return 0;
}

extern "C" int vlmo_isda_aug_bwd(const void* G, int ldg, const float* W, int ldw, const int32_t* k, const float* ck, int ldc,
                                 int B, int V, int A, float r, float* dw, int lddw, float* ws, int64_t ws_bytes,
                                 hipStream_t stream) {
    VLMO_CHECK_ARG(G && W && k && ck && dw && ws, "vlmo_isda_aug_bwd: null pointer");
    VLMO_CHECK_ARG(B > 0 && V > 0 && A > 0 && A % 4 == 0 && A <= ISDA_MAX_A,
                   "vlmo_isda_aug_bwd: need B, V > 0, 0 < A <= %d, A %% 4 == 0 (B=%d V=%d A=%d)", ISDA_MAX_A, B, V, A);
    VLMO_CHECK_ARG(ldg >= V && ldw >= A && ldw % 4 == 0 && ldc >= A && ldc % 4 == 0 && lddw >= A && lddw % 4 == 0,
                   "vlmo_isda_aug_bwd: bad leading dimensions %d/%d/%d/%d", ldg, ldw, ldc, lddw);
    VLMO_CHECK_ARG(ws_bytes >= vlmo_isda_ws_bytes(B, V, A), "vlmo_isda_aug_bwd: workspace too small (need %lld bytes)",
                   (long long)vlmo_isda_ws_bytes(B, V, A));
    const int na = cdiv(A, T64), nn = cdiv(B, T64);
    int nseg, seg_len;
    isda_split(na * nn, V, ROWS_MAX_SEG, &nseg, &seg_len);
    hipLaunchKernelGGL(isda_rows_part_kernel, dim3(na, nn, nseg), dim3(256), 0, stream, (const bf16*)G, ldg, W, ldw, k, B, V,
                       A, seg_len, ws);
    VLMO_CHECK_LAUNCH("vlmo_isda_aug_bwd(rows)");
    hipLaunchKernelGGL(isda_dw_kernel, dim3(na, cdiv(V, T64)), dim3(256), 0, stream, (const bf16*)G, ldg, W, ldw, k, ck, ldc,
                       ws, nseg, B, V, A, r, dw, lddw);
    VLMO_CHECK_LAUNCH("vlmo_isda_aug_bwd(dw)");
    return 0;
}
