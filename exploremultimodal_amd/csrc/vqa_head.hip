// VQA classifier head (models/vlmo/vlmo_module.py:85-93: Linear(hs, 2hs) -> LayerNorm(2hs) -> GELU -> Linear(2hs, vs))
// and its binary cross-entropy loss / score (models/vlmo/objectives.py:12-21, 317-353).  The two Linears run on the
// GEMMs of gemm_nt.hip / gemm_tn.hip; this file holds the row kernels between and after them:
//   ln_gelu_fwd   LayerNorm (fp32 statistics, eps 1e-12) + exact-erf GELU -> the bf16 operand of the second GEMM
//   ln_gelu_bwd   recompute the LayerNorm output, GELU', LayerNorm backward; deterministic column sums (fixed-order
//                 per-wave partials folded in order, no atomics) for d gamma, d beta and the first Linear's d bias
//   vqa_bce       per row of the fp32 logits: BCE-with-logits sum, arg-max, target at the arg-max; in backward mode
//                 the bf16 operand (sigmoid(z) - y) * scale (+ an incoming logits gradient), pad columns zeroed
// The head is 2-4 KFLOP per row and B rows (16..512): one wavefront per row keeps every row in registers.
#include "common.h"
#include "vlmo_hip.h"

namespace {

constexpr int LNG_MAX_D = 2048;
constexpr int LNG_MAX_WAVES = 128;      // partial rows of the column sums

__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_exact_grad(float x) {
    return 0.5f * (1.f + erff(x * 0.70710678118654752f)) + x * 0.39894228040143268f * expf(-0.5f * x * x);
}

// one wave per row; rows beyond M leave the kernel as whole waves (wave_sum needs every lane of a wave)
template <int VPL>
__global__ __launch_bounds__(256) void ln_gelu_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                          const float* __restrict__ b, bf16* __restrict__ h, int ldh,
                                                          float* __restrict__ mean, float* __restrict__ rstd, int M, int d,
                                                          float eps) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int nv = d >> 2;
    const f32x4* xr = (const f32x4*)(x + (size_t)m * ldx);
    f32x4 v[VPL];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = lane + 64 * j;
        v[j] = i < nv ? xr[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        s += v[j][0] + v[j][1] + v[j][2] + v[j][3];
    }
    const float mu = wave_sum(s) / d;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
        if (lane + 64 * j < nv)
#pragma unroll
            for (int k = 0; k < 4; ++k) q += (v[j][k] - mu) * (v[j][k] - mu);
    const float rs = rsqrtf(wave_sum(q) / d + eps);
    if (lane == 0) {
        mean[m] = mu;
        rstd[m] = rs;
    }
    bf16* hr = h + (size_t)m * ldh;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = lane + 64 * j;
        if (i < nv) {
            const f32x4 ww = ((const f32x4*)w)[i], bb = ((const f32x4*)b)[i];
            bf16x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (bf16)gelu_exact((v[j][k] - mu) * rs * ww[k] + bb[k]);
            *(bf16x4*)(hr + 4 * i) = o;
        }
    }
    for (int i = nv + lane; 4 * i < ldh; i += 64) *(bf16x4*)(hr + 4 * i) = bf16x4{(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
}

// wave gw of nw takes rows gw, gw + nw, ...; its column sums (d gamma, d beta, d bias) go to partial row gw of ws [nw, 3d]
template <int VPL>
__global__ __launch_bounds__(256) void ln_gelu_bwd_kernel(const float* __restrict__ dh, int lddh, const float* __restrict__ x,
                                                          int ldx, const float* __restrict__ w, const float* __restrict__ b,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          float* __restrict__ dx, int lddx, bf16* __restrict__ dxb, int lddxb,
                                                          float* __restrict__ ws, int M, int d, int nw) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= nw) return;
    const int nv = d >> 2;
    f32x4 ag[VPL], ab[VPL], ad[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) ag[j] = ab[j] = ad[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m = gw; m < M; m += nw) {
        const float mu = mean[m], rs = rstd[m];
        f32x4 xh[VPL], gw4[VPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int i = lane + 64 * j;
            xh[j] = gw4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < nv) {
                const f32x4 xv = ((const f32x4*)(x + (size_t)m * ldx))[i];
                const f32x4 dv = ((const f32x4*)(dh + (size_t)m * lddh))[i];
                const f32x4 ww = ((const f32x4*)w)[i], bb = ((const f32x4*)b)[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    xh[j][k] = (xv[k] - mu) * rs;
                    const float g = dv[k] * gelu_exact_grad(xh[j][k] * ww[k] + bb[k]);     // d loss / d (LayerNorm output)
                    ag[j][k] += g * xh[j][k];
                    ab[j][k] += g;
                    gw4[j][k] = g * ww[k];
                    s1 += gw4[j][k];
                    s2 += gw4[j][k] * xh[j][k];
                }
            }
        }
        const float c1 = wave_sum(s1) / d, c2 = wave_sum(s2) / d;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int i = lane + 64 * j;
            if (i < nv) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = rs * (gw4[j][k] - c1 - xh[j][k] * c2);
                ad[j] += o;
                if (dx) ((f32x4*)(dx + (size_t)m * lddx))[i] = o;
                if (dxb) *(bf16x4*)(dxb + (size_t)m * lddxb + 4 * i) = bf16x4{(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
            }
        }
        if (dxb)
            for (int i = nv + lane; 4 * i < lddxb; i += 64)
                *(bf16x4*)(dxb + (size_t)m * lddxb + 4 * i) = bf16x4{(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
    }
    float* wr = ws + (size_t)gw * 3 * d;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = lane + 64 * j;
        if (i < nv) {
            ((f32x4*)wr)[i] = ag[j];
            ((f32x4*)(wr + d))[i] = ab[j];
            ((f32x4*)(wr + 2 * d))[i] = ad[j];
        }
    }
}

// out[c] = sum over the nw partial rows in row order (plain stores: the same sum every run)
__global__ __launch_bounds__(256) void ln_gelu_fold_kernel(const float* __restrict__ ws, int nw, int d, float* __restrict__ dw,
                                                           float* __restrict__ db, float* __restrict__ dbias) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= 3 * d) return;
    const int k = c / d;
    float* out = k == 0 ? dw : (k == 1 ? db : dbias);
    if (!out) return;
    float s = 0.f;
    int r = 0;
    for (; r + 8 <= nw; r += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = ws[(size_t)(r + u) * 3 * d + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; r < nw; ++r) s += ws[(size_t)r * 3 * d + c];
    out[c - k * d] = s;
}

// one 256-thread workgroup per row.  Arg-max: the first maximum wins (smallest column among equal maxima).
template <bool BWD>
__global__ __launch_bounds__(256) void vqa_bce_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ y,
                                                      int ldy, int V, float* __restrict__ row_loss,
                                                      int32_t* __restrict__ row_arg, float* __restrict__ row_score,
                                                      const float* __restrict__ dscale, float alpha,
                                                      const float* __restrict__ dadd, int ldadd, bf16* __restrict__ dz,
                                                      int lddz) {
    __shared__ float red_s[4], red_v[4];
    __shared__ int red_i[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* zr = z + (size_t)row * ldz;
    const float* yr = y ? y + (size_t)row * ldy : nullptr;
    const float scale = BWD ? alpha * (dscale ? *dscale : 1.f) : 0.f;
    float s = 0.f, best = -INFINITY;
    int bi = 0x7fffffff;
    for (int n = tid; n < V; n += 256) {
        const float zv = zr[n];
        const float yv = yr ? yr[n] : 0.f;
        s += fmaxf(zv, 0.f) - zv * yv + log1pf(expf(-fabsf(zv)));
        if (zv > best) {
            best = zv;
            bi = n;
        }
        if constexpr (BWD) {
            float g = yr ? (1.f / (1.f + expf(-zv)) - yv) * scale : 0.f;
            if (dadd) g += dadd[(size_t)row * ldadd + n];
            dz[(size_t)row * lddz + n] = (bf16)g;
        }
    }
    if constexpr (BWD)
        for (int n = V + tid; n < lddz; n += 256) dz[(size_t)row * lddz + n] = (bf16)0.f;
    if (!row_loss && !row_arg && !row_score) return;
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        red_s[wave] = s;
        red_v[wave] = best;
        red_i[wave] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        const float tot = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        float bv = red_v[0];
        int bidx = red_i[0];
        for (int q = 1; q < 4; ++q)
            if (red_v[q] > bv || (red_v[q] == bv && red_i[q] < bidx)) {
                bv = red_v[q];
                bidx = red_i[q];
            }
        if (bidx >= V) bidx = 0;        // every logit NaN
        if (row_loss) row_loss[row] = tot;
        if (row_arg) row_arg[row] = bidx;
        if (row_score) row_score[row] = yr ? yr[bidx] : 0.f;
    }
}

// bytes of the partial-row workspace of vlmo_ln_gelu_bwd (include/vlmo_hip.h states the same formula)
int64_t lng_ws_bytes(int M, int d) { return (int64_t)(M < LNG_MAX_WAVES ? M : LNG_MAX_WAVES) * 3 * d * 4; }

int lng_vpl(int d) {
    const int v = (d / 4 + 63) / 64;
    return v <= 1 ? 1 : (v <= 2 ? 2 : (v <= 4 ? 4 : 8));
}

}  // namespace

extern "C" int vlmo_ln_gelu_fwd(const float* x, int ldx, const float* w, const float* b, void* h, int ldh, float* mean,
                                float* rstd, int M, int d, float eps, hipStream_t stream) {
    VLMO_CHECK_ARG(x && w && b && h && mean && rstd, "vlmo_ln_gelu_fwd: null pointer");
    VLMO_CHECK_ARG(M > 0 && d > 0 && d % 4 == 0 && d <= LNG_MAX_D,
                   "vlmo_ln_gelu_fwd: need 0 < d <= %d, d %% 4 == 0 (d=%d, M=%d)", LNG_MAX_D, d, M);
    VLMO_CHECK_ARG(ldx >= d && ldx % 4 == 0 && ldh >= d && ldh % 4 == 0, "vlmo_ln_gelu_fwd: bad ldx/ldh %d/%d", ldx, ldh);
    const dim3 grid((M + 3) / 4);
#define LGF(V) hipLaunchKernelGGL((ln_gelu_fwd_kernel<V>), grid, dim3(256), 0, stream, x, ldx, w, b, (bf16*)h, ldh, mean, rstd, M, d, eps)
    switch (lng_vpl(d)) {
        case 1: LGF(1); break;
        case 2: LGF(2); break;
        case 4: LGF(4); break;
        default: LGF(8); break;
    }
#undef LGF
    VLMO_CHECK_LAUNCH("vlmo_ln_gelu_fwd");
    return 0;
}

extern "C" int vlmo_ln_gelu_bwd(const float* dh, int lddh, const float* x, int ldx, const float* w, const float* b,
                                const float* mean, const float* rstd, float* dx, int lddx, void* dxb, int lddxb, float* dw,
                                float* db, float* dbias, int M, int d, float* ws, int64_t ws_bytes, hipStream_t stream) {
    VLMO_CHECK_ARG(dh && x && w && b && mean && rstd && (dx || dxb), "vlmo_ln_gelu_bwd: null pointer");
    VLMO_CHECK_ARG(M > 0 && d > 0 && d % 4 == 0 && d <= LNG_MAX_D,
                   "vlmo_ln_gelu_bwd: need 0 < d <= %d, d %% 4 == 0 (d=%d, M=%d)", LNG_MAX_D, d, M);
    VLMO_CHECK_ARG(lddh >= d && lddh % 4 == 0 && ldx >= d && ldx % 4 == 0 && (!dx || (lddx >= d && lddx % 4 == 0)) &&
                       (!dxb || (lddxb >= d && lddxb % 4 == 0)),
                   "vlmo_ln_gelu_bwd: bad leading dimensions");
    VLMO_CHECK_ARG(ws && ws_bytes >= lng_ws_bytes(M, d), "vlmo_ln_gelu_bwd: workspace too small (need %lld bytes)",
                   (long long)lng_ws_bytes(M, d));
    const int nw = M < LNG_MAX_WAVES ? M : LNG_MAX_WAVES;
    const dim3 grid((nw + 3) / 4);
#define LGB(V) hipLaunchKernelGGL((ln_gelu_bwd_kernel<V>), grid, dim3(256), 0, stream, dh, lddh, x, ldx, w, b, mean, rstd, dx, lddx, (bf16*)dxb, lddxb, ws, M, d, nw)
    switch (lng_vpl(d)) {
        case 1: LGB(1); break;
        case 2: LGB(2); break;
        case 4: LGB(4); break;
        default: LGB(8); break;
    }
#undef LGB
    VLMO_CHECK_LAUNCH("vlmo_ln_gelu_bwd");
    if (dw || db || dbias) {
        hipLaunchKernelGGL(ln_gelu_fold_kernel, dim3((3 * d + 255) / 256), dim3(256), 0, stream, ws, nw, d, dw, db, dbias);
        VLMO_CHECK_LAUNCH("vlmo_ln_gelu_bwd(fold)");
    }
    return 0;
}

extern "C" int vlmo_vqa_bce(const float* z, int ldz, const float* y, int ldy, int B, int V, float* row_loss,
                            int32_t* row_arg, float* row_score, const float* dscale, float alpha, const float* dadd,
                            int ldadd, void* dz, int lddz, hipStream_t stream) {
    VLMO_CHECK_ARG(z && B > 0 && V > 0 && ldz >= V, "vlmo_vqa_bce: bad logits (B=%d V=%d ldz=%d)", B, V, ldz);
    VLMO_CHECK_ARG(!y || ldy >= V, "vlmo_vqa_bce: bad targets ldy=%d", ldy);
    VLMO_CHECK_ARG(y || (!row_loss && !row_score), "vlmo_vqa_bce: loss and score need targets");
    VLMO_CHECK_ARG(!dadd || ldadd >= V, "vlmo_vqa_bce: bad ldadd=%d", ldadd);
    VLMO_CHECK_ARG(!dz || (lddz >= V && lddz % 64 == 0), "vlmo_vqa_bce: dz needs lddz >= V, a multiple of 64 (lddz=%d)", lddz);
    if (dz)
        hipLaunchKernelGGL((vqa_bce_kernel<true>), dim3(B), dim3(256), 0, stream, z, ldz, y, ldy, V, row_loss, row_arg,
                           row_score, dscale, alpha, dadd, ldadd, (bf16*)dz, lddz);
    else
        hipLaunchKernelGGL((vqa_bce_kernel<false>), dim3(B), dim3(256), 0, stream, z, ldz, y, ldy, V, row_loss, row_arg,
                           row_score, dscale, alpha, dadd, ldadd, (bf16*)nullptr, 0);
    VLMO_CHECK_LAUNCH("vlmo_vqa_bce");
    return 0;
}
