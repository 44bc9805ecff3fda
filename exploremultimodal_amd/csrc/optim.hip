// Multi-tensor optimizer step for the VLMo training loop: global gradient L2 norm + clip coefficient and a
// fused Adam / AdamW update over a LIST of parameter tensors in one launch each (the reference's default
// optimizer is apex FusedAdam(adam_w_mode=True), utils/optim_factory.py:185-186; the clip is
// torch.nn.utils.clip_grad_norm_ inside NativeScalerWithGradNormCount, utils/utils.py:343-364).
// HBM-bound: 16 B read + 12 B written per parameter; work is cut into fixed-size chunks so that ~300 tensors of
// very different sizes fill the chip evenly, one workgroup per chunk.
#include "common.h"
#include "vlmo_hip.h"

namespace {

constexpr int OPT_THREADS = 256;

// Sum over the workgroup in double, for the gradient norm: the order of the tensors in the table and the load path a chunk
// takes should not show in its value (see mt_sqnorm_kernel).
__device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < OPT_THREADS / 64; ++i) t += red[i];
    return t;      // valid in every thread
}

// partial[c] = sum of g^2 over chunk c.  Squares (exact in double) and sums are taken in double and the chunk's total is
// rounded to fp32 once.  The double sum still depends on its order, at ~1e-16 relative per addition, so before the rounding
// the value is the exact sum's to ~1e-13; two orders round to different fp32 values only when the exact sum lies that close
// to the midpoint of two floats (1e-13 against a spacing of 6e-8: a few chunks in a million).  So the 16-byte path and the scalar one, and FusedAdam
// (tensors in group order) and ZeroAdam at world size 1 (the same tensors in bucket order), give the same norm except for
// such a tie: overwhelmingly likely, not guaranteed.
__global__ __launch_bounds__(OPT_THREADS) void mt_sqnorm_kernel(const VlmoTensorList tl, float* __restrict__ partial) {
    __shared__ double red[OPT_THREADS / 64];
    const int c = blockIdx.x;
    const int t = tl.chunk_tensor[c];
    const int64_t off = tl.chunk_start[c];
    const int64_t n = min((int64_t)tl.chunk, tl.numel[t] - off);
    const float* g = (const float*)tl.g[t] + off;
    double a = 0.0;
    auto sq = [&](float x) { a = fma((double)x, (double)x, a); };
    if ((((uintptr_t)g) & 15) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += OPT_THREADS) {
            const f32x4 v = ((const f32x4*)g)[i];
            sq(v[0]), sq(v[1]), sq(v[2]), sq(v[3]);
        }
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += OPT_THREADS) sq(g[i]);
    } else {
        for (int64_t i = threadIdx.x; i < n; i += OPT_THREADS) sq(g[i]);
    }
    const double s = block_sum_d(a, red);
    if (threadIdx.x == 0) partial[c] = (float)s;
}

// out[0] = ||g||_2, out[1] = clip coefficient min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0),
// out[2] = 1 if the norm is not finite (the update is then skipped, as torch.cuda.amp.GradScaler.step does)
__global__ __launch_bounds__(OPT_THREADS) void mt_norm_finish_kernel(const float* __restrict__ partial, int n, float inv_scale,
                                                                    float max_norm, float* __restrict__ out) {
    __shared__ double red[OPT_THREADS / 64];
    double a = 0.0;     // double to the end: the order of the partials shows only below 1e-13 of the sum
    for (int i = threadIdx.x; i < n; i += OPT_THREADS) a += (double)partial[i];
    const float s = (float)block_sum_d(a, red);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(s) * inv_scale;
        const bool bad = !(norm == norm) || norm > 3.0e38f;
        out[0] = norm;
        float coef = inv_scale;
        if (max_norm > 0.f) coef *= fminf(1.f, max_norm / (norm + 1e-6f));
        out[1] = bad ? 0.f : coef;
        out[2] = bad ? 1.f : 0.f;
    }
}

// One step of the weight average e <- e + w (p - e), w = 1 - decay.  e == p is an exact fixed point (p - e = 0), so the
// average of a tensor that never changes never drifts, which decay * e + w * p does not give.  From w = 0.5 on the same
// value is written from p's side, p - (1 - w) (p - e), as torch.lerp does: w = 1 then copies p exactly (w - 1 is exact
// there).  Every kernel that averages calls this.
__device__ __forceinline__ float ema_update(float e, float p, float w) {
    const float d = p - e;
    return w < 0.5f ? fmaf(w, d, e) : fmaf(w - 1.f, d, p);
}

// e[0, n) <- average toward p[0, n): 16-byte accesses when both pointers are aligned, a scalar tail, a scalar path otherwise
__device__ __forceinline__ void ema_chunk(float* e, const float* p, int64_t n, float w) {
    if (((((uintptr_t)e) | ((uintptr_t)p)) & 15) == 0) {
        const int64_t n4 = n >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += OPT_THREADS) {
            f32x4 ee = ((f32x4*)e)[i];
            const f32x4 pp = ((const f32x4*)p)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) ee[j] = ema_update(ee[j], pp[j], w);
            ((f32x4*)e)[i] = ee;
        }
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += OPT_THREADS) e[i] = ema_update(e[i], p[i], w);
    } else {
        for (int64_t i = threadIdx.x; i < n; i += OPT_THREADS) e[i] = ema_update(e[i], p[i], w);
    }
}

// The Adam step of one chunk.  EMA: the weight average of the tensor (ema[t], or 0 for a tensor without one) takes its
// step toward the NEW parameter value in the same pass; a skipped step still moves it, toward the unchanged parameters.
// mt_adam_kernel is the instance without, so the two kernels share every line of the Adam update.
template <bool EMA>
__device__ __forceinline__ void adam_chunk(const VlmoTensorList& tl, const VlmoAdamArgs& a, const float* __restrict__ ctl,
                                           const int64_t* __restrict__ ema, float w) {
    const float gscale = ctl ? ctl[1] : 1.f;
    if (ctl && ctl[2] != 0.f) {             // non-finite gradients: skip the step
        if (EMA) {
            const int t = tl.chunk_tensor[blockIdx.x];
            const int64_t off = tl.chunk_start[blockIdx.x];
            if (ema[t]) ema_chunk((float*)ema[t] + off, (const float*)tl.p[t] + off, min((int64_t)tl.chunk, tl.numel[t] - off), w);
        }
        return;
    }
    const int c = blockIdx.x;
    const int t = tl.chunk_tensor[c];
    const int64_t off = tl.chunk_start[c];
    const int64_t n = min((int64_t)tl.chunk, tl.numel[t] - off);
    float* p = (float*)tl.p[t] + off;
    const float* g = (const float*)tl.g[t] + off;
    float* m = (float*)tl.m[t] + off;
    float* v = (float*)tl.v[t] + off;
    float* e = EMA && ema[t] ? (float*)ema[t] + off : nullptr;
    const float lr = tl.lr[t], wd = tl.wd[t];
    const float b1 = a.beta1, b2 = a.beta2, ob1 = 1.f - a.beta1, ob2 = 1.f - a.beta2;
    auto upd = [&](float& pp, float gg, float& mm, float& vv) {
        gg *= gscale;
        if (!a.adam_w_mode) gg += wd * pp;                 // L2 mode: decay enters the moments
        mm = b1 * mm + ob1 * gg;
        vv = b2 * vv + ob2 * gg * gg;
        const float denom = sqrtf(vv * a.inv_bc2) + a.eps;
        float u = (mm * a.inv_bc1) / denom;
        if (a.adam_w_mode) u += wd * pp;                   // decoupled decay
        pp -= lr * u;
    };
    const bool al = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)e)) & 15) == 0;
    if (al) {
        const int64_t n4 = n >> 2;
        for (int64_t i = threadIdx.x; i < n4; i += OPT_THREADS) {
            f32x4 pp = ((f32x4*)p)[i], mm = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
            const f32x4 gg = ((const f32x4*)g)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = pp[j], y = mm[j], z = vv[j];
                upd(x, gg[j], y, z);
                pp[j] = x, mm[j] = y, vv[j] = z;
            }
            ((f32x4*)p)[i] = pp, ((f32x4*)m)[i] = mm, ((f32x4*)v)[i] = vv;
            if (EMA && e) {
                f32x4 ee = ((f32x4*)e)[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) ee[j] = ema_update(ee[j], pp[j], w);
                ((f32x4*)e)[i] = ee;
            }
        }
        for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += OPT_THREADS) upd(p[i], g[i], m[i], v[i]);
        // the scalar elements average in a loop of their own (each thread re-reads what it just wrote): appended to the
        // update above they changed which of its multiply-adds the compiler fuses, and with that its last bit
        if (EMA && e)
            for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += OPT_THREADS) e[i] = ema_update(e[i], p[i], w);
    } else {
        for (int64_t i = threadIdx.x; i < n; i += OPT_THREADS) upd(p[i], g[i], m[i], v[i]);
        if (EMA && e)
            for (int64_t i = threadIdx.x; i < n; i += OPT_THREADS) e[i] = ema_update(e[i], p[i], w);
    }
}

__global__ __launch_bounds__(OPT_THREADS) void mt_adam_kernel(const VlmoTensorList tl, const VlmoAdamArgs a,
                                                             const float* __restrict__ ctl) {
    adam_chunk<false>(tl, a, ctl, nullptr, 0.f);
}

__global__ __launch_bounds__(OPT_THREADS) void mt_adam_ema_kernel(const VlmoTensorList tl, const VlmoAdamArgs a,
                                                                 const float* __restrict__ ctl,
                                                                 const int64_t* __restrict__ ema, float w) {
    adam_chunk<true>(tl, a, ctl, ema, w);
}

// tl.p[t] = the average (written in place), tl.g[t] = the tensor it follows
__global__ __launch_bounds__(OPT_THREADS) void mt_ema_kernel(const VlmoTensorList tl, float w) {
    const int c = blockIdx.x;
    const int t = tl.chunk_tensor[c];
    const int64_t off = tl.chunk_start[c];
    ema_chunk((float*)tl.p[t] + off, (const float*)tl.g[t] + off, min((int64_t)tl.chunk, tl.numel[t] - off), w);
}

int check_list(const VlmoTensorList* tl, const char* who) {
    VLMO_CHECK_ARG(tl && tl->n_chunks >= 0 && tl->chunk > 0 && tl->chunk % 4 == 0, "%s: bad tensor list", who);
    VLMO_CHECK_ARG(tl->n_chunks == 0 || (tl->g && tl->numel && tl->chunk_tensor && tl->chunk_start), "%s: null table", who);
    return 0;
}

}  // namespace

extern "C" int vlmo_mt_grad_norm(const VlmoTensorList* tl, float inv_scale, float max_norm, float* partial, float* out,
                                 hipStream_t stream) {
    if (int rc = check_list(tl, "vlmo_mt_grad_norm")) return rc;
    VLMO_CHECK_ARG(partial && out, "vlmo_mt_grad_norm: null output");
    if (tl->n_chunks > 0) {
        hipLaunchKernelGGL(mt_sqnorm_kernel, dim3(tl->n_chunks), dim3(OPT_THREADS), 0, stream, *tl, partial);
        VLMO_CHECK_LAUNCH("vlmo_mt_grad_norm");
    }
    hipLaunchKernelGGL(mt_norm_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, stream, partial, tl->n_chunks, inv_scale, max_norm, out);
    VLMO_CHECK_LAUNCH("vlmo_mt_grad_norm(finish)");
    return 0;
}

extern "C" int vlmo_mt_adam(const VlmoTensorList* tl, const VlmoAdamArgs* a, const float* ctl, hipStream_t stream) {
    if (int rc = check_list(tl, "vlmo_mt_adam")) return rc;
    VLMO_CHECK_ARG(a && a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f,
                   "vlmo_mt_adam: bad hyper-parameters");
    if (tl->n_chunks == 0) return 0;
    VLMO_CHECK_ARG(tl->p && tl->m && tl->v && tl->lr && tl->wd, "vlmo_mt_adam: null table");
    hipLaunchKernelGGL(mt_adam_kernel, dim3(tl->n_chunks), dim3(OPT_THREADS), 0, stream, *tl, *a, ctl);
    VLMO_CHECK_LAUNCH("vlmo_mt_adam");
    return 0;
}

extern "C" int vlmo_mt_ema(const VlmoTensorList* tl, float w, hipStream_t stream) {
    if (int rc = check_list(tl, "vlmo_mt_ema")) return rc;
    VLMO_CHECK_ARG(w >= 0.f && w <= 1.f, "vlmo_mt_ema: w = 1 - decay = %g is outside [0, 1]", (double)w);
    if (tl->n_chunks == 0) return 0;
    VLMO_CHECK_ARG(tl->p, "vlmo_mt_ema: null table");
    hipLaunchKernelGGL(mt_ema_kernel, dim3(tl->n_chunks), dim3(OPT_THREADS), 0, stream, *tl, w);
    VLMO_CHECK_LAUNCH("vlmo_mt_ema");
    return 0;
}

extern "C" int vlmo_mt_adam_ema(const VlmoTensorList* tl, const VlmoAdamArgs* a, const float* ctl, const void* const* ema,
                                float w, hipStream_t stream) {
    if (int rc = check_list(tl, "vlmo_mt_adam_ema")) return rc;
    VLMO_CHECK_ARG(a && a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f,
                   "vlmo_mt_adam_ema: bad hyper-parameters");
    VLMO_CHECK_ARG(w >= 0.f && w <= 1.f, "vlmo_mt_adam_ema: w = 1 - decay = %g is outside [0, 1]", (double)w);
    if (tl->n_chunks == 0) return 0;
    VLMO_CHECK_ARG(tl->p && tl->m && tl->v && tl->lr && tl->wd && ema, "vlmo_mt_adam_ema: null table");
    hipLaunchKernelGGL(mt_adam_ema_kernel, dim3(tl->n_chunks), dim3(OPT_THREADS), 0, stream, *tl, *a, ctl, (const int64_t*)ema, w);
    VLMO_CHECK_LAUNCH("vlmo_mt_adam_ema");
    return 0;
}
