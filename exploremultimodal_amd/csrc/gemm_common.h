// MFMA GEMMs for the VLMo hot path on gfx950.
//
//  gemm_nt : C[M,N] = A[M,K] . B[N,K]^T   (both operands K-contiguous)
//            forward linears (x . W^T) and, with pre-transposed weights, dgrad.
//            Reference call sites: vlmo.py:70-80 (qkv), :96 (proj), timm Mlp
//            fc1/fc2 (vlmo.py:141-157), patch-embed conv as GEMM (vlmo.py:304).
//  gemm_tn : C[N1,N2] += A[M,N1]^T . B[M,N2] (reduction over rows, split over
//            the grid's z dimension, fp32 atomics) = wgrad.
//
// Structure (per workgroup): BMxBNx64 tile, operands staged global->LDS by
// LDS-DMA (global_load_lds, 16 B/lane) into a 2-deep ring, XOR-swizzled on the
// SOURCE address so ds_read_b128 fragment reads are bank-conflict free, one
// barrier per K-tile, v_mfma_f32_32x32x16 accumulating in fp32, epilogue
// transposed through wave-private LDS so every global access is a full
// 128/256-byte row segment with the bias/GELU/dropout/layer-scale/residual
// math fused in.
//
// The kernels live in four translation units that build in parallel; this header holds what more than one of them needs
// (problem descriptors, epilogue arithmetic, addressing helpers, gemm_nt_kernel and its launcher):
//   gemm_nt.hip    the 32x32x16 NT path: argument checks, the tile planner (run_nt), vlmo_gemm_nt*, GEMM profiling
//   gemm_nt16.hip  gemm_nt16_kernel: the 16x16x32 NT kernels of every tile height
//   gemm_tn.hip    weight gradients: gemm_tn_kernel, gemm_tn_multi_kernel, tn_reduce_kernel
//   conv.hip       the dVAE convolutions: conv3_dx_kernel and the implicit-GEMM (CONV) instantiations of gemm_nt_kernel
// Nothing is instantiated here, so every kernel belongs to exactly one unit.
#pragma once
#include "common.h"
#include "vlmo_hip.h"

namespace {

struct GemmNT {
    const void* A;
    const void* B;
    int M, N, K, lda, ldb;
    VlmoEpilogue e;
    // implicit-GEMM convolution over an NHWC activation matrix [B*H*W, Cin] (dVAE encoder):
    // K = kw*kw*Cin, k-tile -> (tap, 64-channel chunk); taps outside the image read `zero`
    int cH, cW, cCin, ckw;
    const void* zero;
    int group_m;     // L2 tile swizzle: row-tiles per group
    // two-segment A (vlmo_gemm_nt_2src): columns [0, k1) of the reduction come from A, [k1, K) from A2 (own leading
    // dimension); the partial sum of the first segment is multiplied by seg_scale before the second one is added.
    // k1 == 0: single source.
    const void* A2;
    int lda2, k1;
    float seg_scale;
};

// Up to 4 problems with the same N, K, leading dimensions and epilogue kind in ONE launch (the per-modality
// expert FFNs below the fusion layer: different row ranges, weights, biases): group g owns the logical tiles
// [t0[g], t0[g+1]).  A launch never takes less than one tile time, so two half-empty launches cost twice one.
constexpr int MAX_GROUPS = 4;
struct GemmNTGroups {
    int ngroups;
    int t0[MAX_GROUPS + 1];
    GemmNT g[MAX_GROUPS];
};

// element address split into a wave-uniform 64-bit part and a per-lane 32-bit part
struct RowAddr {
    size_t base;
    uint32_t off;
    template <typename U> __device__ __forceinline__ U* at(const void* p) const {
        return (U*)((char*)((U*)p + base) + off * (uint32_t)sizeof(U));
    }
};
// NT = true: streaming output, a non-temporal store does not push the operand panels the neighbouring tiles re-read
// out of the XCD's L2 (measured per output kind -- bias, u, h, GELU-derivative: non-temporal is equal or better for
// each, -0.3 ms per step together; the same hint on the fp32 residual output costs +0.23 ms and on the outputs of
// the LayerNorm / attention kernels +1.0 ms: their consumers find them in the Infinity Cache)
template <typename T, bool NT = true> __device__ __forceinline__ void store4(T* p, float a, float b, float c, float d) {
    typedef typename Elem<T>::v4 v4;
    const v4 v = {(T)a, (T)b, (T)c, (T)d};
    if constexpr (NT)
        __builtin_nontemporal_store(v, (v4*)p);
    else
        *(v4*)p = v;
}
// epilogue inputs read exactly once (fp32 residual, pre-activation): non-temporal, -0.08 ms per step.  The fp32 residual
// OUTPUT stays a normal store: the next kernel (LayerNorm) reads it back at once, non-temporal was +0.23 ms.
#define NT_LD(p) __builtin_nontemporal_load(p)
template <typename T> __device__ __forceinline__ f32x4 load4(const T* p);
template <> __device__ __forceinline__ f32x4 load4<bf16>(const bf16* p) {
    bf16x4 v = NT_LD((const bf16x4*)p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
template <> __device__ __forceinline__ f32x4 load4<f16>(const f16* p) {
    f16x4 v = NT_LD((const f16x4*)p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// Epilogue math for 4 consecutive output columns (gn..gn+3) of row gm.  Everything that has to come
// from global memory is passed in (bias/gamma: loaded once per tile; `ext` = residual / pre-activation
// row segment and `rs` = drop-path scale: loaded for a whole pass BEFORE any math so the ~1-2 us
// global latencies overlap instead of serialising load -> math -> store per row group).
// keeps the four values live in registers HERE: hipcc otherwise sinks the arithmetic that produced them into the
// guarded block of their only user (the store) -- see epilogue4
__device__ __forceinline__ void pin4(f32x4& v) {
    asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
}

// GD: VlmoEpilogue.relu bit 2 (saved GELU derivative, see VLMO_EPI_BIAS_GELU below) known at compile time (0 / 1) or read from the
// descriptor (-1).  The 16x16x32 kernels instantiate both: with the choice at run time each unrolled epilogue pass carried
// both bodies and the fc1 kernel grew to 110 KB of instructions.
template <typename T, int EPI, int GD = -1>
__device__ __forceinline__ f32x4 epilogue4(const GemmNT& p, int gmb, int row, int gn, f32x4 v, f32x4 bias4,
                                           f32x4 gamma4, f32x4 ext, float rs, bool ok) {
    // ALL arithmetic runs unconditionally (rows past M compute on clamped inputs) and only the stores sit under
    // `ok`: with the math inside the guard every guarded block was the first user of a pending load (bias, residual
    // row) on SOME path, so hipcc put `s_waitcnt vmcnt(0)` in front of each of them -- which also waits for the
    // previous block's STORE: 32 serialised HBM round trips per wave, ~10 us of a 256x256 tile's epilogue.
    const VlmoEpilogue& e = p.e;
    v += bias4;
    // wave-uniform 64-bit row base (scalar unit) + 32-bit in-tile offset: a per-lane 64-bit
    // multiply-add per store costs 4x a plain VALU op
    // (global_* saddr form: SGPR base + zero-extended 32-bit VGPR byte offset)
    const int gm = gmb + row;
    const RowAddr o{(size_t)gmb * e.ldo, (uint32_t)(row * e.ldo + gn)};
    const RowAddr o2{(size_t)gmb * e.ld2, (uint32_t)(row * e.ld2 + gn)};
    if constexpr (EPI == VLMO_EPI_BIAS) {
        const float lo = (e.relu & 1) ? 0.f : -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], lo);
        pin4(v);
        if (ok) store4<T>(o.at<T>(e.out), v[0], v[1], v[2], v[3]);
    } else if constexpr (EPI == VLMO_EPI_F32) {
        if (e.beta != 0.f) v += e.beta * ext;
        pin4(v);
        if (ok) *(f32x4*)o.at<float>(e.out) = v;
    } else if constexpr (EPI == VLMO_EPI_BIAS_GELU) {
        f32x4 h;
        if (GD >= 0 ? GD != 0 : (e.relu & 4) != 0) {
            // `out` receives d h / d u = GELU'(u) * dropout mask / (1 - p) instead of the pre-activation u: the backward's
            // GELU-derivative epilogue (VLMO_EPI_DGELU with the same bit) is then ONE multiply per element -- no erf, no
            // exponential, no dropout hash (27.8 -> ~6 vector instructions per element there for ~5 more here: the
            // Gaussian and the normal CDF are shared with GELU itself)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float u = v[j], ee = gauss_from(u), cdf = norm_cdf_from(u, ee);
                h[j] = u * cdf;
                v[j] = fmaf(u * 0.39894228040143268f, ee, cdf);
            }
            if (e.drop_thresh) {
                const uint64_t bits = drop_bits4(e.seed, ((uint64_t)gm * p.N + gn) >> 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float m = drop_keep(bits, j, e.drop_thresh) ? e.inv_keep : 0.f;
                    h[j] *= m;
                    v[j] *= m;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = gelu_erf(v[j]);
            if (e.drop_thresh) {
                const uint64_t bits = drop_bits4(e.seed, ((uint64_t)gm * p.N + gn) >> 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) h[j] = drop_keep(bits, j, e.drop_thresh) ? h[j] * e.inv_keep : 0.f;
            }
        }
        pin4(v);
        pin4(h);
        if (ok) {
            store4<T>(o.at<T>(e.out), v[0], v[1], v[2], v[3]);   // u (pre-activation)
            store4<T>(o2.at<T>(e.out2), h[0], h[1], h[2], h[3]);
        }
    } else if constexpr (EPI == VLMO_EPI_RESID) {
        if (e.drop_thresh) {
            const uint64_t bits = drop_bits4(e.seed, ((uint64_t)gm * p.N + gn) >> 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = drop_keep(bits, j, e.drop_thresh) ? v[j] * e.inv_keep : 0.f;
        }
        f32x4 x2 = ext + gamma4 * v * rs;
        pin4(v);
        pin4(x2);
        if (ok) {
            if (e.out2) store4<T>(o2.at<T>(e.out2), v[0], v[1], v[2], v[3]);
            *(f32x4*)o.at<float>(e.out) = x2;
        }
    } else if constexpr (EPI == VLMO_EPI_DUAL) {
        // dVAE EncoderBlock tail (dall_e/encoder.py:45-46): out = id + post_gain * res ; out2 = relu(out)
        v = v * e.beta + ext;
        pin4(v);
        if (ok) {
            store4<T>(o.at<T>(e.out), v[0], v[1], v[2], v[3]);
            if (e.out2)
                store4<T>((T*)e.out2 + (size_t)gm * e.ld2 + gn, fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f),
                          fmaxf(v[3], 0.f));
        }
    } else if constexpr (EPI == VLMO_EPI_CE_BWD) {
        // d(cross-entropy)/d(logits) of row gm, recomputed from the logits instead of read back: (softmax - onehot) *
        // row scale (heads.py:86-112 + objectives.py:57-68,571-582).  resid = lse [M], row_scale = dloss / n_valid per
        // row (0 on ignored rows), row_index = labels [M]
        const int gmc = min(gm, p.M - 1);
        const float lse = e.resid[gmc], sc = e.row_scale[gmc];
        const int lab = e.row_index[gmc];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = (__builtin_amdgcn_exp2f((v[j] - lse) * 1.4426950408889634f) - (gn + j == lab ? 1.f : 0.f)) * sc;
        pin4(v);
        if (ok) store4<T>(o.at<T>(e.out), v[0], v[1], v[2], v[3]);
    } else if constexpr (EPI == VLMO_EPI_DGELU) {
        if (GD >= 0 ? GD != 0 : (e.relu & 4) != 0) {
            v *= ext;       // aux holds GELU'(u) * mask / (1 - p), written by the forward's VLMO_EPI_BIAS_GELU with the same bit
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= gelu_erf_grad(ext[j]);
            if (e.drop_thresh) {
                const uint64_t bits = drop_bits4(e.seed, ((uint64_t)gm * p.N + gn) >> 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = drop_keep(bits, j, e.drop_thresh) ? v[j] * e.inv_keep : 0.f;
            }
        }
        pin4(v);
        if (ok) store4<T>(o.at<T>(e.out), v[0], v[1], v[2], v[3]);
    }
    return v;
}

// the row segment an epilogue needs from global memory besides the accumulators (clamped row: always valid)
template <typename T, int EPI>
__device__ __forceinline__ f32x4 epilogue_ext(const GemmNT& p, int gmb, int rowc, int gnc) {
    const VlmoEpilogue& e = p.e;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const RowAddr o{(size_t)gmb * e.ldo, (uint32_t)(rowc * e.ldo + gnc)};
    const RowAddr o2{(size_t)gmb * e.ld2, (uint32_t)(rowc * e.ld2 + gnc)};
    if constexpr (EPI == VLMO_EPI_RESID) {
        return NT_LD((const f32x4*)o.at<float>(e.resid));
    } else if constexpr (EPI == VLMO_EPI_DGELU) {
        return load4<T>(o2.at<T>(e.aux));
    } else if constexpr (EPI == VLMO_EPI_DUAL) {
        return e.resid ? load4<T>(o.at<T>(e.resid)) : z;
    } else if constexpr (EPI == VLMO_EPI_F32) {
        return e.beta != 0.f ? *(const f32x4*)o.at<float>(e.out) : z;
    } else {
        return z;
    }
}

// The rebuilt pointer is typed GLOBAL before it decays to a generic one: an integer -> generic pointer would make every
// access through it a FLAT instruction (which counts on vmcnt AND lgkmcnt, so each epilogue store was followed by
// `s_waitcnt vmcnt(0) lgkmcnt(0)` before the next LDS access: ~10 us of serialised store round trips per 256x256 tile).
__device__ __forceinline__ const void* uniform_ptr(const void* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const void*)(const __attribute__((address_space(1))) void*)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniform_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// bijective XCD-chunked remap: workgroups that share an XCD (bid % 8 equal)
// get a contiguous range of logical tile ids, so the A row-panel re-reads of
// neighbouring column tiles hit that XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + (bid >> 3);
}

// K-tile depth BK (64 or 32): BK=32 halves the LDS ring (32 KB for 128x128) so four workgroups
// fit a CU instead of two (more latency hiding, phases of co-resident workgroups decorrelate).
template <int BK> __device__ __forceinline__ int nt_swz(int row) {
    return BK == 64 ? ((row >> 1) & 7) : ((row >> 2) & 3);
}

template <typename T, int BM, int BN, int WM, int WN, int EPI, bool CONV, int BK, int NSTG, bool PP = false>
__global__ __launch_bounds__(WM * WN * 64, 2) void gemm_nt_kernel(const GemmNTGroups gp) {
    typedef typename Elem<T>::v8 v8;
    // two-segment reduction (vlmo_gemm_nt_2src): instantiated for the f16 (dVAE) kernels only -- the extra branch in the
    // staging step cost the bf16 256x128x32 kernels of the transformer (fc1, qkv) 8-10 %
    constexpr bool SEG2 = __is_same(T, f16) && !CONV;
    constexpr int NW = WM * WN;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int ROWB = BK * 2, CPR = ROWB / 16, SRPI = 1024 / ROWB, KS = BK / 16;
    constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE = A_BYTES + B_BYTES;
    constexpr int NA = BM / SRPI / NW, NB = BN / SRPI / NW;
    static_assert(BM % (SRPI * NW) == 0 && BN % (SRPI * NW) == 0, "tile/wave mismatch");
    static_assert(NW * 32 * TN * 32 * 4 <= NSTG * STAGE, "epilogue LDS must fit in the ring");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int lid_all = xcd_remap(blockIdx.x, gridDim.x);
    // (group, row origin, column origin) of a logical tile
    auto locate = [&](int la, int& gi_, int& m0_, int& n0_) {
        int g = 0;
#pragma unroll
        for (int q = 1; q < MAX_GROUPS; ++q)
            if (q < gp.ngroups && la >= gp.t0[q]) g = q;
        g = __builtin_amdgcn_readfirstlane(g);
        const GemmNT& r = gp.g[g];
        const int M_ = uniform_i(r.M), N_ = uniform_i(r.N);
        const int tiles_n = (N_ + BN - 1) / BN, tiles_m = (M_ + BM - 1) / BM;
        const int lid = la - uniform_i(gp.t0[g]);
        // grouped order: the ~64 tiles an XCD works on at once form a compact group_m x (64/group_m)
        // block, so their A row-panels AND B column-panels together fit the XCD's 4 MiB L2
        const int gmr = uniform_i(r.group_m);
        const int gm_ = gmr > 0 ? gmr : 1;
        const int per_group = gm_ * tiles_n;
        const int first_m = (lid / per_group) * gm_;
        const int gsz = min(tiles_m - first_m, gm_);
        const int in_g = lid % per_group;
        gi_ = g;
        m0_ = (first_m + in_g % gsz) * BM;
        n0_ = (in_g / gsz) * BN;
    };
    const T* a_src[NA];
    const T* b_src[NB];
    int a_yx[NA];            // CONV: (y << 16) | x of the staged output pixel
    // per-lane source addresses of the tile's operand rows (LDS-DMA: one 16-byte chunk per lane)
    auto point = [&](int gi_, int m0_, int n0_) {
        const GemmNT& r = gp.g[gi_];
        const T* A_ = (const T*)uniform_ptr(r.A);
        const T* B_ = (const T*)uniform_ptr(r.B);
        const int M_ = uniform_i(r.M), N_ = uniform_i(r.N), lda_ = uniform_i(r.lda), ldb_ = uniform_i(r.ldb);
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int rr = (i * NW + wave) * SRPI + lane / CPR;
            const int c = (lane % CPR) ^ nt_swz<BK>(rr);
            const int gr = min(m0_ + rr, M_ - 1);
            a_src[i] = A_ + (size_t)gr * lda_ + c * 8;
            if constexpr (CONV) {
                const int cH = uniform_i(r.cH), cW = uniform_i(r.cW);
                const int pix = gr % (cH * cW);
                a_yx[i] = ((pix / cW) << 16) | (pix % cW);
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int rr = (i * NW + wave) * SRPI + lane / CPR;
            const int c = (lane % CPR) ^ nt_swz<BK>(rr);
            const int gr = min(n0_ + rr, N_ - 1);
            b_src[i] = B_ + (size_t)gr * ldb_ + c * 8;
        }
    };
    int gi, m0, n0;
    locate(lid_all, gi, m0, n0);
    point(gi, m0, n0);
    GemmNT pl;
    const GemmNT* pp = &gp.g[gi];
    // the chosen problem, copied into SGPRs ONCE per group (see uniform_i): a dynamically indexed kernarg struct is
    // otherwise re-read with s_load + s_waitcnt at every use (115 scalar loads in the fc1 epilogue before this)
    auto hoist = [&](int gi_) {
        const GemmNT& gq = gp.g[gi_];
        {
            pl.A = uniform_ptr(gq.A), pl.B = uniform_ptr(gq.B), pl.zero = uniform_ptr(gq.zero);
            pl.M = uniform_i(gq.M), pl.N = uniform_i(gq.N), pl.K = uniform_i(gq.K), pl.lda = uniform_i(gq.lda), pl.ldb = uniform_i(gq.ldb);
            pl.cH = uniform_i(gq.cH), pl.cW = uniform_i(gq.cW), pl.cCin = uniform_i(gq.cCin), pl.ckw = uniform_i(gq.ckw);
            pl.group_m = uniform_i(gq.group_m);
            pl.A2 = uniform_ptr(gq.A2), pl.lda2 = uniform_i(gq.lda2), pl.k1 = uniform_i(gq.k1), pl.seg_scale = uniform_f(gq.seg_scale);
            pl.e.out = (void*)uniform_ptr(gq.e.out), pl.e.out2 = (void*)uniform_ptr(gq.e.out2);
            pl.e.bias = (const float*)uniform_ptr(gq.e.bias), pl.e.gamma = (const float*)uniform_ptr(gq.e.gamma);
            pl.e.resid = (const float*)uniform_ptr(gq.e.resid), pl.e.row_scale = (const float*)uniform_ptr(gq.e.row_scale);
            pl.e.row_index = (const int32_t*)uniform_ptr(gq.e.row_index), pl.e.aux = uniform_ptr(gq.e.aux);
            pl.e.ldo = uniform_i(gq.e.ldo), pl.e.ld2 = uniform_i(gq.e.ld2), pl.e.relu = uniform_i(gq.e.relu);
            pl.e.drop_thresh = (uint32_t)uniform_i((int)gq.e.drop_thresh);
            pl.e.inv_keep = uniform_f(gq.e.inv_keep), pl.e.beta = uniform_f(gq.e.beta);
            pl.e.seed = (uint64_t)uniform_ptr((const void*)gq.e.seed);
            pl.e.colpart = (float*)uniform_ptr(gq.e.colpart);
            pp = &pl;
        }
    };
    hoist(gi);

    f32x16 acc[TM][TN];
    const int l31 = lane & 31, h = lane >> 5;
    const int swz = nt_swz<BK>(l31);
    const int a_row_off = (wm * (BM / WM) + l31) * ROWB;
    const int b_row_off = A_BYTES + (wn * (BN / WN) + l31) * ROWB;

    const int nk = pp->K / BK;       // the groups of a launch share N and K
    const int cpt = CONV ? (pp->cCin / BK) : 1, cpad = CONV ? (pp->ckw - 1) / 2 : 0;
    auto stage = [&](int buf, int kt) {
        char* s = smem + buf * STAGE;
        if constexpr (CONV) {
            const GemmNT& p = *pp;
            const int tap = kt / cpt, cc = kt - tap * cpt;
            const int dy = tap / p.ckw - cpad, dx = tap % p.ckw - cpad;
            const int delta = (dy * p.cW + dx) * p.cCin + cc * BK;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int y = (a_yx[i] >> 16) + dy, x = (a_yx[i] & 0xFFFF) + dx;
                const bool in = (unsigned)y < (unsigned)p.cH && (unsigned)x < (unsigned)p.cW;
                const T* src = in ? a_src[i] + delta : (const T*)p.zero;
                glds16(src, s + (i * NW + wave) * 1024);
            }
        } else {
            if (SEG2 && pp->k1 && kt * BK == pp->k1) {
                // second A segment: the same rows of A2, rebased so that `+ kt * BK` keeps addressing the reduction index
                const T* A2_ = (const T*)pp->A2;
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const int rr = (i * NW + wave) * SRPI + lane / CPR;
                    const int c = (lane % CPR) ^ nt_swz<BK>(rr);
                    const int gr = min(m0 + rr, pp->M - 1);
                    a_src[i] = A2_ + (size_t)gr * pp->lda2 + c * 8 - pp->k1;
                }
            }
#pragma unroll
            for (int i = 0; i < NA; ++i) glds16(a_src[i] + kt * BK, s + (i * NW + wave) * 1024);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) glds16(b_src[i] + kt * BK, s + A_BYTES + (i * NW + wave) * 1024);
    };
    auto compute = [&](const char* s) {
        v8 af[KS][TM], bf[KS][TN];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int coff = ((2 * ks + h) ^ swz) << 4;
#pragma unroll
            for (int i = 0; i < TM; ++i) af[ks][i] = *(const v8*)(s + a_row_off + i * 32 * ROWB + coff);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[ks][j] = *(const v8*)(s + b_row_off + j * 32 * ROWB + coff);
        }
        if constexpr (CONV && sizeof(T) == 2 && __is_same(T, f16)) {
            // ReLU on the INPUT (VlmoEpilogue.relu bit 1): the dVAE's residual path convolves relu(x) (encoder.py:21-29)
            // while the identity path and the max-pool take x itself, so the producer would have to write both; four
            // v_pk_max_f16 per fragment beside 4-8 MFMAs are cheaper than a second [B*H*W, C] tensor through HBM
            if (pp->e.relu & 2) {
                const v8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int i = 0; i < TM; ++i) af[ks][i] = __builtin_elementwise_max(af[ks][i], z);
            }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = Elem<T>::mfma(af[ks][i], bf[ks][j], acc[i][j]);
    };
    const GemmNT& p = *pp;
    // first K-tile of the second A segment: the first segment's partial sum takes its scale (EncoderBlock tail:
    // post_gain * res_path + id_path as ONE reduction over [conv_3 output | block input])
    auto seg_boundary = [&](int kt) {
        if constexpr (SEG2) {
            if (pp->k1 && kt * BK == pp->k1 && pp->seg_scale != 1.f) {
                const float sc = pp->seg_scale;
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int k = 0; k < 16; ++k) acc[i][j][k] *= sc;
            }
        }
    };
    // EncoderBlock tail (VLMO_EPI_DUAL, K = n_hid = 64 .. 512): the kernel is a read of the identity map and a write of the
    // output around a one-tile product; with the identity rows fetched in the epilogue passes (8 bytes per lane, 4 KB
    // per wave in flight) a CU pulled 11 GB/s.  All of a wave's identity segments are requested BEFORE the K loop
    // instead: they fly under the operand staging.
    constexpr bool PRE = (EPI == VLMO_EPI_DUAL) && !PP && !CONV;
    constexpr int PRE_LPR = TN * 8, PRE_RPI = 64 / PRE_LPR, PRE_NIT = 32 / PRE_RPI;
    typename Elem<T>::v4 pre[PRE ? TM : 1][PRE ? PRE_NIT : 1];
    if constexpr (PRE) {
        if (p.e.resid) {
            const int gn_ = n0 + wn * (BN / WN) + (lane % PRE_LPR) * 4;
            const int gnc_ = gn_ < p.N ? gn_ : 0;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int gmbc_ = min(m0 + wm * (BM / WM) + i * 32, p.M - 1);
#pragma unroll
                for (int it = 0; it < PRE_NIT; ++it) {
                    const int rowc_ = min(it * PRE_RPI + lane / PRE_LPR, p.M - 1 - gmbc_);
                    pre[i][it] = NT_LD((const typename Elem<T>::v4*)((const T*)p.e.resid + (size_t)(gmbc_ + rowc_) * p.e.ldo + gnc_));
                }
            }
        }
    }
    stage(0, 0);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;
    if constexpr (PP) {
        // Ping-pong schedule (8 waves, WM == 2): every K-tile is four segments separated by raw
        // s_barriers -- read fragments of k-half 0 | 16 MFMAs | read k-half 1 | 16 MFMAs -- and the
        // wm == 1 waves run ONE segment behind the wm == 0 waves (one extra barrier up front, one
        // at the end for wm == 0).  A SIMD hosts one wave of each group, so while one multiplies the
        // other reads LDS: the MFMA pipe and the LDS port are both busy all the time instead of
        // taking turns.  The LDS-DMA of tile t+1 is issued at the start of the first MFMA segment of
        // tile t (all reads of that buffer retired >= 1 barrier earlier) and waited for, by the
        // issuing wave, in its segment before the barrier that opens tile t+1 for the leading group.
        static_assert(NSTG == 2 && WM == 2 && KS == 4, "ping-pong schedule: 2 buffers, 2 row groups, BK = 64");
        v8 af[2][TM], bf[2][TN];
        auto read_half = [&](const char* s_, int hf) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int coff = ((2 * (2 * hf + q) + h) ^ swz) << 4;
#pragma unroll
                for (int i = 0; i < TM; ++i) af[q][i] = *(const v8*)(s_ + a_row_off + i * 32 * ROWB + coff);
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[q][j] = *(const v8*)(s_ + b_row_off + j * 32 * ROWB + coff);
            }
            if constexpr (CONV && sizeof(T) == 2 && __is_same(T, f16)) {
                if (pp->e.relu & 2) {       // ReLU on the convolution's input (see compute())
                    const v8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int q = 0; q < 2; ++q)
#pragma unroll
                        for (int i = 0; i < TM; ++i) af[q][i] = __builtin_elementwise_max(af[q][i], z);
                }
            }
        };
        auto mfma_half = [&]() {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = Elem<T>::mfma(af[q][i], bf[q][j], acc[i][j]);
            __builtin_amdgcn_s_setprio(0);
        };
        auto bar = [&]() {      // raw barrier: no vmcnt drain; nothing may be scheduled across it
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        };
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (wm == 1) bar();
        for (int kt = 0; kt < nk; ++kt) {
            const char* cur = smem + (kt & 1) * STAGE;
            const bool more = kt + 1 < nk;
            seg_boundary(kt);
            read_half(cur, 0);
            // the LDS-DMA of the next K-tile goes out in the READ segment, behind the fragment reads (round 4: in-kernel
            // stamps showed the eight DMA instructions' issue time -- ~400 cycles -- in front of the wave's own MFMAs when
            // they were issued at the head of the MFMA segment; here it runs beside the partner wave's MFMA segment.  The
            // other buffer was last read two segments ago by this group and one segment ago by the other, each behind
            // lgkmcnt(0) + barrier.)  3 273 -> 2 776 cycles per K-tile in the stamped build, +4..9 % per GEMM.
            if (more) stage((kt + 1) & 1, kt + 1);
            bar();
            mfma_half();
            bar();
            read_half(cur, 1);
            if (more && wm == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bar();
            mfma_half();
            if (more && wm == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bar();
        }
        if (wm == 0) bar();
    } else {
        static_assert(NSTG == 2, "two LDS buffers");
        // 2-deep ring: one K-tile in flight behind the one being multiplied
        for (int kt = 0; kt < nk; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
            seg_boundary(kt);
            compute(smem + (kt & 1) * STAGE);
        }
    }

    // ---- epilogue: accumulators -> wave-private LDS -> full-row segments ----
    __syncthreads();
    constexpr int ROWF = TN * 32;                 // floats per LDS row
    constexpr int LPR = TN * 8, RPI = 64 / LPR;   // lanes per row, rows per read instr
    float* ep = (float*)(smem + wave * (32 * ROWF * 4));
    const int rrow = lane / LPR, rcol = (lane % LPR) * 4;
    const int gn = n0 + wn * (BN / WN) + rcol;
    const bool col_ok = gn < p.N;
    const int gnc = col_ok ? gn : 0;
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f}, gamma4 = {1.f, 1.f, 1.f, 1.f};
    if (p.e.bias) bias4 = *(const f32x4*)(p.e.bias + gnc);
    if (EPI == VLMO_EPI_RESID && p.e.gamma) gamma4 = *(const f32x4*)(p.e.gamma + gnc);
    f32x4 csum = {0.f, 0.f, 0.f, 0.f};      // VLMO_EPI_DGELU: column sums of a 32-row block (fc1 bias gradient partials)
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        // issue this pass's global loads first: they fly while the accumulators go through LDS
        constexpr int NIT = 32 / RPI;
        const int gmb = __builtin_amdgcn_readfirstlane(m0 + wm * (BM / WM) + i * 32);
        const int gmbc = min(gmb, p.M - 1);      // edge tiles: a wave's rows may all lie past M
        f32x4 ext[NIT];
        float rs[NIT];
        int ridx[NIT];
        // the drop-path scale is a two-step lookup (token -> scale group -> scale): all index loads of the pass go out
        // first, then all dependent loads, instead of eight index -> wait -> scale round trips in a row
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int gmc = gmbc + min(it * RPI + rrow, p.M - 1 - gmbc);
            ridx[it] = (EPI == VLMO_EPI_RESID && p.e.row_scale && p.e.row_index) ? p.e.row_index[gmc] : gmc;
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int rowc = min(it * RPI + rrow, p.M - 1 - gmbc);
            if constexpr (PRE) {
                const typename Elem<T>::v4 q = pre[i][it];
                ext[it] = p.e.resid ? f32x4{(float)q[0], (float)q[1], (float)q[2], (float)q[3]} : f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                ext[it] = epilogue_ext<T, EPI>(p, gmbc, rowc, gnc);
            }
            rs[it] = (EPI == VLMO_EPI_RESID && p.e.row_scale) ? p.e.row_scale[ridx[it]] : 1.f;
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ep[((r & 3) + 8 * (r >> 2) + 4 * h) * ROWF + j * 32 + l31] = acc[i][j][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        f32x4 v[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) v[it] = *(const f32x4*)(ep + (it * RPI + rrow) * ROWF + rcol);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int row = it * RPI + rrow;
            const int gm = gmb + row;
            if constexpr (EPI == VLMO_EPI_ARGMAX) {
                // fused arg-max over the vocabulary (modeling_discrete_vae.py:246-248): per row, the best
                // (value, index) of this wave's ROWF columns -> partial[gm][chunk]; logits never reach HBM
                f32x4 vv = v[it] + bias4;
                float best = -INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gn + j < p.N && vv[j] > best) {
                        best = vv[j];
                        bi = gn + j;
                    }
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) {
                    const float ob = __shfl_xor(best, o, 64);
                    const int oi = __shfl_xor(bi, o, 64);
                    if (ob > best || (ob == best && oi < bi)) {
                        best = ob;
                        bi = oi;
                    }
                }
                // col_ok of the row's first lane = the wave's first column lies below N: a wave wholly past N (odd chunk
                // count under an even tile) has no chunk, its index would be the next row's chunk 0
                if ((lane % LPR) == 0 && gm < p.M && col_ok) {
                    const int chunk = (n0 + wn * (BN / WN)) / ROWF;
                    float* pv = (float*)p.e.out + ((size_t)gm * p.e.ldo + chunk) * 2;
                    pv[0] = best;
                    ((int*)pv)[1] = bi;
                }
            } else if constexpr (EPI == VLMO_EPI_CE) {
                // fused cross-entropy forward: per row and 64-column chunk {max, sum exp(x - max), arg-max, logit of
                // the row's label or -inf}; the [n, vocabulary] logits never reach HBM.  row_index = labels
                f32x4 vv = v[it] + bias4;
                const int lab = (gm < p.M) ? p.e.row_index[gm] : -1;
                float best = -INFINITY, labv = -INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gn + j < p.N) {
                        if (vv[j] > best) {
                            best = vv[j];
                            bi = gn + j;
                        }
                        if (gn + j == lab) labv = vv[j];
                    }
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) {
                    const float ob = __shfl_xor(best, o, 64);
                    const int oi = __shfl_xor(bi, o, 64);
                    if (ob > best || (ob == best && oi < bi)) {
                        best = ob;
                        bi = oi;
                    }
                    labv = fmaxf(labv, __shfl_xor(labv, o, 64));
                }
                float se = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gn + j < p.N) se += __builtin_amdgcn_exp2f((vv[j] - best) * 1.4426950408889634f);
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) se += __shfl_xor(se, o, 64);
                if ((lane % LPR) == 0 && gm < p.M && col_ok) {      // as above: no chunk for a wave wholly past N
                    const int chunk = (n0 + wn * (BN / WN)) / ROWF;
                    float* pv = (float*)p.e.out + ((size_t)gm * p.e.ldo + chunk) * 4;
                    pv[0] = best;
                    pv[1] = se;
                    ((int*)pv)[2] = bi;
                    pv[3] = labv;
                }
            } else {
                const bool ok = gm < p.M && col_ok;
                const f32x4 w = epilogue4<T, EPI>(p, gmb, row, gn, v[it], bias4, gamma4, ext[it], rs[it], ok);
                if constexpr (EPI == VLMO_EPI_DGELU) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) csum[j] += ok ? w[j] : 0.f;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if constexpr (EPI == VLMO_EPI_DGELU) {
            // column sums of du per 32-row block (one epilogue pass of one wave) -> colpart[block][N]: the fc1 bias gradient
            // is their fold, done with the other column folds of the block instead of a second pass over [M, hidden]
            if (p.e.colpart) {
#pragma unroll
                for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
                    for (int j = 0; j < 4; ++j) csum[j] += __shfl_xor(csum[j], o, 64);
                // colpart has one row per 16 output rows (the 16x16x32 kernels place their passes at multiples of 16):
                // this 32-row pass owns two of them, the sums go to the first, zeros to the second
                const int blk = gmb >> 4;
                if (lane < LPR && col_ok && gmb < p.M) {
                    *(f32x4*)(p.e.colpart + (size_t)blk * p.N + gn) = csum;
                    if (gmb + 16 < p.M) *(f32x4*)(p.e.colpart + (size_t)(blk + 1) * p.N + gn) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                csum = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
}

// EMASK: bit e set = epilogue e is instantiated for this tile shape (every instantiation costs build time and code size)
template <typename T, int BM, int BN, int WM, int WN, bool CONV = false, int BK = 64, int NSTG = 2, bool PP = false,
          unsigned EMASK = 0xFFFFFFFFu>
int launch_nt(int epi, GemmNTGroups& p, hipStream_t st) {
    int tiles = 0;
    for (int q = 0; q < p.ngroups; ++q) {
        p.t0[q] = tiles;
        tiles += ((p.g[q].M + BM - 1) / BM) * ((p.g[q].N + BN - 1) / BN);
    }
    for (int q = p.ngroups; q <= MAX_GROUPS; ++q) p.t0[q] = tiles;
    constexpr int LDS = NSTG * (BM + BN) * BK * 2;
    dim3 grid(tiles), block(WM * WN * 64);
#define VLMO_LAUNCH_EPI(E)                                                                     \
    case E:                                                                                    \
    if constexpr (((EMASK >> E) & 1u) == 0) {                                                  \
        known = false;                                                                         \
    } else {                                                                                   \
        auto k = gemm_nt_kernel<T, BM, BN, WM, WN, E, CONV, BK, NSTG, PP>;                                        \
        if (LDS > 65536) {                                                                     \
            static DeviceOnce attr_set;        /* per kernel instantiation AND per device */      \
            if (attr_set.first())                                                              \
                (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS); \
        }                                                                                      \
        hipLaunchKernelGGL(k, grid, block, LDS, st, p);                                        \
    } break;
    bool known = true;
    switch (epi) {
        VLMO_LAUNCH_EPI(VLMO_EPI_BIAS)
        VLMO_LAUNCH_EPI(VLMO_EPI_F32)
        VLMO_LAUNCH_EPI(VLMO_EPI_DUAL)
        default:
            if constexpr (!CONV) {
                switch (epi) {
                    VLMO_LAUNCH_EPI(VLMO_EPI_BIAS_GELU)
                    VLMO_LAUNCH_EPI(VLMO_EPI_RESID)
                    VLMO_LAUNCH_EPI(VLMO_EPI_DGELU)
                    VLMO_LAUNCH_EPI(VLMO_EPI_ARGMAX)
                    VLMO_LAUNCH_EPI(VLMO_EPI_CE)
                    VLMO_LAUNCH_EPI(VLMO_EPI_CE_BWD)
                    default:
                        known = false;
                }
            } else {
                known = false;
            }
    }
    if (!known) {
        vlmo_set_error("vlmo_gemm_nt/conv: unsupported epilogue %d", epi);
        return -1;
    }
#undef VLMO_LAUNCH_EPI
    VLMO_CHECK_LAUNCH("vlmo_gemm_nt");
    return 0;
}

}  // namespace

// ---- optional in-library timing of GEMM launches (bench.py's roofline): HIP event pairs recorded on the
// launch stream around every vlmo_gemm_nt / vlmo_gemm_tn / vlmo_conv2d_nhwc while profiling is on.  One registry
// for all units, defined in gemm_nt.hip with vlmo_profile_start / vlmo_profile_stop (which list the tags).
namespace vlmo_prof {
struct ProfRec;
struct ProfScope {
    ProfRec* r = nullptr;
    hipStream_t st;
    ProfScope(int tag, double flops, hipStream_t s);
    ~ProfScope();
};
}  // namespace vlmo_prof
using vlmo_prof::ProfScope;

// gemm_nt16.hip: launch the 16x16x32 kernel of tile height 16 * h16 (h16 = 9 .. 20, bf16).  C linkage because
// GemmNTGroups is in the anonymous namespace (its name is part of every kernel symbol): a C++ function taking it can
// only be defined in the unit that calls it.
extern "C" __attribute__((visibility("hidden"))) int launch_nt16_height(int h16, int epi, GemmNTGroups& gp,
                                                                        hipStream_t stream);
