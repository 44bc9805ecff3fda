// gemm_tn: C[N1,N2] += A[M,N1]^T . B[M,N2] (reduction over rows) = the weight gradients: gemm_tn_kernel (split over the
// grid, fp32 atomics or slab + tn_reduce_kernel) and gemm_tn_multi_kernel (several problems in one launch).
#include "gemm_common.h"
#include "tn_multi_plan.h"

namespace {

// ------------------------------------------------------------------ wgrad ---
struct GemmTN {
    const void* A;   // [M, lda], uses columns [0, N1)
    const void* B;   // [M, ldb], uses columns [0, N2)
    float* C;        // [N1, ldc] fp32, atomically accumulated
    int M, N1, N2, lda, ldb, ldc;
    int kt_per_split, tiles;
    float alpha;
    float* slab;     // [splits, N1, N2] fp32 partial products (plain stores) or NULL (see mode)
    int mode;        // without a slab: TN_ATOMIC = fp32 atomics into C, TN_ACCUM = C += alpha * acc (this workgroup
                     // owns the tile: no K split), TN_STORE = C = alpha * acc
};

// 256 zero bytes: the staging source of token rows past the end of the reduction dimension
__device__ __attribute__((aligned(256))) char tn_zero_page[256];

// dual-use 256-byte-row image: chunk swizzle serving the transposed reads
__device__ __forceinline__ int tn_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// Output tile BM x BN (multiples of 128) per workgroup of WM x WN waves; each operand's K-tile (64 token rows)
// is staged as BM/128 resp. BN/128 side-by-side sub-images of [64 rows][128 columns] in the dual-use swizzle.
// PP (the ping-pong kernel): the reduction is staged in 32-token SLICES through a ring of four 32 KB slots instead of
// 64-token tiles through two 64 KB buffers.  The reduction index of this kernel is the ROW of both operands, so a slice
// is still made of whole 256-byte row pieces (the NT kernel cannot do this: its K runs along the rows, half a K-tile is
// half of every cache line).  Slice h + 3 is issued in the read segment of slice h -- four DMA instructions per wave
// and segment instead of eight in every other one -- and waited for with a counted vmcnt that leaves two slices in flight.
template <typename T, int BM, int BN, int WM, int WN, bool PP = false>
__device__ __forceinline__ void gemm_tn_body(const GemmTN& p, const int lid) {
    typedef typename Elem<T>::v8 v8;
    typedef typename Elem<T>::v4 v4;
    constexpr int NW = WM * WN;
    constexpr int SROWS = PP ? 32 : 64;                 // token rows per staged unit
    constexpr int SUB = SROWS * 256;                    // one sub-image
    constexpr int NSA = BM / 128, NSB = BN / 128;
    constexpr int A_BYTES = NSA * SUB, STAGE = (NSA + NSB) * SUB;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int IPS = SROWS / 4;                      // LDS-DMA instructions per sub-image and staged unit
    constexpr int IA = NSA * IPS / NW, IB = NSB * IPS / NW;   // ... per wave
    static_assert((NSA * IPS) % NW == 0 && (NSB * IPS) % NW == 0, "tile/wave mismatch");
    static_assert(!PP || IA + IB == 4, "slice ring: four DMA instructions per wave and slice");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    // 1-D grid of splits x tiles, remapped so that the workgroups one XCD runs are consecutive
    // (split-major): the ~32 tiles of one K-split share that split's token rows through the XCD's L2
    const int tiles_n = (p.N2 + BN - 1) / BN;
    const int split = lid / p.tiles, tile = lid - split * p.tiles;
    const int n1_0 = (tile / tiles_n) * BM, n2_0 = (tile % tiles_n) * BN;
    const int nk_total = (p.M + 63) >> 6;
    const int kt0 = split * p.kt_per_split;
    const int kt1 = min(nk_total, kt0 + p.kt_per_split);
    if (kt0 >= kt1) return;

    // staging: one wave-instruction = 4 rows x 256 B of one sub-image; 16 instructions per sub-image
    int a_off[IA], b_off[IB], a_row[IA], b_row[IB];
#pragma unroll
    for (int i = 0; i < IA; ++i) {
        const int ii = i * NW + wave, sub = ii / IPS, row = (ii % IPS) * 4 + (lane >> 4);
        const int ch = (lane & 15) ^ tn_swz(row);
        a_row[i] = row;
        a_off[i] = min(n1_0 + sub * 128 + ch * 8, p.N1 - 8);
    }
#pragma unroll
    for (int i = 0; i < IB; ++i) {
        const int ii = i * NW + wave, sub = ii / IPS, row = (ii % IPS) * 4 + (lane >> 4);
        const int ch = (lane & 15) ^ tn_swz(row);
        b_row[i] = row;
        b_off[i] = min(n2_0 + sub * 128 + ch * 8, p.N2 - 8);
    }
    // Full units go out in the buffer form of the LDS-DMA (common.h BufSrc): descriptor + scalar unit offset + one fixed 32-bit
    // lane offset, no vector instruction and no scalar load in front of the DMA.  (The pointer form below computed a 64-bit
    // multiply-add per instruction, selected the zero page under a divergent exec mask and fetched that page's address
    // through the GOT with s_load + s_waitcnt lgkmcnt(0) -- which also waited for the fragment reads just issued: ~450
    // cycles per staging call in the stamped build.)  The ragged last unit keeps the pointer form.
    const bool fits32 = (uint64_t)p.M * (uint64_t)max(p.lda, p.ldb) * 2 < 0x7FFFFFFFull;
    BufSrc a_rs, b_rs;
    a_rs.init(p.A);
    b_rs.init(p.B);
    uint32_t a_vo[IA], b_vo[IB];
#pragma unroll
    for (int i = 0; i < IA; ++i) a_vo[i] = (uint32_t)(a_row[i] * p.lda + a_off[i]) * 2u;
#pragma unroll
    for (int i = 0; i < IB; ++i) b_vo[i] = (uint32_t)(b_row[i] * p.ldb + b_off[i]) * 2u;
    // kt: index of the staged unit (64-token K-tile, or 32-token slice with PP)
    auto stage = [&](int buf, int kt) {
        char* s = smem + buf * STAGE;
        if (PP && fits32 && (kt + 1) * SROWS <= p.M) {
            const int sa = kt * SROWS * p.lda * 2, sb = kt * SROWS * p.ldb * 2;
#pragma unroll
            for (int i = 0; i < IA; ++i) a_rs.load16(s + (i * NW + wave) * 1024, a_vo[i], sa);
#pragma unroll
            for (int i = 0; i < IB; ++i) b_rs.load16(s + A_BYTES + (i * NW + wave) * 1024, b_vo[i], sb);
            return;
        }
#pragma unroll
        for (int i = 0; i < IA; ++i) {
            // token rows past M (ragged last K-tile) are staged from a zero page: operand A is then exactly zero
            // there, so the K loop needs no masking (B keeps the clamped last row; 0 * finite = 0)
            const int gr = kt * SROWS + a_row[i];
            const T* src = gr < p.M ? (const T*)p.A + (size_t)gr * p.lda + a_off[i] : (const T*)tn_zero_page;
            glds16(src, s + (i * NW + wave) * 1024);
        }
#pragma unroll
        for (int i = 0; i < IB; ++i) {
            const int gr = min(kt * SROWS + b_row[i], p.M - 1);
            glds16((const T*)p.B + (size_t)gr * p.ldb + b_off[i], s + A_BYTES + (i * NW + wave) * 1024);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

    // transposed-read addressing (ds_read_b64_tr_b16): lane 4q+p of a 16-lane
    // group supplies row q, columns 4p..4p+3 of a 4x16 block
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3, h = lane >> 5;
    const int ncol_a = wm * (BM / WM) + 16 * (g & 1) + 4 * pp;   // + tile*32
    const int ncol_b = wn * (BN / WN) + 16 * (g & 1) + 4 * pp;

    // LDS byte offsets of this lane's transposed reads inside a K-tile image, loop-invariant: the k-step enters
    // additively (16 rows = 4096 B: an immediate offset of the ds_read), only (half, t) need their own register
    // because the chunk swizzle is an XOR.  tn_swz(16 ks + m0) == tn_swz(m0).
    int a_rd[2][TM], b_rd[2][TN];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int m0 = 8 * h + 4 * half + q;
        const int sw = tn_swz(m0);
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            const int na = ncol_a + t * 32;
            a_rd[half][t] = (na >> 7) * SUB + m0 * 256 + ((((na & 127) >> 3) ^ sw) << 4) + (na & 7) * 2;
        }
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            const int nb = ncol_b + t * 32;
            b_rd[half][t] = A_BYTES + (nb >> 7) * SUB + m0 * 256 + ((((nb & 127) >> 3) ^ sw) << 4) + (nb & 7) * 2;
        }
    }
    // fragments of one 16-row k-step ks of the K-tile in image s_.
    // In the ping-pong schedule the transposed reads are INLINE ASM: behind the ds_read_tr builtin hipcc (ROCm 7.2)
    // waits `vmcnt(0)` for every LDS-DMA in flight (the builtin carries no memory operand, so the waitcnt pass
    // assumes it reads what the DMA writes), which put the whole HBM latency of the next K-tile's staging in front
    // of the second read segment of every tile (2.3-3.0 us per K-tile where the plain-load NT kernel takes 1.7).
    // The schedule orders DMA and reads itself (counted vmcnt + barriers); the reads' results are consumed only
    // behind bar() = lgkmcnt(0) + s_barrier + sched_barrier.
    const uint32_t lds0 = (uint32_t)(uintptr_t)LDS_PTR(smem);
    auto tr_read = [&](const char* s_, int off, int imm) -> v4 {
        if constexpr (PP) {
            typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
            u32x2 r;
            const uint32_t addr = lds0 + (uint32_t)(s_ - smem) + (uint32_t)off;
            asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(imm));
            return __builtin_bit_cast(v4, r);
        } else {
            return lds_tr4<T>(s_ + off + imm);
        }
    };
    auto read_step = [&](const char* s_, int ks, v8* af, v8* bf) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                const v4 va = ks == 0 ? tr_read(s_, a_rd[half][t], 0) : ks == 1 ? tr_read(s_, a_rd[half][t], 4096)
                            : ks == 2 ? tr_read(s_, a_rd[half][t], 8192) : tr_read(s_, a_rd[half][t], 12288);
#pragma unroll
                for (int e = 0; e < 4; ++e) af[t][4 * half + e] = va[e];
            }
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const v4 vb = ks == 0 ? tr_read(s_, b_rd[half][t], 0) : ks == 1 ? tr_read(s_, b_rd[half][t], 4096)
                            : ks == 2 ? tr_read(s_, b_rd[half][t], 8192) : tr_read(s_, b_rd[half][t], 12288);
#pragma unroll
                for (int e = 0; e < 4; ++e) bf[t][4 * half + e] = vb[e];
            }
        }
    };
    if constexpr (PP) {
        static_assert(WM == 2, "ping-pong schedule needs two row groups");
        v8 af[2][TM], bf[2][TN];
        auto mfma_half = [&]() {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = Elem<T>::mfma(af[u][i], bf[u][j], acc[i][j]);
            __builtin_amdgcn_s_setprio(0);
        };
        auto bar = [&]() {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        };
        const int ns = 2 * (kt1 - kt0), s0 = 2 * kt0;       // slices of this workgroup
        // this wave's DMA of slice h + 1 has landed; slices h + 2 and h + 3 (four instructions each) may stay in flight
        auto wait_next = [&](int h) {
            if (h + 3 < ns) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if (h + 2 < ns) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        };
        stage(0, s0);
        stage(1, s0 + 1);
        if (ns > 2) stage(2, s0 + 2);
        wait_next(-1);
        __builtin_amdgcn_s_barrier();
        if (wm == 1) bar();
        for (int h_ = 0; h_ < ns; ++h_) {
            const char* cur = smem + (h_ & 3) * STAGE;
            read_step(cur, 0, af[0], bf[0]);
            read_step(cur, 1, af[1], bf[1]);
            // slot (h + 3) & 3 held slice h - 1: read by this group two segments ago, by the other one segment ago
            if (h_ + 3 < ns) stage((h_ + 3) & 3, s0 + h_ + 3);
            if (wm == 1 && h_ + 1 < ns) wait_next(h_);
            bar();
            mfma_half();
            if (wm == 0 && h_ + 1 < ns) wait_next(h_);
            bar();
        }
        if (wm == 0) bar();
    } else {
        stage(0, kt0);
        for (int kt = kt0; kt < kt1; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kt + 1 < kt1) stage((kt - kt0 + 1) & 1, kt + 1);
            const char* s = smem + ((kt - kt0) & 1) * STAGE;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                v8 af[TM], bf[TN];
                read_step(s, ks, af, bf);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = Elem<T>::mfma(af[i], bf[j], acc[i][j]);
            }
        }
    }
    // epilogue: lane = output column, register = output row: each half-wave
    // writes / adds 128 contiguous bytes
    const int l31 = lane & 31;
    if (!p.slab && p.mode == TN_ACCUM) {
        // in-place accumulate by the tile's only owner: all 16 loads of a 32x32 sub-tile are issued before the
        // first add (one HBM round trip per sub-tile; a load -> add -> store chain per element costs 128 of them,
        // ~200 us per workgroup in the first build of this kernel)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int gn = n2_0 + wn * (BN / WN) + j * 32 + l31;
                const int gm0 = n1_0 + wm * (BM / WM) + i * 32 + 4 * h;
                const bool okn = gn < p.N2;
                float old[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int gm = gm0 + (r & 3) + 8 * (r >> 2);
                    old[r] = (okn && gm < p.N1) ? p.C[(size_t)gm * p.ldc + gn] : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int gm = gm0 + (r & 3) + 8 * (r >> 2);
                    if (okn && gm < p.N1) p.C[(size_t)gm * p.ldc + gn] = old[r] + p.alpha * acc[i][j][r];
                }
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int gn = n2_0 + wn * (BN / WN) + j * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gm = n1_0 + wm * (BM / WM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (gm < p.N1 && gn < p.N2) {
                    float* c = p.C + (size_t)gm * p.ldc + gn;
                    if (p.slab)
                        p.slab[((size_t)split * p.N1 + gm) * p.N2 + gn] = acc[i][j][r];
                    else if (p.mode == TN_STORE)
                        *c = p.alpha * acc[i][j][r];
                    else
                        atomicAdd(c, p.alpha * acc[i][j][r]);
                }
            }
        }
}

template <typename T, int BM, int BN, int WM, int WN, bool PP = false>
__global__ __launch_bounds__(WM * WN * 64, 2) void gemm_tn_kernel(const GemmTN p) {
    gemm_tn_body<T, BM, BN, WM, WN, PP>(p, xcd_remap(blockIdx.x, gridDim.x));
}
// dynamic LDS of the 256x256 ping-pong tile (both kernels): the ring of four 32 KB slices
constexpr int TN_LDS_256 = 2 * 4 * 64 * 256;

// Up to MAX_TN_PROBS weight-gradient problems in ONE launch of 256x256 tiles (the four to six linears of one or
// two transformer blocks).  A single weight gradient of VLMo-Base has 9-36 output tiles, so on its own it needs a
// 7-way split of the token dimension (slabs + a reduction pass, or atomics) to occupy 256 CUs; the gradients of two
// blocks together have 216 tiles and need no split at all.  Workgroup b runs order[b], which the host plans
// (tn_multi_plan.h).
struct GemmTNMulti {
    GemmTN p[MAX_TN_PROBS];
    uint16_t order[MAX_TN_ORDER];
};
template <typename T>
__global__ __launch_bounds__(512, 2) void gemm_tn_multi_kernel(const GemmTNMulti mp) {
    const uint32_t code = mp.order[blockIdx.x];
    if (code == TN_NOP) return;
    int gi = (int)(code >> 12);
    const int lid_in = __builtin_amdgcn_readfirstlane((int)(code & 0xFFFu));
    gi = __builtin_amdgcn_readfirstlane(gi);
    // copy the chosen problem into SGPRs ONCE: a dynamically indexed kernarg struct is otherwise re-read with
    // s_load + s_waitcnt at every use inside the K loop (908 scalar loads in the first build of this kernel)
    const GemmTN& q = mp.p[gi];
    GemmTN p;
    p.A = uniform_ptr(q.A), p.B = uniform_ptr(q.B), p.C = (float*)uniform_ptr(q.C);
    p.M = __builtin_amdgcn_readfirstlane(q.M), p.N1 = __builtin_amdgcn_readfirstlane(q.N1);
    p.N2 = __builtin_amdgcn_readfirstlane(q.N2), p.lda = __builtin_amdgcn_readfirstlane(q.lda);
    p.ldb = __builtin_amdgcn_readfirstlane(q.ldb), p.ldc = __builtin_amdgcn_readfirstlane(q.ldc);
    p.kt_per_split = __builtin_amdgcn_readfirstlane(q.kt_per_split), p.tiles = __builtin_amdgcn_readfirstlane(q.tiles);
    p.alpha = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, q.alpha)));
    p.slab = nullptr;
    p.mode = __builtin_amdgcn_readfirstlane(q.mode);
    gemm_tn_body<T, 256, 256, 2, 4, true>(p, lid_in);
}

// C[r, c] += alpha * sum_s slab[s, r, c]   (one float4 per thread)
__global__ __launch_bounds__(256) void tn_reduce_kernel(const float* __restrict__ slab, int splits, int N1, int N2,
                                                        float* __restrict__ C, int ldc, float alpha) {
    const int n4 = N2 >> 2;
    const long total = (long)N1 * n4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int r = (int)(i / n4), c = (int)(i % n4) * 4;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int s2 = 0; s2 < splits; ++s2) a += *(const f32x4*)(slab + ((size_t)s2 * N1 + r) * N2 + c);
        f32x4* o = (f32x4*)(C + (size_t)r * ldc + c);
        *o = *o + alpha * a;
    }
}

// tile / split plan of the weight-gradient GEMM: 256x256 tiles (half the staged bytes per flop, one
// workgroup per CU) when they fill the chip in ONE dispatch round with <= 16 splits, else 128x128 tiles
// (two workgroups per CU) with the fewest splits that fill whole rounds of 512 workgroup slots.
struct TnPlan {
    int big, tiles, splits, per;
};
TnPlan tn_plan(int M, int N1, int N2, int splits_req, int force_tile) {
    const int nk = (M + 63) / 64;
    TnPlan pl{};
    const int t256 = ((N1 + 255) / 256) * ((N2 + 255) / 256);
    const int t128 = ((N1 + 127) / 128) * ((N2 + 127) / 128);
    const bool big_ok = N1 >= 256 && N2 >= 256 && nk >= 16 && t256 <= 256;
    pl.big = force_tile == 256 ? 1 : (force_tile == 128 ? 0 : (big_ok && (256 / t256) <= 16 && (256 / t256) >= 1 && nk / (256 / t256) >= 8));
    pl.tiles = pl.big ? t256 : t128;
    int splits = splits_req;
    if (splits <= 0) {
        if (pl.big) {
            splits = 256 / pl.tiles;
        } else {
            splits = 512 / pl.tiles;
            if (splits < 4) splits = 1024 / pl.tiles;
        }
        if (splits < 1) splits = 1;
    }
    if (splits > nk) splits = nk;
    pl.per = (nk + splits - 1) / splits;
    pl.splits = (nk + pl.per - 1) / pl.per;
    return pl;
}
}  // namespace

extern "C" int64_t vlmo_gemm_tn_ws_bytes(int M, int N1, int N2) {
    const TnPlan a = tn_plan(M, N1, N2, 0, 0);
    return (int64_t)a.splits * N1 * N2 * 4;
}

extern "C" int vlmo_gemm_tn(int dtype, const void* A, int lda, const void* B, int ldb, float* C, int ldc,
                            int M, int N1, int N2, float alpha, int splits, float* ws, int64_t ws_bytes,
                            hipStream_t stream) {
    VLMO_CHECK_ARG(A && B && C, "vlmo_gemm_tn: null operand");
    VLMO_CHECK_ARG(M > 0 && N1 >= 8 && N2 >= 8, "vlmo_gemm_tn: bad problem M=%d N1=%d N2=%d", M, N1, N2);
    VLMO_CHECK_ARG(N1 % 8 == 0 && N2 % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0, "vlmo_gemm_tn: N1,N2,lda,ldb must be multiples of 8");
    VLMO_CHECK_ARG(lda >= N1 && ldb >= N2 && ldc >= N2, "vlmo_gemm_tn: leading dimension too small");
    VLMO_CHECK_ARG(dtype == VLMO_BF16 || dtype == VLMO_F16, "vlmo_gemm_tn: dtype must be bf16 or f16");
    VLMO_CHECK_ARG(splits < 3000, "vlmo_gemm_tn: splits must be below 3000 (got %d)", splits);
    int force = 0;
    if (splits >= 1000) {      // test hook: 1000 + s forces 128x128 tiles, 2000 + s forces 256x256
        force = splits >= 2000 ? 256 : 128;
        splits %= 1000;
    }
    const TnPlan pl = tn_plan(M, N1, N2, splits, force);
    // partial products go to a caller-owned slab (plain stores, then one reduction pass) when the workspace is
    // big enough and there is more than one split; else straight into C with fp32 atomics.  Measured on MI355X:
    // 7 splits of a 3072x768 gradient as atomics cost ~30 us of a 135 us launch (memory-side atomic rate).
    const bool use_slab = ws && pl.splits > 1 && N2 % 4 == 0 && ldc % 4 == 0 && ws_bytes >= (int64_t)pl.splits * N1 * N2 * 4;
    GemmTN p{A, B, C, M, N1, N2, lda, ldb, ldc, pl.per, pl.tiles, alpha, use_slab ? ws : nullptr, TN_ATOMIC};
    dim3 grid(pl.tiles * pl.splits);
    ProfScope prof(64 + (pl.big ? 8 : 0), 2.0 * M * N1 * N2, stream);
    if (pl.big) {
        static DeviceOnce attr;
        if (attr.first()) {
            (void)hipFuncSetAttribute((const void*)gemm_tn_kernel<bf16, 256, 256, 2, 4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_256);
            (void)hipFuncSetAttribute((const void*)gemm_tn_kernel<f16, 256, 256, 2, 4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_256);
        }
        if (dtype == VLMO_F16)
            hipLaunchKernelGGL((gemm_tn_kernel<f16, 256, 256, 2, 4, true>), grid, dim3(512), TN_LDS_256, stream, p);
        else
            hipLaunchKernelGGL((gemm_tn_kernel<bf16, 256, 256, 2, 4, true>), grid, dim3(512), TN_LDS_256, stream, p);
    } else {
        if (dtype == VLMO_F16)
            hipLaunchKernelGGL((gemm_tn_kernel<f16, 128, 128, 2, 2>), grid, dim3(256), 65536, stream, p);
        else
            hipLaunchKernelGGL((gemm_tn_kernel<bf16, 128, 128, 2, 2>), grid, dim3(256), 65536, stream, p);
    }
    VLMO_CHECK_LAUNCH("vlmo_gemm_tn");
    if (use_slab) {
        const long total = (long)N1 * (N2 / 4);
        const int rg = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
        hipLaunchKernelGGL(tn_reduce_kernel, dim3(rg), dim3(256), 0, stream, ws, pl.splits, N1, N2, C, ldc, alpha);
        VLMO_CHECK_LAUNCH("vlmo_gemm_tn(reduce)");
    }
    return 0;
}

// Weight gradients of several linears in as few launches as plan_tn_multi (tn_multi_plan.h) makes of them: validate every
// problem, plan, then execute the plan.  Nothing is enqueued before the whole call is known to be good.
extern "C" int vlmo_gemm_tn_multi(int dtype, const VlmoTnProblem* probs, int n, hipStream_t stream) {
    VLMO_CHECK_ARG(probs && n >= 1, "vlmo_gemm_tn_multi: no problems");
    VLMO_CHECK_ARG(dtype == VLMO_BF16 || dtype == VLMO_F16, "vlmo_gemm_tn_multi: dtype must be bf16 or f16");
    for (int q = 0; q < n; ++q) {
        const VlmoTnProblem& r = probs[q];
        VLMO_CHECK_ARG(r.A && r.B && r.C, "vlmo_gemm_tn_multi: null operand in problem %d", q);
        VLMO_CHECK_ARG(r.M > 0 && r.N1 >= 8 && r.N2 >= 8 && r.N1 % 8 == 0 && r.N2 % 8 == 0 && r.lda % 8 == 0 &&
                           r.ldb % 8 == 0 && r.lda >= r.N1 && r.ldb >= r.N2 && r.ldc >= r.N2,
                       "vlmo_gemm_tn_multi: bad shape in problem %d (M=%d N1=%d N2=%d)", q, r.M, r.N1, r.N2);
    }
    const TnMultiPlan plan = plan_tn_multi(probs, n);
    VLMO_CHECK_ARG(plan.error.empty(), "%s", plan.error.c_str());
    static DeviceOnce attr;
    if (attr.first()) {
        (void)hipFuncSetAttribute((const void*)gemm_tn_multi_kernel<bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_256);
        (void)hipFuncSetAttribute((const void*)gemm_tn_multi_kernel<f16>, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_256);
    }
    for (const TnLaunchPlan& L : plan.launches) {
        GemmTNMulti mp{};
        double flops = 0;
        for (int q = 0; q < L.nq; ++q) {
            const VlmoTnProblem& r = probs[L.q0 + q];
            const VlmoTnProblemPlan& s = L.p[q];
            if (s.zero_first) {
                hipError_t rc = hipMemset2DAsync(r.C, (size_t)r.ldc * 4, 0, (size_t)r.N2 * 4, r.N1, stream);
                if (rc != hipSuccess) {
                    vlmo_set_error("vlmo_gemm_tn_multi: memset failed: %s", hipGetErrorString(rc));
                    return (int)rc;
                }
            }
            mp.p[q] = GemmTN{r.A, r.B, r.C, r.M, r.N1, r.N2, r.lda, r.ldb, r.ldc, s.kt_per_split, s.tiles, r.alpha, nullptr, s.mode};
            flops += 2.0 * r.M * r.N1 * r.N2;
        }
        std::copy(L.order, L.order + L.grid, mp.order);
        ProfScope prof(73, flops, stream);
        if (dtype == VLMO_F16)
            hipLaunchKernelGGL((gemm_tn_multi_kernel<f16>), dim3(L.grid), dim3(512), TN_LDS_256, stream, mp);
        else
            hipLaunchKernelGGL((gemm_tn_multi_kernel<bf16>), dim3(L.grid), dim3(512), TN_LDS_256, stream, mp);
        VLMO_CHECK_LAUNCH("vlmo_gemm_tn_multi");
    }
    return 0;
}

extern "C" int vlmo_gemm_tn_multi_plan(const VlmoTnProblem* probs, int n, int32_t* n_launches, int32_t* launch_q0,
                                       VlmoTnProblemPlan* prob, int32_t* grid, uint16_t* order) {
    VLMO_CHECK_ARG(probs && n >= 1, "vlmo_gemm_tn_multi: no problems");
    VLMO_CHECK_ARG(n_launches && launch_q0 && prob && grid && order, "vlmo_gemm_tn_multi_plan: null output");
    const TnMultiPlan plan = plan_tn_multi(probs, n);
    VLMO_CHECK_ARG(plan.error.empty(), "%s", plan.error.c_str());
    *n_launches = (int32_t)plan.launches.size();
    for (size_t k = 0; k < plan.launches.size(); ++k) {
        const TnLaunchPlan& L = plan.launches[k];
        launch_q0[k] = L.q0, launch_q0[k + 1] = L.q0 + L.nq;
        std::copy(L.p, L.p + L.nq, prob + L.q0);
        grid[k] = L.grid;
        std::copy(L.order, L.order + L.grid, order + k * MAX_TN_ORDER);
    }
    return 0;
}
