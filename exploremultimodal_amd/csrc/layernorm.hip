// LayerNorm forward/backward, one 64-lane wavefront per token row, fp32 math.
// Reference: LayerNorm factory vlmo.py:26-36 bound with eps=1e-12 at
// vlmo_module.py:21-23; used at vlmo.py:188,192 (norm1/norm2) and :413 (norm).
// HBM-bound: each row is read once (16 B/lane vector loads) and kept in
// registers for both the statistics and the normalisation.
#include "common.h"
#include "vlmo_hip.h"

namespace {

template <int VPL, bool OUT_F32>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ b, void* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                     const int32_t* __restrict__ rowmap, int M, int d, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = d >> 2;
    // weight and bias stay in registers for all rows of the wave; TWO rows are in flight per wave (both rows' loads are
    // issued before any arithmetic): the kernel is HBM-bound and a wave's bytes in flight are what it has to offer
    f32x4 ww[VPL], bb[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = min(lane + 64 * j, nv - 1);
        ww[j] = ((const f32x4*)w)[i];
        bb[j] = ((const f32x4*)b)[i];
    }
    const int stride = gridDim.x * 4;
    for (int m0 = blockIdx.x * 4 + wave; m0 < M; m0 += 2 * stride) {
        f32x4 v[2][VPL];
        int mr[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            mr[r] = m0 + r * stride;
            const f32x4* xr = (const f32x4*)(x + (size_t)min(mr[r], M - 1) * d);
#pragma unroll
            for (int j = 0; j < VPL; ++j) v[r][j] = xr[min(lane + 64 * j, nv - 1)];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int m = mr[r];
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < VPL; ++j)
                if (lane + 64 * j < nv) s += v[r][j][0] + v[r][j][1] + v[r][j][2] + v[r][j][3];
            const float mu = wave_sum(s) / d;
            float q = 0.f;
#pragma unroll
            for (int j = 0; j < VPL; ++j)
                if (lane + 64 * j < nv) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float t = v[r][j][k] - mu;
                        q += t * t;
                    }
                }
            const float rs = rsqrtf(wave_sum(q) / d + eps);
            if (m < M) {
                if (lane == 0) {
                    if (mean) mean[m] = mu;
                    if (rstd) rstd[m] = rs;
                }
                const int om = rowmap ? rowmap[m] : m;
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    const int i = lane + 64 * j;
                    f32x4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = (v[r][j][k] - mu) * rs * ww[j][k] + bb[j][k];
                    if (i < nv) {
                        if constexpr (OUT_F32) {
                            ((f32x4*)((float*)y + (size_t)om * d))[i] = o;
                        } else {
                            bf16x4 ob = {(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
                            ((bf16x4*)((bf16*)y + (size_t)om * d))[i] = ob;
                        }
                    }
                }
            }
        }
    }
}

// residual branch fed by the LayerNorm's input gradient (fused form): z = drop(branch) is what forward added as
// x + gamma * rs * z, so dz = mask * dx * gamma * rs, dgamma = sum dx * rs * z, dbias = sum dz  (resid_bwd_kernel)
struct ResidArgs {
    const bf16* zd;
    const float* gamma;
    const float* row_scale;
    const int32_t* row_index;
    bf16* dz;
    uint32_t thresh;
    float inv_keep;
    uint64_t seed;
    // rows [seg, M) form a second segment with its own dropout stream (seed1) whose counters restart at row seg:
    // the per-modality experts of a block below the fusion layer (their FFN residual branches were produced by
    // separate problems of a grouped GEMM).  seg = M: one segment.  No workgroup straddles the boundary, so the
    // column partials of the two segments are separate rows of the workspace: workgroups [0, nb0) work on segment 0
    // (ln_bwd_grid)
    int seg, nb0;
    uint64_t seed1;
};

// Row ring of ln_bwd_kernel: what a row needs from HBM waits in LDS, not in registers.  One slot = the row's dy, x,
// dres and zd pieces, each a linear copy of the global bytes filled by LDS-DMA (one wave-instruction = 1 KB: lane l
// brings bytes [16 l, 16 l + 16) of its KB; the lanes past a piece's end repeat the piece's last 16 bytes, which land
// in the padding up to the next whole KB).  The lane reads its vectors back at j * 1024 + 16 lane (fp32 pieces,
// ds_read_b128) or j * 512 + 8 lane (bf16 pieces, ds_read_b64).  tests/test_ln_ring_layout.py restates this on the host.
// A workgroup of 4 waves with two slots per wave stays within 80 KB (two workgroups per CU) up to VPL = 3, d <= 768:
// 10 KB per slot in the fused form.  VPL = 4 (d <= 1024) has 12 KB slots and one of them per wave, 48 KB; there the 64 KB
// of the column fold set the workgroup's LDS, as before.
template <int VPL, bool DY_F32, bool RESID> struct LnRing {
    static constexpr int HALF = ((VPL + 1) / 2) * 1024;      // a bf16 piece: whole LDS-DMA instructions
    static constexpr int FULL = VPL * 1024;                  // an fp32 piece
    static constexpr int DY = 0, X = DY_F32 ? FULL : HALF, DR = X + FULL, Z = DR + FULL;
    static constexpr int SLOT = Z + (RESID ? HALF : 0);
    static constexpr int NSLOT = (8 * SLOT <= 80 * 1024) ? 2 : 1;
    static constexpr int BYTES = 4 * NSLOT * SLOT;
    static constexpr int STORES = VPL * (RESID ? 2 : 1);     // vector stores per row: dx (, dz)
};

// s_waitcnt vmcnt(n), n wave-uniform (the instruction takes an immediate)
__device__ __forceinline__ void wait_vmcnt(int n) {
#define VLMO_VMCNT_CASE(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n) {
        VLMO_VMCNT_CASE(1) VLMO_VMCNT_CASE(2) VLMO_VMCNT_CASE(3) VLMO_VMCNT_CASE(4) VLMO_VMCNT_CASE(5) VLMO_VMCNT_CASE(6)
        VLMO_VMCNT_CASE(7) VLMO_VMCNT_CASE(8) VLMO_VMCNT_CASE(9) VLMO_VMCNT_CASE(10) VLMO_VMCNT_CASE(11) VLMO_VMCNT_CASE(12)
        VLMO_VMCNT_CASE(13) VLMO_VMCNT_CASE(14) VLMO_VMCNT_CASE(15) VLMO_VMCNT_CASE(16) VLMO_VMCNT_CASE(17) VLMO_VMCNT_CASE(18)
        VLMO_VMCNT_CASE(19) VLMO_VMCNT_CASE(20) VLMO_VMCNT_CASE(21) VLMO_VMCNT_CASE(22) VLMO_VMCNT_CASE(23) VLMO_VMCNT_CASE(24)
        VLMO_VMCNT_CASE(25) VLMO_VMCNT_CASE(26) VLMO_VMCNT_CASE(27) VLMO_VMCNT_CASE(28) VLMO_VMCNT_CASE(29) VLMO_VMCNT_CASE(30)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef VLMO_VMCNT_CASE
}

// A 32-bit word at a wave-uniform address through the scalar cache (read-only inputs only).  The pointers inside
// ResidArgs carry no no-alias promise, so hipcc reads through them with vector loads, and beside an LDS-DMA in flight it
// waits vmcnt(0) at the use of any vector load's result: the ring would drain once per row.
__device__ __forceinline__ uint32_t scalar_load32(const void* p) {
    uint32_t v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}

// one piece of a slot: NI LDS-DMA instructions over nb bytes (a multiple of 16) at src
template <int NI> __device__ __forceinline__ void ring_piece(const char* src, int nb, char* dst, int lane) {
#pragma unroll
    for (int jj = 0; jj < NI; ++jj) glds16(src + min(jj * 1024 + lane * 16, nb - 16), dst + jj * 1024);
}

template <int VPL, bool DY_F32, bool RESID>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const void* __restrict__ dy, const int32_t* __restrict__ rowmap,
                                                     const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ dres, float* __restrict__ dx,
                                                     float* __restrict__ ws, int M, int d, int rows_per_block,
                                                     const ResidArgs ra) {
    constexpr int NCOL = RESID ? 4 : 2;      // column partials per block: dw, db (, dgamma, dbias)
    typedef LnRing<VPL, DY_F32, RESID> Ring;
    constexpr int NSLOT = Ring::NSLOT;
    constexpr int RED_BYTES = 4 * NCOL * VPL * 256 * 4;
    // ONE LDS array: the row ring during the loop, the cross-wave fold of the column sums after it
    __shared__ __attribute__((aligned(16))) char smem[Ring::BYTES > RED_BYTES ? Ring::BYTES : RED_BYTES];
    float(*red)[NCOL][VPL * 256] = (float(*)[NCOL][VPL * 256]) smem;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nv = d >> 2;
    f32x4 aw[VPL], ab[VPL], ww[VPL], ag[VPL], az[VPL], gg[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        aw[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        ab[j] = ag[j] = az[j] = aw[j];
        const int i = lane + 64 * j;
        ww[j] = (i < nv) ? ((const f32x4*)w)[i] : aw[j];
        gg[j] = f32x4{1.f, 1.f, 1.f, 1.f};
        if (RESID && ra.gamma && i < nv) gg[j] = ((const f32x4*)ra.gamma)[i];
    }
    int r0 = blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
    uint64_t drop_seed = 0;
    int drop_row0 = 0;
    if constexpr (RESID) {
        drop_seed = ra.seed;
        if ((int)blockIdx.x < ra.nb0) {
            r1 = min(ra.seg, r0 + rows_per_block);
        } else {
            r0 = ra.seg + ((int)blockIdx.x - ra.nb0) * rows_per_block;
            r1 = min(M, r0 + rows_per_block);
            drop_seed = ra.seed1;
            drop_row0 = ra.seg;
        }
    }
    // Everything a row needs from HBM (dy, x, the incoming residual gradient, mean/rstd) is fetched AHEAD of the
    // arithmetic: beside the weight-gradient GEMMs of the side stream this kernel gets one or two waves per SIMD, so
    // its speed is (bytes in flight per wave) / latency, not occupancy.  The rows in flight wait in the wave's own ring
    // of NSLOT slots in LDS (LnRing): while row k is worked on, rows k + 1 .. k + NSLOT of the wave (4 apart in the
    // matrix) are on their way.  No barrier in the loop: a slot is written and read by one wave only.
    struct Row {
        f32x4 dy[VPL], x[VPL], dr[VPL];
        bf16x4 z[VPL];
        float mu, rs, scale;
    };
    char* const ring = smem + wave * (NSLOT * Ring::SLOT);
    // LDS-DMA instructions of one row's fetch
    const int nfetch = (DY_F32 ? VPL : (VPL + 1) / 2) + VPL + (dres ? VPL : 0) + (RESID ? (VPL + 1) / 2 : 0);
    float mu_s[NSLOT], rs_s[NSLOT], sc_s[NSLOT];
    auto fetch = [&](int m, int s) {
        const int sm = rowmap ? rowmap[m] : m;
        mu_s[s] = mean[m];
        rs_s[s] = rstd[m];
        sc_s[s] = 1.f;
        if constexpr (RESID) {
            if (ra.row_scale) {
                const int ri = ra.row_index ? (int)scalar_load32(ra.row_index + m) : m;
                sc_s[s] = __builtin_bit_cast(float, scalar_load32(ra.row_scale + ri));
            }
        }
        char* slot = ring + s * Ring::SLOT;
        if constexpr (DY_F32)
            ring_piece<VPL>((const char*)dy + (size_t)sm * d * 4, 4 * d, slot + Ring::DY, lane);
        else
            ring_piece<(VPL + 1) / 2>((const char*)dy + (size_t)sm * d * 2, 2 * d, slot + Ring::DY, lane);
        ring_piece<VPL>((const char*)(x + (size_t)m * d), 4 * d, slot + Ring::X, lane);
        if (dres) ring_piece<VPL>((const char*)(dres + (size_t)m * d), 4 * d, slot + Ring::DR, lane);
        if constexpr (RESID) ring_piece<(VPL + 1) / 2>((const char*)(ra.zd + (size_t)m * d), 2 * d, slot + Ring::Z, lane);
    };
    const int m0 = r0 + wave;
    const int nrow = m0 < r1 ? (r1 - m0 + 3) >> 2 : 0;      // rows of this wave: m0 + 4 k
#pragma unroll
    for (int s = 0; s < NSLOT; ++s)
        if (s < nrow) fetch(m0 + 4 * s, s);
    for (int k0 = 0; k0 < nrow; k0 += NSLOT)
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        const int kr = k0 + s, m = m0 + 4 * kr;      // row kr of the wave
        if (kr >= nrow) break;
        // Wait for row kr's slot only.  The vector-memory operations issued AFTER its fetch, all of which may stay in
        // flight: the fetches of rows kr + 1 .. kr + NSLOT - 1 (those that exist) and the stores of the min(kr, NSLOT)
        // rows before kr (a row's fetch is issued ahead of the arithmetic of the row NSLOT before it).
        // (gfx9: loads, LDS-DMA and stores share vmcnt and retire in issue order.)
        int younger = min(kr, NSLOT) * Ring::STORES;
#pragma unroll
        for (int t = 1; t < NSLOT; ++t)
            if (kr + t < nrow) younger += nfetch;
        wait_vmcnt(younger);
        Row cur;
        cur.mu = mu_s[s], cur.rs = rs_s[s], cur.scale = sc_s[s];
        {
            const char* slot = ring + s * Ring::SLOT;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {      // lanes without a column read padding and never use it
                if constexpr (DY_F32) {
                    cur.dy[j] = *(const f32x4*)(slot + Ring::DY + j * 1024 + lane * 16);
                } else {
                    const bf16x4 t = *(const bf16x4*)(slot + Ring::DY + j * 512 + lane * 8);
                    cur.dy[j] = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
                }
                cur.x[j] = *(const f32x4*)(slot + Ring::X + j * 1024 + lane * 16);
                cur.dr[j] = dres ? *(const f32x4*)(slot + Ring::DR + j * 1024 + lane * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (RESID) cur.z[j] = *(const bf16x4*)(slot + Ring::Z + j * 512 + lane * 8);
            }
        }
        // the slot is free once its reads have returned
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (kr + NSLOT < nrow) fetch(m + 4 * NSLOT, s);
        const float mu = cur.mu, rs = cur.rs;
        f32x4 g[VPL], xh[VPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int i = lane + 64 * j;
            if (i < nv) {
                const f32x4 dyv = cur.dy[j], xv = cur.x[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    xh[j][k] = (xv[k] - mu) * rs;
                    g[j][k] = dyv[k] * ww[j][k];
                    s1 += g[j][k];
                    s2 += g[j][k] * xh[j][k];
                    aw[j][k] += dyv[k] * xh[j][k];
                    ab[j][k] += dyv[k];
                }
            } else {
                g[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                xh[j] = g[j];
            }
        }
        const float c1 = wave_sum(s1) / d, c2 = wave_sum(s2) / d;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int i = lane + 64 * j;
            if (i < nv) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = rs * (g[j][k] - c1 - xh[j][k] * c2);
                if (dres) o += cur.dr[j];
                ((f32x4*)(dx + (size_t)m * d))[i] = o;
                if constexpr (RESID) {
                    const f32x4 orr = o * cur.scale;
                    f32x4 v = o * gg[j] * cur.scale;      // same association as resid_bwd_kernel: (dx * gamma) * rs
                    if (ra.thresh) {
                        const uint64_t bits = drop_bits4(drop_seed, ((uint64_t)(m - drop_row0) * d + 4 * i) >> 2);
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = drop_keep(bits, k, ra.thresh) ? v[k] * ra.inv_keep : 0.f;
                    }
                    const bf16x4 vb = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
                    ((bf16x4*)(ra.dz + (size_t)m * d))[i] = vb;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        ag[j][k] += orr[k] * (float)cur.z[j][k];
                        az[j][k] += v[k];
                    }
                }
            }
        }
    }
    __syncthreads();      // every slot has been read: the ring's bytes become red[][]
    // cross-wave reduction of the column sums, then one atomic per column per block
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            red[wave][0][(j * 64 + lane) * 4 + k] = aw[j][k];
            red[wave][1][(j * 64 + lane) * 4 + k] = ab[j][k];
            if constexpr (RESID) {
                red[wave][2][(j * 64 + lane) * 4 + k] = ag[j][k];
                red[wave][3][(j * 64 + lane) * 4 + k] = az[j][k];
            }
        }
    __syncthreads();
    for (int c = threadIdx.x; c < d; c += 256) {
        // column c lives at vector i = c/4 -> (j = i/64, lane = i%64), slot k = c%4
        const int i = c >> 2, idx = ((i >> 6) * 64 + (i & 63)) * 4 + (c & 3);
        if (ws) {
#pragma unroll
            for (int q = 0; q < NCOL; ++q)
                ws[((size_t)blockIdx.x * NCOL + q) * d + c] = red[0][q][idx] + red[1][q][idx] + red[2][q][idx] + red[3][q][idx];
        }
    }
}

}  // namespace

extern "C" int vlmo_ln_fwd(const float* x, const float* w, const float* b, void* y, int out_f32, float* mean,
                           float* rstd, const int32_t* rowmap, int M, int d, float eps, hipStream_t stream) {
    VLMO_CHECK_ARG(x && w && b && y, "vlmo_ln_fwd: null pointer");
    VLMO_CHECK_ARG(M > 0 && d > 0 && d % 4 == 0 && d <= 1024, "vlmo_ln_fwd: need 0 < d <= 1024, d %% 4 == 0 (d=%d, M=%d)", d, M);
    const int grid = min((M + 7) / 8, 8192);
    dispatch_vpl(d, [&](auto V) {
        constexpr int VPL = decltype(V)::value;
        if (out_f32)
            hipLaunchKernelGGL((ln_fwd_kernel<VPL, true>), dim3(grid), dim3(256), 0, stream, x, w, b, y, mean, rstd, rowmap, M, d, eps);
        else
            hipLaunchKernelGGL((ln_fwd_kernel<VPL, false>), dim3(grid), dim3(256), 0, stream, x, w, b, y, mean, rstd, rowmap, M, d, eps);
    });
    VLMO_CHECK_LAUNCH("vlmo_ln_fwd");
    return 0;
}

namespace {
// The grid of ln_bwd_kernel over the rows [0, seg) + [seg, M) (seg = M: one segment): rpb rows per workgroup, a multiple
// of the 4 waves; no workgroup straddles the boundary -- workgroups [0, nb0) take segment 0, [nb0, grid) segment 1, and
// their partial rows of the workspace fold into different gradients; grid <= VLMO_MAX_PARTIAL_BLOCKS.
struct LnBwdGrid {
    int rpb, grid, nb0;
};
LnBwdGrid ln_bwd_grid(int M, int seg) {
    int rpb = (M + VLMO_MAX_PARTIAL_BLOCKS - 1) / VLMO_MAX_PARTIAL_BLOCKS;
    rpb = ((rpb + 3) / 4) * 4;
    if (rpb < 8) rpb = 8;
    auto blocks = [&](int rows) { return (rows + rpb - 1) / rpb; };
    while (blocks(seg) + blocks(M - seg) > VLMO_MAX_PARTIAL_BLOCKS) rpb += 4;
    return {rpb, blocks(seg) + blocks(M - seg), blocks(seg)};
}

// ra (optional): the residual branch; its nb0 is set here.  fold, nb0 (optional): see common.h, ln_resid_seg_bwd.
int ln_bwd_launch(const void* dy, int dy_f32, const int32_t* rowmap, const float* x, const float* w, const float* mean,
                  const float* rstd, const float* dres, float* dx, float* dw, float* db, int M, int d, float* ws,
                  int64_t ws_bytes, ResidArgs* ra, float* dgamma, float* dbias, VlmoColJob* fold, hipStream_t stream) {
    VLMO_CHECK_ARG(dy && x && w && mean && rstd && dx, "vlmo_ln_bwd: null pointer");
    // d % 8: the bf16 pieces of a row (dy, zd) go to LDS in 16-byte units (LnRing)
    VLMO_CHECK_ARG(M > 0 && d > 0 && d % 8 == 0 && d <= 1024, "vlmo_ln_bwd: need 0 < d <= 1024, d %% 8 == 0 (d=%d, M=%d)", d, M);
    const int ncol = ra ? 4 : 2;
    const bool need_w = dw || db || ra;
    VLMO_CHECK_ARG(!need_w || (ws && ws_bytes >= reduce_ws_need(ncol * d)),
                   "vlmo_ln_bwd: workspace too small (need %lld bytes)", (long long)reduce_ws_need(ncol * d));
    if (!need_w) ws = nullptr;
    const LnBwdGrid g = ln_bwd_grid(M, ra ? ra->seg : M);
    const ResidArgs none{};
    if (ra) ra->nb0 = g.nb0;
    dispatch_vpl(d, [&](auto V) {
        constexpr int VPL = decltype(V)::value;
        if (ra)
            hipLaunchKernelGGL((ln_bwd_kernel<VPL, false, true>), dim3(g.grid), dim3(256), 0, stream, dy, rowmap, x, w, mean, rstd, dres, dx, ws, M, d, g.rpb, *ra);
        else if (dy_f32)
            hipLaunchKernelGGL((ln_bwd_kernel<VPL, true, false>), dim3(g.grid), dim3(256), 0, stream, dy, rowmap, x, w, mean, rstd, dres, dx, ws, M, d, g.rpb, none);
        else
            hipLaunchKernelGGL((ln_bwd_kernel<VPL, false, false>), dim3(g.grid), dim3(256), 0, stream, dy, rowmap, x, w, mean, rstd, dres, dx, ws, M, d, g.rpb, none);
    });
    VLMO_CHECK_LAUNCH("vlmo_ln_bwd");
    if (need_w) return fold_partials(fold_job(ws, ncol * d, g.grid, ncol * d, d, dw, db, dgamma, dbias), fold, stream);
    return 0;
}
}  // namespace

extern "C" int vlmo_ln_bwd(const void* dy, int dy_f32, const int32_t* rowmap, const float* x, const float* w,
                           const float* mean, const float* rstd, const float* dres, float* dx, float* dw, float* db,
                           int M, int d, float* ws, int64_t ws_bytes, hipStream_t stream) {
    return ln_bwd_launch(dy, dy_f32, rowmap, x, w, mean, rstd, dres, dx, dw, db, M, d, ws, ws_bytes, nullptr, nullptr,
                         nullptr, nullptr, stream);
}

int ln_bwd_fold(const void* dy, const float* x, const float* w, const float* mean, const float* rstd, const float* dres,
                float* dx, float* dw, float* db, const void* zd, const float* gamma, const float* row_scale,
                const int32_t* row_index, void* dz, float* dgamma, float* dbias, uint32_t drop_thresh, float inv_keep,
                uint64_t seed, int M, int d, float* ws, int64_t ws_bytes, VlmoColJob* fold, hipStream_t stream) {
    ResidArgs ra{(const bf16*)zd, gamma, row_scale, row_index, (bf16*)dz, drop_thresh, inv_keep, seed, M, 0, 0};
    return ln_bwd_launch(dy, 0, nullptr, x, w, mean, rstd, dres, dx, dw, db, M, d, ws, ws_bytes, zd ? &ra : nullptr, dgamma,
                         dbias, fold, stream);
}

extern "C" int vlmo_ln_resid_bwd(const void* dy, const float* x, const float* w, const float* mean, const float* rstd,
                                 const float* dres, float* dx, float* dw, float* db, const void* zd, const float* gamma,
                                 const float* row_scale, const int32_t* row_index, void* dz, float* dgamma, float* dbias,
                                 uint32_t drop_thresh, float inv_keep, uint64_t seed, int M, int d, float* ws,
                                 int64_t ws_bytes, hipStream_t stream) {
    VLMO_CHECK_ARG(zd && dz, "vlmo_ln_resid_bwd: null pointer");
    return ln_bwd_fold(dy, x, w, mean, rstd, dres, dx, dw, db, zd, gamma, row_scale, row_index, dz, dgamma, dbias, drop_thresh,
                       inv_keep, seed, M, d, ws, ws_bytes, nullptr, stream);
}

// LayerNorm backward of one block fused with the residual-branch backward of the block BELOW it (block.hip: norm1
// of block i + the FFN branch of block i-1, whose incoming gradient is exactly the dx this kernel writes).  The
// branch may consist of two row segments [0, seg) and [seg, M) with their own dropout streams (per-modality experts);
// the caller folds the bias-gradient partials of the segments itself: workspace rows [0, *nb0) belong to segment 0,
// [*nb0, fold->rows) to segment 1, columns [3d, 4d).
int ln_resid_seg_bwd(const void* dy, const float* x, const float* w, const float* mean, const float* rstd,
                     const float* dres, float* dx, float* dw, float* db, const void* zd, const float* gamma,
                     const float* row_scale, const int32_t* row_index, void* dz, float* dgamma, uint32_t drop_thresh,
                     float inv_keep, uint64_t seed0, uint64_t seed1, int seg, int M, int d, float* ws, int64_t ws_bytes,
                     VlmoColJob* fold, int* nb0, hipStream_t stream) {
    VLMO_CHECK_ARG(zd && dz && seg >= 1 && seg <= M && fold && nb0, "ln_resid_seg_bwd: bad arguments");
    ResidArgs ra{(const bf16*)zd, gamma, row_scale, row_index, (bf16*)dz, drop_thresh, inv_keep, seed0, seg, 0, seed1};
    const int rc = ln_bwd_launch(dy, 0, nullptr, x, w, mean, rstd, dres, dx, dw, db, M, d, ws, ws_bytes, &ra, dgamma, nullptr,
                                 fold, stream);
    *nb0 = ra.nb0;
    return rc;
}
