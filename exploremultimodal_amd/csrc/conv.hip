// dVAE convolutions over NHWC activation matrices (vlmo_conv2d_nhwc): conv3_dx_kernel for 3x3 bottlenecks and the
// implicit-GEMM instantiations of gemm_nt_kernel (CONV = true).
#include <type_traits>

#include "gemm_common.h"

namespace {
// ---- 3x3 convolution with <= 64 output channels (dall_e EncoderBlock bottleneck of the first group, encoder.py:21-29:
// 112 x 112 x {256 -> 64, 64 -> 64}) ------------------------------------------------------------------------------
// With 64 output channels the implicit GEMM is bound by the per-CU fill rate of its A operand: the generic kernel
// stages the 256 input rows of a tile once per TAP (nine times per channel chunk: 40 KB per 16 MFMAs of a wave).  Here a
// K-step is (dy, 32-channel half chunk): the rows [m0 - 8, m0 + 264) of image row y + dy are staged ONCE and the three
// dx taps read them at row offsets -1 / 0 / +1 (the fragment of a lane whose pixel has no left / right neighbour is
// zeroed in registers); the three taps' weights ride along: 29 KB per 24 MFMAs of a wave, 2.1x fewer staged bytes per
// flop.  256 x 64 tile, 4 waves (64 pixels x 64 channels each), 2-deep LDS ring of 32-deep slices (59 KB: two
// workgroups per CU, as the generic kernel -- a 64-deep ring with one workgroup per CU filled at 20 GB/s per CU and
// lost on the K = 576 convolutions, whose three steps never fill the pipeline), f16.
struct Conv3Args {
    const f16* x;        // [B*H*W, Cin]
    const f16* w;        // [Cout <= 64, 9 * Cin] tap-major, channel-minor
    const f16* zero;     // >= 128 zero bytes
    const float* bias;
    f16* out;            // [B*H*W, ldo]
    int M, H, W, Cin, Cout, ldo, relu;
};
// VLMO_EPI_DUAL (the DUAL instantiations): v = resid + beta * (acc + bias); out = v; out2 = relu(v)
struct Conv3DualArgs : Conv3Args {
    const f16* resid;    // [B*H*W, ldo] or null (= 0)
    f16* out2;           // [B*H*W, ld2] or null
    int ld2;
    float beta;
};

// WM x WN waves of 64 pixels x 64 channels: <4, 1> = 256 x 64 tile (<= 64 output channels), <2, 2> = 128 x 128 tile.
// DUAL: the DecoderBlock tail (dall_e/decoder.py:42-46, conv_4 is the block's 3x3 with n_out channels): the identity
// path's fp16 rows are requested before the K loop (8 x 16 bytes per lane, they fly under the operand staging), put into
// the wave's epilogue image and combined there in fp32, so the sum is rounded to fp16 once.
template <int WM, int WN, bool DUAL>
__global__ __launch_bounds__(256, 2) void conv3_dx_kernel(const std::conditional_t<DUAL, Conv3DualArgs, Conv3Args> a) {
    static_assert(WM * WN == 4, "four waves");
    constexpr int BM = WM * 64, BN = WN * 64, HALO = 8, AROWS = BM + 2 * HALO;
    constexpr int A_BYTES = AROWS * 64, B_BYTES = 3 * BN * 64, STAGE = A_BYTES + B_BYTES;
    constexpr int NAI = AROWS / 16, NBI = 3 * BN / 16;      // one-KiB staging pieces per step (17 + 12 or 9 + 24)
    constexpr int NAS = (NAI + 3) / 4, NBS = NBI / 4;       // ... per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int tiles_n = (a.Cout + BN - 1) / BN;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (lid / tiles_n) * BM, n0 = (lid % tiles_n) * BN;
    const int HW = a.H * a.W, Cin = a.Cin, K = 9 * Cin;
    const int cpt = Cin >> 5, nsteps = 3 * cpt;

    // staging sources: piece ii = i * 4 + wave covers LDS rows ii * 16 .. + 15, lane -> (row, 16-byte chunk of 4)
    const f16* a_src[NAS];
    int a_y[NAS];
#pragma unroll
    for (int i = 0; i < NAS; ++i) {
        const int rr = (i * 4 + wave) * 16 + (lane >> 2);
        const int c = (lane & 3) ^ nt_swz<32>(rr);
        const int pix = min(max(m0 - HALO + rr, 0), a.M - 1);
        a_src[i] = a.x + (size_t)pix * Cin + c * 8;
        a_y[i] = (pix % HW) / a.W;
    }
    const f16* b_src[NBS];
#pragma unroll
    for (int i = 0; i < NBS; ++i) {
        const int rr = (i * 4 + wave) * 16 + (lane >> 2);      // tap dx * BN + output channel of the tile
        const int c = (lane & 3) ^ nt_swz<32>(rr);
        const int n = min(n0 + rr % BN, a.Cout - 1);
        b_src[i] = a.w + (size_t)n * K + (rr / BN) * Cin + c * 8;
    }
    auto stage = [&](int buf, int s_) {
        char* s = smem + buf * STAGE;
        const int dyi = s_ / cpt, hc = s_ - dyi * cpt, dy = dyi - 1;
        const int delta = dy * a.W * Cin + hc * 32;
#pragma unroll
        for (int i = 0; i < NAS; ++i) {
            if (i * 4 + wave < NAI) {
                const bool in = (unsigned)(a_y[i] + dy) < (unsigned)a.H;
                glds16(in ? a_src[i] + delta : a.zero, s + (i * 4 + wave) * 1024);
            }
        }
        const int wofs = dyi * 3 * Cin + hc * 32;
#pragma unroll
        for (int i = 0; i < NBS; ++i) glds16(b_src[i] + wofs, s + A_BYTES + (i * 4 + wave) * 1024);
    };

    const int l31 = lane & 31, h = lane >> 5;
    // A fragment of tap dx, row block i: LDS row HALO + wm * 64 + i * 32 + l31 + dx (the swizzle key of a row does not
    // change with + 32); B fragment: row dxi * BN + wn * 64 + j * 32 + l31
    int a_off[3], a_swz[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int row = HALO + wm * 64 + l31 + (t - 1);
        a_off[t] = row * 64;
        a_swz[t] = nt_swz<32>(row);
    }
    const int b_off = A_BYTES + (wn * 64 + l31) * 64, b_swz = nt_swz<32>(l31);
    bool edge_l[2], edge_r[2];      // the lane's pixel has no left / right neighbour in its image row
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int xx = (m0 + wm * 64 + i * 32 + l31) % a.W;
        edge_l[i] = xx == 0;
        edge_r[i] = xx == a.W - 1;
    }
    const bool relu_in = (a.relu & 2) != 0;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

    // lane -> (row, 8-channel piece) of the wave's 64 x 64 output block in the epilogue's store passes
    f16x8 pre[DUAL ? 8 : 1];
    if constexpr (DUAL) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int ch = lane + 64 * q, row = ch >> 3, c8 = (ch & 7) * 8;
            const int m = m0 + wm * 64 + row, n = n0 + wn * 64 + c8;
            const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            pre[q] = (a.resid && m < a.M && n < a.Cout) ? *(const f16x8*)(a.resid + (size_t)m * a.ldo + n) : z;
        }
    }

    stage(0, 0);
    for (int s_ = 0; s_ < nsteps; ++s_) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (s_ + 1 < nsteps) stage((s_ + 1) & 1, s_ + 1);
        const char* s = smem + (s_ & 1) * STAGE;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                f16x8 af[2], bf[2];
                const int ca = ((2 * ks + h) ^ a_swz[t]) << 4, cb = ((2 * ks + h) ^ b_swz) << 4;
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *(const f16x8*)(s + a_off[t] + i * 2048 + ca);
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = *(const f16x8*)(s + b_off + (t * BN + j * 32) * 64 + cb);
                const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (relu_in) af[i] = __builtin_elementwise_max(af[i], z);
                    if (t == 0) af[i] = edge_l[i] ? z : af[i];
                    if (t == 2) af[i] = edge_r[i] ? z : af[i];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = Elem<f16>::mfma(af[i], bf[j], acc[i][j]);
            }
        }
    }
    // epilogue: bias (+ ReLU) -> f16, through a wave-private [64 pixels][64 channels] LDS image so that every global store
    // is a 16-byte piece of a 128-byte run of an output row
    __syncthreads();
    f16* ep = (f16*)(smem + wave * 8192);
    const bool relu_out = (a.relu & 1) != 0;
    const int nw0 = n0 + wn * 64;
    if constexpr (DUAL) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int ch = lane + 64 * q;
            *(f16x8*)(ep + (ch >> 3) * 64 + (ch & 7) * 8) = pre[q];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = nw0 + j * 32 + l31;
        const float bv = (a.bias && n < a.Cout) ? a.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[i][j][r] + bv;
                if constexpr (DUAL) {
                    f16* slot = ep + (i * 32 + 8 * (r >> 2) + 4 * h + (r & 3)) * 64 + j * 32 + l31;
                    *slot = (f16)((float)*slot + a.beta * v);
                } else {
                    if (relu_out) v = fmaxf(v, 0.f);
                    ep[(i * 32 + 8 * (r >> 2) + 4 * h + (r & 3)) * 64 + j * 32 + l31] = (f16)v;
                }
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int ch = lane + 64 * q, row = ch >> 3, c8 = (ch & 7) * 8;
        const int m = m0 + wm * 64 + row;
        if (m < a.M && nw0 + c8 < a.Cout) {
            const f16x8 v = *(const f16x8*)(ep + row * 64 + c8);
            if constexpr (DUAL) {
                // the next convolution reads both maps back at once: plain stores
                *(f16x8*)(a.out + (size_t)m * a.ldo + nw0 + c8) = v;
                const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
                if (a.out2) *(f16x8*)(a.out2 + (size_t)m * a.ld2 + nw0 + c8) = __builtin_elementwise_max(v, z);
            } else {
                __builtin_nontemporal_store(v, (f16x8*)(a.out + (size_t)m * a.ldo + nw0 + c8));
            }
        }
    }
}

template <int WM, int WN, bool DUAL>
int launch_conv3_dx(const void* x, int B, int H, int W, int Cin, const void* w, int Cout, const void* zero_page,
                    const VlmoEpilogue* e, hipStream_t stream) {
    std::conditional_t<DUAL, Conv3DualArgs, Conv3Args> a{};
    static_cast<Conv3Args&>(a) = Conv3Args{(const f16*)x, (const f16*)w, (const f16*)zero_page, e->bias, (f16*)e->out,
                                           B * H * W, H, W, Cin, Cout, e->ldo, e->relu};
    if constexpr (DUAL) {
        a.resid = (const f16*)(const void*)e->resid, a.out2 = (f16*)e->out2, a.ld2 = e->ld2, a.beta = e->beta;
    }
    constexpr int BM = WM * 64, BN = WN * 64;
    constexpr int LDS = 2 * ((BM + 16) * 64 + 3 * BN * 64);
    static DeviceOnce once;
    if (once.first())
        (void)hipFuncSetAttribute((const void*)conv3_dx_kernel<WM, WN, DUAL>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    const int grid = ((a.M + BM - 1) / BM) * ((Cout + BN - 1) / BN);
    hipLaunchKernelGGL((conv3_dx_kernel<WM, WN, DUAL>), dim3(grid), dim3(256), LDS, stream, a);
    VLMO_CHECK_LAUNCH("vlmo_conv2d_nhwc");
    return 0;
}
}  // namespace

// 2-D convolution, stride 1, "same" zero padding (kw-1)/2, over an NHWC activation matrix
// x [B*H*W, Cin] with weights w [Cout, kw*kw*Cin] (tap-major, channel-minor): dall_e/utils.py:37-48.
extern "C" int vlmo_conv2d_nhwc(int epi, int dtype, const void* x, int B, int H, int W, int Cin, int kw,
                                const void* w, int Cout, const void* zero_page, const VlmoEpilogue* e,
                                hipStream_t stream) {
    VLMO_CHECK_ARG(x && w && e && zero_page, "vlmo_conv2d_nhwc: null pointer");
    VLMO_CHECK_ARG(B > 0 && H > 0 && W > 0 && H < 32768 && W < 32768, "vlmo_conv2d_nhwc: bad geometry");
    VLMO_CHECK_ARG(Cin % 64 == 0 && Cout % 4 == 0, "vlmo_conv2d_nhwc: Cin must be a multiple of 64 (got %d), Cout of 4", Cin);
    VLMO_CHECK_ARG(kw >= 1 && kw % 2 == 1, "vlmo_conv2d_nhwc: kernel width must be odd (dall_e/utils.py:14)");
    VLMO_CHECK_ARG(e->out && e->ldo >= Cout, "vlmo_conv2d_nhwc: bad output");
    VLMO_CHECK_ARG(dtype == VLMO_BF16 || dtype == VLMO_F16, "vlmo_conv2d_nhwc: dtype must be bf16 or f16");
    const int K = kw * kw * Cin;
    GemmNTGroups p{};
    p.ngroups = 1;
    p.g[0] = GemmNT{x, w, B * H * W, Cout, K, Cin, K, *e, H, W, Cin, kw, zero_page, 8, nullptr, 0, 0, 1.f};
    ProfScope prof(32 + epi, 2.0 * B * H * W * Cout * K, stream);
    // wide bottlenecks whose 256 x 256 tiles fill most of one dispatch round (group 3 of the dVAE at 64 images: 196 tiles):
    // the ping-pong kernel with per-tap staging -- half the staged bytes per flop of the 128 x 128 tile
    if (dtype == VLMO_F16 && epi == VLMO_EPI_BIAS && Cout % 256 == 0) {
        const long t256 = (long)((B * H * W + 255) / 256) * (Cout / 256);
        if (t256 >= 160 && (t256 <= 256 || t256 >= 640))
            return launch_nt<f16, 256, 256, 2, 4, true, 64, 2, true, (1u << VLMO_EPI_BIAS)>(epi, p, stream);
    }
    if (dtype == VLMO_F16 && epi == VLMO_EPI_BIAS && kw == 3 && Cin % 32 == 0 && Cout % 8 == 0 && e->ldo % 8 == 0) {
        if (Cout <= 64) return launch_conv3_dx<4, 1, false>(x, B, H, W, Cin, w, Cout, zero_page, e, stream);
        return launch_conv3_dx<2, 2, false>(x, B, H, W, Cin, w, Cout, zero_page, e, stream);
    }
    // DecoderBlock tail (3x3, residual epilogue) under the same shape conditions; the residual rows and the second output
    // move as 16-byte pieces too
    if (dtype == VLMO_F16 && epi == VLMO_EPI_DUAL && kw == 3 && Cin % 32 == 0 && Cout % 8 == 0 && e->ldo % 8 == 0 &&
        (!e->out2 || e->ld2 % 8 == 0)) {
        if (Cout <= 64) return launch_conv3_dx<4, 1, true>(x, B, H, W, Cin, w, Cout, zero_page, e, stream);
        return launch_conv3_dx<2, 2, true>(x, B, H, W, Cin, w, Cout, zero_page, e, stream);
    }
    // <= 64 output channels: a 256 x 64 tile -- with the 128-wide tile half of every MFMA and half of the weight staging
    // multiplied padding
    if (dtype == VLMO_F16 && Cout <= 64 && epi == VLMO_EPI_BIAS)
        return launch_nt<f16, 256, 64, 4, 1, true, 64, 2, false, (1u << VLMO_EPI_BIAS)>(epi, p, stream);
    if (dtype == VLMO_F16) return launch_nt<f16, 128, 128, 2, 2, true>(epi, p, stream);
    return launch_nt<bf16, 128, 128, 2, 2, true>(epi, p, stream);
}
