// The two resampling convolutions of the BEiT-style DiscreteVAE (models/modeling_discrete_vae.py:111-132) over fp16 NHWC
// activation matrices: Conv2d(4, stride 2, padding 1) (vlmo_conv4s2_nhwc) and ConvTranspose2d(4, stride 2, padding 1)
// (vlmo_convt4s2_nhwc), both as implicit MFMA GEMMs with bias (+ ReLU) fused.
//
// Index maps.  Down: output pixel (oy, ox) of the [H/2, W/2] map reads input (2 oy - 1 + ky, 2 ox - 1 + kx), ky, kx in
// 0..3; K = 16 Cin, tap-major (t = 4 ky + kx), channel-minor.  Up: output (oy, ox) of the [2H, 2W] map sums
// x[iy, ix] * w[:, :, ky, kx] over oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx; for output parity (py, px) = (oy & 1, ox & 1)
// and oy = 2 y + py only ky = 1 - py + 2 a, a in 0..1, contributes, from iy = y + py - a (the same along x): each parity
// is a 2 x 2 convolution, K = 4 Cin, over its own quarter of the weight, written to its own quarter of the output
// pixels.  The four parities are blockIdx.y of ONE launch; no zero-stuffed input exists.
//
// Staging: per-tap gather, the form of gemm_nt_kernel<CONV> -- a K-step is (tap, 64-channel chunk), the 128 pixel rows
// of the tile are fetched by LDS-DMA from the tap's source pixel, a tap outside the image reads the zero page.  128 x 128
// tile, four waves of 64 x 64, 2-deep ring of 64-deep slices (64 KB: two workgroups per CU).  A row-slab staging in the
// manner of conv3_dx_kernel (the 2 n + 2 input pixels under n output pixels staged once per (ky, chunk) and read at four
// column offsets) would halve the activation bytes staged per flop of the down-convolution: DESIGN.md section 4m.
#include "gemm_common.h"

namespace {

struct Resample4Args {
    const f16* x;        // [B*H*W, Cin]
    const f16* w;        // down: [Cout, 16 * Cin]; up: [4 parities][Cout, 4 * Cin]
    const f16* zero;     // >= 16 zero bytes
    const float* bias;   // [Cout] or null
    f16* out;            // down: [B*(H/2)*(W/2), ldo]; up: [B*2H*2W, ldo]
    int B, H, W;         // INPUT geometry
    int Cin, Cout, ldo, relu;
};

template <bool UP>
__global__ __launch_bounds__(256, 2) void resample4_kernel(const Resample4Args a) {
    constexpr int BM = 128, BN = 128, BK = 64, NW = 4;
    constexpr int ROWB = BK * 2, A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE = A_BYTES + B_BYTES;
    constexpr int NA = BM / 8 / NW, NB = BN / 8 / NW;      // one-KiB staging pieces (8 rows of 128 bytes) per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // rows of the GEMM: the pixels of the output map (down) or of ONE parity of it = the pixels of the input map (up)
    const int GH = UP ? a.H : a.H / 2, GW = UP ? a.W : a.W / 2;
    const int M = a.B * GH * GW;
    const int py = UP ? (int)(blockIdx.y >> 1) : 0, px = UP ? (int)(blockIdx.y & 1) : 0;
    const int Cin = a.Cin, K = (UP ? 4 : 16) * Cin;
    const int tiles_n = (a.Cout + BN - 1) / BN;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (lid / tiles_n) * BM, n0 = (lid % tiles_n) * BN;
    const f16* wq = a.w + (UP ? (size_t)blockIdx.y * a.Cout * K : 0);

    // staging sources: piece ii = i * 4 + wave covers LDS rows ii * 8 .. + 7, lane -> (row, 16-byte chunk of 8)
    long a_off[NA];          // element offset of (source pixel of tap 0, the lane's chunk) from a.x: may be negative
    int a_y[NA], a_x[NA];    // source pixel of tap 0
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int rr = (i * NW + wave) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ nt_swz<BK>(rr);
        const int gr = min(m0 + rr, M - 1);
        const int b = gr / (GH * GW), pix = gr - b * (GH * GW);
        const int gy = pix / GW, gx = pix - gy * GW;
        a_y[i] = UP ? gy + py : 2 * gy - 1;
        a_x[i] = UP ? gx + px : 2 * gx - 1;
        a_off[i] = (((long)b * a.H + a_y[i]) * a.W + a_x[i]) * Cin + c * 8;
    }
    const f16* b_src[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int rr = (i * NW + wave) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ nt_swz<BK>(rr);
        const int n = min(n0 + rr, a.Cout - 1);
        b_src[i] = wq + (size_t)n * K + c * 8;
    }
    const int cpt = Cin / BK, nk = K / BK;
    auto stage = [&](int buf, int kt) {
        char* s = smem + buf * STAGE;
        const int tap = kt / cpt, cc = kt - tap * cpt;
        // offset of the tap's source pixel from tap 0's: down (ky, kx) = (tap / 4, tap % 4); up (-a, -b) = -(tap / 2, tap % 2)
        const int dy = UP ? -(tap >> 1) : (tap >> 2), dx = UP ? -(tap & 1) : (tap & 3);
        const int delta = (dy * a.W + dx) * Cin + cc * BK;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const bool in = (unsigned)(a_y[i] + dy) < (unsigned)a.H && (unsigned)(a_x[i] + dx) < (unsigned)a.W;
            glds16(in ? a.x + (a_off[i] + delta) : a.zero, s + (i * NW + wave) * 1024);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) glds16(b_src[i] + kt * BK, s + A_BYTES + (i * NW + wave) * 1024);
    };

    const int l31 = lane & 31, h = lane >> 5;
    const int swz = nt_swz<BK>(l31);
    const int a_row_off = (wm * 64 + l31) * ROWB, b_row_off = A_BYTES + (wn * 64 + l31) * ROWB;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
        const char* s = smem + (kt & 1) * STAGE;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            const int coff = ((2 * ks + h) ^ swz) << 4;
            f16x8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = *(const f16x8*)(s + a_row_off + i * 32 * ROWB + coff);
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = *(const f16x8*)(s + b_row_off + j * 32 * ROWB + coff);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = Elem<f16>::mfma(af[i], bf[j], acc[i][j]);
        }
    }
    // epilogue: bias (+ ReLU) -> f16, through a wave-private [64 pixels][64 channels] LDS image so that every global store
    // is a 16-byte piece of a 128-byte run of an output row (conv3_dx_kernel's)
    __syncthreads();
    f16* ep = (f16*)(smem + wave * 8192);
    const bool relu_out = (a.relu & 1) != 0;
    const int nw0 = n0 + wn * 64;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = nw0 + j * 32 + l31;
        const float bv = (a.bias && n < a.Cout) ? a.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[i][j][r] + bv;
                if (relu_out) v = fmaxf(v, 0.f);
                ep[(i * 32 + 8 * (r >> 2) + 4 * h + (r & 3)) * 64 + j * 32 + l31] = (f16)v;
            }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int ch = lane + 64 * q, row = ch >> 3, c8 = (ch & 7) * 8;
        const int m = m0 + wm * 64 + row;
        if (m < M && nw0 + c8 < a.Cout) {
            size_t orow = (size_t)m;
            if (UP) {       // row m = (b, y, x) of the input grid -> output pixel (b, 2 y + py, 2 x + px)
                const int b = m / (GH * GW), pix = m - b * (GH * GW);
                const int gy = pix / GW, gx = pix - gy * GW;
                orow = ((size_t)b * 2 * GH + 2 * gy + py) * (2 * GW) + 2 * gx + px;
            }
            const f16x8 v = *(const f16x8*)(ep + row * 64 + c8);
            *(f16x8*)(a.out + orow * a.ldo + nw0 + c8) = v;
        }
    }
}

template <bool UP>
int launch_resample4(const char* name, const void* x, int B, int H, int W, int Cin, const void* w, int Cout,
                     const void* zero_page, const VlmoEpilogue* e, hipStream_t stream) {
    const Resample4Args a{(const f16*)x, (const f16*)w, (const f16*)zero_page, e->bias, (f16*)e->out, B, H, W, Cin, Cout,
                          e->ldo, e->relu};
    constexpr int LDS = 2 * (128 + 128) * 128;
    const long M = UP ? (long)B * H * W : (long)B * (H / 2) * (W / 2);
    const long tiles = ((M + 127) / 128) * ((Cout + 127) / 128);
    if (tiles > 0x7fffffffL) {
        vlmo_set_error("%s: too many tiles", name);
        return -1;
    }
    hipLaunchKernelGGL(resample4_kernel<UP>, dim3((unsigned)tiles, UP ? 4 : 1), dim3(256), LDS, stream, a);
    VLMO_CHECK_LAUNCH(name);
    return 0;
}

int check_resample4(const char* name, int dtype, const void* x, int B, int H, int W, int Cin, const void* w, int Cout,
                    const void* zero_page, const VlmoEpilogue* e, bool down) {
    VLMO_CHECK_ARG(x && w && e && zero_page, "%s: null pointer", name);
    VLMO_CHECK_ARG(dtype == VLMO_F16, "%s: f16 activations only", name);
    VLMO_CHECK_ARG(B > 0 && H > 0 && W > 0 && H < 16384 && W < 16384, "%s: bad geometry", name);
    VLMO_CHECK_ARG(!down || (H % 2 == 0 && W % 2 == 0), "%s: H and W must be even (got %d x %d)", name, H, W);
    VLMO_CHECK_ARG((long)B * H * W * (down ? 1 : 4) < 0x7fffffffL, "%s: more than 2^31 pixels", name);
    VLMO_CHECK_ARG(Cin > 0 && Cin % 64 == 0, "%s: Cin must be a multiple of 64 (got %d)", name, Cin);
    VLMO_CHECK_ARG(Cout > 0 && Cout % 8 == 0, "%s: Cout must be a multiple of 8 (got %d)", name, Cout);
    VLMO_CHECK_ARG(e->out && e->ldo >= Cout && e->ldo % 8 == 0, "%s: bad output / ldo", name);
    return 0;
}
}  // namespace

extern "C" int vlmo_conv4s2_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, const void* w, int Cout,
                                 const void* zero_page, const VlmoEpilogue* e, hipStream_t stream) {
    if (int rc = check_resample4("vlmo_conv4s2_nhwc", dtype, x, B, H, W, Cin, w, Cout, zero_page, e, true)) return rc;
    ProfScope prof(32 + VLMO_EPI_BIAS, 2.0 * B * (H / 2) * (W / 2) * Cout * 16.0 * Cin, stream);
    return launch_resample4<false>("vlmo_conv4s2_nhwc", x, B, H, W, Cin, w, Cout, zero_page, e, stream);
}

extern "C" int vlmo_convt4s2_nhwc(int dtype, const void* x, int B, int H, int W, int Cin, const void* w, int Cout,
                                  const void* zero_page, const VlmoEpilogue* e, hipStream_t stream) {
    if (int rc = check_resample4("vlmo_convt4s2_nhwc", dtype, x, B, H, W, Cin, w, Cout, zero_page, e, false)) return rc;
    ProfScope prof(32 + VLMO_EPI_BIAS, 2.0 * B * H * W * 4.0 * Cout * 4.0 * Cin, stream);
    return launch_resample4<true>("vlmo_convt4s2_nhwc", x, B, H, W, Cin, w, Cout, zero_page, e, stream);
}
