// Two-view image crop (the reference builds it on the CPU with PIL: data/utils/transforms.py,
// RandomResizedCropAndInterpolationWithTwoPic + flip + ToTensor + Normalize / map_pixels): crop a box out of a packed
// uint8 HWC source, resample it to S x S with PIL's antialiased bicubic or Lanczos windows, flip, normalise.  Entry point
// vlmo_crop_resample, two launches for all jobs of a batch (DESIGN.md 4h has the specification):
//   crop_h_kernel   horizontal pass: a workgroup owns 32 output columns x 32 crop rows of one job.  The source columns
//                   its windows cover are walked in chunks of 128: the chunk's bytes go to LDS as whole aligned dwords
//                   (packed_image.h has the rule that allows it), the chunk's weights are computed once per output
//                   column into LDS, and a thread (one output column, four rows) sums its own taps only.
//                   Writes the fp32 intermediate [h, S, 3] of the job.
//   crop_v_kernel   vertical pass: a workgroup owns 64 output columns x 16 output rows (4 per wave); the weights of the 16
//                   rows are computed once into LDS (chunks of 128 taps), a lane reads the three channels of its column
//                   (12 contiguous bytes, 768 per wave) and writes planar [3, S, S] with the flip and the finish fused in.
// Weights: the window and the filter argument are evaluated in fp64 on the device (a centre near 8192 has an fp32 ulp of
// 5e-4 pixels) and rounded once to fp32; the sums run in fp32 in ascending tap order, and a pixel's sum is divided by the
// sum of its weights at the end.  Nothing is accumulated with atomics and no thread's arithmetic depends on the job's
// position in the table: the same bits from run to run and for every job order.
#include "packed_image.h"

namespace {

constexpr int HX = 32;         // output columns per workgroup, horizontal pass
constexpr int HY = 32;         // crop rows per workgroup (4 per thread)
constexpr int HC = 128;        // source columns per chunk
constexpr int HPITCH = packed::row_pitch(HC * 3);       // bytes of a staged row
constexpr int WPITCH = HC + 1;         // floats per weight row: rows on different banks
constexpr int VX = 64, VY = 16, VC = 128;

struct Finish {
    float mul[2][3], add[2][3];        // [finish mode][channel]: value = v * mul + add
};

__device__ __forceinline__ double filter_weight(int filter, double x) {
    x = fabs(x);
    if (filter == VLMO_FILTER_BICUBIC) {           // Keys, a = -0.5
        if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
        if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
        return 0.0;
    }
    if (x >= 3.0) return 0.0;                      // Lanczos-3: sinc(x) sinc(x / 3)
    if (x < 1e-12) return 1.0;
    return 3.0 * sinpi(x) * sinpi(x / 3.0) / (9.869604401089358 * x * x);
}

// One axis of a job: input length n -> output length S
struct Axis {
    double scale, fs, support;
    int n, filter;
    __device__ __forceinline__ Axis(int n_, int S, int filter_) : n(n_), filter(filter_) {
        scale = (double)n_ / (double)S;
        fs = scale > 1.0 ? scale : 1.0;
        support = (filter_ == VLMO_FILTER_BICUBIC ? 2.0 : 3.0) * fs;
    }
    __device__ __forceinline__ double center(int o) const { return (o + 0.5) * scale; }
    __device__ __forceinline__ void window(int o, int* k0, int* k1) const {
        const double c = center(o);
        const int a = (int)(c - support + 0.5), b = (int)(c + support + 0.5);
        *k0 = a > 0 ? a : 0;
        *k1 = b < n ? b : n;
    }
    __device__ __forceinline__ float weight(int o, int k) const {
        return (float)filter_weight(filter, (k + 0.5 - center(o)) / fs);
    }
};

// rows [no, pitch] of LDS weights for outputs o0 .. o0 + no - 1 and taps cc .. cc + nc - 1: 0 outside an output's window
template <int NC>
__device__ __forceinline__ void fill_weights(float* w, int pitch, const Axis& ax, int o0, int no, int cc, const int* k0,
                                             const int* k1) {
    for (int i = threadIdx.x; i < no * NC; i += 256) {
        const int ol = i / NC, k = cc + i % NC;
        w[ol * pitch + i % NC] = (k >= k0[ol] && k < k1[ol]) ? ax.weight(o0 + ol, k) : 0.f;
    }
}

__global__ __launch_bounds__(256) void crop_h_kernel(const uint8_t* __restrict__ src, const VlmoImage* __restrict__ images,
                                                     const VlmoCropJob* __restrict__ jobs, float* __restrict__ tmp) {
    __shared__ __attribute__((aligned(16))) uint8_t s_src[HY * HPITCH];
    __shared__ float s_w[HX * WPITCH];
    __shared__ int s_k0[HX], s_k1[HX];
    const VlmoCropJob J = jobs[blockIdx.x];
    const int x0 = blockIdx.y * HX, y0 = blockIdx.z * HY;
    if (x0 >= J.S || y0 >= J.h) return;             // the grid is sized for the largest job of the call
    const VlmoImage I = images[J.image];
    const int tid = threadIdx.x;
    const int nx = min(HX, J.S - x0), ny = min(HY, J.h - y0);
    const Axis ax(J.w, J.S, J.filter);
    if (tid < HX) {
        int a = 0, b = 0;
        if (tid < nx) ax.window(x0 + tid, &a, &b);
        s_k0[tid] = a;
        s_k1[tid] = b;
    }
    __syncthreads();
    const int c_lo = s_k0[0], c_hi = s_k1[nx - 1];  // windows move right with the output column
    const int xl = tid & (HX - 1), rl = tid >> 5;   // this thread: column x0 + xl, rows y0 + rl + 8 i
    const int k0 = s_k0[xl], k1 = s_k1[xl];
    // byte offset of crop pixel (y0, 0) in the packed buffer; a row of the image is W * 3 bytes
    const size_t row_bytes = (size_t)I.W * 3;
    const size_t origin = (size_t)I.offset + ((size_t)(J.top + y0) * I.W + J.left) * 3;
    float acc[4][3] = {};
    float wsum = 0.f;
    for (int cc = c_lo; cc < c_hi; cc += HC) {
        const int nc = min(HC, c_hi - cc);
        fill_weights<HC>(s_w, WPITCH, ax, x0, nx, cc, s_k0, s_k1);
        // rows y0 .. y0 + ny - 1, source columns cc .. cc + nc - 1
        const size_t first0 = origin + (size_t)cc * 3;
        packed::stage_rows(s_src, HPITCH, src, first0, row_bytes, ny, nc * 3);
        __syncthreads();
        if (xl < nx) {
            const int ka = max(k0, cc), kb = min(k1, cc + nc);
            const uint8_t* p[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = min(rl + 8 * i, ny - 1);                  // rows past the tile repeat its last row, unused
                p[i] = packed::staged_row(s_src, r, HPITCH, first0 + (size_t)r * row_bytes);
            }
            for (int k = ka; k < kb; ++k) {
                const float wv = s_w[xl * WPITCH + (k - cc)];
                const int b = (k - cc) * 3;
                wsum += wv;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[i][0] = fmaf(wv, (float)p[i][b], acc[i][0]);
                    acc[i][1] = fmaf(wv, (float)p[i][b + 1], acc[i][1]);
                    acc[i][2] = fmaf(wv, (float)p[i][b + 2], acc[i][2]);
                }
            }
        }
        __syncthreads();
    }
    if (xl < nx) {
        const float inv = 1.f / wsum;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rl + 8 * i;
            if (r < ny) {
                float* o = tmp + J.tmp_off + ((size_t)(y0 + r) * J.S + (x0 + xl)) * 3;
                o[0] = acc[i][0] * inv;
                o[1] = acc[i][1] * inv;
                o[2] = acc[i][2] * inv;
            }
        }
    }
}

__global__ __launch_bounds__(256) void crop_v_kernel(const VlmoCropJob* __restrict__ jobs, const float* __restrict__ tmp,
                                                     Finish fin) {
    __shared__ float s_w[VY * (VC + 1)];
    __shared__ int s_k0[VY], s_k1[VY];
    const VlmoCropJob J = jobs[blockIdx.x];
    const int S = J.S;
    const int x0 = blockIdx.y * VX, o0 = blockIdx.z * VY;
    if (x0 >= S || o0 >= S) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int no = min(VY, S - o0);
    const Axis ax(J.h, S, J.filter);
    if (tid < VY) {
        int a = 0, b = 0;
        if (tid < no) ax.window(o0 + tid, &a, &b);
        s_k0[tid] = a;
        s_k1[tid] = b;
    }
    __syncthreads();
    const int c_lo = s_k0[0], c_hi = s_k1[no - 1];
    const int ox = x0 + lane;
    const bool live = ox < S;
    const float* col = tmp + J.tmp_off + (size_t)(live ? ox : x0) * 3;      // row k of the intermediate: + k * S * 3
    float acc[4][3] = {};
    float wsum[4] = {};
    for (int cc = c_lo; cc < c_hi; cc += VC) {
        const int nc = min(VC, c_hi - cc);
        fill_weights<VC>(s_w, VC + 1, ax, o0, no, cc, s_k0, s_k1);
        __syncthreads();
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int ol = wave * 4 + o;
            if (ol < no) {                           // the same for every lane of the wave
                const int ka = max(s_k0[ol], cc), kb = min(s_k1[ol], cc + nc);
                for (int k = ka; k < kb; ++k) {
                    const float wv = s_w[ol * (VC + 1) + (k - cc)];
                    const float* q = col + (size_t)k * S * 3;
                    wsum[o] += wv;
                    acc[o][0] = fmaf(wv, q[0], acc[o][0]);
                    acc[o][1] = fmaf(wv, q[1], acc[o][1]);
                    acc[o][2] = fmaf(wv, q[2], acc[o][2]);
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    const int xo = J.flip ? S - 1 - ox : ox;
    const int f = J.finish;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int oy = o0 + wave * 4 + o;
        if (oy < S) {
            const float inv = 1.f / wsum[o];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                J.out[((size_t)c * S + oy) * S + xo] = fmaf(acc[o][c] * inv, fin.mul[f][c], fin.add[f][c]);
        }
    }
}

int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

extern "C" int vlmo_crop_resample(const uint8_t* src, int64_t src_bytes, const VlmoImage* images, const VlmoImage* images_dev,
                                  int n_images, const VlmoCropJob* jobs, const VlmoCropJob* jobs_dev, int n_jobs,
                                  const float* mean, const float* std, float pixel_eps, float* ws, int64_t ws_bytes,
                                  hipStream_t stream) {
    VLMO_CHECK_ARG(src && images && images_dev && jobs && jobs_dev && mean && std && ws, "vlmo_crop_resample: null pointer");
    // the crop limits the sides of its boxes, not of the images
    if (packed::check_packed("vlmo_crop_resample", "packed buffer", (uintptr_t)src, src_bytes, images, n_images, 0)) return -1;
    VLMO_CHECK_ARG(n_images >= 1, "vlmo_crop_resample: no images");
    VLMO_CHECK_ARG(n_jobs >= 1 && n_jobs <= VLMO_CROP_MAX_JOBS, "vlmo_crop_resample: need 1 <= jobs <= %d per call (got %d)",
                   VLMO_CROP_MAX_JOBS, n_jobs);
    VLMO_CHECK_ARG(pixel_eps >= 0.f && pixel_eps < 0.5f, "vlmo_crop_resample: pixel_eps %g outside [0, 0.5)", (double)pixel_eps);
    int64_t run = 0;
    int max_s = 0, max_h = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const VlmoCropJob& J = jobs[j];
        VLMO_CHECK_ARG(J.image >= 0 && J.image < n_images, "vlmo_crop_resample: job %d: image index %d of %d", j, J.image,
                       n_images);
        const VlmoImage& I = images[J.image];
        VLMO_CHECK_ARG(J.S >= 1 && J.S <= VLMO_CROP_MAX_SIZE, "vlmo_crop_resample: job %d: need 1 <= S <= %d (S=%d)", j,
                       VLMO_CROP_MAX_SIZE, J.S);
        VLMO_CHECK_ARG(J.h >= 1 && J.w >= 1 && J.h <= VLMO_CROP_MAX_SIDE && J.w <= VLMO_CROP_MAX_SIDE,
                       "vlmo_crop_resample: job %d: crop sides must lie in [1, %d] (h=%d w=%d)", j, VLMO_CROP_MAX_SIDE, J.h, J.w);
        VLMO_CHECK_ARG(J.top >= 0 && J.left >= 0 && J.top <= I.H - J.h && J.left <= I.W - J.w,
                       "vlmo_crop_resample: job %d: box (top %d, left %d, h %d, w %d) is not inside its %d x %d image", j,
                       J.top, J.left, J.h, J.w, I.H, I.W);
        VLMO_CHECK_ARG((J.filter == VLMO_FILTER_BICUBIC || J.filter == VLMO_FILTER_LANCZOS) &&
                           (J.finish == VLMO_FINISH_NORMALIZE || J.finish == VLMO_FINISH_MAP_PIXELS) &&
                           (J.flip == 0 || J.flip == 1),
                       "vlmo_crop_resample: job %d: bad filter / finish / flip (%d / %d / %d)", j, J.filter, J.finish, J.flip);
        VLMO_CHECK_ARG(J.out, "vlmo_crop_resample: job %d: null output", j);
        VLMO_CHECK_ARG(J.tmp_off == run, "vlmo_crop_resample: job %d: tmp_off %lld, expected the running sum %lld of h * S * 3",
                       j, (long long)J.tmp_off, (long long)run);
        run += (int64_t)J.h * J.S * 3;
        max_s = J.S > max_s ? J.S : max_s;
        max_h = J.h > max_h ? J.h : max_h;
    }
    VLMO_CHECK_ARG(ws_bytes >= run * 4, "vlmo_crop_resample: workspace too small (need %lld bytes, got %lld)",
                   (long long)(run * 4), (long long)ws_bytes);
    Finish fin;
    for (int c = 0; c < 3; ++c) {
        VLMO_CHECK_ARG(std[c] > 0.f, "vlmo_crop_resample: std[%d] = %g must be positive", c, (double)std[c]);
        fin.mul[VLMO_FINISH_NORMALIZE][c] = (float)(1.0 / (255.0 * (double)std[c]));
        fin.add[VLMO_FINISH_NORMALIZE][c] = (float)(-(double)mean[c] / (double)std[c]);
        fin.mul[VLMO_FINISH_MAP_PIXELS][c] = (float)((1.0 - 2.0 * (double)pixel_eps) / 255.0);
        fin.add[VLMO_FINISH_MAP_PIXELS][c] = pixel_eps;
    }
    hipLaunchKernelGGL(crop_h_kernel, dim3(n_jobs, cdiv(max_s, HX), cdiv(max_h, HY)), dim3(256), 0, stream, src, images_dev,
                       jobs_dev, ws);
    VLMO_CHECK_LAUNCH("vlmo_crop_resample(horizontal)");
    hipLaunchKernelGGL(crop_v_kernel, dim3(n_jobs, cdiv(max_s, VX), cdiv(max_s, VY)), dim3(256), 0, stream, jobs_dev, ws, fin);
    VLMO_CHECK_LAUNCH("vlmo_crop_resample(vertical)");
    return 0;
}
