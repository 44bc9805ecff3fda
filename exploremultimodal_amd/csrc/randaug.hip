// RandAugment on packed uint8 HWC sources (the reference runs data/utils/randaugment.py on the CPU with numpy and cv2, on
// the full-size source before the crop).  Entry point vlmo_randaug (DESIGN.md 4i has the specification): every image of a
// batch carries up to four slots (op, argument); slot s reads the bytes slot s - 1 wrote.  Per slot, for all images at once:
//   hist_kernel     per-channel 256-bin histograms of the images whose op needs statistics (AutoContrast, Equalize,
//                   Contrast): a workgroup walks 32 KB of one image as aligned dwords, counts in LDS (one copy per wave:
//                   four waves do not queue on one address) and merges its non-zero bins into the workspace with 32-bit
//                   integer vector atomics.  Integer sums: the same counts whatever the order.
//   table_kernel    one wave per (image, channel) turns statistics or the argument into a 256-entry byte table; a lane
//                   owns four consecutive bins, the Equalize prefix sum is a wave scan.
//   apply_kernel    one launch over all images; a workgroup reads its image's op and does a table look-up, a warp or a copy
//                   over 8 KB of the image taken as aligned dwords (a dword that lies wholly in the image is stored whole,
//                   the up to three bytes at either end one by one), or a 64 x 32 sharpen tile staged in LDS with its halo.
// packed_image.h has the rule that lets a kernel take an image or a row that starts on any byte as aligned dwords.
// Arithmetic: tables in fp64 (Brightness in fp32), the sharpen blend in fp32, warp coordinates, weights and sums in fp64,
// every multiply and add rounded on its own: the Makefile builds this file with -ffp-contract=off (FLAGS_randaug), because
// a fused multiply-add decides differently which side of an integer a value lands on.  A pragma here would not do: with
// -ffp-contract=fast on the command line the backend fuses regardless.  Nothing depends on an image's
// position in the table.
#include <algorithm>
#include <cmath>
#include <vector>

#include "packed_image.h"

namespace {

constexpr int HIST_BYTES = 32768;      // bytes of an image per hist_kernel workgroup
constexpr int LIN_BYTES = 8192;        // bytes of an image per apply_kernel workgroup (table, warp, copy)
constexpr int TW = 64, TH = 32;        // sharpen tile, pixels
constexpr int SPITCH = packed::row_pitch((TW + 2) * 3);        // bytes of a staged row: the tile and its halo

__host__ __device__ inline bool needs_stats(int op) {
    return op == VLMO_AUG_AUTOCONTRAST || op == VLMO_AUG_EQUALIZE || op == VLMO_AUG_CONTRAST;
}
__host__ __device__ inline bool is_table(int op) {
    return needs_stats(op) || op == VLMO_AUG_BRIGHTNESS || op == VLMO_AUG_SOLARIZE || op == VLMO_AUG_POSTERIZE;
}
__host__ __device__ inline bool is_warp(int op) { return op >= VLMO_AUG_SHEAR_X && op <= VLMO_AUG_ROTATE; }
// PIL's Sharpness: factor 1 and images without an interior are copies
__host__ __device__ inline bool is_sharpen(const VlmoAugSlot& s, int H, int W) {
    return s.op == VLMO_AUG_SHARPNESS && s.a != 1.0 && H >= 3 && W >= 3;
}

struct Layout {        // the workspace: histograms uint32 [n_images][3][256], then tables uint8 [n_images][3][256]
    uint32_t* hist;
    uint8_t* table;
};

__global__ __launch_bounds__(256) void hist_kernel(const uint8_t* __restrict__ src, const VlmoImage* __restrict__ images,
                                                   const VlmoAugSlot* __restrict__ slots, int n_slots, int slot,
                                                   uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[4][768];
    const int img = blockIdx.x;
    if (!needs_stats(slots[(size_t)img * n_slots + slot].op)) return;
    const packed::Span sp(images[img]);
    const size_t begin = sp.begin, end = sp.end, a0 = sp.slice(blockIdx.y, HIST_BYTES);
    if (a0 >= end) return;
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < 4 * 768; i += 256) (&s_h[0][0])[i] = 0;
    __syncthreads();
    uint32_t* h = s_h[wave];
#pragma unroll 4
    for (int i = 0; i < HIST_BYTES / 1024; ++i) {
        const size_t a = a0 + (size_t)i * 1024 + (size_t)tid * 4;
        if (a < end) {                              // a + 3 < buffer size: the buffer is a multiple of 4 bytes long
            const uint32_t v = *(const uint32_t*)(src + a);
            uint32_t c = sp.channel(a);                 // also the channel of byte a + 3; walk backwards from there
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                if (a + j >= begin && a + j < end) atomicAdd(&h[c * 256 + ((v >> (8 * j)) & 0xFF)], 1u);
                c = c == 0 ? 2 : c - 1;
            }
        }
    }
    __syncthreads();
    for (int b = tid; b < 768; b += 256) {
        const uint32_t n = s_h[0][b] + s_h[1][b] + s_h[2][b] + s_h[3][b];
        if (n) atomicAdd(&hist[(size_t)img * 768 + b], n);
    }
}

template <typename T> __device__ __forceinline__ T wave_min_i(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
    return v;
}
template <typename T> __device__ __forceinline__ T wave_max_i(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t clip_trunc(double t) {
    t = t < 0.0 ? 0.0 : t;
    t = t > 255.0 ? 255.0 : t;
    return (uint32_t)(int)t;
}

// One wave per (image, channel); lane l owns bins 4 l .. 4 l + 3 and writes them as one dword.
__global__ __launch_bounds__(256) void table_kernel(const VlmoImage* __restrict__ images, const VlmoAugSlot* __restrict__ slots,
                                                    int n_images, int n_slots, int slot, Layout L) {
    const int lane = threadIdx.x & 63;
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (job >= n_images * 3) return;
    const int img = job / 3, ch = job - img * 3;
    const VlmoAugSlot S = slots[(size_t)img * n_slots + slot];
    if (!is_table(S.op)) return;
    const VlmoImage I = images[img];
    const int npix = I.H * I.W;                     // <= 8192 * 8192 = 2^26
    uint32_t* hist = L.hist + (size_t)img * 768;
    uint32_t t[4];
    const int k0 = lane * 4;
    if (S.op == VLMO_AUG_BRIGHTNESS) {
        const float f = (float)S.a;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = (float)(k0 + j) * f;
            v = v < 0.f ? 0.f : v;
            v = v > 255.f ? 255.f : v;
            t[j] = (uint32_t)(int)v;
        }
    } else if (S.op == VLMO_AUG_SOLARIZE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = (double)(k0 + j) < S.a ? k0 + j : 255 - (k0 + j);
    } else if (S.op == VLMO_AUG_POSTERIZE) {
        const uint32_t mask = (0xFFu << (8 - (int)S.a)) & 0xFFu;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = (uint32_t)(k0 + j) & mask;
    } else if (S.op == VLMO_AUG_CONTRAST) {          // one table for the three channels, from the three channel means
        double m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint4 h = *(const uint4*)(hist + c * 256 + k0);
            const unsigned long long part = (unsigned long long)h.x * k0 + (unsigned long long)h.y * (k0 + 1) +
                                            (unsigned long long)h.z * (k0 + 2) + (unsigned long long)h.w * (k0 + 3);
            m[c] = (double)wave_sum_u64(part) / (double)npix;
        }
        const double mean = (0.114 * m[0] + 0.587 * m[1]) + 0.299 * m[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = clip_trunc(((double)(k0 + j) - mean) * S.a + mean);
    } else {                                         // AutoContrast, Equalize: this channel's histogram
        const uint4 h4 = *(const uint4*)(hist + ch * 256 + k0);
        const uint32_t h[4] = {h4.x, h4.y, h4.z, h4.w};
        int lo = 256, hi = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (h[j]) {
                lo = lo < k0 + j ? lo : k0 + j;
                hi = k0 + j;
            }
        lo = wave_min_i(lo);
        hi = wave_max_i(hi);
        if (S.op == VLMO_AUG_AUTOCONTRAST) {
            if (hi <= lo) {
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = k0 + j;
            } else {
                const double s = 255.0 / (double)(hi - lo);
                const double o = -(double)lo * s;
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = clip_trunc((double)(k0 + j) * s + o);
            }
        } else {
            // bins below this lane's: inclusive wave scan of the lane sums, minus the own sum
            const uint32_t own = h[0] + h[1] + h[2] + h[3];
            uint32_t inc = own;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t u = __shfl_up(inc, o, 64);
                if (lane >= o) inc += u;
            }
            const uint32_t h_last = __shfl(h[hi & 3], hi >> 2, 64);     // hi >= 0: an image has at least one pixel
            const uint32_t step = ((uint32_t)npix - h_last) / 255u;
            uint32_t below = inc - own;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (step == 0) {
                    t[j] = k0 + j;
                } else {
                    const uint32_t q = (step / 2 + below) / step;
                    t[j] = q < 255u ? q : 255u;
                }
                below += h[j];
            }
        }
    }
    *(uint32_t*)(L.table + (size_t)job * 256 + k0) = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);
}

// The affine map of a warp op: source (sx, sy) = (m00 dx + m01 dy + ox, m10 dx + m11 dy + oy), dx = x - cx, dy = y - cy.
// With the unused terms exactly 1, 0 or -f these are the bits of the short forms (x - f y, x + off, ...).
struct Affine {
    double m00, m01, m10, m11, cx, cy, ox, oy;
    __device__ __forceinline__ Affine(const VlmoAugSlot& S, int H, int W) {
        m00 = 1.0, m01 = 0.0, m10 = 0.0, m11 = 1.0, cx = 0.0, cy = 0.0, ox = 0.0, oy = 0.0;
        switch (S.op) {
            case VLMO_AUG_SHEAR_X: m01 = -S.a; break;
            case VLMO_AUG_SHEAR_Y: m10 = -S.a; break;
            case VLMO_AUG_TRANSLATE_X: ox = S.a; break;
            case VLMO_AUG_TRANSLATE_Y: oy = S.a; break;
            default:                                 // Rotate: a = cos, b = sin of the angle
                m00 = S.a, m01 = -S.b, m10 = S.b, m11 = S.a;
                cx = ox = 0.5 * (double)W, cy = oy = 0.5 * (double)H;
        }
    }
};

// Bilinear sample of pixel p (row-major index) of an H x W x 3 image at `img`: the four tap byte offsets (-1 = fill) and weights
struct Taps {
    int off[4];
    double w[4];
    __device__ __forceinline__ Taps(const Affine& A, int p, int H, int W) {
        const int y = p / W, x = p - y * W;
        const double dx = (double)x - A.cx, dy = (double)y - A.cy;
        const double sx = (A.m00 * dx + A.m01 * dy) + A.ox;
        const double sy = (A.m10 * dx + A.m11 * dy) + A.oy;
        const double fx0 = floor(sx), fy0 = floor(sy);
        const double fx = sx - fx0, fy = sy - fy0;
        w[0] = (1.0 - fx) * (1.0 - fy);
        w[1] = fx * (1.0 - fy);
        w[2] = (1.0 - fx) * fy;
        w[3] = fx * fy;
        // taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1); a coordinate far outside never becomes an int
        const bool near = fx0 >= -1.0 && fx0 <= (double)W && fy0 >= -1.0 && fy0 <= (double)H;
        const int x0 = near ? (int)fx0 : -2, y0 = near ? (int)fy0 : -2;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
            off[t] = (tx >= 0 && tx < W && ty >= 0 && ty < H) ? (ty * W + tx) * 3 : -1;
        }
    }
    __device__ __forceinline__ uint32_t sample(const uint8_t* img, int c, double fill) const {
        double p[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) p[t] = off[t] >= 0 ? (double)img[off[t] + c] : fill;
        const double v = ((w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]) + w[3] * p[3];
        const double r = floor(v + 0.5);
        return (uint32_t)(int)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));
    }
};

__global__ __launch_bounds__(256) void apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                    const VlmoImage* __restrict__ images, const VlmoAugSlot* __restrict__ slots,
                                                    int n_slots, int slot, const uint8_t* __restrict__ tables, int fill) {
    __shared__ __attribute__((aligned(16))) uint8_t s_in[(TH + 2) * SPITCH];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[TH * TW * 3];
    const int img = blockIdx.x, tid = threadIdx.x;
    const VlmoAugSlot S = slots[(size_t)img * n_slots + slot];
    const VlmoImage I = images[img];
    const int H = I.H, W = I.W;
    const packed::Span sp(I);
    const size_t begin = sp.begin, end = sp.end;

    if (is_sharpen(S, H, W)) {
        const int tiles_x = (W + TW - 1) / TW;
        const int ty = blockIdx.y / tiles_x, tx = blockIdx.y - ty * tiles_x;
        const int x0 = tx * TW, y0 = ty * TH;
        if (y0 >= H) return;
        const int tw = min(TW, W - x0), th = min(TH, H - y0);
        // staged window: columns cl .. cr, rows rt .. rb (inclusive), clipped to the image
        const int cl = max(x0 - 1, 0), cr = min(x0 + tw, W - 1), rt = max(y0 - 1, 0), rb = min(y0 + th, H - 1);
        const size_t row_bytes = (size_t)W * 3, first0 = begin + (size_t)rt * row_bytes + (size_t)cl * 3;
        packed::stage_rows(s_in, SPITCH, src, first0, row_bytes, rb - rt + 1, (cr - cl + 1) * 3);
        __syncthreads();
        const float f = (float)S.a;
        for (int i = tid; i < th * TW; i += 256) {
            const int ly = i / TW, lx = i - ly * TW;
            if (lx >= tw) continue;
            const int x = x0 + lx, y = y0 + ly;
            // byte of pixel (y, x), channel 0, in the staged window
            const size_t first = first0 + (size_t)(y - rt) * row_bytes;
            const uint8_t* c = packed::staged_row(s_in, y - rt, SPITCH, first) + (x - cl) * 3;
            uint8_t* o = s_out + (ly * TW + lx) * 3;
            if (x == 0 || y == 0 || x == W - 1 || y == H - 1) {
                o[0] = c[0], o[1] = c[1], o[2] = c[2];
                continue;
            }
            // the rows above and below start at their own phase
            const uint8_t* u = packed::staged_row(s_in, y - 1 - rt, SPITCH, first - row_bytes) + (x - cl) * 3;
            const uint8_t* d = packed::staged_row(s_in, y + 1 - rt, SPITCH, first + row_bytes) + (x - cl) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int px = c[k];
                const int sum = u[k - 3] + u[k] + u[k + 3] + c[k - 3] + 5 * px + c[k + 3] + d[k - 3] + d[k] + d[k + 3];
                const int deg = (sum + 6) / 13;
                float v = (float)deg + f * (float)(px - deg);
                v = v < 0.f ? 0.f : v;
                v = v > 255.f ? 255.f : v;
                o[k] = (uint8_t)(int)v;
            }
        }
        __syncthreads();
        const int odw = (tw * 3 + 3 + 3) / 4;
        for (int i = tid; i < th * odw; i += 256) {
            const int r = i / odw;
            packed::store_row_dword(dst, begin + ((size_t)(y0 + r) * W + x0) * 3, tw * 3, s_out + r * TW * 3, i - r * odw);
        }
        return;
    }

    const size_t a0 = sp.slice(blockIdx.y, LIN_BYTES);
    if (a0 >= end) return;
    const bool table = is_table(S.op), warp = is_warp(S.op);
    uint8_t* s_tab = s_in;                           // 768 bytes of the sharpen window's LDS
    if (table) {
        if (tid < 192) ((uint32_t*)s_tab)[tid] = ((const uint32_t*)(tables + (size_t)img * 768))[tid];
        __syncthreads();
    }
    const Affine A(S, H, W);
    const uint8_t* base = src + begin;
    const double dfill = (double)fill;
#pragma unroll 2
    for (int i = 0; i < LIN_BYTES / 1024; ++i) {
        const size_t a = a0 + (size_t)i * 1024 + (size_t)tid * 4;
        if (a >= end) break;
        uint32_t v = 0;
        if (!warp) v = *(const uint32_t*)(src + a);
        // byte j of the dword is byte rel + j of the image; rel may be -3 .. -1 at the first dword
        const long long rel = (long long)a - (long long)begin;
        uint32_t out = v;
        if (table) {
            int c = (int)sp.channel(a);              // channel of byte j is (c + j) mod 3
            out = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                out |= (uint32_t)s_tab[c * 256 + ((v >> (8 * j)) & 0xFF)] << (8 * j);
                c = c == 2 ? 0 : c + 1;
            }
        } else if (warp) {
            // the dword's bytes inside the image belong to at most two pixels
            const long long b_lo = rel < 0 ? 0 : rel, b_hi = min(rel + 3, (long long)(end - begin) - 1);
            const int p_lo = (int)(b_lo / 3), p_hi = (int)(b_hi / 3);
            const Taps T0(A, p_lo, H, W);
            const Taps T1 = p_hi != p_lo ? Taps(A, p_hi, H, W) : T0;
            out = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long b = rel + j;
                if (b < b_lo || b > b_hi) continue;
                const int p = (int)(b / 3), c = (int)(b - (long long)p * 3);
                out |= (p == p_lo ? T0 : T1).sample(base, c, dfill) << (8 * j);
            }
        }
        if (rel >= 0 && a + 4 <= end) {
            *(uint32_t*)(dst + a) = out;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (rel + j >= 0 && a + j < end) dst[a + j] = (uint8_t)(out >> (8 * j));
        }
    }
}

int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

extern "C" int64_t vlmo_randaug_ws_bytes(int n_images) {
    return n_images < 1 ? 0 : (int64_t)n_images * (768 * 4 + 768);
}

extern "C" int vlmo_randaug(const uint8_t* src, uint8_t* out, uint8_t* scratch, int64_t nbytes, const VlmoImage* images,
                            const VlmoImage* images_dev, int n_images, const VlmoAugSlot* slots,
                            const VlmoAugSlot* slots_dev, int n_slots, int fill, void* ws, int64_t ws_bytes,
                            hipStream_t stream) {
    VLMO_CHECK_ARG(n_slots >= 1 && n_slots <= VLMO_AUG_MAX_SLOTS, "vlmo_randaug: need 1 <= slots per image <= %d (got %d)",
                   VLMO_AUG_MAX_SLOTS, n_slots);
    VLMO_CHECK_ARG(src && out && images && images_dev && slots && slots_dev && ws && (scratch || n_slots == 1),
                   "vlmo_randaug: null pointer");
    {
        const uintptr_t p[3] = {(uintptr_t)src, (uintptr_t)out, (uintptr_t)scratch};
        for (int i = 0; i < 3; ++i)
            for (int j = i + 1; j < 3; ++j)
                VLMO_CHECK_ARG(!p[i] || !p[j] || p[i] + (uintptr_t)nbytes <= p[j] || p[j] + (uintptr_t)nbytes <= p[i],
                               "vlmo_randaug: source, result and scratch must not overlap");
    }
    VLMO_CHECK_ARG(n_images >= 1 && n_images <= VLMO_AUG_MAX_IMAGES, "vlmo_randaug: need 1 <= images <= %d per call (got %d)",
                   VLMO_AUG_MAX_IMAGES, n_images);
    if (packed::check_packed("vlmo_randaug", "three buffers", (uintptr_t)src | (uintptr_t)out | (uintptr_t)scratch, nbytes,
                             images, n_images, VLMO_CROP_MAX_SIDE))
        return -1;
    VLMO_CHECK_ARG(fill >= 0 && fill <= 255, "vlmo_randaug: fill %d outside [0, 255]", fill);
    VLMO_CHECK_ARG((uintptr_t)ws % 16 == 0 && ws_bytes >= vlmo_randaug_ws_bytes(n_images),
                   "vlmo_randaug: workspace too small or not 16-byte aligned (need %lld bytes, got %lld)",
                   (long long)vlmo_randaug_ws_bytes(n_images), (long long)ws_bytes);
    std::vector<int> order(n_images);
    for (int i = 0; i < n_images; ++i) order[i] = i;
    // every slot rewrites every image in place of the batch: two images that share bytes would race
    std::sort(order.begin(), order.end(), [&](int a, int b) { return images[a].offset < images[b].offset; });
    for (int i = 1; i < n_images; ++i) {
        const VlmoImage& P = images[order[i - 1]];
        VLMO_CHECK_ARG(P.offset + (int64_t)P.H * P.W * 3 <= images[order[i]].offset, "vlmo_randaug: images %d and %d overlap",
                       order[i - 1], order[i]);
    }
    bool stats[VLMO_AUG_MAX_SLOTS] = {}, tables[VLMO_AUG_MAX_SLOTS] = {};
    int64_t hist_blocks[VLMO_AUG_MAX_SLOTS] = {}, apply_blocks[VLMO_AUG_MAX_SLOTS] = {};
    for (int i = 0; i < n_images; ++i) {
        const VlmoImage& I = images[i];
        const int64_t span = (I.offset & 3) + (int64_t)I.H * I.W * 3;       // from the first aligned dword to the end
        for (int s = 0; s < n_slots; ++s) {
            const VlmoAugSlot& S = slots[(size_t)i * n_slots + s];
            VLMO_CHECK_ARG(S.op >= VLMO_AUG_SKIP && S.op <= VLMO_AUG_CONTRAST, "vlmo_randaug: image %d slot %d: unknown op %d", i,
                           s, S.op);
            VLMO_CHECK_ARG(std::isfinite(S.a) && std::isfinite(S.b), "vlmo_randaug: image %d slot %d: non-finite argument", i, s);
            if (S.op == VLMO_AUG_POSTERIZE)
                VLMO_CHECK_ARG(S.a >= 0.0 && S.a <= 8.0 && S.a == std::floor(S.a),
                               "vlmo_randaug: image %d slot %d: posterize bits %g not an integer in [0, 8]", i, s, S.a);
            if (S.op >= VLMO_AUG_SHEAR_X && S.op <= VLMO_AUG_TRANSLATE_Y)
                VLMO_CHECK_ARG(std::fabs(S.a) <= VLMO_AUG_MAX_SHIFT,
                               "vlmo_randaug: image %d slot %d: shear / translate argument %g outside [-%d, %d]", i, s, S.a,
                               VLMO_AUG_MAX_SHIFT, VLMO_AUG_MAX_SHIFT);
            if (S.op == VLMO_AUG_ROTATE)
                VLMO_CHECK_ARG(std::fabs(S.a) <= 1.0 && std::fabs(S.b) <= 1.0,
                               "vlmo_randaug: image %d slot %d: rotate takes the cosine and sine of the angle (%g, %g)", i, s, S.a,
                               S.b);
            if (needs_stats(S.op)) {
                stats[s] = true;
                hist_blocks[s] = std::max(hist_blocks[s], cdiv64(span, HIST_BYTES));
            }
            tables[s] = tables[s] || is_table(S.op);
            const int64_t nb = is_sharpen(S, I.H, I.W) ? cdiv64(I.W, TW) * cdiv64(I.H, TH) : cdiv64(span, LIN_BYTES);
            apply_blocks[s] = std::max(apply_blocks[s], nb);
        }
    }
    Layout L;
    L.hist = (uint32_t*)ws;
    L.table = (uint8_t*)ws + (size_t)n_images * 768 * 4;
    const size_t hist_bytes = (size_t)n_images * 768 * 4;
    const uint8_t* in = src;
    for (int s = 0; s < n_slots; ++s) {
        uint8_t* to = ((n_slots - 1 - s) & 1) ? scratch : out;
        if (stats[s]) {
            hipError_t e = hipMemsetAsync(L.hist, 0, hist_bytes, stream);
            if (e != hipSuccess) {
                vlmo_set_error("vlmo_randaug: hipMemsetAsync failed: %s", hipGetErrorString(e));
                return (int)e;
            }
            hipLaunchKernelGGL(hist_kernel, dim3(n_images, (unsigned)hist_blocks[s]), dim3(256), 0, stream, in, images_dev,
                               slots_dev, n_slots, s, L.hist);
            VLMO_CHECK_LAUNCH("vlmo_randaug(histogram)");
        }
        if (tables[s]) {
            hipLaunchKernelGGL(table_kernel, dim3((unsigned)cdiv64((int64_t)n_images * 3, 4)), dim3(256), 0, stream, images_dev,
                               slots_dev, n_images, n_slots, s, L);
            VLMO_CHECK_LAUNCH("vlmo_randaug(tables)");
        }
        hipLaunchKernelGGL(apply_kernel, dim3(n_images, (unsigned)apply_blocks[s]), dim3(256), 0, stream, in, to, images_dev,
                           slots_dev, n_slots, s, L.table, fill);
        VLMO_CHECK_LAUNCH("vlmo_randaug(apply)");
        in = to;
    }
    return 0;
}
