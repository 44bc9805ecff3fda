// A packed batch: uint8 HWC images laid end to end in one byte buffer, plus a table of VlmoImage (offset, H, W).  The rule
// that the crop (augment.hip) and RandAugment (randaug.hip) share: an image or a row may start on ANY byte;
// the buffer itself is 4-byte aligned and a multiple of 4 bytes long, so the aligned dword that holds any byte of an image
// lies inside the buffer.  Kernels therefore read, and where all four bytes are theirs write, whole aligned dwords, and
// find a byte again at its phase `address & 3`.  check_packed is the host side of the rule.
// Integer arithmetic only: nothing here depends on the floating-point contraction flag of the file that includes it.
#pragma once
#include "common.h"
#include "vlmo_hip.h"

namespace packed {

// aligned dwords that hold n bytes whatever byte they start on, and the LDS pitch of a staged row of n bytes: the bytes
// and up to 3 leading bytes of the first dword, rounded up to 8
constexpr int row_dwords(int n) { return (n + 3 + 3) / 4; }
constexpr int row_pitch(int n) { return (n + 3 + 7) / 8 * 8; }

// All 256 threads: rows 0 .. nrows - 1 of nbytes each go to LDS as the aligned dwords that hold them and no others.  Row r
// starts at byte first0 + r * stride of src and lands at s + r * pitch; staged_row finds its byte 0 there.
__device__ __forceinline__ void stage_rows(uint8_t* s, int pitch, const uint8_t* __restrict__ src, size_t first0,
                                           size_t stride, int nrows, int nbytes) {
    const int ndw = row_dwords(nbytes);
    for (int i = threadIdx.x; i < nrows * ndw; i += 256) {
        const int r = i / ndw, d = i - r * ndw;
        const size_t first = first0 + (size_t)r * stride;
        const size_t a = (first & ~(size_t)3) + 4 * (size_t)d;
        if (a < first + nbytes) *(uint32_t*)(s + r * pitch + 4 * d) = *(const uint32_t*)(src + a);
    }
}

// byte 0 of staged row `row`, whose first byte has the buffer address `first`
__device__ __forceinline__ const uint8_t* staged_row(const uint8_t* s, int row, int pitch, size_t first) {
    return s + row * pitch + (int)(first & 3);
}

// dword d (counted from the aligned dword that holds byte `first`) of the bytes [first, first + n) of dst, taken from the LDS
// bytes s[0 .. n): stored whole where all four bytes are ours, else byte by byte
__device__ __forceinline__ void store_row_dword(uint8_t* dst, size_t first, int n, const uint8_t* s, int d) {
    const size_t a0 = first & ~(size_t)3;
    const int b = 4 * d - (int)(first - a0);         // index in s of the dword's first byte
    if (b >= n) return;
    if (b >= 0 && b + 4 <= n) {
        *(uint32_t*)(dst + a0 + 4 * (size_t)d) = (uint32_t)s[b] | ((uint32_t)s[b + 1] << 8) | ((uint32_t)s[b + 2] << 16) |
                                                  ((uint32_t)s[b + 3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (b + j >= 0 && b + j < n) dst[a0 + 4 * (size_t)d + j] = s[b + j];
    }
}

// The bytes [begin, end) of an image, walked as aligned dwords from the one that holds `begin`
struct Span {
    size_t begin, end;
    __device__ __forceinline__ explicit Span(const VlmoImage& I) : begin((size_t)I.offset), end(begin + (size_t)I.H * I.W * 3) {}
    // first dword of workgroup wg's slice of `bytes` bytes (a multiple of 4); past the image where this is >= end
    __device__ __forceinline__ size_t slice(unsigned wg, int bytes) const { return (begin & ~(size_t)3) + (size_t)wg * bytes; }
    // channel of the byte at address a; a - begin may be -3 .. -1 in the first dword, which starts before the image
    __device__ __forceinline__ uint32_t channel(size_t a) const { return (uint32_t)(((long long)a - (long long)begin + 3) % 3); }
};

// Host side, for the entry point `fn`: the buffers (`what` names them, `addr` is the OR of their addresses) 4-byte aligned
// and nbytes a positive multiple of 4, every image inside, and its sides at most max_side where that is not 0.
inline int check_packed(const char* fn, const char* what, uintptr_t addr, int64_t nbytes, const VlmoImage* images,
                        int n_images, int max_side) {
    VLMO_CHECK_ARG(addr % 4 == 0 && nbytes > 0 && nbytes % 4 == 0,
                   "%s: the %s must be 4-byte aligned and a multiple of 4 bytes long (%lld bytes)", fn, what, (long long)nbytes);
    for (int i = 0; i < n_images; ++i) {
        const VlmoImage& I = images[i];
        VLMO_CHECK_ARG(!max_side || (I.H >= 1 && I.W >= 1 && I.H <= max_side && I.W <= max_side),
                       "%s: image %d: sides must lie in [1, %d] (%d x %d)", fn, i, max_side, I.H, I.W);
        VLMO_CHECK_ARG(I.H >= 1 && I.W >= 1 && I.offset >= 0 && I.offset <= nbytes && (int64_t)I.H * I.W * 3 <= nbytes - I.offset,
                       "%s: image %d (offset %lld, %d x %d x 3) is not inside the %lld-byte buffer", fn, i, (long long)I.offset,
                       I.H, I.W, (long long)nbytes);
    }
    return 0;
}

}  // namespace packed
