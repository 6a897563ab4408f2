// Frame ingest: Pillow's antialiased 8-bit BILINEAR resize (Resample.c, ImagingResampleHorizontal_8bpc / Vertical_8bpc) on the device.
// The taps come from the host (xmem2_amd/pil_resize.py restates precompute_coeffs + normalize_coeffs_8bpc): per output sample a
// window (first, count) of the source axis and `count` int32 weights with 22 fractional bits.  One axis pass is
//
//   out = clamp((2^21 + sum_k src[first + k] * coeff[k]) >> 22, 0, 255)          per channel, int32 accumulator
//
// (255 * (2^22 + ksize) < 2^31: no overflow).  The horizontal pass runs first and is rounded to uint8, the vertical pass runs on that
// uint8 intermediate - the order and the rounding points of the host library, so the result is the same bytes.  Integer arithmetic
// only, no atomics: the same input gives the same bits.  `flip` mirrors the output columns in the last pass that touches columns.
//
// One thread per output pixel (3 channels, byte loads and stores, the tap row re-read per thread), two launches: the plain first form.
// From the byte counts (6 MB in, 1.2 MB out per 1080p frame, ~6 integer MACs per byte) the stage is EXPECTED to be bound by its
// launches and the H2D copy in front of it rather than by arithmetic; none of that is measured yet (profiles/r07_resize_ingest.txt
// lists what to measure), so neither this form's cost nor what a fused, LDS-staged form would save is known.
#include "common.hpp"

#define RSZ_MAX_SIDE 16384
#define RSZ_THREADS 256
#define RSZ_BITS 22

namespace {

__device__ __forceinline__ uint8_t rsz_clip8(int acc) {
    const int v = acc >> RSZ_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// The window of output sample `o`, clamped to the source axis and to the table's row: a wrong table can give wrong pixels, never a
// read outside the source.
__device__ __forceinline__ void rsz_window(const int* __restrict__ bounds, int o, int in_size, int ksize, int& first, int& count) {
    first = bounds[2 * o];
    count = bounds[2 * o + 1];
    first = first < 0 ? 0 : (first > in_size ? in_size : first);
    count = count < ksize ? count : ksize;
    count = count < in_size - first ? count : in_size - first;
}

// src [H][Ws][3] -> dst [H][Wd][3]; dst column Wd - 1 - x when flip.
__global__ __launch_bounds__(RSZ_THREADS) void resize_h_kernel(const uint8_t* __restrict__ src, int H, int Ws, uint8_t* __restrict__ dst,
                                                               int Wd, int flip, const int* __restrict__ bounds,
                                                               const int* __restrict__ coeffs, int ksize) {
    const int i = blockIdx.x * RSZ_THREADS + threadIdx.x;
    if (i >= H * Wd) return;
    const int y = i / Wd, x = i - y * Wd;
    int first, count;
    rsz_window(bounds, x, Ws, ksize, first, count);
    const uint8_t* p = src + ((size_t)y * Ws + first) * 3;
    const int* k = coeffs + (size_t)x * ksize;
    int a0 = 1 << (RSZ_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < count; ++t) {
        const int c = k[t];
        a0 += p[3 * t] * c;
        a1 += p[3 * t + 1] * c;
        a2 += p[3 * t + 2] * c;
    }
    uint8_t* o = dst + ((size_t)y * Wd + (flip ? Wd - 1 - x : x)) * 3;
    o[0] = rsz_clip8(a0);
    o[1] = rsz_clip8(a1);
    o[2] = rsz_clip8(a2);
}

// src [Hs][W][3] -> dst [Hd][W][3]; dst column W - 1 - x when flip.
__global__ __launch_bounds__(RSZ_THREADS) void resize_v_kernel(const uint8_t* __restrict__ src, int Hs, int W, uint8_t* __restrict__ dst,
                                                               int Hd, int flip, const int* __restrict__ bounds,
                                                               const int* __restrict__ coeffs, int ksize) {
    const int i = blockIdx.x * RSZ_THREADS + threadIdx.x;
    if (i >= Hd * W) return;
    const int y = i / W, x = i - y * W;
    int first, count;
    rsz_window(bounds, y, Hs, ksize, first, count);
    const size_t row = (size_t)W * 3;
    const uint8_t* p = src + (size_t)first * row + (size_t)x * 3;
    const int* k = coeffs + (size_t)y * ksize;
    int a0 = 1 << (RSZ_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < count; ++t) {
        const int c = k[t];
        a0 += p[0] * c;
        a1 += p[1] * c;
        a2 += p[2] * c;
        p += row;
    }
    uint8_t* o = dst + ((size_t)y * W + (flip ? W - 1 - x : x)) * 3;
    o[0] = rsz_clip8(a0);
    o[1] = rsz_clip8(a1);
    o[2] = rsz_clip8(a2);
}

// neither axis changes: a copy, or the mirror
__global__ __launch_bounds__(RSZ_THREADS) void copy_mirror_kernel(const uint8_t* __restrict__ src, int H, int W, uint8_t* __restrict__ dst,
                                                                  int flip) {
    const int i = blockIdx.x * RSZ_THREADS + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    const uint8_t* p = src + (size_t)i * 3;
    uint8_t* o = dst + ((size_t)y * W + (flip ? W - 1 - x : x)) * 3;
    o[0] = p[0];
    o[1] = p[1];
    o[2] = p[2];
}

inline bool rsz_size_ok(int Hs, int Ws, int Hd, int Wd) {
    return Hs <= RSZ_MAX_SIDE && Ws <= RSZ_MAX_SIDE && Hd <= RSZ_MAX_SIDE && Wd <= RSZ_MAX_SIDE;
}

}  // namespace

extern "C" size_t xmem_resize_u8_workspace_bytes(int Hs, int Ws, int Hd, int Wd) {
    if (Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || !rsz_size_ok(Hs, Ws, Hd, Wd)) return 0;
    return (Hs != Hd && Ws != Wd) ? (size_t)Hs * Wd * 3 : 0;       // the horizontal pass's uint8 result, when both passes run
}

extern "C" int xmem_resize_u8_bilinear_aa(const uint8_t* src, int Hs, int Ws, uint8_t* dst, int Hd, int Wd, int flip,
                                          const int32_t* xbounds, const int32_t* xcoeffs, int xksize, const int32_t* ybounds,
                                          const int32_t* ycoeffs, int yksize, void* workspace, size_t workspace_bytes, void* stream) {
    if (!src || !dst || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) return XMEM_ERR_BAD_ARG;
    if (!rsz_size_ok(Hs, Ws, Hd, Wd)) return XMEM_ERR_UNSUPPORTED;
    const bool horiz = Ws != Wd, vert = Hs != Hd;
    if (horiz && (!xbounds || !xcoeffs || xksize <= 0)) return XMEM_ERR_BAD_ARG;
    if (vert && (!ybounds || !ycoeffs || yksize <= 0)) return XMEM_ERR_BAD_ARG;
    if (horiz && vert && (!workspace || workspace_bytes < xmem_resize_u8_workspace_bytes(Hs, Ws, Hd, Wd))) return XMEM_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    flip = flip != 0;
    if (!horiz && !vert) {
        hipLaunchKernelGGL(copy_mirror_kernel, dim3(cdiv(Hs * Ws, RSZ_THREADS)), dim3(RSZ_THREADS), 0, s, src, Hs, Ws, dst, flip);
        return xmem_check_launch();
    }
    const uint8_t* vin = src;
    if (horiz) {
        uint8_t* hout = vert ? (uint8_t*)workspace : dst;
        hipLaunchKernelGGL(resize_h_kernel, dim3(cdiv(Hs * Wd, RSZ_THREADS)), dim3(RSZ_THREADS), 0, s, src, Hs, Ws, hout, Wd, flip,
                           (const int*)xbounds, (const int*)xcoeffs, xksize);
        const int rc = xmem_check_launch();
        if (rc != XMEM_OK || !vert) return rc;
        vin = hout;
    }
    hipLaunchKernelGGL(resize_v_kernel, dim3(cdiv(Hd * Wd, RSZ_THREADS)), dim3(RSZ_THREADS), 0, s, vin, Hs, Wd, dst, Hd,
                       horiz ? 0 : flip, (const int*)ybounds, (const int*)ycoeffs, yksize);
    return xmem_check_launch();
}
