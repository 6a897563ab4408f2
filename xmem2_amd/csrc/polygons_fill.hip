// Even-odd fill of polygon edges into uint8 index maps (include/xmem_hip_raster.h, xmem_polygons_fill; xmem2_amd/polygons.py,
// `fill_exact_host` / `fill_rows_host`, has the definition).  Integer arithmetic throughout.
//
// The workspace holds one toggle bit per (frame, row, image row, column 0..W): `planes` = N R bit-planes of H lines of WW =
// ceil((W + 1) / 32) words.  Launches, whatever the edges hold:
//   clear     the bit-planes and `status` (two memsets);
//   edges     a grid sized by E alone (none with E == 0).  A lane owns an edge: it checks the plane index and the coordinates, clips
//             its rows to [0, H) and walks them.  One walk costs one 64-bit division: num / den at the first row as floor quotient
//             and remainder, after that num grows by 2 one dx per row, so the quotient grows by floor(dx / dy) and the remainder by
//             2 one (dx mod dy), with a carry when it reaches den - the same c = ceil(num / den) as the definition's, row by row.
//             Each crossing is one atomicXor of one bit (column W, which no pixel reads, is left out); XOR commutes, so the planes
//             do not depend on the order.  Edges of at most FILL_SHORT rows are walked by their lane; the taller ones of a wave are
//             handed round with a ballot and walked by all 64 lanes, lane l taking the rows first + l, first + l + 64, ..
//   resolve   a wave owns a line (frame, image row) of the output and walks it in passes of 64 words = 2048 pixels, a lane owning
//             a word.  Per row, highest first: the prefix XOR inside the word by shifts, across the lanes by a ballot of the words'
//             parities, across the passes by a carry bit per row (bit row / 64 of lane row % 64); the bits that are new against the
//             rows above take values[row].  The lane's 32 bytes leave as two 16-byte stores where the address allows, as dwords or
//             bytes otherwise; under overlay the pixels in no row keep what they held.
// No workgroup waits for another, nothing is read back, and nothing is written outside masks, the workspace and status.
#include "common.hpp"
#include "../../include/xmem_hip_raster.h"

#define FILL_MAX_HW 16384
#define FILL_THREADS 256
#define FILL_WAVES (FILL_THREADS / XMEM_WAVE)
#define FILL_SHORT 8                // rows an edge may cross and still be walked by its own lane

namespace {

typedef unsigned long long u64;
typedef long long i64;

// Rows first, first + stride, .. below `last` of the edge (xa, ya) + (dx, dy), dy > 0, into the bit-plane `bits` (lines of WW words).
__device__ __forceinline__ void fill_walk(uint32_t* __restrict__ bits, int WW, int W, int one, int xa, int ya, int dx, int dy, int first,
                                          int last, int stride) {
    if (first >= last) return;
    const i64 den = 2ll * one * dy;
    const i64 num = 2ll * xa * dy + ((2ll * first + 1) * one - 2ll * ya) * dx - (i64)one * dy;
    i64 q = num / den, rem = num - q * den;
    if (rem < 0) { rem += den; --q; }
    const i64 sdx = (i64)dx * stride;
    i64 dq = sdx / dy, dm = sdx - dq * dy;
    if (dm < 0) { dm += dy; --dq; }
    const i64 dr = dm * 2 * one;                                     // < den
    for (int r = first; r < last; r += stride) {
        const i64 c = q + (rem > 0);                                 // ceil(num / den)
        if (c < W) {
            const int ci = c < 0 ? 0 : (int)c;
            atomicXor(bits + (size_t)r * WW + (ci >> 5), 1u << (ci & 31));
        }
        q += dq;
        rem += dr;
        if (rem >= den) { rem -= den; ++q; }
    }
}

__global__ __launch_bounds__(FILL_THREADS) void fill_edges_kernel(const int32_t* __restrict__ edges, const int32_t* __restrict__ plane, int E,
                                                                  int planes, int H, int W, int WW, int frac_bits,
                                                                  uint32_t* __restrict__ bits, int32_t* __restrict__ status) {
    const i64 e = (i64)blockIdx.x * FILL_THREADS + threadIdx.x;
    const int lane = threadIdx.x & (XMEM_WAVE - 1);
    const int one = 1 << frac_bits;
    const int B = XMEM_FILL_COORD_BOUND;
    int xa = 0, ya = 0, dx = 0, dy = 1, p = 0, first = 0, last = 0;
    if (e < E) {
        const int32_t* v = edges + 4 * e;
        const int xb = v[2], yb = v[3];
        xa = v[0];
        ya = v[1];
        p = plane[e];
        if (p < 0 || p >= planes) {
            atomicAdd(status + XMEM_FILL_BAD_PLANE, 1);
            p = 0;
        } else if (xa < -B || xa > B || ya < -B || ya > B || xb < -B || xb > B || yb < -B || yb > B) {
            atomicAdd(status + XMEM_FILL_BAD_COORD, 1);
        } else if (yb > ya) {
            dx = xb - xa;
            dy = yb - ya;
            // 2 ya <= (2 r + 1) one < 2 yb: r from ceil((2 ya - one) / (2 one)) to below ceil((2 yb - one) / (2 one)); >> floors
            first = (2 * ya + one - 1) >> (frac_bits + 1);
            last = (2 * yb + one - 1) >> (frac_bits + 1);
            first = first < 0 ? 0 : first;
            last = last > H ? H : last;
        }
    }
    const size_t plane_words = (size_t)H * WW;
    const bool tall = last - first > FILL_SHORT;
    if (!tall) fill_walk(bits + p * plane_words, WW, W, one, xa, ya, dx, dy, first, last, 1);
    u64 todo = __ballot(tall);
    while (todo) {                                                   // the same for every lane of the wave
        const int src = __ffsll(todo) - 1;
        todo &= todo - 1;
        fill_walk(bits + __shfl(p, src, XMEM_WAVE) * plane_words, WW, W, one, __shfl(xa, src, XMEM_WAVE), __shfl(ya, src, XMEM_WAVE),
                  __shfl(dx, src, XMEM_WAVE), __shfl(dy, src, XMEM_WAVE), __shfl(first, src, XMEM_WAVE) + lane, __shfl(last, src, XMEM_WAVE),
                  XMEM_WAVE);
    }
}

// bits 0..3 -> the bytes 0..3 as 0x00 / 0xff
__device__ __forceinline__ uint32_t fill_byte_mask(uint32_t nibble) { return ((nibble * 0x00204081u) & 0x01010101u) * 0xffu; }

__global__ __launch_bounds__(FILL_THREADS) void fill_resolve_kernel(const uint32_t* __restrict__ bits, int N, int H, int W, int WW, int R,
                                                                    const uint8_t* __restrict__ values, int overlay,
                                                                    uint8_t* __restrict__ masks) {
    const int lane = threadIdx.x & (XMEM_WAVE - 1);
    const i64 line = (i64)blockIdx.x * FILL_WAVES + (threadIdx.x / XMEM_WAVE);
    if (line >= (i64)N * H) return;                                  // the whole wave
    const int n = (int)(line / H), r = (int)(line - (i64)n * H);
    const u64 below = (1ull << lane) - 1;
    uint32_t carry = 0;                      // bit k / 64 of lane k % 64: the parity of row k's toggles in the passes before this one
    uint8_t* __restrict__ dst = masks + (size_t)line * W;
    for (int w0 = 0; w0 < WW; w0 += XMEM_WAVE) {
        const int wi = w0 + lane;
        const bool more = w0 + XMEM_WAVE < WW;
        uint32_t done = 0, val[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) val[j] = 0;
        for (int k = R - 1; k >= 0; --k) {
            uint32_t x = wi < WW ? bits[(((size_t)n * R + k) * H + r) * WW + wi] : 0u;
            x ^= x << 1;
            x ^= x << 2;
            x ^= x << 4;
            x ^= x << 8;
            x ^= x << 16;                                            // bit i: the parity of the word's toggles 0..i
            const u64 odd = __ballot(x >> 31);
            uint32_t in = (__shfl(carry, k & (XMEM_WAVE - 1), XMEM_WAVE) >> (k / XMEM_WAVE)) & 1u;
            in ^= __popcll(odd & below) & 1u;
            if (in) x = ~x;
            if (more && (__popcll(odd) & 1) && lane == (k & (XMEM_WAVE - 1))) carry ^= 1u << (k / XMEM_WAVE);
            const uint32_t fresh = x & ~done;
            if (fresh) {
                const uint32_t v = (values ? (uint32_t)values[k] : (uint32_t)(k + 1)) * 0x01010101u;
#pragma unroll
                for (int j = 0; j < 8; ++j) val[j] |= v & fill_byte_mask((fresh >> (4 * j)) & 15u);
            }
            done |= x;
        }
        const int c0 = wi * 32;
        uint8_t* d = dst + c0;
        const int count = W - c0 < 32 ? W - c0 : 32;                 // <= 0 for a lane beyond the line
        const bool keep = overlay && done != 0xffffffffu;
        if (count == 32 && !((uintptr_t)d & 3)) {
            if (keep) {
#pragma unroll
                for (int j = 0; j < 8; ++j) val[j] |= ((const uint32_t*)d)[j] & ~fill_byte_mask((done >> (4 * j)) & 15u);
            }
            if (!((uintptr_t)d & 15)) {
                ((uint4*)d)[0] = make_uint4(val[0], val[1], val[2], val[3]);
                ((uint4*)d)[1] = make_uint4(val[4], val[5], val[6], val[7]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) ((uint32_t*)d)[j] = val[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int i = 4 * j + b;
                    if (i < count && (!keep || ((done >> i) & 1u))) d[i] = (uint8_t)(val[j] >> (8 * b));
                }
        }
    }
}

int fill_check(int N, int H, int W, int R) {
    if (N < 1 || N > 65535 || R < 1 || R > 254) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > FILL_MAX_HW || W > FILL_MAX_HW) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

size_t fill_bit_bytes(int N, int H, int W, int R) { return (size_t)N * R * H * cdiv(W + 1, 32) * sizeof(uint32_t); }

}  // namespace

extern "C" size_t xmem_polygons_fill_workspace_bytes(int N, int H, int W, int R) {
    return fill_check(N, H, W, R) == XMEM_OK ? align_up(fill_bit_bytes(N, H, W, R), (size_t)256) : 0;
}

extern "C" int xmem_polygons_fill(const int32_t* edges, const int32_t* plane, int E, int N, int H, int W, int R, int frac_bits,
                                  const uint8_t* values, int overlay, uint8_t* masks, int32_t* status, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (E < 0 || frac_bits < 0 || frac_bits > XMEM_FILL_MAX_FRAC_BITS) return XMEM_ERR_BAD_ARG;
    int rc = fill_check(N, H, W, R);
    if (rc != XMEM_OK) return rc;
    if (!masks || !status || !workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)status & 3)) return XMEM_ERR_BAD_ARG;
    if (E > 0 && (!edges || !plane || ((uintptr_t)edges & 3) || ((uintptr_t)plane & 3))) return XMEM_ERR_BAD_ARG;
    if (workspace_bytes < xmem_polygons_fill_workspace_bytes(N, H, W, R)) return XMEM_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    uint32_t* bits = (uint32_t*)workspace;
    const int WW = cdiv(W + 1, 32);
    if (hipMemsetAsync(bits, 0, fill_bit_bytes(N, H, W, R), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    if (hipMemsetAsync(status, 0, XMEM_FILL_STATUS * sizeof(int32_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    if (E > 0) {
        hipLaunchKernelGGL(fill_edges_kernel, dim3((unsigned)cdiv(E, FILL_THREADS)), dim3(FILL_THREADS), 0, s, edges, plane, E, N * R, H, W,
                           WW, frac_bits, bits, status);
        rc = xmem_check_launch();
        if (rc != XMEM_OK) return rc;
    }
    const long long lines = (long long)N * H;
    hipLaunchKernelGGL(fill_resolve_kernel, dim3((unsigned)((lines + FILL_WAVES - 1) / FILL_WAVES)), dim3(FILL_THREADS), 0, s,
                       (const uint32_t*)bits, N, H, W, WW, R, values, overlay, masks);
    return xmem_check_launch();
}
