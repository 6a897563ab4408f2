// Four pixels at a time in packed bytes, shared by temporal.hip (the plain vote) and motion.hip (the motion-compensated one): the
// load and the store of four bytes at any alignment, and the majority vote - the window is an array of dwords, one per frame, and
// the frames that vote are marked by a mask per entry.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace {

// bytes a[0] .. a[nv - 1] as one dword, a[0] in the low byte, the rest zero.  [lo, hi) is the buffer `a` lies in.
__device__ __forceinline__ uint32_t load_bytes4(const uint8_t* a, int nv, const uint8_t* lo, const uint8_t* hi) {
    const unsigned mis = (unsigned)((uintptr_t)a & 3);
    const uint8_t* w = a - mis;
    if (nv == 4 && w >= lo && w + (mis ? 8 : 4) <= hi) {
        const uint32_t d0 = *(const uint32_t*)w;
        if (!mis) return d0;
        const uint32_t d1 = *(const uint32_t*)(w + 4);
        return (uint32_t)((((uint64_t)d1 << 32) | d0) >> (8 * mis));
    }
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < nv) v |= (uint32_t)a[k] << (8 * k);
    return v;
}

__device__ __forceinline__ void store_bytes4(uint8_t* q, uint32_t v, int nv) {
    if (nv == 4 && ((uintptr_t)q & 3) == 0) {
        *(uint32_t*)q = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < nv) q[k] = (uint8_t)(v >> (8 * k));
}

// 0x01 in every byte in which a and b agree
__device__ __forceinline__ uint32_t eq_bytes(uint32_t a, uint32_t b) {
    const uint32_t x = a ^ b;
    const uint32_t nz = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;           // bit 7 of a byte: the byte is not zero (no carry leaves a byte)
    return (~nz >> 7) & 0x01010101u;
}

// the larger of two keys per 16-bit lane; keys stay below 0x8000, so the borrow of a lane never reaches the next
__device__ __forceinline__ uint32_t max_keys(uint32_t a, uint32_t b) {
    const uint32_t ge = (((a | 0x80008000u) - b) >> 15) & 0x00010001u;
    const uint32_t m = ge * 0xffffu;
    return (a & m) | (b & ~m);
}

// the vote of four pixels: w the window, centre at R; vote[k] is 0x01010101 where entry k votes and 0 where it does not
template <int R>
__device__ __forceinline__ uint32_t vote_group(const uint32_t (&w)[2 * R + 1], const uint32_t (&vote)[2 * R + 1]) {
    constexpr int N = 2 * R + 1;
    uint32_t cnt[N], same[N];                                            // occurrences of the entry's label; 0x01 where it is the centre's
#pragma unroll
    for (int k = 0; k < N; ++k) cnt[k] = vote[k];
    same[R] = 0x01010101u;
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = i + 1; j < N; ++j) {
            const uint32_t e = eq_bytes(w[i], w[j]);
            if (i == R) same[j] = e;
            if (j == R) same[i] = e;
            const uint32_t both = e & vote[i] & vote[j];
            cnt[i] += both;
            cnt[j] += both;
        }
    }
    uint32_t best0 = 0, best1 = 0;                                       // pixels 0 and 2, pixels 1 and 3
#pragma unroll
    for (int k = 0; k < N; ++k) {                                        // an entry that does not vote has count 0 and loses to the centre
        const uint32_t inv = ~w[k];
        best0 = max_keys(best0, ((cnt[k] & 0x00ff00ffu) << 9) | ((same[k] & 0x00ff00ffu) << 8) | (inv & 0x00ff00ffu));
        best1 = max_keys(best1, (((cnt[k] >> 8) & 0x00ff00ffu) << 9) | (((same[k] >> 8) & 0x00ff00ffu) << 8) | ((inv >> 8) & 0x00ff00ffu));
    }
    return (~best0 & 0x00ff00ffu) | ((~best1 & 0x00ff00ffu) << 8);
}

}  // namespace
