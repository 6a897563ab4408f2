// The index mask of a frame's class scores with a margin plane and a per-label record (include/xmem_hip_confidence.h;
// xmem2_amd/confidence.py has the definition the bytes are held to).  One kernel, templated on the score type: float32 probabilities,
// or the uint16 sums of the test-time ensemble.
//
//   work     a thread owns four pixels - 16 bytes of a float channel, 8 of a uint16 one - and walks the C channels once, keeping
//            the largest and the second largest score and their indices per pixel.  Both follow the `v > best` rule of
//            argmax_u8_kernel: a newcomer that beats the best pushes it down to second (it was the first maximal one so far), one that
//            only beats the second replaces it; on ties the earlier index stays, so `second` is the first maximal index of the rest.
//            The per-pixel values live in arrays indexed by unrolled loops only: nothing a lane holds is indexed by a label.
//   loads    a channel starts at prob + c P, 16-byte aligned only when P is a multiple of the group and prob is aligned: decided once
//            per call.  Then one load per channel and group; else element loads with a bound check (the ragged end included).
//            Four channels are loaded before the first is compared: a wave waits for memory once per four.
//   counters [C][4] 32-bit counters per workgroup in LDS.  A workgroup walks `iters` consecutive tiles - at most 2^20 pixels, so
//            255 times that fits 32 bits.  Nearly every wave of a mask lies inside one label: then area, margin sum and low count are
//            summed over the wave and added by one lane.  Otherwise a thread adds per run of equal labels among its pixels.  A
//            contested pixel (q < tau) adds to its second label's counter on its own: such pixels are the few on the borders.
//   flush    after the walk the workgroup adds its non-zero counters to the record with 64-bit integer atomics, consecutive lanes to
//            consecutive words.  Integer sums depend on no order: the same input gives the same bytes.
#include "common.hpp"
#include "../../include/xmem_hip_confidence.h"

#define CF_MAX_HW 16384
#define CF_THREADS 1024                  // sixteen waves share one set of counters: a quarter of the 64-bit adds of four-wave workgroups
#define CF_TARGET_BLOCKS 256             // a longer frame gives every workgroup more tiles, not the grid more workgroups
#define CF_REC XMEM_CONFIDENCE_RECORD

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Score;
template <> struct Score<float> {
    typedef float V;
    static constexpr int PX = 4;
    static constexpr int CHUNK = 4;      // channels whose loads are in flight together
    __device__ static __forceinline__ float lowest() { return -INFINITY; }
    __device__ static __forceinline__ float unpack(const u32x4& raw, int k) { return __uint_as_float(raw[k]); }
    __device__ static __forceinline__ uint32_t pack(float v, int) { return __float_as_uint(v); }
    // q of the margin m: the product with a power of two is exact, so no contraction or rounding mode moves it
    __device__ static __forceinline__ int quantise(float m, int) {
        if (!(m > 0.0f)) return 0;
        const float s = m * 256.0f;
        return s >= 255.0f ? 255 : (int)s;
    }
};
template <> struct Score<uint16_t> {
    typedef int V;
    static constexpr int PX = 4;         // 8-byte loads: eight pixels a thread do not fit the registers of sixteen waves
    static constexpr int CHUNK = 4;
    __device__ static __forceinline__ int lowest() { return -1; }
    __device__ static __forceinline__ int unpack(const u32x4& raw, int k) { return (int)((raw[k >> 1] >> (16 * (k & 1))) & 0xffffu); }
    __device__ static __forceinline__ uint32_t pack(uint16_t v, int k) { return (uint32_t)v << (16 * (k & 1)); }
    __device__ static __forceinline__ int quantise(int m, int passes) {
        const int q = m > 0 ? m / passes : 0;
        return q > 255 ? 255 : q;
    }
};

// the thread's four pixels of one channel: one load where the call found every channel aligned, else its `nv` elements one by one
template <typename T>
__device__ __forceinline__ u32x4 load_group(const T* ch, int nv, int vec) {
    constexpr int PX = Score<T>::PX;
    if (vec) {
        if constexpr (sizeof(T) * PX == 16) return *(const u32x4*)ch;
        const uint2 two = *(const uint2*)ch;
        return u32x4{two.x, two.y, 0, 0};
    }
    u32x4 raw = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < PX; ++k)
        if (k < nv) raw[k * (int)sizeof(T) / 4] |= Score<T>::pack(ch[k], k);
    return raw;
}

// a run of pixels of one label into the workgroup's counters; label < 0: no run
__device__ __forceinline__ void add_run(uint32_t* counters, int label, int area, int margin, int low) {
    if (label < 0) return;
    atomicAdd(&counters[label * CF_REC + XMEM_CONFIDENCE_AREA], (uint32_t)area);
    if (margin) atomicAdd(&counters[label * CF_REC + XMEM_CONFIDENCE_MARGIN_SUM], (uint32_t)margin);
    if (low) atomicAdd(&counters[label * CF_REC + XMEM_CONFIDENCE_LOW], (uint32_t)low);
}

template <typename T>
__global__ __launch_bounds__(CF_THREADS) void confidence_kernel(const T* __restrict__ prob, int passes, int C, long long P, int tau,
                                                                int iters, int vec, uint8_t* __restrict__ mask,
                                                                uint8_t* __restrict__ plane, unsigned long long* __restrict__ record) {
    typedef typename Score<T>::V V;
    constexpr int PX = Score<T>::PX, CF_CHUNK = Score<T>::CHUNK;
    __shared__ uint32_t counters[XMEM_CONFIDENCE_MAX_C * CF_REC];
    for (int i = threadIdx.x; i < C * CF_REC; i += CF_THREADS) counters[i] = 0;
    __syncthreads();

    // every lane stays to the end (the wave sums below): a group past the frame owns no pixel
    for (int it = 0; it < iters; ++it) {
        const long long tile = (long long)blockIdx.x * iters + it;
        const long long p0 = (tile * CF_THREADS + threadIdx.x) * PX;
        const int nv = p0 >= P ? 0 : (P - p0 < PX ? (int)(P - p0) : PX);     // pixels of this thread
        V best[PX], sec[PX];
        int top[PX], second[PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            best[k] = sec[k] = Score<T>::lowest();
            top[k] = second[k] = 0;
        }
        // CF_CHUNK channels at a time, their loads issued before the first is compared: a wave's latency is paid once per chunk
        for (int c0 = 0; c0 < C; c0 += CF_CHUNK) {
            // a channel past the last reads the last again and a thread without pixels the frame's first group: every address is
            // inside the scores, no load hangs on a branch, and what such a load brings is never looked at
            u32x4 raw[CF_CHUNK];
#pragma unroll
            for (int u = 0; u < CF_CHUNK; ++u) {
                const int c = c0 + u < C ? c0 + u : C - 1;
                raw[u] = load_group<T>(prob + (size_t)c * (size_t)P + (nv ? p0 : 0), nv, vec);
            }
#pragma unroll
            for (int u = 0; u < CF_CHUNK; ++u) {
                const int c = c0 + u;
                if (c >= C) break;                                       // uniform
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const V v = Score<T>::unpack(raw[u], k);
                    if (c == 0) {
                        best[k] = v;
                    } else if (v > best[k]) {
                        sec[k] = best[k];
                        second[k] = top[k];
                        best[k] = v;
                        top[k] = c;
                    } else if (v > sec[k]) {
                        sec[k] = v;
                        second[k] = c;
                    }
                }
            }
        }
        int q[PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) q[k] = Score<T>::quantise(C > 1 ? best[k] - sec[k] : best[k], passes);

        // ---- mask and plane ------------------------------------------------------------------------------------------------------
        if (mask) {
            uint8_t* o = mask + p0;
            if (nv == PX && ((uintptr_t)o & 3) == 0) {
#pragma unroll
                for (int k = 0; k < PX; k += 4)
                    *(uint32_t*)(o + k) = (uint32_t)top[k] | ((uint32_t)top[k + 1] << 8) | ((uint32_t)top[k + 2] << 16) | ((uint32_t)top[k + 3] << 24);
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (k < nv) o[k] = (uint8_t)top[k];
            }
        }
        if (plane) {
            uint8_t* o = plane + p0;
            if (nv == PX && ((uintptr_t)o & 3) == 0) {
#pragma unroll
                for (int k = 0; k < PX; k += 4)
                    *(uint32_t*)(o + k) = (uint32_t)(255 - q[k]) | ((uint32_t)(255 - q[k + 1]) << 8) | ((uint32_t)(255 - q[k + 2]) << 16) |
                                          ((uint32_t)(255 - q[k + 3]) << 24);
            } else {
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    if (k < nv) o[k] = (uint8_t)(255 - q[k]);
            }
        }

        // ---- counters ------------------------------------------------------------------------------------------------------------
        // pixels rise with the lane: when lane 0 of a wave owns none, no lane of it does
        const int wave_label = __builtin_amdgcn_readfirstlane(nv ? top[0] : -1);
        bool mine_agree = true;
        int sum_q = 0, n_low = 0;
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            if (k < nv) {
                mine_agree = mine_agree && top[k] == wave_label;
                sum_q += q[k];
                n_low += q[k] < tau;
                if (C > 1 && q[k] < tau) atomicAdd(&counters[second[k] * CF_REC + XMEM_CONFIDENCE_CONTESTED], 1u);
            }
        }
        if (wave_label >= 0) {
            if (__all(mine_agree)) {
                const int area = wave_sum_i(nv), margin = wave_sum_i(sum_q), low = wave_sum_i(n_low);
                if ((threadIdx.x & (XMEM_WAVE - 1)) == 0) add_run(counters, wave_label, area, margin, low);
            } else {
                // per run of equal labels among the thread's pixels
                int run_label = -1, run_area = 0, run_margin = 0, run_low = 0;
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const int label = k < nv ? top[k] : -1;
                    if (label != run_label) {
                        add_run(counters, run_label, run_area, run_margin, run_low);
                        run_label = label;
                        run_area = run_margin = run_low = 0;
                    }
                    if (label >= 0) {
                        run_area += 1;
                        run_margin += q[k];
                        run_low += q[k] < tau;
                    }
                }
                add_run(counters, run_label, run_area, run_margin, run_low);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * CF_REC; i += CF_THREADS)
        if (counters[i]) atomicAdd(record + i, (unsigned long long)counters[i]);
}

template <typename T>
int confidence(const T* prob, int passes, int C, int H, int W, int tau, uint8_t* mask, uint8_t* plane, uint64_t* record, void* stream) {
    if (!prob || !record || ((uintptr_t)record & 7)) return XMEM_ERR_BAD_ARG;
    if (C < 1 || C > XMEM_CONFIDENCE_MAX_C || tau < 0 || tau > XMEM_CONFIDENCE_MAX_TAU) return XMEM_ERR_BAD_ARG;
    if (passes < 1 || passes > XMEM_CONFIDENCE_MAX_PASSES) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > CF_MAX_HW || W > CF_MAX_HW) return XMEM_ERR_UNSUPPORTED;
    constexpr int PX = Score<T>::PX;
    const long long P = (long long)H * W;
    const long long per_tile = (long long)CF_THREADS * PX, tiles = (P + per_tile - 1) / per_tile;
    const int iters = (int)((tiles + CF_TARGET_BLOCKS - 1) / CF_TARGET_BLOCKS);      // at most 2^28 / 2^12 / 2^8 = 256 tiles of 2^12 pixels
    const unsigned blocks = (unsigned)((tiles + iters - 1) / iters);
    const int vec = P % PX == 0 && ((uintptr_t)prob & 15) == 0;
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(record, 0, (size_t)C * CF_REC * sizeof(uint64_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    hipLaunchKernelGGL(confidence_kernel<T>, dim3(blocks), dim3(CF_THREADS), 0, s, prob, passes, C, P, tau, iters, vec, mask, plane,
                       (unsigned long long*)record);
    return xmem_check_launch();
}

}  // namespace

extern "C" int xmem_confidence_f32(const float* prob, int C, int H, int W, int tau, uint8_t* mask, uint8_t* plane, uint64_t* record,
                                   void* stream) {
    return confidence<float>(prob, 1, C, H, W, tau, mask, plane, record, stream);
}

extern "C" int xmem_confidence_u16(const uint16_t* acc, int passes, int C, int H, int W, int tau, uint8_t* mask, uint8_t* plane,
                                   uint64_t* record, void* stream) {
    return confidence<uint16_t>(acc, passes, C, H, W, tau, mask, plane, record, stream);
}
