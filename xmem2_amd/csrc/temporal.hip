// Sliding majority vote along the time axis of uint8 index masks (include/xmem_hip_temporal.h; xmem2_amd/temporal.py has the
// definition the bytes are held to).
//
//   work     a thread owns four neighbouring pixels (one dword of a frame) and walks TM_SEG output frames of them.  The window of
//            2 R + 1 dwords lives in registers: R is a template parameter, every index into the window is a compile-time constant
//            and a step moves the window down by one and loads one new frame, one step ahead of its first use.  blockIdx.y is the
//            time segment; a segment fills its own halo of R frames on either side from the INPUT, so a boundary does not show.
//   loads    frame f starts at frames + (f % ring) * HW, which is dword-aligned only when HW is a multiple of 4 or f % ring is:
//            alignment is decided per frame.  An aligned frame costs one dword load per thread, a misaligned one the two aligned
//            dwords round the four bytes and a funnel shift; the few groups whose dwords would leave the buffer, and the last,
//            partial group of a frame, read bytes.  Stores follow the same rule on `out`.
//   vote     four pixels at a time in packed bytes.  No histogram: the count of an entry's label is the number of window entries
//            equal to it, from the (2 R + 1) R pairwise byte comparisons - xor, then a zero-byte test that is exact for bytes of
//            0x80 and more.  A count is at most 15.  The winner is the maximum of the key `count << 9 | is the centre's label << 8 |
//            255 - label`, taken in 16-bit lanes, two pixels per dword.  Where every voting entry equals the centre - nearly all of
//            a mask - the thread skips the vote.
//   changed  the differing bytes of a step are summed over the wave and added by one lane, only where the wave changed any, into the
//            workgroup's TM_SEG counters in LDS; after the walk the workgroup adds its non-zero counters to `changed`.  (One global
//            add per wave and step put every wave of a noisy frame in a queue for one address.)
//
// No float, and no LDS but those 64 bytes: nothing is reused between threads.  The integer adds into the counters are the only
// atomics, and a sum of integers depends on no order: the same input gives the same bytes.
#include "common.hpp"
#include "vote_bytes.hpp"                   // load_bytes4, store_bytes4, eq_bytes, vote_group
#include "../../include/xmem_hip_temporal.h"

#define TM_MAX_HW 16384
#define TM_MAX_T 65535
#define TM_THREADS 256
#define TM_SEG XMEM_TEMPORAL_SEGMENT

namespace {

// pixels p .. p + 3 of the frame at `f` as one dword, pixel p in the low byte; pixels from hw on read as 0.  [lo, hi) is the buffer.
__device__ __forceinline__ uint32_t load_group(const uint8_t* f, int p, int hw, const uint8_t* lo, const uint8_t* hi) {
    return load_bytes4(f + p, min(4, hw - p), lo, hi);
}

__device__ __forceinline__ void store_group(uint8_t* q, uint32_t v, int p, int hw) { store_bytes4(q, v, min(4, hw - p)); }

template <int R>
__global__ __launch_bounds__(TM_THREADS) void temporal_mode_kernel(const uint8_t* __restrict__ frames, int ring, int hw, int T, int t0,
                                                                   int n, const uint8_t* __restrict__ flags, uint8_t* __restrict__ out,
                                                                   int32_t* __restrict__ changed) {
    constexpr int N = 2 * R + 1;
    // every lane stays to the end (the wave sums below): a group past the frame reads zeros and stores nothing
    const long long group = (long long)blockIdx.x * TM_THREADS + threadIdx.x;
    const int p = (int)(group * 4 < hw ? group * 4 : hw);
    const int s0 = t0 + (int)blockIdx.y * TM_SEG, s1 = min(s0 + TM_SEG, t0 + n);
    const uint8_t* const lo = frames;
    const uint8_t* const hi = frames + (size_t)ring * hw;
    uint32_t w[N], vote[N];
    __shared__ int block_changed[TM_SEG];
    if (threadIdx.x < TM_SEG) block_changed[threadIdx.x] = 0;
    __syncthreads();

    auto fetch = [&](int f, uint32_t& v, uint32_t& votes) {
        v = 0;
        votes = 0;
        if (f >= 0 && f < T) {
            v = load_group(frames + (size_t)(f % ring) * hw, p, hw, lo, hi);
            votes = (flags[f] & XMEM_TEMPORAL_PRESENT) ? 0x01010101u : 0u;
        }
    };

#pragma unroll
    for (int k = 1; k < N; ++k) fetch(s0 - R + k - 1, w[k], vote[k]);
    uint32_t next, next_votes;
    fetch(s0 + R, next, next_votes);
    for (int t = s0; t < s1; ++t) {
#pragma unroll
        for (int k = 0; k + 1 < N; ++k) {
            w[k] = w[k + 1];
            vote[k] = vote[k + 1];
        }
        w[N - 1] = next;
        vote[N - 1] = next_votes;
        if (t + 1 < s1) fetch(t + 1 + R, next, next_votes);
        const uint32_t c = w[R];
        uint32_t o = c;
        if (vote[R] && !(flags[t] & XMEM_TEMPORAL_LOCKED)) {
            uint32_t differs = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) differs |= (w[k] ^ c) & (vote[k] * 0xffu);
            if (differs) o = vote_group<R>(w, vote);
        }
        store_group(out + (size_t)(t - t0) * hw + p, o, p, hw);
        int d = __popc(~(eq_bytes(o, c)) & 0x01010101u);
        if (__any(d)) {
            d = wave_sum_i(d);
            if ((threadIdx.x & (XMEM_WAVE - 1)) == 0) atomicAdd(&block_changed[t - s0], d);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < s1 - s0 && block_changed[threadIdx.x]) atomicAdd(changed + (s0 - t0) + threadIdx.x, block_changed[threadIdx.x]);
}

template <int R>
void launch(const uint8_t* frames, int ring, int hw, int T, int t0, int n, const uint8_t* flags, uint8_t* out, int32_t* changed,
            hipStream_t s) {
    const dim3 grid((unsigned)cdiv(cdiv(hw, 4), TM_THREADS), (unsigned)cdiv(n, TM_SEG));
    hipLaunchKernelGGL(temporal_mode_kernel<R>, grid, dim3(TM_THREADS), 0, s, frames, ring, hw, T, t0, n, flags, out, changed);
}

}  // namespace

extern "C" int xmem_temporal_mode(const uint8_t* frames, int ring, int H, int W, int T, int t0, int n, int radius, const uint8_t* flags,
                                  uint8_t* out, int32_t* changed, void* stream) {
    if (!frames || !flags || !out || !changed || ((uintptr_t)changed & 3)) return XMEM_ERR_BAD_ARG;
    if (radius < 1 || radius > XMEM_TEMPORAL_MAX_R || ring < 1) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > TM_MAX_HW || W > TM_MAX_HW || T < 1 || T > TM_MAX_T) return XMEM_ERR_UNSUPPORTED;
    if (n < 1 || t0 < 0 || t0 > T - n) return XMEM_ERR_BAD_ARG;
    const int first = t0 - radius > 0 ? t0 - radius : 0, last = t0 + n - 1 + radius < T - 1 ? t0 + n - 1 + radius : T - 1;
    if (ring < last - first + 1) return XMEM_ERR_BAD_ARG;                // two frames the call reads would share a slot
    const size_t hw = (size_t)H * (size_t)W;
    const uintptr_t a = (uintptr_t)frames, b = (uintptr_t)out;
    if (a < b + (size_t)n * hw && b < a + (size_t)ring * hw) return XMEM_ERR_BAD_ARG;
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(changed, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    switch (radius) {
#define TM_CASE(R) case R: launch<R>(frames, ring, (int)hw, T, t0, n, flags, out, changed, s); break;
        TM_CASE(1) TM_CASE(2) TM_CASE(3) TM_CASE(4) TM_CASE(5) TM_CASE(6) TM_CASE(7)
#undef TM_CASE
    }
    return xmem_check_launch();
}
