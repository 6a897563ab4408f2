// Several device-to-device copies in ONE launch: up to XMEM_COPY_MAX_SEGMENTS (source, destination, byte count) triples travel BY VALUE
// in the kernel arguments, so the call needs no device-side table and may be made eagerly with addresses that change from call to
// call (the session's feature cache: one frame's key-encoder outputs <-> its cache entry, on the side stream).
//
// Byte-exact for every length (0 included) and every alignment.  Per segment the destination is brought to a 16-byte boundary with
// single-byte stores (< 16 of them), the body is written with one 16-byte store per chunk and the last < 16 bytes again byte by byte.
// The body's LOADS are as wide as the source allows once the destination is aligned: 16 bytes when source and destination are
// congruent mod 16 (every whole tensor, every fp32 slice whose offsets are multiples of 4 elements), else 4, 2 or 1 bytes gathered
// into the 16-byte store.  Plain vector loads and stores only.
//
// HBM-bound: the grid is sized to the chip (at most CPY_MAX_BLOCKS blocks of 256 threads = 8 per CU), not to the bytes; every segment
// is spread over the whole grid in turn (grid-stride), four independent 16-byte chunks per thread and iteration in flight.
#include "common.hpp"

#define CPY_THREADS 256
#define CPY_MAX_BLOCKS 2048
#define CPY_UNROLL 4

namespace {

struct CopySegments {
    const uint8_t* src[XMEM_COPY_MAX_SEGMENTS];
    uint8_t* dst[XMEM_COPY_MAX_SEGMENTS];
    size_t bytes[XMEM_COPY_MAX_SEGMENTS];
    int n;
};

// 16 bytes from `p`, which is aligned to sizeof(U), as 16 / sizeof(U) loads of U
template <typename U>
__device__ __forceinline__ uint4 cpy_load16(const uint8_t* p) {
    constexpr int N = 16 / sizeof(U);
    const U* q = reinterpret_cast<const U*>(p);
    U part[N];
#pragma unroll
    for (int i = 0; i < N; ++i) part[i] = q[i];
    uint4 v;
    __builtin_memcpy(&v, part, 16);
    return v;
}

// `chunks` 16-byte chunks from s (aligned to sizeof(U)) to d (aligned to 16), spread over `nt` threads
template <typename U>
__device__ __forceinline__ void cpy_body(const uint8_t* s, uint8_t* d, size_t chunks, size_t tid, size_t nt) {
    size_t i = tid;
    for (; i + (CPY_UNROLL - 1) * nt < chunks; i += CPY_UNROLL * nt) {
        uint4 v[CPY_UNROLL];
#pragma unroll
        for (int u = 0; u < CPY_UNROLL; ++u) v[u] = cpy_load16<U>(s + 16 * (i + u * nt));
#pragma unroll
        for (int u = 0; u < CPY_UNROLL; ++u) *reinterpret_cast<uint4*>(d + 16 * (i + u * nt)) = v[u];
    }
    for (; i < chunks; i += nt) *reinterpret_cast<uint4*>(d + 16 * i) = cpy_load16<U>(s + 16 * i);
}

__global__ __launch_bounds__(CPY_THREADS) void copy_segments_kernel(const CopySegments a) {
    const size_t tid = (size_t)blockIdx.x * CPY_THREADS + threadIdx.x, nt = (size_t)gridDim.x * CPY_THREADS;
    for (int s = 0; s < a.n; ++s) {
        const size_t n = a.bytes[s];
        if (n == 0) continue;
        const uint8_t* src = a.src[s];
        uint8_t* dst = a.dst[s];
        size_t head = (16 - ((uintptr_t)dst & 15)) & 15;          // bytes in front of the destination's first 16-byte boundary
        if (head > n) head = n;
        const size_t chunks = (n - head) >> 4;
        const size_t tail = head + (chunks << 4);                 // first byte behind the body; n - tail < 16
        if (tid < head) dst[tid] = src[tid];
        if (tid < n - tail) dst[tail + tid] = src[tail + tid];
        if (chunks == 0) continue;
        const unsigned mis = (unsigned)((uintptr_t)(src + head) & 15);
        if (mis == 0) cpy_body<uint4>(src + head, dst + head, chunks, tid, nt);
        else if ((mis & 3) == 0) cpy_body<uint32_t>(src + head, dst + head, chunks, tid, nt);
        else if ((mis & 1) == 0) cpy_body<uint16_t>(src + head, dst + head, chunks, tid, nt);
        else cpy_body<uint8_t>(src + head, dst + head, chunks, tid, nt);
    }
}

}  // namespace

extern "C" int xmem_copy_segments(const void* const* src, void* const* dst, const size_t* bytes, int n, void* stream) {
    if (n < 0 || (n > 0 && (!src || !dst || !bytes))) return XMEM_ERR_BAD_ARG;
    for (int i = 0; i < n; ++i) {
        if (bytes[i] == 0) continue;
        if (!src[i] || !dst[i]) return XMEM_ERR_BAD_ARG;
        const uintptr_t s = (uintptr_t)src[i], d = (uintptr_t)dst[i];
        if (s + bytes[i] < s || d + bytes[i] < d) return XMEM_ERR_BAD_ARG;
        if (s < d + bytes[i] && d < s + bytes[i]) return XMEM_ERR_BAD_ARG;      // overlapping ranges: the chunks are copied in no order
    }
    for (int first = 0; first < n; first += XMEM_COPY_MAX_SEGMENTS) {
        CopySegments a;
        a.n = n - first < XMEM_COPY_MAX_SEGMENTS ? n - first : XMEM_COPY_MAX_SEGMENTS;
        size_t chunks = 0;
        for (int i = 0; i < XMEM_COPY_MAX_SEGMENTS; ++i) {
            const bool used = i < a.n;
            a.src[i] = used ? (const uint8_t*)src[first + i] : nullptr;
            a.dst[i] = used ? (uint8_t*)dst[first + i] : nullptr;
            a.bytes[i] = used ? bytes[first + i] : 0;
            chunks += a.bytes[i] / 16 + (a.bytes[i] ? 1 : 0);
        }
        if (chunks == 0) continue;                                              // nothing but empty segments: no launch
        size_t blocks = (chunks + (size_t)CPY_THREADS * CPY_UNROLL - 1) / ((size_t)CPY_THREADS * CPY_UNROLL);
        if (blocks > CPY_MAX_BLOCKS) blocks = CPY_MAX_BLOCKS;
        hipLaunchKernelGGL(copy_segments_kernel, dim3((unsigned)blocks), dim3(CPY_THREADS), 0, (hipStream_t)stream, a);
        const int rc = xmem_check_launch();
        if (rc != XMEM_OK) return rc;
    }
    return XMEM_OK;
}
