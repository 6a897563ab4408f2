// Least-used eviction of a key/value store with SEVERAL object groups (kv_memory_store.py: remove_obsolete_features): every arena of
// the store is compacted by the SAME ascending index of surviving key elements, in one launch per XMEM_COMPACT_MAX_ARENAS arenas.
//
// The store's groups are suffix-aligned: an arena with n_a rows holds the LAST n_a of the store's N elements, its offset is
// off_a = N - n_a (0 for keys, shrinkage, selection, the fp16 filter rows and the usage counters; > 0 for the values of a group that
// appeared later).  With keep[0..m) the surviving elements, arena a keeps its rows keep[j] - off_a for the j with keep[j] >= off_a, in
// that order: j0_a, the first such j, is found by binary search and row keep[j] - off_a goes to destination row j - j0_a.  The
// (key, value) pairing the readout sees is the one it saw before.  m is read on the DEVICE (xmem_select_greater's count), the kept
// count m - j0_a of every arena is written to `kept`: the host learns all sizes in one transfer after the launch.
//
// The descriptors travel BY VALUE in the kernel arguments (as in copy_segments.hip): no device-side table.  The gather is NOT safe in
// place - a destination row may be another workgroup's unread source - so source and destination must not overlap (checked).
// Rows whose width is a multiple of 4 floats on 16-byte-aligned bases (64, 72, 512 floats) move as 16-byte vectors, everything else
// (width 1: shrinkage, use, life) float by float.  Plain vector loads and stores only.
//
// Every read index is checked against n_a before it forms an address and every destination row against n_a as well: an index that is
// not ascending, repeats or is out of range leaves rows unwritten and counts clamped, never an access outside an arena.
#include "common.hpp"

#define CMP_THREADS 256
#define CMP_MAX_BLOCKS 512          // per arena (blockIdx.y): 2 workgroups per CU
#define CMP_UNROLL 4

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));      // one 16-byte load / store

struct CompactArenas {
    const float* src[XMEM_COMPACT_MAX_ARENAS];
    float* dst[XMEM_COMPACT_MAX_ARENAS];
    int width[XMEM_COMPACT_MAX_ARENAS];     // floats per row
    int n[XMEM_COMPACT_MAX_ARENAS];         // rows
    int off[XMEM_COMPACT_MAX_ARENAS];       // first store element the arena holds
    int vec[XMEM_COMPACT_MAX_ARENAS];       // 1: rows move as 16-byte vectors
    const int32_t* keep; const int32_t* m_dev; int keep_cap;
    int32_t* kept;                          // [count]
    int count;
};

// entry i of a table in the kernel arguments, by selection: a dynamically indexed by-value array would be copied to a private array
template <typename T>
__device__ __forceinline__ T pick(const T (&table)[XMEM_COMPACT_MAX_ARENAS], int i) {
    T v = table[0];
#pragma unroll
    for (int k = 1; k < XMEM_COMPACT_MAX_ARENAS; ++k)
        if (i == k) v = table[k];
    return v;
}

// rows [j0, j0 + rows) of the index, `upr` units of V per row: unit u of the destination is unit u % upr of source row keep[j0 + u / upr] - off
template <typename V>
__device__ __forceinline__ void compact_rows(const V* __restrict__ src, V* __restrict__ dst, int upr, int n, int off,
                                             const int32_t* __restrict__ keep, int j0, int rows, size_t tid, size_t nt) {
    const size_t units = (size_t)rows * (size_t)upr;
    for (size_t u0 = tid; u0 < units; u0 += CMP_UNROLL * nt) {
        V v[CMP_UNROLL];
        bool ok[CMP_UNROLL];
#pragma unroll
        for (int i = 0; i < CMP_UNROLL; ++i) {
            const size_t u = u0 + (size_t)i * nt;
            ok[i] = false;
            if (u < units) {
                const size_t r = u / (size_t)upr;
                const size_t c = u - r * (size_t)upr;
                const long long s = (long long)keep[j0 + r] - (long long)off;       // j0 + r < m <= keep_cap
                if (s >= 0 && s < (long long)n) { v[i] = src[(size_t)s * (size_t)upr + c]; ok[i] = true; }
            }
        }
#pragma unroll
        for (int i = 0; i < CMP_UNROLL; ++i)
            if (ok[i]) dst[u0 + (size_t)i * nt] = v[i];                            // u < rows * upr <= n * upr
    }
}

__global__ __launch_bounds__(CMP_THREADS) void store_compact_kernel(const CompactArenas a) {
    const int ai = blockIdx.y;
    if (ai >= a.count) return;
    const int n = pick(a.n, ai), off = pick(a.off, ai), width = pick(a.width, ai);
    const float* src = pick(a.src, ai);
    float* dst = pick(a.dst, ai);
    int m = a.keep_cap > 0 ? *a.m_dev : 0;
    m = m < 0 ? 0 : (m > a.keep_cap ? a.keep_cap : m);
    // first j with keep[j] >= off (the index is ascending; any content terminates and stays inside [0, m])
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.keep[mid] < off) lo = mid + 1; else hi = mid;
    }
    const int j0 = lo;
    int rows = m - j0;
    if (rows > n) rows = n;                       // never with an ascending index of distinct elements below off + n
    if (blockIdx.x == 0 && threadIdx.x == 0) a.kept[ai] = rows;
    if (rows <= 0) return;
    const size_t tid = (size_t)blockIdx.x * CMP_THREADS + threadIdx.x, nt = (size_t)gridDim.x * CMP_THREADS;
    if (pick(a.vec, ai))
        compact_rows<u32x4>(reinterpret_cast<const u32x4*>(src), reinterpret_cast<u32x4*>(dst), width >> 2, n, off, a.keep, j0, rows, tid, nt);
    else
        compact_rows<float>(src, dst, width, n, off, a.keep, j0, rows, tid, nt);
}

}  // namespace

extern "C" int xmem_store_compact(const xmem_compact_arena* arenas, int n_arenas, const int32_t* keep, const int32_t* m_dev, int keep_cap,
                                  int32_t* kept, void* stream) {
    if (n_arenas < 0 || keep_cap < 0) return XMEM_ERR_BAD_ARG;
    if (n_arenas == 0) return XMEM_OK;
    if (!arenas || !m_dev || !kept || (keep_cap > 0 && !keep)) return XMEM_ERR_BAD_ARG;
    for (int i = 0; i < n_arenas; ++i) {
        const xmem_compact_arena& e = arenas[i];
        if (e.n < 0 || e.off < 0 || e.width < 1) return XMEM_ERR_BAD_ARG;
        if ((long long)e.off + e.n != (long long)keep_cap) return XMEM_ERR_BAD_ARG;      // suffix alignment: off_a = N - n_a
        if (e.n == 0) continue;
        if (!e.src || !e.dst) return XMEM_ERR_BAD_ARG;
        if (((uintptr_t)e.src & 3) || ((uintptr_t)e.dst & 3)) return XMEM_ERR_BAD_ARG;
    }
    // no destination may overlap a source (its own or another arena's: the rows are moved in no order) or another destination
    for (int i = 0; i < n_arenas; ++i) {
        if (arenas[i].n == 0) continue;
        const uintptr_t d = (uintptr_t)arenas[i].dst, db = (uintptr_t)arenas[i].n * (uintptr_t)arenas[i].width * sizeof(float);
        if (d + db < d) return XMEM_ERR_BAD_ARG;
        for (int j = 0; j < n_arenas; ++j) {
            if (arenas[j].n == 0) continue;
            const uintptr_t sb = (uintptr_t)arenas[j].n * (uintptr_t)arenas[j].width * sizeof(float);
            const uintptr_t s = (uintptr_t)arenas[j].src;
            if (s + sb < s) return XMEM_ERR_BAD_ARG;
            if (s < d + db && d < s + sb) return XMEM_ERR_BAD_ARG;
            const uintptr_t d2 = (uintptr_t)arenas[j].dst;
            if (j != i && d2 < d + db && d < d2 + sb) return XMEM_ERR_BAD_ARG;
        }
    }
    for (int first = 0; first < n_arenas; first += XMEM_COMPACT_MAX_ARENAS) {
        CompactArenas a;
        a.count = n_arenas - first < XMEM_COMPACT_MAX_ARENAS ? n_arenas - first : XMEM_COMPACT_MAX_ARENAS;
        a.keep = keep; a.m_dev = m_dev; a.keep_cap = keep_cap; a.kept = kept + first;
        size_t most = 1;                                   // units of the largest arena, all of its rows kept: sizes the grid
        for (int i = 0; i < XMEM_COMPACT_MAX_ARENAS; ++i) {
            const bool used = i < a.count;
            const xmem_compact_arena* e = used ? &arenas[first + i] : nullptr;
            a.src[i] = used ? e->src : nullptr;
            a.dst[i] = used ? e->dst : nullptr;
            a.width[i] = used ? e->width : 1;
            a.n[i] = used ? e->n : 0;
            a.off[i] = used ? e->off : 0;
            a.vec[i] = used && e->n > 0 && (e->width & 3) == 0 && (((uintptr_t)e->src | (uintptr_t)e->dst) & 15) == 0 ? 1 : 0;
            const size_t units = (size_t)a.n[i] * (size_t)(a.vec[i] ? a.width[i] >> 2 : a.width[i]);
            if (units > most) most = units;
        }
        size_t blocks = (most + (size_t)CMP_THREADS * CMP_UNROLL - 1) / ((size_t)CMP_THREADS * CMP_UNROLL);
        if (blocks > CMP_MAX_BLOCKS) blocks = CMP_MAX_BLOCKS;
        hipLaunchKernelGGL(store_compact_kernel, dim3((unsigned)blocks, (unsigned)a.count), dim3(CMP_THREADS), 0, (hipStream_t)stream, a);
        const int rc = xmem_check_launch();
        if (rc != XMEM_OK) return rc;
    }
    return XMEM_OK;
}
