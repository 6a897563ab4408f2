// Run-length track export (include/xmem_hip.h, xmem_rle_encode): the run boundaries ("events"), areas and boxes of uint8 label maps
// in the COCO order j = x * H + y, for the labels 1..K.  The map is row-major and the order column-major, so a workgroup owns a strip
// of RLE_TILE whole columns and walks it in tiles of RLE_TILE rows: the tile is read row-major (16-byte loads where the row pitch
// allows them), turned through LDS (rows padded to 17 words: lane r reads word 17 r + c, 64 different banks), and a wave then looks at
// one column of the tile at a time - lane r holds pixel (ty0 + r, x), its predecessor in the order is lane r - 1's pixel, for lane 0
// the pixel above the tile and at the top of a column the bottom pixel of the column before (0 at j = 0).
//
// A pixel whose predecessor differs carries up to two events: the end of the predecessor's label and the start of its own.  Per
// label the wave compacts them with a ballot (rank = popcount of the lanes below), so events leave a wave in ascending order.  A
// column always belongs to the same wave, which meets its tiles from the top down; the running position of (frame, label, column)
// is a plain read-modify-write of that wave's lane 0 on the workspace.  Three launches:
//   count  the walk, adding the number of events to workspace [N][K][W]; areas and boxes per workgroup in LDS (integer atomics),
//          then one integer atomic per label and workgroup on `meta`;
//   scan   one workgroup per frame: exclusive scan of the frame's [K][W] counts in that order - the start of every (label, column)
//          in the frame's packed event list; the per-label totals and the finished boxes go to `meta`;
//   emit   the same walk, writing each event at its scanned position (below `capacity`).
// No workgroup waits for another, no float arithmetic, and no output position depends on the order in which atomics arrive.
// Further down: the compressed COCO strings of a record and back (xmem_rle_compress / xmem_rle_decompress).
#include "common.hpp"

#define RLE_MAX_HW 16384
#define RLE_TILE 64                // rows and columns of a tile
#define RLE_THREADS 256            // 4 waves; wave w owns the columns 16 w .. 16 w + 15 of the strip
#define RLE_STRIDE 17              // words per LDS row: 16 of pixels + 1 of padding
#define RLE_SCAN_THREADS 1024

namespace {

template <bool EMIT>
__global__ __launch_bounds__(RLE_THREADS) void rle_walk_kernel(const uint8_t* __restrict__ masks, int H, int W, int K, int vec_ok,
                                                               int* ofs, int* __restrict__ meta, uint32_t* __restrict__ events,
                                                               int capacity) {
    __shared__ uint32_t s_tile[RLE_TILE][RLE_STRIDE];
    __shared__ uint32_t s_halo[RLE_TILE / 4];
    __shared__ int s_stat[5][256];          // per label: area, max(16384 - x), max(16384 - y), max(x + 1), max(y + 1); 0 = none
    const int n = blockIdx.y, x0 = blockIdx.x * RLE_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* m = masks + (size_t)n * H * W;
    if (!EMIT)
        for (int i = tid; i < 5 * 256; i += RLE_THREADS) (&s_stat[0][0])[i] = 0;      // visible after the first tile's barrier

    for (int ty0 = 0; ty0 < H; ty0 += RLE_TILE) {
        if (vec_ok) {                                    // W % 16 == 0 and a 16-byte aligned map: a chunk is inside the row or outside it
            const int r = tid >> 2, q = tid & 3;
            const int y = ty0 + r, x = x0 + 16 * q;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (y < H && x < W) v = *reinterpret_cast<const uint4*>(m + (size_t)y * W + x);
            s_tile[r][4 * q + 0] = v.x;
            s_tile[r][4 * q + 1] = v.y;
            s_tile[r][4 * q + 2] = v.z;
            s_tile[r][4 * q + 3] = v.w;
        } else {                                         // any pitch: a wave reads 64 consecutive bytes of a row
            const int x = x0 + lane;
#pragma unroll 4
            for (int i = 0; i < RLE_TILE / 4; ++i) {
                const int r = wave + 4 * i, y = ty0 + r;
                uint8_t b = 0;
                if (y < H && x < W) b = m[(size_t)y * W + x];
                reinterpret_cast<uint8_t*>(&s_tile[r][0])[lane] = b;
            }
        }
        if (tid < RLE_TILE) {                            // the predecessors of the tile's first row
            const int x = x0 + tid;
            uint8_t b = 0;
            if (x < W) {
                if (ty0 > 0) b = m[(size_t)(ty0 - 1) * W + x];
                else if (x > 0) b = m[(size_t)(H - 1) * W + x - 1];
            }
            reinterpret_cast<uint8_t*>(&s_halo[0])[tid] = b;
        }
        __syncthreads();

        const int y = ty0 + lane;
        const bool active = y < H;
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int g = 0; g < 4; ++g) {
            const int wq = wave * 4 + g;                 // word of the row: columns 4 wq .. 4 wq + 3
            const uint32_t word = s_tile[lane][wq];
            const uint32_t hword = s_halo[wq];
            for (int b = 0; b < 4; ++b) {
                const int x = x0 + wq * 4 + b;
                if (x >= W) break;                       // uniform over the wave
                const int cur = (int)((word >> (8 * b)) & 255u);
                int prev = __shfl_up(cur, 1, 64);
                if (lane == 0) prev = (int)((hword >> (8 * b)) & 255u);
                const bool cv = active && cur >= 1 && cur <= K;
                if (!EMIT) {
                    unsigned long long pend = __ballot(cv);
                    while (pend) {                       // one turn per label present in this column segment
                        const int L = __shfl(cur, __ffsll((long long)pend) - 1, 64);
                        const unsigned long long mm = __ballot(cv && cur == L);
                        if (lane == 0) {
                            const int ya = ty0 + __ffsll((long long)mm) - 1, yb = ty0 + 63 - __clzll((long long)mm);
                            atomicAdd(&s_stat[0][L], __popcll(mm));
                            atomicMax(&s_stat[1][L], RLE_MAX_HW - x);
                            atomicMax(&s_stat[2][L], RLE_MAX_HW - ya);
                            atomicMax(&s_stat[3][L], x + 1);
                            atomicMax(&s_stat[4][L], yb + 1);
                        }
                        pend &= ~mm;
                    }
                }
                const bool tr = active && prev != cur;
                const bool pv = tr && prev >= 1 && prev <= K, cvt = tr && cv;
                unsigned long long pa = __ballot(pv), pb = __ballot(cvt);
                while (pa | pb) {                        // one turn per label that ends or starts in this column segment
                    const int L = pa ? __shfl(prev, __ffsll((long long)pa) - 1, 64) : __shfl(cur, __ffsll((long long)pb) - 1, 64);
                    const bool mine = (pv && prev == L) || (cvt && cur == L);
                    const unsigned long long mm = __ballot(mine);
                    int* slot = ofs + ((size_t)n * K + (L - 1)) * W + x;
                    int at = 0;
                    if (lane == 0) {                     // this wave alone touches (n, L, x), tile after tile
                        at = *slot;
                        *slot = at + __popcll(mm);
                    }
                    if (EMIT) {
                        at = __shfl(at, 0, 64);
                        const int idx = at + __popcll(mm & below);
                        if (mine && idx < capacity) events[(size_t)n * capacity + idx] = (uint32_t)x * (uint32_t)H + (uint32_t)y;
                    }
                    pa &= ~__ballot(pv && prev == L);
                    pb &= ~__ballot(cvt && cur == L);
                }
            }
        }
        __syncthreads();                                 // the tile is rewritten
    }

    if (!EMIT)
        for (int k = 1 + tid; k <= K; k += RLE_THREADS)
            if (s_stat[0][k] > 0) {
                int* mt = meta + ((size_t)n * K + (k - 1)) * XMEM_RLE_META;
                atomicAdd(mt + 1, s_stat[0][k]);
                atomicMax(mt + 2, s_stat[1][k]);
                atomicMax(mt + 3, s_stat[2][k]);
                atomicMax(mt + 4, s_stat[3][k]);
                atomicMax(mt + 5, s_stat[4][k]);
            }
}

// Exclusive scan of a frame's counts [K][W], label-major: ofs becomes the position of the first event of (label, column) in the frame's
// packed list.  meta: the per-label totals, and the boxes turned from the maxima the count pass collected into x0, y0, x1, y1.
__global__ __launch_bounds__(RLE_SCAN_THREADS) void rle_scan_kernel(int* __restrict__ ofs, int* __restrict__ meta, int K, int W) {
    __shared__ int s_wave[RLE_SCAN_THREADS / XMEM_WAVE];
    __shared__ int s_start[256];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* c = ofs + (size_t)n * K * W;
    const int M = K * W;
    int carry = 0;
    for (int base = 0; base < M; base += RLE_SCAN_THREADS) {
        const int i = base + tid;
        const int v = i < M ? c[i] : 0;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < RLE_SCAN_THREADS / XMEM_WAVE; ++w) {
            const int t = s_wave[w];
            if (w < wave) before += t;
            total += t;
        }
        const int excl = carry + before + incl - v;
        if (i < M) {
            c[i] = excl;
            if (i % W == 0) s_start[i / W] = excl;
        }
        carry += total;
        __syncthreads();                                 // s_wave is rewritten; s_start is read below
    }
    if (tid < K) {
        int* mt = meta + ((size_t)n * K + tid) * XMEM_RLE_META;
        mt[0] = (tid + 1 < K ? s_start[tid + 1] : carry) - s_start[tid];
        if (mt[1] > 0) {
            mt[2] = RLE_MAX_HW - mt[2];
            mt[3] = RLE_MAX_HW - mt[3];
            mt[4] -= 1;
            mt[5] -= 1;
        } else {
            mt[2] = 0; mt[3] = 0; mt[4] = -1; mt[5] = -1;
        }
    }
}

// The inverse of the record (include/xmem_hip.h, xmem_rle_decode): output-driven.  A lane owns RLE_DEC_COLS adjacent columns over
// RLE_DEC_ROWS rows, holds their bytes in registers and stores nothing else, so no event value can steer a store.  For every label row
// with events it finds, per column, the number of events at or below the chunk's first j by binary search, then walks a cursor down
// the column; a pixel inside an odd number of events takes the row's value, later rows overwrite earlier ones.  A wave writes 256
// consecutive bytes of a mask row (dwords when every row starts on a multiple of 4).  The running start of a row in the packed list
// is checked against `capacity` BEFORE any of its events is read; a frame that fails is written all zero.  No atomics, no workspace.
#define RLE_DEC_COLS 4
#define RLE_DEC_ROWS 16
#define RLE_DEC_WAVES 4            // wave w of a workgroup owns the rows 16 w .. 16 w + 15 of its 64

__global__ __launch_bounds__(RLE_DEC_WAVES * XMEM_WAVE) void rle_decode_kernel(const int* __restrict__ meta,
                                                                                const uint32_t* __restrict__ events, int H, int W, int K,
                                                                                int capacity, const uint8_t* __restrict__ values,
                                                                                int dword_ok, uint8_t* __restrict__ masks,
                                                                                int* __restrict__ status) {
    const int n = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = (blockIdx.x * XMEM_WAVE + lane) * RLE_DEC_COLS;
    const int y0 = (blockIdx.y * RLE_DEC_WAVES + wave) * RLE_DEC_ROWS;
    const int* mt = meta + (size_t)n * K * XMEM_RLE_META;
    const uint32_t* ev_frame = events + (size_t)n * capacity;
    uint32_t px[RLE_DEC_ROWS];
#pragma unroll
    for (int r = 0; r < RLE_DEC_ROWS; ++r) px[r] = 0u;

    int base = 0, bad = 0;
    for (int k = 0; k < K; ++k) {                        // uniform over the grid: every thread of a frame reaches the same verdict
        const int cnt = mt[(size_t)k * XMEM_RLE_META];
        if (cnt == 0) continue;
        if (cnt < 0 || cnt > capacity - base) { bad = 1; break; }
        const uint32_t* ev = ev_frame + base;            // ev[0 .. cnt) lies below `capacity`
        base += cnt;
        if (x0 >= W || y0 >= H) continue;
        const uint32_t val = values ? (uint32_t)values[k] : (uint32_t)(k + 1);
#pragma unroll
        for (int c = 0; c < RLE_DEC_COLS; ++c) {
            const int x = x0 + c;
            if (x >= W) break;
            const uint32_t j0 = (uint32_t)x * (uint32_t)H + (uint32_t)y0;
            int lo = 0, hi = cnt;                        // pos: the number of events <= j0
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ev[mid] <= j0) lo = mid + 1; else hi = mid;
            }
            int pos = lo;
            uint32_t next = pos < cnt ? ev[pos] : 0xffffffffu;
#pragma unroll
            for (int r = 0; r < RLE_DEC_ROWS; ++r) {
                const uint32_t j = j0 + (uint32_t)r;
                while (next <= j) {                      // at most cnt - pos turns: next becomes 0xffffffff > j at the end of the list
                    ++pos;
                    next = pos < cnt ? ev[pos] : 0xffffffffu;
                }
                if (pos & 1) px[r] = (px[r] & ~(255u << (8 * c))) | (val << (8 * c));
            }
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) status[n] = bad;
    if (x0 >= W || y0 >= H) return;
    uint8_t* out = masks + (size_t)n * H * W;
#pragma unroll
    for (int r = 0; r < RLE_DEC_ROWS; ++r) {
        const int y = y0 + r;
        if (y >= H) break;
        const uint32_t v = bad ? 0u : px[r];
        uint8_t* row = out + (size_t)y * W + x0;
        if (dword_ok) {                                  // W % 4 == 0: the lane's 4 columns are all inside the row
            *reinterpret_cast<uint32_t*>(row) = v;
        } else {
#pragma unroll
            for (int c = 0; c < RLE_DEC_COLS; ++c)
                if (x0 + c < W) row[c] = (uint8_t)(v >> (8 * c));
        }
    }
}

inline bool rle_args_ok(int N, int W, int K) { return N > 0 && W > 0 && K >= 1 && K <= 254; }
inline bool rle_size_ok(int N, int H, int W) { return H <= RLE_MAX_HW && W <= RLE_MAX_HW && N <= 65535; }

}  // namespace

extern "C" size_t xmem_rle_workspace_bytes(int N, int W, int K) {
    if (!rle_args_ok(N, W, K) || !rle_size_ok(N, 1, W)) return 0;
    return (size_t)N * K * W * sizeof(int32_t);
}

extern "C" int xmem_rle_encode(const uint8_t* masks, int N, int H, int W, int K, int capacity, int32_t* meta, uint32_t* events,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (!masks || !meta || !events || !workspace || H <= 0 || capacity < 1 || !rle_args_ok(N, W, K)) return XMEM_ERR_BAD_ARG;
    if (!rle_size_ok(N, H, W)) return XMEM_ERR_UNSUPPORTED;
    if (workspace_bytes < xmem_rle_workspace_bytes(N, W, K) || ((uintptr_t)workspace & 3)) return XMEM_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    int* ofs = (int*)workspace;
    if (hipMemsetAsync(meta, 0, (size_t)N * K * XMEM_RLE_META * sizeof(int32_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    if (hipMemsetAsync(ofs, 0, (size_t)N * K * W * sizeof(int32_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    // 16-byte loads need every row of every frame to start on a multiple of 16
    const int vec_ok = (W % 16 == 0) && (((uintptr_t)masks & 15) == 0);
    const dim3 grid(cdiv(W, RLE_TILE), N), block(RLE_THREADS);
    hipLaunchKernelGGL(rle_walk_kernel<false>, grid, block, 0, s, masks, H, W, K, vec_ok, ofs, (int*)meta, events, capacity);
    int rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(rle_scan_kernel, dim3(N), dim3(RLE_SCAN_THREADS), 0, s, ofs, (int*)meta, K, W);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(rle_walk_kernel<true>, grid, block, 0, s, masks, H, W, K, vec_ok, ofs, (int*)meta, events, capacity);
    return xmem_check_launch();
}

extern "C" int xmem_rle_decode(const int32_t* meta, const uint32_t* events, int N, int H, int W, int K, int capacity,
                               const uint8_t* values, uint8_t* masks, int32_t* status, void* stream) {
    if (!meta || !events || !masks || !status) return XMEM_ERR_BAD_ARG;
    if (H <= 0 || capacity < 1 || !rle_args_ok(N, W, K) || !rle_size_ok(N, H, W)) return XMEM_ERR_UNSUPPORTED;
    // dword stores need every row of every frame to start on a multiple of 4
    const int dword_ok = (W % 4 == 0) && (((uintptr_t)masks & 3) == 0);
    const dim3 grid(cdiv(W, XMEM_WAVE * RLE_DEC_COLS), cdiv(H, RLE_DEC_WAVES * RLE_DEC_ROWS), N), block(RLE_DEC_WAVES * XMEM_WAVE);
    hipLaunchKernelGGL(rle_decode_kernel, grid, block, 0, (hipStream_t)stream, (const int*)meta, events, H, W, K, capacity, values,
                       dword_ok, masks, (int*)status);
    return xmem_check_launch();
}

// ---- compressed COCO strings (include/xmem_hip.h, xmem_rle_compress / xmem_rle_decompress) --------------------------------------
// The string of a label is a function of its counts c[i] = e[i] - e[i - 1] (e[-1] = 0, e[E] = H * W): the value x[i] = c[i] for
// i <= 2 and c[i] - c[i - 2] after that, written as little-endian groups of 5 bits with a continuation bit (0x20), characters offset
// by 48.  Compress: one thread owns one count - four neighbouring events, a length 1..6 - and the same three steps as the encoder:
//   lengths  the length of every value into the workspace [N][capacity + K], the frame's values label-major;
//   scan     one workgroup per frame: exclusive scan - the position of every value's first character; per-label lengths to str_len;
//   emit     the value again, its characters at the scanned position (below `char_capacity`).
// Decompress: one workgroup per string walks it in chunks of RLE_STR_THREADS characters.  A thread whose character ends a value (bit
// 0x20 clear) assembles it from at most 5 characters before it; the value's index is the rank of its last character (a scan), the
// counts are two stride-2 running sums of the values, the events the running sum of the counts - three block scans per chunk with the
// sums carried from chunk to chunk.  Again three steps:
//   check    the walk without stores: malformed / not a plane / the number of values, per string;
//   scan     one workgroup per frame: the rows' starts in the frame's packed event list, `meta`, capacity overflow;
//   expand   the walk again for the good rows, event i at start + i (below `capacity`).
// The index of a store is always a rank or a scanned length, never a decoded value.  No workgroup waits for another, no atomics on
// global memory: the same input gives the same bytes.
#define RLE_STR_THREADS 256
#define RLE_STR_WAVES (RLE_STR_THREADS / XMEM_WAVE)
#define RLE_STR_MAX_GROUPS 6       // characters of a value the reader accepts: 30 bits
#define RLE_STR_MAX_CAPACITY (1 << 28)

namespace {

// Inclusive scan of one int per thread over the workgroup; `part` holds one word per wave, `total` is the workgroup's sum.  Two
// barriers: part may be reused right after the call.
template <typename T>
__device__ __forceinline__ T rle_block_scan(T v, T* part, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    T before = 0, sum = 0;
    for (int w = 0; w < waves; ++w) {
        const T t = part[w];
        if (w < wave) before += t;
        sum += t;
    }
    __syncthreads();
    total = sum;
    return incl + before;
}

// The frame's labels for the compressor: s_ev[k] = start of label k in the packed events, s_val[k] = start of its values (a label
// with E >= 1 events has E + 1 values, a label without event none), both with a closing entry [K].  Returns false - for every
// thread - when a count is negative or the events did not fit `capacity`: nothing of the frame may be read then.
__device__ __forceinline__ bool rle_label_starts(const int* __restrict__ mt, int K, int capacity, int* s_ev, int* s_val, int* s_ok) {
    if (threadIdx.x == 0) {
        int ev = 0, val = 0, ok = 1;
        for (int k = 0; k < K; ++k) {
            const int e = mt[(size_t)k * XMEM_RLE_META];
            s_ev[k] = ev;
            s_val[k] = val;
            if (e < 0 || e > capacity - ev) { ok = 0; break; }
            ev += e;
            val += e > 0 ? e + 1 : 0;
        }
        s_ev[K] = ev;
        s_val[K] = val;
        *s_ok = ok;
    }
    __syncthreads();
    return *s_ok != 0;
}

// Value t of the frame: its label by binary search in s_val, then x from at most four events.  Unsigned arithmetic: a record that is
// no encoder's (events not ascending) wraps instead of overflowing, and still gives a string of the length the scan counted.
__device__ __forceinline__ int rle_value(const uint32_t* __restrict__ ev_frame, const int* s_ev, const int* s_val, int K, int t,
                                         uint32_t hw) {
    int lo = 0, hi = K - 1;                              // the last k with s_val[k] <= t among labels that have values
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_val[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int i = t - s_val[lo], E = s_ev[lo + 1] - s_ev[lo];        // count i of 0..E; E >= 1 because the label has values
    const uint32_t* e = ev_frame + s_ev[lo];                         // e[0 .. E) lies below `capacity`
    const uint32_t hi_i = i < E ? e[i] : hw, lo_i = i > 0 ? e[i - 1] : 0u;
    uint32_t x = hi_i - lo_i;
    if (i > 2) x -= e[i - 2] - e[i - 3];                             // c[i - 2]; i - 2 <= E - 1
    return (int)x;
}

// the characters of x, at most 7 for any int; returns their number
__device__ __forceinline__ int rle_value_chars(int x, uint8_t (&out)[7]) {
    int n = 0;
    bool more = true;
#pragma unroll
    for (int g = 0; g < 7; ++g) {                        // static indices: the characters stay in registers
        const int c = x & 0x1f;
        x >>= 5;                                         // arithmetic
        const bool next = (c & 0x10) ? (x != -1) : (x != 0);
        out[g] = (uint8_t)((c | (next ? 0x20 : 0)) + 48);
        if (more) n = g + 1;
        more = more && next;
    }
    return n;
}

template <bool EMIT>
__global__ __launch_bounds__(RLE_STR_THREADS) void rle_compress_kernel(const int* __restrict__ meta, const uint32_t* __restrict__ events,
                                                                      int H, int W, int K, int capacity, int char_capacity,
                                                                      int* __restrict__ ofs, uint8_t* __restrict__ chars) {
    __shared__ int s_ev[256], s_val[256], s_ok;
    const int n = blockIdx.y, t = blockIdx.x * RLE_STR_THREADS + threadIdx.x;
    if (!rle_label_starts(meta + (size_t)n * K * XMEM_RLE_META, K, capacity, s_ev, s_val, &s_ok)) return;
    if (t >= s_val[K]) return;
    uint8_t c[7];
    const int len = rle_value_chars(rle_value(events + (size_t)n * capacity, s_ev, s_val, K, t, (uint32_t)H * (uint32_t)W), c);
    int* slot = ofs + (size_t)n * (capacity + K) + t;
    if (!EMIT) {
        *slot = len;
    } else {
        const int at = *slot;
        uint8_t* out = chars + (size_t)n * char_capacity;
#pragma unroll
        for (int g = 0; g < 7; ++g)
            if (g < len && at + g < char_capacity) out[at + g] = c[g];
    }
}

__global__ __launch_bounds__(RLE_SCAN_THREADS) void rle_compress_scan_kernel(const int* __restrict__ meta, int K, int capacity,
                                                                            int* __restrict__ ofs, int* __restrict__ str_len) {
    __shared__ int s_part[RLE_SCAN_THREADS / XMEM_WAVE];
    __shared__ int s_ev[256], s_val[256], s_start[256], s_ok;
    const int n = blockIdx.x, tid = threadIdx.x;
    if (!rle_label_starts(meta + (size_t)n * K * XMEM_RLE_META, K, capacity, s_ev, s_val, &s_ok)) {
        if (tid < K) str_len[(size_t)n * K + tid] = -1;
        return;
    }
    int* c = ofs + (size_t)n * (capacity + K);
    const int M = s_val[K];
    int carry = 0;
    for (int base = 0; base < M; base += RLE_SCAN_THREADS) {         // uniform over the workgroup
        const int i = base + tid;
        const int v = i < M ? c[i] : 0;
        int total;
        const int excl = carry + rle_block_scan(v, s_part, total) - v;
        if (i < M) c[i] = excl;
        carry += total;
    }
    __syncthreads();
    // the first character of label k: the scanned position of its first value (the frame's total where no value follows)
    if (tid <= K) s_start[tid] = s_val[tid] < M ? c[s_val[tid]] : carry;
    __syncthreads();
    if (tid < K) str_len[(size_t)n * K + tid] = s_start[tid + 1] - s_start[tid];
}

// One string, [begin, end) of `chars`.  EMIT = false: -> s_res = {status, number of values}.  EMIT = true: events[i] for i < m - 1.
template <bool EMIT>
__device__ __forceinline__ void rle_string_walk(const uint8_t* __restrict__ chars, int begin, int end, long long hw, int m,
                                                uint32_t* __restrict__ ev_row, int room, int* s_res) {
    __shared__ long long s_part[2 * RLE_STR_WAVES];
    __shared__ int s_ipart[RLE_STR_WAVES];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int rank0 = 0;                                       // values before this chunk
    long long even = 0, odd = 0, pos = 0;                // c[i - 2] for the next even / odd i, and the position, carried
    for (int base = begin; base < end; base += RLE_STR_THREADS) {    // uniform over the workgroup
        const int p = base + tid;
        int c = 0x20, bad = 0;                           // beyond the end: neither a value's last character nor a fault
        if (p < end) {
            c = (int)chars[p] - 48;
            if (c < 0 || c > 63) { bad |= 1; c = 0x20; }
            if (p == end - 1 && (c & 0x20)) bad |= 1;    // the string ends inside a value
        }
        const bool term = !(c & 0x20);
        int x = 0;
        if (term) {
            uint32_t u = (uint32_t)(c & 0x1f);
            if (c & 0x10) u |= 0xffffffe0u;              // the last group carries the sign
            int back = 1;
            for (; back < RLE_STR_MAX_GROUPS && p - back >= begin; ++back) {
                const int d = (int)chars[p - back] - 48; // inside [begin, end); a character outside 48..111 is reported by its owner
                if (d < 0 || d > 63 || !(d & 0x20)) break;
                u = (u << 5) | (uint32_t)(d & 0x1f);
            }
            if (back == RLE_STR_MAX_GROUPS && p - back >= begin) {   // a seventh character of the same value
                const int d = (int)chars[p - back] - 48;
                if (d >= 0 && d <= 63 && (d & 0x20)) bad |= 1;
            }
            x = (int)u;
        }
        int nterm;
        const int i = rank0 + rle_block_scan(term ? 1 : 0, s_ipart, nterm) - 1;      // this value's index, where term
        const bool ev = term && i >= 2 && !(i & 1), od = term && (i & 1);
        long long te, to, tc;
        const long long se = rle_block_scan<long long>(ev ? x : 0, s_part, te);
        const long long so = rle_block_scan<long long>(od ? x : 0, s_part + RLE_STR_WAVES, to);
        long long cnt = 0;
        if (term) {
            cnt = i == 0 ? (long long)x : (i & 1) ? odd + so : even + se;
            if (cnt < 0 || (i > 0 && cnt == 0)) bad |= 2;
        }
        const long long at = pos + rle_block_scan<long long>(cnt, s_part, tc);        // the end of count i: event i
        if (EMIT) {
            if (term && i < m - 1 && i < room) ev_row[i] = (uint32_t)at;
        } else if (bad) {
            atomicOr(&s_bad, bad);
        }
        rank0 += nterm;
        even += te;
        odd += to;
        pos += tc;
    }
    if (!EMIT) {
        __syncthreads();
        if (tid == 0) {
            const int bad = s_bad;
            const int status = (bad & 1) ? 1 : ((bad & 2) || pos != hw) ? 2 : 0;
            s_res[0] = status;
            s_res[1] = status == 0 ? rank0 : 0;
        }
    }
}

// a row's range of `chars`: false when the offsets do not describe one (status 1); an empty range is a row without string
__device__ __forceinline__ bool rle_row_range(const int* __restrict__ str_ofs, int row_in_table, int chars_len, int& begin, int& end) {
    begin = str_ofs[row_in_table];
    end = str_ofs[row_in_table + 1];
    return begin >= 0 && begin <= end && end <= chars_len;
}

// workspace of the reader: int32 [N][K][2] = {number of values (0: no events to write), the row's start in the frame's events}
__global__ __launch_bounds__(RLE_STR_THREADS) void rle_decompress_check_kernel(const uint8_t* __restrict__ chars, int chars_len,
                                                                              const int* __restrict__ str_ofs, int H, int W, int K,
                                                                              int* __restrict__ ws, int* __restrict__ status) {
    __shared__ int s_res[2];
    const int k = blockIdx.x, n = blockIdx.y;
    const size_t row = (size_t)n * K + k;
    int begin, end;
    const bool ok = rle_row_range(str_ofs, n * (K + 1) + k, chars_len, begin, end);
    if (!ok || begin == end) {                           // uniform over the workgroup
        if (threadIdx.x == 0) {
            status[row] = ok ? 0 : 1;
            ws[2 * row] = 0;
        }
        return;
    }
    rle_string_walk<false>(chars, begin, end, (long long)H * W, 0, nullptr, 0, s_res);
    if (threadIdx.x == 0) {
        status[row] = s_res[0];
        ws[2 * row] = s_res[1];
    }
}

__global__ __launch_bounds__(256) void rle_decompress_scan_kernel(int K, int capacity, int* __restrict__ ws, int* __restrict__ meta,
                                                                  int* __restrict__ status) {
    __shared__ int s_part[4];
    const int n = blockIdx.x, k = threadIdx.x;
    const size_t row = (size_t)n * K + k;
    const int m = k < K ? ws[2 * row] : 0;               // K <= 254: one row per thread
    const int e = m > 1 ? m - 1 : 0;
    int total;
    const int start = rle_block_scan(e, s_part, total) - e;
    if (k >= K) return;
    const bool fits = total <= capacity;
    if (!fits && m > 0) status[row] = 3;                 // every good string of the frame: the frame is to be read again with more room
    ws[2 * row] = fits ? m : 0;
    ws[2 * row + 1] = start;
    int* mt = meta + row * XMEM_RLE_META;
    mt[0] = fits ? e : 0;
#pragma unroll
    for (int f = 1; f < XMEM_RLE_META; ++f) mt[f] = 0;
}

__global__ __launch_bounds__(RLE_STR_THREADS) void rle_decompress_expand_kernel(const uint8_t* __restrict__ chars, int chars_len,
                                                                               const int* __restrict__ str_ofs, int H, int W, int K,
                                                                               int capacity, const int* __restrict__ ws,
                                                                               uint32_t* __restrict__ events) {
    const int k = blockIdx.x, n = blockIdx.y;
    const size_t row = (size_t)n * K + k;
    const int m = ws[2 * row], start = ws[2 * row + 1];
    int begin, end;
    if (m < 2 || !rle_row_range(str_ofs, n * (K + 1) + k, chars_len, begin, end)) return;     // uniform over the workgroup
    if (start < 0 || start >= capacity) return;
    rle_string_walk<true>(chars, begin, end, (long long)H * W, m, events + (size_t)n * capacity + start, capacity - start, nullptr);
}

}  // namespace

extern "C" size_t xmem_rle_compress_workspace_bytes(int N, int K, int capacity) {
    if (!rle_args_ok(N, 1, K) || !rle_size_ok(N, 1, 1) || capacity < 1 || capacity > RLE_STR_MAX_CAPACITY) return 0;
    return (size_t)N * ((size_t)capacity + K) * sizeof(int32_t);
}

extern "C" int xmem_rle_compress(const int32_t* meta, const uint32_t* events, int N, int H, int W, int K, int capacity,
                                 int char_capacity, int32_t* str_len, uint8_t* chars, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    if (!meta || !events || !str_len || !chars || !workspace || H <= 0 || capacity < 1 || char_capacity < 1 || !rle_args_ok(N, W, K))
        return XMEM_ERR_BAD_ARG;
    if (!rle_size_ok(N, H, W) || capacity > RLE_STR_MAX_CAPACITY) return XMEM_ERR_UNSUPPORTED;
    if (workspace_bytes < xmem_rle_compress_workspace_bytes(N, K, capacity) || ((uintptr_t)workspace & 3)) return XMEM_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    int* ofs = (int*)workspace;
    const dim3 grid(cdiv(capacity + K, RLE_STR_THREADS), N), block(RLE_STR_THREADS);
    hipLaunchKernelGGL(rle_compress_kernel<false>, grid, block, 0, s, (const int*)meta, events, H, W, K, capacity, char_capacity, ofs,
                       chars);
    int rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(rle_compress_scan_kernel, dim3(N), dim3(RLE_SCAN_THREADS), 0, s, (const int*)meta, K, capacity, ofs,
                       (int*)str_len);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(rle_compress_kernel<true>, grid, block, 0, s, (const int*)meta, events, H, W, K, capacity, char_capacity, ofs,
                       chars);
    return xmem_check_launch();
}

extern "C" size_t xmem_rle_decompress_workspace_bytes(int N, int K) {
    if (!rle_args_ok(N, 1, K) || !rle_size_ok(N, 1, 1)) return 0;
    return (size_t)N * K * 2 * sizeof(int32_t);
}

extern "C" int xmem_rle_decompress(const uint8_t* chars, int chars_len, const int32_t* str_ofs, int N, int H, int W, int K,
                                   int capacity, int32_t* meta, uint32_t* events, int32_t* status, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (!chars || !str_ofs || !meta || !events || !status || !workspace || H <= 0 || capacity < 1 || chars_len < 0 ||
        !rle_args_ok(N, W, K))
        return XMEM_ERR_BAD_ARG;
    if (!rle_size_ok(N, H, W)) return XMEM_ERR_UNSUPPORTED;
    if (workspace_bytes < xmem_rle_decompress_workspace_bytes(N, K) || ((uintptr_t)workspace & 3)) return XMEM_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    int* ws = (int*)workspace;
    const dim3 grid(K, N), block(RLE_STR_THREADS);
    hipLaunchKernelGGL(rle_decompress_check_kernel, grid, block, 0, s, chars, chars_len, (const int*)str_ofs, H, W, K, ws, (int*)status);
    int rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(rle_decompress_scan_kernel, dim3(N), dim3(256), 0, s, K, capacity, ws, (int*)meta, (int*)status);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(rle_decompress_expand_kernel, grid, block, 0, s, chars, chars_len, (const int*)str_ofs, H, W, K, capacity,
                       (const int*)ws, events);
    return xmem_check_launch();
}
