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
