// Polygon outlines of uint8 index maps (include/xmem_hip_polygons.h, xmem_mask_polygons; xmem2_amd/polygons.py has the definition).
//
// Whether a lattice vertex is a corner of label k follows from its 2 x 2 pixels a b / c d (NW NE / SW SE) alone: 1 or 3 of them in
// {m == k} give one corner, the two diagonal patterns (a "saddle") two, anything else none; at most 4 corners meet in a vertex over
// all labels.  A ring alternates horizontal and vertical edges, and on one lattice line the corners of a label pair up in sorted
// order as the ends of its boundary runs (at a saddle the corner of the run from the left / from above sorts first).  So every
// corner gets two ranks within its frame, g in the order (label, y, x) and c in the order (label, x, y) - the labels' shares are the
// same in both and even -, and the corner it is entered from is g ^ 1 when its incoming edge is horizontal, the corner whose c is
// its own c ^ 1 otherwise.  The start of a ring is its smallest g.  Launches, whatever the maps hold:
//   components   xmem_components, 8-connected: `outer` [N][K] counts the roots of every label (poly_outer_kernel);
//   row count    a wave owns a lattice row and walks it in chunks of 64 vertices; per label present a ballot gives the number of
//                corners, added to the wave's own slot (label, row); the counts per (label, column) and the sum of the turns per label
//                (+1 for a corner of 1 pixel, -1 for one of 3 pixels or of a saddle) are integer atomic sums;
//   scan         one workgroup per frame: exclusive scans of both count tables, `meta`: corners = the label's share, rings =
//                2 outer - turns / 4 (outer rings turn by +4, holes by -4, outer rings are the 8-connected components);
//   row emit     the same walk: vert[g] = x | y << 16 | incoming edge horizontal << 31;
//   column emit  a workgroup owns 64 lattice columns and turns tiles of 64 rows through LDS (rows of 17 words: lane r reads word
//                17 r + .., 64 different banks), a wave walks one column at a time: c from the wave's slot (label, column), g by binary
//                search for x in the (label, row) share of vert; colrank[g] = c, colinv[c] = g;
//   init, rounds pred[g]; then `rounds` times: (jump, smallest g, steps back to it) of a window of 2^t corners backwards, doubled;
//                with a capacity of at most 4096 corners these two, the ring scan and the emit are ONE launch, a workgroup per frame
//                with the windows in LDS (poly_rank_lds_kernel); a larger capacity takes ceil(log2(.)) launches on global arrays;
//   ring scan    one workgroup per frame: exclusive scan over g of the ring's length at its start (steps of the start's
//                predecessor + 1) - the rings of a label in the order of their starts, the labels back to back;
//   emit         corner g goes to (start of its ring) + (steps back to the start).
// No workgroup waits for another; every output position is a scanned count; a frame whose corners exceed `capacity` stops after
// the scan.  Every index read from the workspace is checked against the frame's total before it is used.
#include "common.hpp"
#include "../../include/xmem_hip_masks.h"
#include "../../include/xmem_hip_polygons.h"

#define POLY_MAX_HW 16384
#define POLY_THREADS 256
#define POLY_WAVES (POLY_THREADS / XMEM_WAVE)
#define POLY_TILE 64                // lattice columns of a workgroup and rows of a tile in the column walk
#define POLY_STRIDE 68              // bytes of an LDS tile row: 65 pixels, padded to 17 words
#define POLY_SCAN_THREADS 1024
#define POLY_EW_BLOCKS 2048
#define POLY_LDS_CORNERS 4096       // a capacity up to this is ranked by one workgroup per frame in LDS (3 words per corner: 48 KiB)
#define POLY_LDS_PER (POLY_LDS_CORNERS / POLY_SCAN_THREADS)

namespace {

typedef unsigned long long u64;

// the corners of label L at a vertex with the pixels a b / c d: 0, 1 or 2; `turn`: +1 / -1 / -2
__device__ __forceinline__ int poly_corners(int a, int b, int c, int d, int L, int& turn) {
    const int bits = (a == L) | ((b == L) << 1) | ((c == L) << 2) | ((d == L) << 3);
    const int n = __popc(bits);
    turn = n == 1 ? 1 : n == 3 ? -1 : -2;
    if (n == 1 || n == 3) return 1;
    if (bits == 9 || bits == 6) return 2;
    turn = 0;
    return 0;
}

// which of a, b, c, d (bits 0..3) name a label of their own with corners here: the lane's work list
__device__ __forceinline__ int poly_todo(int a, int b, int c, int d) {
    int t, todo = 0;
    if (a && poly_corners(a, b, c, d, a, t)) todo |= 1;
    if (b && b != a && poly_corners(a, b, c, d, b, t)) todo |= 2;
    if (c && c != a && c != b && poly_corners(a, b, c, d, c, t)) todo |= 4;
    if (d && d != a && d != b && d != c && poly_corners(a, b, c, d, d, t)) todo |= 8;
    return todo;
}
__device__ __forceinline__ int poly_pick(int todo, int a, int b, int c, int d) {
    return (todo & 1) ? a : (todo & 2) ? b : (todo & 4) ? c : d;
}
__device__ __forceinline__ int poly_done(int todo, int a, int b, int c, int d, int L) {
    return todo & ~((a == L) | ((b == L) << 1) | ((c == L) << 2) | ((d == L) << 3));
}

__global__ __launch_bounds__(POLY_THREADS) void poly_outer_kernel(const uint8_t* __restrict__ masks, const int32_t* __restrict__ root,
                                                                  int hw, int K, int* outer) {
    const size_t base = (size_t)blockIdx.y * (size_t)hw;
    for (int p = blockIdx.x * POLY_THREADS + threadIdx.x; p < hw; p += gridDim.x * POLY_THREADS) {
        const int v = masks[base + p];
        if (v >= 1 && v <= K && root[base + p] == p) atomicAdd(outer + (size_t)blockIdx.y * K + (v - 1), 1);
    }
}

// One wave per lattice row y (0..H), chunks of 64 vertices.  rowofs [N][K][H + 1]: EMIT = false adds the counts up in it, EMIT = true
// finds the scanned starts there and leaves the ends (the start of the next line of the table).
template <bool EMIT>
__global__ __launch_bounds__(POLY_THREADS) void poly_row_kernel(const uint8_t* __restrict__ masks, int H, int W, int K, int capacity,
                                                                int* rowofs, int* colcnt, int* turn, const int* __restrict__ tot,
                                                                uint32_t* __restrict__ vert) {
    const int n = blockIdx.y, lane = threadIdx.x & 63;
    const int vy = blockIdx.x * POLY_WAVES + (threadIdx.x >> 6);
    if (vy > H) return;                                  // uniform over the wave; no barrier in this kernel
    if (EMIT && tot[n] > capacity) return;
    const uint8_t* m = masks + (size_t)n * H * W;
    const u64 below = (1ull << lane) - 1ull;
    int carry_b = 0, carry_d = 0;
    for (int cx = 0; cx <= W; cx += 64) {
        const int vx = cx + lane;
        int b = 0, d = 0;
        if (vx < W) {
            if (vy > 0) b = m[(size_t)(vy - 1) * W + vx];
            if (vy < H) d = m[(size_t)vy * W + vx];
        }
        if (b > K) b = 0;
        if (d > K) d = 0;
        int a = __shfl_up(b, 1, 64), c = __shfl_up(d, 1, 64);
        if (lane == 0) { a = carry_b; c = carry_d; }
        carry_b = __shfl(b, 63, 64);
        carry_d = __shfl(d, 63, 64);
        if (vx > W) { a = 0; b = 0; c = 0; d = 0; }
        int todo = poly_todo(a, b, c, d);
        u64 pend = __ballot(todo != 0);
        while (pend) {                                   // one turn per label with corners in this chunk
            const int L = __shfl(poly_pick(todo, a, b, c, d), __ffsll((long long)pend) - 1, 64);
            int t;
            const int nc = poly_corners(a, b, c, d, L, t);
            const u64 m1 = __ballot(nc >= 1), m2 = __ballot(nc == 2);
            int* slot = rowofs + ((size_t)n * K + (L - 1)) * (size_t)(H + 1) + vy;
            int at = 0;
            if (lane == 0) {                             // this wave alone touches (n, L, vy)
                at = *slot;
                *slot = at + __popcll(m1) + __popcll(m2);
            }
            at = __shfl(at, 0, 64);
            if (!EMIT) {
                if (nc) atomicAdd(colcnt + ((size_t)n * K + (L - 1)) * (size_t)(W + 1) + vx, nc);
                const int tsum = __popcll(__ballot(t == 1)) - __popcll(__ballot(t == -1)) - 2 * __popcll(m2);
                if (lane == 0 && tsum != 0) atomicAdd(turn + (size_t)n * K + (L - 1), tsum);
            } else if (nc) {
                const int g = at + __popcll(m1 & below) + __popcll(m2 & below);
                const bool aL = a == L, bL = b == L, cL = c == L, dL = d == L;
                // the incoming edge: from the west if c && !a, from the east if b && !d; both corners of a saddle share the answer
                const uint32_t in_h = ((cL && !aL) || (bL && !dL)) ? 0x80000000u : 0u;
                const uint32_t w = (uint32_t)vx | ((uint32_t)vy << 16) | in_h;
                if (g < capacity) vert[(size_t)n * capacity + g] = w;
                if (nc == 2 && g + 1 < capacity) vert[(size_t)n * capacity + g + 1] = w;
            }
            todo = poly_done(todo, a, b, c, d, L);
            pend = __ballot(todo != 0);
        }
    }
}

// Exclusive scans, in place, of a frame's two count tables; both give every label the same share [lbase[k], lbase[k + 1]).
__device__ __forceinline__ int poly_scan_table(int* c, int M, int line, int* s_wave, int* s_start) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < M; base += POLY_SCAN_THREADS) {
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
        for (int w = 0; w < POLY_SCAN_THREADS / XMEM_WAVE; ++w) {
            const int t = s_wave[w];
            if (w < wave) before += t;
            total += t;
        }
        const int excl = carry + before + incl - v;
        if (i < M) {
            c[i] = excl;
            if (s_start && i % line == 0) s_start[i / line] = excl;
        }
        carry += total;
        __syncthreads();
    }
    return carry;
}

__global__ __launch_bounds__(POLY_SCAN_THREADS) void poly_scan_kernel(int* __restrict__ rowofs, int* __restrict__ colofs,
                                                                       const int* __restrict__ outer, const int* __restrict__ turn,
                                                                       int H, int W, int K, int* __restrict__ tot, int* __restrict__ meta) {
    __shared__ int s_wave[POLY_SCAN_THREADS / XMEM_WAVE];
    __shared__ int s_start[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int total = poly_scan_table(rowofs + (size_t)n * K * (H + 1), K * (H + 1), H + 1, s_wave, s_start);
    poly_scan_table(colofs + (size_t)n * K * (W + 1), K * (W + 1), W + 1, s_wave, nullptr);
    if (tid == 0) tot[n] = total;
    if (tid < K) {
        int* mt = meta + ((size_t)n * K + tid) * XMEM_POLY_META;
        mt[XMEM_POLY_CORNERS] = (tid + 1 < K ? s_start[tid + 1] : total) - s_start[tid];
        mt[XMEM_POLY_RINGS] = 2 * outer[(size_t)n * K + tid] - turn[(size_t)n * K + tid] / 4;
    }
}

// One workgroup per 64 lattice columns; wave w walks the columns 16 w .. 16 w + 15 of the strip down the tiles.
__global__ __launch_bounds__(POLY_THREADS) void poly_col_kernel(const uint8_t* __restrict__ masks, int H, int W, int K, int capacity,
                                                                const int* __restrict__ rowofs, int* colofs, const int* __restrict__ tot,
                                                                const uint32_t* __restrict__ vert, int* __restrict__ colrank,
                                                                int* __restrict__ colinv) {
    __shared__ uint32_t s_tile[POLY_TILE * POLY_STRIDE / 4];
    __shared__ uint8_t s_halo[POLY_STRIDE];
    const int n = blockIdx.y, X0 = blockIdx.x * POLY_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int total = tot[n];
    if (total > capacity) return;                        // uniform over the workgroup
    const uint8_t* m = masks + (size_t)n * H * W;
    uint8_t* tile = reinterpret_cast<uint8_t*>(s_tile);
    const int* rows = rowofs + (size_t)n * K * (H + 1);
    const uint32_t* vt = vert + (size_t)n * capacity;
    const u64 below = (1ull << lane) - 1ull;

    for (int ty0 = 0; ty0 <= H; ty0 += POLY_TILE) {
        {                                                // tile column j holds the pixel column X0 - 1 + j, j = 0..64
            const int x = X0 - 1 + lane;
#pragma unroll 4
            for (int i = 0; i < POLY_TILE / POLY_WAVES; ++i) {
                const int r = wave + POLY_WAVES * i, y = ty0 + r;
                uint8_t v = 0;
                if (y < H && x >= 0 && x < W) v = m[(size_t)y * W + x];
                tile[r * POLY_STRIDE + lane] = v;
            }
            if (tid < POLY_TILE) {
                const int y = ty0 + tid, xr = X0 + POLY_TILE - 1;
                uint8_t v = 0;
                if (y < H && xr < W) v = m[(size_t)y * W + xr];
                tile[tid * POLY_STRIDE + POLY_TILE] = v;
            } else if (tid < 2 * POLY_TILE + 1) {        // the pixel row above the tile
                const int j = tid - POLY_TILE, xh = X0 - 1 + j;
                uint8_t v = 0;
                if (ty0 > 0 && xh >= 0 && xh < W) v = m[(size_t)(ty0 - 1) * W + xh];
                s_halo[j] = v;
            }
        }
        __syncthreads();

        const int vy = ty0 + lane;
        for (int jj = 0; jj < POLY_TILE / POLY_WAVES; ++jj) {
            const int cj = wave * (POLY_TILE / POLY_WAVES) + jj, vx = X0 + cj;
            if (vx > W) break;                           // uniform over the wave
            int c = tile[lane * POLY_STRIDE + cj], d = tile[lane * POLY_STRIDE + cj + 1];
            if (c > K) c = 0;
            if (d > K) d = 0;
            int a = __shfl_up(c, 1, 64), b = __shfl_up(d, 1, 64);
            if (lane == 0) {
                a = s_halo[cj];
                b = s_halo[cj + 1];
                if (a > K) a = 0;
                if (b > K) b = 0;
            }
            if (vy > H) { a = 0; b = 0; c = 0; d = 0; }
            int todo = poly_todo(a, b, c, d);
            u64 pend = __ballot(todo != 0);
            while (pend) {
                const int L = __shfl(poly_pick(todo, a, b, c, d), __ffsll((long long)pend) - 1, 64);
                int t;
                const int nc = poly_corners(a, b, c, d, L, t);
                const u64 m1 = __ballot(nc >= 1), m2 = __ballot(nc == 2);
                int* slot = colofs + ((size_t)n * K + (L - 1)) * (size_t)(W + 1) + vx;
                int at = 0;
                if (lane == 0) {                         // this wave alone touches (n, L, vx), tile after tile
                    at = *slot;
                    *slot = at + __popcll(m1) + __popcll(m2);
                }
                at = __shfl(at, 0, 64);
                if (nc) {
                    const int cr = at + __popcll(m1 & below) + __popcll(m2 & below);
                    // the corner's share of the row-major list: the line (L, vy) of the row table, which now holds the ends
                    const int li = (L - 1) * (H + 1) + vy;
                    int lo = li > 0 ? rows[li - 1] : 0, hi = rows[li];
                    if (lo < 0) lo = 0;
                    if (hi > total) hi = total;
                    const int end = hi;
                    while (lo < hi) {                    // the first corner of the line with x >= vx
                        const int mid = (lo + hi) >> 1;
                        if ((int)(vt[mid] & 0xffffu) < vx) lo = mid + 1; else hi = mid;
                    }
                    // a saddle's corners in column order are (north, south); in row order (west, east).  a & d: north is the east one
                    const int first = (nc == 2 && a == L) ? 1 : 0;
                    const int g0 = lo + first, g1 = lo + 1 - first;
                    if (g0 < end && cr < total) {
                        colrank[(size_t)n * capacity + g0] = cr;
                        colinv[(size_t)n * capacity + cr] = g0;
                    }
                    if (nc == 2 && g1 < end && cr + 1 < total) {
                        colrank[(size_t)n * capacity + g1] = cr + 1;
                        colinv[(size_t)n * capacity + cr + 1] = g1;
                    }
                }
                todo = poly_done(todo, a, b, c, d, L);
                pend = __ballot(todo != 0);
            }
        }
        __syncthreads();                                 // the tile is rewritten
    }
}

// pred[g], and the window of one corner: (jump, smallest, steps) = (pred[g], g, 0)
__global__ __launch_bounds__(POLY_THREADS) void poly_init_kernel(const int* __restrict__ tot, int capacity, const uint32_t* __restrict__ vert,
                                                                 const int* __restrict__ colrank, const int* __restrict__ colinv,
                                                                 int* __restrict__ pred, int* __restrict__ jump, int* __restrict__ low,
                                                                 int* __restrict__ steps) {
    const int n = blockIdx.y, g = blockIdx.x * POLY_THREADS + threadIdx.x, total = tot[n];
    if (total > capacity || g >= total) return;
    const size_t f = (size_t)n * capacity;
    int p = g ^ 1;
    if (!(vert[f + g] >> 31)) {
        const int cr = colrank[f + g];
        p = ((unsigned)cr < (unsigned)total && (cr ^ 1) < total) ? colinv[f + (cr ^ 1)] : g;
    }
    if ((unsigned)p >= (unsigned)total) p = g;
    pred[f + g] = p;
    jump[f + g] = p;
    low[f + g] = g;
    steps[f + g] = 0;
}

// windows of `span` corners backwards become windows of 2 span: the nearer half wins a tie, so `steps` is the first way back
__global__ __launch_bounds__(POLY_THREADS) void poly_round_kernel(const int* __restrict__ tot, int capacity, int span,
                                                                  const int* __restrict__ jump_in, const int* __restrict__ low_in,
                                                                  const int* __restrict__ steps_in, int* __restrict__ jump_out,
                                                                  int* __restrict__ low_out, int* __restrict__ steps_out) {
    const int n = blockIdx.y, g = blockIdx.x * POLY_THREADS + threadIdx.x, total = tot[n];
    if (total > capacity || g >= total) return;
    const size_t f = (size_t)n * capacity;
    const int q = jump_in[f + g];                        // below total: poly_init_kernel checked pred, and jumps are preds of preds
    int lo = low_in[f + g], st = steps_in[f + g];
    const int lq = low_in[f + q];
    if (lq < lo) {
        lo = lq;
        st = span + steps_in[f + q];
    }
    jump_out[f + g] = jump_in[f + q];
    low_out[f + g] = lo;
    steps_out[f + g] = st;
}

__global__ __launch_bounds__(POLY_SCAN_THREADS) void poly_ring_scan_kernel(const int* __restrict__ tot, int capacity,
                                                                            const int* __restrict__ pred, const int* __restrict__ low,
                                                                            const int* __restrict__ steps, int* __restrict__ ringofs) {
    __shared__ int s_wave[POLY_SCAN_THREADS / XMEM_WAVE];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, total = tot[n];
    if (total > capacity) return;                        // uniform over the workgroup
    const size_t f = (size_t)n * capacity;
    int carry = 0;
    for (int base = 0; base < total; base += POLY_SCAN_THREADS) {
        const int g = base + tid;
        int v = 0;
        if (g < total && low[f + g] == g) v = steps[f + pred[f + g]] + 1;      // the ring's length, at its start
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, sum = 0;
        for (int w = 0; w < POLY_SCAN_THREADS / XMEM_WAVE; ++w) {
            const int t = s_wave[w];
            if (w < wave) before += t;
            sum += t;
        }
        if (g < total) ringofs[f + g] = carry + before + incl - v;
        carry += sum;
        __syncthreads();
    }
}

__global__ __launch_bounds__(POLY_THREADS) void poly_emit_kernel(const int* __restrict__ tot, int capacity, const uint32_t* __restrict__ vert,
                                                                 const int* __restrict__ low, const int* __restrict__ steps,
                                                                 const int* __restrict__ ringofs, uint32_t* __restrict__ corners) {
    const int n = blockIdx.y, g = blockIdx.x * POLY_THREADS + threadIdx.x, total = tot[n];
    if (total > capacity || g >= total) return;
    const size_t f = (size_t)n * capacity;
    const int s = low[f + g], st = steps[f + g];
    if ((unsigned)s >= (unsigned)total || st < 0) return;
    const long long pos = (long long)ringofs[f + s] + st;
    if (pos >= 0 && pos < total)
        corners[f + pos] = (vert[f + g] & 0x7fffffffu) | (st == 0 ? (1u << XMEM_POLY_FIRST_BIT) : 0u);
}

// init, rounds, ring scan and emit of one frame in one workgroup, for a capacity of at most POLY_LDS_CORNERS: the three words of a
// corner's window live in LDS, thread t owns the corners t, t + 1024, ..  The number of rounds follows the frame's own total - a loop
// inside the launch, uniform over the workgroup.
__global__ __launch_bounds__(POLY_SCAN_THREADS) void poly_rank_lds_kernel(const int* __restrict__ tot, int capacity,
                                                                           const uint32_t* __restrict__ vert, const int* __restrict__ colrank,
                                                                           const int* __restrict__ colinv, uint32_t* __restrict__ corners) {
    __shared__ int s_jump[POLY_LDS_CORNERS], s_low[POLY_LDS_CORNERS], s_steps[POLY_LDS_CORNERS];
    __shared__ int s_wave[POLY_SCAN_THREADS / XMEM_WAVE];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, total = tot[n];
    if (total > capacity || total > POLY_LDS_CORNERS) return;     // uniform over the workgroup
    const size_t f = (size_t)n * capacity;
    int pred[POLY_LDS_PER];
#pragma unroll
    for (int i = 0; i < POLY_LDS_PER; ++i) {
        const int g = tid + POLY_SCAN_THREADS * i;
        pred[i] = 0;
        if (g < total) {
            int p = g ^ 1;
            if (!(vert[f + g] >> 31)) {
                const int cr = colrank[f + g];
                p = ((unsigned)cr < (unsigned)total && (cr ^ 1) < total) ? colinv[f + (cr ^ 1)] : g;
            }
            if ((unsigned)p >= (unsigned)total) p = g;
            pred[i] = p;
            s_jump[g] = p;
            s_low[g] = g;
            s_steps[g] = 0;
        }
    }
    __syncthreads();
    for (int span = 1; span < total; span <<= 1) {
        int nj[POLY_LDS_PER], nl[POLY_LDS_PER], ns[POLY_LDS_PER];
#pragma unroll
        for (int i = 0; i < POLY_LDS_PER; ++i) {
            const int g = tid + POLY_SCAN_THREADS * i;
            if (g < total) {
                const int q = s_jump[g], lq = s_low[q];
                nj[i] = s_jump[q];
                nl[i] = s_low[g];
                ns[i] = s_steps[g];
                if (lq < nl[i]) {
                    nl[i] = lq;
                    ns[i] = span + s_steps[q];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < POLY_LDS_PER; ++i) {
            const int g = tid + POLY_SCAN_THREADS * i;
            if (g < total) {
                s_jump[g] = nj[i];
                s_low[g] = nl[i];
                s_steps[g] = ns[i];
            }
        }
        __syncthreads();
    }
    int carry = 0;                                       // the ring scan; s_jump becomes the start of the ring that begins at g
    for (int i = 0; i < POLY_LDS_PER; ++i) {
        const int g = tid + POLY_SCAN_THREADS * i;
        if (POLY_SCAN_THREADS * i >= total) break;       // uniform
        int v = 0;
        if (g < total && s_low[g] == g) v = s_steps[pred[i]] + 1;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, sum = 0;
        for (int w = 0; w < POLY_SCAN_THREADS / XMEM_WAVE; ++w) {
            const int t = s_wave[w];
            if (w < wave) before += t;
            sum += t;
        }
        if (g < total) s_jump[g] = carry + before + incl - v;
        carry += sum;
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < POLY_LDS_PER; ++i) {
        const int g = tid + POLY_SCAN_THREADS * i;
        if (g < total) {
            const int st = s_steps[g], pos = s_jump[s_low[g]] + st;      // s_low[g] < total: it is a g
            if (st >= 0 && pos >= 0 && pos < total)
                corners[f + pos] = (vert[f + g] & 0x7fffffffu) | (st == 0 ? (1u << XMEM_POLY_FIRST_BIT) : 0u);
        }
    }
}

int poly_check(int N, int H, int W, int K, int capacity) {
    if (N < 1 || N > 65535 || K < 1 || K > 254 || capacity < 1 || capacity > XMEM_POLY_MAX_CAPACITY) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > POLY_MAX_HW || W > POLY_MAX_HW) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

size_t poly_align(size_t bytes) { return align_up(bytes, (size_t)256); }

struct PolyLayout {
    size_t cc, root, area, rowofs, colofs, counters, tot, per_corner, total;
};

// counters: outer [N][K] and turn [N][K]; per_corner: 11 arrays [N][capacity], of which the LDS path needs the first 3
PolyLayout poly_layout(int N, int H, int W, int K, int capacity) {
    PolyLayout l;
    size_t at = 0;
    const size_t plane = poly_align((size_t)N * H * W * sizeof(int32_t));
    l.cc = at;         at += poly_align(xmem_components_workspace_bytes(N, H, W));
    l.root = at;       at += plane;
    l.area = at;       at += plane;
    l.rowofs = at;     at += poly_align((size_t)N * K * (H + 1) * sizeof(int32_t));
    l.colofs = at;     at += poly_align((size_t)N * K * (W + 1) * sizeof(int32_t));
    l.counters = at;   at += poly_align((size_t)N * K * 2 * sizeof(int32_t));
    l.tot = at;        at += poly_align((size_t)N * sizeof(int32_t));
    l.per_corner = at; at += (capacity <= POLY_LDS_CORNERS ? 3 : 11) * poly_align((size_t)N * capacity * sizeof(int32_t));
    l.total = at;
    return l;
}

int poly_rounds(int H, int W, int capacity) {
    long long most = 4ll * (H + 1) * (W + 1);
    if (capacity < most) most = capacity;
    int r = 0;
    while ((1ll << r) < most) ++r;
    return r;
}

}  // namespace

extern "C" size_t xmem_mask_polygons_workspace_bytes(int N, int H, int W, int K, int capacity) {
    return poly_check(N, H, W, K, capacity) == XMEM_OK ? poly_layout(N, H, W, K, capacity).total : 0;
}

extern "C" int xmem_mask_polygons(const uint8_t* masks, int N, int H, int W, int K, int capacity, int32_t* meta, uint32_t* corners,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    int rc = poly_check(N, H, W, K, capacity);
    if (rc != XMEM_OK) return rc;
    if (!masks || !meta || !corners || !workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)meta & 3) || ((uintptr_t)corners & 3))
        return XMEM_ERR_BAD_ARG;
    const PolyLayout l = poly_layout(N, H, W, K, capacity);
    if (workspace_bytes < l.total) return XMEM_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    int32_t* root = (int32_t*)(w + l.root);
    int32_t* area = (int32_t*)(w + l.area);
    int* rowofs = (int*)(w + l.rowofs);
    int* colofs = (int*)(w + l.colofs);
    int* outer = (int*)(w + l.counters);
    int* turn = outer + (size_t)N * K;
    int* tot = (int*)(w + l.tot);
    const size_t arr = poly_align((size_t)N * capacity * sizeof(int32_t));
    char* pc = w + l.per_corner;
    uint32_t* vert = (uint32_t*)pc;
    int* colrank = (int*)(pc + arr);
    int* colinv = (int*)(pc + 2 * arr);
    int* pred = (int*)(pc + 3 * arr);
    int* ringofs = (int*)(pc + 4 * arr);
    int* state[2][3];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j) state[i][j] = (int*)(pc + (5 + 3 * i + j) * arr);

    // rowofs, colofs and the counters are adjacent
    if (hipMemsetAsync(rowofs, 0, l.tot - l.rowofs, s) != hipSuccess) return XMEM_ERR_LAUNCH;
    rc = xmem_components(masks, N, H, W, 8, root, area, w + l.cc, l.root - l.cc, stream);
    if (rc != XMEM_OK) return rc;
    const int hw = H * W;
    int blocks = cdiv(hw, POLY_THREADS * 4);
    if (blocks > POLY_EW_BLOCKS) blocks = POLY_EW_BLOCKS;
    hipLaunchKernelGGL(poly_outer_kernel, dim3((unsigned)blocks, (unsigned)N), dim3(POLY_THREADS), 0, s, masks, (const int32_t*)root, hw,
                       K, outer);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    const dim3 row_grid((unsigned)cdiv(H + 1, POLY_WAVES), (unsigned)N), block(POLY_THREADS);
    hipLaunchKernelGGL(poly_row_kernel<false>, row_grid, block, 0, s, masks, H, W, K, capacity, rowofs, colofs, turn, (const int*)tot, vert);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(poly_scan_kernel, dim3((unsigned)N), dim3(POLY_SCAN_THREADS), 0, s, rowofs, colofs, (const int*)outer,
                       (const int*)turn, H, W, K, tot, (int*)meta);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(poly_row_kernel<true>, row_grid, block, 0, s, masks, H, W, K, capacity, rowofs, colofs, turn, (const int*)tot, vert);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(poly_col_kernel, dim3((unsigned)cdiv(W + 1, POLY_TILE), (unsigned)N), block, 0, s, masks, H, W, K, capacity,
                       (const int*)rowofs, colofs, (const int*)tot, (const uint32_t*)vert, colrank, colinv);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    if (capacity <= POLY_LDS_CORNERS) {
        hipLaunchKernelGGL(poly_rank_lds_kernel, dim3((unsigned)N), dim3(POLY_SCAN_THREADS), 0, s, (const int*)tot, capacity,
                           (const uint32_t*)vert, (const int*)colrank, (const int*)colinv, corners);
        return xmem_check_launch();
    }
    const dim3 corner_grid((unsigned)cdiv(capacity, POLY_THREADS), (unsigned)N);
    hipLaunchKernelGGL(poly_init_kernel, corner_grid, block, 0, s, (const int*)tot, capacity, (const uint32_t*)vert, (const int*)colrank,
                       (const int*)colinv, pred, state[0][0], state[0][1], state[0][2]);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    const int rounds = poly_rounds(H, W, capacity);
    for (int t = 0; t < rounds; ++t) {
        int** in = state[t & 1];
        int** out = state[(t + 1) & 1];
        hipLaunchKernelGGL(poly_round_kernel, corner_grid, block, 0, s, (const int*)tot, capacity, 1 << t, (const int*)in[0],
                           (const int*)in[1], (const int*)in[2], out[0], out[1], out[2]);
        rc = xmem_check_launch();
        if (rc != XMEM_OK) return rc;
    }
    int** fin = state[rounds & 1];
    hipLaunchKernelGGL(poly_ring_scan_kernel, dim3((unsigned)N), dim3(POLY_SCAN_THREADS), 0, s, (const int*)tot, capacity, (const int*)pred,
                       (const int*)fin[1], (const int*)fin[2], ringofs);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(poly_emit_kernel, corner_grid, block, 0, s, (const int*)tot, capacity, (const uint32_t*)vert, (const int*)fin[1],
                       (const int*)fin[2], (const int*)ringofs, corners);
    return xmem_check_launch();
}
