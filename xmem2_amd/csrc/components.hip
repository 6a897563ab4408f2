// Connected components of uint8 index maps and the mask clean-up built on them (include/xmem_hip_masks.h has the definitions).
//
// Labelling is union-find in four launches, whatever the mask holds:
//   cc_local    a workgroup resolves one 32 x 32 tile in LDS: every pixel starts at the first pixel of its horizontal run (one ballot
//               per row), runs are united with the row above by atomicMin on the LDS labels, and the tile's roots are written to the
//               global parent array as frame indices y * W + x.  The order of a tile's pixels is the frame's, so a tile-local root
//               is the smallest frame index of its tile-local component.
//   cc_merge    one thread per pixel of a tile seam unites it with its neighbours across the seam: find both roots, link the LARGER
//               under the smaller with atomicMin(parent + larger, smaller); when the atomic finds that somebody else linked the root
//               first, the displaced link is united in turn.  A parent is always a smaller index of the same component, so the root
//               that survives is the component's smallest index in every order of arrival: `root` is the definition's, bit for bit.
//   cc_flatten  per tile: pixels are counted per tile-local component in LDS, each component then finds its root once, adds its count
//               to area[root] with ONE global atomic and hands the root to its pixels through LDS.
//   cc_gather   area[p] = area[root[p]] (roots keep what was added up in them; nobody else's slot is read).
// The parent array is read by other workgroups while cc_merge links it: those reads are relaxed agent-scope atomic loads.  A stale
// parent would still be an ancestor (links only ever move towards smaller indices) and the atomicMin that links tells the truth.
//
// The clean-up is two labellings and elementwise kernels between them; its cross-pixel facts (the largest component of a label,
// the labels around a hole) are integer max / min atomics, first reduced in LDS or restricted to the holes small enough to matter.
// Every index is formed from (x, y) checked against (W, H); parents and roots are indices the kernels wrote themselves.
#include "common.hpp"
#include "../../include/xmem_hip_masks.h"

#define CC_T 32                     // tile side
#define CC_PIX (CC_T * CC_T)
#define CC_THREADS 256
#define CC_PER (CC_PIX / CC_THREADS)
#define CC_MAX_SIDE 16384
#define CC_MAX_N 65535
#define CC_EW_BLOCKS 2048           // grid-stride elementwise kernels: 8 workgroups per CU
#define CC_LABELS 256

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ int lds_get(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(const int* lab, int i) {
    for (;;) {
        const int p = lds_get(lab + i);
        if (p == i) return i;
        i = p;
    }
}
__device__ __forceinline__ void lds_unite(int* lab, int a, int b) {
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);      // a was a root when read: link it under b unless somebody was faster
        if (old == a) return;
        a = old;                                    // the link a -> old that lost (or won) against b: unite old with b
    }
}

__device__ __forceinline__ int glb_get(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int glb_find(const int* par, int i) {
    for (;;) {
        const int p = glb_get(par + i);
        if (p == i) return i;
        i = p;
    }
}
__device__ __forceinline__ void glb_unite(int* par, int a, int b) {
    for (;;) {
        a = glb_find(par, a);
        b = glb_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

// one tile per workgroup; thread t owns the tile pixels i = k * 256 + t: a wave covers two tile rows, lane & 31 is the column
__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const uint8_t* __restrict__ masks, int H, int W, int conn,
                                                              int32_t* __restrict__ parent, int32_t* __restrict__ area) {
    __shared__ int lab[CC_PIX];
    __shared__ short val[CC_PIX];
    const int t = threadIdx.x, tx0 = blockIdx.x * CC_T, ty0 = blockIdx.y * CC_T;
    const size_t base = (size_t)blockIdx.z * (size_t)H * (size_t)W;
    const int x = t & (CC_T - 1), gx = tx0 + x;
    int v[CC_PER];
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
        const int i = k * CC_THREADS + t, gy = ty0 + (i >> 5);
        const bool in = gx < W && gy < H;
        v[k] = in ? (int)masks[base + (size_t)gy * W + gx] : -1;      // outside the image: equal to nothing
        val[i] = (short)v[k];
        const int left = __shfl_up(v[k], 1, 64);
        const bool same = in && x > 0 && left == v[k];
        const u64 b = __ballot(same);
        const unsigned row = (unsigned)(b >> (threadIdx.x & 32));
        const unsigned z = ~row & (0xFFFFFFFFu >> (31 - x));            // the columns <= x that begin a run (column 0 always does)
        lab[i] = (i & ~(CC_T - 1)) + (31 - __clz((int)z));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
        const int i = k * CC_THREADS + t;
        if (v[k] >= 0 && i >= CC_T) {
            const int u = i - CC_T;
            if (val[u] == v[k]) {
                lds_unite(lab, i, u);               // what lies left and right of u hangs on u's run already
            } else if (conn == 8) {
                if (x > 0 && val[u - 1] == v[k]) lds_unite(lab, i, u - 1);
                if (x < CC_T - 1 && val[u + 1] == v[k]) lds_unite(lab, i, u + 1);
            }
        }
    }
    __syncthreads();
    int r[CC_PER];
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) r[k] = lds_find(lab, k * CC_THREADS + t);
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
        const int i = k * CC_THREADS + t, gy = ty0 + (i >> 5);
        if (v[k] >= 0) {
            const size_t g = (size_t)gy * W + gx;
            parent[base + g] = (ty0 + (r[k] >> 5)) * W + tx0 + (r[k] & (CC_T - 1));
            area[base + g] = 0;
        }
    }
}

// seams: first the rows y = 32 j (j >= 1), W pixels each, then the columns x = 32 j, H pixels each.  A row-seam pixel looks up
// (and up-left, up-right), a column-seam pixel left (and up-left, down-left): every pair of neighbours in different tiles is seen.
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const uint8_t* __restrict__ masks, int H, int W, int conn, int row_seams,
                                                              int col_seams, int32_t* parent) {
    const long long idx = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
    const long long n_row = (long long)row_seams * W, n_col = (long long)col_seams * H;
    if (idx >= n_row + n_col) return;
    const size_t base = (size_t)blockIdx.y * (size_t)H * (size_t)W;
    const uint8_t* m = masks + base;
    int* par = parent + base;
    if (idx < n_row) {
        const int y = ((int)(idx / W) + 1) * CC_T, x = (int)(idx % W);
        if (y >= H) return;
        const int p = y * W + x, v = m[p];
        if (m[p - W] == v) glb_unite(par, p, p - W);
        if (conn == 8) {
            if (x > 0 && m[p - W - 1] == v) glb_unite(par, p, p - W - 1);
            if (x < W - 1 && m[p - W + 1] == v) glb_unite(par, p, p - W + 1);
        }
    } else {
        const long long c = idx - n_row;
        const int x = ((int)(c / H) + 1) * CC_T, y = (int)(c % H);
        if (x >= W) return;
        const int p = y * W + x, v = m[p];
        if (m[p - 1] == v) glb_unite(par, p, p - 1);
        if (conn == 8) {
            if (y > 0 && m[p - W - 1] == v) glb_unite(par, p, p - W - 1);
            if (y < H - 1 && m[p + W - 1] == v) glb_unite(par, p, p + W - 1);
        }
    }
}

// A pixel counts in the LDS slot of its parent when that lies in this tile (its tile-local root, or - for a tile-local root that
// was linked to another component of the same tile - that component's root), else in its own slot: only tile-local roots are counted
// in, and every pixel counts in a slot of its own component.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const int32_t* __restrict__ parent, int H, int W, int32_t* __restrict__ root,
                                                                int32_t* area) {
    __shared__ int cnt[CC_PIX];
    __shared__ int root_of[CC_PIX];
    const int t = threadIdx.x, tx0 = blockIdx.x * CC_T, ty0 = blockIdx.y * CC_T;
    const size_t base = (size_t)blockIdx.z * (size_t)H * (size_t)W;
    const int32_t* par = parent + base;
    const int x = t & (CC_T - 1), gx = tx0 + x;
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) cnt[k * CC_THREADS + t] = 0;
    __syncthreads();
    int slot[CC_PER];
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
        const int i = k * CC_THREADS + t, gy = ty0 + (i >> 5);
        slot[k] = -1;
        if (gx < W && gy < H) {
            const int p = par[gy * W + gx];
            const int py = p / W, px = p - py * W;
            const bool here = px >= tx0 && px < tx0 + CC_T && py >= ty0 && py < ty0 + CC_T;
            slot[k] = here ? (py - ty0) * CC_T + (px - tx0) : i;
            atomicAdd(&cnt[slot[k]], 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
        const int i = k * CC_THREADS + t, c = cnt[i];
        if (c > 0) {                                // a counted slot is a pixel of the image
            int q = (ty0 + (i >> 5)) * W + gx;
            for (int p = par[q]; p != q; p = par[q]) q = p;
            root_of[i] = q;
            atomicAdd(area + base + q, c);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_PER; ++k) {
        const int i = k * CC_THREADS + t, gy = ty0 + (i >> 5);
        if (slot[k] >= 0) root[base + (size_t)gy * W + gx] = root_of[slot[k]];
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_gather_kernel(const int32_t* __restrict__ root, size_t total, int hw, int32_t* area) {
    const size_t nt = (size_t)gridDim.x * CC_THREADS;
    for (size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x; i < total; i += nt) {
        const size_t f = i / (size_t)hw;
        const int p = (int)(i - f * (size_t)hw), r = root[i];
        if (r != p) area[i] = area[f * (size_t)hw + r];          // r < p is a root: its slot is written by nobody in this launch
    }
}

// of equal areas the component with the smaller root is the larger key
__device__ __forceinline__ u64 component_key(int area, int root) { return ((u64)(unsigned)area << 32) | (u64)(~(unsigned)root); }

// the largest component of every label of a frame: one LDS atomicMax per component, one global atomicMax per (workgroup, label seen)
__global__ __launch_bounds__(CC_THREADS) void clean_best_kernel(const uint8_t* __restrict__ masks, const int32_t* __restrict__ root,
                                                                const int32_t* __restrict__ area, int hw, u64* best) {
    __shared__ u64 sbest[CC_LABELS];
    sbest[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * (size_t)hw;
    for (int p = blockIdx.x * CC_THREADS + threadIdx.x; p < hw; p += gridDim.x * CC_THREADS) {
        const int m = masks[base + p];
        if (m > 0 && root[base + p] == p) atomicMax(&sbest[m], component_key(area[base + p], p));
    }
    __syncthreads();
    const u64 b = sbest[threadIdx.x];
    if (b != 0) atomicMax(best + (size_t)blockIdx.y * CC_LABELS + threadIdx.x, b);
}

__device__ __forceinline__ void add_stats(int* sh, int32_t* stats, int a, int b, int slot) {
    // sh[2] was zeroed before the barrier that precedes the counting
    if (a) atomicAdd(&sh[0], a);
    if (b) atomicAdd(&sh[1], b);
    __syncthreads();
    if (threadIdx.x < 2 && sh[threadIdx.x] != 0) atomicAdd(stats + slot + threadIdx.x, sh[threadIdx.x]);
}

// pass A; with holes to follow, the slots of the labels around a hole are reset here
__global__ __launch_bounds__(CC_THREADS) void clean_objects_kernel(const uint8_t* __restrict__ masks, const int32_t* __restrict__ root,
                                                                   const int32_t* __restrict__ area, int hw, int min_area,
                                                                   const u64* __restrict__ best, uint8_t* __restrict__ out,
                                                                   int32_t* __restrict__ lo, int32_t* __restrict__ hi, int32_t* stats) {
    __shared__ int sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * (size_t)hw;
    int comps = 0, pixels = 0;
    for (int p = blockIdx.x * CC_THREADS + threadIdx.x; p < hw; p += gridDim.x * CC_THREADS) {
        const int m = masks[base + p];
        bool drop = false;
        if (m > 0) {
            const int r = root[base + p], a = area[base + p];
            drop = a < min_area || (best != nullptr && best[(size_t)blockIdx.y * CC_LABELS + m] != component_key(a, r));
            if (drop) { pixels += 1; comps += r == p; }
        }
        out[base + p] = drop ? (uint8_t)0 : (uint8_t)m;
        if (lo != nullptr) { lo[base + p] = CC_LABELS; hi[base + p] = 0; }
    }
    add_stats(sh, stats + (size_t)blockIdx.y * XMEM_CLEAN_STATS, comps, pixels, XMEM_CLEAN_COMPONENTS_REMOVED);
}

// pass B, first half: every pixel of a hole small enough to be filled reports the labels of its 4-neighbours, and 0 for the border
__global__ __launch_bounds__(CC_THREADS) void clean_hole_info_kernel(const uint8_t* __restrict__ out, const int32_t* __restrict__ root,
                                                                     const int32_t* __restrict__ area, int H, int W, int max_hole,
                                                                     int32_t* lo, int32_t* hi) {
    const int hw = H * W;
    const size_t base = (size_t)blockIdx.y * (size_t)hw;
    const uint8_t* o = out + base;
    for (int p = blockIdx.x * CC_THREADS + threadIdx.x; p < hw; p += gridDim.x * CC_THREADS) {
        if (o[p] != 0 || area[base + p] > max_hole) continue;
        const int y = p / W, x = p - y * W;
        int mn = CC_LABELS, mx = 0;
        if (x == 0 || y == 0 || x == W - 1 || y == H - 1) mn = 0;
        if (x > 0) { const int k = o[p - 1]; if (k) { mn = min(mn, k); mx = max(mx, k); } }
        if (x < W - 1) { const int k = o[p + 1]; if (k) { mn = min(mn, k); mx = max(mx, k); } }
        if (y > 0) { const int k = o[p - W]; if (k) { mn = min(mn, k); mx = max(mx, k); } }
        if (y < H - 1) { const int k = o[p + W]; if (k) { mn = min(mn, k); mx = max(mx, k); } }
        const int r = root[base + p];
        if (mn < CC_LABELS) atomicMin(lo + base + r, mn);
        if (mx > 0) atomicMax(hi + base + r, mx);
    }
}

// second half: min == max >= 1 says one label all around and no border
__global__ __launch_bounds__(CC_THREADS) void clean_fill_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ area,
                                                                const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int hw,
                                                                int max_hole, uint8_t* out, int32_t* stats) {
    __shared__ int sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.y * (size_t)hw;
    int holes = 0, pixels = 0;
    for (int p = blockIdx.x * CC_THREADS + threadIdx.x; p < hw; p += gridDim.x * CC_THREADS) {
        if (out[base + p] != 0 || area[base + p] > max_hole) continue;
        const int r = root[base + p];
        const int l = lo[base + r], h = hi[base + r];
        if (l == h && h >= 1) {
            out[base + p] = (uint8_t)l;
            pixels += 1;
            holes += r == p;
        }
    }
    add_stats(sh, stats + (size_t)blockIdx.y * XMEM_CLEAN_STATS, holes, pixels, XMEM_CLEAN_HOLES_FILLED);
}

int check_geometry(int N, int H, int W) {
    if (N < 1 || N > CC_MAX_N) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > CC_MAX_SIDE || W > CC_MAX_SIDE) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

size_t plane_bytes(int N, int H, int W) { return align_up((size_t)N * (size_t)H * (size_t)W * sizeof(int32_t), (size_t)256); }
size_t best_bytes(int N) { return (size_t)N * CC_LABELS * sizeof(u64); }      // a multiple of 256

unsigned frame_blocks(int hw) {
    const int b = cdiv(hw, CC_THREADS * 4);
    return (unsigned)(b < 1 ? 1 : (b > CC_EW_BLOCKS ? CC_EW_BLOCKS : b));
}

int label(const uint8_t* masks, int N, int H, int W, int conn, int32_t* root, int32_t* area, int32_t* parent, hipStream_t stream) {
    const int tiles_x = cdiv(W, CC_T), tiles_y = cdiv(H, CC_T);
    const dim3 tiles((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)N);
    hipLaunchKernelGGL(cc_local_kernel, tiles, dim3(CC_THREADS), 0, stream, masks, H, W, conn, parent, area);
    int rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    const long long seam = (long long)(tiles_y - 1) * W + (long long)(tiles_x - 1) * H;
    if (seam > 0) {
        hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)((seam + CC_THREADS - 1) / CC_THREADS), (unsigned)N), dim3(CC_THREADS), 0, stream,
                           masks, H, W, conn, tiles_y - 1, tiles_x - 1, parent);
        rc = xmem_check_launch();
        if (rc != XMEM_OK) return rc;
    }
    hipLaunchKernelGGL(cc_flatten_kernel, tiles, dim3(CC_THREADS), 0, stream, parent, H, W, root, area);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    const size_t total = (size_t)N * (size_t)H * (size_t)W;
    size_t blocks = (total + (size_t)CC_THREADS * 4 - 1) / ((size_t)CC_THREADS * 4);
    if (blocks > CC_EW_BLOCKS) blocks = CC_EW_BLOCKS;
    hipLaunchKernelGGL(cc_gather_kernel, dim3((unsigned)blocks), dim3(CC_THREADS), 0, stream, root, total, H * W, area);
    return xmem_check_launch();
}

}  // namespace

extern "C" size_t xmem_components_workspace_bytes(int N, int H, int W) {
    return check_geometry(N, H, W) == XMEM_OK ? plane_bytes(N, H, W) : 0;
}

extern "C" int xmem_components(const uint8_t* masks, int N, int H, int W, int connectivity, int32_t* root, int32_t* area, void* workspace,
                               size_t workspace_bytes, void* stream) {
    const int rc = check_geometry(N, H, W);
    if (rc != XMEM_OK) return rc;
    if (connectivity != 4 && connectivity != 8) return XMEM_ERR_BAD_ARG;
    if (!masks || !root || !area || !workspace || ((uintptr_t)workspace & 7)) return XMEM_ERR_BAD_ARG;
    if (((uintptr_t)root & 3) || ((uintptr_t)area & 3)) return XMEM_ERR_BAD_ARG;
    if (workspace_bytes < plane_bytes(N, H, W)) return XMEM_ERR_WORKSPACE;
    return label(masks, N, H, W, connectivity, root, area, (int32_t*)workspace, (hipStream_t)stream);
}

extern "C" size_t xmem_mask_clean_workspace_bytes(int N, int H, int W) {
    return check_geometry(N, H, W) == XMEM_OK ? best_bytes(N) + 5 * plane_bytes(N, H, W) : 0;
}

extern "C" int xmem_mask_clean(const uint8_t* masks, int N, int H, int W, int min_area, int max_hole, int keep_largest, uint8_t* out,
                               int32_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_geometry(N, H, W);
    if (rc != XMEM_OK) return rc;
    if (min_area < 0 || max_hole < 0) return XMEM_ERR_BAD_ARG;
    if (!masks || !out || !stats || !workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)stats & 3)) return XMEM_ERR_BAD_ARG;
    const size_t frames = (size_t)N * (size_t)H * (size_t)W;
    const uintptr_t a = (uintptr_t)masks, b = (uintptr_t)out;
    if (a < b + frames && b < a + frames) return XMEM_ERR_BAD_ARG;
    const size_t plane = plane_bytes(N, H, W);
    if (workspace_bytes < best_bytes(N) + 5 * plane) return XMEM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    u64* best = (u64*)w;
    int32_t* parent = (int32_t*)(w + best_bytes(N));
    int32_t* root = (int32_t*)(w + best_bytes(N) + plane);
    int32_t* area = (int32_t*)(w + best_bytes(N) + 2 * plane);
    int32_t* lo = max_hole > 0 ? (int32_t*)(w + best_bytes(N) + 3 * plane) : nullptr;
    int32_t* hi = max_hole > 0 ? (int32_t*)(w + best_bytes(N) + 4 * plane) : nullptr;
    const int hw = H * W;
    const dim3 grid(frame_blocks(hw), (unsigned)N);

    if (hipMemsetAsync(stats, 0, (size_t)N * XMEM_CLEAN_STATS * sizeof(int32_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    rc = label(masks, N, H, W, 8, root, area, parent, s);
    if (rc != XMEM_OK) return rc;
    if (keep_largest) {
        if (hipMemsetAsync(best, 0, best_bytes(N), s) != hipSuccess) return XMEM_ERR_LAUNCH;
        hipLaunchKernelGGL(clean_best_kernel, grid, dim3(CC_THREADS), 0, s, masks, root, area, hw, best);
        rc = xmem_check_launch();
        if (rc != XMEM_OK) return rc;
    }
    hipLaunchKernelGGL(clean_objects_kernel, grid, dim3(CC_THREADS), 0, s, masks, root, area, hw, min_area,
                       keep_largest ? (const u64*)best : (const u64*)nullptr, out, lo, hi, stats);
    rc = xmem_check_launch();
    if (rc != XMEM_OK || max_hole == 0) return rc;
    rc = label(out, N, H, W, 4, root, area, parent, s);
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(clean_hole_info_kernel, grid, dim3(CC_THREADS), 0, s, out, root, area, H, W, max_hole, lo, hi);
    rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(clean_fill_kernel, grid, dim3(CC_THREADS), 0, s, root, area, lo, hi, hw, max_hole, out, stats);
    return xmem_check_launch();
}
