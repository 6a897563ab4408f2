// Feathered mattes, trimaps, grow and shrink of uint8 index masks from a capped, signed, per-label squared distance in integer
// arithmetic (include/xmem_hip_matte.h; xmem2_amd/matte.py has the definitions the bytes are held to).  The separable form of
// edt.hip without its ring of zeros - nothing exists outside the image - and with a cap that bounds both passes:
//
//   column pass  c(y, x) = the distance, capped at cap = R + 1, to the nearest pixel of column x whose CLASS differs from that of
//                (y, x).  The class is `m == k` for the distance of label k and the value m itself for shrink, where it is the
//                distance to the end of the pixel's vertical run and depends on no label.  A thread owns a segment of MT_SEG rows
//                of one column: it looks at most R rows above its segment for the state to start from, walks down, looks at most
//                R rows below, walks back up and keeps the minimum.  One byte per pixel.
//   row pass     one workgroup per row with the squares in LDS, signed by the class.  A pixel searches outwards from its column:
//                a column of the OTHER class costs dx^2, a column of its own class dx^2 + c^2, and the search stops once dx^2 is
//                no better than the best found - after R columns at the latest, since the best starts at c(y, x)^2 <= cap^2.
//
// Grow carries the key `distance << 8 | label` of the nearest object pixel through both passes, so that the minimum is the
// lexicographic one.  No float, no atomics: the same input gives the same bytes.
#include "common.hpp"
#include "../../include/xmem_hip_matte.h"

#define MT_MAX_HW 16384
#define MT_COLS 64         // column pass: columns per workgroup ...
#define MT_SEGS 4          // ... times row segments per workgroup: 256 threads
#define MT_SEG 32          // rows per segment
#define MT_THREADS 256
#define MT_MAX_BLOCKS (1 << 20)
#define MT_NONE 0xFFFFu    // grow: no object pixel within reach in this column

namespace {

// ---- column pass of the distances and of shrink -------------------------------------------------------------------------------------
// planes = N * K with K >= 1: plane p is frame p / K, label p % K + 1, class `m == label`; K == 0: plane p is frame p, class m.
__global__ __launch_bounds__(MT_THREADS) void matte_cols_kernel(const uint8_t* __restrict__ masks, long long planes, int K, int H, int W,
                                                                int cap, uint8_t* __restrict__ col) {
    const int x = blockIdx.x * MT_COLS + threadIdx.x;
    const int y0 = (blockIdx.y * MT_SEGS + threadIdx.y) * MT_SEG;
    if (x >= W || y0 >= H) return;
    const int y1 = min(y0 + MT_SEG, H);
    const size_t hw = (size_t)H * W;
    for (long long p = blockIdx.z; p < planes; p += gridDim.z) {
        const int k = K ? (int)(p % K) + 1 : 0;
        const uint8_t* m = masks + (size_t)(K ? p / K : p) * hw + x;
        uint8_t* o = col + (size_t)p * hw + x;
#define MT_CLASS(v) (K ? (int)((v) == k) : (int)(v))
        int prev = MT_CLASS(m[(size_t)y0 * W]);
        int u = cap;
        for (int d = 1; d < cap && y0 - d >= 0; ++d)
            if (MT_CLASS(m[(size_t)(y0 - d) * W]) != prev) { u = d; break; }
        o[(size_t)y0 * W] = (uint8_t)u;
        for (int y = y0 + 1; y < y1; ++y) {
            const int v = MT_CLASS(m[(size_t)y * W]);
            u = v != prev ? 1 : min(u + 1, cap);
            prev = v;
            o[(size_t)y * W] = (uint8_t)u;
        }
        int dn = cap;                                       // prev is the class of row y1 - 1
        for (int d = 1; d < cap && y1 - 1 + d < H; ++d)
            if (MT_CLASS(m[(size_t)(y1 - 1 + d) * W]) != prev) { dn = d; break; }
        o[(size_t)(y1 - 1) * W] = (uint8_t)min((int)o[(size_t)(y1 - 1) * W], dn);
        for (int y = y1 - 2; y >= y0; --y) {
            const int v = MT_CLASS(m[(size_t)y * W]);
            dn = v != prev ? 1 : min(dn + 1, cap);
            prev = v;
            o[(size_t)y * W] = (uint8_t)min((int)o[(size_t)y * W], dn);
        }
#undef MT_CLASS
    }
}

// ---- row pass of the distances: int32 planes, or T look-ups ---------------------------------------------------------------------------
// rows = N * K * H.  s_v[x] = +c^2 where the pixel carries the label, -c^2 elsewhere; c >= 1, so the sign is the class.
template <bool TABLES>
__global__ __launch_bounds__(MT_THREADS) void matte_rows_kernel(const uint8_t* __restrict__ masks, const uint8_t* __restrict__ col,
                                                                long long rows, int K, int H, int W, int cap2,
                                                                const uint8_t* __restrict__ tables, int T, size_t table_stride,
                                                                int32_t* __restrict__ d2, uint8_t* __restrict__ out) {
    extern __shared__ __align__(16) int16_t s_v[];
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int y = (int)(r % H);
        const long long p = r / H;
        const int k = (int)(p % K) + 1;
        const uint8_t* mrow = masks + ((size_t)(p / K) * H + y) * W;
        const uint8_t* crow = col + (size_t)r * W;
        for (int x = threadIdx.x; x < W; x += MT_THREADS) {
            const int c = crow[x];
            s_v[x] = (int16_t)(mrow[x] == k ? c * c : -(c * c));
        }
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += MT_THREADS) {
            const int me = s_v[x];
            const bool in = me > 0;
            int best = in ? me : -me;                       // <= cap2
            for (int dx = 1; dx * dx < best; ++dx) {
                if (x - dx >= 0) {
                    const int o = s_v[x - dx];
                    best = min(best, dx * dx + ((o > 0) == in ? (o > 0 ? o : -o) : 0));
                }
                if (x + dx < W) {
                    const int o = s_v[x + dx];
                    best = min(best, dx * dx + ((o > 0) == in ? (o > 0 ? o : -o) : 0));
                }
            }
            const int s2 = in ? best : -best;
            if (TABLES) {
                for (int t = 0; t < T; ++t) out[(size_t)t * table_stride + (size_t)r * W + x] = tables[(size_t)t * (2 * cap2 + 1) + (s2 + cap2)];
            } else {
                d2[(size_t)r * W + x] = s2;
            }
        }
        __syncthreads();                                    // s_v is rewritten for the next row
    }
}

// ---- grow -----------------------------------------------------------------------------------------------------------------------------
// key [N][H][W] uint16 = dy << 8 | label of the nearest object pixel of the column within `reach` rows (of two at one distance the
// smaller label: the smaller key), MT_NONE without one.
__device__ __forceinline__ unsigned grow_step(unsigned key, int v, int reach) {
    if (v) return (unsigned)v;
    if (key == MT_NONE || (int)(key >> 8) + 1 > reach) return MT_NONE;
    return key + 256u;
}

__global__ __launch_bounds__(MT_THREADS) void grow_cols_kernel(const uint8_t* __restrict__ masks, int N, int H, int W, int reach,
                                                               uint16_t* __restrict__ key) {
    const int x = blockIdx.x * MT_COLS + threadIdx.x;
    const int y0 = (blockIdx.y * MT_SEGS + threadIdx.y) * MT_SEG;
    if (x >= W || y0 >= H) return;
    const int y1 = min(y0 + MT_SEG, H);
    const size_t hw = (size_t)H * W;
    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        const uint8_t* m = masks + (size_t)n * hw + x;
        uint16_t* o = key + (size_t)n * hw + x;
        unsigned u = MT_NONE;
        for (int d = 1; d <= reach && y0 - d >= 0; ++d) {
            const int v = m[(size_t)(y0 - d) * W];
            if (v) { u = ((unsigned)(d - 1) << 8) | (unsigned)v; break; }      // as seen from row y0 - 1
        }
        for (int y = y0; y < y1; ++y) {
            u = grow_step(u, m[(size_t)y * W], reach);
            o[(size_t)y * W] = (uint16_t)u;
        }
        unsigned dn = MT_NONE;
        for (int d = 1; d <= reach && y1 - 1 + d < H; ++d) {
            const int v = m[(size_t)(y1 - 1 + d) * W];
            if (v) { dn = ((unsigned)(d - 1) << 8) | (unsigned)v; break; }      // as seen from row y1
        }
        for (int y = y1 - 1; y >= y0; --y) {
            dn = grow_step(dn, m[(size_t)y * W], reach);
            o[(size_t)y * W] = (uint16_t)min((unsigned)o[(size_t)y * W], dn);
        }
    }
}

// best = d2 << 8 | label, the lexicographic minimum; a column at dx can only give keys above dx^2 << 8.
__global__ __launch_bounds__(MT_THREADS) void grow_rows_kernel(const uint16_t* __restrict__ key, long long rows, int W, int r2,
                                                               uint8_t* __restrict__ out) {
    extern __shared__ __align__(16) uint16_t s_key[];
    const unsigned none = (unsigned)(r2 + 1) << 8;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const uint16_t* krow = key + (size_t)r * W;
        for (int x = threadIdx.x; x < W; x += MT_THREADS) s_key[x] = krow[x];
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += MT_THREADS) {
            unsigned best = none;
            for (int dx = 0; dx * dx <= r2 && ((unsigned)(dx * dx) << 8) < best; ++dx) {
                if (x - dx >= 0) {
                    const unsigned q = s_key[x - dx];
                    if (q != MT_NONE) {
                        const unsigned g = q >> 8;
                        best = min(best, ((unsigned)(dx * dx) + g * g) << 8 | (q & 255u));
                    }
                }
                if (dx && x + dx < W) {
                    const unsigned q = s_key[x + dx];
                    if (q != MT_NONE) {
                        const unsigned g = q >> 8;
                        best = min(best, ((unsigned)(dx * dx) + g * g) << 8 | (q & 255u));
                    }
                }
            }
            out[(size_t)r * W + x] = best < none ? (uint8_t)(best & 255u) : (uint8_t)0;
        }
        __syncthreads();
    }
}

// ---- shrink: the row pass over the run plane of matte_cols_kernel (K == 0) -------------------------------------------------------------
// s_m: the row of the mask, s_run: its runs.  A pixel of label c goes when a column within reach holds another value in this row
// (dx^2 <= r2) or ends its run of c close enough (dx^2 + run^2 <= r2).
__global__ __launch_bounds__(MT_THREADS) void shrink_rows_kernel(const uint8_t* __restrict__ masks, const uint8_t* __restrict__ run,
                                                                 long long rows, int W, int r2, uint8_t* __restrict__ out) {
    extern __shared__ __align__(16) uint8_t s_b[];
    uint8_t* s_m = s_b;
    uint8_t* s_run = s_b + W;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        for (int x = threadIdx.x; x < W; x += MT_THREADS) {
            s_m[x] = masks[(size_t)r * W + x];
            s_run[x] = run[(size_t)r * W + x];
        }
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += MT_THREADS) {
            const int c = s_m[x];
            bool gone = false;
            if (c) {
                for (int dx = 0; dx * dx <= r2 && !gone; ++dx) {
                    if (x - dx >= 0) {
                        const int g = s_m[x - dx] == c ? s_run[x - dx] : 0;
                        gone = gone || dx * dx + g * g <= r2;
                    }
                    if (x + dx < W) {
                        const int g = s_m[x + dx] == c ? s_run[x + dx] : 0;
                        gone = gone || dx * dx + g * g <= r2;
                    }
                }
            }
            out[(size_t)r * W + x] = gone ? (uint8_t)0 : (uint8_t)c;
        }
        __syncthreads();
    }
}

inline int geometry(int N, int H, int W) {
    if (N < 1 || N > 65535) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > MT_MAX_HW || W > MT_MAX_HW) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

inline int labels_ok(int K, int R) {
    return K >= 1 && K <= XMEM_MATTE_MAX_LABELS && R >= 1 && R <= XMEM_MATTE_MAX_R ? XMEM_OK : XMEM_ERR_BAD_ARG;
}

inline size_t label_planes_bytes(int N, int H, int W, int K) { return align_up((size_t)N * K * H * W, (size_t)8); }

inline dim3 cols_grid(int H, int W, long long planes) {
    return dim3((unsigned)cdiv(W, MT_COLS), (unsigned)cdiv(H, MT_SEGS * MT_SEG), (unsigned)(planes < 65535 ? planes : 65535));
}

inline unsigned rows_grid(long long rows) { return (unsigned)(rows < MT_MAX_BLOCKS ? rows : MT_MAX_BLOCKS); }

inline int isqrt_floor(int v) {
    int r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// the shared body of xmem_signed_edt (d2 set) and xmem_mask_matte (tables, out set): everything was checked by the caller
int signed_distance(const uint8_t* masks, int N, int H, int W, int K, int R, const uint8_t* tables, int T, int32_t* d2, uint8_t* out,
                    uint8_t* col, hipStream_t s) {
    const long long planes = (long long)N * K, rows = planes * H;
    const int cap = R + 1;
    hipLaunchKernelGGL(matte_cols_kernel, cols_grid(H, W, planes), dim3(MT_COLS, MT_SEGS), 0, s, masks, planes, K, H, W, cap, col);
    const int rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    const size_t lds = (size_t)W * sizeof(int16_t);                // at most 32 KiB
    if (d2)
        hipLaunchKernelGGL(matte_rows_kernel<false>, dim3(rows_grid(rows)), dim3(MT_THREADS), lds, s, masks, (const uint8_t*)col, rows, K, H,
                           W, cap * cap, tables, 0, (size_t)0, d2, out);
    else
        hipLaunchKernelGGL(matte_rows_kernel<true>, dim3(rows_grid(rows)), dim3(MT_THREADS), lds, s, masks, (const uint8_t*)col, rows, K, H,
                           W, cap * cap, tables, T, (size_t)rows * W, d2, out);
    return xmem_check_launch();
}

}  // namespace

extern "C" size_t xmem_signed_edt_workspace_bytes(int N, int H, int W, int K) {
    return geometry(N, H, W) == XMEM_OK && K >= 1 && K <= XMEM_MATTE_MAX_LABELS ? label_planes_bytes(N, H, W, K) : 0;
}

extern "C" int xmem_signed_edt(const uint8_t* masks, int N, int H, int W, int K, int R, int32_t* out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    int rc = geometry(N, H, W);
    if (rc != XMEM_OK) return rc;
    if ((rc = labels_ok(K, R)) != XMEM_OK) return rc;
    if (!masks || !out || !workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)out & 3)) return XMEM_ERR_BAD_ARG;
    if (workspace_bytes < label_planes_bytes(N, H, W, K)) return XMEM_ERR_WORKSPACE;
    return signed_distance(masks, N, H, W, K, R, nullptr, 0, out, nullptr, (uint8_t*)workspace, (hipStream_t)stream);
}

extern "C" size_t xmem_mask_matte_workspace_bytes(int N, int H, int W, int K) { return xmem_signed_edt_workspace_bytes(N, H, W, K); }

extern "C" int xmem_mask_matte(const uint8_t* masks, int N, int H, int W, int K, int R, const uint8_t* tables, int T, uint8_t* out,
                               void* workspace, size_t workspace_bytes, void* stream) {
    int rc = geometry(N, H, W);
    if (rc != XMEM_OK) return rc;
    if ((rc = labels_ok(K, R)) != XMEM_OK) return rc;
    if (T < 1 || T > XMEM_MATTE_MAX_TABLES) return XMEM_ERR_BAD_ARG;
    if (!masks || !tables || !out || !workspace || ((uintptr_t)workspace & 7)) return XMEM_ERR_BAD_ARG;
    if (workspace_bytes < label_planes_bytes(N, H, W, K)) return XMEM_ERR_WORKSPACE;
    return signed_distance(masks, N, H, W, K, R, tables, T, nullptr, out, (uint8_t*)workspace, (hipStream_t)stream);
}

extern "C" size_t xmem_mask_grow_workspace_bytes(int N, int H, int W) {
    return geometry(N, H, W) == XMEM_OK ? align_up((size_t)N * H * W * sizeof(uint16_t), (size_t)8) : 0;
}

extern "C" int xmem_mask_grow(const uint8_t* masks, int N, int H, int W, int r2, int shrink, uint8_t* out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    const int rc = geometry(N, H, W);
    if (rc != XMEM_OK) return rc;
    if (r2 < 1 || r2 > XMEM_MATTE_MAX_R * XMEM_MATTE_MAX_R) return XMEM_ERR_BAD_ARG;
    if (!masks || !out || !workspace || ((uintptr_t)workspace & 7)) return XMEM_ERR_BAD_ARG;
    const size_t frames = (size_t)N * (size_t)H * (size_t)W;
    const uintptr_t a = (uintptr_t)masks, b = (uintptr_t)out;
    if (a < b + frames && b < a + frames) return XMEM_ERR_BAD_ARG;
    if (workspace_bytes < xmem_mask_grow_workspace_bytes(N, H, W)) return XMEM_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const int reach = isqrt_floor(r2);                             // rows and columns a pixel within r2 can be away
    const long long rows = (long long)N * H;
    if (shrink) {
        uint8_t* run = (uint8_t*)workspace;
        hipLaunchKernelGGL(matte_cols_kernel, cols_grid(H, W, N), dim3(MT_COLS, MT_SEGS), 0, s, masks, (long long)N, 0, H, W, reach + 1, run);
        const int rc2 = xmem_check_launch();
        if (rc2 != XMEM_OK) return rc2;
        hipLaunchKernelGGL(shrink_rows_kernel, dim3(rows_grid(rows)), dim3(MT_THREADS), (size_t)2 * W, s, masks, (const uint8_t*)run, rows, W,
                           r2, out);
        return xmem_check_launch();
    }
    uint16_t* key = (uint16_t*)workspace;
    hipLaunchKernelGGL(grow_cols_kernel, cols_grid(H, W, N), dim3(MT_COLS, MT_SEGS), 0, s, masks, N, H, W, reach, key);
    const int rc2 = xmem_check_launch();
    if (rc2 != XMEM_OK) return rc2;
    hipLaunchKernelGGL(grow_rows_kernel, dim3(rows_grid(rows)), dim3(MT_THREADS), (size_t)W * sizeof(uint16_t), s, (const uint16_t*)key, rows,
                       W, r2, out);
    return xmem_check_launch();
}
