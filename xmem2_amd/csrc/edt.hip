// The robot user of click evaluation (inference/interact/fbrs/inference/clicker.py:32-59, utils.py:103-110) in integer arithmetic:
// the error planes of a prediction against the ground truth, their exact squared Euclidean distance transform inside a ring of
// zeros, and the next click.  The reference takes sqrt in float64 and compares; sqrt is strictly monotonic on integers below 2^53, so
// comparing the squared distances and taking the smallest linear index among the maxima is the same choice, bit for bit.  No float
// arithmetic beyond `prob > threshold`, no float atomics: the same inputs give the same bits.
//
//   d2(y, x) = min( min over zero pixels (y', x') of the plane of (y - y')^2 + (x - x')^2,  min(y + 1, H - y, x + 1, W - x)^2 ),
//              0 where the plane is 0                                     (np.pad by one ring of zeros, distance_transform_edt, crop)
//
// in the separable form: a column pass g(y, x) = distance to the nearest zero of column x with the ring rows -1 and H included, then a
// row pass d2(y, x) = min over x' of (x - x')^2 + g(y, x')^2 with the ring columns -1 and W (g = 0 there) included.
#include "common.hpp"

#define EDT_MAX_HW 16384   // d2 <= 8192^2 * 2 and every intermediate below fit in int32
#define EDT_COLS 16        // column pass: columns per workgroup ...
#define EDT_SEGS 16        // ... times row segments per column: 256 threads
#define EDT_THREADS 256
#define NC_BLOCKS 256      // partial maxima of the click reduction

namespace {

// ---- error planes and IoU counts -------------------------------------------------------------------------------------------------
// pred = prob > threshold (or mask != 0); gt: 1 object, 255 ignore, anything else background.  planes [2][P]: fn = gt & ~pred,
// fp = ~gt & pred & not_ignore.  counts {inter, union} under the ignore mask: one integer atomic per workgroup and slot.
__global__ __launch_bounds__(EDT_THREADS) void click_errors_kernel(const float* __restrict__ prob, float threshold,
                                                                   const uint8_t* __restrict__ mask, const uint8_t* __restrict__ gt,
                                                                   int P, uint8_t* __restrict__ planes, int* __restrict__ counts) {
    __shared__ int s_sum[2][EDT_THREADS / XMEM_WAVE];
    int inter = 0, uni = 0;
    for (int i = blockIdx.x * EDT_THREADS + threadIdx.x; i < P; i += gridDim.x * EDT_THREADS) {
        const bool pred = prob ? prob[i] > threshold : mask[i] != 0;
        const int g = gt[i];
        const bool obj = g == 1, valid = g != 255;
        planes[i] = obj && !pred;
        planes[(size_t)P + i] = !obj && valid && pred;
        inter += pred && obj;
        uni += (pred && valid) || obj;
    }
    inter = wave_sum_i(inter);
    uni = wave_sum_i(uni);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_sum[0][wave] = inter; s_sum[1][wave] = uni; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int t = 0;
        for (int w = 0; w < EDT_THREADS / XMEM_WAVE; ++w) t += s_sum[threadIdx.x][w];
        if (t) atomicAdd(counts + threadIdx.x, t);
    }
}

// ---- column pass -----------------------------------------------------------------------------------------------------------------
// A workgroup owns EDT_COLS columns of one plane; each column is cut into EDT_SEGS row segments so that a 480-row scan is 30 rows
// deep, not 480.  A: every (column, segment) thread finds the first and the last zero row of its segment.  The nearest zero above a
// segment is then the largest `last` of the segments before it (the ring row -1 if none), the nearest below the smallest `first`
// after it (the ring row H).  B: downwards, the distance to the nearest zero above; C: upwards, the minimum with the nearest below,
// squared.  out holds g^2; the row pass turns it into d2 in place.
__global__ __launch_bounds__(EDT_THREADS) void edt_cols_kernel(const uint8_t* __restrict__ planes, int B, int H, int W,
                                                               int* __restrict__ out) {
    __shared__ int s_first[EDT_SEGS][EDT_COLS], s_last[EDT_SEGS][EDT_COLS];
    const int cx = threadIdx.x, seg = threadIdx.y;
    const int x = blockIdx.x * EDT_COLS + cx;
    const int rows = (H + EDT_SEGS - 1) / EDT_SEGS;
    const int y0 = min(seg * rows, H), y1 = min(y0 + rows, H);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const uint8_t* m = planes + (size_t)b * H * W + x;
        int* o = out + (size_t)b * H * W + x;
        int first = H, last = -1;
        if (x < W)
            for (int y = y0; y < y1; ++y)
                if (m[(size_t)y * W] == 0) {
                    if (first == H) first = y;
                    last = y;
                }
        s_first[seg][cx] = first;
        s_last[seg][cx] = last;
        __syncthreads();
        if (x < W) {
            int up = -1, dn = H;
            for (int s = 0; s < seg; ++s) up = max(up, s_last[s][cx]);
            for (int s = EDT_SEGS - 1; s > seg; --s) dn = min(dn, s_first[s][cx]);
            for (int y = y0; y < y1; ++y) {
                if (m[(size_t)y * W] == 0) up = y;
                o[(size_t)y * W] = y - up;
            }
            for (int y = y1 - 1; y >= y0; --y) {
                const int v = o[(size_t)y * W];
                if (v == 0) dn = y;
                const int d = min(v, dn - y);
                o[(size_t)y * W] = d * d;
            }
        }
        __syncthreads();                 // s_first / s_last are rewritten for the next plane
    }
}

// ---- row pass ----------------------------------------------------------------------------------------------------------------------
// One workgroup per row: g^2 of the row in LDS, one thread per pixel searching outwards from x.  With the ring columns best starts at
// min(g^2(x), (x + 1)^2, (W - x)^2), and a column at distance dx can only improve it while dx^2 < best: the search is exact, and
// dx < x + 1 and dx < W - x keep both reads inside the row.
__global__ __launch_bounds__(EDT_THREADS) void edt_rows_kernel(int* __restrict__ d2, int rows, int W) {
    extern __shared__ __align__(16) int s_g2[];
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        int* row = d2 + (size_t)r * W;
        for (int x = threadIdx.x; x < W; x += EDT_THREADS) s_g2[x] = row[x];
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += EDT_THREADS) {
            int best = s_g2[x];
            if (best > 0) {
                const int l = x + 1, rr = W - x;
                best = min(best, min(l * l, rr * rr));
                for (int dx = 1; dx * dx < best; ++dx) best = min(best, dx * dx + min(s_g2[x - dx], s_g2[x + dx]));
            }
            row[x] = best;
        }
        __syncthreads();
    }
}

// ---- the next click: max of d2 * not_clicked per plane, ties to the smallest linear index --------------------------------------------
// key = d2 << 32 | (2^32 - 1 - index): the maximum key is the maximum d2 at its smallest index (np.where(...)[0] in row-major order).
__device__ __forceinline__ unsigned long long block_max_key(unsigned long long k, unsigned long long* s_k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o, 64);
        k = other > k ? other : k;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                     // s_k may still be read from the previous plane
    if (lane == 0) s_k[wave] = k;
    __syncthreads();
    k = s_k[0];
    for (int w = 1; w < EDT_THREADS / XMEM_WAVE; ++w) k = s_k[w] > k ? s_k[w] : k;
    return k;
}

__global__ __launch_bounds__(EDT_THREADS) void next_click_partial_kernel(const int* __restrict__ d2, const uint8_t* __restrict__ not_clicked,
                                                                         int P, unsigned long long* __restrict__ part) {
    __shared__ unsigned long long s_k[EDT_THREADS / XMEM_WAVE];
    for (int plane = 0; plane < 2; ++plane) {
        unsigned long long k = 0;
        for (int i = blockIdx.x * EDT_THREADS + threadIdx.x; i < P; i += gridDim.x * EDT_THREADS) {
            const unsigned v = not_clicked[i] ? (unsigned)d2[(size_t)plane * P + i] : 0u;
            const unsigned long long c = ((unsigned long long)v << 32) | (0xFFFFFFFFu - (unsigned)i);
            k = c > k ? c : k;
        }
        k = block_max_key(k, s_k);
        if (threadIdx.x == 0) part[blockIdx.x * 2 + plane] = k;
    }
}

__global__ __launch_bounds__(EDT_THREADS) void next_click_final_kernel(const unsigned long long* __restrict__ part, int nblocks, int W,
                                                                       const int* __restrict__ counts, uint8_t* __restrict__ not_clicked,
                                                                       int* __restrict__ record) {
    __shared__ unsigned long long s_k[EDT_THREADS / XMEM_WAVE];
    unsigned long long key[2];
    for (int plane = 0; plane < 2; ++plane) {
        unsigned long long k = 0;
        for (int i = threadIdx.x; i < nblocks; i += EDT_THREADS) k = part[i * 2 + plane] > k ? part[i * 2 + plane] : k;
        key[plane] = block_max_key(k, s_k);
    }
    if (threadIdx.x == 0) {
        const int fn_max = (int)(key[0] >> 32), fp_max = (int)(key[1] >> 32);
        const int positive = fn_max > fp_max;                      // strict: a tie (0 == 0 when pred == gt included) is a negative click
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(positive ? key[0] : key[1]);
        record[0] = positive;
        record[1] = (int)(idx / (unsigned)W);
        record[2] = (int)(idx % (unsigned)W);
        record[3] = fn_max;
        record[4] = fp_max;
        record[5] = counts ? counts[0] : 0;
        record[6] = counts ? counts[1] : 0;
        record[7] = 0;
        not_clicked[idx] = 0;
    }
}

inline bool edt_size_ok(int H, int W) { return H <= EDT_MAX_HW && W <= EDT_MAX_HW; }

inline int blocks_for(int P, int cap) {
    const int g = (P + EDT_THREADS - 1) / EDT_THREADS;
    return g < cap ? g : cap;
}

}  // namespace

extern "C" int xmem_click_errors(const float* prob, float threshold, const uint8_t* mask, const uint8_t* gt, int H, int W,
                                 uint8_t* planes, int32_t* counts, void* stream) {
    if ((prob == nullptr) == (mask == nullptr) || !gt || !planes || !counts || H <= 0 || W <= 0) return XMEM_ERR_BAD_ARG;
    if (!edt_size_ok(H, W)) return XMEM_ERR_UNSUPPORTED;
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    const int P = H * W;
    hipLaunchKernelGGL(click_errors_kernel, dim3(blocks_for(P, 2048)), dim3(EDT_THREADS), 0, s, prob, threshold, mask, gt, P, planes,
                       (int*)counts);
    return xmem_check_launch();
}

extern "C" int xmem_edt_sq(const uint8_t* planes, int B, int H, int W, int32_t* d2, void* stream) {
    if (!planes || !d2 || B <= 0 || H <= 0 || W <= 0) return XMEM_ERR_BAD_ARG;
    if (!edt_size_ok(H, W) || (size_t)B * H > (size_t)INT32_MAX) return XMEM_ERR_UNSUPPORTED;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(edt_cols_kernel, dim3(cdiv(W, EDT_COLS), B < 65535 ? B : 65535), dim3(EDT_COLS, EDT_SEGS), 0, s, planes, B, H, W,
                       (int*)d2);
    int rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    const size_t lds = (size_t)W * sizeof(int);                    // at most 64 KiB
    rc = xmem_ensure_dynamic_lds(reinterpret_cast<const void*>(edt_rows_kernel), lds);
    if (rc != XMEM_OK) return rc;
    const int rows = B * H;
    hipLaunchKernelGGL(edt_rows_kernel, dim3(rows < (1 << 20) ? rows : (1 << 20)), dim3(EDT_THREADS), lds, s, (int*)d2, rows, W);
    return xmem_check_launch();
}

extern "C" size_t xmem_next_click_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0 || !edt_size_ok(H, W)) return 0;
    return (size_t)blocks_for(H * W, NC_BLOCKS) * 2 * sizeof(unsigned long long);
}

extern "C" int xmem_next_click(const int32_t* d2, uint8_t* not_clicked, const int32_t* counts, int H, int W, int32_t* record,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (!d2 || !not_clicked || !record || !workspace || H <= 0 || W <= 0) return XMEM_ERR_BAD_ARG;
    if (!edt_size_ok(H, W)) return XMEM_ERR_UNSUPPORTED;
    if (workspace_bytes < xmem_next_click_workspace_bytes(H, W) || ((uintptr_t)workspace & 7)) return XMEM_ERR_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    const int P = H * W, nb = blocks_for(P, NC_BLOCKS);
    unsigned long long* part = (unsigned long long*)workspace;
    hipLaunchKernelGGL(next_click_partial_kernel, dim3(nb), dim3(EDT_THREADS), 0, s, (const int*)d2, (const uint8_t*)not_clicked, P, part);
    int rc = xmem_check_launch();
    if (rc != XMEM_OK) return rc;
    hipLaunchKernelGGL(next_click_final_kernel, dim3(1), dim3(EDT_THREADS), 0, s, (const unsigned long long*)part, nb, W,
                       (const int*)counts, not_clicked, (int*)record);
    return xmem_check_launch();
}
