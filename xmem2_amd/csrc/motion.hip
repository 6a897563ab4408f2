// 8-bit luma, an exhaustive integer block-motion search and the motion-compensated majority vote (include/xmem_hip_motion.h;
// xmem2_amd/motion.py and temporal.py have the definitions the bytes are held to).
//
//   search   one workgroup per 16 x 16 block of `cur` and pair.  The block (cropped to the image, the rest zero) and the window of
//            `ref` round it - 16 + 2 S rows, columns from x0 - S rounded down to a dword - are staged in LDS, at most 7 KB, by dword
//            loads where the four bytes lie in the image and the two aligned dwords round them in the buffer, else by bytes; what
//            lies outside the image is zero and is never part of a candidate.  The in-bounds candidates of a block are a
//            rectangle dy_lo..dy_hi x dx_lo..dx_hi, the same for every thread, dealt over the threads dx first: neighbouring lanes
//            read neighbouring bytes of one LDS row, mostly the same dwords.  A candidate's row is four dwords assembled from five
//            aligned ones (v_alignbyte_b32) and summed against the block's row with v_sad_u8; the columns a cropped block does
//            not have are masked out of `ref` and are zero in `cur`.  A thread keeps the minimum of the 64-bit key
//            SAD << 32 | d^2 << 16 | (dy + 32) << 8 | (dx + 32); the workgroup's minimum is a wave reduction and four keys in LDS.
//            A minimum depends on no order: no atomics.  The candidate (0, 0) leaves its SAD in LDS for the zero bias.
//   window   the same device function, blockIdx.y the output frame and blockIdx.z the neighbour; a pair that does not exist writes
//            sad = -1 and returns before it touches a frame.
//   vote     a thread owns four horizontally adjacent pixels, x a multiple of four: they share a block, so one vector and one
//            verdict per neighbour.  The displaced dword of each neighbour is gathered with the two-dword funnel shift and the
//            vote is temporal.hip's (vote_bytes.hpp) with the abstaining entries masked.  Changed bytes are summed per wave, then
//            per workgroup in LDS, then added once to `changed`.
//
// No float, no scratch.  The integer adds into `changed` are the only atomics: the same input gives the same bytes.
#include "common.hpp"
#include "vote_bytes.hpp"                   // load_bytes4, store_bytes4, eq_bytes, vote_group
#include "../../include/xmem_hip_motion.h"
#include "../../include/xmem_hip_temporal.h"                             // the flag bits and the largest radius

#define MO_B XMEM_MOTION_BLOCK
#define MO_MAX_S XMEM_MOTION_MAX_SEARCH
#define MO_THREADS 256
#define MO_WAVES (MO_THREADS / XMEM_WAVE)
#define MO_MAX_HW 16384
#define MO_MAX_T 65535
#define MO_MAX_STRIDE (MO_MAX_S / 2 + 5)                                 // dwords of a window row: 16 + 2 S bytes, S rounded up to 4, one spare
#define MO_MAX_ROWS (MO_B + 2 * MO_MAX_S)

static_assert(MO_B == 16, "the kernels are written for 16 x 16 blocks");

namespace {

__device__ __forceinline__ int clamp4(int v) { return v < 0 ? 0 : v > 4 ? 4 : v; }

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

// the search of block (by, bx) of `cur` in `ref`, both [H][W], by the whole workgroup; thread 0 writes vec[0], vec[1] and sad[0]
__device__ __forceinline__ void search_block(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ ref, int H, int W, int by, int bx,
                                             int S, int bias, int8_t* __restrict__ vec, int32_t* __restrict__ sad) {
    __shared__ uint32_t s_cur[MO_B * 4];
    __shared__ uint32_t s_ref[MO_MAX_ROWS * MO_MAX_STRIDE];
    __shared__ unsigned long long s_key[MO_WAVES];
    __shared__ int s_zero;
    const int tid = (int)threadIdx.x;
    const int y0 = by * MO_B, x0 = bx * MO_B;
    const int bh = min(MO_B, H - y0), bw = min(MO_B, W - x0);
    const int sal = (S + 3) & ~3, stride = sal / 2 + 5, rows = MO_B + 2 * S;
    const size_t hw = (size_t)H * W;

    if (tid < MO_B * 4) {
        const int r = tid >> 2, k = tid & 3, nv = clamp4(bw - 4 * k);
        s_cur[tid] = (r < bh && nv > 0) ? load_bytes4(cur + (size_t)(y0 + r) * W + x0 + 4 * k, nv, cur, cur + hw) : 0u;
    }
    for (int i = tid; i < rows * stride; i += MO_THREADS) {
        const int r = i / stride, c = i - r * stride;
        const int y = y0 - S + r, x = x0 - sal + 4 * c;
        uint32_t v = 0;
        if (y >= 0 && y < H && x + 4 > 0 && x < W) {
            const uint8_t* a = ref + (size_t)y * W;
            if (x >= 0 && x + 4 <= W) {
                v = load_bytes4(a + x, 4, ref, ref + hw);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k >= 0 && x + k < W) v |= (uint32_t)a[x + k] << (8 * k);
            }
        }
        s_ref[i] = v;
    }
    __syncthreads();

    // the candidates whose displaced block lies inside the image: a rectangle, the same for every thread
    const int dy_lo = max(-S, -y0), dy_hi = min(S, H - (y0 + bh));
    const int dx_lo = max(-S, -x0), dx_hi = min(S, W - (x0 + bw));
    const int ndx = dx_hi - dx_lo + 1, nc = (dy_hi - dy_lo + 1) * ndx;
    uint32_t colmask[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int nv = clamp4(bw - 4 * k);
        colmask[k] = nv == 4 ? 0xffffffffu : (1u << (8 * nv)) - 1u;
    }
    unsigned long long best = ~0ull;
    for (int c = tid; c < nc; c += MO_THREADS) {
        const int q = c / ndx;
        const int dy = dy_lo + q, dx = dx_lo + (c - q * ndx);
        const int off = sal + dx;                                        // byte column of the displaced block in the window, >= 0
        const unsigned sh = (unsigned)off & 3u;
        const uint32_t* row = s_ref + (S + dy) * stride + (off >> 2);
        const uint32_t* blk = s_cur;
        uint32_t acc = 0;
        for (int r = 0; r < bh; ++r, row += stride, blk += 4) {
            const uint32_t d0 = row[0], d1 = row[1], d2 = row[2], d3 = row[3], d4 = row[4];
            acc = __builtin_amdgcn_sad_u8(blk[0], __builtin_amdgcn_alignbyte(d1, d0, sh) & colmask[0], acc);
            acc = __builtin_amdgcn_sad_u8(blk[1], __builtin_amdgcn_alignbyte(d2, d1, sh) & colmask[1], acc);
            acc = __builtin_amdgcn_sad_u8(blk[2], __builtin_amdgcn_alignbyte(d3, d2, sh) & colmask[2], acc);
            acc = __builtin_amdgcn_sad_u8(blk[3], __builtin_amdgcn_alignbyte(d4, d3, sh) & colmask[3], acc);
        }
        if (dy == 0 && dx == 0) s_zero = (int)acc;
        const unsigned long long key = ((unsigned long long)acc << 32) | ((unsigned)(dy * dy + dx * dx) << 16) | ((unsigned)(dy + 32) << 8)
                                       | (unsigned)(dx + 32);
        best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    if ((tid & (XMEM_WAVE - 1)) == 0) s_key[tid / XMEM_WAVE] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < MO_WAVES; ++w) best = s_key[w] < best ? s_key[w] : best;
        const int won = (int)(best >> 32), zero = s_zero;
        const bool still = zero - won <= bias * bh * bw;
        vec[0] = still ? (int8_t)0 : (int8_t)((int)((best >> 8) & 0xff) - 32);
        vec[1] = still ? (int8_t)0 : (int8_t)((int)(best & 0xff) - 32);
        sad[0] = still ? zero : won;
    }
}

__global__ __launch_bounds__(MO_THREADS) void block_motion_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ ref, int H,
                                                                  int W, int Bx, int S, int bias, int8_t* __restrict__ vec,
                                                                  int32_t* __restrict__ sad) {
    const int blk = (int)blockIdx.x, by = blk / Bx, bx = blk - by * Bx;
    const size_t pair = blockIdx.y, hw = (size_t)H * W, at = pair * gridDim.x + blk;
    search_block(cur + pair * hw, ref + pair * hw, H, W, by, bx, S, bias, vec + 2 * at, sad + at);
}

__global__ __launch_bounds__(MO_THREADS) void motion_window_kernel(const uint8_t* __restrict__ luma, int ring, int H, int W, int Bx, int T,
                                                                   int t0, int radius, const uint8_t* __restrict__ flags, int S, int bias,
                                                                   int8_t* __restrict__ vec, int32_t* __restrict__ sad) {
    const int blk = (int)blockIdx.x, by = blk / Bx, bx = blk - by * Bx;
    const int e = (int)blockIdx.z, j = e < radius ? e - radius : e - radius + 1;
    const int t = t0 + (int)blockIdx.y, f = t + j;
    const size_t hw = (size_t)H * W, at = ((size_t)blockIdx.y * gridDim.z + e) * gridDim.x + blk;
    // the same verdict for the whole workgroup, before it reads a frame
    const bool pair = f >= 0 && f < T && (flags[t] & (XMEM_TEMPORAL_PRESENT | XMEM_TEMPORAL_LOCKED)) == XMEM_TEMPORAL_PRESENT
                      && (flags[f] & XMEM_TEMPORAL_PRESENT);
    if (!pair) {
        if (threadIdx.x == 0) {
            vec[2 * at] = 0;
            vec[2 * at + 1] = 0;
            sad[at] = -1;
        }
        return;
    }
    search_block(luma + (size_t)(t % ring) * hw, luma + (size_t)(f % ring) * hw, H, W, by, bx, S, bias, vec + 2 * at, sad + at);
}

__global__ __launch_bounds__(MO_THREADS) void luma_kernel(const uint8_t* __restrict__ rgb, int hw, uint8_t* __restrict__ out) {
    const int p = (int)(blockIdx.x * MO_THREADS + threadIdx.x);
    if (p >= hw) return;
    const size_t at = (size_t)blockIdx.y * hw + p;
    const uint8_t* s = rgb + at * 3;
    out[at] = (uint8_t)((77u * s[0] + 150u * s[1] + 29u * s[2] + 128u) >> 8);
}

template <int R>
__global__ __launch_bounds__(MO_THREADS) void mode_mc_kernel(const uint8_t* __restrict__ frames, int ring, int H, int W, int T, int t0,
                                                             const uint8_t* __restrict__ flags, const int8_t* __restrict__ vec,
                                                             const int32_t* __restrict__ sad, int max_sad, uint8_t* __restrict__ out,
                                                             int32_t* __restrict__ changed) {
    constexpr int N = 2 * R + 1;
    const int G = (W + 3) / 4, Bx = (W + MO_B - 1) / MO_B, By = (H + MO_B - 1) / MO_B;
    const int g = (int)(blockIdx.x * MO_THREADS + threadIdx.x);
    const int i = (int)blockIdx.y, t = t0 + i;
    const size_t hw = (size_t)H * W;
    const uint8_t* const lo = frames;
    const uint8_t* const hi = frames + (size_t)ring * hw;
    __shared__ int block_changed;
    if (threadIdx.x == 0) block_changed = 0;
    __syncthreads();
    uint32_t c = 0, o = 0;
    if (g < H * G) {                                                     // every lane stays to the end (the wave sums below)
        const int y = g / G, x = (g - y * G) * 4, nv = min(4, W - x);
        c = o = load_bytes4(frames + (size_t)(t % ring) * hw + (size_t)y * W + x, nv, lo, hi);
        if ((flags[t] & (XMEM_TEMPORAL_PRESENT | XMEM_TEMPORAL_LOCKED)) == XMEM_TEMPORAL_PRESENT) {
            const int by = y / MO_B, bx = x / MO_B;
            const int limit = max_sad * min(MO_B, H - by * MO_B) * min(MO_B, W - bx * MO_B);
            uint32_t w[N], vote[N], differs = 0;
            w[R] = c;
            vote[R] = 0x01010101u;
#pragma unroll
            for (int e = 0; e < 2 * R; ++e) {
                const int j = e < R ? e - R : e - R + 1, k = j + R, f = t + j;
                const size_t at = (((size_t)i * (2 * R) + e) * By + by) * Bx + bx;
                const int s = sad[at];
                w[k] = 0;
                vote[k] = 0;
                if (s >= 0 && s <= limit && f >= 0 && f < T) {
                    const int yy = y + vec[2 * at], xx = x + vec[2 * at + 1];
                    if (yy >= 0 && yy < H && xx >= 0 && xx + nv <= W) {  // always so for a vector of the search
                        w[k] = load_bytes4(frames + (size_t)(f % ring) * hw + (size_t)yy * W + xx, nv, lo, hi);
                        vote[k] = 0x01010101u;
                        differs |= w[k] ^ c;
                    }
                }
            }
            if (differs) o = vote_group<R>(w, vote);
        }
        store_bytes4(out + (size_t)i * hw + (size_t)y * W + x, o, nv);
    }
    int d = __popc(~eq_bytes(o, c) & 0x01010101u);
    if (__any(d)) {
        d = wave_sum_i(d);
        if ((threadIdx.x & (XMEM_WAVE - 1)) == 0) atomicAdd(&block_changed, d);
    }
    __syncthreads();
    if (threadIdx.x == 0 && block_changed) atomicAdd(changed + i, block_changed);
}

template <int R>
void launch_mc(const uint8_t* frames, int ring, int H, int W, int T, int t0, int n, const uint8_t* flags, const int8_t* vec,
               const int32_t* sad, int max_sad, uint8_t* out, int32_t* changed, hipStream_t s) {
    const dim3 grid((unsigned)cdiv(H * cdiv(W, 4), MO_THREADS), (unsigned)n);
    hipLaunchKernelGGL(mode_mc_kernel<R>, grid, dim3(MO_THREADS), 0, s, frames, ring, H, W, T, t0, flags, vec, sad, max_sad, out, changed);
}

int check_search(int H, int W, int search, int bias) {
    if (search < 1 || search > MO_MAX_S || bias < 0 || bias > 255) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > MO_MAX_HW || W > MO_MAX_HW) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

// the checks of xmem_temporal_mode on the window of a ring
int check_window(int ring, int H, int W, int T, int t0, int n, int radius) {
    if (radius < 1 || radius > XMEM_TEMPORAL_MAX_R || ring < 1) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > MO_MAX_HW || W > MO_MAX_HW || T < 1 || T > MO_MAX_T) return XMEM_ERR_UNSUPPORTED;
    if (n < 1 || t0 < 0 || t0 > T - n) return XMEM_ERR_BAD_ARG;
    const int first = t0 - radius > 0 ? t0 - radius : 0, last = t0 + n - 1 + radius < T - 1 ? t0 + n - 1 + radius : T - 1;
    if (ring < last - first + 1) return XMEM_ERR_BAD_ARG;                // two frames the call reads would share a slot
    return XMEM_OK;
}

}  // namespace

extern "C" int xmem_luma_u8(const uint8_t* rgb, int N, int H, int W, uint8_t* out, void* stream) {
    if (!rgb || !out || N < 1) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > MO_MAX_HW || W > MO_MAX_HW || N > XMEM_MOTION_MAX_N) return XMEM_ERR_UNSUPPORTED;
    const int hw = H * W;
    hipLaunchKernelGGL(luma_kernel, dim3((unsigned)cdiv(hw, MO_THREADS), (unsigned)N), dim3(MO_THREADS), 0, (hipStream_t)stream, rgb, hw, out);
    return xmem_check_launch();
}

extern "C" int xmem_block_motion(const uint8_t* cur, const uint8_t* ref, int N, int H, int W, int search, int bias, int8_t* vec,
                                 int32_t* sad, void* stream) {
    if (!cur || !ref || !vec || !sad || ((uintptr_t)sad & 3) || N < 1) return XMEM_ERR_BAD_ARG;
    if (const int bad = check_search(H, W, search, bias)) return bad;
    if (N > XMEM_MOTION_MAX_N) return XMEM_ERR_UNSUPPORTED;
    const int Bx = cdiv(W, MO_B), By = cdiv(H, MO_B);
    hipLaunchKernelGGL(block_motion_kernel, dim3((unsigned)(Bx * By), (unsigned)N), dim3(MO_THREADS), 0, (hipStream_t)stream, cur, ref, H, W,
                       Bx, search, bias, vec, sad);
    return xmem_check_launch();
}

extern "C" int xmem_motion_window(const uint8_t* luma, int ring, int H, int W, int T, int t0, int n, int radius, const uint8_t* flags,
                                  int search, int bias, int8_t* vec, int32_t* sad, void* stream) {
    if (!luma || !flags || !vec || !sad || ((uintptr_t)sad & 3)) return XMEM_ERR_BAD_ARG;
    if (const int bad = check_search(H, W, search, bias)) return bad;
    if (const int bad = check_window(ring, H, W, T, t0, n, radius)) return bad;
    const int Bx = cdiv(W, MO_B), By = cdiv(H, MO_B);
    hipLaunchKernelGGL(motion_window_kernel, dim3((unsigned)(Bx * By), (unsigned)n, (unsigned)(2 * radius)), dim3(MO_THREADS), 0,
                       (hipStream_t)stream, luma, ring, H, W, Bx, T, t0, radius, flags, search, bias, vec, sad);
    return xmem_check_launch();
}

extern "C" int xmem_temporal_mode_mc(const uint8_t* frames, int ring, int H, int W, int T, int t0, int n, int radius, const uint8_t* flags,
                                     const int8_t* vec, const int32_t* sad, int max_sad, uint8_t* out, int32_t* changed, void* stream) {
    if (!frames || !flags || !vec || !sad || !out || !changed || ((uintptr_t)changed & 3) || ((uintptr_t)sad & 3)) return XMEM_ERR_BAD_ARG;
    if (max_sad < 0 || max_sad > 255) return XMEM_ERR_BAD_ARG;
    if (const int bad = check_window(ring, H, W, T, t0, n, radius)) return bad;
    const size_t hw = (size_t)H * (size_t)W;
    const uintptr_t a = (uintptr_t)frames, b = (uintptr_t)out;
    if (a < b + (size_t)n * hw && b < a + (size_t)ring * hw) return XMEM_ERR_BAD_ARG;
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(changed, 0, (size_t)n * sizeof(int32_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    switch (radius) {
#define MO_CASE(R) case R: launch_mc<R>(frames, ring, H, W, T, t0, n, flags, vec, sad, max_sad, out, changed, s); break;
        MO_CASE(1) MO_CASE(2) MO_CASE(3) MO_CASE(4) MO_CASE(5) MO_CASE(6) MO_CASE(7)
#undef MO_CASE
    }
    return xmem_check_launch();
}
