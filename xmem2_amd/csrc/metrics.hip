// DAVIS region similarity J and boundary accuracy F, as exact integer counts (util/metrics.py:10-69 batched_jaccard, :75-134
// _seg2bmap, :137-196 f_measure, :199-258 batched_f_measure).  Per frame b and object label k in 1..254, with m = (labels == k):
//   boundary  b = (m^E) | (m^S) | (m^SE), E / S / SE the right / lower / lower-right neighbour, 0 outside the image;
//             last row b = m^E, last column b = m^S, bottom-right pixel 0 (the width=None branch of _seg2bmap)
//   dilation  cv2.dilate(b, disk(r)): covered if some boundary pixel lies at (dy, dx) with dy^2 + dx^2 <= r^2, nothing outside the image
//   counts    [B][256][7] int32: gt_area, pred_area, inter, n_gt, n_pred, gt_match (gt boundary under the dilated pred boundary),
//             pred_match (pred boundary under the dilated gt boundary); the host turns them into J and F (xmem2_amd/metrics.py).
//
// One workgroup (4 waves) owns a 64 x 64 tile of one frame.  It stages both label maps (pred through the 256-entry LUT) over the tile's
// rows +-r (+1 row below) and over three 64-column words (left neighbour, tile, right neighbour; + the column after them) into LDS with
// dword loads, and collects the labels present in the tile extended by one row and one column (the only labels whose counts in this
// tile can be non-zero).  Per present label:
//   A  one wave64 ballot per (map, row, word) packs m into 64-bit words;
//   B  one thread per (map, source row) forms the boundary words, dilates them horizontally by shift-or across the neighbouring words
//      with the half-width w(dy) = floor(sqrt(r^2 - dy^2)) growing as |dy| falls, and ORs each into the output rows y - dy (LDS atomics);
//   C  wave 0, one lane per tile row, takes popcounts and reduces them; lane 0 adds each non-zero total with one global integer atomic.
// Integer sums do not depend on order: the counts are bit-reproducible.  r <= 63 keeps the dilation within one neighbour word a side.
#include "common.hpp"

#define JF_TH 64          // tile rows (wave 0 has one lane per tile row in step C)
#define JF_PITCH 196      // staged bytes per row: columns x0-64 .. x0+128 (193), rounded up to a dword
#define JF_GROUPS 49      // dwords per staged row
#define JF_THREADS 256
#define JF_MAX_R 63
#define JF_MAX_HW 16384   // counts of a 16384 x 16384 frame still fit in int32
#define JF_SLOTS 7

static __host__ __device__ inline size_t jf_stage_bytes(int r) {
    return ((size_t)2 * (JF_TH + 2 * r + 1) * JF_PITCH + 15) / 16 * 16;
}

static inline size_t jf_lds_bytes(int r) {
    const int nrows = JF_TH + 2 * r + 1;
    return jf_stage_bytes(r) + sizeof(uint64_t) * ((size_t)2 * nrows * 3 + 4 * JF_TH);
}

__device__ __forceinline__ uint64_t jf_cols_mask(int base, int W) {      // bits of columns base .. base+63 that lie in [0, W)
    const int lo = base < 0 ? -base : 0;
    const int hi = W - base < 64 ? W - base : 64;
    if (hi <= lo) return 0;
    const uint64_t upto = hi == 64 ? ~0ull : ((1ull << hi) - 1);
    return upto & (~0ull << lo);
}

__global__ __launch_bounds__(JF_THREADS) void jf_counts_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pred,
                                                               const uint8_t* __restrict__ lut, int B, int H, int W, int r,
                                                               int* __restrict__ counts) {
    extern __shared__ __align__(16) uint8_t jf_smem[];
    __shared__ uint8_t s_lut[256];
    __shared__ unsigned s_present[8];
    __shared__ int s_w[JF_MAX_R + 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nrows = JF_TH + 2 * r + 1;          // staged rows y0-r .. y0+TH+r
    const int nsrc = JF_TH + 2 * r;               // boundary rows y0-r .. y0+TH-1+r
    uint8_t* st[2] = {jf_smem, jf_smem + (size_t)nrows * JF_PITCH};
    uint64_t* M = reinterpret_cast<uint64_t*>(jf_smem + jf_stage_bytes(r));   // [2][nrows][3] object bits
    uint64_t* Bc = M + 2 * nrows * 3;                                         // [2][TH] boundary bits of the tile word
    uint64_t* D = Bc + 2 * JF_TH;                                             // [2][TH] dilated boundary bits of the tile word
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * JF_TH;

    s_lut[tid] = lut ? lut[tid] : (uint8_t)tid;                               // JF_THREADS == 256
    if (tid <= r) {
        const int n = r * r - tid * tid;
        int v = (int)sqrtf((float)n);
        while (v * v > n) --v;
        while ((v + 1) * (v + 1) <= n) ++v;
        s_w[tid] = v;
    }

    for (int b = blockIdx.z; b < B; b += gridDim.z) {
        if (tid < 8) s_present[tid] = 0;
        __syncthreads();                                                     // s_lut / s_w written; the previous frame is done
        // ---- stage both maps (pred through the LUT); 0 outside the image -------------------------------------------------
        const uint8_t* g0 = gt + (size_t)b * H * W;
        const uint8_t* p0 = pred + (size_t)b * H * W;
        for (int idx = tid; idx < nrows * JF_GROUPS; idx += JF_THREADS) {
            const int j = idx / JF_GROUPS, g = idx - j * JF_GROUPS;
            const int y = y0 - r + j, x = x0 - 64 + 4 * g;
            uint32_t vg = 0, vp = 0;
            if (y >= 0 && y < H) {
                const uint8_t* rg = g0 + (size_t)y * W;
                const uint8_t* rp = p0 + (size_t)y * W;
                if (x >= 0 && x + 3 < W && ((((uintptr_t)(rg + x)) | ((uintptr_t)(rp + x))) & 3) == 0) {
                    vg = *reinterpret_cast<const uint32_t*>(rg + x);
                    vp = *reinterpret_cast<const uint32_t*>(rp + x);
                } else {
                    for (int q = 0; q < 4; ++q) {
                        const int xx = x + q;
                        if (xx >= 0 && xx < W) {
                            vg |= (uint32_t)rg[xx] << (8 * q);
                            vp |= (uint32_t)rp[xx] << (8 * q);
                        }
                    }
                }
                uint32_t m = 0;
                for (int q = 0; q < 4; ++q) {
                    const int xx = x + q;
                    if (xx >= 0 && xx < W) m |= (uint32_t)s_lut[(vp >> (8 * q)) & 255] << (8 * q);
                }
                vp = m;
            }
            *reinterpret_cast<uint32_t*>(st[0] + (size_t)j * JF_PITCH + 4 * g) = vg;
            *reinterpret_cast<uint32_t*>(st[1] + (size_t)j * JF_PITCH + 4 * g) = vp;
        }
        __syncthreads();
        // ---- labels present in the tile + one row and one column (LDS bitmap) ----------------------------------------------
        {
            int prev = 0;
            for (int idx = tid; idx < (JF_TH + 1) * 65 * 2; idx += JF_THREADS) {
                const int map = idx >= (JF_TH + 1) * 65;
                const int e = idx - map * (JF_TH + 1) * 65;
                const int j = r + e / 65, c = 64 + e % 65;
                const int v = st[map][(size_t)j * JF_PITCH + c];
                if (v != prev && v != 0 && v != 255) atomicOr(&s_present[v >> 5], 1u << (v & 31));
                prev = v;
            }
        }
        __syncthreads();
        unsigned present[8];
        for (int i = 0; i < 8; ++i) present[i] = s_present[i];

        for (int wi = 0; wi < 8; ++wi) {
            while (present[wi]) {
                const int k = wi * 32 + __builtin_ctz(present[wi]);
                present[wi] &= present[wi] - 1;
                // ---- A: object bits, one ballot per (map, row, word) --------------------------------------------------------
                for (int it = wave; it < 2 * nrows * 3; it += JF_THREADS / 64) {
                    const int map = it >= nrows * 3;
                    const int rem = it - map * nrows * 3;
                    const int j = rem / 3, wd = rem - j * 3;
                    const uint64_t bits = __ballot(st[map][(size_t)j * JF_PITCH + wd * 64 + lane] == k);
                    if (lane == 0) M[it] = bits;
                }
                if (tid < 2 * JF_TH) D[tid] = 0;
                __syncthreads();
                // ---- B: boundary words, horizontal dilation, OR into the output rows ----------------------------------------
                for (int it = tid; it < 2 * nsrc; it += JF_THREADS) {
                    const int map = it >= nsrc;
                    const int j = it - map * nsrc;
                    const int s = y0 - r + j;
                    const bool in_tile = j >= r && j < r + JF_TH;
                    if (s < 0 || s >= H) {
                        if (in_tile) Bc[map * JF_TH + j - r] = 0;
                        continue;
                    }
                    const uint64_t* m = M + (size_t)map * nrows * 3 + j * 3;
                    const uint64_t* sv = m + 3;                                  // row s+1 (staged as 0 below the image)
                    const uint64_t e_m = st[map][(size_t)j * JF_PITCH + 192] == k;
                    const uint64_t e_s = st[map][(size_t)(j + 1) * JF_PITCH + 192] == k;
                    const bool last = s == H - 1;
                    uint64_t bw[3];
                    for (int wd = 0; wd < 3; ++wd) {
                        const uint64_t mw = m[wd], sw = sv[wd];
                        const uint64_t E = (mw >> 1) | ((wd < 2 ? (m[wd + 1] & 1) : e_m) << 63);
                        const uint64_t SE = (sw >> 1) | ((wd < 2 ? (sv[wd + 1] & 1) : e_s) << 63);
                        uint64_t v = last ? (mw ^ E) : ((mw ^ E) | (mw ^ sw) | (mw ^ SE));
                        const int base = x0 - 64 + 64 * wd;
                        const int lc = W - 1 - base;                             // the last column, if in this word
                        if (lc >= 0 && lc < 64) {
                            const uint64_t bit = 1ull << lc;
                            v = (v & ~bit) | (last ? 0ull : ((mw ^ sw) & bit));
                        }
                        bw[wd] = v & jf_cols_mask(base, W);
                    }
                    if (in_tile) Bc[map * JF_TH + j - r] = bw[1];
                    if ((bw[0] | bw[1] | bw[2]) == 0) continue;
                    uint64_t h = bw[1];
                    int w = 0;
                    for (int a = r; a >= 0; --a) {                               // |dy| = a, the half-width only grows
                        const int wt = s_w[a];
                        for (; w < wt;) {
                            ++w;
                            h |= (bw[1] >> w) | (bw[2] << (64 - w)) | (bw[1] << w) | (bw[0] >> (64 - w));
                        }
                        if (h == 0) continue;
                        const int i1 = j - r - a, i2 = j - r + a;               // output rows s - dy for dy = +a and -a
                        if (i1 >= 0 && i1 < JF_TH) atomicOr(reinterpret_cast<unsigned long long*>(&D[map * JF_TH + i1]), (unsigned long long)h);
                        if (a != 0 && i2 >= 0 && i2 < JF_TH)
                            atomicOr(reinterpret_cast<unsigned long long*>(&D[map * JF_TH + i2]), (unsigned long long)h);
                    }
                }
                __syncthreads();
                // ---- C: popcounts of the tile rows, wave reduction, one atomic per non-zero slot ---------------------------
                if (wave == 0) {
                    int c[JF_SLOTS] = {0, 0, 0, 0, 0, 0, 0};
                    if (y0 + lane < H) {
                        const int j = r + lane;
                        const uint64_t mg = M[(size_t)j * 3 + 1], mp = M[(size_t)nrows * 3 + j * 3 + 1];
                        const uint64_t bg = Bc[lane], bp = Bc[JF_TH + lane];
                        const uint64_t dg = D[lane], dp = D[JF_TH + lane];
                        c[0] = __popcll(mg);
                        c[1] = __popcll(mp);
                        c[2] = __popcll(mg & mp);
                        c[3] = __popcll(bg);
                        c[4] = __popcll(bp);
                        c[5] = __popcll(bg & dp);
                        c[6] = __popcll(bp & dg);
                    }
                    for (int q = 0; q < JF_SLOTS; ++q)
                        for (int off = 32; off > 0; off >>= 1) c[q] += __shfl_xor(c[q], off, 64);
                    if (lane == 0) {
                        int* dst = counts + ((size_t)b * 256 + k) * JF_SLOTS;
                        for (int q = 0; q < JF_SLOTS; ++q)
                            if (c[q]) atomicAdd(dst + q, c[q]);
                    }
                }
                __syncthreads();
            }
        }
    }
}

extern "C" int xmem_jf_counts(const uint8_t* gt, const uint8_t* pred, const uint8_t* lut, int B, int H, int W, int radius,
                              int32_t* counts, void* stream) {
    if (!gt || !pred || !counts || B <= 0 || H <= 0 || W <= 0 || radius < 0) return XMEM_ERR_BAD_ARG;
    if (radius > JF_MAX_R || H > JF_MAX_HW || W > JF_MAX_HW) return XMEM_ERR_UNSUPPORTED;
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)B * 256 * JF_SLOTS * sizeof(int32_t), s) != hipSuccess) return XMEM_ERR_LAUNCH;
    const size_t lds = jf_lds_bytes(radius);
    const int rc = xmem_ensure_dynamic_lds(reinterpret_cast<const void*>(jf_counts_kernel), lds);
    if (rc != XMEM_OK) return rc;
    const dim3 grid(cdiv(W, 64), cdiv(H, JF_TH), B < 65535 ? B : 65535);
    hipLaunchKernelGGL(jf_counts_kernel, grid, dim3(JF_THREADS), lds, s, gt, pred, lut, B, H, W, radius, (int*)counts);
    return xmem_check_launch();
}
