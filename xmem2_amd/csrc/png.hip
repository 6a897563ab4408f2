// PNG files of uint8 planes, built on the device (include/xmem_hip_png.h; xmem2_amd/png.py has the definition the bytes are held to).
//
//   rows     one workgroup per (frame, row), in the row pass and again in the emit pass.  The Up-filtered row - table look-up of the
//            row and of the row above, their difference - goes into LDS as bytes; thread t owns the bytes [t P, (t + 1) P) of it,
//            P = ceil(L / 256).  A byte's token depends on its offset in its run of equal bytes and on the run's length: a thread
//            finds the first and the last run start of its bytes, two scans over the workgroup (the last start before a thread's
//            bytes, the first one behind them) give it the runs that reach across its ends, and it walks its bytes run by run,
//            jumping over the bytes a match covers.  A token belongs to the thread that owns its first byte.  `walk` is that loop;
//            the row pass counts its bits, the emit pass counts them again - cheaper than storing a role per byte -, scans the
//            counts and walks once more with the bit position in hand.
//   bits     a token is at most 18 bits (an 8-bit length code, 5 extra bits, the 5 bits of distance code 0).  The emit pass ORs
//            the tokens into an LDS image of the words the row's bits touch, aligned to the words of `out`; the image's inner
//            words belong to the row alone and are stored, its first and last word are shared with the neighbouring rows (a row is
//            at least 16 bits: a word has at most three owners) or with the bytes round the block and take a global atomic OR.
//            `out` was zeroed by the call's memset node; bytes at and beyond a frame's capacity are masked off.
//   sums     Adler-32 is A = 1 + sum b, B = sum over bytes of the running A = n + sum b_j (n - j): a row gives sum b and
//            sum b (L + 1 - p) over its own bytes, reduced mod 65521 per thread (a thread's sum stays below 2^64 by far), and the
//            scan launch adds the rows' shares.  CRC-32 is linear over GF(2): the register after a message is the XOR over
//            segments of the segment's register (started at 0) times x^(8 * bytes behind it) mod P, and of the initial word times
//            x^(8 * all bytes).  A thread does a table-driven segment and one multiplication by a power made from x^(2^k) by
//            repeated squaring at compile time; waves XOR their lanes and add one atomic XOR each.
//
// Integer only.  The atomics are OR and XOR (and LDS integer adds), whose results depend on no order.
#include <limits.h>
#include "common.hpp"
#include "../../include/xmem_hip_png.h"

#define PNG_MAX_HW 16384
#define PNG_MAX_N 65535
#define PNG_THREADS 256
#define PNG_CRC_SEGMENT 128          // bytes of the IDAT chunk one thread of the CRC pass reads
#define PNG_ADLER 65521u

namespace {

// ---- CRC-32 (reflected, polynomial 0xedb88320) ---------------------------------------------------------------------------------------

constexpr uint32_t CRC_POLY = 0xedb88320u;

// a(x) b(x) mod P; bit 31 is x^0
constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 31; k >= 0; --k) {
        if ((a >> k) & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

struct CrcTables {
    uint32_t byte[256];              // the register after one byte, started at the byte
    uint32_t x2n[32];                // x^(2^k) mod P
    constexpr CrcTables() : byte(), x2n() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
            byte[i] = c;
        }
        uint32_t p = 1u << 30;       // x^1
        x2n[0] = p;
        for (int k = 1; k < 32; ++k) x2n[k] = p = crc_mul(p, p);
    }
};

__constant__ CrcTables crc_tables = CrcTables();

// r times x^(8 n) mod P: the register r after n more zero bytes
__device__ uint32_t crc_shift(uint32_t r, uint64_t n) {
    uint32_t p = 1u << 31;           // x^0
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1u) p = crc_mul(crc_tables.x2n[k & 31], p);
    return crc_mul(p, r);
}

__device__ __forceinline__ uint32_t crc_byte(const uint32_t* table, uint32_t r, uint32_t b) { return table[(r ^ b) & 0xffu] ^ (r >> 8); }

// ---- tokens --------------------------------------------------------------------------------------------------------------------------

struct Token {
    uint32_t bits;                   // in stream order, first bit in bit 0
    int n;
};

__device__ __forceinline__ Token literal_token(uint32_t v) {
    if (v < 144u) return {__brev(0x30u + v) >> 24, 8};
    return {__brev(0x190u + v - 144u) >> 23, 9};
}

// a match of `len` in 3..258 at distance 1: the length code, its extra bits, five zero bits
__device__ __forceinline__ Token match_token(int len) {
    if (len == 258) return {__brev(0xc5u) >> 24, 13};
    const uint32_t x = (uint32_t)(len - 3);
    if (x < 8u) return {__brev(1u + x) >> 25, 12};
    const int extra = 29 - __clz(x);                                     // floor(log2 x) - 2
    const uint32_t code = 261u + 4u * extra + ((x >> extra) & 3u);
    uint32_t bits;
    int width;
    if (code < 280u) {
        bits = __brev(code - 256u) >> 25;
        width = 7;
    } else {
        bits = __brev(0xc0u + code - 280u) >> 24;
        width = 8;
    }
    return {bits | ((x & ((1u << extra) - 1u)) << width), width + extra + 5};
}

// the tokens that start in the bytes [a, b) of the filtered row d [L], in order.  prev: the last run start before a; next: the first
// one from b on (L without one).  emit(Token).
template <class F>
__device__ __forceinline__ void walk(const uint8_t* d, int a, int b, int prev, int next, F&& emit) {
    if (a >= b) return;
    int i = a;
    int s = (a == 0 || d[a] != d[a - 1]) ? a : prev;
    while (i < b) {
        int e = i + 1;
        while (e < b && d[e] == d[e - 1]) ++e;
        if (e == b) e = next;                                            // the run may go on in the next thread's bytes
        const uint32_t v = d[i];
        const int t = (e - s - 1) % 258;
        const int hi = e < b ? e : b;
        while (i < hi) {
            const int o = i - s, rem = e - i;
            if (o == 0 || (rem <= t && t < 3)) {
                emit(literal_token(v));
                ++i;
                continue;
            }
            const int r = (o - 1) % 258;
            const int step = r == 0 ? (rem < 258 ? rem : 258) : (258 - r < rem ? 258 - r : rem);
            if (r == 0) emit(match_token(step));
            i += step;                                                   // r != 0: inside a match an earlier thread owns
        }
        s = e;
    }
}

struct RowScratch {
    uint8_t table[768];
    int scan[2][2][PNG_THREADS];     // [which value][double buffer][thread]
    uint32_t sums[4];
};

// the filtered row y of frame n into d [L]: per pixel, the table's bytes of the row minus those of the row above (zeros above row 0)
template <int C>
__device__ __forceinline__ void stage_row(const uint8_t* __restrict__ planes, int n, int y, int H, int W, const uint8_t* __restrict__ table,
                                          uint8_t* tab, uint8_t* d) {
    for (int i = threadIdx.x; i < 256 * C; i += PNG_THREADS) tab[i] = table ? table[i] : (uint8_t)i;
    __syncthreads();
    const uint8_t* cur = planes + ((size_t)n * H + y) * W;
    const uint8_t* above = cur - W;
    for (int x = threadIdx.x; x < W; x += PNG_THREADS) {
        const int v = cur[x] * C, u = y > 0 ? above[x] * C : -1;
#pragma unroll
        for (int c = 0; c < C; ++c) d[x * C + c] = (uint8_t)(tab[v + c] - (u < 0 ? 0 : tab[u + c]));
    }
    __syncthreads();
}

// exclusive scans over the workgroup's threads: -> (max of `last` over the threads before this one, else -1; min of `first` over
// the threads behind it, else `none`)
__device__ __forceinline__ void run_scans(RowScratch& sc, int last, int first, int none, int& prev, int& next) {
    const int t = threadIdx.x, u = PNG_THREADS - 1 - t;                  // the second scan runs over the threads in reverse
    sc.scan[0][0][t] = last;
    sc.scan[1][0][u] = first;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < PNG_THREADS; o <<= 1) {
        int p = sc.scan[0][cur][t], q = sc.scan[1][cur][t];
        if (t >= o) {
            p = max(p, sc.scan[0][cur][t - o]);
            q = min(q, sc.scan[1][cur][t - o]);
        }
        sc.scan[0][cur ^ 1][t] = p;
        sc.scan[1][cur ^ 1][t] = q;
        cur ^= 1;
        __syncthreads();
    }
    prev = t > 0 ? sc.scan[0][cur][t - 1] : -1;
    next = u > 0 ? sc.scan[1][cur][u - 1] : none;
    __syncthreads();
}

// the exclusive sum of v over the threads before this one
__device__ __forceinline__ int sum_scan(RowScratch& sc, int v) {
    const int t = threadIdx.x;
    sc.scan[0][0][t] = v;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < PNG_THREADS; o <<= 1) {
        int p = sc.scan[0][cur][t];
        if (t >= o) p += sc.scan[0][cur][t - o];
        sc.scan[0][cur ^ 1][t] = p;
        cur ^= 1;
        __syncthreads();
    }
    const int r = t > 0 ? sc.scan[0][cur][t - 1] : 0;
    __syncthreads();
    return r;
}

// this thread's bytes [a, b) of a row of L, and the run starts that reach across their ends
__device__ __forceinline__ void thread_span(RowScratch& sc, const uint8_t* d, int L, int& a, int& b, int& prev, int& next) {
    const int P = (L + PNG_THREADS - 1) / PNG_THREADS;
    a = min((int)threadIdx.x * P, L);
    b = min(a + P, L);
    int first = L, last = -1;
    for (int i = a; i < b; ++i)
        if (i == 0 || d[i] != d[i - 1]) {
            if (first == L) first = i;
            last = i;
        }
    run_scans(sc, last, first, L, prev, next);
}

struct Layout {                      // of the workspace, in this order; every part 8-byte aligned
    uint64_t* row_ofs;               // [N][H] the bit at which a row starts in its frame's deflate block
    uint64_t* dlen;                  // [N] bytes of the deflate block
    uint32_t* row_bits;              // [N][H]
    uint32_t* row_s;                 // [N][H] sum of the filtered row's bytes mod 65521
    uint32_t* row_t;                 // [N][H] sum of byte * (L + 1 - position) mod 65521
    uint32_t* crc;                   // [N] the IDAT chunk's CRC register
};

inline size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

inline size_t carve(void* ws, int N, int H, Layout* lay) {
    const size_t rows = (size_t)N * H;
    size_t ofs = 0;
    auto take = [&](size_t bytes) {
        void* p = ws ? (char*)ws + ofs : nullptr;
        ofs += align8(bytes);
        return p;
    };
    Layout l;
    l.row_ofs = (uint64_t*)take(rows * 8);
    l.dlen = (uint64_t*)take((size_t)N * 8);
    l.row_bits = (uint32_t*)take(rows * 4);
    l.row_s = (uint32_t*)take(rows * 4);
    l.row_t = (uint32_t*)take(rows * 4);
    l.crc = (uint32_t*)take((size_t)N * 4);
    if (lay) *lay = l;
    return ofs;
}

// ---- row pass ------------------------------------------------------------------------------------------------------------------------

template <int C>
__global__ __launch_bounds__(PNG_THREADS) void png_row_kernel(const uint8_t* __restrict__ planes, int H, int W, const uint8_t* __restrict__ table,
                                                              Layout lay) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    __shared__ RowScratch sc;
    const int y = blockIdx.x, n = blockIdx.y, L = W * C;
    uint8_t* d = dyn;
    if (threadIdx.x < 4) sc.sums[threadIdx.x] = 0;
    stage_row<C>(planes, n, y, H, W, table, sc.table, d);
    int a, b, prev, next;
    thread_span(sc, d, L, a, b, prev, next);
    int bits = threadIdx.x == 0 ? 8 : 0;                                 // the filter byte, a literal 2
    walk(d, a, b, prev, next, [&](Token t) { bits += t.n; });
    uint64_t s = threadIdx.x == 0 ? 2u : 0u, w = threadIdx.x == 0 ? 2ull * (uint64_t)(L + 1) : 0ull;
    for (int i = a; i < b; ++i) {
        s += d[i];
        w += (uint64_t)d[i] * (uint64_t)(L - i);
    }
    bits = wave_sum_i(bits);
    const int sm = wave_sum_i((int)(s % PNG_ADLER)), wm = wave_sum_i((int)(w % PNG_ADLER));
    if ((threadIdx.x & (XMEM_WAVE - 1)) == 0) {
        atomicAdd(&sc.sums[0], (uint32_t)bits);
        atomicAdd(&sc.sums[1], (uint32_t)sm);
        atomicAdd(&sc.sums[2], (uint32_t)wm);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t row = (size_t)n * H + y;
        lay.row_bits[row] = sc.sums[0];
        lay.row_s[row] = sc.sums[1] % PNG_ADLER;
        lay.row_t[row] = sc.sums[2] % PNG_ADLER;
    }
}

// ---- scan of the rows, and every byte outside the deflate block but the IDAT checksum ---------------------------------------------------

__device__ __forceinline__ void put(uint8_t* file, int capacity, uint64_t at, uint32_t byte) {
    if (at < (uint64_t)capacity) file[at] = (uint8_t)byte;
}

__device__ __forceinline__ void put_be32(uint8_t* file, int capacity, uint64_t at, uint32_t v) {
    for (int k = 0; k < 4; ++k) put(file, capacity, at + k, (v >> (24 - 8 * k)) & 0xffu);
}

__global__ __launch_bounds__(PNG_THREADS) void png_scan_kernel(int H, int W, int C, int color_type, const uint8_t* __restrict__ palette,
                                                               int capacity, int32_t* __restrict__ meta, uint8_t* __restrict__ out, Layout lay) {
    __shared__ uint64_t scan[2][PNG_THREADS];
    __shared__ uint32_t sums[3];                                         // Adler A and B shares, the PLTE chunk's CRC register
    const int n = blockIdx.x, t = threadIdx.x;
    const int per = (H + PNG_THREADS - 1) / PNG_THREADS, y0 = min(t * per, H), y1 = min(y0 + per, H);
    const uint32_t* bits = lay.row_bits + (size_t)n * H;
    const uint64_t row_bytes = (uint64_t)W * C + 1, total = (uint64_t)H * row_bytes;
    if (t < 3) sums[t] = 0;
    uint64_t mine = 0, sa = 0, sb = 0;
    for (int y = y0; y < y1; ++y) {
        mine += bits[y];
        const uint64_t s = lay.row_s[(size_t)n * H + y], w = lay.row_t[(size_t)n * H + y];
        sa += s;
        sb += w + s * ((total - (uint64_t)(y + 1) * row_bytes) % PNG_ADLER);          // below 2^6 * 2^33
    }
    scan[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < PNG_THREADS; o <<= 1) {
        uint64_t p = scan[cur][t];
        if (t >= o) p += scan[cur][t - o];
        scan[cur ^ 1][t] = p;
        cur ^= 1;
        __syncthreads();
    }
    uint64_t at = 3 + (t > 0 ? scan[cur][t - 1] : 0);                    // behind BFINAL and BTYPE
    for (int y = y0; y < y1; ++y) {
        lay.row_ofs[(size_t)n * H + y] = at;
        at += bits[y];
    }
    const uint64_t D = (3 + scan[cur][PNG_THREADS - 1] + 7 + 7) / 8;     // the end-of-block code is seven zero bits
    atomicAdd(&sums[0], (uint32_t)(sa % PNG_ADLER));
    atomicAdd(&sums[1], (uint32_t)(sb % PNG_ADLER));

    uint8_t* file = out + (size_t)n * capacity;
    const uint32_t* crc_table = crc_tables.byte;
    const uint64_t idat = color_type == XMEM_PNG_PALETTE ? 33 + 780 : 33;                // where the IDAT chunk starts
    if (color_type == XMEM_PNG_PALETTE) {                                // PLTE: thread t carries entry t
        uint32_t r = 0;
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = palette[3 * t + k];
            put(file, capacity, 41 + 3 * t + k, v);
            r = crc_byte(crc_table, r, v);
        }
        atomicXor(&sums[2], crc_shift(r, (uint64_t)(768 - 3 * (t + 1))));
    }
    __syncthreads();
    if (t != 0) return;
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int k = 0; k < 8; ++k) put(file, capacity, k, sig[k]);
    const uint8_t ihdr[17] = {'I', 'H', 'D', 'R', (uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W, (uint8_t)(H >> 24),
                              (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H, 8, (uint8_t)color_type, 0, 0, 0};
    uint32_t r = 0xffffffffu;
    put_be32(file, capacity, 8, 13);
    for (int k = 0; k < 17; ++k) {
        put(file, capacity, 12 + k, ihdr[k]);
        r = crc_byte(crc_table, r, ihdr[k]);
    }
    put_be32(file, capacity, 29, ~r);
    if (color_type == XMEM_PNG_PALETTE) {
        const uint8_t name[4] = {'P', 'L', 'T', 'E'};
        r = 0xffffffffu;
        put_be32(file, capacity, 33, 768);
        for (int k = 0; k < 4; ++k) {
            put(file, capacity, 37 + k, name[k]);
            r = crc_byte(crc_table, r, name[k]);
        }
        put_be32(file, capacity, 41 + 768, ~(crc_shift(r, 768) ^ sums[2]));
    }
    const uint8_t head[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    put_be32(file, capacity, idat, (uint32_t)(D + 6));
    for (int k = 0; k < 6; ++k) put(file, capacity, idat + 4 + k, head[k]);
    put(file, capacity, idat + 10, 3);                                   // BFINAL = 1, BTYPE = 01; the emit pass ORs row 0 behind them
    const uint32_t A = (1 + sums[0]) % PNG_ADLER, B = (uint32_t)((total + sums[1]) % PNG_ADLER);
    put_be32(file, capacity, idat + 10 + D, (B << 16) | A);
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    for (int k = 0; k < 12; ++k) put(file, capacity, idat + 10 + D + 8 + k, iend[k]);
    const uint64_t length = idat + 10 + D + 20;
    meta[n * XMEM_PNG_META + 0] = (int32_t)(length < (uint64_t)INT_MAX ? length : (uint64_t)INT_MAX);
    meta[n * XMEM_PNG_META + 1] = (int32_t)(D < (uint64_t)INT_MAX ? D : (uint64_t)INT_MAX);
    meta[n * XMEM_PNG_META + 2] = meta[n * XMEM_PNG_META + 3] = 0;
    lay.dlen[n] = D;
    lay.crc[n] = crc_shift(0xffffffffu, 4 + D + 6);                      // the initial word, carried over the whole chunk
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------------

template <int C>
__global__ __launch_bounds__(PNG_THREADS) void png_emit_kernel(const uint8_t* __restrict__ planes, int H, int W, const uint8_t* __restrict__ table,
                                                               int block_at, int capacity, uint8_t* __restrict__ out, Layout lay, int image_words) {
    extern __shared__ __attribute__((aligned(16))) uint8_t dyn[];
    __shared__ RowScratch sc;
    const int y = blockIdx.x, n = blockIdx.y, L = W * C;
    uint32_t* image = (uint32_t*)dyn;
    uint8_t* d = dyn + 4 * (size_t)image_words;
    const size_t row = (size_t)n * H + y;
    const uintptr_t file = (uintptr_t)out + (size_t)n * capacity, file_end = file + (size_t)capacity;
    const uint64_t bit0 = ((uint64_t)file + (uint64_t)block_at) * 8 + lay.row_ofs[row];    // the row's first bit, counted from address 0
    const uint32_t row_bits = lay.row_bits[row];
    const uintptr_t word0 = (uintptr_t)(bit0 >> 5) << 2;                 // the address of the image's word 0
    const int shift0 = (int)(bit0 & 31), words = (int)((shift0 + row_bits + 31) >> 5);
    if (word0 >= file_end) return;                                       // nothing of the row fits (uniform over the workgroup)
    for (int w = threadIdx.x; w < words; w += PNG_THREADS) image[w] = 0;
    stage_row<C>(planes, n, y, H, W, table, sc.table, d);
    int a, b, prev, next;
    thread_span(sc, d, L, a, b, prev, next);
    int bits = threadIdx.x == 0 ? 8 : 0;
    walk(d, a, b, prev, next, [&](Token t) { bits += t.n; });
    int pos = shift0 + sum_scan(sc, bits);
    auto emit = [&](Token t) {
        const uint64_t v = (uint64_t)t.bits << (pos & 31);
        atomicOr(&image[pos >> 5], (uint32_t)v);
        if (v >> 32) atomicOr(&image[(pos >> 5) + 1], (uint32_t)(v >> 32));
        pos += t.n;
    };
    if (threadIdx.x == 0) emit(literal_token(2));
    walk(d, a, b, prev, next, emit);
    __syncthreads();
    for (int w = threadIdx.x; w < words; w += PNG_THREADS) {
        const uintptr_t at = word0 + 4 * (uintptr_t)w;
        uint32_t v = image[w];
        if (at >= file_end) continue;
        if (file_end - at < 4) v &= (1u << (8 * (file_end - at))) - 1u;  // bytes at and beyond the capacity keep their values
        if (!v) continue;
        // shared with the rows or the bytes next to this one, or with the bytes behind the capacity
        if (w == 0 || w == words - 1 || file_end - at < 4) atomicOr((uint32_t*)at, v);
        else *(uint32_t*)at = v;
    }
}

// ---- the IDAT chunk's CRC --------------------------------------------------------------------------------------------------------------

// a frame's file fits its capacity
__device__ __forceinline__ bool fits(const Layout& lay, int n, int idat, int capacity) { return (uint64_t)idat + 30 + lay.dlen[n] <= (uint64_t)capacity; }

__global__ __launch_bounds__(PNG_THREADS) void png_crc_kernel(int idat, int capacity, const uint8_t* __restrict__ out, Layout lay) {
    __shared__ uint32_t table[256];
    const int n = blockIdx.y;
    const uint64_t length = 4 + lay.dlen[n] + 6;                         // type, zlib header, block, Adler-32
    const uint64_t first = ((uint64_t)blockIdx.x * PNG_THREADS + threadIdx.x) * PNG_CRC_SEGMENT;
    if (!fits(lay, n, idat, capacity) || (uint64_t)blockIdx.x * PNG_THREADS * PNG_CRC_SEGMENT >= length) return;   // uniform
    table[threadIdx.x] = crc_tables.byte[threadIdx.x];
    __syncthreads();
    uint32_t r = 0;
    if (first < length) {
        const uint64_t count = length - first < PNG_CRC_SEGMENT ? length - first : PNG_CRC_SEGMENT;
        const uint8_t* p = out + (size_t)n * capacity + idat + 4 + first;
        for (uint64_t k = 0; k < count; ++k) r = crc_byte(table, r, p[k]);
        r = crc_shift(r, length - first - count);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r ^= __shfl_xor(r, o, 64);
    if ((threadIdx.x & (XMEM_WAVE - 1)) == 0 && r) atomicXor(&lay.crc[n], r);
}

__global__ __launch_bounds__(PNG_THREADS) void png_finish_kernel(int N, int idat, int capacity, uint8_t* __restrict__ out, Layout lay) {
    const int n = blockIdx.x * PNG_THREADS + threadIdx.x;
    if (n >= N || !fits(lay, n, idat, capacity)) return;
    put_be32(out + (size_t)n * capacity, capacity, (uint64_t)idat + 8 + lay.dlen[n] + 6, ~lay.crc[n]);
}

inline int channels_of(int color_type) { return color_type == XMEM_PNG_RGB ? 3 : 1; }

// the words of the LDS image of a row of L bytes: 31 bits of the word it starts in, 9 bits a byte at most
inline int image_words_of(int L) { return (31 + 9 * (L + 1) + 31) / 32 + 1; }

}  // namespace

extern "C" size_t xmem_png_workspace_bytes(int N, int H, int W, int channels) {
    if (N < 1 || N > PNG_MAX_N || H < 1 || H > PNG_MAX_HW || W < 1 || W > PNG_MAX_HW || (channels != 1 && channels != 3)) return 0;
    return carve(nullptr, N, H, nullptr);
}

extern "C" int xmem_png_encode(const uint8_t* planes, int N, int H, int W, int color_type, const uint8_t* table, const uint8_t* palette,
                               int capacity, int32_t* meta, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!planes || !meta || !out || !workspace || ((uintptr_t)meta & 3) || ((uintptr_t)out & 3) || capacity < 1) return XMEM_ERR_BAD_ARG;
    if (color_type != XMEM_PNG_GREY && color_type != XMEM_PNG_RGB && color_type != XMEM_PNG_PALETTE) return XMEM_ERR_BAD_ARG;
    if (color_type != XMEM_PNG_GREY && !table) return XMEM_ERR_BAD_ARG;
    if ((color_type == XMEM_PNG_PALETTE) != (palette != nullptr)) return XMEM_ERR_BAD_ARG;
    if (H < 1 || W < 1 || H > PNG_MAX_HW || W > PNG_MAX_HW || N < 1 || N > PNG_MAX_N) return XMEM_ERR_UNSUPPORTED;
    const int C = channels_of(color_type), L = W * C;
    if (workspace_bytes < xmem_png_workspace_bytes(N, H, W, C) || ((uintptr_t)workspace & 7)) return XMEM_ERR_WORKSPACE;
    Layout lay;
    carve(workspace, N, H, &lay);
    const hipStream_t s = (hipStream_t)stream;
    const int idat = color_type == XMEM_PNG_PALETTE ? 33 + 780 : 33, block_at = idat + 10;
    const int image_words = image_words_of(L);
    const size_t row_lds = ((size_t)L + 3) & ~(size_t)3, emit_lds = 4 * (size_t)image_words + row_lds;
    const void* row_fn = C == 3 ? (const void*)png_row_kernel<3> : (const void*)png_row_kernel<1>;
    const void* emit_fn = C == 3 ? (const void*)png_emit_kernel<3> : (const void*)png_emit_kernel<1>;
    int rc = xmem_ensure_dynamic_lds(row_fn, row_lds);
    if (rc == XMEM_OK) rc = xmem_ensure_dynamic_lds(emit_fn, emit_lds);
    if (rc != XMEM_OK) return rc;
    if (hipMemsetAsync(out, 0, (size_t)N * (size_t)capacity, s) != hipSuccess) return XMEM_ERR_LAUNCH;
    const dim3 rows((unsigned)H, (unsigned)N), threads(PNG_THREADS);
    if (C == 3) hipLaunchKernelGGL(png_row_kernel<3>, rows, threads, row_lds, s, planes, H, W, table, lay);
    else hipLaunchKernelGGL(png_row_kernel<1>, rows, threads, row_lds, s, planes, H, W, table, lay);
    hipLaunchKernelGGL(png_scan_kernel, dim3((unsigned)N), threads, 0, s, H, W, C, color_type, palette, capacity, meta, out, lay);
    if (C == 3) hipLaunchKernelGGL(png_emit_kernel<3>, rows, threads, emit_lds, s, planes, H, W, table, block_at, capacity, out, lay, image_words);
    else hipLaunchKernelGGL(png_emit_kernel<1>, rows, threads, emit_lds, s, planes, H, W, table, block_at, capacity, out, lay, image_words);
    // no file is longer than its capacity's worth of checksummed bytes, nor than the worst case of its size
    const uint64_t worst = 4 + ((uint64_t)3 + 9ull * H * (L + 1) + 14) / 8 + 6;
    const uint64_t reach = worst < (uint64_t)capacity ? worst : (uint64_t)capacity;
    const unsigned crc_blocks = (unsigned)((reach + (uint64_t)PNG_THREADS * PNG_CRC_SEGMENT - 1) / ((uint64_t)PNG_THREADS * PNG_CRC_SEGMENT));
    hipLaunchKernelGGL(png_crc_kernel, dim3(crc_blocks, (unsigned)N), threads, 0, s, idat, capacity, out, lay);
    hipLaunchKernelGGL(png_finish_kernel, dim3((unsigned)cdiv(N, PNG_THREADS)), threads, 0, s, N, idat, capacity, out, lay);
    return xmem_check_launch();
}
