// Implicit-GEMM convolution on the CDNA4 fp32 matrix pipe (v_mfma_f32_32x32x2_f32).
//
// GEMM view:  M = B*Ho*Wo output pixels, N = Cout, K = KH*KW*Cin (Cin fastest).
// NHWC activations and [Cout][KH][KW][Cin] weights make both operands K-contiguous, so one
// 128-byte global segment feeds one padded LDS row and every MFMA operand fragment is a single
// ds_read_b128 (row stride 36 floats -> the 16 lanes of a b128 lane-group hit 16 distinct 16-B slots).
//
// MFMA lane maps (cdna_hip_programming.md section 3): A[i=l&31][k=l>>5], B[k=l>>5][j=l&31],
// D[row=(r&3)+8*(r>>2)+4*(l>>5)][col=l&31].  A lane reads 4 consecutive k (float4) at k-offset 4*(l>>5)
// inside an 8-wide group; MFMA step j then contracts k = {j, 4+j} of the group - the same permutation for
// A and B, so the sum is unchanged.  fp32-input MFMA is an exact fmaf chain: results are fp32-roundoff
// class against the reference's CPU convolution.
//
// Replaces the nn.Conv2d/BatchNorm2d/ReLU/residual call sites listed in include/xmem_hip.h.
#include "common.hpp"
#include "gemm_stream.hpp"
#include "pointwise_pair.hpp"
#include <stdlib.h>

// BK (k-depth of a staged tile) is a template parameter: 32 or 64.  LDS rows are padded by 4 floats:
// stride 36 (=9x16 B) or 68 (=17x16 B) floats; both are odd multiples of 16 B, so the 16 lanes of a ds_read_b128
// lane-group (16 distinct rows) fall on 16 distinct 16-B slots of the 256-B bank row.

struct ConvArgs {
    const float* in; const float* w; const float* scale; const float* shift; const float* res;
    float* out; float* partial;
    int B, H, W, Cin, ldin;
    int Ho, Wo, Cout, ldout, ldres;
    int KH, KW, stride, pad;
    int K, M, HoWo;
    int relu_in, relu_out;
    int nk, splitk, kt_per_split;
    int tiles_m, tiles_n;
    int raw;                                   // 1: store the bare accumulator (Winograd-domain GEMM)
    int res_mod;                               // > 0: residual is one image broadcast over the batch (pixel index mod Ho*Wo)
    long in_gstride, w_gstride, out_gstride;   // blockIdx.y = group (the 16 Winograd tile positions), floats
    int a_presplit;                            // SPLIT kernels: the A operand already holds [hi4|lo4] groups (Winograd-domain V)
    int dbg;                                   // tools builds only (-DXMEM_TOOLS, env XMEM_CONV_DBG): 1 = no epilogue stores, 2 = every M-tile loads
                                               // tile 0's A rows (L2-resident operands); results are then wrong - they attribute time
    int dil, skip_taps;                        // DIL kernels only (xmem_conv2d_nhwc_dilated): tap spacing, 1 = skip taps outside the tile
};
#ifdef XMEM_TOOLS
#define CDBG(bit) (p.dbg & (bit))
// XMEM_CONV_DBG & 8: phase timestamps of every workgroup of the pointwise kernel (s_memtime, 100 MHz-class constant clock):
// entry, first tiles requested, first tiles in LDS, k-loop done, stores issued; xmem_conv2d_nhwc prints their averages.
#define CTRACE_MAX 16384
__device__ unsigned long long g_conv_trace[CTRACE_MAX][6];
#define CTRACE(slot) do { if (CDBG(8) && threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && blockIdx.x < CTRACE_MAX) \
    g_conv_trace[blockIdx.x][slot] = __builtin_readcyclecounter(); } while (0)
#else
#define CDBG(bit) 0
#define CTRACE(slot) do { } while (0)
#endif

// ---- SPLIT-OPERAND arithmetic (opt-in mode 'fp32x', never the default) ------------------------------------------------
// An fp32 value x is carried as two halfs, x = hi + lo (+ O(2^-21 |x|)): hi = x rounded toward zero to fp16 (saturating:
// finite values never become inf), lo = fp16(x - hi).  Four channels travel as ONE 16-byte group [hi0 hi1 hi2 hi3 | lo0 lo1
// lo2 lo3] - the same bytes as the four floats they replace, so tensor shapes, pixel strides, LDS layout and every loader of
// this file are unchanged.  As an operand of v_mfma_f32_32x32x16_f16 a group fills the 8 k-slots of a lane, and with B the
// same layout   mfma(A, B) = sum hi_a hi_b + lo_a lo_b,   mfma(A, swap halves of B) = sum hi_a lo_b + lo_a hi_b :
// two fp16 MFMAs (2 x 32 cycles) give all four partial products of 8 channels, where the fp32 pipe spends 4 x 64 cycles.
// Products of halfs are exact in the fp32 accumulator; what is lost is the representation error of the two operands.
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x4 split_pack(const f32x4 v) {
    const fp16x2 h01 = __builtin_amdgcn_cvt_pkrtz(v.x, v.y), h23 = __builtin_amdgcn_cvt_pkrtz(v.z, v.w);
    h16x8 o;
    o[0] = (_Float16)h01.x; o[1] = (_Float16)h01.y; o[2] = (_Float16)h23.x; o[3] = (_Float16)h23.y;
    // the residual of a saturated hi is clamped as well: |x| beyond 131008 saturates instead of turning into inf - inf
    o[4] = (_Float16)__builtin_amdgcn_fmed3f(v.x - (float)h01.x, -65504.f, 65504.f);
    o[5] = (_Float16)__builtin_amdgcn_fmed3f(v.y - (float)h01.y, -65504.f, 65504.f);
    o[6] = (_Float16)__builtin_amdgcn_fmed3f(v.z - (float)h23.x, -65504.f, 65504.f);
    o[7] = (_Float16)__builtin_amdgcn_fmed3f(v.w - (float)h23.y, -65504.f, 65504.f);
    return __builtin_bit_cast(f32x4, o);
}

// ONE: 1x1 / pad 0 (any stride) with Cin % BK == 0 (the pointwise layers and the 16 Winograd-domain GEMMs): operand rows are
// plain matrix rows, so each thread keeps loop-invariant 32-bit byte offsets and the K loop only advances a uniform base -
// no per-tile index arithmetic, bounds tests or exec-masked branches around the loads (rows past M / Cout are clamped:
// their products are never stored).  The address VALU work of the general loader was comparable to the MFMA issue time.
// HALF (the fp16 loop, config['precision'] = 'fp16': the counterpart of the reference's autocast frame loop,
// inference/run_on_video.py:76): activations and weights are IEEE halfs in memory, contracted on v_mfma_f32_32x32x16_f16 with fp32
// accumulation; the epilogue (scale / shift / residual / relu) runs in fp32 and the result is stored as fp32 (HALF = 1: key
// projection, split-K partials) or rounded once to fp16 (HALF = 2: every activation).  Eight halfs occupy the 16 bytes of four
// floats, so with Cin, ldin and K passed in 4-byte units (Cin / 2, ...) every loader of this file is unchanged; a 16-byte
// fragment is ONE fp16 MFMA (k = 16: 8 halfs per lane half) instead of four fp32 ones.
// DIL (xmem_conv2d_nhwc_dilated, fp32 direct form only): tap (kh, kw) reads input pixel (oh*stride - pad + kh*dil, ow*stride - pad + kw*dil).
// With skip_taps, a workgroup first bounds the output rows / columns its M-tile covers and drops every tap whose input rows or
// columns fall outside the map for ALL of them (a k-tile of a !GENERIC plan lies inside one tap: Cin % BK == 0).  A dropped tap
// would only have added exact zero products (acc + 0 * w == acc, and the accumulator starts at +0), so the sum keeps its bits.
template <int BM, int BN, int TM, int TN, int BK, bool GENERIC, bool ONE = false, bool SPLIT = false, int HALF = 0, int NW = 4, bool DIL = false>
__global__ __launch_bounds__(64 * NW) void conv_mfma_kernel(ConvArgs p) {
    constexpr int WN = BN / (32 * TN);
    constexpr int WM = BM / (32 * TM);
    static_assert(WM * WN == NW, "NW waves per workgroup (4; 8 for the 256x128 tile of the fp16 loop)");
    constexpr int LDK = BK + 4;
    constexpr int C4 = BK / 4;                 // float4 columns per staged row
    constexpr int RPP = 64 * NW / C4;          // rows staged per pass of the workgroup's threads
    constexpr int RA = BM / RPP, RB = BN / RPP;
    constexpr int BUF = (BM + BN) * LDK;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lh = lane >> 5;
    const int lrow = tid / C4, c4 = tid % C4;
    CTRACE(0);

    // XCD-aware tile order: consecutive tile ids (same M-tile, neighbouring N-tiles) stay on one XCD / L2.
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int tile_n = bid % p.tiles_n, tile_m = bid / p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const float* __restrict__ gin = p.in + (size_t)blockIdx.y * p.in_gstride;
    const float* __restrict__ gw = p.w + (size_t)blockIdx.y * p.w_gstride;
    float* __restrict__ gout = p.out + (size_t)blockIdx.y * p.out_gstride;

    int a_ih0[RA], a_iw0[RA], a_pix[RA];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m0 + lrow + RPP * i;
        if (m < p.M) {
            const int b = m / p.HoWo, rem = m - b * p.HoWo;
            const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
            a_ih0[i] = oh * p.stride - p.pad;
            a_iw0[i] = ow * p.stride - p.pad;
            a_pix[i] = b * p.H * p.W;
        } else {
            a_ih0[i] = -(1 << 28); a_iw0[i] = -(1 << 28); a_pix[i] = 0;
        }
    }

    const int kt_begin = blockIdx.z * p.kt_per_split;
    const int kt_end = min(p.nk, kt_begin + p.kt_per_split);

    unsigned a_boff[RA], b_boff[RB];           // ONE: byte offsets of this thread's operand rows (k = 0)
    if (ONE) {
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const int m = CDBG(2) ? min(lrow + RPP * i, p.M - 1) : min(m0 + lrow + RPP * i, p.M - 1);
            unsigned pix = (unsigned)m;
            if (p.stride != 1) {               // strided pointwise layer (ResNet downsample): input pixel of output pixel m
                const int b = m / p.HoWo, rem = m - b * p.HoWo;
                const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
                pix = (unsigned)((b * p.H + oh * p.stride) * p.W + ow * p.stride);
            }
            a_boff[i] = (pix * (unsigned)p.ldin + (unsigned)(c4 * 4)) * 4u;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int n = min(n0 + lrow + RPP * i, p.Cout - 1);
            b_boff[i] = ((unsigned)n * (unsigned)p.K + (unsigned)(c4 * 4)) * 4u;
        }
    }

    f32x4 ra[RA], rb[RB];
    auto load_tile = [&](int kt) {
        const int k0 = kt * BK;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        if (ONE) {
            const char* abase = reinterpret_cast<const char*>(gin) + (size_t)k0 * 4;
            const char* bbase = reinterpret_cast<const char*>(gw) + (size_t)k0 * 4;
#pragma unroll
            for (int i = 0; i < RA; ++i) ra[i] = *reinterpret_cast<const f32x4*>(abase + a_boff[i]);
#pragma unroll
            for (int i = 0; i < RB; ++i) rb[i] = *reinterpret_cast<const f32x4*>(bbase + b_boff[i]);
            return;
        }
        if (!GENERIC) {
            const int tap = k0 / p.Cin, c0 = k0 - tap * p.Cin;
            int kh = tap / p.KW, kw = tap - kh * p.KW;
            if (DIL) { kh *= p.dil; kw *= p.dil; }
#pragma unroll
            for (int i = 0; i < RA; ++i) {
                const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
                const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                const long off = (long)(a_pix[i] + ih * p.W + iw) * p.ldin + c0 + c4 * 4;
                ra[i] = ok ? *reinterpret_cast<const f32x4*>(gin + off) : zero;
            }
        } else {
            const int k = k0 + c4 * 4;
            const bool kok = k < p.K;
            const int tap = k / p.Cin, c0 = k - tap * p.Cin;
            int kh = tap / p.KW, kw = tap - kh * p.KW;
            if (DIL) { kh *= p.dil; kw *= p.dil; }
#pragma unroll
            for (int i = 0; i < RA; ++i) {
                const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
                const bool ok = kok && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                const long off = (long)(a_pix[i] + ih * p.W + iw) * p.ldin + c0;
                ra[i] = ok ? *reinterpret_cast<const f32x4*>(gin + off) : zero;
            }
        }
        const int kb = k0 + c4 * 4;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int n = n0 + lrow + RPP * i;
            const bool ok = n < p.Cout && kb < p.K;
            rb[i] = ok ? *reinterpret_cast<const f32x4*>(gw + (size_t)n * p.K + kb) : zero;
        }
    };
    auto store_tile = [&](int buf) {
        float* As = smem + buf * BUF;
        float* Bs = As + BM * LDK;
        if (p.relu_in) {                       // relu-on-load, applied when the data is consumed (never right after the
#pragma unroll                                 // global load: that would stall the wave before its MFMAs)
            for (int i = 0; i < RA; ++i) {
                if (HALF) {
                    const h16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
                    ra[i] = __builtin_bit_cast(f32x4, __builtin_elementwise_max(__builtin_bit_cast(h16x8, ra[i]), z));
                } else {
                    ra[i].x = fmaxf(ra[i].x, 0.f); ra[i].y = fmaxf(ra[i].y, 0.f);
                    ra[i].z = fmaxf(ra[i].z, 0.f); ra[i].w = fmaxf(ra[i].w, 0.f);
                }
            }
        }
        if (SPLIT && !p.a_presplit) {          // fp32 activations become [hi4|lo4] groups on their way into LDS
#pragma unroll
            for (int i = 0; i < RA; ++i) ra[i] = split_pack(ra[i]);
        }
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4*>(&As[(lrow + RPP * i) * LDK + c4 * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(&Bs[(lrow + RPP * i) * LDK + c4 * 4]) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // epilogue store mode (uniform): 0 raw accumulators, 1 split-K partials, 2 scale / shift (/ relu), 3 the same + residual
    const int mode = p.raw ? 0 : (p.splitk > 1 ? 1 : (p.res ? 3 : 2));
    const bool half_io = (HALF == 2) && mode >= 2;                        // activations (output and residual) are halfs; ldout / ldres count halfs
    // Small tiles request their residual values HERE, ahead of the operand tiles: the short-K pointwise layers (64 -> 256 at
    // 1/4 resolution: two k-tiles) are bound by memory round trips per workgroup, and a residual fetched in the epilogue adds a
    // whole one after the last MFMA (the same lane / row mapping as the epilogue below).
    constexpr bool EARLY_RES = TM * TN <= 2;
    float rve[EARLY_RES ? TM * TN : 1][16];
    // Two-accumulator tiles (128x64) also request the per-channel scale / shift of the epilogue here (round 5): -5 ... -12 % on the
    // batch-4 pointwise layers that take that tile; the 64x64 tile does not gain (+-2 %) and keeps the epilogue fetch
    // (profiles/r05_pointwise_prefetch_ab.txt).
    constexpr bool EARLY_SS = TM * TN == 2;
    float sce[EARLY_SS ? TN : 1], she[EARLY_SS ? TN : 1];
    // Round 6: WHERE they are requested.  Until then they stood between a workgroup's entry and its first operand request (~770
    // instructions with a per-element modulo behind a branch for the batch-broadcast case): the residual cost 13 us of a 51 us layer.  The
    // plain case is now 16 clamped rows off ONE 64-bit base, and the requests are issued AFTER the first operand tiles are in LDS, right
    // before the k-loop: they fly under the first k-tile's MFMAs, and the next tile's operand loads - younger - are waited for as a whole
    // anyway.  (Between the first operand request and its wait they lose: the compiler's load counter is the minimum over all paths to
    // a join, so with a path that loads no residual the operand wait becomes vmcnt(0..3), behind every younger residual load.)
    // DIL + skip_taps: bit t of `taps` = tap t reads at least one in-bounds input pixel for some output pixel of this M-tile
    unsigned long long taps = ~0ull;
    if (DIL && !GENERIC && p.skip_taps) {
        const int mlast = min(m0 + BM, p.M) - 1;
        const int b0 = m0 / p.HoWo, b1 = mlast / p.HoWo;
        const int r0 = m0 - b0 * p.HoWo, r1 = mlast - b1 * p.HoWo;
        int oh_lo = 0, oh_hi = p.Ho - 1, ow_lo = 0, ow_hi = p.Wo - 1;     // conservative: the whole map
        if (b0 == b1) {
            oh_lo = r0 / p.Wo; oh_hi = r1 / p.Wo;
            if (oh_lo == oh_hi) { ow_lo = r0 - oh_lo * p.Wo; ow_hi = r1 - oh_hi * p.Wo; }
        }
        unsigned rows = 0, cols = 0;
        for (int t = 0; t < p.KH; ++t) {
            const int lo = oh_lo * p.stride - p.pad + t * p.dil, hi = oh_hi * p.stride - p.pad + t * p.dil;
            if (hi >= 0 && lo < p.H) rows |= 1u << t;
        }
        for (int t = 0; t < p.KW; ++t) {
            const int lo = ow_lo * p.stride - p.pad + t * p.dil, hi = ow_hi * p.stride - p.pad + t * p.dil;
            if (hi >= 0 && lo < p.W) cols |= 1u << t;
        }
        taps = 0;
        for (int kh = 0; kh < p.KH; ++kh)
            if ((rows >> kh) & 1u) taps |= (unsigned long long)cols << (kh * p.KW);
    }
    const int kt_per_tap = DIL && !GENERIC ? p.Cin / BK : 1;
    // first k-tile at or after k whose tap is kept (the identity unless DIL + skip_taps)
    auto next_kt = [&](int k) {
        if (DIL && !GENERIC) {
            while (k < kt_end) {
                const int tap = k / kt_per_tap;
                if ((taps >> tap) & 1ull) break;
                k = (tap + 1) * kt_per_tap;
            }
        }
        return k;
    };
    const int kt_first = next_kt(kt_begin);

    if (kt_first < kt_end) {
        load_tile(kt_first);
        CTRACE(1);
        store_tile(0);
    }

    __syncthreads();
    CTRACE(2);

    if (EARLY_SS) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = min(n0 + wn * 32 * TN + j * 32 + l31, p.Cout - 1);
            sce[j] = mode >= 2 ? p.scale[n] : 1.f;
            she[j] = mode >= 2 ? p.shift[n] : 0.f;
        }
    }
    if (EARLY_RES && mode == 3 && p.res_mod == 0) {
        // plain residual (the rule): 16 unconditional loads from clamped rows, no per-element modulo, no branch
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = min(n0 + wn * 32 * TN + j * 32 + l31, p.Cout - 1);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mb = m0 + wm * 32 * TM + i * 32 + 4 * lh;
                const int left = p.M - 1 - mb;                             // rows below this lane's first one (negative past the end)
                const long rb = (long)mb * p.ldres + n;                     // ONE 64-bit product per block; the rows are 24-bit multiples of ldres
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long t = rb + __mul24(min((r & 3) + 8 * (r >> 2), left), p.ldres);
                    if (half_io) rve[i * TN + j][r] = (float)reinterpret_cast<const _Float16*>(p.res)[t];
                    else rve[i * TN + j][r] = p.res[t];
                }
            }
        }
    } else if (EARLY_RES && mode == 3) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = min(n0 + wn * 32 * TN + j * 32 + l31, p.Cout - 1);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mb = m0 + wm * 32 * TM + i * 32 + 4 * lh;
                const int mr = p.res_mod ? mb % p.res_mod : mb;
                const bool wrap_ok = p.res_mod >= 32;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = (r & 3) + 8 * (r >> 2);
                    int t = mr + o;
                    if (p.res_mod) { if (wrap_ok) { if (t >= p.res_mod) t -= p.res_mod; } else t = (mb + o) % p.res_mod; }
                    // unconditional loads from a clamped row (a predicated load is a branch, and behind a branch every load waits for
                    // its predecessor: rows past M are fetched from row M - 1 and never stored)
                    if (!p.res_mod) t = min(t, p.M - 1);
                    if (half_io) rve[i * TN + j][r] = (float)reinterpret_cast<const _Float16*>(p.res)[(size_t)t * p.ldres + n];
                    else rve[i * TN + j][r] = p.res[(size_t)t * p.ldres + n];
                }
            }
        }
    }

    int step = 0;
    for (int kt = kt_first; kt < kt_end; ) {
        const int buf = DIL ? (step & 1) : ((kt - kt_begin) & 1);
        const int kt_next = next_kt(kt + 1);
        const bool has_next = kt_next < kt_end;
        if (has_next) load_tile(kt_next);          // global loads in flight under the MFMAs below

        const float* As = smem + buf * BUF + (wm * 32 * TM + l31) * LDK + lh * 4;
        const float* Bs = smem + buf * BUF + BM * LDK + (wn * 32 * TN + l31) * LDK + lh * 4;
        // fragment loads run one k-group ahead of the MFMAs (two register sets): the ds_read latency of group kk+1 hides
        // under the MFMA chain of group kk instead of stalling the wave between groups
        f32x4 af[2][TM], bf[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const f32x4*>(As + i * 32 * LDK);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[0][j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * LDK);
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            const int cur = kk & 1, nxt = cur ^ 1;
            if (kk + 1 < BK / 8) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[nxt][i] = *reinterpret_cast<const f32x4*>(As + i * 32 * LDK + (kk + 1) * 8);
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[nxt][j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * LDK + (kk + 1) * 8);
            }
            __builtin_amdgcn_sched_barrier(0);     // keep the prefetch above this k-group's MFMAs
            if (HALF) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, af[cur][i]), __builtin_bit_cast(h16x8, bf[cur][j]),
                                                                           acc[i][j], 0, 0, 0);
            } else if (SPLIT) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const h16x8 b = __builtin_bit_cast(h16x8, bf[cur][j]);
                    const h16x8 bs = __builtin_shufflevector(b, b, 4, 5, 6, 7, 0, 1, 2, 3);
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const h16x8 a = __builtin_bit_cast(h16x8, af[cur][i]);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bs, acc[i][j], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][i][s], bf[cur][j][s], acc[i][j], 0, 0, 0);
            }
        }
        if (has_next) store_tile(buf ^ 1);
        __syncthreads();
        kt = kt_next; ++step;
    }

    CTRACE(3);
    // epilogue: lane owns output channel n (col) and 16 pixels (rows) per 32x32 tile.  The store mode is uniform, so it is
    // decided once and each 32x32 block runs straight-line code: all residual loads of a block are issued together
    // (one memory round trip per block instead of one per element) before the fused scale / shift / add / relu and stores.
    float* const obase = (mode == 1) ? p.partial + (size_t)blockIdx.z * p.M * p.Cout : gout;
    const long ldo = (mode == 1) ? (long)p.Cout : (long)p.ldout;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * 32 * TN + j * 32 + l31;
        if (n >= p.Cout) continue;
        float sc = 1.f, sh = 0.f;
        if (EARLY_SS) { sc = sce[j]; sh = she[j]; }
        else if (mode >= 2) { sc = p.scale[n]; sh = p.shift[n]; }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = m0 + wm * 32 * TM + i * 32 + 4 * lh;          // this lane's rows: mb + (r & 3) + 8 * (r >> 2)
            float* const orow = obase + (size_t)mb * ldo + n;
            _Float16* const orow_h = reinterpret_cast<_Float16*>(obase) + (size_t)mb * ldo + n;
            float rv[16];
            if (EARLY_RES && mode == 3) {
#pragma unroll
                for (int r = 0; r < 16; ++r) rv[r] = rve[i * TN + j][r];
            } else if (mode == 3) {
                int mr = p.res_mod ? mb % p.res_mod : mb;                 // broadcast residual: row index modulo one image
                const bool wrap_ok = p.res_mod >= 32;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = (r & 3) + 8 * (r >> 2);
                    int t = mr + o;
                    if (p.res_mod) { if (wrap_ok) { if (t >= p.res_mod) t -= p.res_mod; } else t = (mb + o) % p.res_mod; }
                    if (!p.res_mod) t = min(t, p.M - 1);          // clamped, unconditional (see the early request above)
                    if (half_io) rv[r] = (float)reinterpret_cast<const _Float16*>(p.res)[(size_t)t * p.ldres + n];
                    else rv[r] = p.res[(size_t)t * p.ldres + n];
                }
            }
            // TWO PHASES (round 6).  gfx9 counts loads AND stores in one in-order counter (vmcnt).  With the fused arithmetic and the store
            // of an element in one loop body - behind the row-bounds branch of that element - the compiler cannot know, at the join after a
            // skipped element, whether scale / shift / residual have arrived, and waits vmcnt(0) in EVERY body: each store then waits for the
            // previous store to land - 16 serialised round trips, 9 000 of a 17 500-cycle workgroup at the 64 -> 256 pointwise layer
            // (profiles/r06_pointwise_epilogue.txt).  Phase 1 consumes every loaded operand; phase 2 only stores registers.
            float vout[16];
            if (mode >= 2) {
                const bool add_res = mode == 3, relu = p.relu_out != 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[i][j][r] * sc + sh;
                    if (add_res) v += rv[r];
                    vout[r] = relu ? fmaxf(v, 0.f) : v;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) vout[r] = acc[i][j][r];
            }
            if (CDBG(1)) { if (vout[0] == 1.2345e-33f) orow[0] = vout[0]; continue; }
            if (m0 + wm * 32 * TM + i * 32 + 32 <= p.M) {      // (wave-uniform) every row of the block exists: straight-line stores
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = (r & 3) + 8 * (r >> 2);
                    if (half_io) orow_h[(long)o * ldo] = (_Float16)vout[r];
                    else orow[(long)o * ldo] = vout[r];
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = (r & 3) + 8 * (r >> 2);
                    if (mb + o >= p.M) continue;
                    if (half_io) orow_h[(long)o * ldo] = (_Float16)vout[r];
                    else orow[(long)o * ldo] = vout[r];
                }
            }
        }
    }
    CTRACE(4);
    if (CDBG(8)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); CTRACE(5); }
}

template <bool HALF_IO>
__global__ void conv_splitk_reduce_kernel(ConvArgs p) {
    const size_t total = (size_t)p.M * p.Cout;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(e / p.Cout), n = (int)(e - (size_t)m * p.Cout);
        float v = 0.f;
#pragma unroll 4                                       // the slabs' loads in flight together (same summation order)
        for (int z = 0; z < p.splitk; ++z) v += p.partial[(size_t)z * total + e];
        v = v * p.scale[n] + p.shift[n];
        const size_t ri = (size_t)(p.res_mod ? m % p.res_mod : m) * p.ldres + n;
        if (p.res) v += HALF_IO ? (float)reinterpret_cast<const _Float16*>(p.res)[ri] : p.res[ri];
        if (p.relu_out) v = fmaxf(v, 0.f);
        if (HALF_IO) reinterpret_cast<_Float16*>(p.out)[(size_t)m * p.ldout + n] = (_Float16)v;
        else p.out[(size_t)m * p.ldout + n] = v;
    }
}

// Cout == 1 (the decoder's mask head, model/modules.py:242): a GEMV per pixel - one wave per output pixel,
// lanes over input channels (float4), wave reduction.  HBM/L2-bound instead of wasting a 64-wide MFMA tile.
template <bool HALF_IN>
__global__ __launch_bounds__(256) void conv_cout1_kernel(ConvArgs p) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= p.M) return;
    const int b = m / p.HoWo, rem = m - b * p.HoWo;
    const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
    float acc = 0.f;
    if (p.KH == 3 && p.KW == 3 && p.Cin <= 256) {
        // 3x3 with one 256-channel chunk per lane group (the mask head: 256 -> 1): the nine taps' loads are requested TOGETHER, from
        // clamped coordinates (a padding tap is selected to zero afterwards).  The general loop below fetches tap after tap behind
        // its bounds branches - nine serialised round trips (round 6).  Same products, same order of additions.
        const int c = lane * 4;
        if (c < p.Cin) {
            f32x4 xv[9], wv[9];
            bool ok[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ih = oh * p.stride - p.pad + t / 3, iw = ow * p.stride - p.pad + t % 3;
                ok[t] = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                const int ihc = min(max(ih, 0), p.H - 1), iwc = min(max(iw, 0), p.W - 1);
                xv[t] = *reinterpret_cast<const f32x4*>(p.in + ((size_t)(b * p.H + ihc) * p.W + iwc) * p.ldin + c);
                wv[t] = *reinterpret_cast<const f32x4*>(p.w + (size_t)t * p.Cin + c);
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (!ok[t]) continue;                  // (no memory operation below: skipping costs nothing)
                if (HALF_IN) {
                    const h16x8 xh = __builtin_bit_cast(h16x8, xv[t]), wh = __builtin_bit_cast(h16x8, wv[t]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float xe = (float)xh[e];
                        if (p.relu_in) xe = fmaxf(xe, 0.f);
                        acc = fmaf(xe, (float)wh[e], acc);
                    }
                } else {
                    f32x4 x = xv[t];
                    if (p.relu_in) { x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f); }
                    acc = fmaf(x.x, wv[t].x, acc); acc = fmaf(x.y, wv[t].y, acc); acc = fmaf(x.z, wv[t].z, acc); acc = fmaf(x.w, wv[t].w, acc);
                }
            }
        }
    } else
    for (int kh = 0; kh < p.KH; ++kh) {
        const int ih = oh * p.stride - p.pad + kh;
        if ((unsigned)ih >= (unsigned)p.H) continue;
        for (int kw = 0; kw < p.KW; ++kw) {
            const int iw = ow * p.stride - p.pad + kw;
            if ((unsigned)iw >= (unsigned)p.W) continue;
            const float* x = p.in + ((size_t)(b * p.H + ih) * p.W + iw) * p.ldin;      // HALF_IN: Cin / ldin count 4-byte units (two halfs)
            const float* w = p.w + (size_t)(kh * p.KW + kw) * p.Cin;
            for (int c = lane * 4; c < p.Cin; c += 256) {
                f32x4 xv = *reinterpret_cast<const f32x4*>(x + c);
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
                if (HALF_IN) {
                    const h16x8 xh = __builtin_bit_cast(h16x8, xv), wh = __builtin_bit_cast(h16x8, wv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float xe = (float)xh[e];
                        if (p.relu_in) xe = fmaxf(xe, 0.f);
                        acc = fmaf(xe, (float)wh[e], acc);
                    }
                } else {
                    if (p.relu_in) { xv.x = fmaxf(xv.x, 0.f); xv.y = fmaxf(xv.y, 0.f); xv.z = fmaxf(xv.z, 0.f); xv.w = fmaxf(xv.w, 0.f); }
                    acc = fmaf(xv.x, wv.x, acc); acc = fmaf(xv.y, wv.y, acc); acc = fmaf(xv.z, wv.z, acc); acc = fmaf(xv.w, wv.w, acc);
                }
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        float v = acc * p.scale[0] + p.shift[0];
        if (p.res) v += p.res[(size_t)(p.res_mod ? m % p.res_mod : m) * p.ldres];
        if (p.relu_out) v = fmaxf(v, 0.f);
        p.out[(size_t)m * p.ldout] = v;
    }
}

// The mask head proper (3x3, stride 1, 256 -> 1 at 1/4 resolution, fp32): one wave per FOUR neighbouring output pixels of a row.  With a
// wave per pixel every wave fetched its own 3 x 3 input vectors and the nine weight vectors: 18 KB through the vector cache for 1 KB of
// new input - 466 MB per launch, 20 us for 60 MFLOP.  Four pixels share a 3 x 6 patch and one set of weights: 27 KB per four pixels
// (3.4x fewer bytes through the cache).  Per pixel the products and the order of the additions are those of conv_cout1_kernel: same bits.
__global__ __launch_bounds__(256) void conv_cout1_row4_kernel(ConvArgs p) {
    const int lane = threadIdx.x & 63;
    const int gpr = (p.Wo + 3) >> 2;                              // groups of four pixels per output row
    const int wid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= p.B * p.Ho * gpr) return;
    const int g = wid % gpr, row = wid / gpr;                     // row = b * Ho + oh
    const int oh = row % p.Ho, b = row / p.Ho;
    const int ow0 = 4 * g;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int c = lane * 4;
    if (c < p.Cin) {
        f32x4 xv[3][6], wv[9];
        bool okr[3], okc[6];
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) okc[cc] = (unsigned)(ow0 - p.pad + cc) < (unsigned)p.W;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int ih = oh - p.pad + r;
            okr[r] = (unsigned)ih < (unsigned)p.H;
            const int ihc = min(max(ih, 0), p.H - 1);
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) {                      // unconditional loads from clamped coordinates, all requested together
                const int iwc = min(max(ow0 - p.pad + cc, 0), p.W - 1);
                xv[r][cc] = *reinterpret_cast<const f32x4*>(p.in + ((size_t)(b * p.H + ihc) * p.W + iwc) * p.ldin + c);
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) wv[t] = *reinterpret_cast<const f32x4*>(p.w + (size_t)t * p.Cin + c);
        if (p.relu_in) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cc = 0; cc < 6; ++cc) {
                    f32x4& x = xv[r][cc];
                    x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f);
                }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int r = t / 3, cc = j + t % 3;
                if (!(okr[r] && okc[cc])) continue;               // a padding tap
                const f32x4 x = xv[r][cc];
                acc[j] = fmaf(x.x, wv[t].x, acc[j]); acc[j] = fmaf(x.y, wv[t].y, acc[j]);
                acc[j] = fmaf(x.z, wv[t].z, acc[j]); acc[j] = fmaf(x.w, wv[t].w, acc[j]);
            }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = wave_sum(acc[j]);
    if (lane < 4 && ow0 + lane < p.Wo) {
        const float a = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
        const int m = row * p.Wo + ow0 + lane;
        float v = a * p.scale[0] + p.shift[0];
        if (p.res) v += p.res[(size_t)(p.res_mod ? m % p.res_mod : m) * p.ldres];
        if (p.relu_out) v = fmaxf(v, 0.f);
        p.out[(size_t)m * p.ldout] = v;
    }
}

// The end of the decoder in ONE launch (xmem_mask_head_gather): the mask head, the input of HiddenUpdater's fused pointwise convolution and
// the hidden-state half of `cat`.  The mask head read relu(g4) through its 3x3 window and hidden_gather_kernel read the same g4 (26.5 MB
// at 480p, the largest tensor of the tail) again for the 4x4 block means, one launch after the other on the decoder's chain.  A pixel
// (k, y, x) of the 1/16 map owns one 4x4 block of g4 and of the logits, one 2x2 block of g8 and one pixel of g16: ONE WAVE per such pixel
// loads the 6x6 patch of g4 around its block once (clamped coordinates, all 36 + 9 weight loads requested together) and makes from it
//   - area4(g4) from the un-relu'd interior, in hidden_gather_kernel's order (dy, then dx, then one multiply by 1/16),
//   - the 16 logits, per pixel the products and the order of the additions of conv_cout1_row4_kernel / conv_cout1_kernel (taps 0..8 with
//     the padding taps skipped, x y z w fma chain, wave_sum, a * scale + shift),
//   - area4(logits) from its own 16 results (row by row, x y z w, times 1/16),
// and copies g16, area2(g8) and the hidden state, float4 groups dealt over the lanes, their loads requested BEFORE the first of their stores
// (a store may alias a later load for all the compiler knows: one round trip per group otherwise).
// The same bits as conv2d + xmem_hidden_update_gather + xmem_copy_channels; channels of g4d past c16 + c8 + c4 + 1 are not written.
struct MaskTailArgs {
    const float *g16, *g8, *g4, *w, *scale, *shift, *hidden;
    float *logits, *g4d, *cat;
    int c16, c8, c4, hd, ldg, ldcat, K, h, wd;
};

__global__ __launch_bounds__(64, 2) void conv_cout1_tail_kernel(MaskTailArgs p) {
    const int lane = threadIdx.x;
    const size_t pix = blockIdx.x;                                // (k * h + y) * w + x of the 1/16 map
    const int x = (int)(pix % p.wd); const size_t ky = pix / p.wd;
    const int y = (int)(ky % p.h);
    const int W4 = 4 * p.wd;
    const int c = lane * 4;
    const bool act = c < p.c4;
    // rows / columns 1..4 of the patch are the wave's own block: only the halo can fall outside the map
    const bool okr0 = y > 0, okr5 = y < p.h - 1, okc0 = x > 0, okc5 = x < p.wd - 1;
    f32x4 xv[6][6], wv[9];
    const float sc = p.scale[0], sf = p.shift[0];                 // (read before the first store: after one they could not be scalar loads)
    if (act) {
        const float* base = p.g4 + ((4 * ky) * (size_t)W4 + 4 * x) * p.c4 + c;       // the block's first pixel
        const long rowl = (long)W4 * p.c4;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const long ro = (r == 0 ? (okr0 ? -1 : 0) : r == 5 ? (okr5 ? 4 : 3) : r - 1) * rowl;
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) {
                const long co = (long)(cc == 0 ? (okc0 ? -1 : 0) : cc == 5 ? (okc5 ? 4 : 3) : cc - 1) * p.c4;
                xv[r][cc] = *reinterpret_cast<const f32x4*>(base + ro + co);
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) wv[t] = *reinterpret_cast<const f32x4*>(p.w + (size_t)t * p.c4 + c);
    }
    // [ g16 | area2(g8) ] -> g4d, hidden -> cat: float4 groups dealt over the lanes.  The first 128 groups of g16 and the first 64 of g8 and of
    // the hidden state (all there are at the served sizes) are straight-line code - every load requested here, the stores further down; a loop
    // makes each pass wait for the one before it.  What is left over goes group by group at the end of the kernel.
    const int n16 = p.c16 >> 2, n8 = p.c8 >> 2, nh = p.hd >> 2;
    float* const o = p.g4d + pix * p.ldg;
    float* const oh = p.cat + pix * p.ldcat;
    const float* const s16 = p.g16 + pix * p.c16;
    const float* const s8 = p.g8 + ((2 * ky) * (size_t)(2 * p.wd) + 2 * x) * p.c8;
    const float* const sh = p.hidden + pix * p.hd;
    const size_t row8 = (size_t)(2 * p.wd) * p.c8;
    const bool a0 = lane < n16, a1 = lane + 64 < n16, b0 = lane < n8, h0 = lane < nh;
    f32x4 va0, va1, vb[4], vh;
    if (a0) va0 = *reinterpret_cast<const f32x4*>(s16 + 4 * lane);
    if (a1) va1 = *reinterpret_cast<const f32x4*>(s16 + 4 * (lane + 64));
    if (h0) vh = *reinterpret_cast<const f32x4*>(sh + 4 * lane);
    if (b0) {
        const float* src = s8 + 4 * lane;
        vb[0] = *reinterpret_cast<const f32x4*>(src); vb[1] = *reinterpret_cast<const f32x4*>(src + p.c8);
        vb[2] = *reinterpret_cast<const f32x4*>(src + row8); vb[3] = *reinterpret_cast<const f32x4*>(src + row8 + p.c8);
    }
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    if (act) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) s += xv[1 + dy][1 + dx];
        *reinterpret_cast<f32x4*>(p.g4d + pix * p.ldg + p.c16 + p.c8 + c) = s * 0.0625f;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int cc = 0; cc < 6; ++cc) {
                f32x4& v = xv[r][cc];
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
#pragma unroll
        for (int j = 0; j < 16; ++j)
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int r = (j >> 2) + t / 3, cc = (j & 3) + t % 3;
                if ((r == 0 && !okr0) || (r == 5 && !okr5) || (cc == 0 && !okc0) || (cc == 5 && !okc5)) continue;      // a padding tap
                const f32x4 v = xv[r][cc];
                acc[j] = fmaf(v.x, wv[t].x, acc[j]); acc[j] = fmaf(v.y, wv[t].y, acc[j]);
                acc[j] = fmaf(v.z, wv[t].z, acc[j]); acc[j] = fmaf(v.w, wv[t].w, acc[j]);
            }
    }
    // (the copies are stored after the arithmetic: nothing of it then waits for a store to land)
    if (a0) *reinterpret_cast<f32x4*>(o + 4 * lane) = va0;
    if (a1) *reinterpret_cast<f32x4*>(o + 4 * (lane + 64)) = va1;
    if (b0) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        s += vb[0]; s += vb[1]; s += vb[2]; s += vb[3];
        *reinterpret_cast<f32x4*>(o + p.c16 + 4 * lane) = s * 0.25f;
    }
    if (h0) *reinterpret_cast<f32x4*>(oh + 4 * lane) = vh;
    float lsum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float a = wave_sum(acc[j]);                         // every lane holds the sum
        acc[j] = a * sc + sf;
        lsum += acc[j];
    }
    if (lane < 4) {                                               // lane dy stores row dy of the block (4 x is a multiple of 4 floats: aligned)
        f32x4 v;
        v.x = lane == 0 ? acc[0] : lane == 1 ? acc[4] : lane == 2 ? acc[8] : acc[12];
        v.y = lane == 0 ? acc[1] : lane == 1 ? acc[5] : lane == 2 ? acc[9] : acc[13];
        v.z = lane == 0 ? acc[2] : lane == 1 ? acc[6] : lane == 2 ? acc[10] : acc[14];
        v.w = lane == 0 ? acc[3] : lane == 1 ? acc[7] : lane == 2 ? acc[11] : acc[15];
        *reinterpret_cast<f32x4*>(p.logits + (4 * ky + lane) * (size_t)W4 + 4 * x) = v;
    }
    if (lane == 4) p.g4d[pix * p.ldg + p.c16 + p.c8 + p.c4] = lsum * 0.0625f;
    // the left-over groups of wider tensors (none at the served sizes)
    for (int g = lane + 128; g < n16; g += 64) *reinterpret_cast<f32x4*>(o + 4 * g) = *reinterpret_cast<const f32x4*>(s16 + 4 * g);
    for (int g = lane + 64; g < n8; g += 64) {
        const float* src = s8 + 4 * g;
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(src), q1 = *reinterpret_cast<const f32x4*>(src + p.c8);
        const f32x4 q2 = *reinterpret_cast<const f32x4*>(src + row8), q3 = *reinterpret_cast<const f32x4*>(src + row8 + p.c8);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        s += q0; s += q1; s += q2; s += q3;
        *reinterpret_cast<f32x4*>(o + p.c16 + 4 * g) = s * 0.25f;
    }
    for (int g = lane + 64; g < nh; g += 64) *reinterpret_cast<f32x4*>(oh + 4 * g) = *reinterpret_cast<const f32x4*>(sh + 4 * g);
}

// ----------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) for the 3x3 / stride 1 / pad 1 convolutions (85 % of the network's FLOPs):
//   Y = A^T [ (G g G^T) .* (B^T d B) ] A      (Lavin & Gray) - 16 multiplies per 2x2 outputs instead of 36.
// The element-wise product over channels is 16 independent GEMMs [tiles x Cin] x [Cin x Cout] that run on the same
// MFMA kernel (blockIdx.y = tile position), between two HBM-bound transform kernels.  All fp32.
// ----------------------------------------------------------------------------------------------
__global__ void wino_input_kernel(const float* __restrict__ in, int ldin, int B, int H, int W, int C, int th, int tw,
                                  int relu_in, float* __restrict__ V, int split) {
    const int C4 = C >> 2;
    const size_t P = (size_t)B * th * tw;
    const size_t total = P * C4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(e % C4);
        size_t t = e / C4;
        const int tx = (int)(t % tw); size_t r = t / tw;
        const int ty = (int)(r % th);
        const int b = (int)(r / th);
        f32x4 d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ih = 2 * ty - 1 + i;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iw = 2 * tx - 1 + j;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                    v = *reinterpret_cast<const f32x4*>(in + (((size_t)b * H + ih) * W + iw) * ldin + c4 * 4);
                d[i][j] = v;
            }
        }
        // relu AFTER every load has been requested: a relu inside the load loop sits behind a (uniform) branch of its own, which
        // makes each load wait for its predecessor's max - 16 / 36 serialised round trips (round 6: 17.3 -> 10 us at 30x54x512)
        if (relu_in) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4 v = d[i][j];
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    d[i][j] = v;
                }
        }
        f32x4 u[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {          // B^T d (rows)
            u[0][j] = d[0][j] - d[2][j];
            u[1][j] = d[1][j] + d[2][j];
            u[2][j] = d[2][j] - d[1][j];
            u[3][j] = d[1][j] - d[3][j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {          // (B^T d) B (columns)
            f32x4 v0 = u[i][0] - u[i][2], v1 = u[i][1] + u[i][2], v2 = u[i][2] - u[i][1], v3 = u[i][1] - u[i][3];
            if (split) { v0 = split_pack(v0); v1 = split_pack(v1); v2 = split_pack(v2); v3 = split_pack(v3); }   // 'fp32x' mode
            float* o = V + ((size_t)(i * 4) * P + t) * C + c4 * 4;
            *reinterpret_cast<f32x4*>(o) = v0;
            *reinterpret_cast<f32x4*>(o + P * C) = v1;
            *reinterpret_cast<f32x4*>(o + 2 * P * C) = v2;
            *reinterpret_cast<f32x4*>(o + 3 * P * C) = v3;
        }
    }
}

__global__ void wino_output_kernel(const float* __restrict__ Mt, int B, int Ho, int Wo, int Cout, int th, int tw,
                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                   const float* __restrict__ res, int ldres, int res_bcast, int relu_out, float* __restrict__ out, int ldout) {
    const int N4 = Cout >> 2;
    const size_t P = (size_t)B * th * tw;
    const size_t total = P * N4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int n4 = (int)(e % N4);
        size_t t = e / N4;
        const int tx = (int)(t % tw); size_t r = t / tw;
        const int ty = (int)(r % th);
        const int b = (int)(r / th);
        // the residual values are requested FIRST, together with the M planes: fetched inside the store loop each one sits behind the
        // bounds branches of its pixel and costs a round trip of its own (round 6: 13.4 -> ~9 us at 60x108x256 with a residual)
        f32x4 rv[2][2];
        if (res) {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int oh = min(2 * ty + dy, Ho - 1), ow = min(2 * tx + dx, Wo - 1);      // clamped: never stored when outside
                    const size_t pix = ((size_t)b * Ho + oh) * Wo + ow;
                    rv[dy][dx] = *reinterpret_cast<const f32x4*>(res + (res_bcast ? (size_t)oh * Wo + ow : pix) * ldres + n4 * 4);
                }
        }
        f32x4 m[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                m[i][j] = *reinterpret_cast<const f32x4*>(Mt + ((size_t)(i * 4 + j) * P + t) * Cout + n4 * 4);
        f32x4 s0[4], s1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {          // A^T m
            s0[j] = m[0][j] + m[1][j] + m[2][j];
            s1[j] = m[1][j] - m[2][j] - m[3][j];
        }
        f32x4 y[2][2];
        y[0][0] = s0[0] + s0[1] + s0[2]; y[0][1] = s0[1] - s0[2] - s0[3];
        y[1][0] = s1[0] + s1[1] + s1[2]; y[1][1] = s1[1] - s1[2] - s1[3];
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + n4 * 4);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + n4 * 4);
        // two phases (see the epilogue of conv_mfma_kernel): every loaded operand is consumed before the first store, so no store waits
        // for its predecessor (loads and stores share the in-order vmcnt counter; a wait inside a bounds branch is a vmcnt(0))
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                f32x4 v = y[dy][dx] * sc + sh;
                if (res) v += rv[dy][dx];
                if (relu_out) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                y[dy][dx] = v;
            }
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int oh = 2 * ty + dy;
            if (oh >= Ho) continue;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int ow = 2 * tx + dx;
                if (ow >= Wo) continue;
                const size_t pix = ((size_t)b * Ho + oh) * Wo + ow;
                *reinterpret_cast<f32x4*>(out + pix * ldout + n4 * 4) = y[dy][dx];
            }
        }
    }
}

// Fused Winograd-domain GEMM + output transform.  One workgroup owns a (tile-pixel block x Cout block) and walks all 16
// tile positions xi = (i, j) as ONE long K loop of 16 * Cin/BK staged tiles: after each position the 32x32 accumulator
// M_xi is folded into the four output-position accumulators  Y[a][b] += At[a][i] * At[b][j] * M_xi  (At entries are
// 0 / +-1), so the [16][tiles][Cout] intermediate never exists and prologue / epilogue are amortised over a 16x deeper
// loop than the per-position GEMMs.  A = V[xi][m][k] (from wino_input_kernel), B = U[xi][n][k] = (G g G^T).
struct WinoArgs {
    const float* V; const float* U; const float* scale; const float* shift; const float* res; float* out;
    int P, Cin, Cout, B, Ho, Wo, th, tw, ldout, ldres, relu_out, nk, tiles_m, tiles_n, res_bcast;
};

template <int BM, int BN, int TM, int TN, int BK>
__global__ __launch_bounds__(256) void wino_fused_kernel(WinoArgs p) {
    constexpr int WN = BN / (32 * TN);
    constexpr int WM = BM / (32 * TM);
    static_assert(WM * WN == 4, "four waves per workgroup");
    constexpr int LDK = BK + 4;
    constexpr int C4 = BK / 4;
    constexpr int RPP = 256 / C4;
    constexpr int RA = BM / RPP, RB = BN / RPP;
    constexpr int BUF = (BM + BN) * LDK;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lh = lane >> 5;
    const int lrow = tid / C4, c4 = tid % C4;

    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int tile_n = bid % p.tiles_n, tile_m = bid / p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const size_t vstride = (size_t)p.P * p.Cin, ustride = (size_t)p.Cout * p.Cin;
    f32x4 ra[RA], rb[RB];
    auto load_tile = [&](int it) {
        const int xi = it / p.nk, kt = it - xi * p.nk;
        const int k = kt * BK + c4 * 4;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const float* va = p.V + (size_t)xi * vstride + k;
        const float* ub = p.U + (size_t)xi * ustride + k;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const int m = m0 + lrow + RPP * i;
            ra[i] = (m < p.P && k < p.Cin) ? *reinterpret_cast<const f32x4*>(va + (size_t)m * p.Cin) : zero;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int n = n0 + lrow + RPP * i;
            rb[i] = (n < p.Cout && k < p.Cin) ? *reinterpret_cast<const f32x4*>(ub + (size_t)n * p.Cin) : zero;
        }
    };
    auto store_tile = [&](int buf) {
        float* As = smem + buf * BUF;
        float* Bs = As + BM * LDK;
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4*>(&As[(lrow + RPP * i) * LDK + c4 * 4]) = ra[i];
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(&Bs[(lrow + RPP * i) * LDK + c4 * 4]) = rb[i];
    };

    f32x16 acc[TM][TN];
    f32x16 y[4][TM][TN];                       // output positions (a, b) = (o >> 1, o & 1)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int r = 0; r < 16; ++r) y[o][i][j][r] = 0.f;
        }

    const int total = 16 * p.nk;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    int kt_in_xi = 0, xi = 0;
    for (int it = 0; it < total; ++it) {
        const int buf = it & 1;
        const bool has_next = it + 1 < total;
        if (has_next) load_tile(it + 1);
        const float* As = smem + buf * BUF + (wm * 32 * TM + l31) * LDK + lh * 4;
        const float* Bs = smem + buf * BUF + BM * LDK + (wn * 32 * TN + l31) * LDK + lh * 4;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            f32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(As + i * 32 * LDK + kk * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * LDK + kk * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
        }
        if (++kt_in_xi == p.nk) {              // position finished: Y[a][b] += At[a][i] * At[b][j] * M_xi
            const int wi = xi >> 2, wj = xi & 3;
            // At = [1 1 1 0; 0 1 -1 -1]
            const float a0 = (wi < 3) ? 1.f : 0.f, a1 = (wi == 0) ? 0.f : (wi == 1 ? 1.f : -1.f);
            const float b0 = (wj < 3) ? 1.f : 0.f, b1 = (wj == 0) ? 0.f : (wj == 1 ? 1.f : -1.f);
            const float c00 = a0 * b0, c01 = a0 * b1, c10 = a1 * b0, c11 = a1 * b1;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = acc[i][j][r];
                        y[0][i][j][r] = fmaf(c00, v, y[0][i][j][r]);
                        y[1][i][j][r] = fmaf(c01, v, y[1][i][j][r]);
                        y[2][i][j][r] = fmaf(c10, v, y[2][i][j][r]);
                        y[3][i][j][r] = fmaf(c11, v, y[3][i][j][r]);
                        acc[i][j][r] = 0.f;
                    }
                }
            kt_in_xi = 0; ++xi;
        }
        if (has_next) store_tile(buf ^ 1);
        __syncthreads();
    }

    // epilogue: lane owns output channel n and 16 tile-pixels per 32x32 tile; each tile-pixel is 2x2 outputs
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * 32 * TN + j * 32 + l31;
        if (n >= p.Cout) continue;
        const float sc = p.scale[n], sh = p.shift[n];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= p.P) continue;
                const int tx = m % p.tw; const int t2 = m / p.tw;
                const int ty = t2 % p.th; const int b = t2 / p.th;
                // two phases (see the epilogue of conv_mfma_kernel): residual values first (clamped addresses), then the four stores
                float vv[4];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int oh = min(2 * ty + (o >> 1), p.Ho - 1), ow = min(2 * tx + (o & 1), p.Wo - 1);
                    const size_t pix = ((size_t)b * p.Ho + oh) * p.Wo + ow;
                    float v = y[o][i][j][r] * sc + sh;
                    if (p.res) v += p.res[(p.res_bcast ? (size_t)oh * p.Wo + ow : pix) * p.ldres + n];
                    vv[o] = p.relu_out ? fmaxf(v, 0.f) : v;
                }
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    const int oh = 2 * ty + (o >> 1), ow = 2 * tx + (o & 1);
                    if (oh >= p.Ho || ow >= p.Wo) continue;
                    const size_t pix = ((size_t)b * p.Ho + oh) * p.Wo + ow;
                    p.out[pix * p.ldout + n] = vv[o];
                }
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------
// Winograd F(4x4, 3x3) for the LARGE 3x3 / stride 1 layers (plan_tile 17..28): 36 multiplies per 4x4 outputs instead of
// 144 - 4x fewer MFMA FLOPs than the direct form (F(2x2): 2.25x) and 2.25 / 4 of F(2x2)'s transform-domain traffic
// (36 values per 16 outputs instead of 16 per 4).  All fp32.
//   V = B^T d B (6x6 input tile, stride 4), M_xi = V_xi U_xi^T on the same MFMA GEMM (36 groups), Y = A^T M A (4x4).
// INTERPOLATION POINTS {0, +-3/4, +-3/2, inf} (round 5; rounds 2-4: the textbook {0, +-1, +-2, inf}).  The error of a Winograd
// convolution is set by the magnitudes in A, B, G, i.e. by the points (Barabasz et al., "Error analysis and improving the accuracy
// of Winograd convolution for DNNs", 2018): with +-1, +-2 the output transform multiplies by up to 8 and the input transform by up to
// 5; with +-3/4, +-3/2 every coefficient of A^T is <= 3.375 and of B^T <= 2.8125.  Simulated in fp32 against an fp64 convolution
// (relu'd normal inputs, Cin 64 / 512 / 1600): max error / max |y| 2.5e-6 / 5.0e-6 / 8.6e-6 -> 7.4e-7 / 1.4e-6 / 2.3e-6 (3.4-3.7x
// lower, rms 2x lower) - the level of F(2x2) and of the direct form's own fp32 summation.  It matters: on the 3-object 480p clip
// (multi-object conditioning) the textbook points cost 73 argmax pixels against the oracle where the reference disagrees with
// itself on 20 and F(2x2) on 1 (profiles/r05_c3_parity_by_plan.txt).  All powers of 3/4 and 3/2 are exact in fp32, so B^T and A^T
// below are exact constants; the non-dyadic factors (1 / N_i) live in G, applied once at load time in fp64 (ops.winograd4_weights).
// Rows of B^T = coefficients of the monic polynomials prod_{k != i} (x - p_k); rows of A^T = powers of the points:
//   p = (0, a, -a, b, -b, inf), a = 3/4, b = 3/2
// ----------------------------------------------------------------------------------------------
#define W4_A 0.75f
#define W4_B 1.5f
#define W4_A2 0.5625f          // a^2
#define W4_B2 2.25f            // b^2
#define W4_A3 0.421875f        // a^3
#define W4_B3 3.375f           // b^3
#define W4_A2B2 1.265625f      // a^2 b^2
#define W4_SUM 2.8125f         // a^2 + b^2
#define W4_AB2 1.6875f         // a b^2
#define W4_BA2 0.84375f        // b a^2
template <typename T>
__device__ __forceinline__ void wino4_bt(const T* d, T* t) {              // t = B^T d for one 6-vector
    t[0] = W4_A2B2 * d[0] - W4_SUM * d[2] + d[4];
    t[1] = -W4_AB2 * d[1] - W4_B2 * d[2] + W4_A * d[3] + d[4];
    t[2] = W4_AB2 * d[1] - W4_B2 * d[2] - W4_A * d[3] + d[4];
    t[3] = -W4_BA2 * d[1] - W4_A2 * d[2] + W4_B * d[3] + d[4];
    t[4] = W4_BA2 * d[1] - W4_A2 * d[2] - W4_B * d[3] + d[4];
    t[5] = W4_A2B2 * d[1] - W4_SUM * d[3] + d[5];
}
template <typename T>
__device__ __forceinline__ void wino4_at(const T* m, T* s) {              // s = A^T m for one 6-vector
    s[0] = m[0] + m[1] + m[2] + m[3] + m[4];
    s[1] = W4_A * m[1] - W4_A * m[2] + W4_B * m[3] - W4_B * m[4];
    s[2] = W4_A2 * m[1] + W4_A2 * m[2] + W4_B2 * m[3] + W4_B2 * m[4];
    s[3] = W4_A3 * m[1] - W4_A3 * m[2] + W4_B3 * m[3] - W4_B3 * m[4] + m[5];
}

// blockIdx.y = 1 (xmem_conv2d_shared_input): the same transform with the activation flag `relu_in2` into `V2` - sibling convolutions
// that read one tensor get the V of both variants (raw, relu) from ONE launch; the second read of a patch is served by the L2.
__global__ __launch_bounds__(256) void wino4_input_kernel(const float* __restrict__ in, int ldin, int B, int H, int W, int C, int th, int tw,
                                                          int relu_in, float* __restrict__ V, int split, float* __restrict__ V2, int relu_in2) {
    if (blockIdx.y) { V = V2; relu_in = relu_in2; }
    const int C4 = C >> 2;
    const size_t P = (size_t)B * th * tw;
    const size_t total = P * C4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(e % C4);
        size_t t = e / C4;
        const int tx = (int)(t % tw); size_t r = t / tw;
        const int ty = (int)(r % th);
        const int b = (int)(r / th);
        f32x4 d[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int ih = 4 * ty - 1 + i;
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int iw = 4 * tx - 1 + j;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                    v = *reinterpret_cast<const f32x4*>(in + (((size_t)b * H + ih) * W + iw) * ldin + c4 * 4);
                d[i][j] = v;
            }
        }
        if (relu_in) {                                 // after the loads, not between them (see wino_input_kernel)
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    f32x4 v = d[i][j];
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    d[i][j] = v;
                }
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {              // columns: d[:, j] <- B^T d[:, j]
            f32x4 col[6], tc[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) col[i] = d[i][j];
            wino4_bt(col, tc);
#pragma unroll
            for (int i = 0; i < 6; ++i) d[i][j] = tc[i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {              // rows: (B^T d) B, stored to the 36 position planes
            f32x4 tr[6];
            wino4_bt(d[i], tr);
#pragma unroll
            for (int j = 0; j < 6; ++j)
                *reinterpret_cast<f32x4*>(V + ((size_t)(i * 6 + j) * P + t) * C + c4 * 4) = split ? split_pack(tr[j]) : tr[j];
        }
    }
}

__global__ __launch_bounds__(256) void wino4_output_kernel(const float* __restrict__ Mt, int B, int Ho, int Wo, int Cout, int th, int tw,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ res, int ldres, int res_bcast, int relu_out,
                                                           float* __restrict__ out, int ldout) {
    const int N4 = Cout >> 2;
    const size_t P = (size_t)B * th * tw;
    const size_t total = P * N4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int n4 = (int)(e % N4);
        size_t t = e / N4;
        const int tx = (int)(t % tw); size_t r = t / tw;
        const int ty = (int)(r % th);
        const int b = (int)(r / th);
        f32x4 rv[4][4];                            // residual values, requested before the M planes (see wino_output_kernel)
        if (res) {
#pragma unroll
            for (int dy = 0; dy < 4; ++dy)
#pragma unroll
                for (int dx = 0; dx < 4; ++dx) {
                    const int oh = min(4 * ty + dy, Ho - 1), ow = min(4 * tx + dx, Wo - 1);      // clamped: never stored when outside
                    const size_t pix = ((size_t)b * Ho + oh) * Wo + ow;
                    rv[dy][dx] = *reinterpret_cast<const f32x4*>(res + (res_bcast ? (size_t)oh * Wo + ow : pix) * ldres + n4 * 4);
                }
        }
        f32x4 s[4][6];                             // A^T m, column by column
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            f32x4 col[6], sc[4];
#pragma unroll
            for (int i = 0; i < 6; ++i) col[i] = *reinterpret_cast<const f32x4*>(Mt + ((size_t)(i * 6 + j) * P + t) * Cout + n4 * 4);
            wino4_at(col, sc);
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i][j] = sc[i];
        }
        const f32x4 scl = *reinterpret_cast<const f32x4*>(scale + n4 * 4);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + n4 * 4);
        // two phases (see the epilogue of conv_mfma_kernel): the 16 outputs are finished in the residual registers first ...
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            f32x4 y[4];
            wino4_at(s[dy], y);
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                f32x4 v = y[dx] * scl + sh;
                if (res) v += rv[dy][dx];
                if (relu_out) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                rv[dy][dx] = v;
            }
        }
        // ... then stored: no store depends on a load any more, none waits for its predecessor
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const int oh = 4 * ty + dy;
            if (oh >= Ho) continue;
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                const int ow = 4 * tx + dx;
                if (ow >= Wo) continue;
                const size_t pix = ((size_t)b * Ho + oh) * Wo + ow;
                *reinterpret_cast<f32x4*>(out + pix * ldout + n4 * 4) = rv[dy][dx];
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------
// SHARED TRANSFORMS (xmem_conv2d_shared_input, xmem_conv2d_nhwc_folded).  Sibling convolutions of a residual block read the same
// tensor: conv1(relu(g)) and downsample(g), and in the batched key pass three layers read f16.  One launch of wino4_input_kernel
// (blockIdx.y: the variant) writes the V of both activation variants; and the branch's output transform is formed inside the main
// convolution's (below), instead of being stored and read back as its residual.  The fold works on TWO channels per lane: two M
// sets and the branch residual requested together would not fit the 256 VGPRs at four.  Per channel its operations and their order
// are those of wino4_output_kernel.
// (The input side deliberately re-runs the UNCHANGED transform code per variant instead of forming both from one loaded patch: the
// compiler contracts a*b + c into fma depending on the code around the expression - even the raw and the relu body of
// wino4_input_kernel are contracted differently - and a kernel that formed both variants from one patch, two channels per lane,
// differed from the separate launches in the last bit of 39 % of a layer's outputs on the MI355X.  Bit-identity with the separate
// convolutions is the contract; the merged launch keeps the launch it saves, the second read of the patch comes from the L2.)
// ----------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct WinoFoldArgs {
    const float* Mt; const float* Mb;                  // [36][P][Cout] of the main convolution and of the branch
    const float* scale; const float* shift;            // main epilogue
    const float* scale_b; const float* shift_b; const float* res_b;      // branch epilogue
    float* out;
    int B, Ho, Wo, Cout, th, tw, ldout, relu_out, ldres_b, res_b_bcast, relu_b;
};

// out = [relu](A^T M A * sc + sh + r), r = [relu_b](A^T M_b A * sc_b + sh_b [+ res_b]): what wino4_output_kernel computes for the
// branch, kept in registers, and then for the main convolution with r as its residual
__global__ __launch_bounds__(256) void wino4_output_fold_kernel(WinoFoldArgs p) {
    const int N2 = p.Cout >> 1;
    const size_t P = (size_t)p.B * p.th * p.tw;
    const size_t total = P * N2;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int n2 = (int)(e % N2);
        size_t t = e / N2;
        const int tx = (int)(t % p.tw); size_t r = t / p.tw;
        const int ty = (int)(r % p.th);
        const int b = (int)(r / p.th);
        f32x2 rv[4][4], mm[6][6], mb[6][6];            // every load of the item is requested before the first arithmetic
        if (p.res_b) {
#pragma unroll
            for (int dy = 0; dy < 4; ++dy)
#pragma unroll
                for (int dx = 0; dx < 4; ++dx) {
                    const int oh = min(4 * ty + dy, p.Ho - 1), ow = min(4 * tx + dx, p.Wo - 1);  // clamped: never stored when outside
                    const size_t pix = ((size_t)b * p.Ho + oh) * p.Wo + ow;
                    rv[dy][dx] = *reinterpret_cast<const f32x2*>(p.res_b + (p.res_b_bcast ? (size_t)oh * p.Wo + ow : pix) * p.ldres_b + n2 * 2);
                }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const size_t off = ((size_t)(i * 6 + j) * P + t) * p.Cout + n2 * 2;
                mb[i][j] = *reinterpret_cast<const f32x2*>(p.Mb + off);
                mm[i][j] = *reinterpret_cast<const f32x2*>(p.Mt + off);
            }
        const f32x2 sclb = *reinterpret_cast<const f32x2*>(p.scale_b + n2 * 2), shb = *reinterpret_cast<const f32x2*>(p.shift_b + n2 * 2);
        const f32x2 scl = *reinterpret_cast<const f32x2*>(p.scale + n2 * 2), sh = *reinterpret_cast<const f32x2*>(p.shift + n2 * 2);
        f32x2 s[4][6];
        // the branch: A^T m column by column, then its epilogue into the residual registers
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            f32x2 col[6], sc[4];
#pragma unroll
            for (int i = 0; i < 6; ++i) col[i] = mb[i][j];
            wino4_at(col, sc);
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i][j] = sc[i];
        }
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            f32x2 y[4];
            wino4_at(s[dy], y);
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                f32x2 v = y[dx] * sclb + shb;
                if (p.res_b) v += rv[dy][dx];
                if (p.relu_b) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); }
                rv[dy][dx] = v;
            }
        }
        // the main convolution with the branch as its residual: the 16 outputs are finished in registers ...
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            f32x2 col[6], sc[4];
#pragma unroll
            for (int i = 0; i < 6; ++i) col[i] = mm[i][j];
            wino4_at(col, sc);
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i][j] = sc[i];
        }
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            f32x2 y[4];
            wino4_at(s[dy], y);
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                f32x2 v = y[dx] * scl + sh;
                v += rv[dy][dx];
                if (p.relu_out) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); }
                rv[dy][dx] = v;
            }
        }
        // ... then stored
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const int oh = 4 * ty + dy;
            if (oh >= p.Ho) continue;
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                const int ow = 4 * tx + dx;
                if (ow >= p.Wo) continue;
                const size_t pix = ((size_t)b * p.Ho + oh) * p.Wo + ow;
                *reinterpret_cast<f32x2*>(p.out + pix * p.ldout + n2 * 2) = rv[dy][dx];
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------
// REDUCED-PRECISION MODE (opt-in, plan_tile 16): the Winograd-domain operands V = B^T d B and U = G g G^T are stored in
// fp16 and contracted on v_mfma_f32_32x32x16_f16 (fp32 accumulation, 16x the fp32 MFMA rate); transforms, epilogue and
// every other kernel stay fp32.  Mirrors the reference's fp16-autocast GPU loop (inference/run_on_video.py:76); it is
// outside the fp32 parity contract and is reported under its own bench key.
// ----------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__global__ void wino_input_f16_kernel(const float* __restrict__ in, int ldin, int B, int H, int W, int C, int th, int tw,
                                      int relu_in, _Float16* __restrict__ V) {
    const int C4 = C >> 2;
    const size_t P = (size_t)B * th * tw;
    const size_t total = P * C4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(e % C4);
        size_t t = e / C4;
        const int tx = (int)(t % tw); size_t r = t / tw;
        const int ty = (int)(r % th);
        const int b = (int)(r / th);
        f32x4 d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ih = 2 * ty - 1 + i;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int iw = 2 * tx - 1 + j;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
                    v = *reinterpret_cast<const f32x4*>(in + (((size_t)b * H + ih) * W + iw) * ldin + c4 * 4);
                    if (relu_in) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
                }
                d[i][j] = v;
            }
        }
        f32x4 u[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u[0][j] = d[0][j] - d[2][j];
            u[1][j] = d[1][j] + d[2][j];
            u[2][j] = d[2][j] - d[1][j];
            u[3][j] = d[1][j] - d[3][j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v[4] = {u[i][0] - u[i][2], u[i][1] + u[i][2], u[i][2] - u[i][1], u[i][1] - u[i][3]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f16x4 hv;
                hv.x = (_Float16)v[j].x; hv.y = (_Float16)v[j].y; hv.z = (_Float16)v[j].z; hv.w = (_Float16)v[j].w;
                *reinterpret_cast<f16x4*>(V + ((size_t)(i * 4 + j) * P + t) * C + c4 * 4) = hv;
            }
        }
    }
}

// M[xi][m][n] = sum_k V[xi][m][k] * U[xi][n][k]  (fp16 x fp16 -> fp32).  One workgroup: BM x BN outputs of one tile position,
// 4 waves (2 x 2), wave tile (BM/2) x (BN/2) of 32x32 MFMA blocks, BK = 64 halfs per stage: register-staged global loads one
// stage ahead, single LDS buffer (144-byte rows: an odd multiple of 16 B -> conflict-free ds_read_b128 fragments).
struct WinoF16Args {
    const _Float16* V; const _Float16* U; float* M;
    int P, Cin, Cout, tiles_m, tiles_n;
};

template <int BM, int BN>
__global__ __launch_bounds__(256) void wino_gemm_f16_kernel(WinoF16Args p) {
    constexpr int BK = 64, LDB = 144;                 // bytes per LDS row
    constexpr int TM = BM / 64, TN = BN / 64;         // 32x32 blocks per wave in M / N
    constexpr int CA = BM * 8 / 256, CB = BN * 8 / 256;   // 16-byte chunks per thread per stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    unsigned char* As = smem16;
    unsigned char* Bs = smem16 + BM * LDB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    int bid = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int tile_n = bid % p.tiles_n, tile_m = bid / p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int xi = blockIdx.y;
    const unsigned char* gA = reinterpret_cast<const unsigned char*>(p.V + (size_t)xi * p.P * p.Cin);
    const unsigned char* gB = reinterpret_cast<const unsigned char*>(p.U + (size_t)xi * p.Cout * p.Cin);
    const size_t rowb = (size_t)p.Cin * 2;            // bytes per operand row

    size_t a_off[CA], b_off[CB];
#pragma unroll
    for (int i = 0; i < CA; ++i) {
        const int c = tid + 256 * i, row = c >> 3, ch = c & 7;
        a_off[i] = (size_t)min(m0 + row, p.P - 1) * rowb + ch * 16;       // rows past M are clamped (never stored)
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
        const int c = tid + 256 * i, row = c >> 3, ch = c & 7;
        b_off[i] = (size_t)min(n0 + row, p.Cout - 1) * rowb + ch * 16;
    }
    f32x4 ra[CA], rb[CB];                             // raw 16-byte chunks
    auto load_stage = [&](int kt) {
        const size_t kb = (size_t)kt * BK * 2;
#pragma unroll
        for (int i = 0; i < CA; ++i) ra[i] = *reinterpret_cast<const f32x4*>(gA + a_off[i] + kb);
#pragma unroll
        for (int i = 0; i < CB; ++i) rb[i] = *reinterpret_cast<const f32x4*>(gB + b_off[i] + kb);
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int i = 0; i < CA; ++i) { const int c = tid + 256 * i; *reinterpret_cast<f32x4*>(As + (c >> 3) * LDB + (c & 7) * 16) = ra[i]; }
#pragma unroll
        for (int i = 0; i < CB; ++i) { const int c = tid + 256 * i; *reinterpret_cast<f32x4*>(Bs + (c >> 3) * LDB + (c & 7) * 16) = rb[i]; }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = p.Cin / BK;
    load_stage(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();                              // previous stage's fragment reads are done
        store_stage();
        __syncthreads();
        if (kt + 1 < nk) load_stage(kt + 1);          // next stage in flight under this stage's MFMAs
        const unsigned char* a0 = As + (wm * (BM / 2) + l31) * LDB + lh * 16;
        const unsigned char* b0 = Bs + (wn * (BN / 2) + l31) * LDB + lh * 16;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
            f16x8 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f16x8*>(a0 + i * 32 * LDB + kk * 32);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f16x8*>(b0 + j * 32 * LDB + kk * 32);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }
    float* gM = p.M + (size_t)xi * p.P * p.Cout;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (BN / 2) + j * 32 + l31;
        if (n >= p.Cout) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = m0 + wm * (BM / 2) + i * 32 + 4 * lh;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mb + (r & 3) + 8 * (r >> 2);
                if (m < p.P) gM[(size_t)m * p.Cout + n] = acc[i][j][r];
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------
namespace {

// ---- plan codes ----------------------------------------------------------------------------------------------------------------
// xmem_conv_desc.plan_tile -> what it asks for (include/xmem_hip.h documents the codes; xmem2_amd/conv_plan.py CODES is the Python
// statement of this table, tests/test_conv_plan_host.py holds the two against each other).  ring > 0: the GEMM runs on the
// streaming kernel (csrc/gemm_stream.hip) with that many LDS stages; bm = bn = 0: the tile is chosen from the size; fallback: the
// code that takes over on a layer this one does not apply to (make_plan: applies).
enum { GEMV = XMEM_CONV_GEMV, DIRECT = XMEM_CONV_DIRECT, F2 = XMEM_CONV_F2, F2_FUSED = XMEM_CONV_F2_FUSED, F2_F16 = XMEM_CONV_F2_F16,
       F4 = XMEM_CONV_F4 };
struct PlanCode { int form, bm, bn, bk, ring, fallback; };
// six classic tiles; each falls back to the same tile of the form whose codes start at `fb`
#define XMEM_TILES6(form, fb) {form, 128, 128, 32, 0, fb}, {form, 128, 64, 32, 0, fb + 1}, {form, 64, 64, 32, 0, fb + 2}, \
                              {form, 128, 128, 64, 0, fb + 3}, {form, 128, 64, 64, 0, fb + 4}, {form, 64, 64, 64, 0, fb + 5}
// six streaming variants; all fall back to the classic code `fb`
#define XMEM_STREAM6(form, fb) {form, 64, 64, 32, 3, fb}, {form, 128, 64, 32, 3, fb}, {form, 128, 128, 32, 3, fb}, \
                               {form, 64, 64, 32, 4, fb}, {form, 128, 64, 32, 4, fb}, {form, 128, 128, 32, 4, fb}
constexpr PlanCode kPlanCodes[41] = {
    {DIRECT, 0, 0, 32, 0, 0},                                                       //  0     the heuristic
    XMEM_TILES6(DIRECT, 0),                                                         //  1..6  (apply to every layer)
    XMEM_TILES6(F2, 1),                                                             //  7..12 -> the direct form with the same tile
    {F2_FUSED, 128, 64, 32, 0, 8}, {F2_FUSED, 64, 64, 32, 0, 9}, {F2_FUSED, 64, 128, 32, 0, 9},   // 13..15 -> F(2x2), separate transform
    {F2_F16, 0, 0, 32, 0, 9},                                                       // 16     (its own kernel contracts 64 halfs per k-tile)
    XMEM_TILES6(F4, 7),                                                             // 17..22 -> F(2x2) with the same tile
    XMEM_STREAM6(F4, 19), XMEM_STREAM6(F2, 9), XMEM_STREAM6(DIRECT, 3)              // 23..28, 29..34, 35..40 -> the classic 64x64 tile
};
#undef XMEM_TILES6
#undef XMEM_STREAM6
// a half-typed call (in_half) runs the BK-32 direct tiles only: plan_tile 1..3, 4 = the 256x128 tile (8 waves, planned as code 1),
// 5 / 6 = the tiles of codes 2 / 3, anything else = the heuristic
constexpr int kHalfCodes[7] = {0, 1, 2, 3, 1, 2, 3};

struct Plan { int form, bm, bn, bk, splitk, kt_per_split, nk; bool generic, split; int ring, half; };

inline bool winograd(const Plan& pl) { return pl.form == F2 || pl.form == F2_FUSED || pl.form == F2_F16 || pl.form == F4; }

inline bool wino_ok(const xmem_conv_desc* d) {
    return d->w_winograd && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->Cin % 32 == 0 && d->Cout % 4 == 0 &&
           d->ldout % 4 == 0 && (!d->res || d->ldres % 4 == 0) && (((uintptr_t)d->out) & 15) == 0 && (!d->res || (((uintptr_t)d->res) & 15) == 0);
}

// argument checks common to the plain (dilation 1, codes 0..40) and the dilated (codes 0..6) entry points
int validate(const xmem_conv_desc* d, int dilation = 1, int max_code = 40) {
    if (!d || !d->in || !d->w || !d->scale || !d->shift || !d->out) return XMEM_ERR_BAD_ARG;
    if (dilation <= 0 || d->B <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->KH <= 0 || d->KW <= 0 ||
        d->stride <= 0 || d->pad < 0) return XMEM_ERR_BAD_ARG;
    if (d->Cin % 4 != 0 || d->ldin % 4 != 0 || d->ldin < d->Cin || d->ldout < d->Cout) return XMEM_ERR_UNSUPPORTED;
    if (d->res && d->ldres < d->Cout) return XMEM_ERR_BAD_ARG;
    if ((long)d->H + 2 * d->pad - (long)dilation * (d->KH - 1) - 1 < 0 || (long)d->W + 2 * d->pad - (long)dilation * (d->KW - 1) - 1 < 0)
        return XMEM_ERR_BAD_ARG;
    if (d->plan_tile < 0 || d->plan_tile > max_code || d->plan_splitk < 0) return XMEM_ERR_BAD_ARG;
    return XMEM_OK;
}

inline void out_dims(const xmem_conv_desc* d, int dilation, int& Ho, int& Wo) {
    Ho = (d->H + 2 * d->pad - dilation * (d->KH - 1) - 1) / d->stride + 1;
    Wo = (d->W + 2 * d->pad - dilation * (d->KW - 1) - 1) / d->stride + 1;
}

// The plan of `d` under plan code `code`: the table entry, the fallbacks of a code that does not apply to this layer, the split-K rule.
Plan make_plan(const xmem_conv_desc* d, int code) {
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    const int M = d->B * Ho * Wo, K = d->KH * d->KW * d->Cin;
    Plan pl = {};
    // split-operand arithmetic ('fp32x', opt-in): every GEMM-shaped path; the Cout = 1 GEMV stays fp32 (it is HBM-bound)
    pl.split = d->arith == 1 && d->w_split != nullptr;
    if (d->Cout == 1) { pl.form = GEMV; pl.split = false; pl.bk = 32; pl.nk = cdiv(K, 32); pl.splitk = 1; pl.kt_per_split = pl.nk; return pl; }
    const bool wok = wino_ok(d);
    // does code `c` apply to this layer?  A code that does not hands over to its fallback (kPlanCodes), until one applies.
    auto applies = [&](const PlanCode& c) {
        if (c.ring)              // the streaming kernel: fp32 operands with Cin % 32 == 0; the Winograd position GEMMs, or a 1x1 / pad 0
            return !pl.split && d->Cin % 32 == 0 &&                                // convolution itself (32-bit byte offsets into both operands)
                   (c.form == DIRECT ? (d->KH == 1 && d->KW == 1 && d->pad == 0 && (double)d->B * d->H * d->W * d->ldin * 4.0 < 2.0e9 &&
                                        (double)d->Cout * d->Cin * 4.0 < 2.0e9)
                                     : (wok && (c.form != F4 || d->w_winograd4 != nullptr)));
        const bool f2_ok = wok && (!pl.split || d->w_winograd_split);
        switch (c.form) {
            case F4: return f2_ok && (pl.split ? d->w_winograd4_split : (const void*)d->w_winograd4) != nullptr;
            case F2_F16: return wok && !pl.split && d->w_winograd_f16 && d->Cin % 64 == 0;    // fp16 storage and split mode exclude each other
            case F2_FUSED: return wok && !pl.split;                                           // no split variant of the fused kernel
            case F2: return f2_ok;
            default: return true;
        }
    };
    while (!applies(kPlanCodes[code])) code = kPlanCodes[code].fallback;
    const PlanCode& c = kPlanCodes[code];
    pl.form = c.form; pl.bm = c.bm; pl.bn = c.bn; pl.bk = c.bk; pl.ring = c.ring;
    auto tiles = [&](int bm, int bn) { return (long)cdiv(M, bm) * cdiv(d->Cout, bn); };
    if (code == 0) {
        // 256 CUs; two resident workgroups per CU is the sweet spot for the 128-wide tiles
        if (d->Cout > 64 && tiles(128, 128) >= 384) { pl.bm = 128; pl.bn = 128; }
        else if (tiles(128, 64) >= 384) { pl.bm = 128; pl.bn = 64; }
        else { pl.bm = 64; pl.bn = 64; }
    }
    if (winograd(pl)) {          // the GEMM runs per tile position: M = tiles, K = Cin, no split-K
        pl.generic = pl.form != F2_F16 && (d->Cin % pl.bk) != 0;
        pl.nk = pl.form == F2_F16 ? d->Cin / 64 : cdiv(d->Cin, pl.bk); pl.splitk = 1; pl.kt_per_split = pl.nk;
        return pl;
    }
    pl.generic = (d->Cin % pl.bk) != 0;
    pl.nk = cdiv(K, pl.bk);
    pl.splitk = 1;
    if (d->plan_splitk > 0) {
        pl.splitk = d->plan_splitk < pl.nk ? d->plan_splitk : pl.nk;
    } else {
        const long t = tiles(pl.bm, pl.bn);
        if (t < 384) {
            int want = (int)cdiv(512, (int)t);
            int maxs = pl.nk / (256 / pl.bk); if (maxs < 1) maxs = 1;
            pl.splitk = want < maxs ? want : maxs;
            if (pl.splitk > 16) pl.splitk = 16;
            if (pl.splitk < 1) pl.splitk = 1;
        }
    }
    if (pl.ring) pl.splitk = 1;                    // the streaming kernel contracts the whole K of a unit
    pl.kt_per_split = cdiv(pl.nk, pl.splitk);
    pl.splitk = cdiv(pl.nk, pl.kt_per_split);
    return pl;
}

// fp16 loop: the descriptor as the fp32 machinery sees it - channels in 4-byte units (two halfs), direct plans only
bool half_view(const xmem_conv_desc* d, xmem_conv_desc& v) {
    if (!d->w_half || d->Cin % 8 != 0 || d->ldin % 8 != 0 || (((uintptr_t)d->in) & 15) != 0 || (((uintptr_t)d->w_half) & 15) != 0) return false;
    v = *d;
    v.Cin = d->Cin / 2; v.ldin = d->ldin / 2;
    v.w_winograd = nullptr; v.w_winograd4 = nullptr; v.w_winograd_f16 = nullptr; v.arith = 0; v.w_split = nullptr;
    return true;
}

// plan of a half-typed call (v: its half view); the 256x128 tile keeps the split-K of the 128x128 plan it is made from
Plan make_plan_half(const xmem_conv_desc* v) {
    Plan pl = make_plan(v, v->plan_tile <= 6 ? kHalfCodes[v->plan_tile] : 0);
    if (v->plan_tile == 4 && pl.form == DIRECT) { pl.bm = 256; pl.bn = 128; }
    return pl;
}

// the plan of a validated descriptor; a half-typed call continues on its half view `hv` (false: it has none)
bool plan_of(const xmem_conv_desc*& d, xmem_conv_desc& hv, Plan& pl) {
    if (d->in_half) {
        if (!half_view(d, hv)) return false;
        d = &hv;
        pl = make_plan_half(d);
    } else pl = make_plan(d, d->plan_tile);
    return true;
}

// half output needs half input (the stems stay fp32); the mask head (Cout = 1) writes fp32 logits
inline bool storage_types_ok(const xmem_conv_desc* d) { return d->in_half ? !(d->out_half && d->Cout == 1) : !d->out_half; }

// ---- workspace: one formula per form, for the size queries and the launches ----
inline size_t wino_tiles(const xmem_conv_desc* d, int Ho, int Wo, int r) { return (size_t)d->B * cdiv(Ho, r) * cdiv(Wo, r); }
// V [(r+2)^2][P][Cin] and, unless the GEMM transforms its own output (fused), M [(r+2)^2][P][Cout]
inline size_t wino_workspace(size_t P, int r, int Cin, int Cout, bool fused) {
    return (size_t)(r + 2) * (r + 2) * P * (Cin + (fused ? 0 : Cout)) * sizeof(float);
}
inline size_t wino_f16_v_bytes(size_t P, int Cin) { return align_up((size_t)16 * P * Cin * 2, 256); }
inline size_t splitk_workspace(const Plan& pl, const xmem_conv_desc* d, int Ho, int Wo) {
    return pl.splitk == 1 ? 0 : (size_t)pl.splitk * d->B * Ho * Wo * d->Cout * sizeof(float);
}
size_t workspace_need(const Plan& pl, const xmem_conv_desc* d, int Ho, int Wo) {
    if (pl.form == F4) return wino_workspace(wino_tiles(d, Ho, Wo, 4), 4, d->Cin, d->Cout, false);
    const size_t P = wino_tiles(d, Ho, Wo, 2);
    if (pl.form == F2_F16) return wino_f16_v_bytes(P, d->Cin) + (size_t)16 * P * d->Cout * sizeof(float);
    if (pl.form == F2 || pl.form == F2_FUSED) return wino_workspace(P, 2, d->Cin, d->Cout, pl.form == F2_FUSED);
    return splitk_workspace(pl, d, Ho, Wo);
}

// ---- launches ----
// what both entry points pass to the direct kernels
ConvArgs conv_args(const xmem_conv_desc* d, const Plan& pl, int Ho, int Wo, void* workspace) {
    ConvArgs a;
    a.in = d->in; a.w = d->w; a.scale = d->scale; a.shift = d->shift; a.res = d->res; a.out = d->out;
    a.partial = reinterpret_cast<float*>(workspace);
    a.B = d->B; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.ldin = d->ldin;
    a.Ho = Ho; a.Wo = Wo; a.Cout = d->Cout; a.ldout = d->ldout; a.ldres = d->ldres;
    a.KH = d->KH; a.KW = d->KW; a.stride = d->stride; a.pad = d->pad;
    a.K = d->KH * d->KW * d->Cin; a.M = d->B * Ho * Wo; a.HoWo = Ho * Wo;
    a.relu_in = d->relu_in; a.relu_out = d->relu_out;
    a.nk = pl.nk; a.splitk = pl.splitk; a.kt_per_split = pl.kt_per_split;
    a.tiles_m = pl.bm ? cdiv(a.M, pl.bm) : 0; a.tiles_n = pl.bn ? cdiv(a.Cout, pl.bn) : 0;
    a.raw = 0; a.res_mod = 0; a.in_gstride = 0; a.w_gstride = 0; a.out_gstride = 0;
    a.a_presplit = 0; a.dbg = 0;
    a.dil = 1; a.skip_taps = 0;
    return a;
}

// Transform kernels are grid-stride over (tile, channel quad) items, one item per thread.  A 1/16-resolution layer has ~15 000 items:
// as 256-thread workgroups that is ~60 workgroups on 60 of the 256 CUs, each bound by its own CU's load / store path (measured
// 10-17 us for 12 MB).  Below 512 workgroups of 256 the items are dealt as 64-thread workgroups instead: four times the CUs.
inline void transform_grid(size_t items, int& blocks, int& threads) {
    threads = items < (size_t)512 * 256 ? 64 : 256;
    size_t b = (items + threads - 1) / threads;
    blocks = (int)(b > 16384 ? 16384 : b);
}

// the 1x1 fast path needs 32-bit byte offsets into both operands (per group)
bool conv_is_one(const ConvArgs& a) {
    return a.KH == 1 && a.KW == 1 && a.pad == 0 &&
           (double)a.B * a.H * a.W * a.ldin * 4.0 < 4.0e9 && (double)a.Cout * a.K * 4.0 < 4.0e9;
}

template <int BM, int BN, int TM, int TN, int BK, bool G>
int launch_cfg(const ConvArgs& a, hipStream_t s, int groups, bool split, int half, bool dilated) {
    // (a workgroup that contracts a single k-tile never touches the second buffer: half the LDS, twice the resident workgroups)
    const size_t lds = (a.kt_per_split == 1 ? 1 : 2) * (size_t)(BM + BN) * (BK + 4) * sizeof(float);
    auto kern = conv_mfma_kernel<BM, BN, TM, TN, BK, G, false, false>;
    if (dilated) kern = conv_mfma_kernel<BM, BN, TM, TN, BK, G, false, false, 0, 4, true>;
    else if (half && BK == 32) {                   // fp16 loop: half operands (HALF 1: fp32 output, 2: half output + residual)
        const bool one = !G && conv_is_one(a);
        if (half == 2) kern = one ? conv_mfma_kernel<BM, BN, TM, TN, 32, false, true, false, 2> : conv_mfma_kernel<BM, BN, TM, TN, 32, G, false, false, 2>;
        else kern = one ? conv_mfma_kernel<BM, BN, TM, TN, 32, false, true, false, 1> : conv_mfma_kernel<BM, BN, TM, TN, 32, G, false, false, 1>;
    } else if (split) {
        kern = conv_mfma_kernel<BM, BN, TM, TN, BK, G, false, true>;
        if (!G && conv_is_one(a)) kern = conv_mfma_kernel<BM, BN, TM, TN, BK, false, true, true>;
    } else if (!G && conv_is_one(a)) kern = conv_mfma_kernel<BM, BN, TM, TN, BK, false, true, false>;
    if (xmem_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds) != XMEM_OK) return XMEM_ERR_LAUNCH;
    dim3 grid(a.tiles_m * a.tiles_n, groups, a.splitk);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
    return xmem_check_launch();
}

// fp16 loop only: 256x128 tile, 8 waves (4 x 2, each 64x64 = four accumulators): 1/85 byte of operand traffic per FLOP instead of
// 1/64 - the half kernels are bound by the L2 -> LDS operand stream, not by the matrix pipe
template <bool G>
int launch_half_256(const ConvArgs& a, hipStream_t s, int half) {
    const size_t lds = 2 * (size_t)(256 + 128) * 36 * sizeof(float);
    const bool one = !G && conv_is_one(a);
    auto kern = conv_mfma_kernel<256, 128, 2, 2, 32, G, false, false, 2, 8>;
    if (half == 2) { if (one) kern = conv_mfma_kernel<256, 128, 2, 2, 32, false, true, false, 2, 8>; }
    else kern = one ? conv_mfma_kernel<256, 128, 2, 2, 32, false, true, false, 1, 8> : conv_mfma_kernel<256, 128, 2, 2, 32, G, false, false, 1, 8>;
    if (xmem_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds) != XMEM_OK) return XMEM_ERR_LAUNCH;
    dim3 grid(a.tiles_m * a.tiles_n, 1, a.splitk);
    hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, a);
    return xmem_check_launch();
}

template <int BK, bool G>
int launch_bk(const Plan& pl, const ConvArgs& a, hipStream_t s, int groups, bool dilated) {
    if (pl.bm == 256) return launch_half_256<G>(a, s, pl.half);
    if (pl.bm == 128 && pl.bn == 128) return launch_cfg<128, 128, 2, 2, BK, G>(a, s, groups, pl.split, pl.half, dilated);
    if (pl.bm == 128 && pl.bn == 64) return launch_cfg<128, 64, 2, 1, BK, G>(a, s, groups, pl.split, pl.half, dilated);
    return launch_cfg<64, 64, 1, 1, BK, G>(a, s, groups, pl.split, pl.half, dilated);
}

// the implicit-GEMM kernel of the plan's tile: `groups` GEMMs (blockIdx.y: the Winograd positions), or the dilated form
int launch_tile(const Plan& pl, const ConvArgs& a, hipStream_t s, int groups = 1, bool dilated = false) {
    if (pl.bk == 64) return pl.generic ? launch_bk<64, true>(pl, a, s, groups, dilated) : launch_bk<64, false>(pl, a, s, groups, dilated);
    return pl.generic ? launch_bk<32, true>(pl, a, s, groups, dilated) : launch_bk<32, false>(pl, a, s, groups, dilated);
}

int launch_splitk_reduce(const ConvArgs& a, bool half_out, hipStream_t s) {
    const size_t total = (size_t)a.M * a.Cout;
    int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096;
    if (half_out) hipLaunchKernelGGL(conv_splitk_reduce_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv_splitk_reduce_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
    return xmem_check_launch();
}

int stream_variant(const Plan& pl) { return pl.bm == 64 ? 0 : (pl.bn == 64 ? 1 : 2); }     // gemm_stream.hpp: 64x64, 128x64, 128x128

// The (r+2)^2 position GEMMs M[xi] = V[xi] U[xi]^T of [P x Cin] x [Cin x Cout]: on the plan's tile of the implicit-GEMM kernel, or
// on the streaming kernel.
int wino_position_gemm(const Plan& pl, const xmem_conv_desc* d, const ConvArgs& a, int r, const float* V, float* Mt, size_t P, hipStream_t s) {
    const int G = (r + 2) * (r + 2);
    const float* U = r == 4 ? d->w_winograd4 : d->w_winograd;
    const void* U_split = r == 4 ? d->w_winograd4_split : d->w_winograd_split;
    if (pl.ring) {
        GemmStreamArgs g = {};
        g.A = V; g.B = U; g.C = Mt;
        g.a_gstride = (long)P * d->Cin; g.b_gstride = (long)d->Cout * d->Cin; g.c_gstride = (long)P * d->Cout;
        g.M = (int)P; g.N = d->Cout; g.K = d->Cin; g.G = G;
        g.lda = d->Cin; g.ldb = d->Cin; g.ldc = d->Cout;
        g.mode = 0; g.stride = 1;
        return gemm_stream_launch(g, stream_variant(pl), pl.ring, s);
    }
    ConvArgs g = a;
    g.in = V; g.w = pl.split ? reinterpret_cast<const float*>(U_split) : U;
    g.a_presplit = 1; g.out = Mt; g.res = nullptr; g.partial = nullptr;
    g.B = 1; g.H = 1; g.W = (int)P; g.ldin = d->Cin; g.Ho = 1; g.Wo = (int)P; g.ldout = d->Cout; g.ldres = 0;
    g.KH = 1; g.KW = 1; g.stride = 1; g.pad = 0; g.K = d->Cin; g.M = (int)P; g.HoWo = (int)P;
    g.relu_in = 0; g.relu_out = 0; g.nk = pl.nk; g.splitk = 1; g.kt_per_split = pl.nk;
    g.tiles_m = cdiv(g.M, pl.bm); g.tiles_n = cdiv(g.Cout, pl.bn);
    g.raw = 1; g.in_gstride = (long)P * d->Cin; g.w_gstride = (long)d->Cout * d->Cin; g.out_gstride = (long)P * d->Cout;
    return launch_tile(pl, g, s, G);
}

// output transform + epilogue of `d` from its M
int wino_output(const xmem_conv_desc* d, int Ho, int Wo, int r, const float* Mt, size_t P, hipStream_t s) {
    const auto output_kernel = r == 4 ? wino4_output_kernel : wino_output_kernel;
    int blocks, threads;
    transform_grid(P * (d->Cout / 4), blocks, threads);
    hipLaunchKernelGGL(output_kernel, dim3(blocks), dim3(threads), 0, s, Mt, d->B, Ho, Wo, d->Cout,
                       cdiv(Ho, r), cdiv(Wo, r), d->scale, d->shift, d->res, d->ldres, d->res_broadcast ? 1 : 0, d->relu_out, d->out, d->ldout);
    return xmem_check_launch();
}

// Unfused Winograd F(r x r, 3x3), r = 2 or 4: input transform -> V, the (r+2)^2 position GEMMs (wino_position_gemm), output
// transform + epilogue.
int run_winograd(const Plan& pl, const xmem_conv_desc* d, const ConvArgs& a, int r, void* workspace, hipStream_t s) {
    const int th = cdiv(a.Ho, r), tw = cdiv(a.Wo, r), G = (r + 2) * (r + 2);
    const size_t P = wino_tiles(d, a.Ho, a.Wo, r);
    if (P > 0x7fffffff) return XMEM_ERR_UNSUPPORTED;
    float* V = reinterpret_cast<float*>(workspace);
    float* Mt = V + (size_t)G * P * d->Cin;
    int blocks, threads, rc;
    transform_grid(P * (d->Cin / 4), blocks, threads);
    if (r == 4) hipLaunchKernelGGL(wino4_input_kernel, dim3(blocks), dim3(threads), 0, s, d->in, d->ldin, d->B, d->H, d->W,
                                   d->Cin, th, tw, d->relu_in, V, pl.split ? 1 : 0, nullptr, 0);
    else hipLaunchKernelGGL(wino_input_kernel, dim3(blocks), dim3(threads), 0, s, d->in, d->ldin, d->B, d->H, d->W,
                            d->Cin, th, tw, d->relu_in, V, pl.split ? 1 : 0);
    if ((rc = wino_position_gemm(pl, d, a, r, V, Mt, P, s)) != XMEM_OK) return rc;
    return wino_output(d, a.Ho, a.Wo, r, Mt, P, s);
}

// ---- shared transforms (xmem_conv2d_shared_input, xmem_conv2d_nhwc_folded) ----
// An fp32 convolution whose plan is F(4x4) on unsplit operands: what the shared entry points run.  XMEM_OK and the plan, or why not.
int f4_plan_of(const xmem_conv_desc* d, Plan& pl) {
    const int rc = validate(d);
    if (rc != XMEM_OK) return rc;
    if (d->in_half || d->out_half) return XMEM_ERR_UNSUPPORTED;
    pl = make_plan(d, d->plan_tile);
    if (pl.form != F4 || pl.split) return XMEM_ERR_UNSUPPORTED;
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    if (wino_tiles(d, Ho, Wo, 4) > 0x7fffffff) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

inline size_t f4_m_bytes(const xmem_conv_desc* d) {
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    return (size_t)36 * wino_tiles(d, Ho, Wo, 4) * d->Cout * sizeof(float);
}

// The layout of xmem_conv2d_shared_input's workspace: V of the raw input (when a consumer reads it), V of relu(input) (likewise),
// then one M as wide as the widest consumer (the consumers run one after the other on the stream).
struct SharedLayout { size_t P, v_floats, m_floats; int n_raw, n_relu; };
int shared_layout(const xmem_conv_desc* const* ds, int n, Plan* pls, SharedLayout& L) {
    if (!ds || n < 2 || n > XMEM_CONV_SHARED_MAX) return XMEM_ERR_BAD_ARG;
    for (int i = 0; i < n; ++i) if (!ds[i]) return XMEM_ERR_BAD_ARG;
    L = {};
    int max_cout = 0;
    for (int i = 0; i < n; ++i) {
        const xmem_conv_desc* d = ds[i];
        const int rc = f4_plan_of(d, pls[i]);
        if (rc != XMEM_OK) return rc;
        if (d->in != ds[0]->in || d->ldin != ds[0]->ldin || d->B != ds[0]->B || d->H != ds[0]->H || d->W != ds[0]->W || d->Cin != ds[0]->Cin)
            return XMEM_ERR_UNSUPPORTED;
        if (d->relu_in) ++L.n_relu; else ++L.n_raw;
        if (d->Cout > max_cout) max_cout = d->Cout;
    }
    int Ho, Wo; out_dims(ds[0], 1, Ho, Wo);
    L.P = wino_tiles(ds[0], Ho, Wo, 4);
    L.v_floats = (size_t)36 * L.P * ds[0]->Cin;
    L.m_floats = (size_t)36 * L.P * max_cout;
    return XMEM_OK;
}
inline size_t shared_bytes(const SharedLayout& L) { return (((L.n_raw ? 1 : 0) + (L.n_relu ? 1 : 0)) * L.v_floats + L.m_floats) * sizeof(float); }

}  // namespace

extern "C" size_t xmem_conv2d_workspace_bytes(const xmem_conv_desc* d) {
    xmem_conv_desc hv; Plan pl;
    if (validate(d) != XMEM_OK || !plan_of(d, hv, pl)) return 0;
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    return workspace_need(pl, d, Ho, Wo);
}

extern "C" int xmem_conv2d_plan_info(const xmem_conv_desc* d, xmem_conv_plan_info* out) {
    if (!out) return XMEM_ERR_BAD_ARG;
    const int rc = validate(d);
    if (rc != XMEM_OK) return rc;
    xmem_conv_desc hv; Plan pl;
    if (!storage_types_ok(d) || !plan_of(d, hv, pl)) return XMEM_ERR_UNSUPPORTED;
    out->form = pl.form; out->bm = pl.bm; out->bn = pl.bn; out->bk = pl.bk; out->splitk = pl.splitk;
    out->stream = pl.ring ? 1 : 0; out->ring = pl.ring;
    return XMEM_OK;
}

extern "C" int xmem_conv2d_nhwc(const xmem_conv_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = validate(d);
    if (rc != XMEM_OK) return rc;
    xmem_conv_desc hv; Plan pl;
    if (!storage_types_ok(d) || !plan_of(d, hv, pl)) return XMEM_ERR_UNSUPPORTED;
    const int half = d->in_half ? (d->out_half ? 2 : 1) : 0;
    pl.half = half;
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    const size_t need = workspace_need(pl, d, Ho, Wo);
    if (need && (!workspace || workspace_bytes < need)) return XMEM_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    ConvArgs a = conv_args(d, pl, Ho, Wo, workspace);
    if (half) a.w = reinterpret_cast<const float*>(d->w_half);
    else if (pl.split) a.w = reinterpret_cast<const float*>(d->w_split);
    a.res_mod = d->res_broadcast ? Ho * Wo : 0;
#ifdef XMEM_TOOLS
    { static const int dbg = getenv("XMEM_CONV_DBG") ? atoi(getenv("XMEM_CONV_DBG")) : 0; a.dbg = dbg; }
#endif
    if (pl.form == F4) return run_winograd(pl, d, a, 4, workspace, s);
    if (pl.form == F2) return run_winograd(pl, d, a, 2, workspace, s);
    if (pl.form == F2_F16) {
        const int th = cdiv(Ho, 2), tw = cdiv(Wo, 2);
        const size_t P = wino_tiles(d, Ho, Wo, 2);
        if (P > 0x7fffffff) return XMEM_ERR_UNSUPPORTED;
        _Float16* V = reinterpret_cast<_Float16*>(workspace);
        float* Mt = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + wino_f16_v_bytes(P, d->Cin));
        size_t tot = P * (d->Cin / 4);
        int blocks = (int)((tot + 255) / 256); if (blocks > 16384) blocks = 16384;
        hipLaunchKernelGGL(wino_input_f16_kernel, dim3(blocks), dim3(256), 0, s, d->in, d->ldin, d->B, d->H, d->W, d->Cin, th, tw,
                           d->relu_in, V);
        WinoF16Args fa;
        fa.V = V; fa.U = reinterpret_cast<const _Float16*>(d->w_winograd_f16); fa.M = Mt;
        fa.P = (int)P; fa.Cin = d->Cin; fa.Cout = d->Cout;
        // 128x128 tiles once they fill the chip, 64x64 for the small (1/16-resolution, few-channel) layers
        const long big = (long)cdiv((int)P, 128) * cdiv(d->Cout, 128) * 16;
        if (big >= 512 && d->Cout >= 128) {
            fa.tiles_m = cdiv((int)P, 128); fa.tiles_n = cdiv(d->Cout, 128);
            hipLaunchKernelGGL((wino_gemm_f16_kernel<128, 128>), dim3(fa.tiles_m * fa.tiles_n, 16), dim3(256), (size_t)256 * 144, s, fa);
        } else {
            fa.tiles_m = cdiv((int)P, 64); fa.tiles_n = cdiv(d->Cout, 64);
            hipLaunchKernelGGL((wino_gemm_f16_kernel<64, 64>), dim3(fa.tiles_m * fa.tiles_n, 16), dim3(256), (size_t)128 * 144, s, fa);
        }
        if ((rc = xmem_check_launch()) != XMEM_OK) return rc;
        tot = P * (d->Cout / 4);
        blocks = (int)((tot + 255) / 256); if (blocks > 16384) blocks = 16384;
        hipLaunchKernelGGL(wino_output_kernel, dim3(blocks), dim3(256), 0, s, Mt, d->B, Ho, Wo, d->Cout, th, tw, d->scale, d->shift,
                           d->res, d->ldres, d->res_broadcast ? 1 : 0, d->relu_out, d->out, d->ldout);
        return xmem_check_launch();
    }
    if (pl.form == F2_FUSED) {
        const int th = cdiv(Ho, 2), tw = cdiv(Wo, 2);
        const size_t P = wino_tiles(d, Ho, Wo, 2);
        if (P > 0x7fffffff) return XMEM_ERR_UNSUPPORTED;
        float* V = reinterpret_cast<float*>(workspace);
        int blocks, threads;
        transform_grid(P * (d->Cin / 4), blocks, threads);
        hipLaunchKernelGGL(wino_input_kernel, dim3(blocks), dim3(threads), 0, s, d->in, d->ldin, d->B, d->H, d->W, d->Cin, th, tw,
                           d->relu_in, V, pl.split ? 1 : 0);
        WinoArgs wa;
        wa.V = V; wa.U = d->w_winograd; wa.scale = d->scale; wa.shift = d->shift; wa.res = d->res; wa.out = d->out;
        wa.P = (int)P; wa.Cin = d->Cin; wa.Cout = d->Cout; wa.B = d->B; wa.Ho = Ho; wa.Wo = Wo; wa.th = th; wa.tw = tw;
        wa.ldout = d->ldout; wa.ldres = d->ldres; wa.relu_out = d->relu_out; wa.nk = cdiv(d->Cin, 32);
        wa.res_bcast = d->res_broadcast ? 1 : 0;
        wa.tiles_m = cdiv(wa.P, pl.bm); wa.tiles_n = cdiv(wa.Cout, pl.bn);
        const size_t lds = 2 * (size_t)(pl.bm + pl.bn) * 36 * sizeof(float);
        dim3 grid(wa.tiles_m * wa.tiles_n);
        if (pl.bm == 128) hipLaunchKernelGGL((wino_fused_kernel<128, 64, 2, 1, 32>), grid, dim3(256), lds, s, wa);
        else if (pl.bn == 64) hipLaunchKernelGGL((wino_fused_kernel<64, 64, 1, 1, 32>), grid, dim3(256), lds, s, wa);
        else hipLaunchKernelGGL((wino_fused_kernel<64, 128, 1, 2, 32>), grid, dim3(256), lds, s, wa);
        return xmem_check_launch();
    }
    if (pl.ring) {                                 // pointwise convolution on the streaming kernel, fused epilogue
        GemmStreamArgs g = {};
        g.A = d->in; g.B = d->w; g.C = d->out; g.scale = d->scale; g.shift = d->shift; g.res = d->res;
        g.M = a.M; g.N = d->Cout; g.K = d->Cin; g.G = 1;
        g.lda = d->ldin; g.ldb = d->Cin; g.ldc = d->ldout; g.ldres = d->ldres;
        g.mode = 1; g.relu_in = d->relu_in; g.relu_out = d->relu_out; g.res_mod = a.res_mod;
        g.stride = d->stride; g.H = d->H; g.W = d->W; g.Wo = Wo; g.HoWo = Ho * Wo;
        return gemm_stream_launch(g, stream_variant(pl), pl.ring, s);
    }
    if (pl.form == GEMV) {
        // (round 4: a variant with EIGHT output pixels of a row per wave measured 28.0 us against 24.9 us for the one-pixel-per-wave form at
        // the 480p mask head - its taps were fetched one after the other behind their bounds branches.  Round 6, with every load of a wave
        // requested together: four pixels per wave 26.8 us against 31.2 (host-side events, same bits), +0.6 % on the B32 line; small maps
        // (2 x 37 x 51: 21 against 16 us) keep one pixel per wave - too few waves otherwise)
        if (half) hipLaunchKernelGGL(conv_cout1_kernel<true>, dim3(cdiv(a.M, 4)), dim3(256), 0, s, a);
        else if (a.M >= 8192 && a.KH == 3 && a.KW == 3 && a.stride == 1 && a.Cin <= 256 && a.Ho == a.H + 2 * a.pad - 2 && a.Wo == a.W + 2 * a.pad - 2)
            hipLaunchKernelGGL(conv_cout1_row4_kernel, dim3(cdiv(a.B * a.Ho * ((a.Wo + 3) / 4), 4)), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(conv_cout1_kernel<false>, dim3(cdiv(a.M, 4)), dim3(256), 0, s, a);
        return xmem_check_launch();
    }
    if ((rc = launch_tile(pl, a, s)) != XMEM_OK) return rc;
#ifdef XMEM_TOOLS
    if (a.dbg & 8) {
        static int printed = 0;
        (void)hipStreamSynchronize(s);
        const int n = a.tiles_m * a.tiles_n < CTRACE_MAX ? a.tiles_m * a.tiles_n : CTRACE_MAX;
        static unsigned long long h[CTRACE_MAX][6];
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_conv_trace), sizeof(unsigned long long) * 6 * n);
        if (printed++ % 16 == 4) {
            double d[6] = {0, 0, 0, 0, 0, 0}; unsigned long long tmin = ~0ull, tmax = 0;
            for (int i = 0; i < n; ++i) { for (int k = 1; k < 6; ++k) d[k] += (double)(h[i][k] - h[i][0]); if (h[i][0] < tmin) tmin = h[i][0]; if (h[i][5] > tmax) tmax = h[i][5]; }
            fprintf(stderr, "[conv trace] %d workgroups: entry -> first tiles requested %.0f, in LDS %.0f, k-loop done %.0f, stores issued %.0f, stores landed %.0f ticks (mean); "
                            "first entry -> last store landed %.0f ticks; ticks are s_memtime units (100 MHz = 10 ns on gfx950)\n", n, d[1] / n, d[2] / n, d[3] / n, d[4] / n, d[5] / n,
                    (double)(tmax - tmin));
        }
    }
#endif
    return pl.splitk > 1 ? launch_splitk_reduce(a, half == 2, s) : rc;
}

// A bottleneck's expand 1x1 (`e`: + residual, relu) and the next block's reduce 1x1 (`r`: relu, reading e's output) in one launch
// (csrc/pointwise_pair.hip).  Both plans are resolved exactly as xmem_conv2d_nhwc would resolve them: the pair kernel gives the bits of
// the classic direct tiles with split-K 1 and of nothing else, so any other plan is the caller's cue to run the two layers separately.
extern "C" int xmem_conv2d_pointwise_pair(const xmem_conv_desc* e, const xmem_conv_desc* r, void* stream) {
    int rc = validate(e);
    if (rc != XMEM_OK) return rc;
    if ((rc = validate(r)) != XMEM_OK) return rc;
    if (r->in != e->out || r->ldin != e->ldout || r->Cin != e->Cout || r->B != e->B || r->H != e->H || r->W != e->W) return XMEM_ERR_BAD_ARG;
    for (const xmem_conv_desc* d : {e, r}) {
        if (d->in_half || d->out_half || d->arith != 0) return XMEM_ERR_UNSUPPORTED;                 // fp32 only
        if (d->KH != 1 || d->KW != 1 || d->pad != 0 || d->stride != 1) return XMEM_ERR_UNSUPPORTED;
        if (d->relu_in || !d->relu_out || d->res_broadcast) return XMEM_ERR_UNSUPPORTED;
    }
    if (!e->res || r->res) return XMEM_ERR_UNSUPPORTED;
    if (!pointwise_pair_supported(e->Cin, e->Cout, r->Cout)) return XMEM_ERR_UNSUPPORTED;
    if ((((uintptr_t)e->in) & 15) != 0 || e->ldres >= (1 << 23) || (double)e->B * e->H * e->W >= 2.0e9) return XMEM_ERR_UNSUPPORTED;
    for (const xmem_conv_desc* d : {e, r}) {
        const Plan pl = make_plan(d, d->plan_tile);
        if (pl.form != DIRECT || pl.splitk != 1 || pl.ring || pl.generic || pl.split) return XMEM_ERR_UNSUPPORTED;
    }
    PairArgs a;
    a.A = e->in; a.W1 = e->w; a.scale1 = e->scale; a.shift1 = e->shift; a.res = e->res;
    a.W2 = r->w; a.scale2 = r->scale; a.shift2 = r->shift; a.y = e->out; a.z = r->out;
    a.M = e->B * e->H * e->W; a.K1 = e->Cin; a.N1 = e->Cout; a.N2 = r->Cout;
    a.lda = e->ldin; a.ldres = e->ldres; a.ldy = e->ldout; a.ldz = r->ldout;
    return pointwise_pair_launch(a, reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t xmem_conv2d_shared_input_workspace_bytes(const xmem_conv_desc* const* descs, int n) {
    Plan pls[XMEM_CONV_SHARED_MAX]; SharedLayout L;
    return shared_layout(descs, n, pls, L) == XMEM_OK ? shared_bytes(L) : 0;
}

extern "C" size_t xmem_conv2d_m_bytes(const xmem_conv_desc* d) {
    Plan pl;
    return f4_plan_of(d, pl) == XMEM_OK ? f4_m_bytes(d) : 0;
}

extern "C" int xmem_conv2d_shared_input(const xmem_conv_desc* const* descs, int n, void* const* defer_m, const size_t* defer_m_bytes,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    Plan pls[XMEM_CONV_SHARED_MAX]; SharedLayout L;
    int rc = shared_layout(descs, n, pls, L);
    if (rc != XMEM_OK) return rc;
    if (!workspace || workspace_bytes < shared_bytes(L)) return XMEM_ERR_WORKSPACE;
    for (int i = 0; i < n; ++i)
        if (defer_m && defer_m[i] && (!defer_m_bytes || defer_m_bytes[i] < f4_m_bytes(descs[i]) || (((uintptr_t)defer_m[i]) & 15) != 0))
            return XMEM_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const xmem_conv_desc* d0 = descs[0];
    int Ho, Wo; out_dims(d0, 1, Ho, Wo);
    const int th = cdiv(Ho, 4), tw = cdiv(Wo, 4);
    float* Vraw = reinterpret_cast<float*>(workspace);
    float* Vrelu = Vraw + (L.n_raw ? L.v_floats : 0);
    float* Mt = Vrelu + (L.n_relu ? L.v_floats : 0);
    int blocks, threads;
    const int variants = (L.n_raw ? 1 : 0) + (L.n_relu ? 1 : 0);       // one V per distinct relu_in; with both, raw first
    transform_grid(L.P * (d0->Cin / 4), blocks, threads);
    hipLaunchKernelGGL(wino4_input_kernel, dim3(blocks, variants), dim3(threads), 0, s, d0->in, d0->ldin, d0->B, d0->H, d0->W, d0->Cin,
                       th, tw, L.n_raw ? 0 : 1, Vraw, 0, Vrelu, 1);
    if ((rc = xmem_check_launch()) != XMEM_OK) return rc;
    for (int i = 0; i < n; ++i) {                  // each consumer under its own plan: position GEMMs, then its output transform
        const xmem_conv_desc* d = descs[i];
        const ConvArgs a = conv_args(d, pls[i], Ho, Wo, nullptr);
        float* m = defer_m && defer_m[i] ? reinterpret_cast<float*>(defer_m[i]) : Mt;
        if ((rc = wino_position_gemm(pls[i], d, a, 4, d->relu_in ? Vrelu : Vraw, m, L.P, s)) != XMEM_OK) return rc;
        if (m == Mt && (rc = wino_output(d, Ho, Wo, 4, Mt, L.P, s)) != XMEM_OK) return rc;
    }
    return XMEM_OK;
}

extern "C" int xmem_conv2d_output_from_m(const xmem_conv_desc* d, const void* m, size_t m_bytes, void* stream) {
    Plan pl;
    const int rc = f4_plan_of(d, pl);
    if (rc != XMEM_OK) return rc;
    if (!m || m_bytes < f4_m_bytes(d)) return XMEM_ERR_WORKSPACE;
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    return wino_output(d, Ho, Wo, 4, reinterpret_cast<const float*>(m), wino_tiles(d, Ho, Wo, 4), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int xmem_conv2d_nhwc_folded(const xmem_conv_desc* d, const xmem_conv_desc* branch, const void* branch_m, size_t branch_m_bytes,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    Plan pl, plb;
    int rc = f4_plan_of(d, pl);
    if (rc != XMEM_OK) return rc;
    if (!branch || (rc = f4_plan_of(branch, plb)) != XMEM_OK) return rc ? rc : XMEM_ERR_BAD_ARG;
    if (d->res) return XMEM_ERR_BAD_ARG;          // the branch is the residual
    int Ho, Wo, Hb, Wb; out_dims(d, 1, Ho, Wo); out_dims(branch, 1, Hb, Wb);
    if (branch->B != d->B || Hb != Ho || Wb != Wo || branch->Cout != d->Cout) return XMEM_ERR_UNSUPPORTED;
    if (!branch_m || branch_m_bytes < f4_m_bytes(branch) || (((uintptr_t)branch_m) & 15) != 0) return XMEM_ERR_WORKSPACE;
    if (branch->res && (branch->ldres % 4 != 0 || (((uintptr_t)branch->res) & 15) != 0)) return XMEM_ERR_UNSUPPORTED;
    const size_t need = workspace_need(pl, d, Ho, Wo);
    if (!workspace || workspace_bytes < need) return XMEM_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int th = cdiv(Ho, 4), tw = cdiv(Wo, 4);
    const size_t P = wino_tiles(d, Ho, Wo, 4);
    float* V = reinterpret_cast<float*>(workspace);
    float* Mt = V + (size_t)36 * P * d->Cin;
    int blocks, threads;
    transform_grid(P * (d->Cin / 4), blocks, threads);
    hipLaunchKernelGGL(wino4_input_kernel, dim3(blocks), dim3(threads), 0, s, d->in, d->ldin, d->B, d->H, d->W, d->Cin, th, tw,
                       d->relu_in, V, 0, nullptr, 0);
    const ConvArgs a = conv_args(d, pl, Ho, Wo, nullptr);
    if ((rc = wino_position_gemm(pl, d, a, 4, V, Mt, P, s)) != XMEM_OK) return rc;
    WinoFoldArgs f;
    f.Mt = Mt; f.Mb = reinterpret_cast<const float*>(branch_m);
    f.scale = d->scale; f.shift = d->shift; f.scale_b = branch->scale; f.shift_b = branch->shift; f.res_b = branch->res;
    f.out = d->out;
    f.B = d->B; f.Ho = Ho; f.Wo = Wo; f.Cout = d->Cout; f.th = th; f.tw = tw; f.ldout = d->ldout; f.relu_out = d->relu_out;
    f.ldres_b = branch->ldres; f.res_b_bcast = branch->res_broadcast ? 1 : 0; f.relu_b = branch->relu_out;
    transform_grid(P * (d->Cout / 2), blocks, threads);
    hipLaunchKernelGGL(wino4_output_fold_kernel, dim3(blocks), dim3(threads), 0, s, f);
    return xmem_check_launch();
}

extern "C" int xmem_mask_head_gather(const float* g16, int c16, const float* g8, int c8, const float* g4, int c4, const float* w,
                                     const float* scale, const float* shift, const float* hidden, int hd, float* logits, float* g4d,
                                     int ldg4d, float* cat, int ldcat, int K, int h, int wd, void* stream) {
    if (!g16 || !g8 || !g4 || !w || !scale || !shift || !hidden || !logits || !g4d || !cat) return XMEM_ERR_BAD_ARG;
    if (K <= 0 || h <= 0 || wd <= 0 || c16 <= 0 || c8 <= 0 || c4 <= 0 || hd <= 0) return XMEM_ERR_BAD_ARG;
    if (c16 % 4 || c8 % 4 || c4 % 4 || hd % 4 || ldg4d % 4 || ldcat % 4 || c4 > 256) return XMEM_ERR_UNSUPPORTED;    // one float4 of g4 per lane
    if (ldg4d < c16 + c8 + c4 + 1 || ldcat < hd) return XMEM_ERR_UNSUPPORTED;
    if (((uintptr_t)g16 | (uintptr_t)g8 | (uintptr_t)g4 | (uintptr_t)w | (uintptr_t)hidden | (uintptr_t)logits | (uintptr_t)g4d | (uintptr_t)cat) & 15)
        return XMEM_ERR_UNSUPPORTED;
    if ((double)K * h * wd >= 2.0e9 / 16) return XMEM_ERR_UNSUPPORTED;            // one workgroup per 1/16 pixel; 16 logits each
    MaskTailArgs a;
    a.g16 = g16; a.g8 = g8; a.g4 = g4; a.w = w; a.scale = scale; a.shift = shift; a.hidden = hidden;
    a.logits = logits; a.g4d = g4d; a.cat = cat;
    a.c16 = c16; a.c8 = c8; a.c4 = c4; a.hd = hd; a.ldg = ldg4d; a.ldcat = ldcat; a.K = K; a.h = h; a.wd = wd;
    hipLaunchKernelGGL(conv_cout1_tail_kernel, dim3(K * h * wd), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    return xmem_check_launch();
}

// ----------------------------------------------------------------------------------------------
// dilated convolution: the direct implicit GEMM with tap spacing `dilation` (DIL kernels above).  Plans are the direct tiles only
// (plan codes 0..6, split-K as in make_plan); no Winograd, no fp16 / split-operand modes, Cout >= 2.  With dilation 1 and the same
// plan the products and their order are those of xmem_conv2d_nhwc: the same bits.
// ----------------------------------------------------------------------------------------------
namespace {

int validate_dilated(const xmem_conv_desc* d, int dilation) {
    const int rc = validate(d, dilation, 6);
    if (rc != XMEM_OK) return rc;
    if (d->Cout == 1 || d->in_half || d->out_half || d->arith != 0 || d->res_broadcast) return XMEM_ERR_UNSUPPORTED;
    if ((long)dilation * (d->KH - 1) > (1 << 20) || (long)dilation * (d->KW - 1) > (1 << 20)) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

// the plan of the undilated descriptor with the same output size: H' = H - (dil - 1)(KH - 1) gives (H' + 2 pad - KH) / s + 1 =
// (H + 2 pad - dil (KH - 1) - 1) / s + 1 (make_plan only reads the output size, K, Cin and Cout of a direct plan)
Plan make_plan_dilated(const xmem_conv_desc* d, int dilation) {
    xmem_conv_desc v = *d;
    v.H = d->H - (dilation - 1) * (d->KH - 1);
    v.W = d->W - (dilation - 1) * (d->KW - 1);
    v.w_winograd = nullptr; v.w_winograd4 = nullptr; v.w_winograd_f16 = nullptr; v.w_split = nullptr; v.arith = 0;
    return make_plan(&v, v.plan_tile);
}

}  // namespace

extern "C" size_t xmem_conv2d_dilated_workspace_bytes(const xmem_conv_desc* d, int dilation) {
    if (validate_dilated(d, dilation) != XMEM_OK) return 0;
    int Ho, Wo; out_dims(d, dilation, Ho, Wo);
    return splitk_workspace(make_plan_dilated(d, dilation), d, Ho, Wo);
}

extern "C" int xmem_conv2d_nhwc_dilated(const xmem_conv_desc* d, int dilation, int flags, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    int rc = validate_dilated(d, dilation);
    if (rc != XMEM_OK) return rc;
    if (flags & ~XMEM_DILATED_NO_TAP_SKIP) return XMEM_ERR_BAD_ARG;
    const Plan pl = make_plan_dilated(d, dilation);
    int Ho, Wo; out_dims(d, dilation, Ho, Wo);
    if ((double)d->B * Ho * Wo >= 2.0e9 || (double)d->B * d->H * d->W * d->ldin >= 2.0e9) return XMEM_ERR_UNSUPPORTED;
    ConvArgs a = conv_args(d, pl, Ho, Wo, workspace);
    a.dil = dilation;
    a.skip_taps = (flags & XMEM_DILATED_NO_TAP_SKIP) || d->KH * d->KW > 64 || d->KH > 32 || d->KW > 32 ? 0 : 1;
    const size_t need = splitk_workspace(pl, d, Ho, Wo);
    if (need && (!workspace || workspace_bytes < need)) return XMEM_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = launch_tile(pl, a, s, 1, true);
    if (rc != XMEM_OK || pl.splitk == 1) return rc;
    return launch_splitk_reduce(a, false, s);
}
