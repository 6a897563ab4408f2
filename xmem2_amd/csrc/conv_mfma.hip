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
//
// This unit: the kernel family, the split-K reduce and their launchers (conv_mfma.hpp).  The planner is csrc/conv_plan.hpp, the
// Winograd forms are csrc/conv_winograd.hip, the entry points and the Cout = 1 kernels csrc/conv.hip.
#include "conv_mfma.hpp"
#include <stdio.h>
#include <stdlib.h>

using namespace conv_plan;

// BK (k-depth of a staged tile) is a template parameter: 32 or 64.  LDS rows are padded by 4 floats:
// stride 36 (=9x16 B) or 68 (=17x16 B) floats; both are odd multiples of 16 B, so the 16 lanes of a ds_read_b128
// lane-group (16 distinct rows) fall on 16 distinct 16-B slots of the 256-B bank row.

#ifdef XMEM_TOOLS
#define CDBG(bit) (p.dbg & (bit))
// XMEM_CONV_DBG & 8: phase timestamps of every workgroup of the pointwise kernel (s_memtime, 100 MHz-class constant clock):
// entry, first tiles requested, first tiles in LDS, k-loop done, stores issued; conv_trace_report (below) prints their averages.
#define CTRACE_MAX 16384
__device__ unsigned long long g_conv_trace[CTRACE_MAX][6];
#define CTRACE(slot) do { if (CDBG(8) && threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && blockIdx.x < CTRACE_MAX) \
    g_conv_trace[blockIdx.x][slot] = __builtin_readcyclecounter(); } while (0)
#else
#define CDBG(bit) 0
#define CTRACE(slot) do { } while (0)
#endif

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

// ----------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------
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

namespace {

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

}  // namespace

int launch_tile(const Plan& pl, const ConvArgs& a, hipStream_t s, int groups, bool dilated) {
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

#ifdef XMEM_TOOLS
int conv_dbg_from_env() {
    static const int dbg = getenv("XMEM_CONV_DBG") ? atoi(getenv("XMEM_CONV_DBG")) : 0;
    return dbg;
}

// XMEM_CONV_DBG & 8, after a launch_tile: the averages of the phase timestamps its workgroups left in g_conv_trace
void conv_trace_report(const ConvArgs& a, hipStream_t s) {
    if (!(a.dbg & 8)) return;
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
