// ResNet-50 bottleneck pair: block b's expand 1x1 (conv3: K1 -> N1 = 4 K1, + residual, relu) and block b+1's reduce 1x1 (conv1:
// N1 -> N2, relu) in ONE launch.  A 256-thread workgroup owns 64 consecutive pixels and walks N1 in chunks of 64 channels:
//   expand GEMM of the chunk (64 x 64 x K1, k-tiles of 32 through double-buffered LDS, the classic 64x64 tile of conv_mfma.hip)
//   -> epilogue -> the chunk of y goes to global memory (the next block's residual) AND into an LDS tile
//   -> reduce GEMM: the chunk is the next K-slab (64 wide) of acc2 [64 x N2], which stays in registers over all chunks.
// y is never read back from memory, the A tile's re-reads stay in this CU's cache, and a workgroup does N1 / 64 x (1 + N2 / K1) times
// the MFMA work of a K1-deep classic workgroup behind one prologue.
//
// SAME BITS as the two separate launches: both GEMMs keep the lane map of conv_mfma.hip (8-groups of k ascending, a lane holding 4
// consecutive k at offset 4 * (lane >> 5), MFMA step j contracting k = {j, 4 + j}), the reduce slabs arrive in ascending channel
// order, one accumulator chain per output element, and the epilogues are the classic tile's expressions.
//
// Every step is straight-line code (the k-tile and slab loops are unrolled; the only loop is over chunks): the operand loads of step
// s + 1 are requested before the MFMAs of step s, the residual / scale / shift of a chunk under its first k-tile, and no load sits
// behind a branch, so the compiler's vmcnt waits are exact.
#include "pointwise_pair.hpp"

namespace {

constexpr int LDK = 36;            // expand k-tile rows: 32 floats + 4 (odd multiple of 16 B: conflict-free ds_read_b128)
constexpr int LDY = 68;            // y chunk rows: 64 floats + 4

template <int N2> struct PairShape {
    static constexpr int RK = N2 == 256 ? 16 : 32;         // k-depth of a staged W2 tile (N2 = 256: 16, so that two stages stay within 40 KB)
    static constexpr int LDR = RK + 4;                     // 36 or 20 floats: both odd multiples of 16 B
    static constexpr int NR = 64 / RK;                     // reduce steps per chunk
    static constexpr int STAGE = (128 * LDK > N2 * LDR) ? 128 * LDK : N2 * LDR;      // floats per LDS stage
    static constexpr size_t LDS = (size_t)(2 * STAGE + 64 * LDY) * sizeof(float);
};

template <int K1, int N2>
__global__ __launch_bounds__(256, 2) void conv_pointwise_pair_kernel(PairArgs p) {
    using S = PairShape<N2>;
    constexpr int NK1 = K1 / 32;               // expand k-tiles
    constexpr int RK = S::RK, LDR = S::LDR, NR = S::NR, STAGE = S::STAGE;
    constexpr int C4R = RK / 4;                // float4 columns of a W2 tile row
    constexpr int RPPR = 256 / C4R;            // W2 rows staged per pass
    constexpr int RW = N2 / RPPR;              // passes (2 or 4)
    constexpr int TN2 = N2 / 64;               // 32x32 accumulators of the reduce GEMM per wave (2 x 2 waves over 64 x N2)
    static_assert((NK1 + NR) % 2 == 0, "a chunk is an even number of steps: the LDS stage parity is static");
    static_assert(RW <= 4, "four staging registers per thread");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const Ys = smem + 2 * STAGE;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int lrow = tid >> 3, c4 = tid & 7;
    const int lrowr = tid / C4R, c4r = tid % C4R;          // (powers of two: shifts)
    const int m0 = blockIdx.x * 64;
    const int N1 = 4 * K1;
    const int NC = N1 / 64;

    // operand rows of this thread (rows past M are clamped: their products are never stored)
    const float* a_ptr[2];
    const float* w1_ptr[2];
    const float* w2_ptr[RW];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        a_ptr[i] = p.A + (size_t)min(m0 + lrow + 32 * i, p.M - 1) * p.lda + c4 * 4;
        w1_ptr[i] = p.W1 + (size_t)(lrow + 32 * i) * K1 + c4 * 4;
    }
    f32x4 st[4];
    auto load_expand = [&](int c, int kt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) st[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + kt * 32);
#pragma unroll
        for (int i = 0; i < 2; ++i) st[2 + i] = *reinterpret_cast<const f32x4*>(w1_ptr[i] + (size_t)c * 64 * K1 + kt * 32);
    };
    load_expand(0, 0);
#pragma unroll
    for (int i = 0; i < RW; ++i) w2_ptr[i] = p.W2 + (size_t)(lrowr + RPPR * i) * N1 + c4r * 4;
    auto load_reduce = [&](int c, int rt) {
#pragma unroll
        for (int i = 0; i < RW; ++i) st[i] = *reinterpret_cast<const f32x4*>(w2_ptr[i] + c * 64 + rt * RK);
    };
    auto store_expand = [&](int buf) {
        float* As = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(&As[(lrow + 32 * i) * LDK + c4 * 4]) = st[i];     // rows 0..63 A, 64..127 W1
    };
    auto store_reduce = [&](int buf) {
        float* Ws = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < RW; ++i) *reinterpret_cast<f32x4*>(&Ws[(lrowr + RPPR * i) * LDR + c4r * 4]) = st[i];
    };

    f32x16 acc1, acc2[TN2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[r] = 0.f;
#pragma unroll
    for (int j = 0; j < TN2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[j][r] = 0.f;

    // this lane's rows of a 32x32 block: mb + (r & 3) + 8 * (r >> 2); its column: l31
    const int mb = m0 + wm * 32 + 4 * lh;
    const int left = p.M - 1 - mb;             // rows below this lane's first one (negative past the end)
    const float* const res_lane = p.res + (size_t)mb * p.ldres + wn * 32 + l31;
    float* const y_lane = p.y + (size_t)mb * p.ldy + wn * 32 + l31;
    float* const ys_lane = Ys + (wm * 32 + 4 * lh) * LDY + wn * 32 + l31;

    store_expand(0);
    __syncthreads();

    float rv[16], sc1 = 0.f, sh1 = 0.f;
    for (int c = 0; c < NC; ++c) {
        // ---- expand GEMM of chunk c: acc1 [64 x 64] over K1 ----
#pragma unroll
        for (int kt = 0; kt < NK1; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < NK1) load_expand(c, kt + 1);
            else load_reduce(c, 0);
            if (kt == 0) {
                // residual rows, scale and shift of the chunk: in flight under its MFMAs (16 unconditional loads from clamped rows)
                const int n = c * 64 + wn * 32 + l31;
                sc1 = p.scale1[n]; sh1 = p.shift1[n];
#pragma unroll
                for (int r = 0; r < 16; ++r) rv[r] = res_lane[(long)__mul24(min((r & 3) + 8 * (r >> 2), left), p.ldres) + c * 64];
            }
            const float* As = smem + buf * STAGE + (wm * 32 + l31) * LDK + lh * 4;
            const float* Bs = smem + buf * STAGE + 64 * LDK + (wn * 32 + l31) * LDK + lh * 4;
            f32x4 af[2], bf[2];
            af[0] = *reinterpret_cast<const f32x4*>(As);
            bf[0] = *reinterpret_cast<const f32x4*>(Bs);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int cur = kk & 1, nxt = cur ^ 1;
                if (kk + 1 < 4) {
                    af[nxt] = *reinterpret_cast<const f32x4*>(As + (kk + 1) * 8);
                    bf[nxt] = *reinterpret_cast<const f32x4*>(Bs + (kk + 1) * 8);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][s], bf[cur][s], acc1, 0, 0, 0);
            }
            if (kt == NK1 - 1) {
                // expand epilogue, two phases: every loaded operand is consumed first, then the stores (registers only)
                float vout[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc1[r] * sc1 + sh1;
                    v += rv[r];
                    vout[r] = fmaxf(v, 0.f);
                    acc1[r] = 0.f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) ys_lane[((r & 3) + 8 * (r >> 2)) * LDY] = vout[r];
                float* const yc = y_lane + c * 64;
                if (m0 + wm * 32 + 32 <= p.M) {            // (wave-uniform) every row of the block exists
#pragma unroll
                    for (int r = 0; r < 16; ++r) yc[(long)((r & 3) + 8 * (r >> 2)) * p.ldy] = vout[r];
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int o = (r & 3) + 8 * (r >> 2);
                        if (o <= left) yc[(long)o * p.ldy] = vout[r];
                    }
                }
            }
            if (kt + 1 < NK1) store_expand(buf ^ 1);
            else store_reduce(buf ^ 1);
            __syncthreads();
        }
        // ---- reduce GEMM: chunk c of y (LDS) is K-slab c of acc2 [64 x N2] ----
        const int cn = min(c + 1, NC - 1);     // (the last chunk requests its own first tile again: no branch around the loads)
#pragma unroll
        for (int rt = 0; rt < NR; ++rt) {
            const int buf = (NK1 + rt) & 1;
            if (rt + 1 < NR) load_reduce(c, rt + 1);
            else load_expand(cn, 0);
            const float* Ya = Ys + (wm * 32 + l31) * LDY + rt * RK + lh * 4;
            const float* Wb = smem + buf * STAGE + (wn * (N2 / 2) + l31) * LDR + lh * 4;
            f32x4 af[2], bf[2][TN2];
            af[0] = *reinterpret_cast<const f32x4*>(Ya);
#pragma unroll
            for (int j = 0; j < TN2; ++j) bf[0][j] = *reinterpret_cast<const f32x4*>(Wb + j * 32 * LDR);
#pragma unroll
            for (int kk = 0; kk < RK / 8; ++kk) {
                const int cur = kk & 1, nxt = cur ^ 1;
                if (kk + 1 < RK / 8) {
                    af[nxt] = *reinterpret_cast<const f32x4*>(Ya + (kk + 1) * 8);
#pragma unroll
                    for (int j = 0; j < TN2; ++j) bf[nxt][j] = *reinterpret_cast<const f32x4*>(Wb + j * 32 * LDR + (kk + 1) * 8);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int j = 0; j < TN2; ++j)
                        acc2[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[cur][s], bf[cur][j][s], acc2[j], 0, 0, 0);
            }
            if (rt + 1 < NR) store_reduce(buf ^ 1);
            else store_expand(buf ^ 1);
            __syncthreads();
        }
    }

    // ---- reduce epilogue ----
#pragma unroll
    for (int j = 0; j < TN2; ++j) {
        const int n = wn * (N2 / 2) + j * 32 + l31;
        const float sc = p.scale2[n], sh = p.shift2[n];
        float* const zrow = p.z + (size_t)mb * p.ldz + n;
        float vout[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = acc2[j][r] * sc + sh;
            vout[r] = fmaxf(v, 0.f);
        }
        if (m0 + wm * 32 + 32 <= p.M) {
#pragma unroll
            for (int r = 0; r < 16; ++r) zrow[(long)((r & 3) + 8 * (r >> 2)) * p.ldz] = vout[r];
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = (r & 3) + 8 * (r >> 2);
                if (o <= left) zrow[(long)o * p.ldz] = vout[r];
            }
        }
    }
}

template <int K1, int N2>
int launch(const PairArgs& a, hipStream_t s) {
    auto kern = conv_pointwise_pair_kernel<K1, N2>;
    const size_t lds = PairShape<N2>::LDS;
    if (xmem_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds) != XMEM_OK) return XMEM_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(cdiv(a.M, 64)), dim3(256), lds, s, a);
    return xmem_check_launch();
}

}  // namespace

bool pointwise_pair_supported(int K1, int N1, int N2) {
    return (K1 == 64 || K1 == 128 || K1 == 256) && N1 == 4 * K1 && (N2 == K1 || N2 == 2 * K1) && N2 <= 256;
}

size_t pointwise_pair_lds_bytes(int N2) {
    return N2 == 256 ? PairShape<256>::LDS : N2 == 128 ? PairShape<128>::LDS : PairShape<64>::LDS;
}

int pointwise_pair_launch(const PairArgs& a, hipStream_t s) {
    if (!pointwise_pair_supported(a.K1, a.N1, a.N2) || a.M <= 0) return XMEM_ERR_UNSUPPORTED;
    if (a.K1 == 64) return a.N2 == 64 ? launch<64, 64>(a, s) : launch<64, 128>(a, s);
    if (a.K1 == 128) return a.N2 == 128 ? launch<128, 128>(a, s) : launch<128, 256>(a, s);
    return launch<256, 256>(a, s);
}
