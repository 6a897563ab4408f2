// The Winograd forms of the 3x3 / stride 1 / pad 1 convolutions: the F(2x2), F(4x4) and fp16 transform kernels, the fused F(2x2)
// kernel, the fp16 position GEMM, and the driver that puts a convolution together from them (conv_winograd.hpp).  The fp32
// position GEMMs run on the implicit-GEMM kernel (csrc/conv_mfma.hip) or the streaming kernel (csrc/gemm_stream.hip).
#include "conv_winograd.hpp"
#include "gemm_stream.hpp"

using namespace conv_plan;

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

// Transform kernels are grid-stride over (tile, channel quad) items, one item per thread.  A 1/16-resolution layer has ~15 000 items:
// as 256-thread workgroups that is ~60 workgroups on 60 of the 256 CUs, each bound by its own CU's load / store path (measured
// 10-17 us for 12 MB).  Below 512 workgroups of 256 the items are dealt as 64-thread workgroups instead: four times the CUs.
inline void transform_grid(size_t items, int& blocks, int& threads) {
    threads = items < (size_t)512 * 256 ? 64 : 256;
    size_t b = (items + threads - 1) / threads;
    blocks = (int)(b > 16384 ? 16384 : b);
}

// the grid of a transform of `form`: the fp16 form keeps 256-thread workgroups at every size
inline void form_grid(int form, size_t items, int& blocks, int& threads) {
    if (form != F2_F16) return transform_grid(items, blocks, threads);
    threads = 256;
    const size_t b = (items + 255) / 256;
    blocks = (int)(b > 16384 ? 16384 : b);
}

inline int form_r(int form) { return form == F4 ? 4 : 2; }

// F2_F16: the 16 position GEMMs on halfs
int wino_gemm_f16(const xmem_conv_desc* d, const _Float16* V, float* Mt, size_t P, hipStream_t s) {
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
    return xmem_check_launch();
}

// F2_FUSED: position GEMMs, output transform and epilogue in one kernel
int wino_fused(const Plan& pl, const xmem_conv_desc* d, int Ho, int Wo, const float* V, size_t P, hipStream_t s) {
    WinoArgs wa;
    wa.V = V; wa.U = d->w_winograd; wa.scale = d->scale; wa.shift = d->shift; wa.res = d->res; wa.out = d->out;
    wa.P = (int)P; wa.Cin = d->Cin; wa.Cout = d->Cout; wa.B = d->B; wa.Ho = Ho; wa.Wo = Wo; wa.th = cdiv(Ho, 2); wa.tw = cdiv(Wo, 2);
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

}  // namespace

void wino_input(int form, const xmem_conv_desc* d, size_t P, int relu_in, void* V, bool split, hipStream_t s, float* V2, int relu_in2) {
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    const int r = form_r(form), th = cdiv(Ho, r), tw = cdiv(Wo, r);
    int blocks, threads;
    form_grid(form, P * (d->Cin / 4), blocks, threads);
    if (form == F4)
        hipLaunchKernelGGL(wino4_input_kernel, dim3(blocks, V2 ? 2 : 1), dim3(threads), 0, s, d->in, d->ldin, d->B, d->H, d->W, d->Cin, th, tw,
                           relu_in, reinterpret_cast<float*>(V), split ? 1 : 0, V2, relu_in2);
    else if (form == F2_F16)
        hipLaunchKernelGGL(wino_input_f16_kernel, dim3(blocks), dim3(threads), 0, s, d->in, d->ldin, d->B, d->H, d->W, d->Cin, th, tw,
                           relu_in, reinterpret_cast<_Float16*>(V));
    else
        hipLaunchKernelGGL(wino_input_kernel, dim3(blocks), dim3(threads), 0, s, d->in, d->ldin, d->B, d->H, d->W, d->Cin, th, tw,
                           relu_in, reinterpret_cast<float*>(V), split ? 1 : 0);
}

// on the plan's tile of the implicit-GEMM kernel, or on the streaming kernel
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

int wino_output(int form, const xmem_conv_desc* d, int Ho, int Wo, const float* Mt, size_t P, hipStream_t s) {
    const int r = form_r(form);
    const auto output_kernel = r == 4 ? wino4_output_kernel : wino_output_kernel;
    int blocks, threads;
    form_grid(form, P * (d->Cout / 4), blocks, threads);
    hipLaunchKernelGGL(output_kernel, dim3(blocks), dim3(threads), 0, s, Mt, d->B, Ho, Wo, d->Cout,
                       cdiv(Ho, r), cdiv(Wo, r), d->scale, d->shift, d->res, d->ldres, d->res_broadcast ? 1 : 0, d->relu_out, d->out, d->ldout);
    return xmem_check_launch();
}

int wino_output_fold(const xmem_conv_desc* d, const xmem_conv_desc* branch, int Ho, int Wo, const float* Mt, const float* Mb, size_t P,
                     hipStream_t s) {
    WinoFoldArgs f;
    f.Mt = Mt; f.Mb = Mb;
    f.scale = d->scale; f.shift = d->shift; f.scale_b = branch->scale; f.shift_b = branch->shift; f.res_b = branch->res;
    f.out = d->out;
    f.B = d->B; f.Ho = Ho; f.Wo = Wo; f.Cout = d->Cout; f.th = cdiv(Ho, 4); f.tw = cdiv(Wo, 4); f.ldout = d->ldout; f.relu_out = d->relu_out;
    f.ldres_b = branch->ldres; f.res_b_bcast = branch->res_broadcast ? 1 : 0; f.relu_b = branch->relu_out;
    int blocks, threads;
    transform_grid(P * (d->Cout / 2), blocks, threads);
    hipLaunchKernelGGL(wino4_output_fold_kernel, dim3(blocks), dim3(threads), 0, s, f);
    return xmem_check_launch();
}

// The workspace holds V [(r+2)^2][P][Cin] (F2_F16: halfs, padded to wino_f16_v_bytes) and behind it, for the unfused forms, M.
int run_winograd(const Plan& pl, const xmem_conv_desc* d, const ConvArgs& a, void* workspace, hipStream_t s) {
    const int r = form_r(pl.form), G = (r + 2) * (r + 2);
    const size_t P = wino_tiles(d, a.Ho, a.Wo, r);
    if (!wino_tiles_fit(P)) return XMEM_ERR_UNSUPPORTED;
    const size_t v_bytes = pl.form == F2_F16 ? wino_f16_v_bytes(P, d->Cin) : (size_t)G * P * d->Cin * sizeof(float);
    const float* V = reinterpret_cast<const float*>(workspace);
    float* Mt = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + v_bytes);
    wino_input(pl.form, d, P, d->relu_in, workspace, pl.split, s);
    if (pl.form == F2_FUSED) return wino_fused(pl, d, a.Ho, a.Wo, V, P, s);
    const int rc = pl.form == F2_F16 ? wino_gemm_f16(d, reinterpret_cast<const _Float16*>(workspace), Mt, P, s)
                                     : wino_position_gemm(pl, d, a, r, V, Mt, P, s);
    if (rc != XMEM_OK) return rc;
    return wino_output(pl.form, d, a.Ho, a.Wo, Mt, P, s);
}
