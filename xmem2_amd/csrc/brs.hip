// f-BRS click refinement (inference/interact/fbrs/inference/predictors/brs.py, brs_functors.py, brs_losses.py): the pieces of the
// objective and of its data gradient that are not convolutions.  The per-channel scale and bias on the optimised feature map, the
// BRSMaskLoss over the click squares with its gradient on the low-resolution logits (the adjoint of the align_corners upsample),
// the ReLU gates of the backward pass and the reduction of the feature gradient to the 2C parameters.  fp32, gfx950.
//
// DETERMINISM: L-BFGS and the strict `<` that keeps the best prediction need the same x to give the same bits.  No kernel here adds
// floats with atomics: the loss is summed by one workgroup in a fixed order, the logit gradient is gathered (every low-resolution
// pixel walks the click terms in list order), the channel sums run in two fixed-order stages.  Only integer counts use atomics.
#include "common.hpp"
#include <limits.h>
#include <math.h>

namespace {

inline int grid_for(size_t n, int block = 256, int cap = 8192) {
    size_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

bool misaligned(const void* p) { return (((uintptr_t)p) & 15) != 0; }

// as csrc/click.hip: the same source cell and weight as the output kernel of the click network, so that the mask of an evaluation is
// the mask xmem_click_prob would give for the same logits
__device__ __forceinline__ void ac_src(int o, int n_in, int n_out, int& i0, int& i1, float& l) {
    if (n_out <= 1 || n_in <= 1) { i0 = i1 = 0; l = 0.f; return; }
    const int den = n_out - 1, num = o * (n_in - 1);
    i0 = num / den;
    const int rem = num - i0 * den;
    i1 = min(i0 + 1, n_in - 1);
    l = (float)rem / (float)den;
}

__device__ __forceinline__ float lerp4(float p00, float p01, float p10, float p11, float ly, float lx) {
    if (ly == 0.f && lx == 0.f) return p00;
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11);
}

// ---- y = x (1 + s[c]) + b[c] ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void brs_affine_kernel(const float* __restrict__ x, const float* __restrict__ sb, float* __restrict__ y,
                                                         size_t n4, int C4) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(e % C4);
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + e * 4);
        const f32x4 s = *reinterpret_cast<const f32x4*>(sb + q * 4);
        const f32x4 b = *reinterpret_cast<const f32x4*>(sb + (size_t)(C4 + q) * 4);
        *reinterpret_cast<f32x4*>(y + e * 4) = v * (1.f + s) + b;
    }
}

// ---- ReLU gates ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relu_gate_kernel(const float* __restrict__ y, const float* __restrict__ g, float* __restrict__ out,
                                                        size_t n4) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (size_t)gridDim.x * blockDim.x) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(y + e * 4);
        f32x4 v = *reinterpret_cast<const f32x4*>(g + e * 4);
        v.x = a.x > 0.f ? v.x : 0.f; v.y = a.y > 0.f ? v.y : 0.f; v.z = a.z > 0.f ? v.z : 0.f; v.w = a.w > 0.f ? v.w : 0.f;
        *reinterpret_cast<f32x4*>(out + e * 4) = v;
    }
}

// the adjoint of a Cout = 1 pointwise layer is an outer product: out[p][c] = y[p][c] > 0 ? g1[p] w[c] : 0
__global__ __launch_bounds__(256) void relu_gate_outer_kernel(const float* __restrict__ y, const float* __restrict__ g1,
                                                              const float* __restrict__ w, float* __restrict__ out, size_t n4, int C4) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(e % C4);
        const float gp = g1[e / C4];
        const f32x4 a = *reinterpret_cast<const f32x4*>(y + e * 4);
        const f32x4 k = *reinterpret_cast<const f32x4*>(w + q * 4);
        f32x4 v;
        v.x = a.x > 0.f ? gp * k.x : 0.f; v.y = a.y > 0.f ? gp * k.y : 0.f; v.z = a.z > 0.f ? gp * k.z : 0.f; v.w = a.w > 0.f ? gp * k.w : 0.f;
        *reinterpret_cast<f32x4*>(out + e * 4) = v;
    }
}

// ---- the loss ----------------------------------------------------------------------------------------------------------------------
// record layout (floats; 4..7 hold int32 bits): 0 data loss, 1 f_max_pos, 2 f_max_neg, 3 final f (xmem_brs_param_grad), 4 + 2 b
// intersection and 5 + 2 b union of sample b's mask with the last mask
constexpr int REC_LOSS = 0, REC_MAXPOS = 1, REC_MAXNEG = 2, REC_F = 3, REC_COUNTS = 4;
constexpr int TERM_WORDS = 8;        // y0, y1, x0, x1 (int bits), ly, lx, coefficient, 0

__global__ void brs_record_init_kernel(float* __restrict__ rec) {
    if (threadIdx.x < 8) rec[threadIdx.x] = 0.f;          // int 0 has the bits of 0.f
}

// one pass over the B H W pixels: the mask bit of the upsampled logit, its store, and the integer counts against the last mask
__global__ __launch_bounds__(256) void brs_mask_kernel(const float* __restrict__ logits, int B, int h4, int w4, int H, int W,
                                                       const uint8_t* __restrict__ last, uint8_t* __restrict__ mask, int* __restrict__ counts) {
    const size_t P = (size_t)H * W;
    for (int b = 0; b < B; ++b) {
        int inter = 0, uni = 0;
        const float* l = logits + (size_t)b * h4 * w4;
        for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < P; e += (size_t)gridDim.x * blockDim.x) {
            const int x = (int)(e % W), y = (int)(e / W);
            int y0, y1, x0, x1; float ly, lx;
            ac_src(y, h4, H, y0, y1, ly);
            ac_src(x, w4, W, x0, x1, lx);
            const float v = lerp4(l[(size_t)y0 * w4 + x0], l[(size_t)y0 * w4 + x1], l[(size_t)y1 * w4 + x0], l[(size_t)y1 * w4 + x1], ly, lx);
            const int m = v > 0.f ? 1 : 0, o = last[b * P + e] ? 1 : 0;
            mask[b * P + e] = (uint8_t)m;
            inter += m & o; uni += m | o;
        }
        inter = wave_sum_i(inter); uni = wave_sum_i(uni);
        if ((threadIdx.x & 63) == 0) {
            if (inter) atomicAdd(counts + 2 * b, inter);
            if (uni) atomicAdd(counts + 2 * b + 1, uni);
        }
    }
}

// rects [B][cap][5] int32: rows [r0, r1) x columns [c0, c1) (at most 3 x 3, already clipped to the map, possibly empty) and the polarity
// (1 positive, 0 negative).  The click maps of the reference are SETS of pixels: a pixel inside several squares of one polarity
// counts once - it belongs to the first such square of its sample's list.
__device__ __forceinline__ bool brs_owned(const int* __restrict__ rects, int k, int y, int x, int pol) {
    for (int j = 0; j < k; ++j) {
        const int* r = rects + j * 5;
        if (r[4] == pol && y >= r[0] && y < r[1] && x >= r[2] && x < r[3]) return false;
    }
    return true;
}

__device__ __forceinline__ float block_sum_256(float v, float* sh) {       // fixed order: the same inputs give the same bits
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_max_256(float v, float* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fmaxf(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// ONE workgroup: the loss sums and maxima over the click-square pixels of both samples, and one term per (sample, square, pixel of
// the 3 x 3) with the interpolation cell of its pixel and dL/d(upsampled logit) - zero for a pixel outside the clipped square or owned
// by an earlier square.
__global__ __launch_bounds__(256) void brs_terms_kernel(const float* __restrict__ logits, int B, int h4, int w4, int H, int W,
                                                        const int* __restrict__ rects, const int* __restrict__ count, int cap,
                                                        float eps, float* __restrict__ terms, float* __restrict__ rec) {
    __shared__ float sh[256];
    const int n = min(max(count[0], 0), cap);
    const int total = B * n * 9;
    // pass 1: the number of positive / negative pixels (exact in floats: at most B cap 9)
    float npos = 0.f, nneg = 0.f;
    for (int t = threadIdx.x; t < total; t += 256) {
        const int b = t / (n * 9), k = (t / 9) % n, d = t % 9;
        const int* rb = rects + (size_t)b * cap * 5;
        const int* r = rb + k * 5;
        const int y = r[0] + d / 3, x = r[2] + d % 3;
        if (y < r[1] && x < r[3] && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && brs_owned(rb, k, y, x, r[4])) { if (r[4]) npos += 1.f; else nneg += 1.f; }
    }
    npos = block_sum_256(npos, sh);
    nneg = block_sum_256(nneg, sh);
    const float dpos = npos + eps, dneg = nneg + eps;
    float spos = 0.f, sneg = 0.f, mpos = 0.f, mneg = 0.f;
    for (int t = threadIdx.x; t < total; t += 256) {
        const int b = t / (n * 9), k = (t / 9) % n, d = t % 9;
        const int* rb = rects + (size_t)b * cap * 5;
        const int* r = rb + k * 5;
        const int y = r[0] + d / 3, x = r[2] + d % 3;
        float* o = terms + ((size_t)b * cap * 9 + (size_t)k * 9 + d) * TERM_WORDS;
        int y0 = 0, y1 = 0, x0 = 0, x1 = 0; float ly = 0.f, lx = 0.f, coef = 0.f;
        if (y < r[1] && x < r[3] && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && brs_owned(rb, k, y, x, r[4])) {
            ac_src(y, h4, H, y0, y1, ly);
            ac_src(x, w4, W, x0, x1, lx);
            const float* l = logits + (size_t)b * h4 * w4;
            const float v = lerp4(l[(size_t)y0 * w4 + x0], l[(size_t)y0 * w4 + x1], l[(size_t)y1 * w4 + x0], l[(size_t)y1 * w4 + x1], ly, lx);
            const float p = sigmoidf_(v), q = 1.f - p;
            if (r[4]) { spos += q * q; mpos = fmaxf(mpos, fabsf(q)); coef = -2.f * q / dpos * (p * q); }
            else      { sneg += p * p; mneg = fmaxf(mneg, fabsf(p)); coef = 2.f * p / dneg * (p * q); }
        }
        reinterpret_cast<int*>(o)[0] = y0; reinterpret_cast<int*>(o)[1] = y1; reinterpret_cast<int*>(o)[2] = x0; reinterpret_cast<int*>(o)[3] = x1;
        o[4] = ly; o[5] = lx; o[6] = coef; o[7] = 0.f;
    }
    spos = block_sum_256(spos, sh); sneg = block_sum_256(sneg, sh);
    mpos = block_max_256(mpos, sh); mneg = block_max_256(mneg, sh);
    if (threadIdx.x == 0) { rec[REC_LOSS] = spos / dpos + sneg / dneg; rec[REC_MAXPOS] = mpos; rec[REC_MAXNEG] = mneg; }
}

// the adjoint of the upsample in gather form: low-resolution pixel (b, i, j) walks its sample's terms in list order
__global__ __launch_bounds__(256) void brs_dlogit_kernel(const float* __restrict__ terms, const int* __restrict__ count, int cap, int B,
                                                         int h4, int w4, float* __restrict__ dlogit) {
    const int n = min(max(count[0], 0), cap);
    const size_t total = (size_t)B * h4 * w4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % w4), i = (int)((e / w4) % h4), b = (int)(e / ((size_t)w4 * h4));
        const float* tb = terms + (size_t)b * cap * 9 * TERM_WORDS;
        float acc = 0.f;
        for (int t = 0; t < n * 9; ++t) {
            const float* o = tb + (size_t)t * TERM_WORDS;
            const float coef = o[6];
            if (coef == 0.f) continue;
            const int y0 = reinterpret_cast<const int*>(o)[0], y1 = reinterpret_cast<const int*>(o)[1];
            const int x0 = reinterpret_cast<const int*>(o)[2], x1 = reinterpret_cast<const int*>(o)[3];
            if ((i != y0 && i != y1) || (j != x0 && j != x1)) continue;
            const float ly = o[4], lx = o[5], hy = 1.f - ly, hx = 1.f - lx;
            float wgt = 0.f;
            if (ly == 0.f && lx == 0.f) wgt = (i == y0 && j == x0) ? 1.f : 0.f;          // lerp4 reads p00 alone there
            else {
                if (i == y0 && j == x0) wgt += hy * hx;
                if (i == y0 && j == x1) wgt += hy * lx;
                if (i == y1 && j == x0) wgt += ly * hx;
                if (i == y1 && j == x1) wgt += ly * lx;
            }
            acc += coef * wgt;
        }
        dlogit[e] = acc;
    }
}

// ---- the parameter gradient ----------------------------------------------------------------------------------------------------
// stage 1: block `c` of `chunks` sums its rows [c R, (c + 1) R) for every channel quad: lane l of 256 / C4 takes rows l, l + lanes, ...
// in order, then lane 0 adds the lanes in order.  partial [chunks][2][C]: sum g x, sum g.
__global__ __launch_bounds__(256) void brs_param_partial_kernel(const float* __restrict__ g, const float* __restrict__ x, size_t N, int C4,
                                                                size_t rows_per_chunk, float* __restrict__ partial) {
    extern __shared__ float lds[];             // [lanes][2][C]
    const int lanes = 256 / C4, lane = threadIdx.x / C4, q = threadIdx.x % C4, C = C4 * 4;
    const size_t r0 = (size_t)blockIdx.x * rows_per_chunk, r1 = min(N, r0 + rows_per_chunk);
    f32x4 sx = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    if (lane < lanes) {
        for (size_t r = r0 + lane; r < r1; r += lanes) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + (r * C4 + q) * 4);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (r * C4 + q) * 4);
            sx += gv * xv; s1 += gv;
        }
        *reinterpret_cast<f32x4*>(lds + ((size_t)lane * 2 + 0) * C + q * 4) = sx;
        *reinterpret_cast<f32x4*>(lds + ((size_t)lane * 2 + 1) * C + q * 4) = s1;
    }
    __syncthreads();
    if (lane == 0) {
        for (int l = 1; l < lanes; ++l) {
            sx += *reinterpret_cast<const f32x4*>(lds + ((size_t)l * 2 + 0) * C + q * 4);
            s1 += *reinterpret_cast<const f32x4*>(lds + ((size_t)l * 2 + 1) * C + q * 4);
        }
        *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 0) * C + q * 4) = sx;
        *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.x * 2 + 1) * C + q * 4) = s1;
    }
}

// stage 2: one workgroup adds the chunks in order, adds the regulariser's gradient, and thread 0 forms f = data loss + regulariser
__global__ __launch_bounds__(256) void brs_param_final_kernel(const float* __restrict__ partial, int chunks, int C, const float* __restrict__ sb,
                                                              float reg_weight, float reg_bias_weight, float* __restrict__ rec,
                                                              float* __restrict__ grad) {
    for (int c = threadIdx.x; c < 2 * C; c += 256) {
        const int half = c / C, ch = c % C;
        float acc = 0.f;
        for (int k = 0; k < chunks; ++k) acc += partial[((size_t)k * 2 + half) * C + ch];
        grad[c] = acc + 2.f * reg_weight * (half ? reg_bias_weight : 1.f) * sb[c];
    }
    if (threadIdx.x == 0) {
        float ss = 0.f, bb = 0.f;
        for (int c = 0; c < C; ++c) { ss += sb[c] * sb[c]; bb += sb[C + c] * sb[C + c]; }
        rec[REC_F] = rec[REC_LOSS] + reg_weight * (ss + reg_bias_weight * bb);
    }
}

}  // namespace

extern "C" int xmem_brs_affine_nhwc(const float* x, const float* scale_bias, float* y, int B, int h, int w, int C, void* stream) {
    if (!x || !scale_bias || !y || B <= 0 || h <= 0 || w <= 0 || C <= 0) return XMEM_ERR_BAD_ARG;
    if (C % 4 || misaligned(x) || misaligned(scale_bias) || misaligned(y)) return XMEM_ERR_UNSUPPORTED;
    const size_t n4 = (size_t)B * h * w * (C / 4);
    hipLaunchKernelGGL(brs_affine_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, x, scale_bias, y, n4, C / 4);
    return xmem_check_launch();
}

extern "C" int xmem_relu_gate_nhwc(const float* y, const float* g, float* out, size_t n, void* stream) {
    if (!y || !g || !out || n == 0) return XMEM_ERR_BAD_ARG;
    if (n % 4 || misaligned(y) || misaligned(g) || misaligned(out)) return XMEM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(relu_gate_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, y, g, out, n / 4);
    return xmem_check_launch();
}

extern "C" int xmem_relu_gate_outer_nhwc(const float* y, const float* g1, const float* w, float* out, size_t pixels, int C, void* stream) {
    if (!y || !g1 || !w || !out || pixels == 0 || C <= 0) return XMEM_ERR_BAD_ARG;
    if (C % 4 || misaligned(y) || misaligned(w) || misaligned(out)) return XMEM_ERR_UNSUPPORTED;
    const size_t n4 = pixels * (size_t)(C / 4);
    hipLaunchKernelGGL(relu_gate_outer_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, y, g1, w, out, n4, C / 4);
    return xmem_check_launch();
}

extern "C" size_t xmem_brs_loss_workspace_bytes(int B, int cap) {
    return B > 0 && cap > 0 ? (size_t)B * cap * 9 * TERM_WORDS * sizeof(float) : 0;
}

extern "C" int xmem_brs_loss(const float* logits, int B, int h4, int w4, int H, int W, const int32_t* rects, const int32_t* count, int cap,
                             const uint8_t* last_mask, uint8_t* mask, float* record, float* dlogit, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (!logits || !rects || !count || !last_mask || !mask || !record || !dlogit || !workspace) return XMEM_ERR_BAD_ARG;
    if (B < 1 || B > 2 || h4 <= 0 || w4 <= 0 || H <= 0 || W <= 0 || cap <= 0) return XMEM_ERR_BAD_ARG;
    if ((long long)H * h4 > INT_MAX || (long long)W * w4 > INT_MAX || (long long)B * cap * 9 > INT_MAX) return XMEM_ERR_UNSUPPORTED;
    if (workspace_bytes < xmem_brs_loss_workspace_bytes(B, cap) || misaligned(workspace)) return XMEM_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* terms = (float*)workspace;
    hipLaunchKernelGGL(brs_record_init_kernel, dim3(1), dim3(64), 0, s, record);
    hipLaunchKernelGGL(brs_mask_kernel, dim3(grid_for((size_t)H * W, 256, 1024)), dim3(256), 0, s, logits, B, h4, w4, H, W, last_mask, mask,
                       reinterpret_cast<int*>(record) + REC_COUNTS);
    hipLaunchKernelGGL(brs_terms_kernel, dim3(1), dim3(256), 0, s, logits, B, h4, w4, H, W, rects, count, cap, 1e-5f, terms, record);
    hipLaunchKernelGGL(brs_dlogit_kernel, dim3(grid_for((size_t)B * h4 * w4)), dim3(256), 0, s, terms, count, cap, B, h4, w4, dlogit);
    return xmem_check_launch();
}

constexpr int BRS_MAX_CHUNKS = 256;

extern "C" size_t xmem_brs_param_grad_workspace_bytes(int C) {
    return C > 0 ? (size_t)BRS_MAX_CHUNKS * 2 * C * sizeof(float) : 0;
}

extern "C" int xmem_brs_param_grad(const float* g, const float* x, int B, int h, int w, int C, const float* scale_bias, float reg_weight,
                                   float reg_bias_weight, float* record, float* grad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!g || !x || !scale_bias || !record || !grad || !workspace || B <= 0 || h <= 0 || w <= 0 || C <= 0) return XMEM_ERR_BAD_ARG;
    if (C % 4 || C > 1024 || misaligned(g) || misaligned(x) || misaligned(workspace)) return XMEM_ERR_UNSUPPORTED;
    if (workspace_bytes < xmem_brs_param_grad_workspace_bytes(C)) return XMEM_ERR_WORKSPACE;
    const size_t N = (size_t)B * h * w;
    const int C4 = C / 4, lanes = 256 / C4;
    // a chunk holds at least 8 rows per lane; at most BRS_MAX_CHUNKS chunks
    size_t rows = (N + BRS_MAX_CHUNKS - 1) / BRS_MAX_CHUNKS;
    if (rows < (size_t)lanes * 8) rows = (size_t)lanes * 8;
    const int chunks = (int)((N + rows - 1) / rows);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(brs_param_partial_kernel, dim3(chunks), dim3(256), (size_t)lanes * 2 * C * sizeof(float), s, g, x, N, C4, rows,
                       (float*)workspace);
    hipLaunchKernelGGL(brs_param_final_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, chunks, C, scale_bias, reg_weight,
                       reg_bias_weight, record, grad);
    return xmem_check_launch();
}
