// Click-to-mask (the f-BRS click network, inference/interact/fbrs/) around its convolutions: the click distance maps with the rgb_conv
// input MLP, depthwise 3x3 convolutions, align_corners=True resampling (NHWC channel slices and planar crop / paste), the flip-averaged
// sigmoid output and the mask bounding box of the zoom-in.  fp32, gfx950.
#include "common.hpp"
#include <limits.h>
#include <math.h>

namespace {

inline int grid_for(size_t n, int block = 256, int cap = 8192) {
    size_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

// F.interpolate(mode='bilinear', align_corners=True): output index o of n_out reads source coordinate o (n_in - 1) / (n_out - 1)
// (0 when n_out == 1).  Integer quotient and remainder: the cell index is exact and the weight is rounded once, so equal sizes give
// weight 0 everywhere and torch's float32 coordinate (scale rounded, product rounded) is at least as far from the real value.
__device__ __forceinline__ void ac_src(int o, int n_in, int n_out, int& i0, int& i1, float& l) {
    if (n_out <= 1 || n_in <= 1) { i0 = i1 = 0; l = 0.f; return; }
    const int den = n_out - 1, num = o * (n_in - 1);
    i0 = num / den;
    const int rem = num - i0 * den;
    i1 = min(i0 + 1, n_in - 1);
    l = (float)rem / (float)den;
}

__device__ __forceinline__ float lerp4(float p00, float p01, float p10, float p11, float ly, float lx) {
    if (ly == 0.f && lx == 0.f) return p00;              // a grid point: the source value itself (equal sizes copy bit for bit)
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11);
}

// ---- click distance maps + rgb_conv ------------------------------------------------------------------------------------------
// DistMaps in cpu mode (fbrs/model/ops.py:46-53, 78; fbrs/utils/cython/_get_dist_maps.pyx) in closed form, then
// DistMapsModel.rgb_conv (is_deeplab_model.py:36-41, 54) per pixel.  par: w1 [8][5], b1 [8], w2 [3][8], b2 [3] with the BatchNorm
// between LeakyReLU and the second convolution folded into w2 / b2 by the caller.
constexpr int RGB_PAR = 8 * 5 + 8 + 3 * 8 + 3;

__global__ __launch_bounds__(256) void click_input_kernel(const float* __restrict__ image, const float* __restrict__ clicks, int cap,
                                                          const int* __restrict__ counts, float radius, const float* __restrict__ par,
                                                          int H, int W, int B, float* __restrict__ out, float* __restrict__ feat) {
    __shared__ float sp[RGB_PAR];
    for (int i = threadIdx.x; i < RGB_PAR; i += blockDim.x) sp[i] = par[i];
    __syncthreads();
    const size_t P = (size_t)H * W, total = (size_t)B * P;
    const int n[2] = {min(max(counts[0], 0), cap), min(max(counts[1], 0), cap)};
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int s = (int)(e / P), pix = (int)(e % P);
        const int y = pix / W, x = pix % W;
        const int xs = s ? W - 1 - x : x;                 // sample 1: the mirrored image (AddHorizontalFlip, transforms/flip.py:8-21)
        float in5[5];
        in5[0] = image[(size_t)y * W + xs]; in5[1] = image[P + (size_t)y * W + xs]; in5[2] = image[2 * P + (size_t)y * W + xs];
#pragma unroll
        for (int pol = 0; pol < 2; ++pol) {
            float d = 1e6f;
            const float* c = clicks + (size_t)pol * cap * 2;
            for (int i = 0; i < n[pol]; ++i) {
                const float cr = rintf(c[2 * i]);
                const float cc = rintf(s ? (float)(W - 1) - c[2 * i + 1] : c[2 * i + 1]);
                if (!(cr >= 0.f && cr < (float)H && cc >= 0.f && cc < (float)W)) continue;
                const float dy = ((float)y - cr) / radius, dx = ((float)x - cc) / radius;
                d = fminf(d, dy * dy + dx * dx);
            }
            const float f = tanhf(2.f * sqrtf(d));
            in5[3 + pol] = f;
            if (feat) feat[((size_t)s * 2 + pol) * P + pix] = f;
        }
        float o[3] = {sp[72], sp[73], sp[74]};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float a = sp[40 + j];
#pragma unroll
            for (int k = 0; k < 5; ++k) a += sp[j * 5 + k] * in5[k];
            a = a > 0.f ? a : 0.2f * a;
#pragma unroll
            for (int m = 0; m < 3; ++m) o[m] += sp[48 + m * 8 + j] * a;
        }
        const f32x4 lo = {o[0], o[1], o[2], 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(out + e * 8) = lo;
        *reinterpret_cast<f32x4*>(out + e * 8 + 4) = hi;
    }
}

// ---- depthwise 3x3 -----------------------------------------------------------------------------------------------------------
// nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False) of SeparableConv2d (fbrs/model/modeling/basic_blocks.py:63-64) on NHWC.
// One thread per (pixel, channel quad): nine 16-byte loads of neighbouring pixels (consecutive lanes read consecutive quads of one
// pixel, so a wave reads whole pixels) and nine of the weights [9][C].
__global__ __launch_bounds__(256) void depthwise3x3_kernel(const float* __restrict__ in, int ldin, const float* __restrict__ w,
                                                           float* __restrict__ out, int ldout, int B, int H, int W, int C4) {
    const size_t total = (size_t)B * H * W * C4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(e % C4);
        const size_t pix = e / C4;
        const int x = (int)(pix % W), y = (int)((pix / W) % H);
        const size_t img = pix - ((size_t)y * W + x);     // first pixel of this batch element
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + ky - 1;
            if ((unsigned)yy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = x + kx - 1;
                if ((unsigned)xx >= (unsigned)W) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(in + (img + (size_t)yy * W + xx) * ldin + q * 4);
                const f32x4 k = *reinterpret_cast<const f32x4*>(w + ((size_t)(ky * 3 + kx) * C4 + q) * 4);
                acc += v * k;
            }
        }
        *reinterpret_cast<f32x4*>(out + pix * ldout + q * 4) = acc;
    }
}

// ---- align_corners=True resampling ---------------------------------------------------------------------------------------------
__global__ void resize_ac_nhwc_kernel(const float* __restrict__ in, int ldin, int Hi, int Wi, float* __restrict__ out, int ldout,
                                      int Ho, int Wo, int C4, int B) {
    const size_t total = (size_t)B * Ho * Wo * C4;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(e % C4);
        const size_t pix = e / C4;
        const int x = (int)(pix % Wo), y = (int)((pix / Wo) % Ho), b = (int)(pix / ((size_t)Wo * Ho));
        int y0, y1, x0, x1; float ly, lx;
        ac_src(y, Hi, Ho, y0, y1, ly);
        ac_src(x, Wi, Wo, x0, x1, lx);
        const float* p = in + (size_t)b * Hi * Wi * ldin + q * 4;
        const f32x4 p00 = *reinterpret_cast<const f32x4*>(p + ((size_t)y0 * Wi + x0) * ldin);
        f32x4 v = p00;
        if (ly != 0.f || lx != 0.f) {
            const f32x4 p01 = *reinterpret_cast<const f32x4*>(p + ((size_t)y0 * Wi + x1) * ldin);
            const f32x4 p10 = *reinterpret_cast<const f32x4*>(p + ((size_t)y1 * Wi + x0) * ldin);
            const f32x4 p11 = *reinterpret_cast<const f32x4*>(p + ((size_t)y1 * Wi + x1) * ldin);
            const float hy = 1.f - ly, hx = 1.f - lx;
            v = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11);
        }
        *reinterpret_cast<f32x4*>(out + pix * ldout + q * 4) = v;
    }
}

// planar [C][Hi][Wi]: the crop rows [r0, r0 + Hc) x columns [c0, c0 + Wc) resized to Hd x Wd and written at (pr0, pc0) of [C][Ho][Wo];
// fill: the threads cover the whole destination and write zeros outside the rectangle, else only the rectangle
__global__ void resize_ac_kernel(const float* __restrict__ in, int C, int Hi, int Wi, int r0, int c0, int Hc, int Wc,
                                 float* __restrict__ out, int Ho, int Wo, int pr0, int pc0, int Hd, int Wd, int fill) {
    const int Ht = fill ? Ho : Hd, Wt = fill ? Wo : Wd;
    const size_t total = (size_t)C * Ht * Wt;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int tx = (int)(e % Wt), ty = (int)((e / Wt) % Ht), c = (int)(e / ((size_t)Wt * Ht));
        const int oy = fill ? ty : ty + pr0, ox = fill ? tx : tx + pc0;       // destination pixel
        const int y = oy - pr0, x = ox - pc0;                                  // position inside the rectangle
        float v = 0.f;
        if ((unsigned)y < (unsigned)Hd && (unsigned)x < (unsigned)Wd) {
            int y0, y1, x0, x1; float ly, lx;
            ac_src(y, Hc, Hd, y0, y1, ly);
            ac_src(x, Wc, Wd, x0, x1, lx);
            const float* p = in + ((size_t)c * Hi + r0) * Wi + c0;
            v = lerp4(p[(size_t)y0 * Wi + x0], p[(size_t)y0 * Wi + x1], p[(size_t)y1 * Wi + x0], p[(size_t)y1 * Wi + x1], ly, lx);
        }
        out[((size_t)c * Ho + oy) * Wo + ox] = v;
    }
}

// ---- output ------------------------------------------------------------------------------------------------------------------
// DistMapsModel.forward's upsample (is_deeplab_model.py:63-64), AddHorizontalFlip.inv_transform on the LOGITS (flip.py:23-28; it is
// the last transform, so its inverse runs first: predictors/base.py:46-47) and SigmoidForPred
__global__ void click_prob_kernel(const float* __restrict__ logits, int h4, int w4, int H, int W, int with_flip, float* __restrict__ prob) {
    const size_t P = (size_t)H * W;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < P; e += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(e % W), y = (int)(e / W);
        int y0, y1, x0, x1; float ly, lx;
        ac_src(y, h4, H, y0, y1, ly);
        ac_src(x, w4, W, x0, x1, lx);
        const float* l = logits;
        float v = lerp4(l[(size_t)y0 * w4 + x0], l[(size_t)y0 * w4 + x1], l[(size_t)y1 * w4 + x0], l[(size_t)y1 * w4 + x1], ly, lx);
        if (with_flip) {
            ac_src(W - 1 - x, w4, W, x0, x1, lx);
            l = logits + (size_t)h4 * w4;
            const float u = lerp4(l[(size_t)y0 * w4 + x0], l[(size_t)y0 * w4 + x1], l[(size_t)y1 * w4 + x0], l[(size_t)y1 * w4 + x1], ly, lx);
            v = 0.5f * (v + u);
        }
        prob[e] = sigmoidf_(v);
    }
}

// ---- bounding box of prob > threshold ------------------------------------------------------------------------------------------
__global__ void mask_bbox_init_kernel(int* __restrict__ out) {
    if (threadIdx.x == 0) { out[0] = INT_MAX; out[1] = -1; out[2] = INT_MAX; out[3] = -1; out[4] = 0; }
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// get_bbox_from_mask (fbrs/utils/misc.py:19-25) of prob > thr, with the pixels of `pix` [n][2] (row, col; get_object_roi sets the
// positive clicks, transforms/zoom_in.py:130-132) joining the box but not the count.  Integer min / max / add: exact in any order.
__global__ __launch_bounds__(256) void mask_bbox_kernel(const float* __restrict__ prob, int H, int W, float thr, const int* __restrict__ pix,
                                                        int n, int* __restrict__ out) {
    int rmin = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1, cnt = 0;
    const size_t P = (size_t)H * W, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t e = t0; e < P; e += (size_t)gridDim.x * blockDim.x) {
        if (prob[e] > thr) {
            const int y = (int)(e / W), x = (int)(e % W);
            rmin = min(rmin, y); rmax = max(rmax, y); cmin = min(cmin, x); cmax = max(cmax, x); ++cnt;
        }
    }
    if (t0 < (size_t)n) {
        const int y = pix[2 * t0], x = pix[2 * t0 + 1];
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
            rmin = min(rmin, y); rmax = max(rmax, y); cmin = min(cmin, x); cmax = max(cmax, x);
        }
    }
    rmin = wave_min_i(rmin); rmax = wave_max_i(rmax); cmin = wave_min_i(cmin); cmax = wave_max_i(cmax); cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0 && rmax >= 0) {
        atomicMin(out + 0, rmin); atomicMax(out + 1, rmax); atomicMin(out + 2, cmin); atomicMax(out + 3, cmax);
        if (cnt) atomicAdd(out + 4, cnt);
    }
}

// (prob > threshold).float(): the mask FBRSController.interact returns (fbrs_controller.py:46)
__global__ void prob_threshold_kernel(const float* __restrict__ prob, size_t n, float thr, float* __restrict__ out) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x)
        out[e] = prob[e] > thr ? 1.f : 0.f;
}

bool misaligned(const void* p) { return (((uintptr_t)p) & 15) != 0; }

}  // namespace

extern "C" int xmem_click_input(const float* image, const float* clicks, int cap, const int32_t* counts, float radius,
                                const float* rgb_conv, int H, int W, int with_flip, float* out, float* features, void* stream) {
    if (!image || !clicks || !counts || !rgb_conv || !out || cap <= 0 || H <= 0 || W <= 0 || !(radius > 0.f)) return XMEM_ERR_BAD_ARG;
    if (misaligned(out)) return XMEM_ERR_UNSUPPORTED;
    const int B = with_flip ? 2 : 1;
    hipLaunchKernelGGL(click_input_kernel, dim3(grid_for((size_t)B * H * W)), dim3(256), 0, (hipStream_t)stream,
                       image, clicks, cap, counts, radius, rgb_conv, H, W, B, out, features);
    return xmem_check_launch();
}

extern "C" int xmem_depthwise3x3_nhwc(const float* in, int ldin, const float* w, float* out, int ldout, int B, int H, int W, int C,
                                      void* stream) {
    if (!in || !w || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || ldin < C || ldout < C) return XMEM_ERR_BAD_ARG;
    if (C % 4 || ldin % 4 || ldout % 4 || misaligned(in) || misaligned(w) || misaligned(out)) return XMEM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(depthwise3x3_kernel, dim3(grid_for((size_t)B * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       in, ldin, w, out, ldout, B, H, W, C / 4);
    return xmem_check_launch();
}

extern "C" int xmem_resize_bilinear_ac_nhwc(const float* in, int ldin, int B, int Hi, int Wi, int C, float* out, int ldout,
                                            int Ho, int Wo, void* stream) {
    if (!in || !out || B <= 0 || Hi <= 0 || Wi <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || ldin < C || ldout < C) return XMEM_ERR_BAD_ARG;
    if (C % 4 || ldin % 4 || ldout % 4 || misaligned(in) || misaligned(out)) return XMEM_ERR_UNSUPPORTED;
    if ((long long)Ho * Hi > INT_MAX || (long long)Wo * Wi > INT_MAX) return XMEM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(resize_ac_nhwc_kernel, dim3(grid_for((size_t)B * Ho * Wo * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       in, ldin, Hi, Wi, out, ldout, Ho, Wo, C / 4, B);
    return xmem_check_launch();
}

extern "C" int xmem_resize_bilinear_ac(const float* in, int C, int Hi, int Wi, int r0, int c0, int Hc, int Wc,
                                       float* out, int Ho, int Wo, int pr0, int pc0, int Hd, int Wd, int zero_fill, void* stream) {
    if (!in || !out || C <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0 || Hc <= 0 || Wc <= 0 || Hd <= 0 || Wd <= 0) return XMEM_ERR_BAD_ARG;
    if (r0 < 0 || c0 < 0 || r0 + Hc > Hi || c0 + Wc > Wi || pr0 < 0 || pc0 < 0 || pr0 + Hd > Ho || pc0 + Wd > Wo) return XMEM_ERR_BAD_ARG;
    if ((long long)Hd * Hc > INT_MAX || (long long)Wd * Wc > INT_MAX) return XMEM_ERR_UNSUPPORTED;
    const size_t total = (size_t)C * (zero_fill ? (size_t)Ho * Wo : (size_t)Hd * Wd);
    hipLaunchKernelGGL(resize_ac_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                       in, C, Hi, Wi, r0, c0, Hc, Wc, out, Ho, Wo, pr0, pc0, Hd, Wd, zero_fill ? 1 : 0);
    return xmem_check_launch();
}

extern "C" int xmem_click_prob(const float* logits, int h4, int w4, int H, int W, int with_flip, float* prob, void* stream) {
    if (!logits || !prob || h4 <= 0 || w4 <= 0 || H <= 0 || W <= 0) return XMEM_ERR_BAD_ARG;
    if ((long long)H * h4 > INT_MAX || (long long)W * w4 > INT_MAX) return XMEM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(click_prob_kernel, dim3(grid_for((size_t)H * W)), dim3(256), 0, (hipStream_t)stream,
                       logits, h4, w4, H, W, with_flip ? 1 : 0, prob);
    return xmem_check_launch();
}

extern "C" int xmem_mask_bbox(const float* prob, int H, int W, float threshold, const int32_t* click_pixels, int n_clicks,
                              int32_t* out, void* stream) {
    if (!prob || !out || H <= 0 || W <= 0 || n_clicks < 0 || (n_clicks > 0 && !click_pixels)) return XMEM_ERR_BAD_ARG;
    const int grid = grid_for((size_t)H * W, 256, 1024);
    if ((size_t)n_clicks > (size_t)grid * 256) return XMEM_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(mask_bbox_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out);
    hipLaunchKernelGGL(mask_bbox_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, prob, H, W, threshold, click_pixels, n_clicks, out);
    return xmem_check_launch();
}

extern "C" int xmem_prob_threshold(const float* prob, size_t n, float threshold, float* out, void* stream) {
    if (!prob || !out || n == 0) return XMEM_ERR_BAD_ARG;
    hipLaunchKernelGGL(prob_threshold_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, prob, n, threshold, out);
    return xmem_check_launch();
}
