// The convolution entry points of the C ABI, and the Cout = 1 kernels (the decoder's mask head and its fused tail).
// An entry point validates and plans (csrc/conv_plan.hpp), checks the workspace, and dispatches on the plan's form: the
// implicit-GEMM kernels (csrc/conv_mfma.hip), the Winograd forms (csrc/conv_winograd.hip), the streaming kernel
// (csrc/gemm_stream.hip), the pointwise pair (csrc/pointwise_pair.hip) or the GEMV kernels below.
#include "conv_winograd.hpp"
#include "gemm_stream.hpp"
#include "pointwise_pair.hpp"

using namespace conv_plan;

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
// host side
// ----------------------------------------------------------------------------------------------
namespace {

// pointwise convolution on the streaming kernel, fused epilogue
int launch_pointwise_stream(const Plan& pl, const xmem_conv_desc* d, const ConvArgs& a, hipStream_t s) {
    GemmStreamArgs g = {};
    g.A = d->in; g.B = d->w; g.C = d->out; g.scale = d->scale; g.shift = d->shift; g.res = d->res;
    g.M = a.M; g.N = d->Cout; g.K = d->Cin; g.G = 1;
    g.lda = d->ldin; g.ldb = d->Cin; g.ldc = d->ldout; g.ldres = d->ldres;
    g.mode = 1; g.relu_in = d->relu_in; g.relu_out = d->relu_out; g.res_mod = a.res_mod;
    g.stride = d->stride; g.H = d->H; g.W = d->W; g.Wo = a.Wo; g.HoWo = a.HoWo;
    return gemm_stream_launch(g, stream_variant(pl), pl.ring, s);
}

int launch_cout1(const ConvArgs& a, int half, hipStream_t s) {
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

}  // namespace

extern "C" size_t xmem_conv2d_workspace_bytes(const xmem_conv_desc* d) { return conv_plan::workspace_bytes(d); }
extern "C" int xmem_conv2d_plan_info(const xmem_conv_desc* d, xmem_conv_plan_info* out) { return conv_plan::plan_info(d, out); }
extern "C" size_t xmem_conv2d_dilated_workspace_bytes(const xmem_conv_desc* d, int dilation) { return conv_plan::dilated_workspace_bytes(d, dilation); }
extern "C" size_t xmem_conv2d_m_bytes(const xmem_conv_desc* d) { return conv_plan::m_bytes(d); }
extern "C" size_t xmem_conv2d_shared_input_workspace_bytes(const xmem_conv_desc* const* descs, int n) {
    return conv_plan::shared_input_workspace_bytes(descs, n);
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
    a.dbg = conv_dbg_from_env();
    if (winograd(pl)) return run_winograd(pl, d, a, workspace, s);
    if (pl.ring) return launch_pointwise_stream(pl, d, a, s);
    if (pl.form == GEMV) return launch_cout1(a, half, s);
    if ((rc = launch_tile(pl, a, s)) != XMEM_OK) return rc;
    conv_trace_report(a, s);
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
    float* Vraw = reinterpret_cast<float*>(workspace);
    float* Vrelu = Vraw + (L.n_raw ? L.v_floats : 0);
    float* Mt = Vrelu + (L.n_relu ? L.v_floats : 0);
    // one V per distinct relu_in, from one launch; with both, raw first
    wino_input(F4, d0, L.P, L.n_raw ? 0 : 1, Vraw, false, s, L.n_raw && L.n_relu ? Vrelu : nullptr, 1);
    if ((rc = xmem_check_launch()) != XMEM_OK) return rc;
    for (int i = 0; i < n; ++i) {                  // each consumer under its own plan: position GEMMs, then its output transform
        const xmem_conv_desc* d = descs[i];
        const ConvArgs a = conv_args(d, pls[i], Ho, Wo, nullptr);
        float* m = defer_m && defer_m[i] ? reinterpret_cast<float*>(defer_m[i]) : Mt;
        if ((rc = wino_position_gemm(pls[i], d, a, 4, d->relu_in ? Vrelu : Vraw, m, L.P, s)) != XMEM_OK) return rc;
        if (m == Mt && (rc = wino_output(F4, d, Ho, Wo, Mt, L.P, s)) != XMEM_OK) return rc;
    }
    return XMEM_OK;
}

extern "C" int xmem_conv2d_output_from_m(const xmem_conv_desc* d, const void* m, size_t m_bytes, void* stream) {
    Plan pl;
    const int rc = f4_plan_of(d, pl);
    if (rc != XMEM_OK) return rc;
    if (!m || m_bytes < f4_m_bytes(d)) return XMEM_ERR_WORKSPACE;
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    return wino_output(F4, d, Ho, Wo, reinterpret_cast<const float*>(m), wino_tiles(d, Ho, Wo, 4), reinterpret_cast<hipStream_t>(stream));
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
    const size_t P = wino_tiles(d, Ho, Wo, 4);
    float* V = reinterpret_cast<float*>(workspace);
    float* Mt = V + (size_t)36 * P * d->Cin;
    wino_input(F4, d, P, d->relu_in, V, false, s);
    const ConvArgs a = conv_args(d, pl, Ho, Wo, nullptr);
    if ((rc = wino_position_gemm(pl, d, a, 4, V, Mt, P, s)) != XMEM_OK) return rc;
    return wino_output_fold(d, branch, Ho, Wo, Mt, reinterpret_cast<const float*>(branch_m), P, s);
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

// Dilated convolution: the direct implicit GEMM with tap spacing `dilation` (the DIL kernels of conv_mfma.hip; validate_dilated /
// make_plan_dilated in conv_plan.hpp).  With dilation 1 and the same plan the products and their order are those of
// xmem_conv2d_nhwc: the same bits.
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
