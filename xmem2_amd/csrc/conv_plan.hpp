// The convolution planner: what a descriptor's plan_tile / plan_splitk resolve to, the argument checks, the workspace formulas and
// the bodies of the pure size / plan queries of the C ABI.  Integer logic only and free of HIP: the kernel units (conv.hip,
// conv_mfma.hip, conv_winograd.hip) include it, and a plain host compiler builds it for tools/conv_plan_sweep.cpp, which runs
// it under the sanitizers (tests/test_conv_plan_host.py).  Internal to the library (not part of the C ABI).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/xmem_hip.h"
#include "host_math.hpp"

namespace conv_plan {

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

inline int stream_variant(const Plan& pl) { return pl.bm == 64 ? 0 : (pl.bn == 64 ? 1 : 2); }     // gemm_stream.hpp: 64x64, 128x64, 128x128

inline bool wino_ok(const xmem_conv_desc* d) {
    return d->w_winograd && d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == 1 && d->Cin % 32 == 0 && d->Cout % 4 == 0 &&
           d->ldout % 4 == 0 && (!d->res || d->ldres % 4 == 0) && (((uintptr_t)d->out) & 15) == 0 && (!d->res || (((uintptr_t)d->res) & 15) == 0);
}

// argument checks common to the plain (dilation 1, codes 0..40) and the dilated (codes 0..6) entry points
inline int validate(const xmem_conv_desc* d, int dilation = 1, int max_code = 40) {
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
inline Plan make_plan(const xmem_conv_desc* d, int code) {
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
inline bool half_view(const xmem_conv_desc* d, xmem_conv_desc& v) {
    if (!d->w_half || d->Cin % 8 != 0 || d->ldin % 8 != 0 || (((uintptr_t)d->in) & 15) != 0 || (((uintptr_t)d->w_half) & 15) != 0) return false;
    v = *d;
    v.Cin = d->Cin / 2; v.ldin = d->ldin / 2;
    v.w_winograd = nullptr; v.w_winograd4 = nullptr; v.w_winograd_f16 = nullptr; v.arith = 0; v.w_split = nullptr;
    return true;
}

// plan of a half-typed call (v: its half view); the 256x128 tile keeps the split-K of the 128x128 plan it is made from
inline Plan make_plan_half(const xmem_conv_desc* v) {
    Plan pl = make_plan(v, v->plan_tile <= 6 ? kHalfCodes[v->plan_tile] : 0);
    if (v->plan_tile == 4 && pl.form == DIRECT) { pl.bm = 256; pl.bn = 128; }
    return pl;
}

// the plan of a validated descriptor; a half-typed call continues on its half view `hv` (false: it has none)
inline bool plan_of(const xmem_conv_desc*& d, xmem_conv_desc& hv, Plan& pl) {
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
// the Winograd kernels carry the tile count P in an int
inline bool wino_tiles_fit(size_t P) { return P <= 0x7fffffff; }
// V [(r+2)^2][P][Cin] and, unless the GEMM transforms its own output (fused), M [(r+2)^2][P][Cout]
inline size_t wino_workspace(size_t P, int r, int Cin, int Cout, bool fused) {
    return (size_t)(r + 2) * (r + 2) * P * (Cin + (fused ? 0 : Cout)) * sizeof(float);
}
inline size_t wino_f16_v_bytes(size_t P, int Cin) { return align_up((size_t)16 * P * Cin * 2, 256); }
inline size_t splitk_workspace(const Plan& pl, const xmem_conv_desc* d, int Ho, int Wo) {
    return pl.splitk == 1 ? 0 : (size_t)pl.splitk * d->B * Ho * Wo * d->Cout * sizeof(float);
}
inline size_t workspace_need(const Plan& pl, const xmem_conv_desc* d, int Ho, int Wo) {
    if (pl.form == F4) return wino_workspace(wino_tiles(d, Ho, Wo, 4), 4, d->Cin, d->Cout, false);
    const size_t P = wino_tiles(d, Ho, Wo, 2);
    if (pl.form == F2_F16) return wino_f16_v_bytes(P, d->Cin) + (size_t)16 * P * d->Cout * sizeof(float);
    if (pl.form == F2 || pl.form == F2_FUSED) return wino_workspace(P, 2, d->Cin, d->Cout, pl.form == F2_FUSED);
    return splitk_workspace(pl, d, Ho, Wo);
}

// ---- dilated convolution (xmem_conv2d_nhwc_dilated): the direct tiles only (plan codes 0..6, split-K as in make_plan); no Winograd,
// no fp16 / split-operand modes, Cout >= 2 ----
inline int validate_dilated(const xmem_conv_desc* d, int dilation) {
    const int rc = validate(d, dilation, 6);
    if (rc != XMEM_OK) return rc;
    if (d->Cout == 1 || d->in_half || d->out_half || d->arith != 0 || d->res_broadcast) return XMEM_ERR_UNSUPPORTED;
    if ((long)dilation * (d->KH - 1) > (1 << 20) || (long)dilation * (d->KW - 1) > (1 << 20)) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

// the plan of the undilated descriptor with the same output size: H' = H - (dil - 1)(KH - 1) gives (H' + 2 pad - KH) / s + 1 =
// (H + 2 pad - dil (KH - 1) - 1) / s + 1 (make_plan only reads the output size, K, Cin and Cout of a direct plan)
inline Plan make_plan_dilated(const xmem_conv_desc* d, int dilation) {
    xmem_conv_desc v = *d;
    v.H = d->H - (dilation - 1) * (d->KH - 1);
    v.W = d->W - (dilation - 1) * (d->KW - 1);
    v.w_winograd = nullptr; v.w_winograd4 = nullptr; v.w_winograd_f16 = nullptr; v.w_split = nullptr; v.arith = 0;
    return make_plan(&v, v.plan_tile);
}

// ---- shared transforms (xmem_conv2d_shared_input, xmem_conv2d_nhwc_folded) ----
// An fp32 convolution whose plan is F(4x4) on unsplit operands: what the shared entry points run.  XMEM_OK and the plan, or why not.
inline int f4_plan_of(const xmem_conv_desc* d, Plan& pl) {
    const int rc = validate(d);
    if (rc != XMEM_OK) return rc;
    if (d->in_half || d->out_half) return XMEM_ERR_UNSUPPORTED;
    pl = make_plan(d, d->plan_tile);
    if (pl.form != F4 || pl.split) return XMEM_ERR_UNSUPPORTED;
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    if (!wino_tiles_fit(wino_tiles(d, Ho, Wo, 4))) return XMEM_ERR_UNSUPPORTED;
    return XMEM_OK;
}

inline size_t f4_m_bytes(const xmem_conv_desc* d) {
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    return (size_t)36 * wino_tiles(d, Ho, Wo, 4) * d->Cout * sizeof(float);
}

// The layout of xmem_conv2d_shared_input's workspace: V of the raw input (when a consumer reads it), V of relu(input) (likewise),
// then one M as wide as the widest consumer (the consumers run one after the other on the stream).
struct SharedLayout { size_t P, v_floats, m_floats; int n_raw, n_relu; };
inline int shared_layout(const xmem_conv_desc* const* ds, int n, Plan* pls, SharedLayout& L) {
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

// ---- the pure queries of the C ABI (the extern "C" symbols in conv.hip are one-line wrappers) ----
inline size_t workspace_bytes(const xmem_conv_desc* d) {
    xmem_conv_desc hv; Plan pl;
    if (validate(d) != XMEM_OK || !plan_of(d, hv, pl)) return 0;
    int Ho, Wo; out_dims(d, 1, Ho, Wo);
    return workspace_need(pl, d, Ho, Wo);
}

inline int plan_info(const xmem_conv_desc* d, xmem_conv_plan_info* out) {
    if (!out) return XMEM_ERR_BAD_ARG;
    const int rc = validate(d);
    if (rc != XMEM_OK) return rc;
    xmem_conv_desc hv; Plan pl;
    if (!storage_types_ok(d) || !plan_of(d, hv, pl)) return XMEM_ERR_UNSUPPORTED;
    out->form = pl.form; out->bm = pl.bm; out->bn = pl.bn; out->bk = pl.bk; out->splitk = pl.splitk;
    out->stream = pl.ring ? 1 : 0; out->ring = pl.ring;
    return XMEM_OK;
}

inline size_t dilated_workspace_bytes(const xmem_conv_desc* d, int dilation) {
    if (validate_dilated(d, dilation) != XMEM_OK) return 0;
    int Ho, Wo; out_dims(d, dilation, Ho, Wo);
    return splitk_workspace(make_plan_dilated(d, dilation), d, Ho, Wo);
}

inline size_t m_bytes(const xmem_conv_desc* d) {
    Plan pl;
    return f4_plan_of(d, pl) == XMEM_OK ? f4_m_bytes(d) : 0;
}

inline size_t shared_input_workspace_bytes(const xmem_conv_desc* const* descs, int n) {
    Plan pls[XMEM_CONV_SHARED_MAX]; SharedLayout L;
    return shared_layout(descs, n, pls, L) == XMEM_OK ? shared_bytes(L) : 0;
}

}  // namespace conv_plan
