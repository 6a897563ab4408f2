// The implicit-GEMM convolution kernels (csrc/conv_mfma.hip): their argument block, the split-operand packing that the Winograd
// input transforms share, and the launchers the entry points (conv.hip) and the Winograd driver (conv_winograd.hip) call.
// Internal to the library (not part of the C ABI).
#pragma once
#include "common.hpp"
#include "conv_plan.hpp"

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

// what every entry point passes to the direct kernels
ConvArgs conv_args(const xmem_conv_desc* d, const conv_plan::Plan& pl, int Ho, int Wo, void* workspace);
// the implicit-GEMM kernel of the plan's tile: `groups` GEMMs (blockIdx.y: the Winograd positions), or the dilated form
int launch_tile(const conv_plan::Plan& pl, const ConvArgs& a, hipStream_t s, int groups = 1, bool dilated = false);
int launch_splitk_reduce(const ConvArgs& a, bool half_out, hipStream_t s);

// tools builds only (-DXMEM_TOOLS): ConvArgs.dbg from the environment (XMEM_CONV_DBG), and the report of the workgroup phase
// timestamps that a launch_tile with dbg & 8 left behind
#ifdef XMEM_TOOLS
int conv_dbg_from_env();
void conv_trace_report(const ConvArgs& a, hipStream_t s);
#else
inline int conv_dbg_from_env() { return 0; }
inline void conv_trace_report(const ConvArgs&, hipStream_t) {}
#endif
