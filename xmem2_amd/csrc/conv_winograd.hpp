// The Winograd forms of the 3x3 / stride 1 / pad 1 convolutions (csrc/conv_winograd.hip): the whole convolution (run_winograd) and
// the three steps the shared-transform entry points of conv.hip put together themselves.  `form` is a form of conv_plan.hpp:
// F2 / F2_FUSED (fp32 F(2x2)), F2_F16, F4.  Internal to the library (not part of the C ABI).
#pragma once
#include "conv_mfma.hpp"

// Input transform of `d`'s input under activation flag `relu_in` into V (F2_F16: halfs; `split`: [hi4|lo4] groups).  F4 with V2: the
// same launch also writes the variant under `relu_in2` into V2 (blockIdx.y = 1).  P = wino_tiles of the form.
void wino_input(int form, const xmem_conv_desc* d, size_t P, int relu_in, void* V, bool split, hipStream_t s,
                float* V2 = nullptr, int relu_in2 = 0);
// The (r+2)^2 position GEMMs M[xi] = V[xi] U[xi]^T of [P x Cin] x [Cin x Cout], r = 2 or 4
int wino_position_gemm(const conv_plan::Plan& pl, const xmem_conv_desc* d, const ConvArgs& a, int r, const float* V, float* Mt, size_t P,
                       hipStream_t s);
// output transform + epilogue of `d` from its M
int wino_output(int form, const xmem_conv_desc* d, int Ho, int Wo, const float* Mt, size_t P, hipStream_t s);
// F4 output transform of `d` (M in Mt) with the output transform + epilogue of `branch` (M in Mb) folded in as its residual
int wino_output_fold(const xmem_conv_desc* d, const xmem_conv_desc* branch, int Ho, int Wo, const float* Mt, const float* Mb, size_t P,
                     hipStream_t s);
// the convolution of a Winograd plan: input transform -> V, GEMMs, output transform + epilogue (workspace: workspace_need bytes)
int run_winograd(const conv_plan::Plan& pl, const xmem_conv_desc* d, const ConvArgs& a, void* workspace, hipStream_t s);
