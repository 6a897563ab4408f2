// A bottleneck's expand 1x1 (+ residual + relu) and the next block's reduce 1x1 (+ relu) in one launch (csrc/pointwise_pair.hip).
// Internal to the library (not part of the C ABI): the entry point is xmem_conv2d_pointwise_pair in csrc/conv.hip.
#pragma once
#include "common.hpp"

struct PairArgs {
    const float* A;            // [M][K1], pixel stride lda floats
    const float* W1;           // [N1][K1] expand weights
    const float* scale1;       // per expand channel
    const float* shift1;
    const float* res;          // [M][N1], pixel stride ldres
    const float* W2;           // [N2][N1] reduce weights
    const float* scale2;       // per reduce channel
    const float* shift2;
    float* y;                  // [M][N1], pixel stride ldy:  relu(A W1^T * scale1 + shift1 + res)
    float* z;                  // [M][N2], pixel stride ldz:  relu(y W2^T * scale2 + shift2)
    int M, K1, N1, N2;
    int lda, ldres, ldy, ldz;
};

// K1 in {64, 128, 256} with N1 = 4 K1 and N2 in {64, 128, 256}, N2 in {K1, 2 K1}
bool pointwise_pair_supported(int K1, int N1, int N2);
size_t pointwise_pair_lds_bytes(int N2);
int pointwise_pair_launch(const PairArgs& a, hipStream_t s);
