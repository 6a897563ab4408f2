// The convolution planner (xmem2_amd/csrc/conv_plan.hpp) on its own, built by a plain host compiler - no HIP, no GPU:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/conv_plan_sweep.cpp -o conv_plan_sweep
// Reads layers from stdin, one per line: the 12 integers B H W Cin ldin Cout K stride pad ldout ldres out_off (LAYER_COLS of
// tests/test_conv_plan_host.py), and walks that test's grid over each: operand sets x modes x plan_tile -1..42 x plan_splitk
// {0, 1, 3, 64}, then dilations {1, 2, 6} x plan_tile 0..7 x the same split-Ks.  One line per descriptor, in the order of the test's
// query():  "I rc form bm bn bk splitk stream ring workspace_bytes"  and  "D dilated_workspace_bytes".
// tests/test_conv_plan_host.py runs it under the sanitizers against tests/golden/conv_plan_info.npz.
#include <stdio.h>
#include "../xmem2_amd/csrc/conv_plan.hpp"

namespace {

const int kSplitKs[4] = {0, 1, 3, 64};
const int kDilations[3] = {1, 2, 6};
char* const kPtr = reinterpret_cast<char*>(0x10000);              // nothing is dereferenced: any non-null 16-byte-aligned value

// make_desc of the test: operands 0 = {w_winograd, w_winograd4, w_winograd_f16}, 1 = {w_winograd}, 2 = {}; mode 0 = fp32, 1 = fp32x,
// 2 = fp32x + w_winograd4_split, 3 = half with fp32 output, 4 = half with half output
xmem_conv_desc make_desc(const long* r, int operands, int mode) {
    xmem_conv_desc d = {};
    const float* p = reinterpret_cast<const float*>(kPtr);
    d.in = p; d.w = p; d.scale = p; d.shift = p;
    d.B = (int)r[0]; d.H = (int)r[1]; d.W = (int)r[2]; d.Cin = (int)r[3]; d.ldin = (int)r[4];
    d.Cout = (int)r[5]; d.KH = (int)r[6]; d.KW = (int)r[6]; d.stride = (int)r[7]; d.pad = (int)r[8];
    d.out = reinterpret_cast<float*>(kPtr + r[11]); d.ldout = (int)r[9];
    if (r[10]) { d.res = p; d.ldres = (int)r[10]; }
    if (operands <= 1) d.w_winograd = p;
    if (operands == 0) { d.w_winograd4 = p; d.w_winograd_f16 = p; }
    if (mode == 1 || mode == 2) {
        d.arith = 1; d.w_split = p;
        d.w_winograd_split = operands <= 1 ? p : nullptr;
        d.w_winograd4_split = mode == 2 && operands == 0 ? p : nullptr;
    }
    if (mode >= 3) { d.in_half = 1; d.out_half = mode == 4; d.w_half = p; }
    return d;
}

}  // namespace

int main() {
    long r[12];
    while (scanf("%ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld", r, r + 1, r + 2, r + 3, r + 4, r + 5, r + 6, r + 7, r + 8, r + 9, r + 10,
                 r + 11) == 12) {
        for (int operands = 0; operands < 3; ++operands)
            for (int mode = 0; mode < 5; ++mode) {
                xmem_conv_desc d = make_desc(r, operands, mode);
                for (d.plan_tile = -1; d.plan_tile <= 42; ++d.plan_tile)
                    for (int sk : kSplitKs) {
                        d.plan_splitk = sk;
                        xmem_conv_plan_info pi = {};
                        const int rc = conv_plan::plan_info(&d, &pi);
                        if (rc != XMEM_OK) pi = {};
                        printf("I %d %d %d %d %d %d %d %d %zu\n", rc, pi.form, pi.bm, pi.bn, pi.bk, pi.splitk, pi.stream, pi.ring,
                               conv_plan::workspace_bytes(&d));
                    }
            }
        xmem_conv_desc d = make_desc(r, 0, 0);
        for (int dil : kDilations)
            for (d.plan_tile = 0; d.plan_tile <= 7; ++d.plan_tile)
                for (int sk : kSplitKs) {
                    d.plan_splitk = sk;
                    printf("D %zu\n", conv_plan::dilated_workspace_bytes(&d, dil));
                }
    }
    return 0;
}
