// Integer helpers of the host code.  Free of HIP: common.hpp includes this, and so does the convolution planner (conv_plan.hpp),
// which a plain host compiler builds.
#pragma once
#include <stddef.h>

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
