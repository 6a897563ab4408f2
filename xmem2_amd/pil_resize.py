"""Pillow's 8-bit antialiased BILINEAR resize, restated (host side; no torch device needed).

`Image.resize(size, Image.BILINEAR)` on an 8-bit image is integer arithmetic on fixed-point taps (Pillow's Resample.c:
precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc): per axis and output sample a window
`[xmin, xmin + xmax)` of the source and `xmax` triangle-filter weights, normalised in float64 and rounded to 22 fractional bits;
one pass computes `clamp((2**21 + sum(src[xmin + x] * coeff[x])) >> 22, 0, 255)` per channel.  The horizontal pass runs first and is
rounded to uint8, the vertical pass runs on that result; a pass whose input and output size are equal is skipped.  The int32
accumulator cannot overflow: the coefficients of one output sum to 2**22 up to one rounding per tap, 255 * (2**22 + ksize) < 2**31.

`taps` is the table both the numpy emulation below and the HIP kernel (csrc/resize_u8.hip, `ops.resize_u8`) read, so the device
resize is defined by this file and pinned to the installed Pillow by tests/test_pil_resize_host.py, byte for byte.
"""
import functools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
MAX_SIDE = 16384             # include/xmem_hip.h: xmem_resize_u8_bilinear_aa


@functools.lru_cache(maxsize=64)
def taps(in_size, out_size):
    """(bounds int32 [out, 2] = (xmin, xmax), coeffs int32 [out, ksize]) of one axis, BILINEAR filter over the full image box.
    Cached per geometry; the arrays are read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f'taps: sizes must be positive (got {in_size} -> {out_size})')
    scale = float(in_size) / out_size
    fs = max(scale, 1.0)
    support = fs                                            # the triangle filter's support is 1.0
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)          # int() truncates towards zero, as the C cast does
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss))
            w.append(v)
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coeffs[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


def _pass(a, out_size, axis):
    """One axis pass of a uint8 [H, W, C] array."""
    bounds, coeffs = taps(a.shape[axis], out_size)
    src = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        k = coeffs[xx, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (src[xmin:xmin + n] * k).sum(0)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8_host(a, th, tw, flip=False):
    """uint8 [H, W, 3] -> uint8 [th, tw, 3]: what `Image.fromarray(a).resize((tw, th), Image.BILINEAR)` gives, mirrored left-right
    when `flip`.  The numpy emulation of the two kernel passes and the CPU oracle of `taps`."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError('resize_u8_host: expected a uint8 [H, W, C] array')
    if a.shape[1] != tw:
        a = _pass(a, tw, 1)
    if a.shape[0] != th:
        a = _pass(a, th, 0)
    return np.ascontiguousarray(a[:, ::-1] if flip else a)
