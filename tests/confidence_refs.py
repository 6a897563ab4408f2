"""Inputs for the confidence tests: class scores drawn so that ties and the floor, cap and threshold boundaries occur in numbers."""
import numpy as np

PLANTED = (0, 64, 128, 192, 256)


def scores(rng, C, H, W):
    """float32 [C,H,W] of k / 256: half the values from a palette of five (ties between classes are frequent), half uniform in
    0..256; the first pixel is an all-class tie and the last one has the largest margin there is."""
    k = np.where(rng.random((C, H, W)) < 0.5, rng.choice(PLANTED, size=(C, H, W)), rng.integers(0, 257, size=(C, H, W)))
    k[:, 0, 0] = 128
    if C > 1 and H * W > 1:
        k[:, -1, -1] = 0
        k[C // 2, -1, -1] = 256
    return (k / 256).astype(np.float32)


def sums(rng, C, H, W, passes):
    """uint16 [C,H,W]: sums of `passes` bytes, from the same drawing"""
    return np.minimum(np.round(scores(rng, C, H, W) * 255 * passes), 255 * passes).astype(np.uint16)
