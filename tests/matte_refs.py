"""Brute-force restatements of xmem2_amd/matte.py over all pairs of pixels, and the inputs that test_matte_host.py and
test_gpu_matte.py share.  O((H W)^2): for maps of a few hundred pixels."""
import numpy as np


def _pair_d2(h, w):
    """int64 [HW, HW]: the squared distance between every two pixel centres"""
    yy, xx = np.divmod(np.arange(h * w, dtype=np.int64), w)
    return (yy[:, None] - yy[None]) ** 2 + (xx[:, None] - xx[None]) ** 2


def signed_d2_brute(m, k, R):
    h, w = m.shape
    cap2 = (R + 1) ** 2
    d2 = _pair_d2(h, w)
    inside = (m == k).reshape(-1)
    out = np.empty(h * w, np.int64)
    for side, sign in ((inside, 1), (~inside, -1)):
        if side.any():
            others = d2[np.ix_(side, ~side)]
            nearest = others.min(1) if others.shape[1] else np.full(int(side.sum()), cap2)       # a minimum over no pixel is cap2
            out[side] = sign * np.minimum(nearest, cap2)
    return out.reshape(h, w).astype(np.int32)


def grow_brute(m, r):
    h, w = m.shape
    r2 = int(np.floor(float(r) * float(r)))
    d2 = _pair_d2(h, w)
    flat = m.reshape(-1).astype(np.int64)
    out = flat.copy()
    for p in range(h * w):
        if r < 0:
            if flat[p] and (d2[p][flat != flat[p]] <= r2).any():
                out[p] = 0
        elif flat[p] == 0:
            q = (flat != 0) & (d2[p] <= r2)
            if q.any():
                out[p] = min(zip(d2[p][q].tolist(), flat[q].tolist()))[1]            # the lexicographic minimum of (distance, label)
    return out.reshape(h, w).astype(np.uint8)


def blob(h, w, rng, labels=(1, 2, 3), p=0.5):
    """smooth random regions of the labels (and 0): thresholded sums of a few random plane waves"""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    m = np.zeros((h, w), np.uint8)
    for lab in labels:
        f = sum(np.cos(rng.uniform(0.05, 0.6) * yy + rng.uniform(0.05, 0.6) * xx * rng.choice([-1, 1]) + rng.uniform(0, 6.3)) for _ in range(3))
        m[f > np.quantile(f, 1 - p / len(labels))] = lab
    return m


def contents(h, w, seed=0):
    """{name: uint8 [h, w]}: the contents the device kernels are held to at every size"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[:h, :w]
    out = {}
    touching = np.zeros((h, w), np.uint8)                                # one blob that touches all four borders ...
    touching[(np.abs(yy - (h - 1) / 2) <= max(h // 5, 0.5)) | (np.abs(xx - (w - 1) / 2) <= max(w // 5, 0.5))] = 1
    out['touching'] = touching
    out['whole'] = np.full((h, w), 2, np.uint8)
    out['empty'] = np.zeros((h, w), np.uint8)
    single = np.zeros((h, w), np.uint8)
    single[h // 3, w // 2] = 1
    out['single'] = single
    out['checker'] = (((yy + xx) & 1) * (1 + (yy & 1))).astype(np.uint8)          # labels 1 and 2 on the odd squares
    tie = np.zeros((h, w), np.uint8)                                     # ... two labels at equal distances from the pixels between them
    tie[:, : max(w // 4, 1)] = 3
    tie[:, w - max(w // 4, 1):] = 1
    tie[: max(h // 6, 1), :] = np.where(tie[: max(h // 6, 1), :] == 0, 2, tie[: max(h // 6, 1), :])
    tie[h - max(h // 6, 1):, :] = np.where(tie[h - max(h // 6, 1):, :] == 0, 1, tie[h - max(h // 6, 1):, :])
    out['tie'] = tie
    lattice = np.zeros((h, w), np.uint8)                                 # single pixels of three labels on a lattice of pitch 4:
    on = (yy % 4 == 0) & (xx % 4 == 0)                                   # every pixel between them has rivals at one distance
    lattice[on] = ((yy // 4 + xx // 4) % 3 + 1)[on]
    out['lattice'] = lattice
    out['blobs'] = blob(h, w, rng)
    return out
