#!/usr/bin/env python
"""Pins DAVIS J&F (xmem2_amd/metrics.py, the `xmem_jf_counts` kernel) against the REFERENCE's own util/metrics.py.

    python tests/golden/make_jf_goldens.py          # writes tests/golden/jf.npz  (needs /root/reference)

util/metrics.py cannot be imported as it stands in the build container: it imports cv2 and skimage, neither installed, and it uses
np.int / np.float / np.bool, which numpy 2 removed.  This script installs three shims before the import:

  * np.int / np.float / np.bool = int / float / bool (what those aliases always were);
  * `cv2.dilate(src, kernel)` = scipy.ndimage.binary_dilation(src, structure=kernel, border_value=0) - OpenCV's dilation with its
    default constant border, which never wins a maximum (the kernels here are symmetric disks, so the anchor convention is moot);
  * `skimage.morphology.disk(r)` = the (2r+1)^2 grid with X^2 + Y^2 <= r^2, skimage's own definition.

Everything else - _seg2bmap, f_measure's radius, the precision / recall cases, the J / F arithmetic, the object-id logic and the
averaging - is the reference's code.  Per case the file holds the inputs (uint8 [B,H,W]), bound_th, nb_objects (-1: None), the
reference's J and F with average_over_objects=False and =True, and the integer counts [B,256,7] of xmem_jf_counts built from the
reference's own _seg2bmap and the shimmed dilation (gt_area, pred_area, inter, n_gt, n_pred, gt_match, pred_match).
Deterministic: rerunning it reproduces jf.npz array for array."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.dont_write_bytecode = True


def _install_shims():
    import scipy.ndimage as ndi
    for name, typ in (('int', int), ('float', float), ('bool', bool)):
        setattr(np, name, typ)
    cv2 = types.ModuleType('cv2')
    cv2.dilate = lambda src, kernel: ndi.binary_dilation(src, structure=kernel, border_value=0).astype(src.dtype)
    sys.modules['cv2'] = cv2
    skimage = types.ModuleType('skimage')
    morphology = types.ModuleType('skimage.morphology')

    def disk(radius, dtype=np.uint8):
        L = np.arange(-radius, radius + 1)
        X, Y = np.meshgrid(L, L)
        return np.array((X ** 2 + Y ** 2) <= radius ** 2, dtype=dtype)
    morphology.disk = disk
    skimage.morphology = morphology
    sys.modules['skimage'] = skimage
    sys.modules['skimage.morphology'] = morphology


def _reference():
    _install_shims()
    import importlib.util
    spec = importlib.util.spec_from_file_location('ref_metrics', os.path.join(REF, 'util', 'metrics.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_counts(ref, gt, pred, bound_th):
    """[B,256,7] int32 from the reference's _seg2bmap and f_measure's dilation, for every label 1..254 present in either map."""
    import cv2
    from skimage.morphology import disk
    B, H, W = gt.shape
    r = bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((H, W)))
    se = disk(r).astype(np.uint8)
    out = np.zeros((B, 256, 7), np.int32)
    for b in range(B):
        for k in np.union1d(np.unique(gt[b]), np.unique(pred[b])):
            if k == 0 or k == 255:
                continue
            mg, mp = gt[b] == k, pred[b] == k
            bg, bp = ref._seg2bmap(mg), ref._seg2bmap(mp)
            dg, dp = cv2.dilate(bg.astype(np.uint8), se), cv2.dilate(bp.astype(np.uint8), se)
            out[b, k] = [mg.sum(), mp.sum(), (mg & mp).sum(), bg.sum(), bp.sum(), (bg * dp).sum(), (bp * dg).sum()]
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _blobs(rng, shape, ids, n_per=1, rmin=0.08, rmax=0.3):
    H, W = shape
    yy, xx = np.mgrid[:H, :W]
    lab = np.zeros(shape, np.uint8)
    for k in ids:
        for _ in range(n_per):
            cy, cx = rng.uniform(0, H), rng.uniform(0, W)
            ry, rx = rng.uniform(rmin, rmax) * H + 0.5, rng.uniform(rmin, rmax) * W + 0.5
            lab[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = k
    return lab


def _perturb(rng, lab, shift=3, flip_frac=0.01):
    out = np.roll(lab, (int(rng.integers(-shift, shift + 1)), int(rng.integers(-shift, shift + 1))), axis=(0, 1))
    noise = rng.random(lab.shape) < flip_frac
    out = out.copy()
    out[noise] = lab[noise]
    return out


def _video(rng, T, shape, ids):
    gt = np.stack([_blobs(rng, shape, ids) for _ in range(T)])
    pred = np.stack([_perturb(rng, g) for g in gt])
    return gt, pred


def _erode(mask, it):
    import scipy.ndimage as ndi
    out = np.zeros_like(mask)
    for k in np.unique(mask):
        if k != 0:
            out[ndi.binary_erosion(mask == k, iterations=it)] = k
    return out


def cases():
    from PIL import Image
    rng = np.random.default_rng(20261016)
    c = {}
    c['multi'] = _video(rng, 4, (97, 131), [1, 3, 7]) + (0.008, None)
    gt, pred = c['multi'][:2]
    c['multi_nb8'] = (gt, pred, 0.008, 8)
    # object 2 appears at frame 3; object 1 vanishes after frame 2 (in the prediction one frame late)
    T, shape = 6, (64, 80)
    gt = np.zeros((T,) + shape, np.uint8); pred = np.zeros_like(gt)
    for t in range(T):
        a, b = _blobs(rng, shape, [1]), _blobs(rng, shape, [2])
        if t <= 2:
            gt[t][a == 1] = 1
        if t <= 3:
            pred[t][_perturb(rng, a) == 1] = 1
        if t >= 3:
            gt[t][b == 2] = 2
            pred[t][_perturb(rng, b) == 2] = 2
    c['late_vanish'] = (gt, pred, 0.008, None)
    gt, _ = _video(rng, 3, (50, 70), [1, 2])
    c['empty_pred'] = (gt, np.zeros_like(gt), 0.008, None)
    gt, pred = _video(rng, 3, (72, 96), [1, 2])
    pred = pred.copy()
    pred[:, 5:20, 10:30] = 5                                        # an object absent from the ground truth
    gt, pred = gt.copy(), pred.copy()
    gt[:, 30:34, :] = 255; gt[:, :, 60:63] = 255                     # void bands
    pred[:, 40:42, :] = 255
    c['absent_void'] = (gt, pred, 0.008, None)
    c['odd'] = _video(rng, 3, (67, 129), [1, 2, 4]) + (0.008, None)
    c['row_1xW'] = _video(rng, 2, (1, 50), [1, 2]) + (0.008, None)
    c['col_Hx1'] = _video(rng, 2, (40, 1), [1]) + (0.008, None)
    c['tiny_2x2'] = (np.array([[[1, 0], [1, 1]], [[0, 0], [0, 2]]], np.uint8), np.array([[[1, 1], [0, 1]], [[0, 0], [2, 2]]], np.uint8),
                     0.008, None)
    c['p480'] = _video(rng, 1, (480, 854), [1, 2, 3]) + (0.008, None)      # radius 8
    c['p1080'] = _video(rng, 1, (1080, 1920), [1, 2]) + (0.008, None)      # radius 18
    gt, pred = _video(rng, 3, (60, 90), [1, 2])
    c['bound3'] = (gt, pred, 3, None)
    c['bound1'] = (gt, pred, 1, None)
    ann = os.path.join(HERE, 'chair', 'Annotations')
    chair = np.stack([np.array(Image.open(os.path.join(ann, f)).convert('P'), np.uint8) for f in sorted(os.listdir(ann))])
    c['chair_shift'] = (chair, np.roll(chair, (4, -6), axis=(1, 2)), 0.008, None)
    c['chair_erode'] = (chair, _erode(chair, 3), 0.008, None)
    return c


def main():
    ref = _reference()
    out = {}
    for name, (gt, pred, bound_th, nb) in cases().items():
        gt, pred = np.ascontiguousarray(gt, np.uint8), np.ascontiguousarray(pred, np.uint8)
        out[f'{name}/gt'], out[f'{name}/pred'] = gt, pred
        out[f'{name}/bound_th'] = np.float64(bound_th)
        out[f'{name}/nb_objects'] = np.int64(-1 if nb is None else nb)
        for avg in (False, True):
            tag = 'avg' if avg else 'obj'
            out[f'{name}/J_{tag}'] = np.asarray(ref.batched_jaccard(gt, pred, average_over_objects=avg, nb_objects=nb), np.float64)
            out[f'{name}/F_{tag}'] = np.asarray(ref.batched_f_measure(gt, pred, average_over_objects=avg, nb_objects=nb,
                                                                     bound_th=bound_th), np.float64)
        out[f'{name}/counts'] = reference_counts(ref, gt, pred, bound_th)
        print(f'{name:12s} {gt.shape}  J {out[f"{name}/J_avg"].mean():.4f}  F {out[f"{name}/F_avg"].mean():.4f}')
    path = os.path.join(HERE, 'jf.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
