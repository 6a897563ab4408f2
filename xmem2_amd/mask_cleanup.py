"""Clean-up of index masks: despeckle, fill holes, keep the largest component - the definition, on the host, in numpy.

This module is what `ops.components` / `ops.clean_masks` (csrc/components.hip, include/xmem_hip_masks.h) are tested against bit for
bit; the product path never calls it.  Everything is integer and nothing depends on an order of traversal.

components_host(mask, connectivity) -> (root, area), int32 [H,W].  A component is a maximal 4- or 8-connected set of pixels of EQUAL
value, the value 0 included.  root[p] is the row-major index y * W + x of the component's first pixel, area[p] its size.

clean_host(mask, min_area, max_hole, keep_largest) -> (out, stats), two passes:
  A, objects: the 8-connected components of the labels k >= 1.  A component becomes 0 when `keep_largest` is set and it is not the
     largest of its label (of equal areas the one with the smaller root is the largest), or when its area < min_area.
  B, holes, only with max_hole > 0, on the result of A: a 4-connected component of value 0 is filled with the label k when it touches
     no border pixel of the image, its area <= max_hole, and every 4-neighbour of its pixels outside it carries k.  A hole between
     two labels stays.  (8 for the objects and 4 for the background is the usual dual pair.)
stats, int32 [4]: components removed, pixels removed, holes filled, pixels filled.
"""
import numpy as np

STATS = ('components_removed', 'pixels_removed', 'holes_filled', 'pixels_filled')
KEYS = ('min_area', 'max_hole', 'keep_largest')
_OFFSETS = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, 1), (1, -1))}       # one of each pair of opposite neighbours


def _mask2d(mask):
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.dtype != np.uint8 or mask.size == 0:
        raise ValueError(f'mask: expected a non-empty uint8 [H,W] array, got {mask.dtype} {mask.shape}')
    return mask


def _pairs(h, w, dy, dx):
    """slices (a, b) with b = a shifted by (dy, dx), dy >= 0"""
    ys_a, ys_b = slice(0, h - dy), slice(dy, h)
    xs_a, xs_b = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    return (ys_a, xs_a), (ys_b, xs_b)


def components_host(mask, connectivity=8):
    mask = _mask2d(mask)
    if connectivity not in _OFFSETS:
        raise ValueError(f'connectivity = {connectivity!r} must be 4 or 8')
    h, w = mask.shape
    lab = np.arange(h * w, dtype=np.int64).reshape(h, w)
    edges = []
    for dy, dx in _OFFSETS[connectivity]:
        a, b = _pairs(h, w, dy, dx)
        if mask[a].size:
            edges.append((a, b, mask[a] == mask[b]))
    # lab[p] is always a pixel of p's component with an index <= p, and between rounds a pixel that names itself (a root).  A round
    # takes every pair of equal neighbours whose roots differ and gives the larger root the smallest root it met (a minimum: no
    # order), then replaces labels by the labels of the pixels they name until that changes nothing.  When no pair differs, every
    # component has one root that names itself, which is the component's smallest index.
    flat = lab.reshape(-1)
    while True:
        larger, smaller = [], []
        for a, b, same in edges:
            la, lb = lab[a], lab[b]
            differ = same & (la != lb)
            if differ.any():
                larger.append(np.maximum(la[differ], lb[differ]))
                smaller.append(np.minimum(la[differ], lb[differ]))
        if not larger:
            break
        np.minimum.at(flat, np.concatenate(larger), np.concatenate(smaller))
        while True:
            jumped = flat[lab]
            if (jumped == lab).all():
                break
            lab[...] = jumped
    root = lab.astype(np.int32)
    area = np.bincount(root.reshape(-1), minlength=h * w)[root].astype(np.int32)
    return root, area


def clean_host(mask, min_area=0, max_hole=0, keep_largest=False):
    mask = _mask2d(mask)
    spec = parse_cleanup({'min_area': min_area, 'max_hole': max_hole, 'keep_largest': keep_largest}) or {}
    min_area, max_hole, keep_largest = spec.get('min_area', 0), spec.get('max_hole', 0), spec.get('keep_largest', False)
    h, w = mask.shape
    stats = np.zeros(4, np.int32)
    flat = mask.reshape(-1)
    out = mask.copy()
    root, area = components_host(mask, 8)
    roots = np.unique(root[mask > 0])                                # ascending: of equal areas the first one met wins
    drop = np.zeros(h * w, bool)
    best = {}
    for r in roots:
        k, a = int(flat[r]), int(area.reshape(-1)[r])
        if k not in best or a > best[k][0]:
            best[k] = (a, int(r))
    for r in roots:
        k, a = int(flat[r]), int(area.reshape(-1)[r])
        if a < min_area or (keep_largest and best[k][1] != int(r)):
            drop[r] = True
            stats[0] += 1
            stats[1] += a
    out[drop[root]] = 0
    if max_hole > 0:
        root, area = components_host(out, 4)
        zero = out == 0
        n = h * w
        border = np.zeros((h, w), bool)
        border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
        lo = np.full(n, 256, np.int64)
        hi = np.zeros(n, np.int64)
        np.minimum.at(lo, root[zero & border], 0)
        for dy, dx in ((0, 1), (1, 0)):
            a, b = _pairs(h, w, dy, dx)
            for p, q in ((a, b), (b, a)):                            # p: the hole's pixel, q: its neighbour
                sel = zero[p] & (out[q] > 0)
                np.minimum.at(lo, root[p][sel], out[q][sel])
                np.maximum.at(hi, root[p][sel], out[q][sel])
        rr = root.reshape(-1)
        fill = zero & ((lo == hi) & (hi >= 1))[root] & (area <= max_hole)
        out[fill] = lo[root[fill]].astype(np.uint8)
        stats[2] = int((fill.reshape(-1) & (rr == np.arange(n))).sum())
        stats[3] = int(fill.sum())
    return out, stats


def parse_cleanup(spec):
    """config['mask_cleanup'] -> None (nothing to do) or {'min_area': int, 'max_hole': int, 'keep_largest': bool} with the defaults
    filled in.  Accepts None or a dict with any of those keys; unknown keys, negative or non-integer thresholds, a `keep_largest`
    that is not a bool (or 0 / 1) raise ValueError."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError(f'mask_cleanup: expected None or a dict with any of {KEYS}, got {type(spec).__name__}')
    unknown = sorted(set(spec) - set(KEYS), key=str)
    if unknown:
        raise ValueError(f'mask_cleanup: unknown keys {unknown} (known: {KEYS})')
    out = {}
    for key in ('min_area', 'max_hole'):
        v = spec.get(key, 0)
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'mask_cleanup: {key} = {v!r} must be an integer')
        if not 0 <= int(v) < 2 ** 31:
            raise ValueError(f'mask_cleanup: {key} = {v!r} must be in 0..2^31-1')
        out[key] = int(v)
    v = spec.get('keep_largest', False)
    if not isinstance(v, (bool, np.bool_)) and not (isinstance(v, (int, np.integer)) and int(v) in (0, 1)):
        raise ValueError(f'mask_cleanup: keep_largest = {v!r} must be a bool')
    out['keep_largest'] = bool(v)
    if out['min_area'] <= 1 and out['max_hole'] == 0 and not out['keep_largest']:      # no component has an area below 1
        return None
    return out
