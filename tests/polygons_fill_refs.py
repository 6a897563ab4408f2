"""Inputs shared by test_polygons_fill_host.py and test_gpu_polygons_fill.py: a small clip as a counts file with polygons and as its
polygon-only twin, and random fractional polygons with the awkward cases in them."""
import json

import numpy as np

LABELS = [3, 7, 9]


def clip():
    """5 frames 33 x 65, dense ids 1..3 as ragged blobs (frame 2 has no mask)"""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[:33, :65]
    frames = []
    for t in range(5):
        m = np.zeros((33, 65), np.uint8)
        for k in (1, 2, 3):
            cy, cx, r = rng.integers(4, 29), rng.integers(4, 61), rng.integers(3, 9)
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
        m[rng.random(m.shape) < 0.03] = 0                             # holes and ragged edges
        frames.append(None if t == 2 else m)
    return frames


def counts_doc(polygons=True):
    """the clip through `TrackWriter` (labels 3, 7, 9), the polygon option on"""
    from xmem2_amd import rle
    w = rle.TrackWriter(33, 65, polygons=polygons)
    for t, m in enumerate(clip()):
        w.add_mask(f'{t:05d}.jpg', m, k=3, labels=LABELS)
    return w.to_dict()


def twin(doc):
    """the polygon-only twin: `counts` stripped, boxes and areas null, `size` kept in the first track and dropped in the others"""
    out = json.loads(json.dumps(doc))
    for a, ann in enumerate(out['annotations']):
        for seg in ann['segmentations']:
            if seg is not None:
                del seg['counts']
                if a:
                    del seg['size']
        ann['bboxes'] = [None] * len(ann['bboxes'])
        ann['areas'] = None if a == 1 else [None] * len(ann['areas'])
    return out


def random_rings(rng, H, W, n=3):
    """n random rings of 1..7 vertices around an H x W plane: about 4 in 10 vertices on pixel corners or centres, some outside"""
    rings = []
    for _ in range(n):
        k = int(rng.integers(1, 8))
        pts = np.stack([rng.uniform(-4, W + 4, k), rng.uniform(-4, H + 4, k)], 1)
        snap = rng.random(k) < 0.4
        pts[snap] = np.floor(pts[snap]) + rng.choice([0, 0.5], (int(snap.sum()), 2))
        rings.append(pts.tolist())
    return rings


def awkward_rings(H, W):
    """vertices outside all four sides, a ring wholly outside, rings of 1 and 2 vertices, repeated vertices, a bow-tie"""
    return [[(-3.5, -2.25), (W + 3.0, -1.0), (W + 5.5, H + 2.0), (-2.0, H + 4.75)],
            [(W + 2.0, 1.0), (W + 9.0, 1.0), (W + 9.0, H + 3.0)],
            [(1.5, 1.5)],
            [(0.5, 0.5), (W - 0.5, H - 0.5)],
            [(1.0, 0.0), (1.0, 0.0), (W / 2, H - 1.0), (W / 2, H - 1.0), (0.0, H / 2), (1.0, 0.0)],
            [(0.0, 0.0), (W * 1.0, H * 1.0), (W * 1.0, 0.0), (0.0, H * 1.0)]]
