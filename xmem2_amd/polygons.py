"""Polygon outlines of index masks: the definition, on the host, in numpy.

This module is what `ops.mask_polygons` (csrc/polygons.hip, include/xmem_hip_polygons.h) is tested against word for word, and the
reader of what it writes; the product path traces on the device and never calls `rings_host`.

Lattice.  Vertices are the integer points (x, y), 0 <= x <= W, 0 <= y <= H; pixel (row y, column x) is the unit square with the
corners (x, y) and (x + 1, y + 1).  For label k the region is R = {mask == k}; outside the image is not R.  The boundary is the set
of directed unit edges with R on the right-hand side of travel (x to the right, y down): for a pixel of R its top (x, y) -> (x+1, y)
when the pixel above is not R, its right side (x+1, y) -> (x+1, y+1), its bottom (x+1, y+1) -> (x, y+1) and its left side
(x, y+1) -> (x, y) likewise.  Directions: 0 +x, 1 +y, 2 -x, 3 -y.

Successor.  A vertex has as many incoming as outgoing edges: 0, 1 or 2.  With two (a saddle: exactly two diagonal pixels of its
2 x 2 neighbourhood are in R) an edge that arrives with direction d leaves with (d + 3) mod 4, which joins the two pixels: R is
8-connected and its complement 4-connected, the pair `mask_cleanup` uses.

Rings.  The edges fall into closed rings.  A corner is a vertex visit where the direction changes (every saddle visit is one).  A
ring is the list of its corners (x, y) in travelling order from its corner with the smallest (y, x); the rings of a label are
ordered by that corner.  The doubled shoelace sum `area2` is positive for outer rings and negative for holes; the number of outer
rings is the label's number of 8-connected components.  Filling all rings of a label even-odd (`fill_host`) gives R back.

record_host(mask, K) -> (meta int32 [K, 2] = corners, rings per label 1..K; uint32 words, the labels' corner lists back to back,
one word x | y << 16 | first corner of its ring << 31): what the device writes for one frame.
"""
import numpy as np

META = 2                     # int32 per (frame, label): corners, rings
FIRST = np.uint32(1 << 31)   # the flag of a ring's first corner in a corner word
_STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))


def _mask2d(mask):
    mask = np.asarray(mask)
    if mask.ndim != 2 or mask.dtype != np.uint8 or mask.size == 0:
        raise ValueError(f'mask: expected a non-empty uint8 [H,W] array, got {mask.dtype} {mask.shape}')
    return mask


def default_capacity(H, W):
    """corners per frame a record has room for unless the caller says otherwise: the run-length export's default"""
    return max(2048, 4 * int(W))


def rings_host(mask, k):
    """The rings of label `k` of the uint8 map `mask` [H,W]: a list of rings, each a list of corners (x, y)."""
    mask = _mask2d(mask)
    h, w = mask.shape
    r = np.zeros((h + 2, w + 2), bool)
    r[1:-1, 1:-1] = mask == k
    # out[d][vy, vx]: an edge leaves the vertex (vx, vy) with direction d.  r[vy + 1, vx + 1] is the pixel (vy, vx) south-east of it.
    se, sw, ne, nw = r[1:, 1:], r[1:, :-1], r[:-1, 1:], r[:-1, :-1]
    out = (se & ~ne) * 1 + (sw & ~se) * 2 + (nw & ~sw) * 4 + (ne & ~nw) * 8
    ys, xs = np.nonzero(out)
    left = {(int(x), int(y)): int(b) for x, y, b in zip(xs, ys, out[ys, xs])}         # directions not yet travelled, per vertex
    rings = []
    for start in zip(xs.tolist(), ys.tolist()):
        # ascending (y, x): every edge at a smaller vertex is travelled, so an edge still open here belongs to a ring whose
        # smallest vertex this is - a vertex with one outgoing edge, visited once
        bits = left[start]
        if not bits:
            continue
        if bits & (bits - 1):
            raise AssertionError('a ring starts at a saddle')
        ring, (x, y), d = [start], start, bits.bit_length() - 1
        while True:
            if not left[(x, y)] >> d & 1:
                raise AssertionError('the boundary is not a union of rings')
            left[(x, y)] &= ~(1 << d)
            x, y = x + _STEP[d][0], y + _STEP[d][1]
            if (x, y) == start:
                break
            bits = int(out[y, x])
            nd = (d + 3) % 4 if _saddle(bits) else bits.bit_length() - 1
            if nd != d:
                ring.append((x, y))
            d = nd
        rings.append(ring)
    return rings          # in the order of their starts already


def _saddle(bits):
    return bits in (5, 10)       # two outgoing edges, opposite to each other: directions 0 and 2, or 1 and 3


def area2(ring):
    """the doubled shoelace sum of a ring: positive for an outer ring, negative for a hole"""
    p = np.asarray(ring, np.int64).reshape(-1, 2)
    q = np.roll(p, -1, axis=0)
    return int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())


def pack_rings(rings):
    """corner words of a label's rings, in order"""
    words = []
    for ring in rings:
        p = np.asarray(ring, np.int64).reshape(-1, 2)
        w = (p[:, 0] | (p[:, 1] << 16)).astype(np.uint32)
        w[0] |= FIRST
        words.append(w)
    return np.concatenate(words) if words else np.zeros(0, np.uint32)


def unpack_rings(words):
    """the inverse of `pack_rings`: a list of rings, each a list of (x, y)"""
    words = np.asarray(words, np.uint32).reshape(-1)
    if words.size and not words[0] & FIRST:
        raise ValueError('corner words: the first word does not begin a ring')
    starts = np.nonzero(words & FIRST)[0].tolist() + [len(words)]
    xs, ys = (words & 0xffff).astype(np.int64), ((words >> 16) & 0x7fff).astype(np.int64)
    return [list(zip(xs[a:b].tolist(), ys[a:b].tolist())) for a, b in zip(starts[:-1], starts[1:])]


def record_host(mask, K):
    """(meta int32 [K,2], corner words uint32) of one frame, as the device writes them"""
    mask = _mask2d(mask)
    meta = np.zeros((K, META), np.int32)
    words = []
    for k in range(1, K + 1):
        rings = rings_host(mask, k) if (mask == k).any() else []
        meta[k - 1] = (sum(len(r) for r in rings), len(rings))
        words.append(pack_rings(rings))
    return meta, np.concatenate(words) if words else np.zeros(0, np.uint32)


def split_record(rec, B, K, capacity):
    """views (meta int32 [B,K,2], corners uint32 [B,capacity]) of the flat int32 record of `ops.mask_polygons(wait=False)`"""
    rec = np.asarray(rec)
    if rec.dtype != np.int32 or rec.ndim != 1 or rec.size != B * K * META + B * capacity:
        raise ValueError(f'record: expected {B * K * META + B * capacity} int32 words, got {rec.dtype} {rec.shape}')
    return rec[:B * K * META].reshape(B, K, META), rec[B * K * META:].view(np.uint32).reshape(B, capacity)


def label_rings(meta, words):
    """per label 1..K the list of rings, from one frame's meta [K,2] and its packed corner words"""
    out, at = [], 0
    for corners, rings in np.asarray(meta).reshape(-1, META).tolist():
        got = unpack_rings(words[at:at + corners])
        if len(got) != rings:
            raise ValueError(f'corner words: {len(got)} rings where meta says {rings}')
        out.append(got)
        at += corners
    return out


def label_flat(meta, words, tolerance=0):
    """per label 1..K the rings as flat integer lists [x0, y0, x1, y1, ..] - what the `polygons` key of tracks.json holds -, each
    ring reduced by `simplify(., tolerance)`; exact rings go from the words to the lists without a Python step per corner"""
    if tolerance:
        return [[flat(simplify(r, tolerance)) for r in rings] for rings in label_rings(meta, words)]
    words = np.asarray(words, np.uint32).reshape(-1)
    xy = np.empty(2 * len(words), np.int64)
    xy[0::2], xy[1::2] = words & 0xffff, (words >> 16) & 0x7fff
    first = np.nonzero(words & FIRST)[0]
    out, at = [], 0
    for corners, rings in np.asarray(meta).reshape(-1, META).tolist():
        a, b = np.searchsorted(first, (at, at + corners))
        if b - a != rings or (corners and (a == len(first) or first[a] != at)):
            raise ValueError(f'corner words: {b - a} rings where meta says {rings}')
        cuts = first[a:b].tolist() + [at + corners]
        out.append([xy[2 * s:2 * e].tolist() for s, e in zip(cuts[:-1], cuts[1:])])
        at += corners
    return out


def fill_host(rings, H, W):
    """Even-odd fill of rings (lists of (x, y), or flat [x0, y0, x1, y1, ..] lists) -> bool [H,W]: a pixel is set when its centre
    lies inside an odd number of rings.  Exact rings give the label's region back; this is the reader of the `polygons` key."""
    cross = np.zeros((H, W + 1), np.int64)
    for ring in rings:
        p = np.asarray(ring, np.float64).reshape(-1, 2)
        q = np.roll(p, -1, axis=0)
        for (xa, ya), (xb, yb) in zip(p.tolist(), q.tolist()):
            if ya == yb:
                continue
            lo, hi = (ya, yb) if ya < yb else (yb, ya)
            rows = np.arange(max(0, int(np.ceil(lo - 0.5))), min(H, int(np.floor(hi - 0.5)) + 1))         # lo < row + 0.5 < hi
            rows = rows[(rows + 0.5 > lo) & (rows + 0.5 < hi)]
            if rows.size == 0:
                continue
            xi = xa + (rows + 0.5 - ya) * (xb - xa) / (yb - ya)
            cols = np.clip(np.ceil(xi - 0.5).astype(np.int64), 0, W)                 # the first pixel whose centre is right of it
            np.add.at(cross, (rows, cols), 1)
    return (np.cumsum(cross, axis=1)[:, :W] & 1).astype(bool)


# ---- the exact fill: fixed point, integer arithmetic (csrc/polygons_fill.hip is held to it bit for bit) ---------------------------
#
# Vertices are moved to the grid of 1 / 2**frac_bits pixel first (`quantise`); everything after that is integer.  one = 2**frac_bits.
# An edge, normalised to ya < yb (horizontal edges take no part), crosses image row r when 2 ya <= (2 r + 1) one < 2 yb - half open,
# so a vertex that lies exactly on a centre line counts once - and toggles the first column whose centre is at or right of it:
# c = ceil(num / den), num = 2 xa dy + ((2 r + 1) one - 2 ya) dx - one dy, den = 2 one dy, clipped to [0, W].  A pixel is inside when
# the running parity of the toggles along its row is odd.  With |v| one <= 2^28 every product stays below 2^62.
MAX_FRAC_BITS = 8
COORD_BOUND = 1 << 28        # of a quantised coordinate's magnitude


def _frac_bits(frac_bits):
    if isinstance(frac_bits, (bool, np.bool_)) or not isinstance(frac_bits, (int, np.integer)) or not 0 <= frac_bits <= MAX_FRAC_BITS:
        raise ValueError(f'frac_bits = {frac_bits!r} must be an integer in 0..{MAX_FRAC_BITS}')
    return int(frac_bits)


def quantise(v, frac_bits=8):
    """np.rint(v * 2**frac_bits) as int64.  Refuses non-finite values and |v| * 2**frac_bits > 2^28."""
    one = 1 << _frac_bits(frac_bits)
    v = np.asarray(v, np.float64)
    if not np.isfinite(v).all():
        raise ValueError('quantise: a coordinate is not finite')
    if v.size and np.abs(v).max() * one > COORD_BOUND:
        raise ValueError(f'quantise: a coordinate exceeds 2^28 / 2^{frac_bits} pixels')
    return np.rint(v * one).astype(np.int64)


def _ring_edges(ring, frac_bits):
    """int64 [n, 4] = xa, ya, xb, yb with ya < yb of a ring's edges (its last vertex joins its first), horizontal ones dropped"""
    p = quantise(np.asarray(ring, np.float64).reshape(-1, 2), frac_bits)
    q = np.roll(p, -1, axis=0)
    up = p[:, 1] > q[:, 1]
    e = np.where(up[:, None], np.concatenate([q, p], 1), np.concatenate([p, q], 1))
    return e[e[:, 1] != e[:, 3]]


def _ceil_div(a, b):
    return -((-a) // b)


def fill_exact_host(rings, H, W, frac_bits=8):
    """Even-odd fill of rings (lists of (x, y) or flat lists, ints or floats) -> bool [H,W] by the integer rule above.  Rings with
    fewer than 3 vertices, repeated vertices, self-intersections and vertices outside the plane are all taken as they come."""
    one = 1 << _frac_bits(frac_bits)
    H, W = int(H), int(W)
    parts = [_ring_edges(r, frac_bits) for r in rings if len(r)]
    e = np.concatenate(parts) if parts else np.zeros((0, 4), np.int64)
    xa, ya, xb, yb = e.T
    r0 = np.clip(_ceil_div(2 * ya - one, 2 * one), 0, H)             # the rows are clipped here, none outside the plane is walked
    r1 = np.clip(_ceil_div(2 * yb - one, 2 * one), 0, H)
    n = np.maximum(r1 - r0, 0)
    at = np.repeat(np.arange(len(e)), n)                             # one entry per crossing
    r = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + r0[at]
    dx, dy = (xb - xa)[at], (yb - ya)[at]
    num = 2 * xa[at] * dy + ((2 * r + 1) * one - 2 * ya[at]) * dx - one * dy
    c = np.clip(_ceil_div(num, 2 * one * dy), 0, W)
    cross = np.bincount(r * (W + 1) + c, minlength=H * (W + 1)).reshape(H, W + 1)
    return (np.cumsum(cross, axis=1)[:, :W] & 1).astype(bool)


def fill_rows_host(rows, H, W, values=None, frac_bits=8, base=None):
    """uint8 [H,W] from a list of ring lists: row i is filled even-odd on its own, a pixel takes values[i] (default i + 1) of the
    highest row that contains it, else `base`'s value, or 0 - `rle.decode`'s overlap rule.  A union of polygons (COCO, labelme:
    several polygons for one object) is one row per polygon with equal values."""
    values = list(range(1, len(rows) + 1)) if values is None else [int(v) for v in values]
    if len(values) != len(rows) or any(not 0 <= v <= 255 for v in values):
        raise ValueError(f'fill_rows_host: values must be {len(rows)} integers in 0..255')
    out = np.zeros((H, W), np.uint8) if base is None else np.array(base, np.uint8).reshape(H, W)
    for rings, v in zip(rows, values):
        out[fill_exact_host(rings, H, W, frac_bits)] = v
    return out


def pack_edges(frames, R, frac_bits=8):
    """(edges int32 [E, 4] = xa, ya, xb, yb with ya < yb, plane int32 [E] = frame * R + row) of `frames`: a list of frames, each a
    list of at most R rows, each a list of rings - what `ops.fill_polygons` uploads.  Work per vertex, vectorised per ring."""
    edges, plane = [], []
    for f, rows in enumerate(frames):
        if len(rows) > R:
            raise ValueError(f'pack_edges: frame {f} has {len(rows)} rows, R = {R}')
        for i, rings in enumerate(rows):
            for ring in rings:
                if len(ring):
                    e = _ring_edges(ring, frac_bits)
                    edges.append(e)
                    plane.append(np.full(len(e), f * R + i, np.int32))
    if not edges:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int32)
    return np.concatenate(edges).astype(np.int32), np.concatenate(plane)


def _segment_distance(p, a, b):
    p, a, b = (np.asarray(v, np.float64) for v in (p, a, b))
    ab = b - a
    den = float(ab @ ab)
    t = 0.0 if den == 0 else min(1.0, max(0.0, float((p - a) @ ab) / den))
    return float(np.hypot(*(p - (a + t * ab))))


def _rdp(points, first, last, tolerance, keep):
    """Ramer-Douglas-Peucker on points[first..last]: marks what stays between two kept ends"""
    stack = [(first, last)]
    while stack:
        a, b = stack.pop()
        worst, at = -1.0, -1
        for i in range(a + 1, b):
            dist = _segment_distance(points[i], points[a], points[b])
            if dist > worst:
                worst, at = dist, i
        if at >= 0 and worst > tolerance:
            keep[at] = True
            stack += [(a, at), (at, b)]


def simplify(ring, tolerance):
    """Ramer-Douglas-Peucker over a ring's corners.  The ring is cut at its start corner and at the corner farthest from it (the
    first of equals) and each half is reduced; kept vertices are original corners in the original order, beginning with the start
    corner, and every dropped corner lies within `tolerance` of the segment that replaced it.  A ring that would keep fewer than 3
    vertices stays as it was.  tolerance None or 0: the ring itself.  Simplified rings are lossy."""
    ring = [tuple(p) for p in ring]
    if tolerance is None or tolerance == 0:
        return ring
    if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)) or not tolerance > 0:
        raise ValueError(f'simplify: tolerance = {tolerance!r} must be None or a number >= 0')
    n = len(ring)
    if n < 4:
        return ring
    pts = np.asarray(ring, np.float64)
    far = int(np.argmax(((pts - pts[0]) ** 2).sum(axis=1)))
    closed = ring + [ring[0]]
    keep = [False] * (n + 1)
    keep[0] = keep[far] = keep[n] = True
    _rdp(closed, 0, far, float(tolerance), keep)
    _rdp(closed, far, n, float(tolerance), keep)
    out = [ring[i] for i in range(n) if keep[i]]
    return out if len(out) >= 3 else ring


def to_coco(rings):
    """The outer rings (positive `area2`) as COCO `segmentation` polygons: flat float lists [x0, y0, x1, y1, ..].  COCO takes the
    UNION of the polygons of an object, so holes are lost there; `fill_host` over all rings is the exact reader."""
    return [[float(v) for p in ring for v in p] for ring in rings if area2(ring) > 0]


def flat(ring):
    """a ring as the flat integer list [x0, y0, x1, y1, ..] of the `polygons` key of tracks.json"""
    return [int(v) for p in ring for v in p]


def parse_polygons(spec):
    """config['tracks_polygons'] -> None (off) or {'tolerance': t}, t = 0 for exact rings.  Accepts None, False, True or a dict with
    the one key 'tolerance' (None or a finite number >= 0); anything else raises ValueError."""
    if spec is None or spec is False:
        return None
    if spec is True:
        return {'tolerance': 0}
    if not isinstance(spec, dict):
        raise ValueError(f'tracks_polygons: expected None, True or {{"tolerance": t}}, got {spec!r}')
    unknown = sorted(set(spec) - {'tolerance'}, key=str)
    if unknown:
        raise ValueError(f'tracks_polygons: unknown keys {unknown} (known: tolerance)')
    t = spec.get('tolerance', 0)
    if t is None:
        t = 0
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, float, np.integer, np.floating)) or not (0 <= t < float('inf')):
        raise ValueError(f'tracks_polygons: tolerance = {t!r} must be None or a finite number >= 0')
    t = float(t)
    return {'tolerance': int(t) if t == int(t) else t}


def from_labelme(paths_or_dir, file_names=None):
    """labelme's per-frame JSON files -> a polygon-only tracks document (xmem2_amd/rle.py reads it: `TrackReader`).  Each file holds
    `imageHeight`, `imageWidth` and `shapes`: [{label, points [[x, y], ..], shape_type, group_id}], and is named like its frame.
    `paths_or_dir`: a directory (its *.json, sorted) or a list of files; `file_names`: the video's frames - a frame without a file
    gets null entries - default: the annotated frames themselves.  A label that parses as an integer in 1..255 keeps its value; the
    other names get, in sorted order, the smallest values no numeric label took (1..n when there is none) and are recorded in the
    video entry as `label_names`.  One track per label, ordered by value; the polygons of a label in a frame are the entry's rings,
    filled each on its own (`"fill": "union"`).  A shape that is no polygon raises ValueError."""
    import json
    import os
    if isinstance(paths_or_dir, (str, os.PathLike)):
        folder = str(paths_or_dir)
        paths = [os.path.join(folder, n) for n in sorted(os.listdir(folder)) if n.endswith('.json')]
    else:
        paths = [str(p) for p in paths_or_dir]
    if not paths:
        raise ValueError('from_labelme: no annotation files')
    stem = lambda p: os.path.splitext(os.path.basename(p))[0]
    frames, size = {}, None
    for path in paths:
        with open(path) as f:
            doc = json.load(f)
        hw = (int(doc['imageHeight']), int(doc['imageWidth']))
        if size is not None and hw != size:
            raise ValueError(f'from_labelme: {path} is {hw}, the files before it {size}')
        size = hw
        shapes = []
        for i, shape in enumerate(doc['shapes']):
            kind = shape.get('shape_type', 'polygon')
            if kind != 'polygon':
                raise ValueError(f'from_labelme: {path}, shape {i} ({shape.get("label")!r}) is a {kind!r}, only polygons are read')
            pts = np.asarray(shape['points'], np.float64)
            if pts.ndim != 2 or pts.shape[1] != 2 or not np.isfinite(pts).all():
                raise ValueError(f'from_labelme: {path}, shape {i} ({shape.get("label")!r}): points must be finite [x, y] pairs')
            shapes.append((str(shape['label']), pts.reshape(-1).tolist()))
        if stem(path) in frames:
            raise ValueError(f'from_labelme: two files are named {stem(path)!r}')
        frames[stem(path)] = shapes
    if file_names is None:
        file_names = [stem(p) for p in paths]
    file_names = [str(n) for n in file_names]
    stems = [os.path.splitext(n)[0] for n in file_names]
    stray = sorted(set(frames) - set(stems))
    if stray:
        raise ValueError(f'from_labelme: no frame is named like {stray}')

    def numeric(label):
        try:
            return int(label) if 1 <= int(label) <= 255 and str(int(label)) == label.strip() else None
        except ValueError:
            return None
    labels = sorted({label for shapes in frames.values() for label, _ in shapes})
    value = {label: numeric(label) for label in labels if numeric(label) is not None}
    free = (v for v in range(1, 256) if v not in set(value.values()))
    names = {}
    for label in labels:
        if label not in value:
            value[label] = next(free, None)
            if value[label] is None:
                raise ValueError('from_labelme: more labels than the 255 values of an index mask')
            names[str(value[label])] = label
    anns = []
    for n, label in enumerate(sorted(value, key=value.get), start=1):
        seg = []
        for s in stems:
            rings = [pts for lab, pts in frames.get(s, []) if lab == label]
            seg.append({'size': list(size), 'polygons': rings} if rings else None)
        anns.append({'id': n, 'video_id': 1, 'category_id': 1, 'label': value[label], 'segmentations': seg,
                     'bboxes': [None] * len(stems), 'areas': [None] * len(stems)})
    video = {'id': 1, 'height': size[0], 'width': size[1], 'length': len(stems), 'file_names': file_names, 'polygons': {'fill': 'union'}}
    if names:
        video['label_names'] = names
    return {'videos': [video], 'categories': [{'id': 1, 'name': 'object'}], 'annotations': anns}
