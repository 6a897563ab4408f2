"""Oracle and inputs of the mask clean-up tests (test_mask_cleanup_host.py, test_gpu_components.py, test_gpu_mask_cleanup_stream.py).

The oracle is scipy.ndimage.label, written from the definition in the issue and not from xmem2_amd/mask_cleanup.py: structure
ones((3,3)) for 8-connectivity, generate_binary_structure(2, 1) for 4-connectivity, ndimage.minimum of the linear index for `root`
and ndimage.sum for `area`.  ndimage.label knows foreground and background only, so a map of several values is labelled value by value.
"""
import numpy as np
from scipy import ndimage

STRUCTURE = {8: np.ones((3, 3), int), 4: ndimage.generate_binary_structure(2, 1)}


def components_ref(mask, connectivity):
    """(root, area) int32 [H,W]: per pixel the smallest row-major index and the size of its component of equal values"""
    h, w = mask.shape
    index = np.arange(h * w).reshape(h, w)
    root = np.full((h, w), -1, np.int64)
    area = np.zeros((h, w), np.int64)
    for value in np.unique(mask):
        lab, n = ndimage.label(mask == value, structure=STRUCTURE[connectivity])
        ids = np.arange(1, n + 1)
        first = np.asarray(ndimage.minimum(index, lab, ids)).astype(np.int64)
        size = np.asarray(ndimage.sum(np.ones((h, w)), lab, ids)).astype(np.int64)
        sel = lab > 0
        root[sel] = first[lab[sel] - 1]
        area[sel] = size[lab[sel] - 1]
    assert (root >= 0).all()
    return root.astype(np.int32), area.astype(np.int32)


def clean_ref(mask, min_area=0, max_hole=0, keep_largest=False):
    """(out, stats): pass A on the 8-connected components of each label, pass B on the 4-connected zero components of A's result"""
    h, w = mask.shape
    index = np.arange(h * w).reshape(h, w)
    out = mask.copy()
    stats = np.zeros(4, np.int32)
    for k in np.unique(mask):
        if k == 0:
            continue
        lab, n = ndimage.label(mask == k, structure=STRUCTURE[8])
        ids = np.arange(1, n + 1)
        size = np.asarray(ndimage.sum(np.ones((h, w)), lab, ids)).astype(np.int64)
        first = np.asarray(ndimage.minimum(index, lab, ids)).astype(np.int64)
        largest = min(range(n), key=lambda i: (-size[i], first[i]))
        for i in range(n):
            if size[i] < min_area or (keep_largest and i != largest):
                out[lab == i + 1] = 0
                stats[0] += 1
                stats[1] += size[i]
    if max_hole > 0:
        src = out.copy()
        lab, n = ndimage.label(src == 0, structure=STRUCTURE[4])
        for i, sl in enumerate(ndimage.find_objects(lab)):
            if sl[0].start == 0 or sl[1].start == 0 or sl[0].stop == h or sl[1].stop == w:
                continue                                             # touches a border pixel
            # the component with one pixel of margin: its 4-neighbours outside it are the dilation minus itself
            win = (slice(sl[0].start - 1, sl[0].stop + 1), slice(sl[1].start - 1, sl[1].stop + 1))
            comp = lab[win] == i + 1
            if comp.sum() > max_hole:
                continue
            ring = ndimage.binary_dilation(comp, structure=STRUCTURE[4]) & ~comp
            around = np.unique(src[win][ring])
            if len(around) == 1:
                out[win][comp] = around[0]
                stats[2] += 1
                stats[3] += comp.sum()
    return out, stats


# ---- inputs -------------------------------------------------------------------------------------------------------------------

RANDOM = ((1, .35), (1, .6), (3, .5), (3, .8))                       # (K, p): m = (random < p) * integers(1, K + 1)
TILE = 32                                                            # side of the tile a workgroup resolves in LDS (components.hip)
SHAPES = ((1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (65, 129), (128, 200),
          (TILE - 1, TILE + 1), (TILE + 1, TILE - 1), (TILE, TILE), (2 * TILE + 1, 2 * TILE - 1))
CLEAN_ARGS = ((4, 6, False), (0, 0, True), (4, 6, True))


def random_mask(h, w, K, p, seed=0):
    rng = np.random.default_rng(seed)
    return ((rng.random((h, w)) < p) * rng.integers(1, K + 1, (h, w))).astype(np.uint8)


def serpentine(h=96, w=160):
    """a one-pixel-wide path of label 1 that winds through the whole image: rows 0, 2, 4, ... joined alternately right and left"""
    m = np.zeros((h, w), np.uint8)
    m[0::2, :] = 1
    for i, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = 1
    return m


def rings(h=71, w=93):
    """concentric one-pixel rings, label 1 / 0 / 2 / 0 from the border inwards: nested holes, every zero ring lies between two labels"""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(yy, h - 1 - yy), np.minimum(xx, w - 1 - xx))
    return np.array([1, 0, 2, 0], np.uint8)[d % 4]


def stripes(h=40, w=300):
    return np.broadcast_to(((np.arange(w) % 255) + 1).astype(np.uint8), (h, w)).copy()


def checkerboard(h=37, w=70):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) % 2).astype(np.uint8)


def border_hole(h=40, w=70):
    """label 3 everywhere but a hole that touches the left border (must stay), one inside (filled) and one between 3 and 5 (must stay)"""
    m = np.full((h, w), 3, np.uint8)
    m[10:12, 0:2] = 0
    m[20:22, 35:37] = 0
    m[30:34, 40:50] = 5
    m[31:33, 39] = 0
    m[h - 1, w - 1] = 0
    return m


def equal_blobs(h=50, w=90):
    """two 6 x 6 blobs of label 2 (keep_largest keeps the first), a smaller one, and a larger blob of label 1 astride tile corners"""
    m = np.zeros((h, w), np.uint8)
    m[5:11, 60:66] = 2
    m[30:36, 10:16] = 2
    m[40:43, 70:73] = 2
    m[28:36, 28:36] = 1
    m[2:4, 2:4] = 1
    return m


def blobs_480p(h=480, w=854):
    """smooth blobs of 3 labels with pin-holes and specks: the product size"""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), np.uint8)
    for k, (cy, cx, ry, rx) in enumerate(((150, 200, 90, 140), (300, 600, 120, 160), (380, 250, 60, 200)), start=1):
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 + 0.15 * np.sin(xx / 9.0) * np.cos(yy / 7.0) < 1] = k
    noise = rng.random((h, w))
    m[noise < 0.004] = 0                                             # pin-holes (and nothing where there was background)
    speck = noise > 0.997
    m[speck] = rng.integers(1, 4, (h, w))[speck].astype(np.uint8)
    return m


def patterns():
    """name -> uint8 [H,W]: every pattern of the list but the random ones per shape (random_mask) and the 480p frame (blobs_480p)"""
    return {'zeros': np.zeros((45, 67), np.uint8), 'ones': np.ones((45, 67), np.uint8), 'checkerboard': checkerboard(),
            'serpentine': serpentine(), 'rings': rings(), 'stripes': stripes(), 'border_hole': border_hole(),
            'equal_blobs': equal_blobs()}
