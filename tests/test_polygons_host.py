"""Polygon outlines without a GPU: the host definition (xmem2_amd/polygons.py) on the worked examples and against scipy on random
masks, `simplify`, the third header, its binding and the build lists, the argument checks of the C entry points (which answer before
any GPU work), config['tracks_polygons'] and the track writer with the option off and on."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from conftest import GOLDEN, ROOT
from xmem2_amd import polygons as P

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # xmem_status (include/xmem_hip.h)
CHAIR = os.path.join(GOLDEN, 'chair')


# ---- the ring definition --------------------------------------------------------------------------------------------------------
def test_the_worked_examples():
    block = np.ones((5, 5), np.uint8)
    block[2, 2] = 0
    assert P.rings_host(block, 1) == [[(0, 0), (5, 0), (5, 5), (0, 5)], [(2, 2), (2, 3), (3, 3), (3, 2)]]
    assert [P.area2(r) for r in P.rings_host(block, 1)] == [50, -2]
    for n in (1, 2, 7, 40):
        for diag in (np.eye(n, dtype=np.uint8), np.ascontiguousarray(np.eye(n, dtype=np.uint8)[:, ::-1])):
            (ring,) = P.rings_host(diag, 1)
            assert len(ring) == 4 * n and P.area2(ring) == 2 * n
    yy, xx = np.mgrid[:33, :65]
    rings = P.rings_host(((yy + xx) % 2 == 0).astype(np.uint8), 1)
    assert (len(rings), sum(map(len, rings)), max(map(len, rings))) == (977, 4292, 388)


def test_the_chair_annotations():
    from PIL import Image
    ann = os.path.join(CHAIR, 'Annotations')
    counts = []
    for name in sorted(os.listdir(ann)):
        m = np.array(Image.open(os.path.join(ann, name)).convert('P'), np.uint8)
        assert m.shape == (480, 720)
        rings = P.rings_host(m, 1)
        counts.append((len(rings), sum(map(len, rings))))
        np.testing.assert_array_equal(P.fill_host(rings, 480, 720), m == 1)
    assert len(counts) == 10 and all(4 <= r <= 6 and 342 <= c <= 486 for r, c in counts), counts


def _random_masks():
    rng = np.random.default_rng(2024)
    for i in range(240):
        h, w = (int(v) for v in rng.integers(1, 41, 2))
        yield i, rng.random((h, w)) < (0.2, 0.5, 0.8)[i % 3]


def test_scipy_invariants_and_the_fill_round_trip_on_random_masks():
    checked = 0
    for i, region in _random_masks():
        h, w = region.shape
        rings = P.rings_host(region.astype(np.uint8) * 3, 3)
        np.testing.assert_array_equal(P.fill_host(rings, h, w), region, err_msg=str(i))
        areas = [P.area2(r) for r in rings]
        assert all(areas) and sum(areas) == 2 * int(region.sum())
        assert sum(a > 0 for a in areas) == ndimage.label(region, np.ones((3, 3)))[1]
        assert sum(a < 0 for a in areas) == ndimage.label(~np.pad(region, 1))[1] - 1
        starts = [r[0] for r in rings]
        assert starts == sorted(starts, key=lambda p: (p[1], p[0])) and len(set(starts)) == len(starts)
        for r in rings:
            assert r[0] == min(r, key=lambda p: (p[1], p[0])) and r.count(r[0]) == 1
            q = r[1:] + r[:1]
            assert all((a[0] == b[0]) != (a[1] == b[1]) for a, b in zip(r, q))          # axis-parallel, never of length 0
        checked += 1
    assert checked == 240


def test_record_and_its_readers():
    rng = np.random.default_rng(3)
    m = rng.integers(0, 5, size=(19, 23)).astype(np.uint8)
    meta, words = P.record_host(m, 3)                                 # label 4 is above K
    assert meta.shape == (3, 2) and meta.dtype == np.int32 and words.dtype == np.uint32 and len(words) == meta[:, 0].sum()
    per_label = P.label_rings(meta, words)
    for k in (1, 2, 3):
        assert per_label[k - 1] == P.rings_host(m, k) and meta[k - 1].tolist() == [sum(map(len, per_label[k - 1])), len(per_label[k - 1])]
    assert int((words >> 31).sum()) == meta[:, 1].sum()
    assert P.unpack_rings(P.pack_rings(per_label[0])) == per_label[0]
    assert P.label_flat(meta, words) == [[P.flat(r) for r in rings] for rings in per_label]
    assert P.label_flat(meta, words, 1.5) == [[P.flat(P.simplify(r, 1.5)) for r in rings] for rings in per_label]
    with pytest.raises(ValueError):
        P.label_flat(meta[:, ::-1], words)
    rec = np.concatenate([meta.reshape(-1), words.view(np.int32), np.zeros(5, np.int32)])
    got_meta, got_words = P.split_record(rec, 1, 3, len(words) + 5)
    np.testing.assert_array_equal(got_meta[0], meta)
    np.testing.assert_array_equal(got_words[0, :len(words)], words)
    with pytest.raises(ValueError):
        P.split_record(rec, 1, 3, len(words))
    with pytest.raises(ValueError):
        P.rings_host(m.astype(np.int32), 1)
    assert P.to_coco(P.rings_host(np.pad(np.ones((1, 1), np.uint8), 1), 1)) == [[1.0, 1.0, 2.0, 1.0, 2.0, 2.0, 1.0, 2.0]]
    block = np.ones((5, 5), np.uint8)
    block[2, 2] = 0
    assert len(P.to_coco(P.rings_host(block, 1))) == 1                # the hole is lost there
    assert P.default_capacity(480, 854) == 3416 and P.default_capacity(100, 100) == 2048


# ---- simplify ---------------------------------------------------------------------------------------------------------------------
def test_simplify():
    square = [(3, 4), (4, 4), (4, 5), (3, 5)]
    assert P.simplify(square, 5) == square                            # a 1-pixel ring: fewer than 3 would stay
    kept_fewer = 0
    for i, region in _random_masks():
        if i % 4:
            continue
        for ring in P.rings_host(region.astype(np.uint8), 1):
            assert P.simplify(ring, 0) == ring and P.simplify(ring, None) == ring
            for tol in (0.5, 1.0, 2.5):
                out = P.simplify(ring, tol)
                assert out[0] == ring[0] and len(out) >= 3
                at = [0]
                for p in out[1:]:                                     # a subsequence, in order
                    at.append(ring.index(p, at[-1] + 1))
                closed = ring + [ring[0]]
                for a, b in zip(at, at[1:] + [len(ring)]):
                    for j in range(a + 1, b):
                        assert P._segment_distance(closed[j], closed[a], closed[b]) <= tol + 1e-9
                kept_fewer += len(out) < len(ring)
    assert kept_fewer > 50
    with pytest.raises(ValueError):
        P.simplify(square, -1)


# ---- header, binding and build ----------------------------------------------------------------------------------------------------
def _declared(path):
    text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', text)))


def test_third_header_parses_and_the_library_exports_it():
    from xmem2_amd import _header, _lib, _lib_masks, _lib_polygons, build
    path = os.path.join(ROOT, 'include', 'xmem_hip_polygons.h')
    constants, structs, sigs = _header.parse(open(path).read())
    assert structs == {} and constants['XMEM_POLY_META'] == 2 == _lib_polygons.POLY_META == P.META
    assert 1 << constants['XMEM_POLY_FIRST_BIT'] == int(P.FIRST)
    assert sorted(sigs) == _declared(path) == sorted(_lib_polygons.EXPORTED_SYMBOLS) == ['xmem_mask_polygons', 'xmem_mask_polygons_workspace_bytes']
    assert sigs['xmem_mask_polygons'] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 +
                                          [ctypes.c_size_t, ctypes.c_void_p])
    assert sigs['xmem_mask_polygons_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 5)
    lib = _lib_polygons.load()
    assert lib is _lib.load()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # the first two headers and what is derived from them stay where they are
    assert len(_lib._SIGS) == 103 and _lib.ABI_VERSION == 5 and len(_lib_masks.EXPORTED_SYMBOLS) == 4
    assert not set(sigs) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib_masks.EXPORTED_SYMBOLS))
    assert 'polygons.hip' in build.SOURCES and build.PUBLIC_HEADERS == ['xmem_hip.h', 'xmem_hip_masks.h', 'xmem_hip_polygons.h']


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib_masks, _lib_polygons
    lib = _lib_polygons.load()
    p = ctypes.c_void_p(4096)                                        # never dereferenced: every call below is refused on the host
    big = 1 << 44
    query = lib.xmem_mask_polygons_workspace_bytes

    def trace(masks=p, N=1, H=8, W=8, K=2, capacity=64, meta=p, corners=p, ws=p, nbytes=big):
        return lib.xmem_mask_polygons(masks, N, H, W, K, capacity, meta, corners, ws, nbytes, None)

    need = query(1, 480, 854, 5, 3416)
    cc = _lib_masks.load().xmem_components_workspace_bytes(1, 480, 854)
    assert need >= cc + 4 * (2 * 480 * 854 + 5 * (481 + 855) + 3 * 3416)               # up to 4096 corners are ranked in LDS
    assert query(1, 480, 854, 5, 4097) >= cc + 4 * (2 * 480 * 854 + 5 * (481 + 855) + 11 * 4097) > query(1, 480, 854, 5, 4096)
    assert query(2, 480, 854, 5, 3416) > need and query(1, 480, 854, 5, 6832) > need and query(1, 480, 854, 6, 3416) > need
    assert query(1, 16384, 16384, 254, 1 << 28) > 0 and query(65535, 1, 1, 1, 1) > 0
    for args in ((0, 8, 8, 1, 8), (65536, 8, 8, 1, 8), (1, 0, 8, 1, 8), (1, 8, 0, 1, 8), (1, 16385, 8, 1, 8), (1, 8, 16385, 1, 8),
                 (1, 8, 8, 0, 8), (1, 8, 8, 255, 8), (1, 8, 8, 1, 0), (1, 8, 8, 1, -3), (1, 8, 8, 1, (1 << 28) + 1)):
        assert query(*args) == 0, args
    assert trace(N=0) == BAD_ARG and trace(N=65536) == BAD_ARG and trace(K=0) == BAD_ARG and trace(K=255) == BAD_ARG
    assert trace(capacity=0) == BAD_ARG and trace(capacity=-1) == BAD_ARG and trace(capacity=(1 << 28) + 1) == BAD_ARG
    for kw in ({'H': 0}, {'W': 0}, {'H': 16385}, {'W': 16385}, {'H': -1}):
        assert trace(**kw) == UNSUPPORTED, kw
    for name in ('masks', 'meta', 'corners', 'ws'):
        assert trace(**{name: None}) == BAD_ARG, name
    assert trace(ws=ctypes.c_void_p(4100)) == BAD_ARG                # the workspace is 8-byte aligned
    assert trace(nbytes=0) == WORKSPACE and trace(nbytes=query(1, 8, 8, 2, 64) - 1) == WORKSPACE


def test_ops_refuses_host_tensors_and_bad_options():
    import torch
    from xmem2_amd import ops
    m = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.mask_polygons(m, 1)
    assert set(ops.POLY_STATS) == {'launches', 'retries'}


# ---- the option and the writer --------------------------------------------------------------------------------------------------
def test_parse_polygons_and_the_default_config():
    from xmem2_amd.configuration import VIDEO_INFERENCE_CONFIG
    assert 'tracks_polygons' not in VIDEO_INFERENCE_CONFIG
    assert P.parse_polygons(None) is None and P.parse_polygons(False) is None
    assert P.parse_polygons(True) == {'tolerance': 0} == P.parse_polygons({}) == P.parse_polygons({'tolerance': None})
    assert P.parse_polygons({'tolerance': 1.5}) == {'tolerance': 1.5} and P.parse_polygons({'tolerance': np.float32(2)}) == {'tolerance': 2}
    for bad in ({'tolerance': -1}, {'tolerance': '1'}, {'tolerance': True}, {'tolerance': float('inf')}, {'tolerance': float('nan')},
                {'tol': 1}, 1.5, 'yes', [1]):
        with pytest.raises(ValueError):
            P.parse_polygons(bad)


def _frames():
    rng = np.random.default_rng(20)
    out = []
    for t in range(4):
        m = np.repeat(np.repeat(rng.integers(0, 3, size=(6, 8)), 4, 0), 5, 1).astype(np.uint8)
        m[t:t + 3, 2 * t:2 * t + 3] = 0
        out.append(m)
    out[2] = None                                                     # a frame without mask
    return out


def _written(form, polygons=None):
    from xmem2_amd import rle
    w = rle.TrackWriter(24, 40, polygons=polygons) if polygons is not None else rle.TrackWriter(24, 40)
    for t, m in enumerate(_frames()):
        w.add_mask(f'{t:05d}.jpg', m, k=2, labels=[3, 7], counts=form)
    return json.dumps(w.to_dict(), separators=(',', ':'))


@pytest.mark.parametrize('form', ['list', 'compressed'])
def test_the_writer_with_the_option_off_writes_what_it_wrote_before(form):
    """tests/golden/tracks_writer_<form>.json: these frames through the writer of the commit before the option existed."""
    with open(os.path.join(GOLDEN, f'tracks_writer_{form}.json')) as f:
        assert _written(form) == f.read()


@pytest.mark.parametrize('form', ['list', 'compressed'])
def test_the_writer_with_the_option_on(form):
    from xmem2_amd import rle
    off, exact, loose = (json.loads(_written(form, p)) for p in (None, True, {'tolerance': 1.5}))
    assert 'polygons' not in off['videos'][0] and exact['videos'][0]['polygons'] == {'tolerance': 0, 'fill': 'evenodd'}
    assert loose['videos'][0]['polygons'] == {'tolerance': 1.5, 'fill': 'evenodd'}
    frames = _frames()
    seen = 0
    for a_off, a_exact, a_loose in zip(off['annotations'], exact['annotations'], loose['annotations']):
        assert a_off['bboxes'] == a_exact['bboxes'] and a_off['areas'] == a_exact['areas'] == a_loose['areas']
        dense = [3, 7].index(a_exact['label']) + 1
        for t, (s_off, s_exact, s_loose) in enumerate(zip(a_off['segmentations'], a_exact['segmentations'], a_loose['segmentations'])):
            if s_off is None:
                assert s_exact is None and s_loose is None
                continue
            assert {k: v for k, v in s_exact.items() if k != 'polygons'} == s_off and list(s_exact) == ['size', 'counts', 'polygons']
            np.testing.assert_array_equal(P.fill_host(s_exact['polygons'], 24, 40), frames[t] == dense)
            np.testing.assert_array_equal(P.fill_host(s_exact['polygons'], 24, 40), rle.decode(s_exact['counts'], 24, 40))
            rings = P.rings_host(frames[t], dense)
            assert s_exact['polygons'] == [P.flat(r) for r in rings] and s_loose['polygons'] == [P.flat(P.simplify(r, 1.5)) for r in rings]
            seen += 1
    assert seen >= 5
    reader = rle.TrackReader(exact)                                   # readers ignore the key
    for t, m in enumerate(frames):
        got = reader.mask_host(t)
        assert (got is None) == (m is None)
        if m is not None:
            np.testing.assert_array_equal(got, np.array([0, 3, 7], np.uint8)[m])
    w = rle.TrackWriter(24, 40, polygons=True)
    with pytest.raises(ValueError):
        w.add_frame('x.jpg', np.zeros((1, rle.META), np.int32), np.zeros(0, np.uint32))             # the option on, no polygons given


def test_the_tools_parse_the_option():
    from xmem2_amd import rle
    args = rle.parse_args(['--tracks', 'a.json', '--polygons', '--out', 'b.json'])
    assert args.polygons == 0.0 and args.clean is None and args.recode is None
    assert rle.parse_args(['--tracks', 'a.json', '--polygons', '1.5', '--out', 'b.json']).polygons == 1.5
    assert rle.parse_args(['--tracks', 'a.json', '--out', 'b']).polygons is None
    for bad in ('-1', 'inf', 'x'):
        with pytest.raises(SystemExit):
            rle.parse_args(['--tracks', 'a.json', '--polygons', bad, '--out', 'b.json'])
