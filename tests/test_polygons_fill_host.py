"""Polygons read back, without a GPU: the exact integer fill (xmem2_amd/polygons.py: quantise, fill_exact_host, fill_rows_host,
pack_edges) against the ring tracer, `fill_host` and a brute force in fractions; the fourth header, its binding and the build lists;
the argument checks of the C entry points (which answer before any GPU work); polygon-only entries in `TrackReader` and behind it;
the labelme importer on hand-written fixtures (tests/golden/labelme)."""
import ctypes
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from polygons_fill_refs import clip as _clip, counts_doc as _counts_doc, random_rings, twin as _twin
from xmem2_amd import polygons as P

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # xmem_status (include/xmem_hip.h)
LABELME = os.path.join(GOLDEN, 'labelme')
_MASKS = []


def _random_masks():
    """120 random masks up to 40 x 70 with their rings, made once"""
    if not _MASKS:
        rng = np.random.default_rng(0)
        for _ in range(120):
            h, w = int(rng.integers(1, 41)), int(rng.integers(1, 71))
            m = (rng.random((h, w)) < rng.choice([0.3, 0.5, 0.8])).astype(np.uint8)
            _MASKS.append((m, P.rings_host(m, 1) if m.any() else []))
    return _MASKS


# ---- the definition ---------------------------------------------------------------------------------------------------------------
def test_exact_rings_fill_back_to_their_mask_at_every_grid():
    for m, rings in _random_masks():
        for fb in (0, 4, 8):
            got = P.fill_exact_host(rings, *m.shape, frac_bits=fb)
            assert got.dtype == bool and got.shape == m.shape
            np.testing.assert_array_equal(got, m == 1)
    np.testing.assert_array_equal(P.fill_exact_host([P.flat(r) for r in _random_masks()[3][1]], *_random_masks()[3][0].shape),
                                  _random_masks()[3][0] == 1)        # flat lists are rings too


def test_simplified_integer_rings_fill_as_fill_host_does():
    compared = 0
    for m, rings in _random_masks():
        for tol in (0.7, 1.5, 3.0):
            s = [P.simplify(r, tol) for r in rings]
            np.testing.assert_array_equal(P.fill_exact_host(s, *m.shape), P.fill_host(s, *m.shape))
            compared += 1
    assert compared == 360


def _brute(rings_q, H, W, fb):
    """per pixel: the edges that cross its centre line (half open) at or left of its centre, in fractions"""
    one = 1 << fb
    out = np.zeros((H, W), bool)
    for r in range(H):
        yc = Fraction((2 * r + 1) * one, 2)
        xs = []
        for p in rings_q:
            q = np.roll(p, -1, axis=0)
            for (xa, ya), (xb, yb) in zip(p.tolist(), q.tolist()):
                if ya != yb and min(ya, yb) <= yc < max(ya, yb):
                    xs.append(xa + (yc - ya) * Fraction(xb - xa, yb - ya))
        for c in range(W):
            xc = Fraction((2 * c + 1) * one, 2)
            out[r, c] = sum(x <= xc for x in xs) & 1
    return out


def test_fixed_point_polygons_against_a_brute_force_in_fractions():
    rng = np.random.default_rng(1)
    seen_snapped = seen_outside = 0
    for _ in range(150):
        H, W, fb = int(rng.integers(1, 14)), int(rng.integers(1, 36)), int(rng.choice([1, 4, 8]))
        rings = random_rings(rng, H, W, int(rng.integers(1, 4)))
        pts = np.concatenate([np.asarray(r) for r in rings])
        seen_snapped += int((pts * 2 == np.rint(pts * 2)).all(1).sum())
        seen_outside += int(((pts < 0).any(1) | (pts[:, 0] > W) | (pts[:, 1] > H)).sum())
        got = P.fill_exact_host(rings, H, W, frac_bits=fb)
        want = _brute([P.quantise(r, fb) for r in rings], H, W, fb)
        assert int((got != want).sum()) == 0
    assert seen_snapped > 100 and seen_outside > 100


def test_a_vertex_on_a_centre_line_counts_once():
    # a diamond whose left and right vertices lie on the centre line of row 2: the half-open rule fills that row, the strict one
    # of `fill_host` sees no crossing there
    diamond = [(2.5, 0.5), (4.5, 2.5), (2.5, 4.5), (0.5, 2.5)]
    got = P.fill_exact_host([diamond], 5, 5)
    # row 2: crossings at x = 0.5 and 4.5, a centre AT a crossing is right of it: columns 0..3; row 1: x = 1.5 and 3.5: columns 1, 2
    assert got[2].tolist() == [True, True, True, True, False] and got[1].tolist() == [False, True, True, False, False]
    assert not P.fill_host([diamond], 5, 5)[2].any()
    for ring in ([], [(1, 1)], [(1, 1), (3, 4)], [(1, 1), (1, 1), (1, 1)]):      # fewer than 3 vertices, repeated ones: nothing
        assert not P.fill_exact_host([ring], 6, 6).any()
    bow = P.fill_exact_host([[(0, 0), (6, 6), (6, 0), (0, 6)]], 6, 6)             # a bow-tie: two triangles, even-odd
    # row 1 is crossed at x = 0, 1.5, 4.5 and 6: columns 0, then 4 and 5; the rows hold 1, 3, 5, 5, 3, 1 pixels
    assert bow[1].tolist() == [True, False, False, False, True, True] and bow.sum(1).tolist() == [1, 3, 5, 5, 3, 1]


def test_fill_rows_host_overlap_values_and_base():
    a, b = [[(0, 0), (4, 0), (4, 4), (0, 4)]], [[(2, 2), (6, 2), (6, 6), (2, 6)]]
    m = P.fill_rows_host([a, b], 6, 6)
    assert m.dtype == np.uint8 and m[1, 1] == 1 and m[3, 3] == 2 and m[5, 5] == 2 and m[0, 5] == 0      # the highest row wins
    assert (P.fill_rows_host([b, a], 6, 6)[3, 3], P.fill_rows_host([a, b], 6, 6, values=[9, 9])[3, 3]) == (2, 9)
    np.testing.assert_array_equal(P.fill_rows_host([a, b], 6, 6, values=[9, 9]) == 9, (m > 0))             # a union: equal values
    # the same two squares as ONE row are even-odd: the overlap is outside
    assert P.fill_rows_host([a + b], 6, 6)[3, 3] == 0
    base = np.full((6, 6), 77, np.uint8)
    over = P.fill_rows_host([a], 6, 6, values=[5], base=base)
    assert over[1, 1] == 5 and over[5, 5] == 77 and base[1, 1] == 77
    with pytest.raises(ValueError):
        P.fill_rows_host([a, b], 6, 6, values=[1])
    with pytest.raises(ValueError):
        P.fill_rows_host([a], 6, 6, values=[256])


def test_pack_edges():
    frames = [[[[(0, 0), (4, 0), (4, 3), (0, 3)]], []], [[], [[1.5, 0.25, 3, 2, 0, 2], [(5, 5)]]]]
    edges, plane = P.pack_edges(frames, 2, frac_bits=4)
    assert edges.dtype == plane.dtype == np.int32 and edges.shape == (4, 4) and plane.tolist() == [0, 0, 3, 3]
    assert (edges[:, 1] < edges[:, 3]).all()                          # ya < yb, the horizontals are gone
    assert sorted(edges[:2].tolist()) == [[0, 0, 0, 48], [64, 0, 64, 48]]
    assert sorted(edges[2:].tolist()) == [[24, 4, 0, 32], [24, 4, 48, 32]]
    assert P.pack_edges([[[]], [[]]], 1)[0].shape == (0, 4)
    with pytest.raises(ValueError):
        P.pack_edges([[[], []]], 1)
    # the packed edges are the definition's: toggles rebuilt from them give the fill
    m, rings = _random_masks()[5]
    e, p = P.pack_edges([[rings]], 1, frac_bits=0)
    assert len(e) == sum(len(r) for r in rings) // 2 and not p.any()


def test_quantise_refusals():
    assert P.quantise([0.5, -1.25, 3], 2).tolist() == [2, -5, 12] and P.quantise([2.5, 3.5], 0).tolist() == [2, 4]
    assert P.quantise([(1 << 20)], 8).tolist() == [1 << 28] and P.quantise([], 8).dtype == np.int64
    for bad in ([float('nan')], [float('inf')], [(1 << 20) + 1], [-(1 << 20) - 1]):
        with pytest.raises(ValueError):
            P.quantise(bad, 8)
    for fb in (-1, 9, 2.0, True, None):
        with pytest.raises(ValueError):
            P.quantise([1.0], fb)
    with pytest.raises(ValueError):
        P.fill_exact_host([[(0, 0), (float('nan'), 1), (1, 1)]], 4, 4)


# ---- header, binding and build ----------------------------------------------------------------------------------------------------
def _declared(path):
    text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', text)))


def test_fourth_header_parses_and_the_library_exports_it():
    from xmem2_amd import _header, _lib, _lib_masks, _lib_polygons, _lib_raster, build
    path = os.path.join(ROOT, 'include', 'xmem_hip_raster.h')
    constants, structs, sigs = _header.parse(open(path).read())
    assert structs == {} and constants['XMEM_FILL_MAX_FRAC_BITS'] == 8 == _lib_raster.MAX_FRAC_BITS == P.MAX_FRAC_BITS
    assert constants['XMEM_FILL_COORD_BOUND'] == 1 << 28 == P.COORD_BOUND and constants['XMEM_FILL_STATUS'] == 2
    assert sorted(sigs) == _declared(path) == sorted(_lib_raster.EXPORTED_SYMBOLS) == ['xmem_polygons_fill', 'xmem_polygons_fill_workspace_bytes']
    assert sigs['xmem_polygons_fill'] == (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_int] +
                                          [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p])
    assert sigs['xmem_polygons_fill_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    lib = _lib_raster.load()
    assert lib is _lib.load()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib_masks.EXPORTED_SYMBOLS) | set(_lib_polygons.EXPORTED_SYMBOLS)
    assert not set(sigs) & others and len(others) == 103 + 4 + 2 and _lib.ABI_VERSION == 5
    assert 'polygons_fill.hip' in build.SOURCES and [os.path.basename(p) for p in build.LATER_HEADERS] == ['xmem_hip_raster.h']


def test_build_tracks_the_fourth_header(tmp_path, monkeypatch):
    from xmem2_amd import build
    assert os.path.samefile(build.LATER_HEADERS[0], os.path.join(ROOT, 'include', 'xmem_hip_raster.h'))
    digest = build.source_digest()
    copy = tmp_path / 'xmem_hip_raster.h'
    copy.write_bytes(open(build.LATER_HEADERS[0], 'rb').read())
    monkeypatch.setattr(build, 'LATER_HEADERS', [str(copy)])
    assert build.source_digest() == digest
    assert build.needs_build()                                       # the copy is newer than the library
    copy.write_bytes(copy.read_bytes() + b'\n/* changed */\n')
    assert build.source_digest() != digest


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib_raster
    lib = _lib_raster.load()
    p = ctypes.c_void_p(4096)                                        # never dereferenced: every call below is refused on the host
    big = 1 << 44
    query = lib.xmem_polygons_fill_workspace_bytes

    def fill(edges=p, plane=p, E=3, N=1, H=8, W=8, R=2, frac_bits=8, values=p, overlay=0, masks=p, status=p, ws=p, nbytes=big):
        return lib.xmem_polygons_fill(edges, plane, E, N, H, W, R, frac_bits, values, overlay, masks, status, ws, nbytes, None)

    assert query(1, 480, 854, 5) >= 4 * 5 * 480 * 27 and query(2, 480, 854, 5) >= 2 * 4 * 5 * 480 * 27
    assert query(1, 8, 31, 1) >= 4 * 8 and query(1, 8, 32, 1) >= 4 * 8 * 2          # column W has a bit of its own
    assert query(65535, 16384, 16384, 254) >= 65535 * 254 * 16384 * 513 * 4 and query(1, 1, 1, 1) > 0
    for args in ((0, 8, 8, 1), (65536, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 16385, 8, 1), (1, 8, 16385, 1), (1, 8, 8, 0), (1, 8, 8, 255),
                 (-1, 8, 8, 1), (1, 8, 8, -2)):
        assert query(*args) == 0, args
    for kw in ({'N': 0}, {'N': 65536}, {'R': 0}, {'R': 255}, {'E': -1}, {'frac_bits': -1}, {'frac_bits': 9}):
        assert fill(**kw) == BAD_ARG, kw
    for kw in ({'H': 0}, {'W': 0}, {'H': 16385}, {'W': 16385}, {'H': -1}):
        assert fill(**kw) == UNSUPPORTED, kw
    for name in ('edges', 'plane', 'masks', 'status', 'ws'):
        assert fill(**{name: None}) == BAD_ARG, name
    assert fill(ws=ctypes.c_void_p(4100)) == BAD_ARG                 # the workspace is 8-byte aligned
    assert fill(status=ctypes.c_void_p(4098)) == BAD_ARG and fill(edges=ctypes.c_void_p(4097)) == BAD_ARG
    assert fill(nbytes=0) == WORKSPACE and fill(nbytes=query(1, 8, 8, 2) - 1) == WORKSPACE
    assert fill(E=0, edges=None, plane=None, nbytes=0) == WORKSPACE  # no edges: their pointers are not asked for, the rest is


def test_ops_refuses_host_tensors_and_bad_options():
    import torch
    from xmem2_amd import ops
    square = [[[[(0, 0), (2, 0), (2, 2), (0, 2)]]]]
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.fill_polygons(square, 4, 4, out=torch.zeros(1, 4, 4, dtype=torch.uint8))
    for kw in ({'H': 0}, {'W': 16385}, {'frac_bits': 9}, {'values': [1, 2]}, {'values': [256]}, {'overlay': True}):
        with pytest.raises(ValueError):
            ops.fill_polygons(square, **dict({'H': 4, 'W': 4}, **kw))
    with pytest.raises(ValueError):
        ops.fill_polygons([], 4, 4)
    with pytest.raises(ValueError):
        ops.fill_polygons([[[[(0, 0), (float('inf'), 0), (2, 2)]]]], 4, 4)
    assert set(ops.FILL_STATS) == {'launches'} and ops.FILL_WORKSPACE_CAP == 256 << 20


# ---- readers and the product ------------------------------------------------------------------------------------------------------
def test_a_polygon_only_twin_reads_as_its_counts_file(tmp_path):
    from xmem2_amd import rle
    doc = _counts_doc()
    twin = _twin(doc)
    a, b = rle.TrackReader(doc), rle.TrackReader(twin)
    assert not a.has_polygons() and b.has_polygons() and b.fill == 'evenodd' and a.labels == b.labels == [3, 7, 9]
    for t, m in enumerate(_clip()):
        assert a.has_mask(t) == b.has_mask(t) == (m is not None) and b.has_polygons(t) == (m is not None)
        if m is None:
            assert b.mask_host(t) is None
            continue
        np.testing.assert_array_equal(a.mask_host(t), np.array([0, 3, 7, 9], np.uint8)[m])
        np.testing.assert_array_equal(b.mask_host(t), a.mask_host(t))
        with pytest.raises(ValueError, match='no record'):
            b.record(t)
    path = tmp_path / 'twin.json'
    path.write_text(json.dumps(twin))
    video, masks = rle.read_tracks(path)                              # and so the PNG writer of the command line
    assert masks[2] is None and all((m == a.mask_host(t)).all() for t, m in enumerate(masks) if m is not None)
    assert rle.main(['--tracks', str(path), '--out', str(tmp_path / 'png')]) == 0
    from PIL import Image
    np.testing.assert_array_equal(np.array(Image.open(tmp_path / 'png' / '00003.png')), a.mask_host(3))
    assert rle.recode_tracks(twin, 'compressed') == twin              # nothing to recode
    bad = json.loads(json.dumps(twin))
    bad['annotations'][0]['segmentations'][0]['size'] = [33, 64]      # `size` is optional, and checked when present
    with pytest.raises(ValueError, match='is not the video'):
        rle.TrackReader(bad)
    bad = json.loads(json.dumps(twin))
    bad['videos'][0]['polygons']['fill'] = 'nonzero'
    with pytest.raises(ValueError, match='fill'):
        rle.TrackReader(bad)
    no_boxes = json.loads(json.dumps(doc))
    no_boxes['annotations'][0]['bboxes'] = None                       # a counts track still needs its boxes and areas
    with pytest.raises((ValueError, TypeError)):
        rle.TrackReader(no_boxes)


def test_union_fills_every_ring_on_its_own():
    from xmem2_amd import rle
    rings = [[0, 0, 4, 0, 4, 4, 0, 4], [2, 2, 6, 2, 6, 6, 2, 6]]
    doc = {'videos': [{'id': 1, 'height': 6, 'width': 6, 'length': 1, 'file_names': ['a.jpg'], 'polygons': {'fill': 'union'}}],
           'annotations': [{'id': 1, 'label': 4, 'segmentations': [{'polygons': rings}], 'bboxes': [None], 'areas': [None]}]}
    union = rle.TrackReader(doc).mask_host(0)
    doc['videos'][0]['polygons']['fill'] = 'evenodd'
    evenodd = rle.TrackReader(doc).mask_host(0)
    del doc['videos'][0]['polygons']                                  # the default is what this project writes
    np.testing.assert_array_equal(rle.TrackReader(doc).mask_host(0), evenodd)
    assert union[3, 3] == 4 and evenodd[3, 3] == 0 and union.sum() == 4 * 28 and evenodd.sum() == 4 * 24
    np.testing.assert_array_equal(union == 4, P.fill_exact_host(rings[:1], 6, 6) | P.fill_exact_host(rings[1:], 6, 6))
    np.testing.assert_array_equal(evenodd == 4, P.fill_exact_host(rings, 6, 6))


def test_a_frame_that_mixes_the_forms_is_refused():
    from xmem2_amd import rle
    doc = _counts_doc()
    mixed = json.loads(json.dumps(doc))
    del mixed['annotations'][1]['segmentations'][3]['counts']
    r = rle.TrackReader(mixed)
    with pytest.raises(ValueError, match='frame 3 mixes'):
        r.mask_host(3)
    with pytest.raises(ValueError, match='frame 3 mixes'):
        r.record(3)
    np.testing.assert_array_equal(r.mask_host(1), rle.TrackReader(doc).mask_host(1))      # the other frames read as before
    # an entry with both keys is read from its counts: spoiling the polygons changes nothing
    both = json.loads(json.dumps(doc))
    both['annotations'][0]['segmentations'][0]['polygons'] = [[0, 0, 5, 0, 5, 5]]
    np.testing.assert_array_equal(rle.TrackReader(both).mask_host(0), rle.TrackReader(doc).mask_host(0))


def test_from_labelme_on_the_fixtures(tmp_path):
    from xmem2_amd import rle
    names = ['00000.jpg', '00001.jpg', '00002.jpg']
    doc = P.from_labelme(LABELME, names)
    video = doc['videos'][0]
    assert (video['height'], video['width'], video['length'], video['file_names']) == (12, 16, 3, names)
    assert video['polygons'] == {'fill': 'union'} and video['label_names'] == {'1': 'cat', '2': 'dog'}
    assert [a['label'] for a in doc['annotations']] == [1, 2, 7]
    cat, dog, seven = (a['segmentations'] for a in doc['annotations'])
    assert cat == [None, None, {'size': [12, 16], 'polygons': [[1.3, 2.7, 6.8, 3.1, 4.2, 9.9]]}]
    assert dog == [{'size': [12, 16], 'polygons': [[10.5, 4.0, 19.0, 5.5, 12.0, 13.5]]}, None, None]
    assert seven[0]['polygons'] == [[2.0, 1.5, 9.25, 1.5, 9.25, 6.0, 2.0, 6.0]] and seven[1:] == [None, None]
    assert all(a['bboxes'] == [None] * 3 == a['areas'] for a in doc['annotations'])
    r = rle.TrackReader(json.loads(json.dumps(doc)))
    assert [r.has_mask(t) for t in range(3)] == [True, False, True] and r.mask_host(1) is None and r.fill == 'union'
    m0 = r.mask_host(0)
    want = np.zeros((12, 16), np.uint8)
    want[1:6, 2:9] = 7                       # centres 1.5 .. 5.5 lie in [1.5, 6) - half open -, centres 2.5 .. 8.5 in [2, 9.25)
    np.testing.assert_array_equal(m0 == 7, want == 7)
    np.testing.assert_array_equal(m0 == 2, P.fill_exact_host([[10.5, 4.0, 19.0, 5.5, 12.0, 13.5]], 12, 16))
    assert (m0 == 2).sum() > 10 and (m0 == 2)[:, 15].any() and set(np.unique(m0)) == {0, 2, 7}      # it runs off the right side
    np.testing.assert_array_equal(r.mask_host(2) == 1, P.fill_exact_host([[1.3, 2.7, 6.8, 3.1, 4.2, 9.9]], 12, 16))
    # without file_names the annotated frames are the video; a list of files is taken as the directory is
    only = P.from_labelme([os.path.join(LABELME, '00002.json'), os.path.join(LABELME, '00000.json')])
    assert only['videos'][0]['file_names'] == ['00002', '00000'] and only['annotations'][0]['segmentations'][1] is None
    with pytest.raises(ValueError, match=r"00000\.json, shape 0 \('cat'\) is a 'rectangle'"):
        P.from_labelme(os.path.join(GOLDEN, 'labelme_rectangle'))
    with pytest.raises(ValueError, match='no frame is named'):
        P.from_labelme(LABELME, ['00000.jpg'])
    out = tmp_path / 'sub' / 'tracks.json'
    assert rle.main(['--from-labelme', LABELME, '--out', str(out)]) == 0
    assert json.loads(out.read_text()) == P.from_labelme(LABELME)
    for argv in (['--out', 'x'], ['--tracks', 'a', '--from-labelme', 'b', '--out', 'x'], ['--tracks', 'a'],
                 ['--from-labelme', 'b', '--out', 'x', '--from-polygons']):
        with pytest.raises(SystemExit):
            rle.parse_args(argv)
    args = rle.parse_args(['--tracks', 'a.json', '--verify-polygons'])
    assert args.verify_polygons and args.out is None and not args.from_polygons
    assert rle.parse_args(['--tracks', 'a.json', '--from-polygons', '--out', 'b.json']).from_polygons


def test_the_annotation_reader_of_run_on_video_takes_the_twin(tmp_path):
    """`VideoReader` is what `run_on_video` builds for `masks_in_path`: the first annotation it yields is the same from both files."""
    from PIL import Image
    from xmem2_amd.run_on_video import VideoReader
    imgs = tmp_path / 'JPEGImages'
    imgs.mkdir()
    for t in range(5):
        Image.new('RGB', (65, 33), (10 * t, 0, 0)).save(imgs / f'{t:05d}.jpg')
    doc = _counts_doc()
    masks = {}
    for name, d in (('counts', doc), ('twin', _twin(doc))):
        (tmp_path / name).mkdir()
        (tmp_path / name / 'tracks.json').write_text(json.dumps(d))
        reader = VideoReader('', str(imgs), str(tmp_path / name), use_all_masks=False)
        assert reader.tracks is not None
        got = [reader[i].mask for i in range(len(reader))]
        assert got[0] is not None and all(m is None for m in got[1:])
        masks[name] = got[0]
    np.testing.assert_array_equal(masks['twin'], masks['counts'])
    np.testing.assert_array_equal(masks['counts'], np.array([0, 3, 7, 9], np.uint8)[_clip()[0]])
