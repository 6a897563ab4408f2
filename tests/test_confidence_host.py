"""Confidence and uncertainty maps on the host: `confidence.stats_host` on hand-written cases with known answers, `parse_confidence`,
`review_queue` on a made-up table, the eighth header with its binding and its place in the build, the entry points' refusals (which
touch no GPU), the tracks writer with and without scores, and that `run_on_video` does not import the module on its own."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import confidence_refs as R
from conftest import ROOT
from xmem2_amd import confidence as CF

HEADER = os.path.join(ROOT, 'include', 'xmem_hip_confidence.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
BAD_ARG, UNSUPPORTED = -1, -2


def _pixel(values, tau=CF.DEFAULT_TAU, passes=None):
    """one pixel with these class scores -> (top, q, record as nested lists)"""
    dtype = np.float32 if passes is None else np.uint16
    mask, plane, record = CF.stats_host(np.array(values, dtype).reshape(-1, 1, 1), tau, passes)
    assert mask.shape == plane.shape == (1, 1) and mask.dtype == plane.dtype == np.uint8 and record.dtype == np.int64
    return int(mask[0, 0]), 255 - int(plane[0, 0]), record.tolist()


# ---- the definition ---------------------------------------------------------------------------------------------------------------------

def test_one_class():
    assert _pixel([0.5]) == (0, 128, [[1, 128, 0, 0]])                              # m = p[top]; no second, nothing contested
    assert _pixel([0.125]) == (0, 32, [[1, 32, 1, 0]])
    assert _pixel([0.0]) == (0, 0, [[1, 0, 1, 0]])
    assert _pixel([1.0]) == (0, 255, [[1, 255, 0, 0]])


def test_an_exact_tie():
    # q == 0, top the first index, second the first of the rest
    assert _pixel([0.25, 0.5, 0.5, 0.5]) == (1, 0, [[0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]])
    assert _pixel([0.5, 0.5]) == (0, 0, [[1, 0, 1, 0], [0, 0, 0, 1]])
    assert _pixel([0.5, 0.25, 0.25]) == (0, 64, [[1, 64, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])     # the second's own tie: q = tau is not low
    assert _pixel([0.5, 0.25, 0.25], tau=65)[2] == [[1, 64, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]]   # ... and goes to the first of them


def test_the_floor_and_the_cap():
    just_under = np.nextafter(np.float32(10 / 256), np.float32(0))
    assert _pixel([just_under, 0.0])[1] == 9                                        # m * 256 just under an integer
    assert _pixel([10 / 256, 0.0])[1] == 10                                         # ... and exactly on it
    assert _pixel([0.75, 0.25])[1] == 128
    assert _pixel([255 / 256, 0.0])[1] == 255                                       # m * 256 == 255
    assert _pixel([np.nextafter(np.float32(255 / 256), np.float32(0)), 0.0])[1] == 254
    assert _pixel([1.0, 0.0])[1] == 255                                             # m * 256 == 256: capped
    assert _pixel([0.0, 1e-30])[:2] == (1, 0)                                       # m > 0 but below 1 / 256
    assert _pixel([-0.5, -0.25])[:2] == (1, 64)                                     # only the difference counts


def test_the_threshold():
    tau = 40
    for q, low in ((tau - 1, 1), (tau, 0)):
        top, got, record = _pixel([0.0, q / 256], tau)
        assert (top, got) == (1, q) and record == [[0, 0, 0, low], [1, q, low, 0]]
    assert _pixel([0.0, 0.0], tau=0)[2] == [[1, 0, 0, 0], [0, 0, 0, 0]]             # tau = 0: nothing is low
    assert _pixel([1.0, 0.0], tau=256)[2] == [[1, 255, 1, 0], [0, 0, 0, 1]]         # tau = 256: everything is
    for bad in (-1, 257, True, 64.0, None):
        with pytest.raises(ValueError, match='tau'):
            CF.stats_host(np.zeros((2, 1, 1), np.float32), bad)


def test_the_integer_route():
    assert _pixel([100, 30], passes=1) == (0, 70, [[1, 70, 0, 0], [0, 0, 0, 0]])
    assert _pixel([1020, 0], passes=4)[1] == 255 and _pixel([1019, 0], passes=4)[1] == 254       # floor division
    assert _pixel([400, 147, 400], passes=4) == (0, 0, [[1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 1]])
    assert _pixel([400, 147], passes=4)[1] == 63 and _pixel([400, 147], passes=4)[2][0] == [1, 63, 1, 0]
    assert _pixel([65535, 0], passes=257)[1] == 255 and _pixel([65535, 257], passes=257)[1] == 254
    assert _pixel([65535, 0], passes=1)[1] == 255                                   # capped
    assert _pixel([777], passes=4) == (0, 194, [[1, 194, 0, 0]])
    for bad in (0, 258, True, 2.0):
        with pytest.raises(ValueError, match='passes'):
            CF.stats_host(np.zeros((2, 1, 1), np.uint16), 64, bad)
    with pytest.raises(ValueError):
        CF.stats_host(np.zeros((2, 1, 1), np.float32), 64, 2)                      # the dtype says which route
    with pytest.raises(ValueError):
        CF.stats_host(np.zeros((2, 1, 1), np.uint16))
    with pytest.raises(ValueError):
        CF.stats_host(np.zeros((256, 1, 1), np.float32))


def test_a_frame_adds_up():
    prob = R.scores(np.random.default_rng(5), 4, 9, 11)
    mask, plane, record = CF.stats_host(prob, 64)
    np.testing.assert_array_equal(mask, prob.argmax(0))                             # numpy's argmax is the first maximal index too
    q = 255 - plane.astype(np.int64)
    srt = np.sort(prob, 0)
    np.testing.assert_array_equal(q, np.minimum(255, ((srt[-1] - srt[-2]) * 256).astype(np.int64)))
    assert record[:, 0].sum() == 99 and record[:, 1].sum() == q.sum() and record[:, 2].sum() == record[:, 3].sum() == (q < 64).sum()
    assert (q == 0).any() and (q == 255).any() and ((q > 0) & (q < 64)).any()


def test_derived_values():
    area = np.array([[50, 10, 0], [60, 0, 0], [40, 10, 10]])
    msum = np.array([[50 * 255, 10 * 51, 0], [60 * 255, 0, 0], [40 * 200, 10 * 255, 10 * 102]])
    conf = CF.object_confidence(area, msum)
    assert conf[0, 0] == 1.0 and conf[0, 1] == 0.2 and np.isnan(conf[0, 2]) and conf.dtype == np.float64
    fc = CF.frame_confidence(area, msum)
    assert fc[0] == 0.2 and np.isnan(fc[1]) and fc[2] == 0.4                        # the background is no object
    assert np.isnan(CF.frame_confidence(area[:, :1], msum[:, :1])).all()
    ts = CF.track_scores(area, msum, [False, False, True])
    assert ts[1] == 0.2 and np.isnan(ts[2]) and ts[0] == 1.0
    assert CF.track_scores(area, msum, [True, False, False])[1] == 1.0


# ---- the option -----------------------------------------------------------------------------------------------------------------------

def test_parse_confidence():
    from xmem2_amd.configuration import VIDEO_INFERENCE_CONFIG
    assert 'confidence' not in VIDEO_INFERENCE_CONFIG
    assert CF.parse_confidence(None) is None
    assert CF.parse_confidence(True) == CF.parse_confidence({}) == {'threshold': 64, 'maps': False}
    assert CF.parse_confidence({'threshold': 0, 'maps': True}) == {'threshold': 0, 'maps': True}
    assert CF.parse_confidence({'threshold': np.int64(256)}) == {'threshold': 256, 'maps': False}
    assert CF.parse_confidence({'maps': True}) == {'threshold': 64, 'maps': True}
    for bad in (False, 1, 64, 'yes', [64], {'threshold': -1}, {'threshold': 257}, {'threshold': 64.0}, {'threshold': True},
                {'maps': 1}, {'maps': None}, {'tau': 64}, {'threshold': 64, 'plane': True}):
        with pytest.raises(ValueError, match='confidence'):
            CF.parse_confidence(bad)


def test_review_queue():
    nan = float('nan')
    #       0    1    2    3    4    5    6    7
    conf = [0.9, 0.2, 0.5, 0.2, nan, 0.1, 0.3, nan]
    assert CF.review_queue(conf, k=3) == [5, 1, 3]                                  # lowest first, ties to the lower index
    assert CF.review_queue(conf, k=8) == [5, 1, 3, 6, 2, 0, 4, 7]                   # NaN last, in index order
    assert CF.review_queue(conf, skip=[5, 1], k=3) == [3, 6, 2]                     # references and frames without a mask
    assert CF.review_queue(conf, k=3, min_gap=1) == [5, 1, 3]
    assert CF.review_queue(conf, k=4, min_gap=1) == [5, 1, 3, 7]                    # 6, 2, 0 and 4 each sit next to a chosen frame
    assert CF.review_queue(conf, k=3, min_gap=2) == [5, 1]                          # 3 is within 2 of 1, 7 within 2 of 5
    assert CF.review_queue(conf, k=4, min_gap=3) == [5, 1]
    assert CF.review_queue(conf, skip=range(8), k=2) == [] and CF.review_queue([], k=2) == []
    assert CF.review_queue(conf, k=100) == CF.review_queue(conf, k=8)
    for kw in ({'k': 0}, {'k': True}, {'k': 1.0}, {'min_gap': -1}, {'min_gap': 0.5}):
        with pytest.raises(ValueError):
            CF.review_queue(conf, **kw)


# ---- the eighth header, its binding, the build -----------------------------------------------------------------------------------------

def test_eighth_header_parses_and_the_library_exports_it():
    from xmem2_amd import _header, _lib, _lib_confidence, _lib_masks, _lib_matte, _lib_png, _lib_polygons, _lib_raster, _lib_temporal, build
    text = open(HEADER).read()
    constants, structs, sigs = _header.parse(text)
    assert structs == {} and constants == {'XMEM_CONFIDENCE_MAX_C': 255, 'XMEM_CONFIDENCE_MAX_TAU': 256, 'XMEM_CONFIDENCE_MAX_PASSES': 257,
                                           'XMEM_CONFIDENCE_RECORD': 4, 'XMEM_CONFIDENCE_AREA': 0, 'XMEM_CONFIDENCE_MARGIN_SUM': 1,
                                           'XMEM_CONFIDENCE_LOW': 2, 'XMEM_CONFIDENCE_CONTESTED': 3}
    assert (_lib_confidence.MAX_C, _lib_confidence.MAX_TAU, _lib_confidence.MAX_PASSES) == (CF.MAX_C, CF.MAX_TAU, CF.MAX_PASSES)
    assert _lib_confidence.RECORD == len(CF.FIELDS)
    assert [CF.FIELDS[i] for i in (_lib_confidence.AREA, _lib_confidence.MARGIN_SUM, _lib_confidence.LOW, _lib_confidence.CONTESTED)] == list(CF.FIELDS)
    declared = sorted(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S))))
    assert sorted(sigs) == declared == sorted(_lib_confidence.EXPORTED_SYMBOLS) == ['xmem_confidence_f32', 'xmem_confidence_u16']
    i, p = ctypes.c_int, ctypes.c_void_p
    assert sigs['xmem_confidence_f32'] == (i, [p] + [i] * 4 + [p] * 4)
    assert sigs['xmem_confidence_u16'] == (i, [p] + [i] * 5 + [p] * 4)
    lib = _lib_confidence.load()
    assert lib is _lib.load()
    for name in sigs:
        fn = getattr(lib, name)
        assert fn.restype is i and list(fn.argtypes) == sigs[name][1]
    others = set()
    for m in (_lib, _lib_masks, _lib_polygons, _lib_raster, _lib_matte, _lib_temporal, _lib_png):
        others |= set(m.EXPORTED_SYMBOLS)
    assert not set(sigs) & others and len(_lib.EXPORTED_SYMBOLS) == 103 and _lib.ABI_VERSION == 5
    assert build.SOURCES[-1] == 'confidence.hip' and [os.path.basename(f) for f in build.CONFIDENCE_HEADERS] == ['xmem_hip_confidence.h']


def test_build_tracks_the_eighth_header(tmp_path, monkeypatch):
    from xmem2_amd import build
    assert os.path.samefile(build.CONFIDENCE_HEADERS[0], HEADER)
    digest = build.source_digest()
    copy = tmp_path / 'xmem_hip_confidence.h'
    copy.write_bytes(open(HEADER, 'rb').read())
    monkeypatch.setattr(build, 'CONFIDENCE_HEADERS', [str(copy)])
    assert build.source_digest() == digest
    assert build.needs_build()                                       # the copy is newer than the library
    copy.write_bytes(copy.read_bytes() + b'\n/* changed */\n')
    assert build.source_digest() != digest


def test_the_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib_confidence
    lib = _lib_confidence.load()
    p = ctypes.c_void_p(4096)                                        # never dereferenced: every call below is refused on the host

    def f32(prob=p, C=3, H=8, W=8, tau=64, mask=p, plane=p, record=p):
        return lib.xmem_confidence_f32(prob, C, H, W, tau, mask, plane, record, None)

    def u16(acc=p, passes=2, C=3, H=8, W=8, tau=64, mask=p, plane=p, record=p):
        return lib.xmem_confidence_u16(acc, passes, C, H, W, tau, mask, plane, record, None)

    for call in (f32, u16):
        for kw in ({'record': None}, {'record': ctypes.c_void_p(4100)}, {'C': 0}, {'C': 256}, {'C': -1}, {'tau': -1}, {'tau': 257}):
            assert call(**kw) == BAD_ARG, (call.__name__, kw)
        for kw in ({'H': 0}, {'W': 0}, {'H': -1}, {'H': 16385}, {'W': 16385}):
            assert call(**kw) == UNSUPPORTED, (call.__name__, kw)
    assert f32(prob=None) == BAD_ARG and u16(acc=None) == BAD_ARG
    for passes in (0, -1, 258):
        assert u16(passes=passes) == BAD_ARG, passes


def test_the_op_refuses_host_tensors_and_bad_options():
    import torch
    from xmem2_amd import ops
    for call in (lambda: ops.confidence_stats(torch.zeros((2, 4, 4))), lambda: ops.confidence_stats(torch.zeros((2, 4, 4), dtype=torch.uint16), passes=2)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()


# ---- the tracks writer -----------------------------------------------------------------------------------------------------------------

def _writer(form):
    from xmem2_amd import rle
    rng = np.random.default_rng(20)                                  # the frames of tests/golden/tracks_writer_<form>.json
    w = rle.TrackWriter(24, 40)
    for t in range(4):
        m = np.repeat(np.repeat(rng.integers(0, 3, size=(6, 8)), 4, 0), 5, 1).astype(np.uint8)
        m[t:t + 3, 2 * t:2 * t + 3] = 0
        w.add_mask(f'{t:05d}.jpg', None if t == 2 else m, k=2, labels=[3, 7], counts=form)
    return w


@pytest.mark.parametrize('form', ['list', 'compressed'])
def test_the_tracks_writer_with_and_without_scores(form):
    from xmem2_amd import rle
    with open(os.path.join(GOLDEN, f'tracks_writer_{form}.json')) as f:
        golden = f.read()
    assert json.dumps(_writer(form).to_dict(), separators=(',', ':')) == golden     # without scores: the bytes it always wrote
    w = _writer(form)
    nan = float('nan')
    w.set_confidence({3: (0.75, [0.5, 0.625, nan, nan]), 7: (nan, [0.25, 0.125, 0.0, 1.0])})
    text = json.dumps(w.to_dict(), separators=(',', ':'))
    assert 'NaN' not in text
    doc, off = json.loads(text), json.loads(golden)
    assert [a['score'] for a in doc['annotations']] == [0.75, None]
    want = {3: [0.5, 0.625, None, None], 7: [0.25, 0.125, None, 1.0]}
    for ann in doc['annotations']:
        assert list(ann)[-1] == 'score'
        for t, seg in enumerate(ann['segmentations']):
            assert (seg is None) == (t == 2)
            if seg is not None:
                assert list(seg) == ['size', 'counts', 'confidence'] and seg.pop('confidence') == want[ann['label']][t]
        del ann['score']
    assert doc == off                                                               # minus the two keys: the same file
    reader = rle.TrackReader(json.loads(text))                                      # the readers ignore both
    plain = rle.TrackReader(off)
    for t in range(4):
        assert (reader.mask_host(t) is None) == (plain.mask_host(t) is None)
        if t != 2:
            np.testing.assert_array_equal(reader.mask_host(t), plain.mask_host(t))


# ---- nothing is imported without the key ---------------------------------------------------------------------------------------------

def test_run_on_video_does_not_import_the_module():
    code = ('import sys; import xmem2_amd.run_on_video, xmem2_amd.session; '
            'bad = [m for m in sys.modules if m.endswith(("xmem2_amd.confidence", "xmem2_amd._lib_confidence"))]; '
            'print(bad); sys.exit(1 if bad else 0)')
    done = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
