"""GPU tests of the tools behind `python -m xmem2_amd.rle` (xmem2_amd/rle.py: `clean_tracks`, `grow_tracks`, `polygon_tracks`,
`verify_polygons`, `counts_from_polygons`, `main`) on five frames of 23 x 37 in batches of two, so the last batch is short.  Every
expected document is built from the host definitions - `TrackWriter.add_mask`, `mask_cleanup.clean_host`, `matte.grow_host`,
`polygons.record_host` / `label_flat`, `polygons.fill_rows_host` - and compared as a whole; the launches of the encoder, the tracer
and the fill across each call are those of ceil(frames / batch) batches."""
import json
import math

import numpy as np
import pytest

from xmem2_amd import matte, ops, rle
from xmem2_amd import polygons as P
from xmem2_amd.mask_cleanup import STATS, clean_host, parse_cleanup

pytestmark = pytest.mark.gpu
H, W, T, BATCH = 23, 37, 5, 2
NB = math.ceil(T / BATCH)
NAMES = [f'{t:05d}.jpg' for t in range(T)]
LABELS = [7, 3, 5]                                                    # in file order; 5 never has a pixel
SPEC = parse_cleanup({'min_area': 3, 'max_hole': 4})


def _clip():
    """dense maps, ids in file order (1 is label 7, 2 is label 3); frame 2 has no mask.  Object 1 ends in column 14 + t and object 2
    begins in column 16 + t: one background column between them.  A speckle each, a hole of 2 pixels and one of 6."""
    frames = []
    for t in range(T):
        m = np.zeros((H, W), np.uint8)
        m[3:13, 4 + t:15 + t] = 1
        m[3:13, 16 + t:25 + t] = 2
        m[6:8, 7 + t] = 0
        m[9:11, 18 + t:21 + t] = 0
        m[17, 30 - t] = 1
        m[20, 3 + t] = 2
        frames.append(None if t == 2 else m)
    return frames


def _doc(frames, labels=LABELS, names=NAMES, counts='list', polygons=None):
    w = rle.TrackWriter(H, W, polygons=polygons)
    for n, m in zip(names, frames):
        w.add_mask(n, m, k=len(labels), labels=labels, counts=counts)
    return w.to_dict()


def _cleaned(frames):
    """(frames, totals) by `clean_host`"""
    done = [None if m is None else clean_host(m, **SPEC) for m in frames]
    totals = np.sum([s for _, s in (d for d in done if d is not None)], axis=0, dtype=np.int64) if any(d is not None for d in done) \
        else np.zeros(len(STATS), np.int64)
    return [None if d is None else d[0] for d in done], dict(zip(STATS, (int(v) for v in totals)))


def _grown(frames, r, labels=LABELS):
    """(frames with dense ids in ascending order of the labels, those labels) by `grow_host` on the label maps"""
    to_label = np.array([0] + list(labels), np.uint8)
    order = sorted(labels)
    to_dense = np.zeros(256, np.uint8)
    to_dense[order] = np.arange(1, len(order) + 1)
    return [None if m is None else to_dense[matte.grow_host(to_label[m], r)] for m in frames], order


def _nulled(doc):
    """the document with every entry null: tracks without any entry"""
    out = json.loads(json.dumps(doc))
    for ann in out['annotations']:
        for key in ('segmentations', 'bboxes', 'areas'):
            ann[key] = [None] * T
    return out


def _launches():
    return np.array([ops.RLE_STATS['launches'], ops.POLY_STATS['launches'], ops.FILL_STATS['launches']])


def _same(got, want):
    assert got == want
    assert json.dumps(got) == json.dumps(want)                        # the order of the keys too


def _twin(doc):
    """the polygon-only twin: `counts`, `size`, `bboxes` and `areas` gone; the third track, which has no entry, gets one whose polygon
    encloses no pixel centre"""
    out = json.loads(json.dumps(doc))
    for ann in out['annotations']:
        ann['segmentations'] = [None if seg is None else {'polygons': seg['polygons']} for seg in ann['segmentations']]
        del ann['bboxes'], ann['areas']
    out['annotations'][2]['segmentations'][1] = {'polygons': [[2, 2, 2.4, 2, 2.4, 2.4, 2, 2.4]]}
    return out


# ---- clean_tracks ---------------------------------------------------------------------------------------------------------------------
def test_clean_tracks_on_lists_strings_and_both():
    frames = _clip()
    cleaned, totals = _cleaned(frames)
    assert totals['components_removed'] == 8 and totals['pixels_removed'] == 8 and totals['holes_filled'] == 4 and totals['pixels_filled'] == 8
    before = _launches()
    doc, got = rle.clean_tracks(_doc(frames), SPEC, batch=BATCH)
    assert (_launches() - before).tolist() == [NB, 0, 0]
    _same(doc, _doc(cleaned))
    assert got == totals and list(got) == list(STATS)
    assert [a['label'] for a in doc['annotations']] == LABELS and doc['annotations'][2]['segmentations'] == [None] * T
    doc, got = rle.clean_tracks(_doc(frames, counts='compressed'), SPEC, batch=BATCH)
    _same(doc, _doc(cleaned, counts='compressed'))
    assert got == totals
    mixed = _doc(frames)
    for seg in mixed['annotations'][0]['segmentations']:
        if seg is not None:
            seg['counts'] = rle.compress_counts(seg['counts'])
    doc, got = rle.clean_tracks(mixed, SPEC, batch=BATCH)
    _same(doc, _doc(cleaned))                                         # lists, unless every entry was a string
    assert got == totals


def test_clean_and_grow_of_files_without_names_without_tracks_and_without_entries(tmp_path):
    frames = _clip()
    cleaned, totals = _cleaned(frames)
    numbers = [str(t) for t in range(T)]
    unnamed = _doc(frames)
    del unnamed['videos'][0]['file_names']
    path = tmp_path / 'unnamed.json'
    path.write_text(json.dumps(unnamed))                              # the file, not the document
    doc, got = rle.clean_tracks(str(path), SPEC, batch=BATCH)
    _same(doc, _doc(cleaned, names=numbers))
    assert got == totals
    grown, order = _grown(frames, -1)
    _same(rle.grow_tracks(str(path), -1, batch=BATCH), _doc(grown, labels=order, names=numbers))
    # frames and no tracks: the frames, nothing else, and no launch
    bare = _doc([None] * T)
    assert bare['annotations'] == [] and bare['videos'][0]['file_names'] == NAMES
    before = _launches()
    doc, got = rle.clean_tracks(bare, SPEC, batch=BATCH)
    _same(doc, bare)
    assert got == dict.fromkeys(STATS, 0)
    _same(rle.grow_tracks(bare, 2, batch=BATCH), bare)
    assert (_launches() - before).tolist() == [0, 0, 0]               # no track: there is nothing to decode or to encode
    # tracks and no entry: every empty row survives, in file order when cleaned and in ascending order of the labels when grown
    empty = _nulled(_doc(frames))
    before = _launches()
    doc, got = rle.clean_tracks(empty, SPEC, batch=BATCH)
    _same(doc, empty)
    assert got == dict.fromkeys(STATS, 0)
    doc = rle.grow_tracks(empty, 1, batch=BATCH)
    assert (_launches() - before).tolist() == [2 * NB, 0, 0]
    want = json.loads(json.dumps(empty))
    want['annotations'] = [dict(want['annotations'][i], id=n) for n, i in enumerate((1, 2, 0), start=1)]       # the labels 3, 5, 7
    _same(doc, want)


# ---- grow_tracks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', (1, -1, 2.5))
def test_grow_tracks(r):
    frames = _clip()
    grown, order = _grown(frames, r)
    assert order == [3, 5, 7]
    if r == 1:                                                        # the column between the two objects is one pixel from either
        assert all(m[5, 15 + t] == 1 and m[5, 14 + t] == 3 and m[5, 16 + t] == 1 for t, m in enumerate(grown) if m is not None)
    before = _launches()
    doc = rle.grow_tracks(_doc(frames), r, batch=BATCH)
    assert (_launches() - before).tolist() == [NB, 0, 0]
    _same(doc, _doc(grown, labels=order))
    assert [a['label'] for a in doc['annotations']] == [3, 5, 7] and doc['annotations'][1]['areas'] == [None] * T
    if r == 1:
        _same(rle.grow_tracks(_doc(frames, counts='compressed'), r, batch=BATCH), _doc(grown, labels=order, counts='compressed'))


# ---- polygon_tracks -------------------------------------------------------------------------------------------------------------------
def test_polygon_tracks_replaces_the_polygons_some_entries_have():
    frames = _clip()
    given = _doc(frames)
    junk = [[0, 0, 1, 0, 1, 1]]
    seg = given['annotations'][0]['segmentations']
    seg[0] = dict({'polygons': junk}, **seg[0])                       # the key comes first here, and stays first
    seg[3]['polygons'] = junk
    given['annotations'][1]['segmentations'][4]['polygons'] = junk
    want = json.loads(json.dumps(given))
    for t, m in enumerate(frames):
        if m is not None:
            for ann, rings in zip(want['annotations'], P.label_flat(*P.record_host(m, len(LABELS)), 0)):
                if ann['segmentations'][t] is not None:
                    ann['segmentations'][t]['polygons'] = rings
    want['videos'][0]['polygons'] = {'tolerance': P.parse_polygons({'tolerance': 0})['tolerance'], 'fill': 'evenodd'}
    before = _launches()
    doc = rle.polygon_tracks(given, {'tolerance': 0}, batch=BATCH)
    assert (_launches() - before).tolist() == [0, NB, 0]
    _same(doc, want)
    assert list(doc['annotations'][0]['segmentations'][0]) == ['polygons', 'size', 'counts']
    assert list(doc['annotations'][0]['segmentations'][1]) == ['size', 'counts', 'polygons']
    assert junk not in [s['polygons'] for a in doc['annotations'] for s in a['segmentations'] if s is not None]
    assert given['annotations'][0]['segmentations'][3]['polygons'] == junk      # the document that was passed is left alone
    assert doc == _doc(frames, polygons={'tolerance': 0})             # what the writer makes of the clip with the option on


# ---- verify_polygons ------------------------------------------------------------------------------------------------------------------
def _box(x0, y0, x1, y1):
    """the outline of the pixels x0..x1, y0..y1 as a flat ring of lattice corners"""
    return [x0, y0, x1 + 1, y0, x1 + 1, y1 + 1, x0, y1 + 1]


def _ring_clip():
    """track 1 (label 7): a frame of pixels around a hole; track 2 (label 3): a box that moves; frame 2 has no mask"""
    frames = []
    for t in range(T):
        m = np.zeros((H, W), np.uint8)
        m[4:12, 5:16] = 1
        m[6:10, 8:13] = 0
        m[14:20, 20 + t:27 + t] = 2
        frames.append(None if t == 2 else m)
    return frames


def _exact(fill):
    """an exact file of `_ring_clip` under the rule `fill`: with the hole as a ring, or as four overlapping boxes around it"""
    doc = _doc(_ring_clip(), labels=[7, 3], polygons=True)
    if fill == 'union':
        doc['videos'][0]['polygons']['fill'] = 'union'
        for seg in doc['annotations'][0]['segmentations']:
            if seg is not None:
                seg['polygons'] = [_box(5, 4, 15, 5), _box(5, 10, 15, 11), _box(5, 4, 7, 11), _box(13, 4, 15, 11)]
    return doc


def _polygon_only(doc):
    """`doc` without its counts: the reader then fills the polygons"""
    out = json.loads(json.dumps(doc))
    for ann in out['annotations']:
        for seg in ann['segmentations']:
            if seg is not None:
                del seg['counts']
    return out


@pytest.mark.parametrize('fill', rle.FILL_RULES)
def test_verify_polygons_on_an_exact_file_and_under_the_other_rule(fill):
    doc = _exact(fill)
    assert len(doc['annotations'][0]['segmentations'][0]['polygons']) == (2 if fill == 'evenodd' else 4)
    for t in (0, 1, 3, 4):                                            # the host's fill agrees that the file is exact
        np.testing.assert_array_equal(rle.TrackReader(doc).mask_host(t), rle.TrackReader(_polygon_only(doc)).mask_host(t))
    before = _launches()
    report = rle.verify_polygons(doc, batch=BATCH)
    assert (_launches() - before).tolist() == [0, 0, math.ceil(4 / BATCH)]      # the four frames that have entries
    track = {'frames': 4, 'differ': 0, 'min_iou': 1.0, 'mean_iou': 1.0}
    assert report == {'tolerance': 0, 'fill': fill, 'tracks': [dict(track, id=1, label=7), dict(track, id=2, label=3)], 'frames': 4, 'differ': 0}
    assert list(report) == ['tolerance', 'fill', 'tracks', 'frames', 'differ']
    assert list(report['tracks'][0]) == ['id', 'label', 'frames', 'differ', 'min_iou', 'mean_iou']
    # the same polygons under the other rule: the hole is filled (union of the two rings), or the corners of the boxes cancel (even-odd)
    doc['videos'][0]['polygons']['fill'] = 'union' if fill == 'evenodd' else 'evenodd'
    report = rle.verify_polygons(doc, batch=BATCH)
    area, hole, corners = 8 * 11 - 4 * 5, 4 * 5, 4 * 2 * 3
    iou = area / (area + hole) if fill == 'evenodd' else (area - corners) / area
    assert report['differ'] == 4 and report['tracks'][1] == dict(track, id=2, label=3)
    assert report['tracks'][0] == {'id': 1, 'label': 7, 'frames': 4, 'differ': 4, 'min_iou': iou, 'mean_iou': float(np.mean([iou] * 4))}


def test_verify_polygons_reports_the_track_and_the_frame_of_a_moved_polygon():
    doc = _exact('evenodd')
    seg = doc['annotations'][1]['segmentations'][3]
    assert P.fill_exact_host(seg['polygons'], H, W).tolist() == P.fill_exact_host([_box(23, 14, 29, 19)], H, W).tolist()
    seg['polygons'] = [_box(24, 14, 30, 19)]                          # one pixel to the right
    report = rle.verify_polygons(doc, batch=BATCH)
    iou = (6 * 6) / (6 * 8)
    good = {'id': 1, 'label': 7, 'frames': 4, 'differ': 0, 'min_iou': 1.0, 'mean_iou': 1.0}
    moved = {'id': 2, 'label': 3, 'frames': 4, 'differ': 1, 'min_iou': iou, 'mean_iou': float(np.mean([1.0, 1.0, iou, 1.0]))}
    assert report == {'tolerance': 0, 'fill': 'evenodd', 'tracks': [good, moved], 'frames': 4, 'differ': 1}


# ---- counts_from_polygons ---------------------------------------------------------------------------------------------------------------
def _counts_back(twin):
    """what `counts_from_polygons` has to give for `twin`, by `fill_rows_host` and `encode_host`"""
    want = json.loads(json.dumps(twin))
    anns = want['annotations']
    for ann in anns:
        ann['bboxes'] = [None] * T
        ann['areas'] = [None] * T
    for t in range(T):
        rows = [([] if ann['segmentations'][t] is None else ann['segmentations'][t]['polygons']) for ann in anns]
        if not any(ann['segmentations'][t] is not None for ann in anns):
            continue
        dense = P.fill_rows_host(rows, H, W)
        for a, ann in enumerate(anns):
            seg = ann['segmentations'][t]
            if seg is None:
                continue
            r = rle.encode_host(dense, a + 1)
            ann['segmentations'][t] = dict({'size': [H, W], 'counts': r.counts}, polygons=seg['polygons'])
            x0, y0, x1, y1 = r.box
            ann['bboxes'][t] = [x0, y0, x1 - x0 + 1, y1 - y0 + 1] if r.area else [0, 0, 0, 0]
            ann['areas'][t] = r.area
    return want


def test_counts_from_polygons_without_boxes_and_areas_and_with_an_entry_that_holds_no_pixel():
    frames = _clip()
    twin = _twin(_doc(frames, polygons=True))
    assert all('bboxes' not in ann and 'areas' not in ann for ann in twin['annotations'])
    want = _counts_back(twin)
    sliver = want['annotations'][2]
    assert sliver['areas'] == [None, 0, None, None, None] and sliver['bboxes'][1] == [0, 0, 0, 0]
    assert sliver['segmentations'][1]['counts'] == [H * W]
    for t, m in enumerate(frames):                                    # the exact rings give the clip back
        if m is not None:
            assert [ann['areas'][t] for ann in want['annotations'][:2]] == [int((m == 1).sum()), int((m == 2).sum())]
    before = _launches()
    doc = rle.counts_from_polygons(twin, batch=BATCH)
    assert (_launches() - before).tolist() == [math.ceil(4 / BATCH), 0, math.ceil(4 / BATCH)]      # the four polygon frames
    _same(doc, want)
    assert list(doc['annotations'][0]) == ['id', 'video_id', 'category_id', 'label', 'segmentations', 'bboxes', 'areas']
    assert 'bboxes' not in twin['annotations'][0]                     # the document that was passed is left alone


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_main_chains_its_steps_in_order_and_writes_once(tmp_path, capsys):
    frames = _clip()
    twin = _twin(_doc(frames, polygons=True))
    src, out = tmp_path / 'twin.json', tmp_path / 'made' / 'out.json'
    src.write_text(json.dumps(twin))
    before = _launches()
    assert rle.main(['--tracks', str(src), '--from-polygons', '--clean', json.dumps({'min_area': 3, 'max_hole': 4}), '--grow', '1',
                     '--polygons', '--recode', 'compressed', '--out', str(out)]) == 0
    assert (_launches() - before).tolist() == [3, 1, 1]               # one batch each: from-polygons fills and encodes, clean and grow encode
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    text = out.read_text()
    cleaned, totals = _cleaned(frames)
    assert list(report) == ['from_polygons', 'clean', 'grow', 'polygons', 'recode', 'bytes', 'out']
    assert report == {'from_polygons': True, 'clean': totals, 'grow': 1.0, 'polygons': {'tolerance': 0.0, 'fill': 'evenodd'},
                      'recode': 'compressed', 'bytes': len(text), 'out': str(out)}
    assert list(report['clean']) == list(STATS)
    # the functions, in that order
    doc = rle.counts_from_polygons(twin)
    doc, _ = rle.clean_tracks(doc, SPEC)
    doc = rle.recode_tracks(rle.polygon_tracks(rle.grow_tracks(doc, 1.0), {'tolerance': 0.0}), 'compressed')
    assert text == json.dumps(doc, separators=(',', ':'))
    # and the host definitions, in that order
    grown, order = _grown(cleaned, 1.0)
    _same(json.loads(text), _doc(grown, labels=order, counts='compressed', polygons={'tolerance': 0.0}))
