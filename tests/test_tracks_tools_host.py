"""Host tests of the shared pieces behind `python -m xmem2_amd.rle` (xmem2_amd/rle.py, `matte.matte_tracks`):

1. `pack_rows`, which lets one `ops.fill_polygons` serve a batch of frames: literal rows and values for both width rules (a track's
   widest row list, or at least one row per track) and both fill rules, a track without a polygon in the batch, the all-empty batch;
2. `read_tracks` gives what `TrackReader.mask_host` gives on the chair tracks, on overlapping tracks with a null frame, on a
   compressed file and on a polygon-only file, and every refusal the two share has one type and one text.  The two are NOT one loop:
   `read_tracks` reads a counts file whose video names a fill rule nobody knows (it never fills), `TrackReader` refuses it, and a
   track without `bboxes` is a KeyError in the one and a ValueError in the other - both are pinned here;
3. the five tools that need one track per label say so, by name, before any device work;
4. `batches`; 5. `TrackWriter.open_track`."""
import json
import re

import numpy as np
import pytest

import polygons_fill_refs as R
from test_rle_decode_host import _chair_tracks, _overlap_doc


# ---- 1. the row packer ------------------------------------------------------------------------------------------------------------
R1, R2, R3, R4, R5, R6 = ([i, 0, i + 4, 0, i + 4, 3] for i in range(6))
RINGS_OF = [[[R1, R2], None], [None, None], [[R3], [R4, R5, R6]]]     # [track][frame]: the second track has no polygon in the batch


def test_pack_rows_evenodd_gives_one_row_per_entry():
    from xmem2_amd.rle import pack_rows
    assert pack_rows(RINGS_OF, [9, 8, 7], 'evenodd') == ([[[R1, R2], [R3]], [[], [R4, R5, R6]]], [9, 7])
    assert pack_rows(RINGS_OF, [9, 8, 7], 'evenodd', least=1) == ([[[R1, R2], [], [R3]], [[], [], [R4, R5, R6]]], [9, 8, 7])


def test_pack_rows_union_gives_one_row_per_ring_padded_to_the_widest_frame():
    from xmem2_amd.rle import pack_rows
    assert pack_rows(RINGS_OF, [9, 8, 7], 'union') == ([[[R1], [R2], [R3], [], []], [[], [], [R4], [R5], [R6]]], [9, 9, 7, 7, 7])
    assert pack_rows(RINGS_OF, [9, 8, 7], 'union', least=1) == ([[[R1], [R2], [], [R3], [], []], [[], [], [], [R4], [R5], [R6]]],
                                                                 [9, 9, 8, 7, 7, 7])


@pytest.mark.parametrize('fill', ('evenodd', 'union'))
def test_pack_rows_of_a_batch_without_any_polygon_still_has_a_row(fill):
    from xmem2_amd.rle import pack_rows
    nothing = [[None, None, None], [None, None, None]]
    assert pack_rows(nothing, [4, 5], fill) == ([[[]], [[]], [[]]], [4])          # the first track's slot, widened to one row
    assert pack_rows(nothing, [4, 5], fill, least=1) == ([[[], []], [[], []], [[], []]], [4, 5])
    assert pack_rows([[[]]], [4], fill, least=1) == ([[[]]], [4])     # an entry with no ring: one row without a ring under either rule


# ---- 2. read_tracks and TrackReader -------------------------------------------------------------------------------------------------
def _agree(path_or_doc, tmp_path):
    from xmem2_amd import rle
    if isinstance(path_or_doc, dict):
        path = tmp_path / 'doc.json'
        path.write_text(json.dumps(path_or_doc))
    else:
        path = path_or_doc
    video, masks = rle.read_tracks(path)
    reader = rle.TrackReader(path)
    assert video == reader.video and len(masks) == len(reader)
    for t, m in enumerate(masks):
        got = reader.mask_host(t)
        assert (m is None) == (got is None) == (not reader.has_mask(t))
        if m is not None:
            assert m.dtype == got.dtype == np.uint8
            np.testing.assert_array_equal(m, got)
    return masks


def test_read_tracks_is_mask_host_on_the_chair_tracks(tmp_path):
    path, _, maps = _chair_tracks(tmp_path / 'tracks.json', skip=(4,))
    masks = _agree(path, tmp_path)
    assert masks[4] is None
    np.testing.assert_array_equal(masks[7], maps[7])


def test_read_tracks_is_mask_host_on_overlapping_tracks_compressed_and_polygon_only_files(tmp_path):
    from xmem2_amd import rle
    doc, _ = _overlap_doc()
    masks = _agree(doc, tmp_path)
    assert masks[1] is None and set(np.unique(masks[0])) == {0, 9, 200}
    comp = _agree(rle.recode_tracks(doc, 'compressed'), tmp_path)
    np.testing.assert_array_equal(comp[0], masks[0])
    exact = R.counts_doc()
    want = _agree(exact, tmp_path)
    got = _agree(R.twin(exact), tmp_path)                             # polygon-only: filled on the host
    assert got[2] is None
    for t in (0, 1, 3, 4):
        np.testing.assert_array_equal(got[t], want[t])


def _refused(tmp_path, doc, text, read=True):
    """both say `text`, as a ValueError and nothing more special; `read`: whether the reader has to read frame 0 to see it"""
    from xmem2_amd import rle
    path = tmp_path / 'bad.json'
    path.write_text(json.dumps(doc))
    for attempt in (lambda: rle.read_tracks(path), (lambda: rle.TrackReader(path).mask_host(0)) if read else (lambda: rle.TrackReader(path))):
        with pytest.raises(ValueError, match='^' + re.escape(text) + '$') as e:
            attempt()
        assert type(e.value) is ValueError


def test_read_tracks_and_track_reader_refuse_in_the_same_words(tmp_path):
    doc, _ = _overlap_doc()

    def spoiled():
        return json.loads(json.dumps(doc))
    _refused(tmp_path, dict(doc, videos=doc['videos'] * 2), 'read_tracks: expected one video per file', read=False)
    _refused(tmp_path, dict(doc, videos=[]), 'read_tracks: expected one video per file', read=False)
    bad = spoiled()
    bad['annotations'][0]['label'] = 256
    _refused(tmp_path, bad, 'read_tracks: label 256 does not fit an index PNG', read=False)
    bad = spoiled()
    bad['annotations'][2]['label'] = 0
    _refused(tmp_path, bad, 'read_tracks: label 0 does not fit an index PNG', read=False)
    for key in ('segmentations', 'bboxes', 'areas'):
        bad = spoiled()
        bad['annotations'][1][key] = bad['annotations'][1][key][:2]
        _refused(tmp_path, bad, 'read_tracks: track 2 does not have one entry per frame', read=False)
    bad = spoiled()
    bad['annotations'][2]['segmentations'][0]['size'] = [4, 5]
    _refused(tmp_path, bad, "read_tracks: track 3, frame 0: size [4, 5] is not the video's [5, 4]", read=False)
    bad = spoiled()
    bad['annotations'][0]['segmentations'][0]['counts'] = [3, 3]
    _refused(tmp_path, bad, 'decode: counts do not describe a 5 x 4 plane')
    bad = spoiled()
    bad['annotations'][0]['segmentations'][0]['counts'] = 'P'          # a continuation bit and nothing after it
    _refused(tmp_path, bad, 'decompress_counts: the string ends inside a value')
    # a polygon-only entry: `read_tracks` hands the file to the reader
    twin = R.twin(R.counts_doc())
    bad = json.loads(json.dumps(twin))
    bad['videos'][0]['polygons']['fill'] = 'nonzero'
    _refused(tmp_path, bad, "read_tracks: polygons.fill = 'nonzero', known: ('evenodd', 'union')", read=False)
    bad = json.loads(json.dumps(twin))
    bad['annotations'][0]['segmentations'][0]['size'] = [33, 64]
    _refused(tmp_path, bad, "read_tracks: track 1, frame 0: size [33, 64] is not the video's [33, 65]", read=False)
    bad = json.loads(json.dumps(twin))
    bad['annotations'][0]['bboxes'] = [None]
    _refused(tmp_path, bad, 'read_tracks: track 1 does not have one entry per frame', read=False)
    bad = json.loads(json.dumps(twin))
    bad['annotations'][1]['segmentations'][0] = {'size': [33, 65], 'counts': [33 * 65]}
    _refused(tmp_path, bad, 'TrackReader: frame 0 mixes polygon-only entries with counts entries; the two forms are not layered')


def test_where_read_tracks_and_track_reader_differ(tmp_path):
    """Why `read_tracks` keeps its own loop: it reads a counts file whatever fill rule the video names, and the reader does not."""
    from xmem2_amd import rle
    doc = R.counts_doc()                                              # counts and polygons in every entry: read from the counts
    want = [rle.TrackReader(doc).mask_host(t) for t in range(5)]
    doc['videos'][0]['polygons']['fill'] = 'nonzero'
    path = tmp_path / 'fill.json'
    path.write_text(json.dumps(doc))
    _, masks = rle.read_tracks(path)
    for t in (0, 1, 3, 4):
        np.testing.assert_array_equal(masks[t], want[t])
    with pytest.raises(ValueError, match=re.escape("read_tracks: polygons.fill = 'nonzero', known: ('evenodd', 'union')")):
        rle.TrackReader(path)
    doc, _ = _overlap_doc()
    del doc['annotations'][1]['bboxes']
    path.write_text(json.dumps(doc))
    with pytest.raises(KeyError, match='bboxes'):
        rle.read_tracks(path)
    with pytest.raises(ValueError, match='^' + re.escape('read_tracks: track 2 does not have one entry per frame') + '$'):
        rle.TrackReader(path)


# ---- 3. one track per label -----------------------------------------------------------------------------------------------------
def test_the_tools_refuse_two_tracks_with_one_label_by_their_own_name(tmp_path, monkeypatch):
    from xmem2_amd import matte, rle
    from xmem2_amd.mask_cleanup import parse_cleanup
    doc, _ = _overlap_doc()                                           # the labels 9, 200, 9
    path = tmp_path / 'twice.json'
    path.write_text(json.dumps(doc))

    def no_device(*a, **k):
        raise AssertionError('the refusal comes before any device work')
    monkeypatch.setattr(rle.TrackReader, 'masks_device', no_device)
    calls = {'clean_tracks': lambda d: rle.clean_tracks(d, parse_cleanup({'min_area': 2}), batch=2),
             'grow_tracks': lambda d: rle.grow_tracks(d, 1, batch=2),
             'polygon_tracks': lambda d: rle.polygon_tracks(d, True, batch=2),
             'counts_from_polygons': lambda d: rle.counts_from_polygons(d, batch=2),
             'matte_tracks': lambda d: matte.matte_tracks(d, tmp_path / 'mattes', matte.parse_mattes(True), batch=2)}
    for name, call in calls.items():
        for given in (doc, str(path)):
            with pytest.raises(ValueError, match='^' + re.escape(f'{name}: two tracks share a label') + '$') as e:
                call(given)
            assert type(e.value) is ValueError
    assert not (tmp_path / 'mattes').exists()


# ---- 4. the batch iterator --------------------------------------------------------------------------------------------------------
def test_batches():
    from xmem2_amd.rle import batches
    assert list(batches(range(0), 4)) == []
    assert list(batches(range(3), 4)) == [[0, 1, 2]]
    assert list(batches(range(6), 3)) == [[0, 1, 2], [3, 4, 5]]
    assert list(batches(range(5), 2)) == [[0, 1], [2, 3], [4]]
    assert list(batches([7, 3, 9], 2)) == [[7, 3], [9]]               # any sequence of frames, not only 0..n-1
    for step in (0, -3):
        assert list(batches(range(3), step)) == [[0], [1], [2]]       # clamped to 1
    assert list(batches(range(4), 2.9)) == [[0, 1], [2, 3]]           # int(), as the loops always took it
    assert all(type(b) is list for b in batches(range(5), 2))


# ---- 5. a track without any entry -------------------------------------------------------------------------------------------------
def test_open_track_is_what_the_private_poke_was():
    from xmem2_amd.rle import TrackWriter
    m = np.zeros((5, 4), np.uint8)
    m[1:3, 1:3] = 1

    def written(open_track):
        w = TrackWriter(5, 4)
        open_track(w, 8)                                              # before any frame: the first annotation
        w.add_mask('a.png', m, k=1, labels=[5])
        w.add_mask('b.png', None)
        open_track(w, 5)                                              # a track that is open keeps its entries and its place
        open_track(w, 2)
        return w.to_dict()
    doc = written(lambda w, lab: w.open_track(lab))
    assert doc == written(lambda w, lab: w._tracks.setdefault(lab, {}))
    assert [(a['id'], a['label']) for a in doc['annotations']] == [(1, 8), (2, 5), (3, 2)]
    assert doc['annotations'][0]['segmentations'] == [None, None] == doc['annotations'][2]['areas']
    assert doc['annotations'][1]['areas'] == [4, None] and doc['annotations'][1]['bboxes'] == [[1, 1, 2, 2], None]
