"""Host tests of reading tracks.json back (xmem2_amd/rle.py `events_from_counts` / `TrackReader`, `run_on_video.VideoReader` on a
tracks file, the `xmem_rle_decode` symbol, `evaluate --pred-format`):

1. `events_from_counts` is the inverse of `counts_from_events` and refuses what `decode` refuses;
2. `TrackReader` agrees with `read_tracks` on the chair annotations and on a file with overlapping tracks, a null frame and labels
   that are not 1, 2, ...; its packed record is `record_host`'s;
3. `VideoReader` on a tracks file and on a tracks-only directory yields the masks and the first-mask choice of the PNG directory the
   tracks were made from; a missing path fails as before;
4. the flag, the symbol, the ABI version."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

CHAIR = os.path.join(GOLDEN, 'chair')
CHAIR_ANN = os.path.join(CHAIR, 'Annotations')
SHAPES = [(1, 1), (1, 7), (7, 1), (17, 33), (63, 65)]


def _chair_maps():
    from PIL import Image
    names = sorted(os.listdir(CHAIR_ANN))
    return names, [np.array(Image.open(os.path.join(CHAIR_ANN, n)).convert('P'), np.uint8) for n in names]


def _chair_tracks(path, skip=()):
    """tracks.json of the chair annotations (frames in `skip` without a mask), named like the JPEG frames."""
    from xmem2_amd.rle import TrackWriter
    names, maps = _chair_maps()
    w = TrackWriter(480, 720)
    for i, (n, m) in enumerate(zip(names, maps)):
        w.add_mask(n[:-4] + '.jpg', None if i in skip else m)
    return w.write(str(path)), names, maps


# ---- 1. events_from_counts ----------------------------------------------------------------------------------------------------
def test_events_from_counts_inverts_counts_from_events_on_random_maps():
    from xmem2_amd.rle import counts_from_events, encode_host, events_from_counts
    rng = np.random.default_rng(21)
    for shape in SHAPES:
        h, w = shape
        for density in list(rng.random(12)) + [0.0, 1.0]:
            r = encode_host((rng.random(shape) < density).astype(np.uint8), 1)
            ev = events_from_counts(r.counts, h, w)
            assert ev.dtype == np.uint32
            np.testing.assert_array_equal(ev, r.events)
            assert counts_from_events(ev, h, w) == r.counts
    assert events_from_counts([6], 2, 3).tolist() == [] and events_from_counts([0, 6], 2, 3).tolist() == [0]
    assert events_from_counts([5, 1], 2, 3).tolist() == [5] and events_from_counts([2, 2, 2], 2, 3).tolist() == [2, 4]


@pytest.mark.parametrize('bad', [[], [-1, 7], [2, 0, 4], [3, 2], [3, 4], [0, 0, 6]])
def test_events_from_counts_refuses_what_decode_refuses(bad):
    from xmem2_amd.rle import decode, events_from_counts
    with pytest.raises(ValueError):
        decode(bad, 2, 3)
    with pytest.raises(ValueError):
        events_from_counts(bad, 2, 3)


# ---- 2. TrackReader -----------------------------------------------------------------------------------------------------------
def test_track_reader_agrees_with_read_tracks_on_the_chair_annotations(tmp_path):
    from xmem2_amd import rle
    path, names, maps = _chair_tracks(tmp_path / 'tracks.json', skip=(4,))
    video, want = rle.read_tracks(path)
    r = rle.TrackReader(path)
    assert (r.height, r.width, r.length, len(r)) == (480, 720, 10, 10) and r.file_names == video['file_names'] and r.labels == [1]
    for t in range(10):
        assert r.has_mask(t) == (want[t] is not None) == (t != 4)
        got = r.mask_host(t)
        if t == 4:
            assert got is None
            continue
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want[t])
        np.testing.assert_array_equal(got, maps[t])
        meta, events = r.record(t)                                   # the packed record of a frame is the encoder's
        want_meta, want_events = rle.record_host(maps[t], 1)
        assert meta.shape == (1, rle.META) and meta.dtype == np.int32 and events.dtype == np.uint32
        assert meta[0, 0] == want_meta[0, 0] and 532 <= meta[0, 0] <= 666
        np.testing.assert_array_equal(events, want_events)
    assert r.frame_index('frame_000003') == 3 and r.frame_index('frame_000003.jpg') == 3 and r.frame_index('frame_000003.png') == 3
    assert r.frame_index('nothing') is None
    for bad in (-1, 10, True, 1.0):
        with pytest.raises(IndexError):
            r.has_mask(bad)
    with open(path) as f:
        doc = json.load(f)
    np.testing.assert_array_equal(rle.TrackReader(doc).mask_host(0), want[0])      # the parsed document is taken too


def _overlap_doc():
    """Three tracks with the labels 9, 200, 9 on 5 x 4 planes: frame 0 has overlapping entries, frame 1 none, frame 2 one."""
    from xmem2_amd.rle import encode_host
    h, w = 5, 4
    a, b, c = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    a[0:4, 0:3] = 1
    b[2:5, 1:4] = 1
    c[3:5, 0:2] = 1

    def ann(i, label, planes):
        segs = [None if p is None else {'size': [h, w], 'counts': encode_host(p, 1).counts} for p in planes]
        return {'id': i, 'video_id': 1, 'category_id': 1, 'label': label, 'segmentations': segs,
                'bboxes': [None] * len(planes), 'areas': [None] * len(planes)}
    doc = {'videos': [{'id': 1, 'height': h, 'width': w, 'length': 3, 'file_names': ['a.png', 'b.png', 'c.png']}],
           'categories': [{'id': 1, 'name': 'object'}],
           'annotations': [ann(1, 9, [a, None, None]), ann(2, 200, [b, None, c]), ann(3, 9, [c, None, None])]}
    return doc, (a, b, c)


def test_track_reader_on_overlapping_tracks_a_null_frame_and_sparse_labels(tmp_path):
    from xmem2_amd import rle
    doc, (a, b, c) = _overlap_doc()
    path = tmp_path / 'tracks.json'
    path.write_text(json.dumps(doc))
    _, want = rle.read_tracks(path)
    r = rle.TrackReader(str(path))
    assert r.labels == [9, 200, 9] and [r.has_mask(t) for t in range(3)] == [True, False, True]
    first = np.zeros((5, 4), np.uint8)
    first[a == 1] = 9
    first[b == 1] = 200
    first[c == 1] = 9                                                 # the later annotation wins
    np.testing.assert_array_equal(want[0], first)
    np.testing.assert_array_equal(r.mask_host(0), first)
    assert r.mask_host(1) is None and want[1] is None
    np.testing.assert_array_equal(r.mask_host(2), want[2])
    meta, events = r.record(0)
    assert meta[:, 0].tolist() == [len(rle.encode_host(p, 1).events) for p in (a, b, c)]
    np.testing.assert_array_equal(events, np.concatenate([rle.encode_host(p, 1).events for p in (a, b, c)]))
    meta, events = r.record(1)
    assert not meta.any() and len(events) == 0


def test_track_reader_keeps_the_validation_of_read_tracks(tmp_path):
    from xmem2_amd import rle
    doc, _ = _overlap_doc()

    def both(d, match):
        p = tmp_path / 'bad.json'
        p.write_text(json.dumps(d))
        with pytest.raises(ValueError, match=match):
            rle.read_tracks(p)
        with pytest.raises(ValueError, match=match):
            rle.TrackReader(p)
    both(dict(doc, videos=doc['videos'] * 2), 'one video per file')
    bad = json.loads(json.dumps(doc))
    bad['annotations'][0]['label'] = 256
    both(bad, 'does not fit an index PNG')
    bad = json.loads(json.dumps(doc))
    bad['annotations'][1]['areas'] = [None]
    both(bad, 'one entry per frame')
    bad = json.loads(json.dumps(doc))
    bad['annotations'][2]['segmentations'][0]['size'] = [4, 5]
    both(bad, 'is not the video')
    bad = json.loads(json.dumps(doc))
    bad['annotations'][0]['segmentations'][0]['counts'] = [3, 3]
    p = tmp_path / 'counts.json'
    p.write_text(json.dumps(bad))
    with pytest.raises(ValueError):
        rle.TrackReader(p).mask_host(0)
    with pytest.raises(ValueError):
        rle.TrackReader(p).record(0)


def test_the_converter_keeps_its_output(tmp_path):
    from PIL import Image
    from xmem2_amd import rle
    path, names, maps = _chair_tracks(tmp_path / 'tracks.json', skip=(4,))
    assert rle.main(['--tracks', path, '--out', str(tmp_path / 'png')]) == 0
    for t, n in enumerate(names):
        got = np.array(Image.open(tmp_path / 'png' / n))
        np.testing.assert_array_equal(got, np.zeros_like(maps[t]) if t == 4 else maps[t])


# ---- 3. VideoReader -----------------------------------------------------------------------------------------------------------
def _clip(root, n):
    names = sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages')))[:n]
    imgs = root / 'JPEGImages'
    imgs.mkdir(parents=True)
    for nm in names:
        os.symlink(os.path.join(CHAIR, 'JPEGImages', nm), imgs / nm)
    return str(imgs), names


@pytest.mark.parametrize('use_all_masks', [True, False])
def test_video_reader_on_a_tracks_file_and_a_tracks_only_directory(tmp_path, use_all_masks):
    from xmem2_amd.run_on_video import VideoReader
    from xmem2_amd.scribble import _palette
    imgs, names = _clip(tmp_path / 'clip', 4)
    path, _, maps = _chair_tracks(tmp_path / 'ann' / 'tracks.json')
    ref = VideoReader('', imgs, CHAIR_ANN, use_all_masks=use_all_masks)
    for mask_dir in (path, os.path.dirname(path)):
        r = VideoReader('', imgs, mask_dir, use_all_masks=use_all_masks)
        assert r.tracks is not None and len(r) == len(ref) == 4
        assert r.reference_mask.mode == 'P' and r.reference_mask.getpalette() == _palette()
        for i in range(4):
            a, b = ref[i], r[i]
            assert a.frame == b.frame and a.shape == b.shape
            assert (a.mask is None) == (b.mask is None) == (not use_all_masks and i != 0)
            if a.mask is not None:
                assert b.mask.dtype == np.uint8
                np.testing.assert_array_equal(a.mask, b.mask)
    assert ref.tracks is None


def test_video_reader_first_mask_is_the_first_frame_with_an_entry(tmp_path):
    from xmem2_amd.run_on_video import VideoReader
    imgs, names = _clip(tmp_path / 'clip', 4)
    path, _, maps = _chair_tracks(tmp_path / 'tracks.json', skip=(0, 1))
    r = VideoReader('', imgs, path, use_all_masks=False)
    assert [r[i].mask is None for i in range(4)] == [True, True, False, True]
    np.testing.assert_array_equal(r[2].mask, maps[2])
    r = VideoReader('', imgs, path, use_all_masks=True)
    assert [r[i].mask is None for i in range(4)] == [True, True, False, False]


def test_video_reader_fails_on_a_missing_path_as_before(tmp_path):
    from xmem2_amd.run_on_video import VideoReader
    imgs, _ = _clip(tmp_path / 'clip', 2)
    with pytest.raises(FileNotFoundError):
        VideoReader('', imgs, str(tmp_path / 'nomasks'))
    (tmp_path / 'empty').mkdir()
    with pytest.raises(IndexError):
        VideoReader('', imgs, str(tmp_path / 'empty'))


# ---- 4. the flag and the symbol -----------------------------------------------------------------------------------------------
def test_evaluate_accepts_pred_format():
    from xmem2_amd import evaluate, metrics
    assert evaluate.parse_args(['--gt', 'g', '--pred', 'p']).pred_format == 'auto'
    for fmt in ('auto', 'png', 'tracks'):
        assert evaluate.parse_args(['--gt', 'g', '--pred', 'p', '--pred-format', fmt]).pred_format == fmt
    with pytest.raises(SystemExit):
        evaluate.parse_args(['--gt', 'g', '--pred', 'p', '--pred-format', 'coco'])
    assert metrics.PRED_FORMATS == ('auto', 'png', 'tracks')
    with pytest.raises(ValueError, match='pred_format'):
        metrics.compute_metrics('g', 'p', pred_format='coco')


def test_rle_decode_is_declared_listed_and_exported_and_the_abi_version_stays_5():
    from xmem2_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, 'xmem_rle_decode') and lib.xmem_version() == 5 == _lib.ABI_VERSION


def test_rle_decode_abi_rejects_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib
    lib = _lib.load()
    one = 16                                                          # stands for a non-null pointer: every call returns before using it
    good = dict(meta=one, events=one, N=1, H=8, W=8, K=1, capacity=64, values=None, masks=one, status=one)

    def call(**over):
        a = dict(good, **over)
        return lib.xmem_rle_decode(a['meta'], a['events'], a['N'], a['H'], a['W'], a['K'], a['capacity'], a['values'], a['masks'],
                                   a['status'], None)
    for name in ('meta', 'events', 'masks', 'status'):
        assert call(**{name: None}) == -1
    for over in (dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(K=0), dict(K=255), dict(N=0), dict(capacity=0)):
        assert call(**over) == _lib.UNSUPPORTED, over


def test_ops_rle_decode_validates_before_it_needs_a_device():
    import torch
    from xmem2_amd import ops
    rec = torch.zeros(70, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.rle_decode(rec, 8, 8, 1, 64)
    for bad in (dict(H=0), dict(W=16385), dict(K=255), dict(K=True), dict(capacity=0)):
        a = dict(dict(H=8, W=8, K=1, capacity=64), **bad)
        with pytest.raises(ValueError):
            ops.rle_decode(rec, a['H'], a['W'], a['K'], a['capacity'])
