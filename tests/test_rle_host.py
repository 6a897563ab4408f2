"""Host tests of the run-length track export (xmem2_amd/rle.py, the `xmem_rle_*` symbols, config['save_tracks']):

1. `encode_host` / `decode`, the specification the kernel is tested against: round trips and fixed vectors;
2. `TrackWriter` / `read_tracks` / the converter on the chair annotations and on small maps (null entries, inverted label mapping,
   boxes, areas);
3. the new symbols, the config key, and bad arguments answered without touching the GPU."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

CHAIR_ANN = os.path.join(GOLDEN, 'chair', 'Annotations')
SHAPES = [(1, 1), (1, 7), (7, 1), (17, 33), (63, 65)]


# ---- 1. the specification ---------------------------------------------------------------------------------------------------
def test_encode_decode_round_trip_on_random_planes():
    from xmem2_amd.rle import counts_from_events, decode, encode_host
    rng = np.random.default_rng(11)
    n = 0
    for shape in SHAPES:
        for density in rng.random(24):
            m = (rng.random(shape) < density).astype(np.uint8)
            r = encode_host(m, 1)
            h, w = shape
            assert sum(r.counts) == h * w
            assert len(r.counts) == len(r.events) + 1
            assert all(c > 0 for c in r.counts[1:])
            assert r.counts == counts_from_events(r.events, h, w)
            np.testing.assert_array_equal(decode(r.counts, h, w), m == 1)
            assert r.area == int(m.sum())
            n += 1
    assert n == 120


def test_fixed_vectors():
    from xmem2_amd.rle import EMPTY_BOX, encode_host
    assert encode_host(np.ones((2, 3), np.uint8), 1).counts == [0, 6]
    r = encode_host(np.zeros((2, 3), np.uint8), 1)
    assert r.counts == [6] and r.area == 0 and r.box == EMPTY_BOX and len(r.events) == 0
    yy, xx = np.mgrid[:8, :8]
    assert len(encode_host(((xx + yy) & 1).astype(np.uint8), 1).events) == 56
    wrap = np.zeros((4, 2), np.uint8)                                 # H = 4: the run continues from the bottom of column 0 into column 1
    wrap[2:4, 0] = 1
    wrap[0:2, 1] = 1
    r = encode_host(wrap, 1)
    assert r.counts == [2, 4, 2] and r.events.tolist() == [2, 6] and r.area == 4 and r.box == (0, 0, 1, 3)
    multi = np.array([[0, 2, 2], [5, 5, 2]], np.uint8)                # only the asked label counts; others are background to it
    assert encode_host(multi, 2).counts == [2, 1, 1, 2] and encode_host(multi, 5).counts == [1, 1, 1, 1, 2]
    assert encode_host(multi, 3).counts == [6]


def test_decode_refuses_counts_of_another_plane():
    from xmem2_amd.rle import decode
    for bad in ([5], [2, 0, 4], [], [3, -1, 4]):
        with pytest.raises(ValueError):
            decode(bad, 2, 3)


# ---- 2. the file -------------------------------------------------------------------------------------------------------------
def _chair_annotations():
    from PIL import Image
    names = sorted(os.listdir(CHAIR_ANN))
    return names, [np.array(Image.open(os.path.join(CHAIR_ANN, n)).convert('P'), np.uint8) for n in names]


def test_writer_converter_round_trip_on_the_chair_annotations(tmp_path):
    from PIL import Image
    from xmem2_amd import rle
    names, masks = _chair_annotations()
    w = rle.TrackWriter(*masks[0].shape)
    for n, m in zip(names, masks):
        w.add_mask(n[:-4] + '.jpg', m)
    path = w.write(tmp_path)
    assert path == str(tmp_path / 'tracks.json')
    doc = json.load(open(path))
    assert set(doc) == {'videos', 'categories', 'annotations'}
    assert doc['videos'] == [{'id': 1, 'height': 480, 'width': 720, 'length': len(names), 'file_names': [n[:-4] + '.jpg' for n in names]}]
    assert doc['categories'] == [{'id': 1, 'name': 'object'}]
    (ann,) = doc['annotations']
    assert ann['id'] == 1 and ann['video_id'] == 1 and ann['category_id'] == 1 and ann['label'] == 1
    for t, m in enumerate(masks):
        ys, xs = np.nonzero(m == 1)
        assert ann['areas'][t] == int((m == 1).sum())
        assert ann['bboxes'][t] == [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]
        assert ann['segmentations'][t]['size'] == [480, 720] and sum(ann['segmentations'][t]['counts']) == 480 * 720
    # the way back, through the command line's entry point
    assert rle.main(['--tracks', path, '--out', str(tmp_path / 'png'), '--palette-from', os.path.join(CHAIR_ANN, names[0])]) == 0
    for n, m in zip(names, masks):
        back = Image.open(tmp_path / 'png' / n)
        assert back.mode == 'P' and back.getpalette()[:12] == Image.open(os.path.join(CHAIR_ANN, n)).getpalette()[:12]
        np.testing.assert_array_equal(np.array(back), m)
    video, decoded = rle.read_tracks(path)
    assert video['length'] == len(names)
    for d, m in zip(decoded, masks):
        np.testing.assert_array_equal(d, m)


def test_null_entries_and_inverted_label_mapping(tmp_path):
    """Annotation labels 5 and 9 (dense ids 1 and 2, as MaskMapper numbers them), 9 appearing only from the third frame on; a frame
    without a mask; a frame in which label 5 has no pixel."""
    from xmem2_amd import rle
    from xmem2_amd.mask_mapper import MaskMapper
    mapper = MaskMapper()
    first = np.zeros((6, 5), np.uint8)
    first[1:3, 1:4] = 5
    mapper.convert_mask(first, exhaustive=True)
    assert rle.inverse_labels(mapper, 1) == [5]
    third = first.copy()
    third[4:6, 0:2] = 9
    mapper.convert_mask(third, exhaustive=True)
    assert mapper.remappings == {5: 1, 9: 2} and rle.inverse_labels(mapper, 2) == [5, 9]
    dense = lambda raw: np.select([raw == 5, raw == 9], [1, 2], 0).astype(np.uint8)
    only9 = np.zeros((6, 5), np.uint8)
    only9[5, 4] = 9                                                   # the last pixel of the order
    w = rle.TrackWriter(6, 5)
    w.add_mask('a.jpg', dense(first), k=1, labels=[5])
    w.add_mask('b.jpg', None)
    w.add_mask('c.jpg', dense(third), k=2, labels=[5, 9])
    w.add_mask('d.jpg', dense(only9), k=2, labels=[5, 9])
    doc = w.to_dict()
    a5, a9 = doc['annotations']
    assert (a5['label'], a9['label']) == (5, 9) and (a5['id'], a9['id']) == (1, 2)
    assert [s is None for s in a5['segmentations']] == [False, True, False, True]
    assert [s is None for s in a9['segmentations']] == [True, True, False, False]
    for ann in (a5, a9):
        for seg, box, area in zip(ann['segmentations'], ann['bboxes'], ann['areas']):
            assert (seg is None) == (box is None) == (area is None)
    assert a5['bboxes'][0] == [1, 1, 3, 2] and a5['areas'][0] == 6
    assert a9['bboxes'][2] == [0, 4, 2, 2] and a9['areas'][2] == 4
    assert a9['bboxes'][3] == [4, 5, 1, 1] and a9['areas'][3] == 1 and a9['segmentations'][3]['counts'] == [29, 1]
    path = w.write(tmp_path / 'out' / 'tracks.json')
    _, decoded = rle.read_tracks(path)
    np.testing.assert_array_equal(decoded[0], first)
    assert decoded[1] is None
    np.testing.assert_array_equal(decoded[2], third)
    np.testing.assert_array_equal(decoded[3], only9)
    written = rle.tracks_to_pngs(path, tmp_path / 'png')              # no palette: mode L, the label values
    assert [os.path.basename(p) for p in written] == ['a.png', 'b.png', 'c.png', 'd.png']
    from PIL import Image
    np.testing.assert_array_equal(np.array(Image.open(written[2])), third)
    assert not np.array(Image.open(written[1])).any()


def test_label_events_refuses_a_truncated_frame():
    from xmem2_amd import rle
    yy, xx = np.mgrid[:8, :8]
    meta, events = rle.record_host(((xx + yy) & 1).astype(np.uint8), 1)
    assert meta[0, 0] == 56 and len(rle.label_events(meta, events)[0]) == 56
    with pytest.raises(ValueError):
        rle.label_events(meta, events[:16])
    assert rle.default_capacity(480, 720) == 2880 and rle.default_capacity(64, 64) == rle.MIN_CAPACITY


# ---- 3. symbols, config, bad arguments --------------------------------------------------------------------------------------
def test_rle_symbols_are_declared_listed_and_exported_and_the_abi_version_stays_5():
    from xmem2_amd import _lib, build, rle
    assert 5 == _lib.ABI_VERSION and _lib.RLE_META == rle.META and 'rle.hip' in build.SOURCES
    lib = _lib.load()
    assert hasattr(lib, 'xmem_rle_encode') and hasattr(lib, 'xmem_rle_workspace_bytes') and lib.xmem_version() == 5


def test_save_tracks_is_off_by_default():
    from xmem2_amd.configuration import VIDEO_INFERENCE_CONFIG
    assert VIDEO_INFERENCE_CONFIG['save_tracks'] is False


def test_rle_abi_rejects_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib
    lib = _lib.load()
    one = 16                                                          # stands for a non-null pointer: every call returns before using it
    assert lib.xmem_rle_encode(None, 1, 8, 8, 1, 64, one, one, one, 1 << 20, None) == -1
    assert lib.xmem_rle_encode(one, 1, 8, 8, 1, 64, None, one, one, 1 << 20, None) == -1
    assert lib.xmem_rle_encode(one, 1, 8, 8, 1, 64, one, None, one, 1 << 20, None) == -1
    assert lib.xmem_rle_encode(one, 1, 8, 8, 1, 64, one, one, None, 1 << 20, None) == -1
    for k in (0, -1, 255):
        assert lib.xmem_rle_encode(one, 1, 8, 8, k, 64, one, one, one, 1 << 20, None) == -1
        assert lib.xmem_rle_workspace_bytes(1, 8, k) == 0
    assert lib.xmem_rle_encode(one, 0, 8, 8, 1, 64, one, one, one, 1 << 20, None) == -1
    assert lib.xmem_rle_encode(one, 1, 0, 8, 1, 64, one, one, one, 1 << 20, None) == -1
    assert lib.xmem_rle_encode(one, 1, 8, 8, 1, 0, one, one, one, 1 << 20, None) == -1
    assert lib.xmem_rle_encode(one, 1, 16385, 8, 1, 64, one, one, one, 1 << 20, None) == _lib.UNSUPPORTED
    assert lib.xmem_rle_encode(one, 1, 8, 16385, 1, 64, one, one, one, 1 << 30, None) == _lib.UNSUPPORTED
    assert lib.xmem_rle_workspace_bytes(1, 16385, 1) == 0
    assert lib.xmem_rle_encode(one, 1, 8, 8, 1, 64, one, one, one, 16, None) == -3      # workspace too small
    assert lib.xmem_rle_workspace_bytes(3, 720, 5) == 3 * 5 * 720 * 4


def test_ops_rle_encode_has_no_cpu_path():
    import torch
    from xmem2_amd import ops
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.rle_encode(torch.zeros(4, 4, dtype=torch.uint8), 1)
