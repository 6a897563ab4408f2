"""GPU tests of reading tracks.json back (csrc/rle.hip `xmem_rle_decode`, ops.rle_decode, rle.TrackReader.masks_device, J&F from
tracks, tracks as annotations, VideoSession.load_tracks):

1. the kernel against the numpy specification `rle.decode`, exactly: tile-edge shapes, K in {1, 3, 254} with most rows empty, the
   patterns that sit on the order's edges, batches with a frame without entry, exact and larger capacity, overlapping rows, a value
   table, the device round trip through `rle_encode`, the status of a frame that does not fit;
2. `compute_metrics` from tracks equals `compute_metrics` from PNGs of the same predictions and opens no prediction image;
3. `run_on_video` with a tracks file as annotations equals the run with the PNG directory the file was made from;
4. `VideoSession.load_tracks` restores what `save_tracks` wrote."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_rle import _chair, _write_clip, checkpoint, net      # noqa: F401  (the fixtures and clips of the encoder's tests)

pytestmark = pytest.mark.gpu
CHAIR = os.path.join(GOLDEN, 'chair')
CHAIR_ANN = os.path.join(CHAIR, 'Annotations')
SHAPES = [(1, 1), (1, 7), (5, 1), (5, 3), (33, 16), (64, 64), (67, 130)]
KS = (1, 3, 254)


# ---- 1. the kernel against the specification ------------------------------------------------------------------------------
def _want(meta, events, H, W, values=None):
    """One frame by the specification: `rle.decode` of every row's counts, rows in ascending order, the later one wins."""
    from xmem2_amd import rle
    out = np.zeros((H, W), np.uint8)
    for k, ev in enumerate(rle.label_events(meta, events)):
        if len(ev):
            out[rle.decode(rle.counts_from_events(ev, H, W), H, W)] = (k + 1) if values is None else values[k]
    return out


def _records(maps, K):
    """(meta [B, K, META], list of packed events) of label maps: `rle.record_host`, encoding only the labels a map holds."""
    from xmem2_amd import rle
    meta, events = np.zeros((len(maps), K, rle.META), np.int32), []
    for b, m in enumerate(maps):
        ev = [np.zeros(0, np.uint32)]
        for lab in np.unique(m):                                      # ascending, as the rows are packed
            if 1 <= lab <= K:
                r = rle.encode_host(m, int(lab))
                meta[b, lab - 1] = (len(r.events), r.area) + tuple(r.box)
                ev.append(r.events)
        events.append(np.concatenate(ev))
    return meta, events


def _patterns(H, W, K, rng):
    """The label maps of the issue's patterns, with the labels 1, (K + 1) // 2 and K only: most rows of the record stay empty."""
    lo, mid, hi = 1, (K + 1) // 2, K
    zero = np.zeros((H, W), np.uint8)
    full = np.full((H, W), hi, np.uint8)                              # events = [0]
    first, last, cols = zero.copy(), zero.copy(), zero.copy()
    first[0, 0] = lo
    last[-1, -1] = hi                                                 # an odd number of events, the event H * W - 1
    cols[:, 2:4] = mid                                                # one run across the column boundary (nothing when W < 3)
    yy, xx = np.mgrid[:H, :W]
    board = np.where((yy + xx) & 1, lo, hi if K > 1 else 0).astype(np.uint8)      # an event at almost every pixel
    blobs = np.repeat(np.repeat(rng.choice([0, lo, mid, hi], size=(-(-H // 5), -(-W // 3))), 5, 0), 3, 1)[:H, :W].astype(np.uint8)
    return [zero, full, first, last, cols, board, blobs]


def _decode_and_compare(meta, events, H, W, K, capacity=None, values=None):
    from xmem2_amd import ops
    got = ops.rle_decode((meta, events), H, W, K, capacity, values=values)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (len(events), H, W)
    got = got.cpu().numpy()
    for b in range(len(events)):
        np.testing.assert_array_equal(got[b], _want(meta[b], events[b], H, W, values), err_msg=f'frame {b}, {H} x {W}, K {K}')
    return got


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_the_specification_on_the_patterns(shape):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    for K in KS:
        maps = _patterns(H, W, K, rng)
        meta, events = _records(maps, K)
        assert events[1].tolist() == [0] and events[3].tolist() == [H * W - 1]
        largest = max(len(e) for e in events)
        for capacity in (max(1, largest), largest + 17):              # exactly the largest frame's total, and larger
            got = _decode_and_compare(meta, events, H, W, K, capacity)
            np.testing.assert_array_equal(got, np.stack(maps))        # the maps the records were made from
        one = _decode_and_compare(meta[5:6], events[5:6], H, W, K)    # N = 1, the capacity the frame needs
        np.testing.assert_array_equal(one[0], maps[5])


def test_kernel_on_a_chair_frame():
    from PIL import Image
    chair = np.array(Image.open(os.path.join(CHAIR_ANN, 'frame_000000.png')).convert('P'), np.uint8)
    assert chair.shape == (480, 720)
    for K in KS:
        m = chair.copy()
        m[m == 1] = K
        m[:200][m[:200] == K] = (K + 1) // 2
        m[:, 700:] = 1
        meta, events = _records([m, chair], K)
        got = _decode_and_compare(meta, events, 480, 720, K)
        np.testing.assert_array_equal(got, np.stack([m, chair]))


def test_a_batch_of_33_with_a_frame_without_entry():
    rng = np.random.default_rng(33)
    H, W, K = 67, 130, 3
    maps = [_patterns(H, W, K, rng)[-1] for _ in range(33)]
    maps[17] = np.zeros((H, W), np.uint8)
    meta, events = _records(maps, K)
    assert not meta[17].any() and len(events[17]) == 0
    got = _decode_and_compare(meta, events, H, W, K)
    np.testing.assert_array_equal(got, np.stack(maps))
    assert not got[17].any() and got[16].any() and got[18].any()


@pytest.mark.parametrize('shape', [(5, 3), (33, 16), (67, 130)])
def test_the_higher_row_wins_and_values_are_applied(shape):
    from xmem2_amd import rle
    H, W = shape
    a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    a[1:H - 1, 0:W - 1] = 1
    b[H // 2:, W // 2:] = 1
    ea, eb = rle.encode_host(a, 1).events, rle.encode_host(b, 1).events
    meta = np.zeros((1, 3, rle.META), np.int32)
    meta[0, :, 0] = len(ea), len(ea), len(eb)                        # rows 1 and 2 over one rectangle, row 3 across them
    events = [np.concatenate([ea, ea, eb])]
    plain = _decode_and_compare(meta, events, H, W, 3)[0]
    want = np.zeros(shape, np.uint8)
    want[a == 1] = 2
    want[b == 1] = 3
    np.testing.assert_array_equal(plain, want)
    table = np.array([255, 9, 9], np.uint8)                           # 255 and a duplicate
    mapped = _decode_and_compare(meta, events, H, W, 3, values=table)[0]
    np.testing.assert_array_equal(mapped, np.where(want > 0, 9, 0))
    lone = _decode_and_compare(meta[:, :1], [ea], H, W, 1, values=np.array([255], np.uint8))[0]
    np.testing.assert_array_equal(lone, a * 255)


@pytest.mark.parametrize('shape', [(5, 3), (64, 64), (67, 130)])
def test_device_round_trip_needs_no_host_step(shape, monkeypatch):
    from xmem2_amd import ops
    H, W = shape
    rng = np.random.default_rng(7)
    m = torch.from_numpy(rng.integers(0, 6, size=(3, H, W)).astype(np.uint8)).cuda()
    K, cap = 3, 2 * 3 * H * W
    rec = ops.rle_encode(m, K, cap, wait=False)
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: pytest.fail('the device record must not be copied to the host'))
    got, status = ops.rle_decode(rec, H, W, K, cap, check=False)
    monkeypatch.undo()
    assert status.cpu().tolist() == [0, 0, 0]
    want = m.cpu().numpy().copy()
    want[want > K] = 0                                                # labels above K belong to no row
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    out = torch.full((3, H, W), 77, dtype=torch.uint8, device='cuda')
    assert ops.rle_decode(rec, H, W, K, cap, out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_both_store_paths_agree():
    """A map whose rows start on multiples of 4 takes dword stores; the same record into an odd address takes byte stores."""
    from xmem2_amd import ops
    rng = np.random.default_rng(5)
    maps = [_patterns(70, 128, 3, rng)[-1], _patterns(70, 128, 3, rng)[-2]]
    meta, events = _records(maps, 3)
    store = torch.zeros(2 * 70 * 128 + 1, dtype=torch.uint8, device='cuda')
    odd = store[1:].view(2, 70, 128)
    assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    ops.rle_decode((meta, events), 70, 128, 3, out=odd)
    np.testing.assert_array_equal(odd.cpu().numpy(), np.stack(maps))
    assert int(store[0]) == 0
    np.testing.assert_array_equal(ops.rle_decode((meta, events), 70, 128, 3).cpu().numpy(), np.stack(maps))


def test_a_frame_that_does_not_fit_is_zero_with_status_1_and_its_neighbours_are_exact():
    from xmem2_amd import ops
    H, W, K = 33, 16, 3
    rng = np.random.default_rng(3)
    pats = _patterns(H, W, K, rng)
    maps = [pats[-1], pats[5], pats[4]]                               # blobs, the checkerboard (does not fit), two columns
    meta, events = _records(maps, K)
    capacity = max(len(events[0]), len(events[2]))
    assert len(events[1]) > capacity >= 1
    got, status = ops.rle_decode((meta, events), H, W, K, capacity, check=False)
    assert status.dtype == torch.int32 and status.cpu().tolist() == [0, 1, 0]
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got[0], maps[0])
    assert not got[1].any()
    np.testing.assert_array_equal(got[2], maps[2])
    with pytest.raises(RuntimeError, match=r'frame\(s\) \[1\]'):
        ops.rle_decode((meta, events), H, W, K, capacity)
    # the same through the encoder: its meta holds the true counts of a frame it could not write completely
    dev = torch.from_numpy(np.stack(maps)).cuda()
    rec = ops.rle_encode(dev, K, capacity, wait=False)
    got, status = ops.rle_decode(rec, H, W, K, capacity, check=False)
    assert status.cpu().tolist() == [0, 1, 0] and not got[1].any()
    np.testing.assert_array_equal(got[0].cpu().numpy(), maps[0])
    np.testing.assert_array_equal(got[2].cpu().numpy(), maps[2])


def test_ops_rle_decode_validates():
    from xmem2_amd import ops, rle
    rec = torch.zeros(rle.META + 8, dtype=torch.int32, device='cuda')
    assert not ops.rle_decode(rec, 4, 4, 1, 8).any()
    with pytest.raises(ValueError):
        ops.rle_decode(rec, 4, 4, 1)                                  # a device record without its capacity
    with pytest.raises(ValueError):
        ops.rle_decode(rec, 4, 4, 1, 7)                               # not a whole number of frames
    with pytest.raises(RuntimeError):
        ops.rle_decode(rec.float(), 4, 4, 1, 8)
    with pytest.raises(RuntimeError):
        ops.rle_decode(rec, 4, 4, 1, 8, out=torch.zeros((1, 4, 5), dtype=torch.uint8, device='cuda'))
    for values in ([1, 2], [256], np.array([1.0])):
        with pytest.raises(ValueError):
            ops.rle_decode(rec, 4, 4, 1, 8, values=values)
    with pytest.raises(ValueError):
        ops.rle_decode((np.zeros((2, 1, rle.META), np.int32), [np.zeros(0, np.uint32)]), 4, 4, 1)


def test_track_reader_masks_device():
    from xmem2_amd import rle
    from test_rle_decode_host import _overlap_doc
    doc, _ = _overlap_doc()
    r = rle.TrackReader(doc)
    for batch in (32, 1):
        masks, present = r.masks_device(batch=batch)
        assert masks.is_cuda and masks.dtype == torch.uint8 and tuple(masks.shape) == (3, 5, 4) and present.tolist() == [True, False, True]
        got = masks.cpu().numpy()
        for t in range(3):
            want = r.mask_host(t)
            np.testing.assert_array_equal(got[t], np.zeros((5, 4), np.uint8) if want is None else want)
    dense, _ = r.masks_device(frames=[2, 0], values='dense')
    lut = np.array([0, 9, 200, 9], np.uint8)                          # row -> label: 'dense' writes the row numbers 1..n
    got = dense.cpu().numpy()
    np.testing.assert_array_equal(lut[got[0]], r.mask_host(2))
    np.testing.assert_array_equal(lut[got[1]], r.mask_host(0))
    assert got.max() == 3


# ---- 2. evaluation ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def results(tmp_path_factory):
    """The chair annotations as ground truth and shifted copies with a second label patched in as predictions, written twice: as
    palette PNGs carrying the ground truth's palette and as tracks.json."""
    from PIL import Image
    from xmem2_amd.rle import TrackWriter
    root = tmp_path_factory.mktemp('results')
    (root / 'gt').mkdir()
    os.symlink(CHAIR_ANN, root / 'gt' / 'chair')
    names = sorted(os.listdir(CHAIR_ANN))
    palette = Image.open(os.path.join(CHAIR_ANN, names[0])).getpalette()
    (root / 'png' / 'chair' / 'masks').mkdir(parents=True)
    writer, gt_writer, preds = TrackWriter(480, 720), TrackWriter(480, 720), []
    for i, n in enumerate(names):
        gt = np.array(Image.open(os.path.join(CHAIR_ANN, n)).convert('P'), np.uint8)
        p = np.roll(gt, (3 + i, -5), axis=(0, 1))
        p[10:40, 20:90] = 2
        im = Image.fromarray(p)
        im.putpalette(palette)
        im.save(root / 'png' / 'chair' / 'masks' / n)
        writer.add_mask(n, p)
        gt_writer.add_mask(n, gt)
        preds.append(p)
    writer.write(str(root / 'tracks' / 'chair'))
    gt_writer.write(str(root / 'gt_tracks' / 'chair'))
    return root, names, preds


def test_compute_metrics_from_tracks_equals_from_pngs_and_opens_no_prediction(results, monkeypatch):
    from PIL import Image
    from xmem2_amd import metrics
    root, names, preds = results
    from_png = metrics.compute_metrics(root / 'gt', root / 'png')
    opened, original = [], Image.open

    def spy(fp, *a, **k):
        opened.append(os.path.realpath(str(fp)))
        return original(fp, *a, **k)
    monkeypatch.setattr(Image, 'open', spy)
    monkeypatch.setattr(metrics, '_load_pred', lambda *a, **k: pytest.fail('a prediction was read as a PNG'))
    from_tracks = metrics.compute_metrics(root / 'gt', root / 'tracks')
    assert len(opened) == len(names) and all(p.startswith(os.path.realpath(CHAIR_ANN)) for p in opened)
    assert from_tracks.equals(from_png) and list(from_tracks.index) == ['chair']
    assert 0 < from_tracks['iou'].iloc[0] < 1 and 0 < from_tracks['f'].iloc[0] < 1
    assert metrics.compute_metrics(root / 'gt', root / 'tracks', pred_format='tracks').equals(from_png)
    opened.clear()
    assert metrics.compute_metrics(root / 'gt_tracks', root / 'tracks').equals(from_png)        # the ground truth from tracks too
    assert opened == []


def test_compute_metrics_formats_and_mismatches(results, tmp_path):
    import shutil
    from xmem2_amd import metrics
    from xmem2_amd.rle import TrackWriter
    root, names, preds = results
    with pytest.raises(FileNotFoundError):
        metrics.compute_metrics(root / 'gt', root / 'tracks', pred_format='png')                # no masks/ there
    with pytest.raises(FileNotFoundError):
        metrics.compute_metrics(root / 'gt', root / 'png', pred_format='tracks')                # no tracks.json there
    both = tmp_path / 'both' / 'chair'
    shutil.copytree(root / 'png' / 'chair', both)
    short = TrackWriter(480, 720)
    for n, p in zip(names[:9], preds):
        short.add_mask(n, p)
    short.write(str(both))
    from_png = metrics.compute_metrics(root / 'gt', root / 'png')
    assert metrics.compute_metrics(root / 'gt', tmp_path / 'both').equals(from_png)             # masks/ has files: they are read
    with pytest.raises(ValueError, match='chair'):
        metrics.compute_metrics(root / 'gt', tmp_path / 'both', pred_format='tracks')           # 9 frames for 10
    small = TrackWriter(240, 360)
    for n, p in zip(names, preds):
        small.add_mask(n, p[::2, ::2])
    small.write(str(tmp_path / 'small' / 'chair'))
    with pytest.raises(ValueError, match='chair'):
        metrics.compute_metrics(root / 'gt', tmp_path / 'small')                                # no resampling for tracks


# ---- 3. tracks as annotations -------------------------------------------------------------------------------------------------
def _png_arrays(out_dir):
    from PIL import Image
    d = os.path.join(str(out_dir), 'masks')
    return {n: np.array(Image.open(os.path.join(d, n))) for n in sorted(os.listdir(d))}


def test_run_on_video_with_a_tracks_file_as_annotations(checkpoint, net, tmp_path):
    from PIL import Image
    from xmem2_amd.rle import TrackWriter
    from xmem2_amd.run_on_video import run_on_video
    from xmem2_amd.session import VideoSession
    imgs, msks, names = _chair(tmp_path / 'clip', 5)
    writer = TrackWriter(480, 720)
    for n in names:
        writer.add_mask(n, np.array(Image.open(os.path.join(msks, n[:-4] + '.png')).convert('P'), np.uint8))
    tracks = writer.write(str(tmp_path / 'ann.json'))
    common = dict(frames_with_masks=[0, 3], print_progress=False, save_overlay=False, network=net,
                  overwrite_config={'model': checkpoint, 'save_tracks': True})
    a = run_on_video(imgs, msks, str(tmp_path / 'from_png'), **common)
    b = run_on_video(imgs, tracks, str(tmp_path / 'from_tracks'), **common)
    assert a.equals(b) and list(b['mask_provided']) == [True, False, False, True, False]
    pa, pb = _png_arrays(tmp_path / 'from_png'), _png_arrays(tmp_path / 'from_tracks')
    assert list(pa) == list(pb) == [n[:-4] + '.png' for n in names]
    for n in pa:
        np.testing.assert_array_equal(pa[n], pb[n], err_msg=n)
        assert pa[n].any()
    assert open(tmp_path / 'from_png' / 'tracks.json', 'rb').read() == open(tmp_path / 'from_tracks' / 'tracks.json', 'rb').read()

    with pytest.raises(NotADirectoryError):
        VideoSession(imgs, str(tmp_path / 'nomasks'))
    s = VideoSession(imgs, tracks, overwrite_config={'model': checkpoint}, network=net)
    assert s.reader.tracks is not None and s.frames[4].mask is not None
    assert s.save_reference(0) is False and s.references == [0]


# ---- 4. the session ---------------------------------------------------------------------------------------------------------
def test_session_load_tracks_restores_what_save_tracks_wrote(checkpoint, net, tmp_path):
    from xmem2_amd.session import VideoSession
    imgs, msks, names = _write_clip(tmp_path / 'clip')                # the labels 3 and 7: dense ids differ from the labels
    config = {'model': checkpoint, 'size': -1, 'mem_every': 2}
    s = VideoSession(imgs, msks, overwrite_config=dict(config), network=net)
    s.save_reference(0)
    s.full_propagation()
    path = s.save_tracks(tmp_path / 'first')
    s.save(tmp_path / 'first', save_overlay=False)

    fresh = VideoSession(imgs, msks, overwrite_config=dict(config), network=net)
    assert fresh.load_tracks(path) == list(range(7))
    assert fresh._present == s._present and fresh.mapper.remappings == s.mapper.remappings == {3: 1, 7: 2}
    assert fresh.references == []                                     # references are not touched
    assert torch.equal(fresh.masks, s.masks) and int(fresh.masks.max()) == 2
    for t in range(7):
        assert torch.equal(fresh.mask(t), s.mask(t))
    fresh.save(tmp_path / 'second', save_overlay=False)
    pa, pb = _png_arrays(tmp_path / 'first'), _png_arrays(tmp_path / 'second')
    assert list(pa) == list(pb) and len(pa) == 7
    for n in pa:
        np.testing.assert_array_equal(pa[n], pb[n], err_msg=n)
    again = fresh.save_tracks(tmp_path / 'second')
    assert open(again, 'rb').read() == open(path, 'rb').read()
    assert fresh.stats(compute_jf=True)[['frame', 'J', 'F']].equals(s.stats(compute_jf=True)[['frame', 'J', 'F']])

    doc = json.load(open(path))                                       # frames 2 and 5 without entry: not present, not written
    for ann in doc['annotations']:
        for t in (2, 5):
            ann['segmentations'][t] = ann['bboxes'][t] = ann['areas'][t] = None
    (tmp_path / 'holes').mkdir()
    (tmp_path / 'holes' / 'tracks.json').write_text(json.dumps(doc))
    partial = VideoSession(imgs, None, overwrite_config=dict(config), network=net)
    assert partial.load_tracks(tmp_path / 'holes', batch=3) == [0, 1, 3, 4, 6]      # the directory that holds the file; gaps inside a launch
    assert partial._present == [True, True, False, True, True, False, True]
    for t in range(7):
        want = s.masks[t] if t not in (2, 5) else torch.zeros_like(s.masks[t])
        assert torch.equal(partial.masks[t], want)
    assert partial.mask(2) is None

    for change in (dict(height=95), dict(file_names=names[:-1] + ['other.png']), dict(length=6, file_names=names[:6])):
        bad = json.loads(json.dumps(doc))
        bad['videos'][0].update(change)
        if 'length' in change:
            for ann in bad['annotations']:
                for key in ('segmentations', 'bboxes', 'areas'):
                    ann[key] = ann[key][:6]
        if 'height' in change:
            for ann in bad['annotations']:
                ann['segmentations'] = [None] * 7
        (tmp_path / 'bad.json').write_text(json.dumps(bad))
        before = partial.masks.clone()
        with pytest.raises(ValueError, match='load_tracks'):
            partial.load_tracks(tmp_path / 'bad.json')
        assert torch.equal(partial.masks, before)
