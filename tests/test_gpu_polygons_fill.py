"""GPU tests of the polygon fill (csrc/polygons_fill.hip, ops.fill_polygons / ops.fill_edges) and of what reads polygons through it.
Every fill is compared with `polygons.fill_rows_host` byte for byte, lands inside sentinel-guarded buffers at a 16-byte aligned and
at an odd address (the 16-byte, dword and byte stores), and runs twice: the bytes are the same.

1. sizes: widths at the bit-word seams, one to 33 rows, lines longer than one pass of the wave, an edge taller than any workgroup;
2. content: exact and simplified rings of random masks, random fractional polygons with the awkward cases, frac_bits 0 and 8, 254 rows;
3. rows, values, overlay, more than 254 rows and frames in chunks under a forced workspace cap;
4. skipped edges and the status, argument handling through the C ABI, capture and replay, the round trip through `ops.mask_polygons`;
5. `TrackReader.masks_device` on a polygon-only file, `--verify-polygons` and `--from-polygons`."""
import ctypes
import json

import numpy as np
import pytest
import torch

import polygons_fill_refs as R
from test_gpu_rle import _write_clip, checkpoint, net      # noqa: F401  (the fixtures and the clip of the encoder's tests)
from xmem2_amd import ops
from xmem2_amd import polygons as P
from xmem2_amd import rle

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def _guarded(N, H, W, guard, fill=None):
    """(buffer, view [N,H,W] at offset `guard`): the bytes around the view hold SENTINEL"""
    buf = torch.full((N * H * W + 2 * guard,), SENTINEL, dtype=torch.uint8, device='cuda')
    view = buf[guard:guard + N * H * W].view(N, H, W)
    if fill is not None:
        view.copy_(torch.from_numpy(fill).cuda())
    return buf, view


def _guards_hold(buf, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[-guard:] == SENTINEL).all())


def _reference(frames, H, W, values, frac_bits, base=None):
    R_ = max(1, max(len(rows) for rows in frames))
    v = list(range(1, R_ + 1)) if values is None else list(values)
    return np.stack([P.fill_rows_host(rows, H, W, values=v[:len(rows)], frac_bits=frac_bits, base=None if base is None else base[i])
                     for i, rows in enumerate(frames)])


def _check(frames, H, W, values=None, frac_bits=8, want=None):
    want = _reference(frames, H, W, values, frac_bits) if want is None else want
    outs = []
    for guard in (64, 67):
        buf, view = _guarded(len(frames), H, W, guard)
        got = ops.fill_polygons(frames, H, W, values=values, frac_bits=frac_bits, out=view)
        assert got is view and _guards_hold(buf, guard)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])
    again = ops.fill_polygons(frames, H, W, values=values, frac_bits=frac_bits)
    assert again.dtype == torch.uint8 and tuple(again.shape) == (len(frames), H, W) and torch.equal(again, outs[0])
    return want


# ---- sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', (1, 31, 32, 33, 63, 64, 65))
def test_widths_at_the_word_seams(W):
    rng = np.random.default_rng(W)
    for H in (1, 2, 33):
        frames = [[R.random_rings(rng, H, W), R.awkward_rings(H, W)], [R.random_rings(rng, H, W, 5), [[(0, 0), (W, 0), (W, H), (0, H)]]]]
        want = _check(frames, H, W)
        assert (want[1] == 2).all()                                   # the plane's own outline fills it, column W - 1 included


@pytest.mark.parametrize('W', (2047, 2048, 2100))
def test_lines_longer_than_one_pass_of_the_wave(W):
    rng = np.random.default_rng(W)
    span = [[(5.5, 0), (W - 3.25, 0), (W - 3.25, 3), (5.5, 3)]]      # one parity run from word 0 to the last word, across the pass seam
    want = _check([[R.random_rings(rng, 3, W, 6), span], [[[(0, 0), (W, 0), (W, 3), (0, 3)]], R.random_rings(rng, 3, W, 4)]], 3, W)
    assert want[0, 1, 4] != 2 and want[0, 1, 5] == 2 and want[0, 1, W - 4] == 2 and want[0, 1, W - 3] != 2


def test_an_edge_taller_than_a_workgroup():
    tri = [(1.0, -5.0), (7.0, 150.0), (2.0, 310.0)]
    want = _check([[[tri]], [[tri, [(0, 100), (8, 100), (8, 260), (0, 260)]]]], 300, 8)
    assert (want[0] == 1).sum() > 300 and (want[0].any(1)).sum() > 280          # it crosses nearly every row of the plane


# ---- content ----------------------------------------------------------------------------------------------------------------------
def _label_masks():
    rng = np.random.default_rng(11)
    out = []
    for p in (0.55, 0.2, 0.0):
        m = np.zeros((33, 65), np.uint8)
        sel = rng.random((33, 65)) < p
        m[sel] = rng.integers(1, 4, int(sel.sum()))
        out.append(m)
    return out


@pytest.mark.parametrize('frac_bits', (0, 8))
def test_exact_rings_of_random_masks(frac_bits):
    masks = _label_masks()                                            # uneven ring counts, the last frame has none
    frames = [[P.rings_host(m, k) if (m == k).any() else [] for k in (1, 2, 3)] for m in masks]
    assert [sum(len(r) for r in rows) for rows in frames][2] == 0 and sum(len(r) for r in frames[0]) > 100
    _check(frames, 33, 65, frac_bits=frac_bits, want=np.stack(masks))


def test_simplified_rings():
    yy, xx = np.mgrid[:64, :96]
    m = (((yy - 30) ** 2 + (xx - 40) ** 2 <= 26 ** 2) & ~((yy - 28) ** 2 + (xx - 44) ** 2 <= 9 ** 2)).astype(np.uint8)
    frames = [[[P.simplify(r, tol) for r in P.rings_host(m, 1)]] for tol in (0.7, 1.5, 3.0)]
    want = _check(frames, 64, 96)
    for i in range(3):
        np.testing.assert_array_equal(want[i] == 1, P.fill_host(frames[i][0], 64, 96))
    assert (want[2] != m).any() and max(len(r) for r in frames[2][0]) < 40


@pytest.mark.parametrize('frac_bits', (0, 8))
def test_random_fractional_polygons(frac_bits):
    rng = np.random.default_rng(7 + frac_bits)
    for H, W in ((13, 35), (40, 70)):
        frames = [[R.random_rings(rng, H, W, 4), R.awkward_rings(H, W), R.random_rings(rng, H, W, 2)], [R.awkward_rings(H, W)], []]
        _check(frames, H, W, frac_bits=frac_bits)


def test_254_rows_of_one_tiny_ring():
    rows = [[[(2 * (i % 35) + .25, 4 * (i // 35)), (2 * (i % 35) + 2.25, 4 * (i // 35)), (2 * (i % 35) + 1.0, 4 * (i // 35) + 3.5)]] for i in range(254)]
    want = _check([rows, rows[::-1]], 40, 70)
    assert len(np.unique(want[0])) == 255


# ---- rows, values, overlay, chunks ------------------------------------------------------------------------------------------------
def _squares():
    a, b, c = ([[(x, x), (x + 20, x), (x + 20, x + 14), (x, x + 14)]] for x in (2, 9, 16))
    return [[a, b, c], [c, [], a]]


def test_overlapping_rows_and_a_values_table():
    want = _check(_squares(), 33, 65, values=[5, 200, 5])
    assert set(np.unique(want)) == {0, 5, 200} and want[0, 12, 12] == 200 and want[0, 17, 17] == 5 and want[1, 17, 17] == 5


def test_overlay_keeps_what_no_row_covers():
    base = np.random.default_rng(3).integers(0, 256, (2, 33, 65)).astype(np.uint8)
    want = _reference(_squares(), 33, 65, [5, 200, 5], 8, base=base)
    assert (want == base).any() and (want != base).any()
    for guard in (64, 67):
        buf, view = _guarded(2, 33, 65, guard, fill=base)
        ops.fill_polygons(_squares(), 33, 65, values=[5, 200, 5], out=view, overlay=True)
        assert _guards_hold(buf, guard)
        np.testing.assert_array_equal(view.cpu().numpy(), want)


def test_more_than_254_rows_and_frames_in_chunks(monkeypatch):
    rows = [[[(3 * (i % 21) + .5, 2 * (i // 21)), (3 * (i % 21) + 8.5, 2 * (i // 21)), (3 * (i % 21) + 4.0, 2 * (i // 21) + 9.0)]] for i in range(300)]
    values = [(7 * i) % 251 + 1 for i in range(300)]
    frames = [rows, rows[::-1], rows[:100], [], rows[150:]]
    before = ops.FILL_STATS['launches']
    want = _check(frames[:2], 40, 70, values=values)                  # 300 rows: two layers, the second over the first
    assert ops.FILL_STATS['launches'] - before == 3 * 2
    with pytest.raises(ValueError):
        ops.fill_polygons(frames[:2], 40, 70)                         # row + 1 does not fit a byte
    per_plane = 4 * 40 * 3                                            # bytes of one (frame, row) bit-plane: 40 lines of 3 words
    monkeypatch.setattr(ops, 'FILL_WORKSPACE_CAP', 120 * per_plane)   # 120 rows of one frame per call
    before = ops.FILL_STATS['launches']
    chunked = ops.fill_polygons(frames, 40, 70, values=values)
    assert ops.FILL_STATS['launches'] - before == 3 * 5
    np.testing.assert_array_equal(chunked.cpu().numpy(), _reference(frames, 40, 70, values, 8))
    np.testing.assert_array_equal(chunked[:2].cpu().numpy(), want)
    few = _squares() + _squares()[::-1] + _squares()[:1]              # 5 frames of 3 rows, 2 frames per call
    monkeypatch.setattr(ops, 'FILL_WORKSPACE_CAP', 2 * 3 * 4 * 33 * 3)
    before = ops.FILL_STATS['launches']
    chunked = ops.fill_polygons(few, 33, 65, values=[5, 200, 5])
    assert ops.FILL_STATS['launches'] - before == 3
    np.testing.assert_array_equal(chunked.cpu().numpy(), _reference(few, 33, 65, [5, 200, 5], 8))


# ---- safety and errors ------------------------------------------------------------------------------------------------------------
def test_skipped_edges_are_counted_and_touch_nothing():
    frames = _squares()
    edges, plane = P.pack_edges(frames, 3)
    bad_plane = np.array([[0, 0, 256, 2560]], np.int32)
    bad_coord = np.array([[0, 0, (1 << 28) + 1, 2560]], np.int32)
    edges = np.concatenate([bad_plane, edges[:5], bad_coord, edges[5:]])
    plane = np.concatenate([[2 * 3], plane[:5], [1], plane[5:]]).astype(np.int32)
    buf, view = _guarded(2, 33, 65, 64)
    got, status = ops.fill_edges(edges, plane, 2, 33, 65, 3, out=view, check=False)
    assert status.dtype == torch.int32 and status.cpu().tolist() == [1, 1] and _guards_hold(buf, 64)
    np.testing.assert_array_equal(got.cpu().numpy(), _reference(frames, 33, 65, None, 8))
    plane[0] = -1
    assert ops.fill_edges(edges, plane, 2, 33, 65, 3, check=False)[1].cpu().tolist() == [1, 1]
    with pytest.raises(ValueError, match='1 edges name a plane'):
        ops.fill_edges(edges, plane, 2, 33, 65, 3)
    _, status = ops.fill_polygons(frames, 33, 65, check=False)
    assert status.cpu().tolist() == [0, 0]


def test_argument_handling_through_the_c_abi():
    from xmem2_amd import _lib_raster
    lib = _lib_raster.load()
    N, H, W, R_ = 2, 5, 40, 3
    nbytes = lib.xmem_polygons_fill_workspace_bytes(N, H, W, R_)
    assert nbytes >= 4 * N * R_ * H * 2
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    status = torch.full((2,), 9, dtype=torch.int32, device='cuda')
    buf, view = _guarded(N, H, W, 64)
    stream = _lib_raster.stream_ptr()

    def call(E=0, edges=None, plane=None, overlay=0, size=nbytes, values=None):
        return lib.xmem_polygons_fill(edges, plane, E, N, H, W, R_, 8, values, overlay, ctypes.c_void_p(view.data_ptr()),
                                      ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(ws.data_ptr()), size, stream)
    assert call(size=nbytes - 1) == -3 and call(E=1) == -1            # refused on the host: nothing has been written
    torch.cuda.synchronize()
    assert bool((view == SENTINEL).all()) and status.cpu().tolist() == [9, 9]
    assert call(overlay=1) == 0                                       # no edges under overlay: the planes are kept
    torch.cuda.synchronize()
    assert bool((view == SENTINEL).all()) and status.cpu().tolist() == [0, 0]
    assert call() == 0                                                # no edges: the planes are cleared
    torch.cuda.synchronize()
    assert bool((view == 0).all()) and _guards_hold(buf, 64)
    e = torch.tensor([[0, 0, 0, 5 * 256], [30 * 256, 0, 30 * 256, 5 * 256]], dtype=torch.int32, device='cuda')
    p = torch.tensor([4, 4], dtype=torch.int32, device='cuda')         # frame 1, row 1
    table = torch.tensor([11, 12, 13], dtype=torch.uint8, device='cuda')
    assert call(E=2, edges=ctypes.c_void_p(e.data_ptr()), plane=ctypes.c_void_p(p.data_ptr()), values=ctypes.c_void_p(table.data_ptr())) == 0
    torch.cuda.synchronize()
    want = np.zeros((N, H, W), np.uint8)
    want[1, :, :30] = 12
    np.testing.assert_array_equal(view.cpu().numpy(), want)
    assert _guards_hold(buf, 64)


# ---- capture and round trip ---------------------------------------------------------------------------------------------------------
def test_the_call_is_capturable_and_replays_the_same_bytes():
    """No read-back and no host synchronisation inside the call, and every launch goes to the one stream the call is given: what is
    captured is a single chain without parallel branches, and a replay over a spoiled output and status gives the bytes again."""
    from xmem2_amd import _lib_raster
    lib = _lib_raster.load()
    frames = _squares()
    e, p = (torch.from_numpy(a).cuda() for a in P.pack_edges(frames, 3))
    out = torch.empty((2, 33, 65), dtype=torch.uint8, device='cuda')
    status = torch.empty(2, dtype=torch.int32, device='cuda')
    ws = torch.empty(lib.xmem_polygons_fill_workspace_bytes(2, 33, 65, 3), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.xmem_polygons_fill(ctypes.c_void_p(e.data_ptr()), ctypes.c_void_p(p.data_ptr()), len(p), 2, 33, 65, 3, 8, None, 0,
                                    ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                    ws.numel(), _lib_raster.stream_ptr())
    assert rc == 0
    want = _reference(frames, 33, 65, None, 8)
    for spoil in (7, 0):
        out.fill_(spoil)
        status.fill_(5)
        ws.fill_(spoil)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        assert status.cpu().tolist() == [0, 0]


@pytest.mark.parametrize('shape', ((33, 65), (64, 96)), ids=lambda s: f'{s[0]}x{s[1]}')
def test_round_trip_through_the_tracer(shape):
    rng = np.random.default_rng(shape[0])
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    m = np.zeros(shape, np.uint8)                                     # three overlapping blobs with holes, one cut by the border
    for k, (cy, cx, r) in enumerate(((shape[0] // 3, shape[1] // 4, shape[0] // 3), (shape[0] // 2, shape[1] // 2, shape[0] // 4),
                                     (shape[0] - 4, shape[1] - 9, shape[0] // 3)), start=1):
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
    m[rng.random(shape) < 0.04] = 0
    assert sorted(np.unique(m)) == [0, 1, 2, 3]
    d = torch.from_numpy(m).cuda()
    meta, words = ops.mask_polygons(d, 3)
    got = ops.fill_polygons([P.label_rings(meta[0], words[0])], *shape)
    assert torch.equal(got[0], d)


# ---- readers and the command line ---------------------------------------------------------------------------------------------------
def test_track_reader_fills_a_polygon_only_file_on_the_device():
    doc = R.counts_doc()
    a, b = rle.TrackReader(doc), rle.TrackReader(R.twin(doc))
    for values in ('label', 'dense', [9, 0, 250]):
        for batch in (32, 2):
            want, present = a.masks_device(values=values, batch=batch)
            got, present_b = b.masks_device(values=values, batch=batch)
            assert tuple(got.shape) == (5, 33, 65) and present.tolist() == present_b.tolist() == [True, True, False, True, True]
            assert torch.equal(got, want)
    np.testing.assert_array_equal(b.masks_device([3, 0])[0].cpu().numpy(), np.stack([a.mask_host(3), a.mask_host(0)]))
    mixed = json.loads(json.dumps(doc))
    del mixed['annotations'][1]['segmentations'][3]['counts']
    with pytest.raises(ValueError, match='frame 3 mixes'):
        rle.TrackReader(mixed).masks_device()
    # a union file whose entries hold several overlapping rings, next to a counts frame in the same batch
    union = R.twin(doc)
    union['videos'][0]['polygons']['fill'] = 'union'
    union['annotations'][0]['segmentations'][1]['polygons'] = [[0, 0, 20, 0, 20, 14, 0, 14], [9.5, 7, 30, 7, 30, 20.25, 9.5, 20.25]]
    union['annotations'][2]['segmentations'][0] = doc['annotations'][2]['segmentations'][0]
    for seg in (ann['segmentations'][0] for ann in union['annotations'][:2]):
        if seg is not None:
            seg.update(size=[33, 65], counts=[33 * 65])
    r = rle.TrackReader(union)
    got = r.masks_device(batch=3)[0].cpu().numpy()
    for t in (0, 1, 3, 4):
        np.testing.assert_array_equal(got[t], r.mask_host(t))
    assert got[1, 10, 15] != 0 and not r.has_polygons(0) and r.has_polygons(1)


def test_verify_polygons_and_from_polygons(tmp_path, capsys):
    exact = R.counts_doc()
    loose = R.counts_doc({'tolerance': 2.0})
    for name, doc in (('exact', exact), ('loose', loose), ('twin', R.twin(exact))):
        (tmp_path / f'{name}.json').write_text(json.dumps(doc))

    def verify(name):
        code = rle.main(['--tracks', str(tmp_path / f'{name}.json'), '--verify-polygons'])
        return code, json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    code, report = verify('exact')
    assert code == 0 and report['tolerance'] == 0 and report['differ'] == 0 and report['frames'] == 4
    assert [t['label'] for t in report['tracks']] == R.LABELS
    assert all(t['differ'] == 0 and t['min_iou'] == 1.0 == t['mean_iou'] and 1 <= t['frames'] <= 4 for t in report['tracks'])
    code, report = verify('loose')                                    # a tolerance: the cost is reported, the status is 0
    assert code == 0 and report['tolerance'] == 2.0 and report['differ'] > 0
    assert any(t['differ'] > 0 and 0.0 <= t['min_iou'] < 1.0 and t['min_iou'] <= t['mean_iou'] < 1.0 for t in report['tracks'])
    want = rle.TrackReader(loose)                                     # the report's numbers are the host's
    a, t0 = next((a, t) for a, ann in enumerate(loose['annotations']) for t, seg in enumerate(ann['segmentations']) if seg is not None)
    ious = []
    for t, seg in enumerate(loose['annotations'][a]['segmentations']):
        if seg is not None:
            x, y = want.mask_host(t) == R.LABELS[a], None
            filled = np.zeros((33, 65), np.uint8)
            for b, ann in enumerate(loose['annotations']):
                if ann['segmentations'][t] is not None:
                    filled[P.fill_exact_host(ann['segmentations'][t]['polygons'], 33, 65)] = b + 1
            y = filled == a + 1
            ious.append(1.0 if not (x | y).any() else (x & y).sum() / (x | y).sum())
    assert report['tracks'][a]['min_iou'] == pytest.approx(min(ious), abs=1e-12) and report['tracks'][a]['frames'] == len(ious)
    spoiled = json.loads(json.dumps(exact))
    spoiled['annotations'][a]['segmentations'][t0]['polygons'] = [[0, 0, 9, 0, 9, 9]]
    (tmp_path / 'spoiled.json').write_text(json.dumps(spoiled))
    code, report = verify('spoiled')                                  # the file says exact and is not
    assert code == 1 and report['differ'] == 1 and report['tracks'][a]['differ'] == 1
    code, report = verify('twin')                                     # no entry has both keys: nothing to compare
    assert code == 0 and report['frames'] == 0
    # --from-polygons: the counts, boxes and areas of the exact file come back, the polygons stay
    assert rle.main(['--tracks', str(tmp_path / 'twin.json'), '--from-polygons', '--out', str(tmp_path / 'back.json')]) == 0
    back = json.loads((tmp_path / 'back.json').read_text())
    assert back['annotations'] == exact['annotations'] and back['videos'] == exact['videos']
    assert list(next(seg for seg in back['annotations'][2]['segmentations'] if seg is not None)) == ['size', 'counts', 'polygons']
    assert rle.main(['--tracks', str(tmp_path / 'twin.json'), '--from-polygons', '--recode', 'compressed', '--out', str(tmp_path / 'c.json')]) == 0
    assert json.loads((tmp_path / 'c.json').read_text()) == rle.recode_tracks(exact, 'compressed')


def test_session_load_tracks_takes_a_polygon_only_file(checkpoint, net, tmp_path):
    """`save_tracks(polygons=True)`, `counts` stripped: `load_tracks` fills the resident masks with the dense ids it decodes from counts."""
    from xmem2_amd.session import VideoSession
    imgs, msks, names = _write_clip(tmp_path / 'clip')                # the labels 3 and 7: dense ids differ from the labels
    config = {'model': checkpoint, 'size': -1, 'mem_every': 2}
    s = VideoSession(imgs, msks, overwrite_config=dict(config), network=net)
    s.save_reference(0)
    s.full_propagation()
    doc = json.load(open(s.save_tracks(tmp_path / 'first', polygons=True)))
    only = R.twin(doc)
    for ann in only['annotations']:
        ann['segmentations'][2] = None                                # a gap inside a launch
    (tmp_path / 'only.json').write_text(json.dumps(only))
    fresh = VideoSession(imgs, None, overwrite_config=dict(config), network=net)
    assert fresh.load_tracks(tmp_path / 'only.json', batch=3) == [0, 1, 3, 4, 5, 6]
    assert fresh.mapper.remappings == s.mapper.remappings == {3: 1, 7: 2}
    for t in range(7):
        assert torch.equal(fresh.masks[t], s.masks[t] if t != 2 else torch.zeros_like(s.masks[t])), t
