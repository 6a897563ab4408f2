"""GPU tests of the compressed COCO string form of the track counts (csrc/rle.hip `xmem_rle_compress` / `xmem_rle_decompress`,
ops.rle_compress / ops.rle_decompress, config['tracks_counts']):

1. compress against `rle.compress_counts` on `rle.encode_host`: edge shapes and patterns, the chair annotations, a string longer than
   a chunk, wide values from a hand-made record, both overflow kinds, determinism;
2. decompress against `rle.decompress_counts`: the same patterns, batches with holes, every malformed and non-plane kind, capacity
   overflow, and painting through the existing decoder;
3. the device round trip without a host step;
4. the product: run_on_video / the ensemble / VideoSession / compute_metrics / tracks as annotations with the compressed form."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_rle import (_assert_tracks_decode_to_the_pngs, _chair, _mask_bytes, _write_clip, checkpoint,      # noqa: F401
                          net)                                       # noqa: F401  (the fixtures and clips of the encoder's tests)

pytestmark = pytest.mark.gpu
CHAIR_ANN = os.path.join(GOLDEN, 'chair', 'Annotations')
SHAPES = [(1, 1), (5, 3), (33, 16), (67, 130)]
RUNS = [1, 2, 15, 16, 17, 511, 512, 600, 20000, 1 << 20]


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def _from_runs(shape, runs):
    """An index map from (label, start, stop) runs in the COCO order j = x * H + y."""
    H, W = shape
    flat = np.zeros(H * W, np.uint8)
    for lab, a, b in runs:
        flat[a:b] = lab
    return np.ascontiguousarray(flat.reshape(W, H).T)


def _patterns(shape, seed=0):
    """uint8 [B,H,W] for K = 3: random maps, full, empty, a single pixel, pixel 0 set (a first count of 0), a label that ends at the
    last pixel (an odd number of events), labels with exactly 2, 3 and 4 counts (the i > 2 boundary of the differences)."""
    H, W = shape
    n = H * W
    rng = np.random.default_rng(seed + 1000 * H + W)
    maps = [rng.integers(0, 4, size=shape).astype(np.uint8), rng.integers(0, 4, size=shape).astype(np.uint8),
            np.repeat(np.repeat(rng.integers(0, 4, size=(-(-H // 5), -(-W // 3))), 5, 0), 3, 1)[:H, :W].astype(np.uint8),
            np.full(shape, 2, np.uint8), np.zeros(shape, np.uint8)]
    if n >= 15:
        maps += [_from_runs(shape, [(1, n // 2, n // 2 + 1)]),                                   # counts [n/2, 1, rest]: 3
                 _from_runs(shape, [(1, 0, 1)]),                                                 # counts [0, 1, n - 1]
                 _from_runs(shape, [(3, n // 2, n)]),                                            # counts [n/2, n - n/2]: 2
                 _from_runs(shape, [(1, 1, 3), (2, 3, 5), (1, n - 2, n)]),                       # label 1: [1, 2, n - 5, 2]: 4; label 2: 3
                 _from_runs(shape, [(2, 0, 2), (3, 2, 3), (2, 7, n)])]                           # label 2: [0, 2, 5, n - 7]: first count 0, 4 counts
    return np.stack(maps)


def _host_strings(maps, K):
    """The definition: per frame, per label, the compressed string of `encode_host`'s counts ('' for a label without event)."""
    from xmem2_amd import rle
    out = []
    for m in maps:
        rows = []
        for k in range(1, K + 1):
            r = rle.encode_host(m, k)
            rows.append(rle.compress_counts(r.counts) if len(r.events) else '')
        out.append(rows)
    return out


def _record(maps, K, capacity):
    from xmem2_amd import ops
    return ops.rle_encode(torch.from_numpy(np.ascontiguousarray(maps)).cuda(), K, capacity, wait=False)


def _events_of(strings, H, W):
    """host: per frame the packed events and per-row counts of a [B][K] table of strings / None"""
    from xmem2_amd import rle
    frames = []
    for rows in strings:
        ev = [rle.events_from_counts(s, H, W) if s else np.zeros(0, np.uint32) for s in rows]
        frames.append(([len(e) for e in ev], np.concatenate(ev) if ev else np.zeros(0, np.uint32)))
    return frames


def _check_decompress(strings, H, W, K, capacity=None):
    """ops.rle_decompress of good strings against the host definition; returns (record, capacity)."""
    from xmem2_amd import ops, rle
    record = ops.rle_decompress(strings, H, W, K, capacity)
    B = len(strings)
    capacity = record.numel() // B - K * rle.META
    meta, events = rle.split_record(record.cpu().numpy(), B, K, capacity)
    for b, (lens, want) in enumerate(_events_of(strings, H, W)):
        assert meta[b, :, 0].tolist() == lens and not meta[b, :, 1:].any(), f'meta of frame {b}'
        np.testing.assert_array_equal(events[b, :len(want)], want, err_msg=f'events of frame {b}')
    return record, capacity


# ---- 1. compress ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_compress_equals_the_definition(shape):
    from xmem2_amd import ops, rle
    H, W = shape
    maps = _patterns(shape)
    capacity = 2 * H * W + 2
    want = _host_strings(maps, 3)
    got = ops.rle_compress(_record(maps, 3, capacity), H, W, 3, capacity, char_capacity=8 * H * W + 8)
    assert got == want
    # the same through the device tensor, as a frame loop reads it
    ccap = max(1, max(sum(len(s) for s in rows) for rows in want))
    dev = ops.rle_compress(_record(maps, 3, capacity), H, W, 3, capacity, char_capacity=ccap, wait=False)
    assert dev.dtype == torch.uint8 and dev.numel() == 4 * len(maps) * 3 + len(maps) * ccap
    str_len, chars = rle.split_string_record(dev.cpu().numpy(), len(maps), 3, ccap)
    assert str_len.tolist() == [[len(s) for s in rows] for rows in want]
    assert [rle.label_strings(str_len[b], chars[b]) for b in range(len(maps))] == want


def test_compress_the_chair_annotations_in_one_batch():
    from PIL import Image
    from xmem2_amd import ops, rle
    maps = np.stack([np.array(Image.open(os.path.join(CHAIR_ANN, n)).convert('P'), np.uint8) for n in sorted(os.listdir(CHAIR_ANN))])
    before = dict(ops.RLE_STRING_STATS)
    capacity = rle.default_capacity(480, 720)
    got = ops.rle_compress(_record(maps, 1, capacity), 480, 720, 1, capacity)           # the default character capacity
    assert got == _host_strings(maps, 1)
    assert ops.RLE_STRING_STATS['retries'] == before['retries']                         # far below the default: no frame again
    assert max(len(rows[0]) for rows in got) * 4 < rle.default_char_capacity(480, 720)
    three = maps[:3].copy()
    three[:, :200][three[:, :200] == 1] = 3
    three[:, :, 500:] = 2
    assert ops.rle_compress(_record(three, 3, capacity), 480, 720, 3, capacity) == _host_strings(three, 3)


def _alternating():
    """1500 x 2: label 1 on every even j (3000 events, one string of about 3000 values), labels 2 and 3 share the odd ones."""
    j = np.arange(3000)
    flat = np.where(j % 2 == 0, 1, np.where(j % 4 == 1, 2, 3)).astype(np.uint8)
    return np.ascontiguousarray(flat.reshape(2, 1500).T)[None]


def test_strings_longer_than_a_chunk():
    from xmem2_amd import ops
    maps = _alternating()
    want = _host_strings(maps, 3)
    assert len(want[0][0]) >= 3000 and min(len(s) for s in want[0]) > 1024
    capacity = 6100
    assert ops.rle_compress(_record(maps, 3, capacity), 1500, 2, 3, capacity, char_capacity=8000) == want
    record, cap = _check_decompress(want, 1500, 2, 3)
    np.testing.assert_array_equal(ops.rle_decode(record, 1500, 2, 3, cap).cpu().numpy(), maps)


def _wide_counts():
    """Counts of three rows of a 16384 x 16384 plane: 2^27-scale counts and 6-character differences of both signs; about 1000 runs of
    every length class (a string of several chunks whose values straddle the chunk borders); [0, 2^28]."""
    hw = 1 << 28
    a = [5, 3, 1 << 27, 7, 4, 1 << 26]
    a.append(hw - sum(a))
    rng = np.random.default_rng(28)
    b = [int(v) for v in rng.choice(RUNS, size=1000)]
    b.append(hw - sum(b))
    assert b[-1] > 0
    return [a, b, [0, hw]]


def test_wide_values_from_a_hand_made_record():
    from xmem2_amd import ops, rle
    H = W = 16384
    counts = _wide_counts()
    want = [rle.compress_counts(c) for c in counts]
    assert want[2] == '0PPPPP8' and 'PPPPP' in want[0]
    values = [c - counts[0][i - 2] if i > 2 else c for i, c in enumerate(counts[0])]
    assert any(v >= 1 << 24 for v in values) and any(v < -(1 << 24) for v in values)   # 6 characters, both signs
    events = [np.cumsum(c[:-1]).astype(np.uint32) for c in counts]
    capacity = sum(len(e) for e in events) + 5
    buf = np.zeros(3 * rle.META + capacity, np.int32)
    meta, ev = rle.split_record(buf, 1, 3, capacity)
    meta[0, :, 0] = [len(e) for e in events]
    ev[0, :capacity - 5] = np.concatenate(events)
    got = ops.rle_compress(torch.from_numpy(buf).cuda(), H, W, 3, capacity, char_capacity=8192)
    assert got == [want]
    record = ops.rle_decompress([want], H, W, 3, capacity)
    back_meta, back_ev = rle.split_record(record.cpu().numpy(), 1, 3, capacity)
    assert back_meta[0, :, 0].tolist() == [len(e) for e in events]
    np.testing.assert_array_equal(back_ev[0, :capacity - 5], np.concatenate(events))


def test_character_overflow_reports_true_lengths_and_writes_nothing_beyond():
    from xmem2_amd import _lib, ops, rle
    H, W, K = 33, 16, 3
    rng = np.random.default_rng(9)
    maps = np.stack([_from_runs((H, W), [(1, 3, 9), (2, 20, 40)]), rng.integers(0, 4, size=(H, W)).astype(np.uint8)])
    want = _host_strings(maps, K)
    totals = [sum(len(s) for s in rows) for rows in want]
    assert totals[1] > totals[0]
    ccap = totals[1] - 1                                              # one byte too small for the last frame
    capacity = 2 * H * W
    rec = _record(maps, K, capacity)
    lib = _lib.load()
    guard = 64
    str_len = torch.full((2, K), 7, dtype=torch.int32, device='cuda')
    chars = torch.full((2 * ccap + guard,), 0xAA, dtype=torch.uint8, device='cuda')
    ws = torch.empty(lib.xmem_rle_compress_workspace_bytes(2, K, capacity), dtype=torch.uint8, device='cuda')
    _lib.check(lib.xmem_rle_compress(_lib.ptr(rec), rec.data_ptr() + 4 * 2 * K * rle.META, 2, H, W, K, capacity, ccap, _lib.ptr(str_len),
                                     _lib.ptr(chars), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert str_len.cpu().tolist() == [[len(s) for s in rows] for rows in want]         # the true lengths, also of the frame that is cut
    host = chars.cpu().numpy()
    assert (host[2 * ccap:] == 0xAA).all()                                             # nothing behind the buffer
    assert bytes(host[:totals[0]]).decode() == ''.join(want[0]) and (host[totals[0]:ccap] == 0xAA).all()
    assert bytes(host[ccap:2 * ccap]).decode() == ''.join(want[1])[:ccap]              # cut, not shifted
    before = dict(ops.RLE_STRING_STATS)
    assert ops.rle_compress(rec, H, W, K, capacity, char_capacity=ccap) == want        # wait=True: that frame again, at its exact size
    assert ops.RLE_STRING_STATS['retries'] == before['retries'] + 1


def test_event_overflow_marks_the_frame_and_leaves_its_neighbours_exact():
    from xmem2_amd import ops, rle
    H, W, K = 33, 16, 3
    rng = np.random.default_rng(10)
    quiet = _from_runs((H, W), [(1, 3, 9), (3, 20, 40), (1, 100, 101)])
    maps = np.stack([quiet, rng.integers(0, 4, size=(H, W)).astype(np.uint8), quiet[::-1].copy()])
    want = _host_strings(maps, K)
    capacity = 16                                                     # the noisy frame has hundreds of events
    rec = _record(maps, K, capacity)
    dev = ops.rle_compress(rec, H, W, K, capacity, char_capacity=64, wait=False)
    str_len, chars = rle.split_string_record(dev.cpu().numpy(), 3, K, 64)
    assert str_len[1].tolist() == [-1, -1, -1] and not chars[1].any()
    for b in (0, 2):
        assert rle.label_strings(str_len[b], chars[b]) == want[b]
    got = ops.rle_compress(rec, H, W, K, capacity, char_capacity=64)
    assert got[0] == want[0] and got[1] is None and got[2] == want[2]


def test_two_runs_give_the_same_bytes():
    from xmem2_amd import ops
    maps = _patterns((67, 130), seed=3)
    capacity = 2 * 67 * 130
    rec = _record(maps, 3, capacity)
    a = ops.rle_compress(rec, 67, 130, 3, capacity, char_capacity=40000, wait=False)
    b = ops.rle_compress(rec, 67, 130, 3, capacity, char_capacity=40000, wait=False)
    assert torch.equal(a, b) and int(a[4 * len(maps) * 3:].count_nonzero()) > 10000
    strings = [[s or None for s in rows] for rows in _host_strings(maps, 3)]
    c, d = ops.rle_decompress(strings, 67, 130, 3, capacity), ops.rle_decompress(strings, 67, 130, 3, capacity)
    assert torch.equal(c, d)


def test_ops_rle_compress_validates():
    from xmem2_amd import ops
    rec = torch.zeros(3 * 6 + 64, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.rle_compress(rec, 8, 8, 3, 63)                            # not a whole number of frames
    with pytest.raises(ValueError):
        ops.rle_compress(rec, 8, 8, 3, 64, char_capacity=0)
    with pytest.raises(RuntimeError):
        ops.rle_compress(rec.float(), 8, 8, 3, 64)
    assert ops.rle_compress(rec, 8, 8, 3, 64) == [['', '', '']]       # no events: no strings


# ---- 2. decompress --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES)
def test_decompress_equals_the_definition(shape):
    from xmem2_amd import ops
    H, W = shape
    maps = _patterns(shape)
    strings = [[s or None for s in rows] for rows in _host_strings(maps, 3)]
    record, capacity = _check_decompress(strings, H, W, 3)
    np.testing.assert_array_equal(ops.rle_decode(record, H, W, 3, capacity).cpu().numpy(), maps)
    as_bytes = [[s.encode() if s else None for s in rows] for rows in strings]
    assert torch.equal(ops.rle_decompress(as_bytes, H, W, 3, capacity), record)


def test_decompress_a_batch_of_33_frames_with_holes():
    from xmem2_amd import ops, rle
    H, W, K = 33, 16, 3
    rng = np.random.default_rng(33)
    maps = rng.integers(0, 4, size=(33, H, W)).astype(np.uint8)
    maps[7] = 0                                                       # a frame without any entry
    maps[12][maps[12] == 2] = 0                                       # rows with an empty range, in the middle and at both ends
    maps[13][maps[13] == 1] = 0
    maps[14][maps[14] == 3] = 0
    strings = [[s or None for s in rows] for rows in _host_strings(maps, K)]
    strings[20][1] = rle.compress_counts([H * W])                     # another tool's empty mask: one count, no event
    maps[20][maps[20] == 2] = 0
    assert strings[7] == [None] * 3 and strings[12][1] is None
    record, capacity = _check_decompress(strings, H, W, K)
    np.testing.assert_array_equal(ops.rle_decode(record, H, W, K, capacity).cpu().numpy(), maps)


def test_decompress_reports_every_bad_kind_and_leaves_the_neighbours_exact():
    from xmem2_amd import ops, rle
    H, W, K = 33, 16, 3
    n = H * W
    maps = _patterns((H, W), seed=5)[:3]
    good = [[s or None for s in rows] for rows in _host_strings(maps, K)]
    bad = [('5/3', 1), ('5p3', 1), ('PPPPPPP0', 1), (rle.compress_counts([3, 4])[:-1] + 'P', 1), ('5P', 1),     # malformed
           (rle.compress_counts([3, -1, n - 2]), 2), (rle.compress_counts([2, 0, n - 2]), 2), (rle.compress_counts([5]), 2),
           (rle.compress_counts([n - 1, 2]), 2), (rle.compress_counts([0, 0, n]), 2)]                           # not a plane
    for s, _ in bad[5:]:
        rle.decompress_counts(s)                                      # well-formed, but ...
        with pytest.raises(ValueError):
            rle.decode(s, H, W)
    for s, _ in bad[:5]:
        with pytest.raises(ValueError):
            rle.decompress_counts(s)
    strings, want_status = [], []
    for i, (s, code) in enumerate(bad):                               # the bad row first, in the middle, last; good frames between
        rows = list(good[i % 3])
        rows[i % 3] = s
        strings += [rows, [list(r) for r in good][(i + 1) % 3]]
        want_status += [[code if k == i % 3 else 0 for k in range(K)], [0] * K]
    capacity = 2 * n
    with pytest.raises(ValueError, match='frame 0, row 0'):
        ops.rle_decompress(strings, H, W, K, capacity)
    record, status = ops.rle_decompress(strings, H, W, K, capacity, check=False)
    assert status.cpu().tolist() == want_status
    meta, events = rle.split_record(record.cpu().numpy(), len(strings), K, capacity)
    cleaned = [[None if want_status[b][k] else s for k, s in enumerate(rows)] for b, rows in enumerate(strings)]
    for b, (lens, want) in enumerate(_events_of(cleaned, H, W)):      # a bad row: no events; the others as if it had no string
        assert meta[b, :, 0].tolist() == lens and not meta[b, :, 1:].any()
        np.testing.assert_array_equal(events[b, :len(want)], want)
        assert not events[b, len(want):].any()
    with pytest.raises(ValueError, match='empty'):
        ops.rle_decompress([['', None, None]], H, W, K)
    # offsets that are no range of the characters are malformed too, and nothing outside the characters is read
    chars = torch.frombuffer(bytearray(b'53' * 8), dtype=torch.uint8).cuda()
    ofs = torch.tensor([[0, 5, 3, 3], [3, 3, 17, 17], [-1, 2, 2, 2]], dtype=torch.int32, device='cuda')
    _, status = ops.rle_decompress((chars, ofs), H, W, K, 8, check=False)
    assert status.cpu().tolist() == [[2, 1, 0], [0, 1, 1], [1, 0, 0]]


def test_decompress_capacity_overflow_is_status_3():
    from xmem2_amd import ops, rle
    H, W, K = 33, 16, 3
    maps = np.stack([_from_runs((H, W), [(1, 3, 9), (3, 20, 40)]), np.random.default_rng(4).integers(0, 4, size=(H, W)).astype(np.uint8),
                     _from_runs((H, W), [(2, 0, 5)])])
    strings = [[s or None for s in rows] for rows in _host_strings(maps, K)]
    record, status = ops.rle_decompress(strings, H, W, K, 8, check=False)
    assert status.cpu().tolist() == [[0, 0, 0], [3, 3, 3], [0, 0, 0]]
    meta, events = rle.split_record(record.cpu().numpy(), 3, K, 8)
    assert not meta[1].any() and not events[1].any()
    assert meta[0, :, 0].tolist() == [2, 0, 2] and events[0, :4].tolist() == [3, 9, 20, 40] and events[2, :2].tolist() == [0, 5]
    with pytest.raises(ValueError, match='frame 1, row 0'):
        ops.rle_decompress(strings, H, W, K, 8)
    masks, frame_status = ops.rle_decode(record, H, W, K, 8, check=False)
    assert frame_status.cpu().tolist() == [0, 0, 0]
    np.testing.assert_array_equal(masks[0].cpu().numpy(), maps[0])


def test_decompress_then_decode_paints_like_the_host_and_the_higher_row_wins():
    from xmem2_amd import ops, rle
    H, W, K = 33, 16, 3
    rng = np.random.default_rng(6)
    frames, want = [], []
    for _ in range(3):
        planes = [rng.random((H, W)) < p for p in (0.5, 0.3, 0.2)]                   # rows of another tool: they overlap
        rows = [rle.compress_counts(rle.encode_host(p.astype(np.uint8), 1).counts) for p in planes]
        frames.append(rows)
        paint = np.zeros((H, W), np.uint8)
        for k, s in enumerate(rows):
            paint[rle.decode(s, H, W)] = (7, 9, 200)[k]
        want.append(paint)
    assert ((np.stack(want) == 7).any() and (np.stack(want) == 200).any())
    record = ops.rle_decompress(frames, H, W, K)
    capacity = record.numel() // 3 - K * rle.META
    got = ops.rle_decode(record, H, W, K, capacity, values=[7, 9, 200])
    np.testing.assert_array_equal(got.cpu().numpy(), np.stack(want))


# ---- 3. the device round trip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 3), (64, 64), (67, 130)])
def test_device_round_trip_without_a_host_step(shape, monkeypatch):
    from xmem2_amd import ops
    H, W = shape
    maps = torch.from_numpy(_patterns(shape, seed=8)).cuda()
    B, K, capacity, ccap = maps.shape[0], 3, 2 * H * W + 2, 8 * H * W + 8
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: pytest.fail('a tensor went to the host'))
    rec = ops.rle_encode(maps, K, capacity, wait=False)
    srec = ops.rle_compress(rec, H, W, K, capacity, ccap, wait=False)
    record, status = ops.rle_decompress(ops.rle_string_offsets(srec, B, K, ccap), H, W, K, capacity, check=False)
    back, frame_status = ops.rle_decode(record, H, W, K, capacity, check=False)
    monkeypatch.undo()
    assert not status.any() and not frame_status.any()
    assert torch.equal(back, maps)
    assert torch.equal(record[:B * K * 6].view(B, K, 6)[:, :, 0], rec[:B * K * 6].view(B, K, 6)[:, :, 0])       # the event counts


# ---- 4. the product -------------------------------------------------------------------------------------------------------------
def test_run_on_video_writes_compressed_tracks_and_reads_them_as_annotations(checkpoint, net, tmp_path):
    from xmem2_amd import ops, rle
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = _chair(tmp_path / 'clip', 5)
    first = os.path.join(msks, names[0][:-4] + '.png')
    common = dict(frames_with_masks=[0, 3], print_progress=False, save_overlay=False, network=net)
    run_on_video(imgs, msks, str(tmp_path / 'list'), overwrite_config={'model': checkpoint, 'save_tracks': True}, **common)
    before = (dict(ops.RLE_STATS), dict(ops.RLE_STRING_STATS))
    config = {'model': checkpoint, 'save_tracks': True, 'tracks_counts': 'compressed'}
    a = run_on_video(imgs, msks, str(tmp_path / 'comp'), overwrite_config=dict(config), **common)
    assert ops.RLE_STATS['retries'] == before[0]['retries'] and ops.RLE_STRING_STATS['retries'] == before[1]['retries']   # the defaults fit
    assert ops.RLE_STRING_STATS['launches'] == before[1]['launches'] + 5
    assert _mask_bytes(tmp_path / 'comp') == _mask_bytes(tmp_path / 'list')
    doc, _ = _assert_tracks_decode_to_the_pngs(tmp_path / 'comp' / 'tracks.json', tmp_path / 'comp' / 'masks', names, first, [1])
    segs = doc['annotations'][0]['segmentations']
    assert all(isinstance(s['counts'], str) and s['size'] == [480, 720] for s in segs) and len(segs) == 5
    listed = open(tmp_path / 'list' / 'tracks.json', 'rb').read()
    assert json.dumps(rle.recode_tracks(doc, 'list'), separators=(',', ':')).encode() == listed       # the file 'list' writes
    assert len(open(tmp_path / 'comp' / 'tracks.json', 'rb').read()) < len(listed)
    # the predictions written by a tool that only has strings, as annotations: the same masks as from the PNG annotations
    from PIL import Image
    writer = rle.TrackWriter(480, 720)
    for n in names:
        writer.add_mask(n, np.array(Image.open(os.path.join(msks, n[:-4] + '.png')).convert('P'), np.uint8), counts='compressed')
    tracks = writer.write(str(tmp_path / 'ann.json'))
    b = run_on_video(imgs, tracks, str(tmp_path / 'from_tracks'), overwrite_config=dict(config), **common)
    assert a.equals(b) and list(b['mask_provided']) == [True, False, False, True, False]
    assert _mask_bytes(tmp_path / 'from_tracks') == _mask_bytes(tmp_path / 'comp')
    assert open(tmp_path / 'from_tracks' / 'tracks.json', 'rb').read() == open(tmp_path / 'comp' / 'tracks.json', 'rb').read()
    masks, present = rle.TrackReader(tracks).masks_device()            # decompressed and painted on the device
    assert present.all()
    for t, n in enumerate(names):
        np.testing.assert_array_equal(masks[t].cpu().numpy(), np.array(Image.open(os.path.join(msks, n[:-4] + '.png')).convert('P')))


def test_compressed_tracks_only_copies_neither_mask_nor_events_to_the_host(checkpoint, net, tmp_path, monkeypatch):
    from xmem2_amd import rle
    from xmem2_amd import run_on_video as rov
    imgs, msks, names = _chair(tmp_path / 'clip', 3)
    shapes = []
    submit = rov.AsyncMaskFetcher.submit

    def spy(self, tag, mask_gpu):
        shapes.append(tuple(mask_gpu.shape))
        return submit(self, tag, mask_gpu)
    monkeypatch.setattr(rov.AsyncMaskFetcher, 'submit', spy)
    monkeypatch.setattr(rle, 'label_events', lambda *a, **k: pytest.fail('an event list was read on the host'))
    rov.run_on_video(imgs, msks, str(tmp_path / 'only'), frames_with_masks=[0], print_progress=False, network=net,
                     overwrite_config={'model': checkpoint, 'save_tracks': True, 'save_masks': False, 'tracks_counts': 'compressed'})
    # meta + string lengths + characters: less than the list form's record, never the 480 x 720 mask
    assert shapes == [(4 * rle.META + 4 + rle.default_char_capacity(480, 720),)] * 3
    assert shapes[0][0] < 4 * (rle.META + rle.default_capacity(480, 720)) and not os.path.exists(tmp_path / 'only' / 'masks')
    monkeypatch.undo()
    doc = json.load(open(tmp_path / 'only' / 'tracks.json'))
    assert all(isinstance(s['counts'], str) for s in doc['annotations'][0]['segmentations'])
    assert all(m is not None and m.any() for m in rle.read_tracks(tmp_path / 'only' / 'tracks.json')[1])


def test_track_loop_redoes_a_frame_whose_events_or_characters_did_not_fit():
    """Both overflow kinds of the frame loop, without a network: the loop's own submit / finish on a noisy frame."""
    from xmem2_amd import ops, rle
    from xmem2_amd.mask_mapper import MaskMapper
    from xmem2_amd.frame_outputs import Tag, _TrackLoop
    H, W, K = 33, 16, 3
    noisy = np.random.default_rng(12).integers(0, 4, size=(H, W)).astype(np.uint8)
    quiet = _from_runs((H, W), [(1, 3, 9), (2, 20, 40), (3, 50, 60)])
    mapper = MaskMapper()
    mapper.convert_mask(np.array([[1, 2, 3]], np.uint8), exhaustive=True)
    for capacity, ccap in ((16, 4096), (4096, 16)):                   # the events do not fit; the characters do not fit
        loop = _TrackLoop('compressed')
        before = (ops.RLE_STATS['retries'], ops.RLE_STRING_STATS['retries'])
        arrived = []
        for t, m in enumerate((quiet, noisy, quiet)):
            dev = torch.from_numpy(m).cuda()
            if t > 0:                                                 # the noisy frame alone gets the small room
                loop.events.size, loop.chars.size = (capacity, ccap) if t == 1 else (4096, 4096)
            arrived += loop.submit(Tag(f'{t}.png'), dev, mapper)
        arrived += loop.drain()
        for item in arrived:
            loop.finish(item, mapper)
        assert (ops.RLE_STATS['retries'] - before[0], ops.RLE_STRING_STATS['retries'] - before[1]) == ((1, 0) if capacity == 16 else (0, 1))
        want = rle.TrackWriter(H, W)
        for t, m in enumerate((quiet, noisy, quiet)):
            want.add_mask(f'{t}.png', m, k=K, counts='compressed')
        assert loop.writer.to_dict() == want.to_dict()


def test_ensemble_and_session_write_compressed_tracks_and_the_session_loads_them(checkpoint, net, tmp_path):
    from xmem2_amd import rle
    from xmem2_amd import run_on_video as rov
    from xmem2_amd.session import VideoSession
    imgs, msks, names = _write_clip(tmp_path / 'clip')                # the labels 3 and 7
    config = {'model': checkpoint, 'size': -1, 'mem_every': 2}
    rov.run_on_video_ensemble(imgs, msks, str(tmp_path / 'ens'), frames_with_masks=[0], print_progress=False, save_overlay=False, network=net,
                              overwrite_config=dict(config, ensemble=[[-1, True]], save_tracks=True, tracks_counts='compressed'))
    doc, _ = _assert_tracks_decode_to_the_pngs(tmp_path / 'ens' / 'tracks.json', tmp_path / 'ens' / 'masks', names,
                                               os.path.join(msks, names[0]), [3, 7])
    assert all(isinstance(s['counts'], str) for a in doc['annotations'] for s in a['segmentations'] if s is not None)

    s = VideoSession(imgs, msks, overwrite_config=dict(config), network=net)
    s.save_reference(0)
    s.propagate(0, 'forward', stop=4)                                 # frames 5 and 6 have no mask
    listed = s.save_tracks(tmp_path / 'list')
    path = s.save_tracks(tmp_path / 'comp', counts='compressed')
    doc = json.load(open(path))
    assert all(isinstance(seg['counts'], str) for a in doc['annotations'] for seg in a['segmentations'] if seg is not None)
    assert json.dumps(rle.recode_tracks(doc, 'list'), separators=(',', ':')).encode() == open(listed, 'rb').read()
    with pytest.raises(ValueError):
        s.save_tracks(tmp_path / 'zip', counts='zip')
    fresh = VideoSession(imgs, msks, overwrite_config=dict(config), network=net)
    assert fresh.load_tracks(path) == [0, 1, 2, 3, 4]
    assert fresh._present == s._present and torch.equal(fresh.masks, s.masks) and int(fresh.masks.max()) == 2
    masks, present = rle.TrackReader(path).masks_device(values='dense', batch=3)     # string frames and frames without entry in a launch
    assert present.tolist() == [True] * 5 + [False] * 2 and torch.equal(masks, s.masks)
    mixed = rle.recode_tracks(doc, 'list')                            # a file that mixes the forms frame by frame and row by row
    for a in mixed['annotations']:
        for t in (0, 3):
            a['segmentations'][t] = doc['annotations'][a['id'] - 1]['segmentations'][t]
    mixed['annotations'][0]['segmentations'][1] = doc['annotations'][0]['segmentations'][1]
    masks, present = rle.TrackReader(mixed).masks_device(values='dense', batch=4)
    assert torch.equal(masks, s.masks)


def test_compute_metrics_from_compressed_tracks_equals_from_pngs(tmp_path):
    from PIL import Image
    from xmem2_amd import metrics
    from xmem2_amd.rle import TrackWriter
    (tmp_path / 'gt').mkdir()
    os.symlink(CHAIR_ANN, tmp_path / 'gt' / 'chair')
    names = sorted(os.listdir(CHAIR_ANN))
    palette = Image.open(os.path.join(CHAIR_ANN, names[0])).getpalette()
    (tmp_path / 'png' / 'chair' / 'masks').mkdir(parents=True)
    writer = TrackWriter(480, 720)
    for i, n in enumerate(names):
        p = np.roll(np.array(Image.open(os.path.join(CHAIR_ANN, n)).convert('P'), np.uint8), (3 + i, -5), axis=(0, 1))
        p[10:40, 20:90] = 2
        im = Image.fromarray(p)
        im.putpalette(palette)
        im.save(tmp_path / 'png' / 'chair' / 'masks' / n)
        writer.add_mask(n, p, counts='compressed')
    writer.write(str(tmp_path / 'tracks' / 'chair'))
    from_png = metrics.compute_metrics(tmp_path / 'gt', tmp_path / 'png')
    assert metrics.compute_metrics(tmp_path / 'gt', tmp_path / 'tracks').equals(from_png)              # auto
    assert metrics.compute_metrics(tmp_path / 'gt', tmp_path / 'tracks', pred_format='tracks').equals(from_png)
    assert 0 < from_png['iou'].iloc[0] < 1
