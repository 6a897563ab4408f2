"""GPU tests of the run-length track export (csrc/rle.hip, ops.rle_encode, config['save_tracks'], VideoSession.save_tracks):

1. the kernel against the numpy specification `rle.encode_host`, for every label: events, true counts, areas and boxes exactly equal,
   over tile-edge shapes, the chair annotations, batches, labels absent or above K, both load paths (16-byte and any pitch);
2. overflow: a frame whose events do not fit is encoded again and comes back whole; two runs give the same bytes;
3. run_on_video / run_on_video_ensemble / VideoSession with the option on: the PNGs are those of a run without it, tracks.json decodes
   to them, no mask travels when only tracks are asked for, and nothing is encoded with the option off."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CHAIR = os.path.join(GOLDEN, 'chair')
SHAPES = [(1, 1), (1, 64), (64, 1), (17, 33), (63, 65), (65, 63), (128, 256)]


# ---- 1. the kernel against the specification ------------------------------------------------------------------------------
def _check(maps, K, capacity=None):
    """ops.rle_encode of uint8 maps [B,H,W] (or a device tensor of them) against rle.record_host, label by label."""
    from xmem2_amd import ops, rle
    dev = maps if torch.is_tensor(maps) else torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    host = dev.cpu().numpy()
    meta, events = ops.rle_encode(dev, K, capacity)
    assert meta.shape == (host.shape[0], K, rle.META) and meta.dtype == np.int32 and len(events) == host.shape[0]
    for b in range(host.shape[0]):
        want_meta, want_events = rle.record_host(host[b], K)
        np.testing.assert_array_equal(meta[b], want_meta, err_msg=f'meta of frame {b}, shape {host.shape[1:]}, K {K}')
        assert events[b].dtype == np.uint32
        np.testing.assert_array_equal(events[b], want_events, err_msg=f'events of frame {b}, shape {host.shape[1:]}, K {K}')
        for k, ev in enumerate(rle.label_events(meta[b], events[b]), start=1):
            r = rle.encode_host(host[b], k)
            np.testing.assert_array_equal(ev, r.events)
            assert tuple(meta[b, k - 1]) == (len(r.events), r.area) + r.box
    return meta, events


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_the_specification_on_random_maps(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    for K in (1, 3, 254):
        noise = rng.integers(0, K + 1, size=(2,) + shape).astype(np.uint8)          # every pixel its own label: events everywhere
        _check(noise, K)
        blocks = np.repeat(np.repeat(rng.integers(0, K + 1, size=(1, -(-shape[0] // 5), -(-shape[1] // 3))), 5, 1), 3, 2)
        _check(blocks[:, :shape[0], :shape[1]].astype(np.uint8), K)                 # runs that cross rows, columns and tiles


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_on_full_empty_and_edge_frames(shape):
    from xmem2_amd import rle
    H, W = shape
    full, empty = np.full(shape, 2, np.uint8), np.zeros(shape, np.uint8)
    first, last = empty.copy(), empty.copy()
    first[0, 0] = 1
    last[-1, -1] = 3
    wrap = empty.copy()                                               # a run from the bottom of a column into the top of the next
    wrap[H // 2:, 0] = 1
    wrap[:H // 2 + 1, W - 1] = 1
    if W > 1:
        wrap[:H // 2 + 1, 1] = 1
    above = np.where(np.arange(H * W).reshape(shape) % 3 == 0, 255, 1).astype(np.uint8)   # 255 is above K: no plane of its own
    meta, events = _check(np.stack([full, empty, first, last, wrap, above]), 3)     # label 2 absent in most, label 3 in all but one
    assert tuple(meta[0, 1]) == (1, H * W, 0, 0, W - 1, H - 1) and events[0].tolist() == [0]     # counts [0, H*W]
    assert not meta[1, :, :2].any() and len(events[1]) == 0 and tuple(meta[1, 0, 2:]) == rle.EMPTY_BOX
    assert events[2][0] == 0 and events[3][0] == H * W - 1 and tuple(meta[3, 2]) == (1, 1, W - 1, H - 1, W - 1, H - 1)


def test_kernel_on_the_column_wrap_plane():
    from xmem2_amd import ops, rle
    wrap = np.zeros((4, 2), np.uint8)
    wrap[2:4, 0] = 1
    wrap[0:2, 1] = 1
    meta, events = _check(wrap[None], 1)
    assert events[0].tolist() == [2, 6] and rle.counts_from_events(events[0], 4, 2) == [2, 4, 2]
    one = ops.rle_encode(torch.from_numpy(wrap).cuda(), 1)            # [H,W] is a batch of one
    assert one[0].shape == (1, 1, rle.META) and one[1][0].tolist() == [2, 6]


def test_kernel_on_the_chair_annotations_in_one_batch():
    from PIL import Image
    from xmem2_amd import rle
    ann = os.path.join(CHAIR, 'Annotations')
    maps = np.stack([np.array(Image.open(os.path.join(ann, n)).convert('P'), np.uint8) for n in sorted(os.listdir(ann))])
    assert maps.shape == (10, 480, 720)
    meta, events = _check(maps, 1)
    assert 0 < meta[:, 0, 0].min() and meta[:, 0, 0].max() < rle.default_capacity(480, 720)   # far below the default capacity
    three = maps.copy()                                               # three labels, different contents per frame
    three[:, :200][three[:, :200] == 1] = 3
    three[:, :, 500:] = 2
    _check(three[:3], 3)


def test_both_load_paths_agree():
    """A map whose rows are 16-byte aligned takes the 16-byte loads; the same bytes at an odd address take the byte loads."""
    from xmem2_amd import ops
    rng = np.random.default_rng(5)
    maps = rng.integers(0, 4, size=(2, 70, 128)).astype(np.uint8)
    aligned = torch.from_numpy(maps).cuda()
    store = torch.empty(maps.size + 1, dtype=torch.uint8, device='cuda')
    odd = store[1:].view(maps.shape)
    odd.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 1 and odd.is_contiguous()
    a, b = _check(aligned, 3), _check(odd, 3)
    np.testing.assert_array_equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)


def test_ops_rle_encode_validates():
    from xmem2_amd import ops
    m = torch.zeros((4, 4), dtype=torch.uint8, device='cuda')
    for bad_k in (0, 255, True, 1.0):
        with pytest.raises(ValueError):
            ops.rle_encode(m, bad_k)
    with pytest.raises(ValueError):
        ops.rle_encode(m, 1, capacity=0)
    with pytest.raises(RuntimeError):
        ops.rle_encode(m.float(), 1)
    with pytest.raises(RuntimeError):
        ops.rle_encode(m[None, None], 1)


# ---- 2. overflow and determinism ----------------------------------------------------------------------------------------------
def test_overflow_is_encoded_again_with_the_exact_size(monkeypatch):
    from xmem2_amd import ops, rle
    yy, xx = np.mgrid[:64, :64]
    board = ((xx + yy) & 1).astype(np.uint8)
    quiet = np.zeros((64, 64), np.uint8)
    quiet[10:20, 10:20] = 1                                           # 20 events: does not fit 16 either
    tiny = np.zeros((64, 64), np.uint8)
    tiny[3, 3] = 1                                                    # 2 events: fits
    want = [rle.encode_host(m, 1) for m in (board, quiet, tiny)]
    calls, original = [], ops.rle_encode

    def spy(masks, K, capacity=None, wait=True):
        calls.append((tuple(masks.shape), capacity))
        return original(masks, K, capacity, wait)
    monkeypatch.setattr(ops, 'rle_encode', spy)
    retries = ops.RLE_STATS['retries']
    meta, events = ops.rle_encode(torch.from_numpy(np.stack([board, quiet, tiny])).cuda(), 1, capacity=16)
    assert calls == [((3, 64, 64), 16), ((1, 64, 64), len(want[0].events)), ((1, 64, 64), 20)]
    assert ops.RLE_STATS['retries'] == retries + 2
    for b in range(3):
        np.testing.assert_array_equal(events[b], want[b].events)      # the full list, nothing cut off
        assert tuple(meta[b, 0]) == (len(want[b].events), want[b].area) + want[b].box
    assert len(events[0]) > 16 and len(events[0]) == meta[0, 0, 0]


def test_two_runs_give_the_same_bytes():
    from xmem2_amd import ops, rle
    rng = np.random.default_rng(9)
    maps = torch.from_numpy(rng.integers(0, 6, size=(3, 130, 200)).astype(np.uint8)).cuda()
    K, cap = 5, 4 * 130 * 200
    recs = [ops.rle_encode(maps, K, cap, wait=False).cpu().numpy() for _ in range(2)]
    used = []
    for rec in recs:
        meta, events = rle.split_record(rec, 3, K, cap)
        used.append(meta.tobytes() + b''.join(events[b, :meta[b, :, 0].sum()].tobytes() for b in range(3)))
    assert used[0] == used[1] and len(used[0]) > 3 * K * rle.META * 4
    a, b = ops.rle_encode(maps, K), ops.rle_encode(maps, K)          # the default capacity overflows here: the retried frames too
    assert a[0].tobytes() == b[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))


# ---- 3. the video loops -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def checkpoint(synth_sd, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt') / 'XMem_synth.pth'
    torch.save(synth_sd, path)
    return str(path)


@pytest.fixture(scope='module')
def net(checkpoint):
    from xmem2_amd.network import XMem
    return XMem({'precision': 'fp32'}, checkpoint).to('cuda').eval()


def _chair(root, n):
    names = sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages')))[:n]
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(parents=True); msks.mkdir(parents=True)
    for nm in names:
        os.symlink(os.path.join(CHAIR, 'JPEGImages', nm), imgs / nm)
        os.symlink(os.path.join(CHAIR, 'Annotations', nm[:-4] + '.png'), msks / (nm[:-4] + '.png'))
    return str(imgs), str(msks), names


def _mask_bytes(out_dir):
    d = os.path.join(str(out_dir), 'masks')
    return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


def _spy(monkeypatch):
    from xmem2_amd import ops
    calls, original = [], ops.rle_encode

    def spy(masks, K, capacity=None, wait=True):
        calls.append((tuple(masks.shape), K, wait))
        return original(masks, K, capacity, wait)
    monkeypatch.setattr(ops, 'rle_encode', spy)
    return calls


def _assert_tracks_decode_to_the_pngs(tracks_path, masks_dir, names, first_annotation, labels):
    """tracks.json -> index masks (the annotations' labels) -> the colour mapping of the writers == the written PNGs, pixel for
    pixel; and the set of labels in the file is `labels`."""
    from PIL import Image
    from xmem2_amd import rle
    video, decoded = rle.read_tracks(tracks_path)
    assert video['file_names'] == list(names) and video['length'] == len(names)
    doc = json.load(open(tracks_path))
    assert sorted(a['label'] for a in doc['annotations']) == sorted(labels)
    ref = Image.open(first_annotation).convert('P')
    for name, ids in zip(names, decoded):
        png = Image.open(os.path.join(masks_dir, name[:-4] + '.png'))
        ids = np.zeros((video['height'], video['width']), np.uint8) if ids is None else ids       # no entry at all: an empty mask
        assert ids.shape == png.size[::-1]
        want = Image.fromarray(ids).quantize(palette=ref, dither=Image.Dither.NONE).convert('RGB')    # VideoReader.map_the_colors_back
        np.testing.assert_array_equal(np.array(want), np.array(png), err_msg=name)
    return doc, decoded


def test_run_on_video_on_the_chair_clip(checkpoint, net, tmp_path, monkeypatch):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = _chair(tmp_path / 'clip', 4)
    first = os.path.join(msks, names[0][:-4] + '.png')
    calls = _spy(monkeypatch)
    common = dict(frames_with_masks=[0], print_progress=False, save_overlay=False, network=net)
    off = run_on_video(imgs, msks, str(tmp_path / 'off'), overwrite_config={'model': checkpoint}, **common)
    assert calls == [] and not os.path.exists(tmp_path / 'off' / 'tracks.json')                # the option off: nothing is encoded
    both = run_on_video(imgs, msks, str(tmp_path / 'both'), overwrite_config={'model': checkpoint, 'save_tracks': True}, **common)
    assert [c for c in calls if not c[2]] == [((480, 720), 1, False)] * 4                      # one launch sequence per frame, no waiting
    assert _mask_bytes(tmp_path / 'both') == _mask_bytes(tmp_path / 'off')                     # the PNGs: byte-identical
    assert list(both['frame']) == list(off['frame']) == names
    doc, decoded = _assert_tracks_decode_to_the_pngs(tmp_path / 'both' / 'tracks.json', tmp_path / 'both' / 'masks', names, first, [1])
    (ann,) = doc['annotations']
    for t, ids in enumerate(decoded):
        ys, xs = np.nonzero(ids == 1)
        assert ann['areas'][t] == len(ys) > 0
        assert ann['bboxes'][t] == [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]
    only = run_on_video(imgs, msks, str(tmp_path / 'only'), overwrite_config={'model': checkpoint, 'save_tracks': True, 'save_masks': False},
                        **common)
    assert list(only['frame']) == names and not os.path.exists(tmp_path / 'only' / 'masks')
    assert open(tmp_path / 'only' / 'tracks.json', 'rb').read() == open(tmp_path / 'both' / 'tracks.json', 'rb').read()


def test_tracks_only_copies_no_mask_to_the_host(checkpoint, net, tmp_path, monkeypatch):
    from xmem2_amd import run_on_video as rov
    imgs, msks, names = _chair(tmp_path / 'clip', 3)
    shapes = []
    submit = rov.AsyncMaskFetcher.submit

    def spy(self, tag, mask_gpu):
        shapes.append(tuple(mask_gpu.shape))
        return submit(self, tag, mask_gpu)
    monkeypatch.setattr(rov.AsyncMaskFetcher, 'submit', spy)
    rov.run_on_video(imgs, msks, str(tmp_path / 'only'), frames_with_masks=[0], print_progress=False, network=net,
                     overwrite_config={'model': checkpoint, 'save_tracks': True, 'save_masks': False})
    from xmem2_amd import rle
    assert len(shapes) == 3 and all(len(s) == 1 for s in shapes)                               # the record, never the 480 x 720 mask
    assert shapes[0] == (4 * (rle.META + rle.default_capacity(480, 720)),) and shapes[0][0] * 20 < 480 * 720


def _write_clip(root, labels=(3, 7), hw=(96, 128), t=7):
    """A small synthetic clip whose annotation labels are not 1, 2: the file must carry them, not the dense ids."""
    from PIL import Image
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(parents=True); msks.mkdir(parents=True)
    frames, masks = synthetic_frames(t, *hw, seed=1234), synthetic_masks(t, len(labels), *hw)
    pal = [0] * 768
    for i, lab in enumerate(labels):
        pal[3 * lab:3 * lab + 3] = [(200, 0, 0), (0, 200, 0)][i]
    names = [f'frame_{i:06d}.png' for i in range(t)]
    for i, nm in enumerate(names):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(imgs / nm)
        idx = np.zeros(hw, np.uint8)
        for o, lab in enumerate(labels):
            idx[masks[i, o] > 0] = lab
        im = Image.fromarray(idx)
        im.putpalette(pal)
        im.save(msks / nm)
    return str(imgs), str(msks), names


def test_ensemble_writes_the_tracks_of_its_merged_masks(checkpoint, net, tmp_path, monkeypatch):
    from xmem2_amd import run_on_video as rov
    imgs, msks, names = _write_clip(tmp_path / 'clip')
    merged, submit = [], rov.AsyncMaskFetcher.submit

    def spy(self, tag, mask_gpu):
        if mask_gpu.dim() == 2:
            merged.append(mask_gpu.cpu().numpy())
        return submit(self, tag, mask_gpu)
    monkeypatch.setattr(rov.AsyncMaskFetcher, 'submit', spy)
    rov.run_on_video_ensemble(imgs, msks, str(tmp_path / 'out'), frames_with_masks=[0], print_progress=False, save_overlay=False, network=net,
                          overwrite_config={'model': checkpoint, 'size': -1, 'mem_every': 2, 'ensemble': [[-1, True]], 'save_tracks': True})
    _, decoded = _assert_tracks_decode_to_the_pngs(tmp_path / 'out' / 'tracks.json', tmp_path / 'out' / 'masks', names,
                                                   os.path.join(msks, names[0]), [3, 7])
    lut = np.zeros(256, np.uint8)
    lut[1], lut[2] = 3, 7                                             # dense ids -> the annotation's labels
    assert len(merged) == len(names)
    for ids, dense in zip(decoded, merged):
        np.testing.assert_array_equal(ids if ids is not None else np.zeros_like(dense), lut[dense])


def test_session_save_tracks(checkpoint, net, tmp_path, monkeypatch):
    from xmem2_amd import rle
    from xmem2_amd.session import VideoSession
    imgs, msks, names = _write_clip(tmp_path / 'clip')
    s = VideoSession(imgs, msks, overwrite_config={'model': checkpoint, 'size': -1, 'mem_every': 2}, network=net)
    s.save_reference(0)
    s.propagate(0, 'forward', stop=4)                                 # frames 5 and 6 have no mask yet
    monkeypatch.setattr(s, '_host_masks', lambda: pytest.fail('save_tracks must not copy the masks to the host'))
    path = s.save_tracks(tmp_path / 'partial')
    assert path == str(tmp_path / 'partial' / 'tracks.json')
    video, decoded = rle.read_tracks(path)
    assert video['length'] == 7 and video['file_names'] == names and decoded[5] is None and decoded[6] is None
    doc = json.load(open(path))
    assert [a['label'] for a in doc['annotations']] == [3, 7]
    for ann in doc['annotations']:
        assert ann['segmentations'][5:] == [None, None] and ann['bboxes'][5:] == [None, None] and ann['areas'][5:] == [None, None]
    for t in range(5):
        assert decoded[t] is not None
        np.testing.assert_array_equal(decoded[t], s.mask(t).cpu().numpy())
    monkeypatch.undo()
    s.full_propagation()
    s.save(tmp_path / 'full', save_overlay=False)
    s.save_tracks(tmp_path / 'full')
    _, decoded = _assert_tracks_decode_to_the_pngs(tmp_path / 'full' / 'tracks.json', tmp_path / 'full' / 'masks', names,
                                                   os.path.join(msks, names[0]), [3, 7])
    for t in range(7):
        np.testing.assert_array_equal(decoded[t], s.mask(t).cpu().numpy())
