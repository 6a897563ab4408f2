"""GPU tests of the polygon tracer (csrc/polygons.hip, ops.mask_polygons) and of config['tracks_polygons']:

1. the kernels against the numpy definition `polygons.record_host`: `meta` and every corner word exactly equal, over tile-edge shapes,
   K = 1, 3, 254, noise and block maps, full / empty / corner-pixel frames, labels above K, batches, an odd base pointer;
2. saddles and long rings: the checkerboard and its complement, diagonals of 1500 pixels (one ring of 6000 corners), nesting;
3. the chair annotations, and the number of outer rings against the 8-connected components of `ops.components`;
4. overflow (the true counts, the frame traced again) and two runs giving the same bytes;
5. the product: run_on_video, VideoSession.save_tracks and `python -m xmem2_amd.rle --polygons` with the option on and off."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
CHAIR = os.path.join(GOLDEN, 'chair')
SHAPES = [(1, 1), (1, 64), (64, 1), (17, 33), (33, 65), (63, 65), (65, 63), (128, 256)]


# ---- 1. the kernels against the definition -----------------------------------------------------------------------------------
def _check(maps, K, capacity=None):
    """ops.mask_polygons of uint8 maps [B,H,W] (or a device tensor of them) against polygons.record_host, frame by frame."""
    from xmem2_amd import ops, polygons
    dev = maps if torch.is_tensor(maps) else torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    host = dev.cpu().numpy()
    meta, words = ops.mask_polygons(dev, K, capacity)
    assert meta.shape == (host.shape[0], K, polygons.META) and meta.dtype == np.int32 and len(words) == host.shape[0]
    for b in range(host.shape[0]):
        want_meta, want_words = polygons.record_host(host[b], K)
        np.testing.assert_array_equal(meta[b], want_meta, err_msg=f'meta of frame {b}, shape {host.shape[1:]}, K {K}')
        assert words[b].dtype == np.uint32
        np.testing.assert_array_equal(words[b], want_words, err_msg=f'corners of frame {b}, shape {host.shape[1:]}, K {K}')
    return meta, words


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_equals_the_definition_on_random_maps(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    cap = 4 * shape[0] * shape[1]
    for K in (1, 3, 254):
        noise = rng.integers(0, K + 1, size=(2,) + shape).astype(np.uint8)          # every pixel its own label: corners everywhere
        _check(noise, K, cap)
        blocks = np.repeat(np.repeat(rng.integers(0, K + 1, size=(1, -(-shape[0] // 5), -(-shape[1] // 3))), 5, 1), 3, 2)
        _check(blocks[:, :shape[0], :shape[1]].astype(np.uint8), K, cap)            # edges that cross rows, columns and tiles


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_on_full_empty_and_corner_frames(shape):
    H, W = shape
    full, empty = np.full(shape, 2, np.uint8), np.zeros(shape, np.uint8)
    pixels = empty.copy()
    pixels[0, 0] = pixels[0, -1] = pixels[-1, 0] = pixels[-1, -1] = 1               # one pixel at each image corner
    above = np.where(np.arange(H * W).reshape(shape) % 3 == 0, 255, 1).astype(np.uint8)   # 255 is above K: part of no region
    meta, words = _check(np.stack([full, empty, pixels]), 3)                        # B = 3 with the empty frame in the middle
    assert tuple(meta[0, 1]) == (4, 1) and not meta[0, (0, 2)].any()
    assert words[0].tolist() == [1 << 31, W, W | H << 16, H << 16]
    assert not meta[1].any() and len(words[1]) == 0
    _check(above[None], 3, 4 * H * W)


def test_kernel_on_an_odd_base_pointer_and_an_odd_width():
    rng = np.random.default_rng(5)
    maps = rng.integers(0, 4, size=(2, 70, 129)).astype(np.uint8)
    aligned = torch.from_numpy(maps).cuda()
    store = torch.empty(maps.size + 1, dtype=torch.uint8, device='cuda')
    odd = store[1:].view(maps.shape)
    odd.copy_(aligned)
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    a, b = _check(aligned, 3, 4 * 70 * 129), _check(odd, 3, 4 * 70 * 129)
    np.testing.assert_array_equal(a[0], b[0])
    from xmem2_amd import ops
    one = ops.mask_polygons(odd[0], 3, 4 * 70 * 129)                                # [H,W] is a batch of one
    assert one[0].shape == (1, 3, 2)
    np.testing.assert_array_equal(one[0][0], a[0][0])
    np.testing.assert_array_equal(one[1][0], a[1][0])


def test_both_ranking_paths_agree():
    """Up to 4096 corners of capacity a frame is ranked by one workgroup in LDS, above that in rounds on global arrays."""
    rng = np.random.default_rng(11)
    maps = rng.integers(0, 4, size=(2, 44, 45)).astype(np.uint8)                    # 3652 and 3718 corners (polygons.record_host)
    lds, glb = _check(maps, 3, 4096), _check(maps, 3, 4097)
    assert lds[0][:, :, 0].sum(axis=1).tolist() == [3652, 3718]                     # more than three corners per thread of the workgroup
    np.testing.assert_array_equal(lds[0], glb[0])
    for x, y in zip(lds[1], glb[1]):
        np.testing.assert_array_equal(x, y)


def test_ops_mask_polygons_validates():
    from xmem2_amd import ops
    m = torch.zeros((4, 4), dtype=torch.uint8, device='cuda')
    for bad_k in (0, 255, True, 1.0):
        with pytest.raises(ValueError):
            ops.mask_polygons(m, bad_k)
    with pytest.raises(ValueError):
        ops.mask_polygons(m, 1, capacity=0)
    with pytest.raises(RuntimeError):
        ops.mask_polygons(m.float(), 1)
    with pytest.raises(RuntimeError):
        ops.mask_polygons(m[None, None], 1)


# ---- 2. saddles and long rings ---------------------------------------------------------------------------------------------------
def test_checkerboard_and_its_complement():
    yy, xx = np.mgrid[:33, :65]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)
    meta, words = _check(np.stack([board, 1 - board]), 1, 4 * 33 * 65)
    assert tuple(meta[0, 0]) == (4292, 977)
    assert int((words[0] >> 31).sum()) == 977


@pytest.mark.parametrize('anti', [False, True])
def test_a_diagonal_of_1500_pixels_is_one_ring_of_6000_corners(anti):
    """Every inner vertex is a saddle, visited twice; the ring is longer than a workgroup and needs 13 rounds of pointer jumping."""
    from xmem2_amd import polygons
    n = 1500
    diag = np.eye(n, dtype=np.uint8)
    if anti:
        diag = np.ascontiguousarray(diag[:, ::-1])
    assert polygons.default_capacity(n, n) == 4 * n
    meta, words = _check(diag[None], 1)
    assert tuple(meta[0, 0]) == (4 * n, 1) and int((words[0] >> 31).sum()) == 1


def test_a_ring_inside_a_hole_inside_a_ring():
    m = np.zeros((9, 9), np.uint8)
    m[1:8, 1:8] = 1
    m[2:7, 2:7] = 0
    m[3:6, 3:6] = 1
    m[4, 4] = 2
    meta, words = _check(m[None], 2)
    assert meta[0].tolist() == [[16, 4], [4, 1]]


# ---- 3. real annotations and the component count -----------------------------------------------------------------------------
def _chair_maps():
    from PIL import Image
    ann = os.path.join(CHAIR, 'Annotations')
    return np.stack([np.array(Image.open(os.path.join(ann, n)).convert('P'), np.uint8) for n in sorted(os.listdir(ann))])


def test_the_chair_annotations_and_their_components():
    from xmem2_amd import ops, polygons
    maps = _chair_maps()
    assert maps.shape == (10, 480, 720)
    three = maps.copy()                                               # three labels, different contents per frame
    three[:, :200][three[:, :200] == 1] = 3
    three[:, :, 500:] = 2
    K = 3
    meta, words = _check(three, K)
    assert 0 < meta[:, :, 0].sum(axis=1).min() and meta[:, :, 0].sum(axis=1).max() < polygons.default_capacity(480, 720)
    root, _ = ops.components(torch.from_numpy(three).cuda(), connectivity=8)
    root = root.cpu().numpy()
    for b in range(len(three)):
        for k, rings in enumerate(polygons.label_rings(meta[b], words[b]), start=1):
            outer = sum(polygons.area2(r) > 0 for r in rings)
            assert outer == len(np.unique(root[b][three[b] == k])), (b, k)
    plain_meta, _ = _check(maps, 1)
    assert 4 <= plain_meta[:, 0, 1].min() and plain_meta[:, 0, 1].max() <= 6          # 4-6 rings per frame
    assert 342 <= plain_meta[:, 0, 0].min() and plain_meta[:, 0, 0].max() <= 486      # 342-486 corners per frame


# ---- 4. overflow and determinism ---------------------------------------------------------------------------------------------
def test_overflow_keeps_the_true_counts_and_is_traced_again(monkeypatch):
    from xmem2_amd import ops, polygons
    yy, xx = np.mgrid[:33, :65]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)
    tiny = np.zeros((33, 65), np.uint8)
    tiny[3, 3] = 1                                                    # 4 corners: fits
    maps = torch.from_numpy(np.stack([board, tiny])).cuda()
    want = [polygons.record_host(m, 1) for m in (board, tiny)]
    rec = ops.mask_polygons(maps, 1, capacity=4291, wait=False).cpu().numpy()
    meta, corners = polygons.split_record(rec, 2, 1, 4291)
    np.testing.assert_array_equal(meta[0], want[0][0])                # the true counts, corners and rings, though nothing fitted
    np.testing.assert_array_equal(meta[1], want[1][0])
    np.testing.assert_array_equal(corners[1, :4], want[1][1])
    calls, original = [], ops.mask_polygons

    def spy(masks, K, capacity=None, wait=True):
        calls.append((tuple(masks.shape), capacity))
        return original(masks, K, capacity, wait)
    monkeypatch.setattr(ops, 'mask_polygons', spy)
    retries = ops.POLY_STATS['retries']
    meta, words = ops.mask_polygons(maps, 1, capacity=4291)
    assert calls == [((2, 33, 65), 4291), ((1, 33, 65), 4292)]
    assert ops.POLY_STATS['retries'] == retries + 1
    for b in range(2):
        np.testing.assert_array_equal(meta[b], want[b][0])
        np.testing.assert_array_equal(words[b], want[b][1])             # the whole frame, nothing cut off


def test_two_runs_give_the_same_bytes():
    from xmem2_amd import ops, polygons
    rng = np.random.default_rng(9)
    maps = torch.from_numpy(rng.integers(0, 6, size=(3, 130, 200)).astype(np.uint8)).cuda()
    K, cap = 5, 4 * 130 * 200
    recs = [ops.mask_polygons(maps, K, cap, wait=False).cpu().numpy() for _ in range(2)]
    used = []
    for rec in recs:
        meta, corners = polygons.split_record(rec, 3, K, cap)
        used.append(meta.tobytes() + b''.join(corners[b, :meta[b, :, 0].sum()].tobytes() for b in range(3)))
    assert used[0] == used[1] and len(used[0]) > 3 * K * polygons.META * 4


# ---- 5. the product ------------------------------------------------------------------------------------------------------------
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
    calls, original = [], ops.mask_polygons

    def spy(masks, K, capacity=None, wait=True):
        calls.append((tuple(masks.shape), K, wait))
        return original(masks, K, capacity, wait)
    monkeypatch.setattr(ops, 'mask_polygons', spy)
    return calls


def _without_polygons(doc):
    doc = json.loads(json.dumps(doc))
    assert doc['videos'][0].pop('polygons')['fill'] == 'evenodd'
    for ann in doc['annotations']:
        for seg in ann['segmentations']:
            if seg is not None:
                seg.pop('polygons')
    return doc


def _assert_polygons_fill_to_the_pngs(doc, masks_dir, first_annotation):
    """every frame rebuilt from the `polygons` entries alone, colour-mapped as the writers do == the written PNG, pixel for pixel"""
    from PIL import Image
    from xmem2_amd import polygons
    (video,) = doc['videos']
    h, w = video['height'], video['width']
    ref = Image.open(first_annotation).convert('P')
    entries = 0
    for t, name in enumerate(video['file_names']):
        ids = np.zeros((h, w), np.uint8)
        for ann in doc['annotations']:
            seg = ann['segmentations'][t]
            if seg is not None:
                region = polygons.fill_host(seg['polygons'], h, w)
                assert int(region.sum()) == ann['areas'][t]
                ids[region] = ann['label']
                entries += 1
        png = Image.open(os.path.join(masks_dir, name[:-4] + '.png'))
        want = Image.fromarray(ids).quantize(palette=ref, dither=Image.Dither.NONE).convert('RGB')    # VideoReader.map_the_colors_back
        np.testing.assert_array_equal(np.array(want), np.array(png), err_msg=name)
    return entries


def test_run_on_video_with_polygons_on_the_chair_clip(checkpoint, net, tmp_path, monkeypatch):
    from xmem2_amd import polygons
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = _chair(tmp_path / 'clip', 3)
    first = os.path.join(msks, names[0][:-4] + '.png')
    calls = _spy(monkeypatch)
    common = dict(frames_with_masks=[0], print_progress=False, save_overlay=False, network=net)

    def run(tag, **config):
        run_on_video(imgs, msks, str(tmp_path / tag), overwrite_config=dict(config, model=checkpoint, save_tracks=True), **common)
        return open(tmp_path / tag / 'tracks.json', 'rb').read()
    plain = run('plain')                                              # a run that never heard of the option
    assert run('off', tracks_polygons=None) == plain and calls == []  # off: never called, the file byte for byte
    on = json.loads(run('on', tracks_polygons=True))
    assert calls == [((480, 720), 1, False)] * 3                      # one launch sequence per frame, no waiting
    assert _mask_bytes(tmp_path / 'on') == _mask_bytes(tmp_path / 'plain')                     # the PNGs: byte-identical
    assert on['videos'][0]['polygons'] == {'tolerance': 0, 'fill': 'evenodd'}
    assert _without_polygons(on) == json.loads(plain)                 # counts, sizes, boxes and areas are unchanged
    assert _assert_polygons_fill_to_the_pngs(on, tmp_path / 'on' / 'masks', first) == 3
    del calls[:]
    loose = json.loads(run('loose', tracks_polygons={'tolerance': 1.5}, tracks_counts='compressed'))
    assert len(calls) == 3 and loose['videos'][0]['polygons'] == {'tolerance': 1.5, 'fill': 'evenodd'}
    (a_on,), (a_loose,) = on['annotations'], loose['annotations']
    fewer = 0
    for s_on, s_loose in zip(a_on['segmentations'], a_loose['segmentations']):
        exact = [list(zip(r[0::2], r[1::2])) for r in s_on['polygons']]
        assert s_loose['polygons'] == [polygons.flat(polygons.simplify(r, 1.5)) for r in exact]
        fewer += sum(map(len, s_loose['polygons'])) < sum(map(len, s_on['polygons']))
    assert fewer == 3
    # the tool adds to the plain file what the frame loop wrote: traced from the decoded tracks, on the device
    out = tmp_path / 'tool.json'
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))] +
                                                      os.environ.get('PYTHONPATH', '').split(os.pathsep)))
    done = subprocess.run([sys.executable, '-m', 'xmem2_amd.rle', '--tracks', str(tmp_path / 'plain' / 'tracks.json'), '--polygons',
                           '--out', str(out)], capture_output=True, text=True, env=env, timeout=300)
    assert done.returncode == 0, done.stderr
    assert json.loads(done.stdout)['polygons'] == {'tolerance': 0, 'fill': 'evenodd'}
    assert json.load(open(out)) == on


def test_a_frame_whose_corners_do_not_fit_is_traced_again_in_the_loop(monkeypatch):
    from xmem2_amd import ops, polygons, rle
    from xmem2_amd.frame_outputs import Tag, _TrackLoop

    class Mapper:
        remappings, labels = {}, [1]
    yy, xx = np.mgrid[:33, :65]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)                     # 4292 corners, the default room is 2048
    quiet = np.zeros((33, 65), np.uint8)
    quiet[3:9, 4:40] = 1
    loop = _TrackLoop('list', True)
    retries = ops.POLY_STATS['retries']
    arrived = []
    for t, m in enumerate((quiet, board, quiet)):
        arrived += loop.submit(Tag(f'{t}.png'), torch.from_numpy(m).cuda(), Mapper)
    arrived += loop.drain()
    assert loop.corners.size == 2048
    for item in arrived:
        loop.finish(item, Mapper)
    assert ops.POLY_STATS['retries'] == retries + 1 and loop.corners.size == 2 * 4292
    doc = loop.writer.to_dict()
    for t, m in enumerate((quiet, board, quiet)):
        seg = doc['annotations'][0]['segmentations'][t]
        assert seg['polygons'] == [polygons.flat(r) for r in polygons.rings_host(m, 1)]
        np.testing.assert_array_equal(rle.decode(seg['counts'], 33, 65), m == 1)


def _write_clip(root, labels=(3, 7), hw=(96, 128), t=5):
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


def test_session_save_tracks_with_polygons(checkpoint, net, tmp_path, monkeypatch):
    from xmem2_amd import polygons
    from xmem2_amd.session import VideoSession
    imgs, msks, names = _write_clip(tmp_path / 'clip')
    s = VideoSession(imgs, msks, overwrite_config={'model': checkpoint, 'size': -1, 'mem_every': 2}, network=net)
    s.save_reference(0)
    s.propagate(0, 'forward', stop=3)                                 # frame 4 has no mask yet
    calls = _spy(monkeypatch)
    plain = open(s.save_tracks(tmp_path / 'plain'), 'rb').read()
    assert calls == []
    monkeypatch.setattr(s, '_host_masks', lambda: pytest.fail('save_tracks must not copy the masks to the host'))
    on = json.load(open(s.save_tracks(tmp_path / 'on', polygons=True)))
    assert calls == [((4, 96, 128), 2, True)]
    assert _without_polygons(on) == json.loads(plain)
    assert [a['label'] for a in on['annotations']] == [3, 7]
    for t in range(5):
        ids = s.mask(t).cpu().numpy() if t < 4 else None
        for ann in on['annotations']:
            seg = ann['segmentations'][t]
            if t == 4:
                assert seg is None
            elif seg is not None:
                np.testing.assert_array_equal(polygons.fill_host(seg['polygons'], 96, 128), ids == ann['label'])
            else:
                assert not (ids == ann['label']).any()
    monkeypatch.undo()
    s.full_propagation()
    s.save(tmp_path / 'full', save_overlay=False)
    s.save_tracks(tmp_path / 'full', polygons={'tolerance': 0})
    s.save(tmp_path / 'ref', save_overlay=False)
    assert _mask_bytes(tmp_path / 'full') == _mask_bytes(tmp_path / 'ref')
    full = json.load(open(tmp_path / 'full' / 'tracks.json'))
    assert _assert_polygons_fill_to_the_pngs(full, tmp_path / 'full' / 'masks', os.path.join(msks, names[0])) >= 5
