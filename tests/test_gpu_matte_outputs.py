"""config['mattes'] through every output path, on a synthetic clip (5 frames of 96 x 128, two objects whose labels are 2 and 5) with
the synthetic network: the planes run_on_video writes are `table[signed_d2_host(.)]` of the mask PNGs it writes, per label; masks and
tracks are the bytes of a run that has never heard of the option, with it off and with it on; VideoSession.save_mattes and
`python -m xmem2_amd.matte` (--tracks and --masks) write the loop's files; `python -m xmem2_amd.rle --grow` gives `grow_host` of the
written masks; VideoSession.grow is `ops.grow_masks` in place."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from xmem2_amd import matte

pytestmark = pytest.mark.gpu

T_CLIP, HW = 5, (96, 128)
LABELS = (2, 5)                                               # dense ids 1 and 2: the directories carry the labels, not the ids
COLOURS = {2: (200, 0, 0), 5: (0, 200, 0)}
SPEC = {'feather': 3, 'trimap': 2}
COMMON = dict(frames_with_masks=[0], print_progress=False, save_overlay=False)


@pytest.fixture(scope='module')
def checkpoint(synth_sd, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt') / 'XMem_synth.pth'
    torch.save(synth_sd, path)
    return str(path)


@pytest.fixture(scope='module')
def cfg(checkpoint):
    return {'model': checkpoint, 'size': -1, 'mem_every': 2, 'save_tracks': True}


@pytest.fixture(scope='module')
def net(checkpoint):
    from xmem2_amd.network import XMem
    return XMem({'precision': 'fp32'}, checkpoint).to('cuda').eval()


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    root = tmp_path_factory.mktemp('clip')
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(); msks.mkdir()
    frames, masks = synthetic_frames(T_CLIP, *HW, seed=1234), synthetic_masks(T_CLIP, 2, *HW)
    pal = [0] * 768
    for lab, rgb in COLOURS.items():
        pal[3 * lab:3 * lab + 3] = rgb
    names = [f'frame_{i:06d}.png' for i in range(T_CLIP)]
    for i, name in enumerate(names):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(imgs / name)
        idx = np.zeros(HW, np.uint8)
        for o, lab in enumerate(LABELS):
            idx[masks[i, o] > 0] = lab
        im = Image.fromarray(idx, mode='P'); im.putpalette(pal); im.save(msks / name)
    return str(imgs), str(msks), names


def _files(root, subs=('masks',)):
    """{relative path: bytes} of everything under the given sub-directories of `root`"""
    out = {}
    for sub in subs:
        for d, _, files in os.walk(os.path.join(str(root), sub)):
            for f in files:
                out[os.path.relpath(os.path.join(d, f), str(root))] = open(os.path.join(d, f), 'rb').read()
    return out


def _written_ids(out_dir, names):
    """the written mask PNGs mapped to dense ids"""
    ids = []
    for n in names:
        rgb = np.array(Image.open(os.path.join(str(out_dir), 'masks', n)).convert('RGB'))
        m = np.zeros(HW, np.uint8)
        for dense, lab in enumerate(LABELS, start=1):
            m[(rgb == np.array(COLOURS[lab], np.uint8)).all(-1)] = dense
        assert ((m > 0) == rgb.any(-1)).all(), n
        ids.append(m)
    return ids


def _want_planes(ids, names, spec=SPEC):
    """{relative path: uint8 [H, W]} by the definition"""
    parsed = matte.parse_mattes(spec)
    want = {}
    for n, m in zip(names, ids):
        for sub, planes in matte.planes_host(m, len(LABELS), parsed).items():
            for lab, plane in zip(LABELS, planes):
                want[os.path.join(sub, str(lab), n)] = plane
    return want


def _check_planes(root, want):
    got = _files(root, matte.OUTPUTS)
    assert sorted(got) == sorted(want)
    for rel, plane in want.items():
        img = Image.open(os.path.join(str(root), rel))
        assert img.mode == 'L' and img.size == HW[::-1], rel
        np.testing.assert_array_equal(np.array(img), plane, err_msg=rel)
    return got


@pytest.fixture(scope='module')
def runs(cfg, net, clip, tmp_path_factory):
    """run_on_video without the key, with the key None and with the option on, once"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    root = tmp_path_factory.mktemp('runs')
    for name, extra in (('absent', {}), ('none', {'mattes': None}), ('on', {'mattes': dict(SPEC)})):
        run_on_video(imgs, msks, str(root / name), overwrite_config=dict(cfg, **extra), network=net, **COMMON)
    return root


def test_the_loop_writes_the_definition_of_its_own_masks(runs, clip):
    names = clip[2]
    ids = _written_ids(runs / 'on', names)
    print('pixels per frame of the two objects:', [(int((m == 1).sum()), int((m == 2).sum())) for m in ids])
    assert any((m == 1).any() for m in ids) and any((m == 2).any() for m in ids), 'an object is in no frame: the test shows too little'
    want = _want_planes(ids, names)
    assert len(want) == 2 * len(LABELS) * T_CLIP
    soft = sum(int(((p > 0) & (p < 255)).sum()) for rel, p in want.items() if rel.startswith('mattes'))
    unknown = sum(int((p == 128).sum()) for rel, p in want.items() if rel.startswith('trimaps'))
    print('soft matte pixels:', soft, 'unknown trimap pixels:', unknown)
    assert soft > 0 and unknown > 0
    _check_planes(runs / 'on', want)


def test_masks_and_tracks_are_untouched(runs):
    absent = _files(runs / 'absent')
    assert len(absent) == T_CLIP
    tracks = open(runs / 'absent' / 'tracks.json', 'rb').read()
    for other in ('none', 'on'):
        assert _files(runs / other) == absent, other
        assert open(runs / other / 'tracks.json', 'rb').read() == tracks, other
    for off in ('absent', 'none'):
        assert sorted(os.listdir(runs / off)) == ['masks', 'tracks.json']
    assert sorted(os.listdir(runs / 'on')) == ['masks', 'mattes', 'tracks.json', 'trimaps']


def test_options_of_the_loop(cfg, net, clip, runs, tmp_path):
    from xmem2_amd.run_on_video import run_on_video, run_on_video_ensemble
    imgs, msks, names = clip
    ids = _written_ids(runs / 'on', names)
    # trimaps only, no mask PNGs: the planes have writers of their own
    over = dict(cfg, mattes={'feather': None, 'trimap': 4}, save_masks=False)
    run_on_video(imgs, msks, str(tmp_path / 'tri'), overwrite_config=over, network=net, **COMMON)
    assert sorted(os.listdir(tmp_path / 'tri')) == ['tracks.json', 'trimaps']
    _check_planes(tmp_path / 'tri', _want_planes(ids, names, {'feather': None, 'trimap': 4}))
    with pytest.raises(ValueError, match='mattes'):
        run_on_video(imgs, msks, str(tmp_path / 'bad'), overwrite_config=dict(cfg, mattes={'feather': -1}), network=net, **COMMON)
    # the ensemble: the planes of the merged masks it writes
    run_on_video_ensemble(imgs, msks, str(tmp_path / 'ens'), overwrite_config=dict(cfg, mattes=True), network=net, **COMMON)
    _check_planes(tmp_path / 'ens', _want_planes(_written_ids(tmp_path / 'ens', names), names, True))


def test_session_save_mattes_and_grow(cfg, net, clip, runs, tmp_path):
    from xmem2_amd import ops
    from xmem2_amd.session import VideoSession
    imgs, msks, names = clip
    s = VideoSession(imgs, msks, overwrite_config={k: v for k, v in cfg.items() if k != 'save_tracks'}, network=net)
    s.save_reference(0)
    s.full_propagation()
    assert s.save_mattes(tmp_path / 'session', batch=2, **SPEC) == 2 * len(LABELS) * T_CLIP
    assert _files(tmp_path / 'session', matte.OUTPUTS) == _files(runs / 'on', matte.OUTPUTS)       # the files of the loop
    assert sorted(os.listdir(tmp_path / 'session')) == ['mattes', 'trimaps']
    s.save_mattes(tmp_path / 'default')
    ids = [s.masks[t].cpu().numpy() for t in range(T_CLIP)]         # dense ids (`mask(t)` carries the labels)
    _check_planes(tmp_path / 'default', _want_planes(ids, names, True))
    with pytest.raises(ValueError, match='mattes'):
        s.save_mattes(tmp_path / 'bad', blur=1)
    before = s.masks.clone()
    s.grow(2.5, batch=2)
    for t in range(T_CLIP):
        np.testing.assert_array_equal(s.masks[t].cpu().numpy(), matte.grow_host(ids[t], 2.5), err_msg=names[t])
    s.grow(-3)
    assert torch.equal(s.masks, ops.grow_masks(ops.grow_masks(before, 2.5), -3))


def test_the_tools_on_results_that_exist(runs, clip, tmp_path):
    from xmem2_amd import rle
    msks, names = clip[1], clip[2]
    tracks = str(runs / 'absent' / 'tracks.json')
    labels = _written_ids(runs / 'absent', names)
    lut = np.array((0,) + LABELS, np.uint8)
    original = [lut[m] for m in labels]                              # the masks with the annotation's labels, as the tracks carry them
    # rle --grow, then rle --out DIR: grow_host of the original masks, both signs
    for r in (3, -2.5):
        grown = str(tmp_path / f'grow{r}' / 'tracks.json')
        assert rle.main(['--tracks', tracks, '--grow', str(r), '--out', grown]) == 0
        assert rle.main(['--tracks', grown, '--out', str(tmp_path / f'grow{r}' / 'png')]) == 0
        for n, m in zip(names, original):
            got = np.array(Image.open(tmp_path / f'grow{r}' / 'png' / n))
            np.testing.assert_array_equal(got, matte.grow_host(m, r), err_msg=f'{n} r={r}')
        doc_areas = {a['label']: a['areas'] for a in json.load(open(grown))['annotations']}
        for lab in LABELS:                                           # areas are re-encoded from the grown masks
            assert doc_areas[lab] == [int((matte.grow_host(m, r) == lab).sum()) for m in original]
    # python -m xmem2_amd.matte: --tracks and --masks agree with each other, and with the loop
    args = ['--feather', '3', '--trimap', '2']
    assert matte.main(['--tracks', tracks, '--out', str(tmp_path / 'from_tracks')] + args) == 0
    assert rle.main(['--tracks', tracks, '--out', str(tmp_path / 'png')]) == 0
    assert matte.main(['--masks', str(tmp_path / 'png'), '--out', str(tmp_path / 'from_masks')] + args) == 0
    a, b = _files(tmp_path / 'from_tracks', matte.OUTPUTS), _files(tmp_path / 'from_masks', matte.OUTPUTS)
    assert len(a) == 2 * len(LABELS) * T_CLIP and a == b == _files(runs / 'on', matte.OUTPUTS)
    # the colour PNGs of run_on_video, their labels named by the annotation's palette
    assert matte.main(['--masks', str(runs / 'absent' / 'masks'), '--palette-from', os.path.join(msks, names[0]), '--out',
                       str(tmp_path / 'from_rgb')] + args) == 0
    assert _files(tmp_path / 'from_rgb', matte.OUTPUTS) == a
    with pytest.raises(ValueError, match='palette-from'):
        matte.main(['--masks', str(runs / 'absent' / 'masks'), '--out', str(tmp_path / 'no_palette')] + args)
