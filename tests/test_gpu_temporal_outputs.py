"""config['temporal_smooth'] through every output path, on a synthetic clip (10 frames of 96 x 128, two objects whose labels are 2 and
5, frames 0 and 4 annotated) with the synthetic network: without the key, and with it None, the files are those of a run that has
never heard of the option; with it on, the written masks, the tracks and the mattes are those of `temporal.mode_host` of the masks the
off-run writes, with the annotated frames locked.  VideoSession.smooth and `python -m xmem2_amd.rle --smooth` give the same masks
from results that exist."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from xmem2_amd import matte, temporal

pytestmark = pytest.mark.gpu

T_CLIP, HW = 10, (96, 128)
LABELS = (2, 5)                                               # dense ids 1 and 2
COLOURS = {2: (200, 0, 0), 5: (0, 200, 0)}
GIVEN = [0, 4]
COMMON = dict(frames_with_masks=GIVEN, print_progress=False, save_overlay=False)
LUT = np.array((0,) + LABELS, np.uint8)


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


def _make_clip(root, T):
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(); msks.mkdir()
    frames, masks = synthetic_frames(T, *HW, seed=1234), synthetic_masks(T, 2, *HW)
    pal = [0] * 768
    for lab, rgb in COLOURS.items():
        pal[3 * lab:3 * lab + 3] = rgb
    names = [f'frame_{i:06d}.png' for i in range(T)]
    for i, name in enumerate(names):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(imgs / name)
        idx = np.zeros(HW, np.uint8)
        for o, lab in enumerate(LABELS):
            idx[masks[i, o] > 0] = lab
        im = Image.fromarray(idx, mode='P'); im.putpalette(pal); im.save(msks / name)
    return str(imgs), str(msks), names


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    return _make_clip(tmp_path_factory.mktemp('clip'), T_CLIP)


def _files(root, subs=('masks',)):
    out = {}
    for sub in subs:
        for d, _, files in os.walk(os.path.join(str(root), sub)):
            for f in files:
                out[os.path.relpath(os.path.join(d, f), str(root))] = open(os.path.join(d, f), 'rb').read()
    return out


def _written_ids(out_dir, names):
    """the written mask PNGs mapped to dense ids, uint8 [T,H,W]"""
    ids = []
    for n in names:
        rgb = np.array(Image.open(os.path.join(str(out_dir), 'masks', n)).convert('RGB'))
        m = np.zeros(HW, np.uint8)
        for dense, lab in enumerate(LABELS, start=1):
            m[(rgb == np.array(COLOURS[lab], np.uint8)).all(-1)] = dense
        assert ((m > 0) == rgb.any(-1)).all(), n
        ids.append(m)
    return np.stack(ids)


def _tracks_ids(tracks, names, tmp):
    """a tracks file decoded to index PNGs by the command line, uint8 [T,H,W] of LABELS"""
    from xmem2_amd import rle
    assert rle.main(['--tracks', str(tracks), '--out', str(tmp)]) == 0
    return np.stack([np.array(Image.open(os.path.join(str(tmp), n))) for n in names])


def _locked(T=T_CLIP):
    return [t in GIVEN for t in range(T)]


@pytest.fixture(scope='module')
def runs(cfg, net, clip, tmp_path_factory):
    """run_on_video without the key, with the key None, and with radius 1 and 2, once; -> (root, {name: DataFrame})"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    root = tmp_path_factory.mktemp('runs')
    dfs = {}
    for name, extra in (('absent', {}), ('none', {'temporal_smooth': None}), ('r1', {'temporal_smooth': 1}), ('r2', {'temporal_smooth': {'radius': 2}})):
        dfs[name] = run_on_video(imgs, msks, str(root / name), overwrite_config=dict(cfg, **extra), network=net, **COMMON)
    return root, dfs


def test_without_the_option_nothing_changes(runs):
    root, dfs = runs
    absent = _files(root / 'absent')
    assert len(absent) == T_CLIP
    assert _files(root / 'none') == absent
    assert open(root / 'none' / 'tracks.json', 'rb').read() == open(root / 'absent' / 'tracks.json', 'rb').read()
    for off in ('absent', 'none'):
        assert sorted(os.listdir(root / off)) == ['masks', 'tracks.json'] and 'temporal_smooth' not in dfs[off].attrs


@pytest.mark.parametrize('name, r', [('r1', 1), ('r2', 2)])
def test_the_loop_writes_the_vote_of_the_masks_it_would_have_written(runs, clip, name, r, tmp_path):
    root, dfs = runs
    names = clip[2]
    off = _written_ids(root / 'absent', names)
    assert (off == 1).any() and (off == 2).any(), 'an object is in no frame: the test shows too little'
    want, changed = temporal.mode_host(off, r, locked=_locked())
    print(f'r = {r}: pixels changed per frame {changed.tolist()}')
    assert changed.sum() > 0, 'the vote changes nothing on this clip: the test shows nothing'
    np.testing.assert_array_equal(_written_ids(root / name, names), want)
    assert dfs[name].attrs['temporal_smooth'] == {'radius': r, 'pixels_changed': int(changed.sum()), 'frames_changed': int((changed > 0).sum())}
    assert dfs[name]['frame'].tolist() == names and dfs[name]['mask_provided'].tolist() == _locked()      # every frame once, in order
    np.testing.assert_array_equal(_tracks_ids(root / name / 'tracks.json', names, tmp_path / 'png'), LUT[want])
    doc = json.load(open(root / name / 'tracks.json'))
    assert {a['label']: a['areas'] for a in doc['annotations']} == {lab: [int((m == lab).sum()) for m in LUT[want]] for lab in LABELS}


def test_mattes_are_those_of_the_smoothed_masks(cfg, net, clip, runs, tmp_path):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    spec = {'feather': 3, 'trimap': 2}
    run_on_video(imgs, msks, str(tmp_path / 'both'), overwrite_config=dict(cfg, temporal_smooth=2, mattes=dict(spec)), network=net, **COMMON)
    assert _files(tmp_path / 'both') == _files(runs[0] / 'r2')
    smoothed = _written_ids(tmp_path / 'both', names)
    parsed = matte.parse_mattes(spec)
    got = _files(tmp_path / 'both', matte.OUTPUTS)
    assert len(got) == 2 * len(LABELS) * T_CLIP
    for n, m in zip(names, smoothed):
        for sub, planes in matte.planes_host(m, len(LABELS), parsed).items():
            for lab, plane in zip(LABELS, planes):
                rel = os.path.join(sub, str(lab), n)
                np.testing.assert_array_equal(np.array(Image.open(tmp_path / 'both' / rel)), plane, err_msg=rel)


def test_a_clip_shorter_than_the_radius_and_a_bad_value(cfg, net, tmp_path):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = _make_clip(tmp_path, 2)
    common = dict(COMMON, frames_with_masks=[0])
    run_on_video(imgs, msks, str(tmp_path / 'off'), overwrite_config=dict(cfg), network=net, **common)
    df = run_on_video(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(cfg, temporal_smooth=2), network=net, **common)
    assert sorted(os.listdir(tmp_path / 'on' / 'masks')) == names and df['frame'].tolist() == names
    want, changed = temporal.mode_host(_written_ids(tmp_path / 'off', names), 2, locked=[True, False])
    np.testing.assert_array_equal(_written_ids(tmp_path / 'on', names), want)
    assert df.attrs['temporal_smooth'] == {'radius': 2, 'pixels_changed': int(changed.sum()), 'frames_changed': int((changed > 0).sum())}
    with pytest.raises(ValueError, match='temporal_smooth'):
        run_on_video(imgs, msks, str(tmp_path / 'bad'), overwrite_config=dict(cfg, temporal_smooth=8), network=net, **common)


def test_the_ensemble(cfg, net, clip, tmp_path):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    imgs, msks, names = clip
    run_on_video_ensemble(imgs, msks, str(tmp_path / 'off'), overwrite_config=dict(cfg), network=net, **COMMON)
    df = run_on_video_ensemble(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(cfg, temporal_smooth=2), network=net, **COMMON)
    want, changed = temporal.mode_host(_written_ids(tmp_path / 'off', names), 2, locked=_locked())
    np.testing.assert_array_equal(_written_ids(tmp_path / 'on', names), want)
    assert df.attrs['temporal_smooth']['pixels_changed'] == int(changed.sum())
    print('ensemble: pixels changed', int(changed.sum()))


def test_session_smooth(cfg, net, clip):
    from xmem2_amd.session import VideoSession
    imgs, msks, names = clip
    s = VideoSession(imgs, msks, overwrite_config={k: v for k, v in cfg.items() if k != 'save_tracks'}, network=net)
    for t in GIVEN:
        s.save_reference(t)
    s.full_propagation()
    before = s.masks.clone()
    want, changed = temporal.mode_host(before.cpu().numpy(), 2, present=s._present, locked=_locked())
    assert changed.sum() > 0
    assert s.smooth(2, batch=3) == changed.tolist()
    small = s.masks.clone()
    s.masks.copy_(before)
    assert s.smooth(2, batch=64) == changed.tolist()
    assert torch.equal(s.masks, small)
    np.testing.assert_array_equal(small.cpu().numpy(), want)
    s.masks.copy_(before)
    assert s.smooth(7, batch=1) == temporal.mode_host(before.cpu().numpy(), 7, locked=_locked())[1].tolist()      # a halo of seven batches
    np.testing.assert_array_equal(s.masks.cpu().numpy(), temporal.mode_host(before.cpu().numpy(), 7, locked=_locked())[0])
    with pytest.raises(ValueError):
        s.smooth(0)


def test_rle_smooth_on_a_file_that_exists(runs, clip, tmp_path):
    from xmem2_amd import rle
    root, names = runs[0], clip[2]
    tracks = str(root / 'absent' / 'tracks.json')
    in_loop = _tracks_ids(root / 'r2' / 'tracks.json', names, tmp_path / 'loop')
    doc, changed = rle.smooth_tracks(tracks, 2, locked=GIVEN, batch=3)            # a batch smaller than the clip, with its halo
    rle.write_json(doc, str(tmp_path / 'batch3.json'))
    np.testing.assert_array_equal(_tracks_ids(tmp_path / 'batch3.json', names, tmp_path / 'b3'), in_loop)
    want_changed = temporal.mode_host(_written_ids(root / 'absent', names), 2, locked=_locked())[1]
    assert changed == want_changed.tolist()
    assert rle.main(['--tracks', tracks, '--smooth', '2', '--lock', '0,4', '--out', str(tmp_path / 'cli.json')]) == 0
    assert json.load(open(tmp_path / 'cli.json')) == json.load(open(tmp_path / 'batch3.json'))
    assert not rle.TrackReader(str(tmp_path / 'cli.json')).all_compressed()
    # a compressed file stays compressed
    assert rle.main(['--tracks', tracks, '--recode', 'compressed', '--out', str(tmp_path / 'c.json')]) == 0
    assert rle.main(['--tracks', str(tmp_path / 'c.json'), '--smooth', '2', '--lock', '0,4', '--out', str(tmp_path / 'cs.json')]) == 0
    assert rle.TrackReader(str(tmp_path / 'cs.json')).all_compressed()
    np.testing.assert_array_equal(_tracks_ids(tmp_path / 'cs.json', names, tmp_path / 'cs'), in_loop)
