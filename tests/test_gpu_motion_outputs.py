"""config['temporal_smooth'] with 'motion' through the frame loop and the session, on the chair clip of tests/golden/chair with the
synthetic network: the written masks are `temporal.mode_mc_host` of the masks a run without smoothing writes and the lumas of the
frames, references locked; without the key the files are those of a run that has never heard of the option.

On this clip the votes change no pixel - the chair's masks do not flicker under the synthetic weights - so the second half of the
file runs every surface on a synthetic clip whose masks do, and asserts that they do.

The clip is the chair clip cropped to the 200 x 236 window round the chair (rows 0..199, columns 176..411: cropped last blocks both
ways): `block_motion_host` takes a second per pair of full 480 x 720 frames and the reference needs eighteen pairs."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import motion_refs as R
from conftest import ROOT
from xmem2_amd import motion, temporal

pytestmark = pytest.mark.gpu

CHAIR = os.path.join(ROOT, 'tests', 'golden', 'chair')
ROWS, COLS = slice(0, 200), slice(176, 412)
GIVEN = [0, 4]
COMMON = dict(frames_with_masks=GIVEN, print_progress=False, save_overlay=False)
SPEC = {'radius': 1, 'motion': True}


@pytest.fixture(scope='module')
def checkpoint(synth_sd, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt') / 'XMem_synth.pth'
    torch.save(synth_sd, path)
    return str(path)


@pytest.fixture(scope='module')
def cfg(checkpoint):
    return {'model': checkpoint, 'size': -1, 'mem_every': 2}


@pytest.fixture(scope='module')
def net(checkpoint):
    from xmem2_amd.network import XMem
    return XMem({'precision': 'fp32'}, checkpoint).to('cuda').eval()


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    """(frames dir, annotations dir, names, lumas uint8 [T,H,W]) of the cropped chair clip, frames written as PNG"""
    root = tmp_path_factory.mktemp('chair')
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(); msks.mkdir()
    names, lumas = [], []
    for f in sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages'))):
        name = f[:-4] + '.png'
        rgb = np.array(Image.open(os.path.join(CHAIR, 'JPEGImages', f)).convert('RGB'))[ROWS, COLS]
        Image.fromarray(rgb).save(imgs / name)
        ann = Image.open(os.path.join(CHAIR, 'Annotations', name))
        cut = Image.fromarray(np.array(ann)[ROWS, COLS], mode='P')
        cut.putpalette(ann.getpalette())
        cut.save(msks / name)
        names.append(name)
        lumas.append(motion.luma_host(rgb))
    return str(imgs), str(msks), names, np.stack(lumas)


def _files(root, sub='masks'):
    return {f: open(os.path.join(str(root), sub, f), 'rb').read() for f in sorted(os.listdir(os.path.join(str(root), sub)))}


def _written_ids(out_dir, names):
    """the written mask PNGs as dense ids (one object: 0 and 1), uint8 [T,H,W]"""
    return np.stack([(np.array(Image.open(os.path.join(str(out_dir), 'masks', n)).convert('RGB')).any(-1)).astype(np.uint8) for n in names])


def _locked(T):
    return [t in GIVEN for t in range(T)]


@pytest.fixture(scope='module')
def runs(cfg, net, clip, tmp_path_factory):
    """run_on_video without the key, with the key None and with the compensated vote, once -> (root, {name: DataFrame})"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names, _ = clip
    root = tmp_path_factory.mktemp('runs')
    dfs = {}
    for name, extra in (('absent', {}), ('none', {'temporal_smooth': None}), ('mc', {'temporal_smooth': dict(SPEC)})):
        dfs[name] = run_on_video(imgs, msks, str(root / name), overwrite_config=dict(cfg, **extra), network=net, **COMMON)
    return root, dfs


@pytest.fixture(scope='module')
def reference(runs, clip):
    """(masks of the run without smoothing, mode_mc_host of them, changed), computed once"""
    off = _written_ids(runs[0] / 'absent', clip[2])
    want, changed = temporal.mode_mc_host(off, clip[3], 1, locked=_locked(len(off)))
    return off, want, changed


def test_without_the_option_nothing_changes(runs, clip):
    root, dfs = runs
    absent = _files(root / 'absent')
    assert len(absent) == len(clip[2]) and _files(root / 'none') == absent
    for off in ('absent', 'none'):
        assert 'temporal_smooth' not in dfs[off].attrs


def test_the_loop_writes_the_compensated_vote_of_the_masks_it_would_have_written(runs, clip, reference):
    root, dfs = runs
    names = clip[2]
    off, want, changed = reference
    assert off.any() and not off.all()
    print(f'pixels changed per frame {changed.tolist()}; by the plain vote {temporal.mode_host(off, 1, locked=_locked(len(off)))[1].tolist()}')
    np.testing.assert_array_equal(_written_ids(root / 'mc', names), want)
    attrs = dfs['mc'].attrs['temporal_smooth']
    assert attrs == {'radius': 1, 'pixels_changed': int(changed.sum()), 'frames_changed': int((changed > 0).sum()),
                     'motion': {'search': 16, 'bias': 1, 'max_sad': 24}}
    assert dfs['mc']['frame'].tolist() == names and dfs['mc']['mask_provided'].tolist() == _locked(len(names))


def test_resize_on_device_takes_the_source_frames(cfg, net, clip, runs, tmp_path):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names, _ = clip
    run_on_video(imgs, msks, str(tmp_path / 'dev'), overwrite_config=dict(cfg, resize_on_device=True, temporal_smooth=dict(SPEC)),
                 network=net, **COMMON)
    assert _files(tmp_path / 'dev') == _files(runs[0] / 'mc')


def test_session_smooth_with_motion(cfg, net, clip):
    from xmem2_amd.session import VideoSession
    imgs, msks, names, lumas = clip
    s = VideoSession(imgs, msks, overwrite_config=dict(cfg), network=net)
    for t in GIVEN:
        s.save_reference(t)
    s.full_propagation()
    before = s.masks.clone()
    want, changed = temporal.mode_mc_host(before.cpu().numpy(), lumas, 1, present=s._present, locked=_locked(len(names)))
    print(f'pixels changed per frame {changed.tolist()}')
    for batch in (3, 64):
        s.masks.copy_(before)
        assert s.smooth(1, batch=batch, motion=True) == changed.tolist()
        np.testing.assert_array_equal(s.masks.cpu().numpy(), want)
    with pytest.raises(ValueError):
        s.smooth(1, motion={'search': 0})


def test_a_resized_run_is_refused_before_any_frame(cfg, net, clip, tmp_path):
    from xmem2_amd.run_on_video import run_on_video
    from xmem2_amd.session import VideoSession
    imgs, msks, names, _ = clip
    with pytest.raises(ValueError, match='resize_on_device'):
        run_on_video(imgs, msks, str(tmp_path / 'small'), overwrite_config=dict(cfg, size=96, temporal_smooth=dict(SPEC)), network=net, **COMMON)
    assert not os.path.isdir(tmp_path / 'small' / 'masks') or not os.listdir(tmp_path / 'small' / 'masks')
    s = VideoSession(imgs, msks, overwrite_config=dict(cfg, size=96), network=net)
    with pytest.raises(ValueError, match="masks' size"):
        s.smooth(1, motion=True)


# ---- the flickering clip -------------------------------------------------------------------------------------------------------------
# The chair's masks do not flicker under the synthetic weights: the votes above change no pixel, so those tests hold the plumbing (every
# frame once, in order, the report, the refusals) and little else.  The clip of motion_refs.make_flicker_clip - two objects, a texture
# that moves a pixel a frame, hundreds of pixels changed per frame - is where every surface is held to `mode_mc_host` with work to do.

MOTION = {'search': 4, 'bias': 1, 'max_sad': 40}


@pytest.fixture(scope='module')
def flicker(tmp_path_factory):
    return R.make_flicker_clip(tmp_path_factory.mktemp('flicker'))


@pytest.fixture(scope='module')
def flicker_off(cfg, net, flicker, tmp_path_factory):
    """the run without smoothing, with its tracks file -> (directory, its masks as dense ids)"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names, _ = flicker
    out = tmp_path_factory.mktemp('flicker_off')
    run_on_video(imgs, msks, str(out), overwrite_config=dict(cfg, save_tracks=True), network=net, **dict(COMMON, frames_with_masks=R.FLICKER_GIVEN))
    return out, R.flicker_written_ids(out, names)


def _want(off, lumas, r, **kw):
    want, changed = temporal.mode_mc_host(off, lumas, r, locked=R.flicker_locked(), **kw)
    print(f'r = {r} {kw}: pixels changed per frame {changed.tolist()}')
    assert changed.sum() > 0, 'the vote changes nothing on this clip: the test shows nothing'
    return want, changed


@pytest.mark.parametrize('r', [1, 2])
def test_the_loop_on_a_clip_whose_masks_flicker(cfg, net, flicker, flicker_off, tmp_path, r):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names, lumas = flicker
    df = run_on_video(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(cfg, temporal_smooth={'radius': r, 'motion': dict(MOTION)}),
                      network=net, **dict(COMMON, frames_with_masks=R.FLICKER_GIVEN))
    want, changed = _want(flicker_off[1], lumas, r, **MOTION)
    np.testing.assert_array_equal(R.flicker_written_ids(tmp_path / 'on', names), want)
    assert df.attrs['temporal_smooth'] == {'radius': r, 'pixels_changed': int(changed.sum()), 'frames_changed': int((changed > 0).sum()),
                                           'motion': MOTION}


def test_resize_on_device_searches_the_source_frames_of_a_resized_run(cfg, net, flicker, tmp_path):
    """the working size is 64 x 85, the masks and the motion search are 96 x 128: the lumas come from `src_u8`"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names, lumas = flicker
    small = dict(cfg, size=64, resize_on_device=True)
    common = dict(COMMON, frames_with_masks=R.FLICKER_GIVEN)
    run_on_video(imgs, msks, str(tmp_path / 'off'), overwrite_config=dict(small), network=net, **common)
    run_on_video(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(small, temporal_smooth={'radius': 1, 'motion': dict(MOTION)}),
                 network=net, **common)
    want, _ = _want(R.flicker_written_ids(tmp_path / 'off', names), lumas, 1, **MOTION)
    np.testing.assert_array_equal(R.flicker_written_ids(tmp_path / 'on', names), want)


def test_session_smooth_with_motion_on_a_clip_whose_masks_flicker(cfg, net, flicker):
    from xmem2_amd.session import VideoSession
    imgs, msks, names, lumas = flicker
    s = VideoSession(imgs, msks, overwrite_config=dict(cfg), network=net)
    for t in R.FLICKER_GIVEN:
        s.save_reference(t)
    s.full_propagation()
    before = s.masks.clone()
    assert all(s._present)
    want, changed = _want(before.cpu().numpy(), lumas, 2, **MOTION)
    for batch in (3, 64):                                                        # 3: batch boundaries inside the clip, a halo of 2
        s.masks.copy_(before)
        assert s.smooth(2, batch=batch, motion=dict(MOTION)) == changed.tolist(), batch
        np.testing.assert_array_equal(s.masks.cpu().numpy(), want, err_msg=f'batch {batch}')


def _tracks_ids(tracks, names, tmp):
    """a tracks file decoded to index PNGs by the command line, uint8 [T,H,W] of labels"""
    from xmem2_amd import rle
    assert rle.main(['--tracks', str(tracks), '--out', str(tmp)]) == 0
    return np.stack([np.array(Image.open(os.path.join(str(tmp), n))) for n in names])


def test_rle_smooth_with_motion_on_a_file_that_exists(flicker, flicker_off, tmp_path, capsys):
    import json
    from xmem2_amd import rle
    imgs, _, names, lumas = flicker
    out, off = flicker_off
    tracks = str(out / 'tracks.json')
    want, changed = _want(off, lumas, 2, **MOTION)
    doc, got_changed = rle.smooth_tracks(tracks, 2, locked=R.FLICKER_GIVEN, batch=3, motion=dict(MOTION), lumas=imgs)   # batches with a halo
    assert got_changed == changed.tolist()
    rle.write_json(doc, str(tmp_path / 'batch3.json'))
    np.testing.assert_array_equal(_tracks_ids(tmp_path / 'batch3.json', names, tmp_path / 'b3'), R.FLICKER_LUT[want])
    # the command line: its search range, the default bias and max_sad
    want, changed = _want(off, lumas, 2, search=4)
    capsys.readouterr()
    assert rle.main(['--tracks', tracks, '--smooth', '2', '--lock', '0,4', '--motion', imgs, '--motion-search', '4',
                     '--out', str(tmp_path / 'cli.json')]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report['motion'] == {'search': 4, 'bias': 1, 'max_sad': 24} and report['pixels_changed'] == int(changed.sum())
    np.testing.assert_array_equal(_tracks_ids(tmp_path / 'cli.json', names, tmp_path / 'cli'), R.FLICKER_LUT[want])
    (tmp_path / 'frames').mkdir()
    with pytest.raises(ValueError, match='0 frames'):
        rle.smooth_tracks(tracks, 2, motion=True, lumas=str(tmp_path / 'frames'))
