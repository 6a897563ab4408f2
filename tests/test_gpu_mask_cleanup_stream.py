"""config['mask_cleanup'] through every output path, on the chair clip (10 frames, 480 x 720, one object) with the synthetic network:
what is written with the option on is `mask_cleanup.clean_host` of what is written without it - PNGs of run_on_video, of the ensemble
and of VideoSession.save, the tracks of save_tracks, VideoSession.clean and `python -m xmem2_amd.rle --clean` - and without the option
the bytes are those of a run that has never heard of it."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN
from xmem2_amd import mask_cleanup as M

pytestmark = pytest.mark.gpu

CHAIR = os.path.join(GOLDEN, 'chair')
SPEC = {'min_area': 32, 'max_hole': 32}
COMMON = dict(frames_with_masks=[0], print_progress=False, save_overlay=False)


@pytest.fixture(scope='module')
def checkpoint(synth_sd, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt') / 'XMem_synth.pth'
    torch.save(synth_sd, path)
    return str(path)


@pytest.fixture(scope='module')
def net(checkpoint):
    from xmem2_amd.network import XMem
    return XMem({'precision': 'fp32'}, checkpoint).to('cuda').eval()


@pytest.fixture(scope='module')
def clip(tmp_path_factory):
    root = tmp_path_factory.mktemp('chair')
    names = sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages')))
    assert len(names) == 10
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(); msks.mkdir()
    for nm in names:
        os.symlink(os.path.join(CHAIR, 'JPEGImages', nm), imgs / nm)
        os.symlink(os.path.join(CHAIR, 'Annotations', nm[:-4] + '.png'), msks / (nm[:-4] + '.png'))
    return str(imgs), str(msks), names


def _png_bytes(out_dir):
    d = os.path.join(str(out_dir), 'masks')
    return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


def _png_ids(out_dir, names):
    """the written PNGs as index masks: the clip has one object, so every coloured pixel is label 1"""
    return [np.array(Image.open(os.path.join(str(out_dir), 'masks', n[:-4] + '.png')).convert('RGB')).any(-1).astype(np.uint8) for n in names]


def _cleaned(ids):
    """(clean_host of every mask, the totals of its counters); the totals must show that the clean-up did something"""
    done = [M.clean_host(m, **SPEC) for m in ids]
    totals = np.sum([s for _, s in done], axis=0)
    print('clean_host totals (components removed, pixels removed, holes filled, pixels filled):', totals.tolist())
    assert totals[0] > 0 and totals[2] > 0, 'the clean-up does nothing on this clip: the test shows nothing'
    return [m for m, _ in done], dict(zip(M.STATS, (int(v) for v in totals)))


@pytest.fixture(scope='module')
def single(checkpoint, net, clip, tmp_path_factory):
    """run_on_video without the key: (its PNG bytes, clean_host of its masks, the totals)"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    out = tmp_path_factory.mktemp('single_off')
    run_on_video(imgs, msks, str(out), overwrite_config={'model': checkpoint}, network=net, **COMMON)
    ids = _png_ids(out, names)
    for n, m in zip(names, ids):
        root, area = M.components_host(m, 8)
        root4, area4 = M.components_host(m, 4)
        print(n, 'object components:', sorted(int(area.reshape(-1)[r]) for r in np.unique(root[m > 0])),
              'zero components:', sorted(int(area4.reshape(-1)[r]) for r in np.unique(root4[m == 0])))
    return (_png_bytes(out),) + _cleaned(ids)


def _same_masks(got, want, names):
    for n, a, b in zip(names, got, want):
        np.testing.assert_array_equal(a, b, err_msg=n)


def test_run_on_video(checkpoint, net, clip, single, tmp_path):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    off_bytes, want, totals = single
    df = run_on_video(imgs, msks, str(tmp_path / 'on'), overwrite_config={'model': checkpoint, 'mask_cleanup': dict(SPEC)}, network=net,
                      **COMMON)
    _same_masks(_png_ids(tmp_path / 'on', names), want, names)
    assert df.attrs['cleanup'] == totals and list(df['frame']) == names
    none = run_on_video(imgs, msks, str(tmp_path / 'none'), overwrite_config={'model': checkpoint, 'mask_cleanup': None}, network=net,
                        **COMMON)
    assert _png_bytes(tmp_path / 'none') == off_bytes and 'cleanup' not in none.attrs
    run_on_video(imgs, msks, str(tmp_path / 'noop'), overwrite_config={'model': checkpoint, 'mask_cleanup': {'min_area': 0}}, network=net,
                 **COMMON)
    assert _png_bytes(tmp_path / 'noop') == off_bytes
    with pytest.raises(ValueError, match='mask_cleanup'):
        run_on_video(imgs, msks, str(tmp_path / 'bad'), overwrite_config={'model': checkpoint, 'mask_cleanup': {'min_area': -1}},
                     network=net, **COMMON)


def test_in_loop_tracks_and_the_scorer_see_the_cleaned_mask(checkpoint, net, clip, single, tmp_path):
    from xmem2_amd import rle
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    _, want, totals = single
    over = {'model': checkpoint, 'mask_cleanup': dict(SPEC), 'save_tracks': True, 'save_masks': False}
    df = run_on_video(imgs, msks, str(tmp_path / 'on'), overwrite_config=over, network=net, compute_jf=True, **COMMON)
    assert df.attrs['cleanup'] == totals and not os.path.exists(tmp_path / 'on' / 'masks')
    video, decoded = rle.read_tracks(tmp_path / 'on' / 'tracks.json')
    _same_masks(decoded, want, names)
    (ann,) = json.load(open(tmp_path / 'on' / 'tracks.json'))['annotations']
    assert ann['areas'] == [int(m.sum()) for m in want]
    gt = [(np.array(Image.open(os.path.join(msks, n[:-4] + '.png'))) > 0) for n in names]
    j_ref = [float((g & (w == 1)).sum()) / float((g | (w == 1)).sum()) for w, g in zip(want, gt)]     # one object: J is its IoU
    np.testing.assert_allclose(np.asarray(df['J'], float), j_ref, rtol=0, atol=1e-6)


def test_ensemble(checkpoint, net, clip, tmp_path):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    imgs, msks, names = clip
    over = {'model': checkpoint, 'mem_every': 2}
    run_on_video_ensemble(imgs, msks, str(tmp_path / 'off'), overwrite_config=dict(over), network=net, **COMMON)
    want, totals = _cleaned(_png_ids(tmp_path / 'off', names))
    df = run_on_video_ensemble(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(over, mask_cleanup=dict(SPEC), save_tracks=True),
                               network=net, **COMMON)
    _same_masks(_png_ids(tmp_path / 'on', names), want, names)
    assert df.attrs['cleanup'] == totals
    from xmem2_amd import rle
    _same_masks(rle.read_tracks(tmp_path / 'on' / 'tracks.json')[1], want, names)
    run_on_video_ensemble(imgs, msks, str(tmp_path / 'none'), overwrite_config=dict(over, mask_cleanup=None), network=net, **COMMON)
    assert _png_bytes(tmp_path / 'none') == _png_bytes(tmp_path / 'off')


def test_session(checkpoint, net, clip, tmp_path):
    from xmem2_amd import rle
    from xmem2_amd.session import VideoSession
    imgs, msks, names = clip
    off = VideoSession(imgs, msks, overwrite_config={'model': checkpoint}, network=net)
    off.save_reference(0)
    off.full_propagation()
    off.save(tmp_path / 'off', save_overlay=False)
    off_tracks = off.save_tracks(tmp_path / 'off')
    assert 'cleanup' not in off.stats().attrs
    want, totals = _cleaned(_png_ids(tmp_path / 'off', names))

    on = VideoSession(imgs, msks, overwrite_config={'model': checkpoint, 'mask_cleanup': dict(SPEC)}, network=net)
    on.save_reference(0)
    on.full_propagation()
    on.save(tmp_path / 'on', save_overlay=False)
    _same_masks(_png_ids(tmp_path / 'on', names), want, names)
    assert on.stats().attrs['cleanup'] == totals
    _same_masks([on.mask(t).cpu().numpy() for t in range(len(names))], want, names)          # what the selector reads
    on_tracks = on.save_tracks(tmp_path / 'on')
    video, _ = rle.read_tracks(on_tracks)
    (ann,) = json.load(open(on_tracks))['annotations']
    for t, m in enumerate(want):
        np.testing.assert_array_equal(rle.decode(ann['segmentations'][t]['counts'], video['height'], video['width']), m == 1, err_msg=names[t])

    # the masks of an uncleaned propagation, cleaned as they stand: the in-loop result
    assert off.clean(batch=4, **SPEC) == totals
    assert torch.equal(off.masks, on.masks)
    assert off.clean() == dict.fromkeys(M.STATS, 0) and torch.equal(off.masks, on.masks)

    # and the uncleaned tracks file through the tool: the file the cleaned session wrote
    assert rle.main(['--tracks', off_tracks, '--clean', json.dumps(SPEC), '--out', str(tmp_path / 'tool' / 'tracks.json')]) == 0
    assert json.load(open(tmp_path / 'tool' / 'tracks.json')) == json.load(open(on_tracks))
    assert rle.main(['--tracks', off_tracks, '--clean', json.dumps(SPEC), '--recode', 'compressed', '--out', str(tmp_path / 'tool' / 'c.json')]) == 0
    assert json.load(open(tmp_path / 'tool' / 'c.json')) == rle.recode_tracks(json.load(open(on_tracks)), 'compressed')
    assert rle.main(['--tracks', str(tmp_path / 'tool' / 'c.json'), '--clean', '{"keep_largest": true}', '--out', str(tmp_path / 'tool' / 'k.json')]) == 0
    kept = json.load(open(tmp_path / 'tool' / 'k.json'))             # the compressed form is kept
    assert all(isinstance(s['counts'], str) for s in kept['annotations'][0]['segmentations'] if s is not None)
    _same_masks(rle.read_tracks(tmp_path / 'tool' / 'k.json')[1], [M.clean_host(m, keep_largest=True)[0] for m in want], names)
