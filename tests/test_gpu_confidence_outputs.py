"""config['confidence'] through the frame loops, on a synthetic clip (10 frames of 96 x 128, two objects whose labels are 2 and 5,
frames 0 and 4 annotated) with the synthetic network: without the key, and with it None, the files are those of a run that has never
heard of the option; with it on, the masks are unchanged, the table's areas are the pixel counts of the written masks, the frame
confidence and the tracks' scores follow from the table, and the uncertainty maps are one grey PNG per frame - the same pixels whether
the host or the device builds the file.  The ensemble and VideoSession keep the same table."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from xmem2_amd import confidence as CF

pytestmark = pytest.mark.gpu

T_CLIP, HW = 10, (96, 128)
LABELS = (2, 5)                                               # dense ids 1 and 2
COLOURS = {2: (200, 0, 0), 5: (0, 200, 0)}
GIVEN = [0, 4]
COMMON = dict(frames_with_masks=GIVEN, print_progress=False, save_overlay=False)


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


def _counts(ids):
    return np.stack([np.bincount(m.ravel(), minlength=len(LABELS) + 1) for m in ids])


def _check_table(table, ids):
    """the table of a run against the masks it wrote (no clean-up, no vote: the record describes what was written)"""
    assert sorted(table) == ['area', 'contested', 'labels', 'low', 'margin_sum', 'threshold'] and table['labels'] == [0, *LABELS]
    for name in CF.FIELDS:
        assert table[name].shape == (len(ids), len(LABELS) + 1) and table[name].dtype == np.int64, name
    np.testing.assert_array_equal(table['area'], _counts(ids))
    assert (table['margin_sum'] <= 255 * table['area']).all() and (table['low'] <= table['area']).all()
    assert (table['contested'].sum(1) == table['low'].sum(1)).all()                  # every low pixel is contested by its second
    assert (table['margin_sum'] > 0).any() and table['low'].sum() > 0, 'nothing is unsure on this clip: the test shows too little'


@pytest.fixture(scope='module')
def runs(cfg, net, clip, tmp_path_factory):
    """run_on_video without the key, with the key None, with maps written by the host and with maps built on the device, once"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    root = tmp_path_factory.mktemp('runs')
    dfs = {}
    for name, extra in (('absent', {}), ('none', {'confidence': None}), ('maps', {'confidence': {'threshold': 80, 'maps': True}}),
                        ('device', {'confidence': {'threshold': 80, 'maps': True}, 'png_on_device': True})):
        dfs[name] = run_on_video(imgs, msks, str(root / name), overwrite_config=dict(cfg, **extra), network=net, **COMMON)
    return root, dfs


def test_without_the_option_nothing_changes(runs):
    root, dfs = runs
    absent = _files(root / 'absent')
    assert len(absent) == T_CLIP
    assert _files(root / 'none') == absent
    assert open(root / 'none' / 'tracks.json', 'rb').read() == open(root / 'absent' / 'tracks.json', 'rb').read()
    for off in ('absent', 'none'):
        assert sorted(os.listdir(root / off)) == ['masks', 'tracks.json']
        assert 'confidence' not in dfs[off].attrs and 'confidence' not in dfs[off].columns


def test_with_the_option_the_masks_stay_and_the_table_describes_them(runs, clip):
    root, dfs = runs
    names = clip[2]
    df = dfs['maps']
    assert _files(root / 'maps') == _files(root / 'absent')
    ids = _written_ids(root / 'maps', names)
    assert (ids == 1).any() and (ids == 2).any(), 'an object is in no frame: the test shows too little'
    table = df.attrs['confidence']
    assert table['threshold'] == 80
    _check_table(table, ids)
    assert df['frame'].tolist() == names
    want = CF.frame_confidence(table['area'], table['margin_sum'])
    np.testing.assert_array_equal(df['confidence'].to_numpy(), want)                 # NaN equals NaN here
    conf = CF.object_confidence(table['area'], table['margin_sum'])
    print('frame confidence', np.round(want, 4).tolist())
    assert np.nanmin(want) >= 0 and np.nanmax(want) <= 1 and np.isfinite(want).any()
    # tracks.json: minus the two keys it is the off-run's file; the scores follow from the table
    doc, off = json.load(open(root / 'maps' / 'tracks.json')), json.load(open(root / 'absent' / 'tracks.json'))
    scores = CF.track_scores(table['area'], table['margin_sum'], [t in GIVEN for t in range(T_CLIP)])
    for ann in doc['annotations']:
        col = table['labels'].index(ann['label'])
        assert ann.pop('score') == scores[col] and 0 < scores[col] <= 1
        for t, seg in enumerate(ann['segmentations']):
            if seg is not None:
                assert seg.pop('confidence') == conf[t, col]
    assert doc == off


def test_the_maps(runs, clip):
    root, dfs = runs
    names = clip[2]
    assert sorted(os.listdir(root / 'maps')) == sorted(os.listdir(root / 'device')) == ['masks', 'tracks.json', 'uncertainty']
    assert sorted(os.listdir(root / 'maps' / 'uncertainty')) == sorted(os.listdir(root / 'device' / 'uncertainty')) == names
    table = dfs['maps'].attrs['confidence']
    for name in CF.FIELDS:
        np.testing.assert_array_equal(dfs['device'].attrs['confidence'][name], table[name])
    ids = _written_ids(root / 'maps', names)
    np.testing.assert_array_equal(_written_ids(root / 'device', names), ids)
    for t, n in enumerate(names):
        host, dev = Image.open(root / 'maps' / 'uncertainty' / n), Image.open(root / 'device' / 'uncertainty' / n)
        assert host.mode == dev.mode == 'L' and host.size == dev.size == HW[::-1]
        plane = np.array(host)
        np.testing.assert_array_equal(np.array(dev), plane, err_msg=n)
        q = 255 - plane.astype(np.int64)                                             # the plane and the record are one pass
        assert [int(q[ids[t] == c].sum()) for c in range(3)] == table['margin_sum'][t].tolist()
        assert [int((q[ids[t] == c] < 80).sum()) for c in range(3)] == table['low'][t].tolist()


def test_a_bad_value(cfg, net, clip, tmp_path):
    from xmem2_amd.run_on_video import run_on_video, run_on_video_ensemble
    imgs, msks, _ = clip
    for run in (run_on_video, run_on_video_ensemble):
        with pytest.raises(ValueError, match='confidence'):
            run(imgs, msks, str(tmp_path / 'bad'), overwrite_config=dict(cfg, confidence={'threshold': 300}), network=net, **COMMON)


def test_the_ensemble(cfg, net, clip, tmp_path):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    imgs, msks, names = clip
    run_on_video_ensemble(imgs, msks, str(tmp_path / 'off'), overwrite_config=dict(cfg), network=net, **COMMON)
    df = run_on_video_ensemble(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(cfg, confidence=True), network=net, **COMMON)
    assert _files(tmp_path / 'on') == _files(tmp_path / 'off')                       # two passes: the kernel's argmax of the sum is the merge's
    table = df.attrs['confidence']
    assert table['threshold'] == 64
    _check_table(table, _written_ids(tmp_path / 'on', names))
    np.testing.assert_array_equal(df['confidence'].to_numpy(), CF.frame_confidence(table['area'], table['margin_sum']))


def test_the_session(cfg, net, clip):
    from xmem2_amd.session import VideoSession
    imgs, msks, names = clip
    config = {k: v for k, v in cfg.items() if k != 'save_tracks'}
    plain = VideoSession(imgs, msks, overwrite_config=dict(config), network=net)
    with pytest.raises(RuntimeError, match='confidence'):
        plain.review_queue()
    s = VideoSession(imgs, msks, overwrite_config=dict(config, confidence=True), network=net)
    for t in GIVEN:
        s.save_reference(t)
    s.propagate(0, 'forward', stop=5)
    part = s.confidence()
    assert part['frames'] == list(range(6)) and part['area'].shape == (6, 3)
    s.full_propagation()
    full = s.confidence()
    assert full['frames'] == list(range(T_CLIP)) and full['labels'] == [0, *LABELS] and full['threshold'] == 64
    ids = s.masks.cpu().numpy()
    np.testing.assert_array_equal(full['area'], _counts(ids))
    np.testing.assert_array_equal(full['confidence'], CF.frame_confidence(full['area'], full['margin_sum']))
    queue = s.review_queue(k=T_CLIP)
    assert sorted(queue) == [t for t in range(T_CLIP) if t not in GIVEN]             # no reference, every other frame once
    assert queue == CF.review_queue(full['confidence'], GIVEN, k=T_CLIP) and s.review_queue(k=2) == queue[:2]
    assert all(abs(a - b) > 2 for i, a in enumerate(s.review_queue(k=3, min_gap=2)) for b in s.review_queue(k=3, min_gap=2)[:i])
    # a second propagation of a part overwrites those rows and no other
    s.save_reference(7)
    s.propagate(6, 'forward', stop=8)
    after = s.confidence()
    rest = [t for t in range(T_CLIP) if t not in (6, 7, 8)]
    for name in CF.FIELDS:
        np.testing.assert_array_equal(after[name][rest], full[name][rest], err_msg=name)
    np.testing.assert_array_equal(after['area'], _counts(s.masks.cpu().numpy()))
    assert 7 not in s.review_queue(k=T_CLIP)
    off = VideoSession(imgs, msks, overwrite_config=dict(config), network=net)       # the masks are those of a session without the key
    for t in GIVEN:
        off.save_reference(t)
    off.propagate(0, 'forward', stop=5)
    off.full_propagation()
    assert torch.equal(off.masks, torch.from_numpy(ids).cuda())
