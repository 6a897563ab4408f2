"""config['png_on_device'] through every output path, on the synthetic clip of the temporal tests (10 frames of 96 x 128, two objects
whose labels are 2 and 5, frames 0 and 4 annotated) with the synthetic network: the files have the names of a run without the option
and open to the same mode, size and pixels; without the key the files are byte for byte those of a run that has never heard of it."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from test_gpu_temporal_outputs import COLOURS, COMMON, GIVEN, HW, LABELS, LUT, T_CLIP, _files, _make_clip, _written_ids

pytestmark = pytest.mark.gpu


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
    return _make_clip(tmp_path_factory.mktemp('clip'), T_CLIP)


MATTES = {'feather': 3, 'trimap': 2}


@pytest.fixture(scope='module')
def runs(cfg, net, clip, tmp_path_factory):
    """run_on_video without the key, with the key None, 'rgb' and 'palette', each with mattes and a trimap, once"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    root = tmp_path_factory.mktemp('runs')
    dfs = {}
    for name, extra in (('absent', {}), ('none', {'png_on_device': None}), ('rgb', {'png_on_device': True}),
                        ('palette', {'png_on_device': {'mode': 'palette'}})):
        dfs[name] = run_on_video(imgs, msks, str(root / name), overwrite_config=dict(cfg, mattes=dict(MATTES), **extra), network=net, **COMMON)
    return root, dfs


def _same_images(a, b):
    """two sets of files {relative path: bytes}: the same names, every pair opens to the same mode, size and pixels"""
    assert sorted(a) == sorted(b) and a
    for rel in a:
        x, y = Image.open(io.BytesIO(a[rel])), Image.open(io.BytesIO(b[rel]))
        assert x.mode == y.mode and x.size == y.size, rel
        np.testing.assert_array_equal(np.array(x), np.array(y), err_msg=rel)


def test_without_the_option_nothing_changes(runs):
    root, dfs = runs
    subs = ('masks', 'mattes', 'trimaps')
    absent = _files(root / 'absent', subs)
    assert len(absent) == T_CLIP * (1 + 2 * len(LABELS))
    assert _files(root / 'none', subs) == absent
    assert sorted(os.listdir(root / 'none')) == sorted(os.listdir(root / 'absent')) == ['masks', 'mattes', 'trimaps']


def test_rgb_files_open_to_what_the_host_writes(runs, clip):
    from png_refs import chunks
    root, dfs = runs
    off, on = _files(root / 'absent'), _files(root / 'rgb')
    _same_images(off, on)
    assert off != on                                                 # the device's own files, not Pillow's
    for data in on.values():
        assert [k for k, _ in chunks(data)] == [b'IHDR', b'IDAT', b'IEND'] and Image.open(io.BytesIO(data)).mode == 'RGB'
    ids = _written_ids(root / 'rgb', clip[2])
    assert (ids == 1).any() and (ids == 2).any(), 'an object is in no frame: the test shows too little'
    assert dfs['rgb'].equals(dfs['absent']) and dfs['rgb']['frame'].tolist() == clip[2]
    assert sorted(os.listdir(root / 'rgb')) == ['masks', 'mattes', 'trimaps']


def test_palette_files_are_index_pngs(runs, clip):
    root, dfs = runs
    names = clip[2]
    dense = _written_ids(root / 'absent', names)
    want_palette = Image.open(os.path.join(clip[1], names[0])).getpalette()
    for n, m in zip(names, dense):
        im = Image.open(root / 'palette' / 'masks' / n)
        assert im.mode == 'P' and im.size == (HW[1], HW[0])
        np.testing.assert_array_equal(np.array(im), LUT[m])
        assert im.getpalette()[:768] == (want_palette + [0] * 768)[:768]
        for lab in LABELS:
            assert tuple(im.getpalette()[3 * lab:3 * lab + 3]) == COLOURS[lab]
    assert sorted(os.listdir(root / 'palette' / 'masks')) == names and dfs['palette'].equals(dfs['absent'])


@pytest.mark.parametrize('name', ['rgb', 'palette'])
def test_mattes_and_trimaps_are_pixel_equal(runs, name):
    root, _ = runs
    subs = ('mattes', 'trimaps')
    off, on = _files(root / 'absent', subs), _files(root / name, subs)
    assert len(off) == 2 * len(LABELS) * T_CLIP
    _same_images(off, on)
    assert off != on


def test_the_ensemble(cfg, net, clip, tmp_path):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    imgs, msks, names = clip
    subs = ('masks', 'mattes', 'trimaps')
    a = run_on_video_ensemble(imgs, msks, str(tmp_path / 'off'), overwrite_config=dict(cfg, mattes=dict(MATTES)), network=net, **COMMON)
    b = run_on_video_ensemble(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(cfg, mattes=dict(MATTES), png_on_device=True), network=net, **COMMON)
    _same_images(_files(tmp_path / 'off', subs), _files(tmp_path / 'on', subs))
    assert a.equals(b) and b['frame'].tolist() == names


def _spy_on_fetchers(monkeypatch):
    """the shapes of everything any AsyncMaskFetcher is given"""
    from xmem2_amd import run_on_video as rov
    seen, real = [], rov.AsyncMaskFetcher.submit

    def submit(self, tag, mask_gpu):
        seen.append(tuple(mask_gpu.shape))
        return real(self, tag, mask_gpu)
    monkeypatch.setattr(rov.AsyncMaskFetcher, 'submit', submit)
    return seen


def test_no_mask_plane_travels_without_overlays(cfg, net, clip, runs, tmp_path, monkeypatch):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    seen = _spy_on_fetchers(monkeypatch)
    df = run_on_video(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(cfg, png_on_device=True), network=net, **COMMON)
    assert len(seen) == T_CLIP and all(len(s) == 1 for s in seen), f'a plane went to the host: {seen}'
    assert df.equals(runs[1]['absent'])
    _same_images(_files(runs[0] / 'absent'), _files(tmp_path / 'on'))
    # with tracks too, still no plane; the tracks file is what it is without the option
    del seen[:]
    run_on_video(imgs, msks, str(tmp_path / 'tracks_off'), overwrite_config=dict(cfg, save_tracks=True), network=net, **COMMON)
    assert sum(len(s) == 2 for s in seen) == T_CLIP
    del seen[:]
    run_on_video(imgs, msks, str(tmp_path / 'tracks_on'), overwrite_config=dict(cfg, save_tracks=True, png_on_device=True), network=net, **COMMON)
    assert len(seen) == 2 * T_CLIP and all(len(s) == 1 for s in seen)
    assert open(tmp_path / 'tracks_on' / 'tracks.json', 'rb').read() == open(tmp_path / 'tracks_off' / 'tracks.json', 'rb').read()
    _same_images(_files(runs[0] / 'absent'), _files(tmp_path / 'tracks_on'))


def test_with_overlays_the_mask_travels_for_them_alone(cfg, net, clip, tmp_path, monkeypatch):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    common = dict(COMMON, save_overlay=True)
    run_on_video(imgs, msks, str(tmp_path / 'off'), overwrite_config=dict(cfg), network=net, **common)
    seen = _spy_on_fetchers(monkeypatch)
    run_on_video(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(cfg, png_on_device=True), network=net, **common)
    assert sum(len(s) == 2 for s in seen) == T_CLIP and sum(len(s) == 1 for s in seen) == T_CLIP
    assert _files(tmp_path / 'on', ('overlay',)) == _files(tmp_path / 'off', ('overlay',)) and len(_files(tmp_path / 'on', ('overlay',))) == T_CLIP
    on = _files(tmp_path / 'on')
    _same_images(_files(tmp_path / 'off'), on)
    assert all(data[37:41] == b'IDAT' for data in on.values())       # built on the device: Pillow writes other chunks first


def test_a_starting_capacity_of_64_bytes(cfg, net, clip, runs, tmp_path, monkeypatch):
    from xmem2_amd import ops, png
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    monkeypatch.setattr(png, 'default_capacity', lambda H, W, mode: 64)
    before = ops.PNG_STATS['retries']
    run_on_video(imgs, msks, str(tmp_path / 'on'), overwrite_config=dict(cfg, mattes=dict(MATTES), png_on_device=True), network=net, **COMMON)
    retries = ops.PNG_STATS['retries'] - before
    print('frames encoded again:', retries)
    assert retries >= 2                                              # the first mask and the first planes at least
    subs = ('masks', 'mattes', 'trimaps')
    assert _files(tmp_path / 'on', subs) == _files(runs[0] / 'rgb', subs)        # the same bytes as with room from the start


def test_session_save_and_the_session_command(cfg, net, clip, tmp_path):
    from xmem2_amd.session import VideoSession
    imgs, msks, names = clip
    s = VideoSession(imgs, msks, overwrite_config=dict(cfg), network=net)
    for t in GIVEN:
        s.save_reference(t)
    s.full_propagation()
    s.save(str(tmp_path / 'host'), save_overlay=True)
    s.save(str(tmp_path / 'rgb'), save_overlay=True, png_on_device=True, batch=4)
    s.save(str(tmp_path / 'pal'), save_overlay=False, png_on_device={'mode': 'palette'})
    host, rgb = _files(tmp_path / 'host'), _files(tmp_path / 'rgb')
    assert len(host) == T_CLIP and host != rgb
    _same_images(host, rgb)
    assert _files(tmp_path / 'host', ('overlay',)) == _files(tmp_path / 'rgb', ('overlay',))
    assert os.listdir(tmp_path / 'pal') == ['masks']
    masks = s.masks.cpu().numpy()
    for t, n in enumerate(names):
        im = Image.open(tmp_path / 'pal' / 'masks' / n)
        assert im.mode == 'P'
        np.testing.assert_array_equal(np.array(im), LUT[masks[t]])
    with pytest.raises(ValueError):
        s.save(str(tmp_path / 'bad'), png_on_device={'mode': 'grey'})


def test_rle_out_dir_on_the_device(cfg, net, clip, tmp_path):
    from xmem2_amd import rle
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, names = clip
    run_on_video(imgs, msks, str(tmp_path / 'run'), overwrite_config=dict(cfg, save_tracks=True, save_masks=False), network=net, **COMMON)
    tracks = str(tmp_path / 'run' / 'tracks.json')
    annotation = os.path.join(msks, names[0])
    for tag, extra in (('l', []), ('p', ['--palette-from', annotation])):
        assert rle.main(['--tracks', tracks, '--out', str(tmp_path / (tag + '_host'))] + extra) == 0
        assert rle.main(['--tracks', tracks, '--out', str(tmp_path / (tag + '_dev')), '--png-on-device'] + extra) == 0
        host = {f: open(tmp_path / (tag + '_host') / f, 'rb').read() for f in os.listdir(tmp_path / (tag + '_host'))}
        dev = {f: open(tmp_path / (tag + '_dev') / f, 'rb').read() for f in os.listdir(tmp_path / (tag + '_dev'))}
        assert sorted(host) == names and host != dev
        _same_images(host, dev)
        if tag == 'p':
            for f in names:
                a, b = Image.open(tmp_path / 'p_host' / f), Image.open(tmp_path / 'p_dev' / f)
                np.testing.assert_array_equal(np.array(a.convert('RGB')), np.array(b.convert('RGB')))


def test_the_matte_command(cfg, net, clip, runs, tmp_path):
    from xmem2_amd import matte
    root, _ = runs
    args = ['--masks', str(root / 'palette' / 'masks'), '--feather', '3', '--trimap', '2']
    assert matte.main(args + ['--out', str(tmp_path / 'host')]) == 0
    assert matte.main(args + ['--out', str(tmp_path / 'dev'), '--png-on-device']) == 0
    subs = ('mattes', 'trimaps')
    host, dev = _files(tmp_path / 'host', subs), _files(tmp_path / 'dev', subs)
    assert len(host) == 2 * len(LABELS) * T_CLIP and host != dev
    _same_images(host, dev)
    _same_images(_files(root / 'absent', subs), dev)                 # and those are the loop's planes


def test_a_bad_value(cfg, net, clip, tmp_path):
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, _ = clip
    with pytest.raises(ValueError, match='png_on_device'):
        run_on_video(imgs, msks, str(tmp_path / 'bad'), overwrite_config=dict(cfg, png_on_device={'mode': 'grey'}), network=net, **COMMON)
