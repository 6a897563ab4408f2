"""Every side output of the frame loop at once - tracks with compressed counts and polygons, mattes and trimaps, masks built on the
device, uncertainty maps - on the clip of the PNG tests (10 frames of 96 x 128, labels 2 and 5, frames 0 and 4 given: two objects, a
late annotation, a delivery depth shorter than the video).  Each family writes in the combined run what it writes in a run of its own;
with a starting room of 16 events, characters, corners and bytes every frame is done again at its exact size when its record
arrives, and the files are those of a run that had room from the start.  The ensemble's merged mask is a buffer rewritten every frame,
which a frame done again reads one frame late: there a lost copy shows in a file.

The starting room: `test_sixteen_is_below_what_the_clip_needs` holds 16 against the host definitions on the clip's ground truth.  With
the events' room at 16 too, a frame's characters are never the only thing that did not fit - the events' retry makes the strings, and
`RLE_STRING_STATS` rises only inside that retry - so the loop's character-only retry is shown by a second combined run that starts
with 16 characters and the default events.
The tracks' run of its own keeps config['confidence'] without maps: the scores are part of tracks.json."""
import json

import numpy as np
import pytest

from test_gpu_png_outputs import COMMON, MATTES, _files, _same_images, cfg, checkpoint, clip, net  # noqa: F401 (fixtures)
from test_gpu_temporal_outputs import HW, LABELS, T_CLIP

gpu = pytest.mark.gpu

TRACKS = dict(save_tracks=True, tracks_counts='compressed', tracks_polygons=True)
FAMILIES = {                                                         # a run of its own, with png_on_device where the family uses it
    'tracks': dict(TRACKS, confidence={'maps': False}),
    'masks': dict(png_on_device=True),
    'mattes': dict(mattes=dict(MATTES), png_on_device=True),
    'uncertainty': dict(confidence={'maps': True}, png_on_device=True),
}
COMBINED = dict(TRACKS, mattes=dict(MATTES), png_on_device=True, confidence={'maps': True})
SUBS = ('masks', 'mattes', 'trimaps', 'uncertainty')
TINY = 16


def _tiny(mp, events=True):
    """every starting room is TINY (`events=False`: the events keep theirs, so that only the characters do not fit)"""
    from xmem2_amd import png, polygons, rle
    mp.setattr(png, 'default_capacity', lambda H, W, mode: TINY)
    if events:
        mp.setattr(rle, 'default_capacity', lambda h, w: TINY)
    mp.setattr(rle, 'default_char_capacity', lambda h, w, capacity=None: TINY)
    mp.setattr(polygons, 'default_capacity', lambda H, W: TINY)


def _retries():
    from xmem2_amd import ops
    return {name: getattr(ops, name)['retries'] for name in ('RLE_STATS', 'RLE_STRING_STATS', 'POLY_STATS', 'PNG_STATS')}


def _tracks(root):
    with open(root / 'tracks.json') as fh:
        return json.load(fh)


def test_sixteen_is_below_what_the_clip_needs():
    """the retries are a condition on the inputs: by the host definitions, every frame of the clip's ground truth needs more"""
    from xmem2_amd import png, polygons, rle
    from xmem2_amd.synth import synthetic_masks
    masks = synthetic_masks(T_CLIP, 2, *HW)
    for t in range(T_CLIP):
        idx = np.zeros(HW, np.uint8)
        for o in range(2):
            idx[masks[t, o] > 0] = o + 1
        runs = [rle.encode_host(idx, k) for k in (1, 2)]
        events, chars = sum(len(r.events) for r in runs), sum(len(rle.compress_counts(r.counts)) for r in runs)
        corners = int(polygons.record_host(idx, 2)[0][:, 0].sum())
        assert events > TINY and chars > TINY and corners > TINY, (t, events, chars, corners)
        assert events <= rle.default_capacity(*HW), 'the events must fit their default room for the character-only retry'
        assert len(png.encode_host(idx, 'rgb', np.zeros((256, 3), np.uint8))) > TINY
        assert len(png.encode_host(np.where(idx > 0, 255, 0).astype(np.uint8), 'grey')) > TINY


@pytest.fixture(scope='module')
def runs(cfg, net, clip, tmp_path_factory):
    """run_on_video: the combined run with tiny rooms ('tiny'), with tiny rooms but the events' ('chars'), with the default ones
    ('default'), and each family alone with tiny rooms -> (root, {name: DataFrame}, {name: the retries a run added})"""
    from xmem2_amd.run_on_video import run_on_video
    imgs, msks, _ = clip
    root = tmp_path_factory.mktemp('together')
    dfs, retries = {}, {}

    def run(name, extra):
        before = _retries()
        dfs[name] = run_on_video(imgs, msks, str(root / name), overwrite_config=dict(cfg, **extra), network=net, **COMMON)
        retries[name] = {k: v - before[k] for k, v in _retries().items()}
    with pytest.MonkeyPatch.context() as mp:
        _tiny(mp)
        run('tiny', COMBINED)
        for name, extra in FAMILIES.items():
            run(name, extra)
    with pytest.MonkeyPatch.context() as mp:
        _tiny(mp, events=False)
        run('chars', COMBINED)
    run('default', COMBINED)
    return root, dfs, retries


@gpu
def test_every_retry_path_fired(runs):
    _, _, retries = runs
    print('retries added:', retries)
    for name in ('RLE_STATS', 'RLE_STRING_STATS', 'POLY_STATS', 'PNG_STATS'):
        assert retries['tiny'][name] > 0, f'{name}: no frame was done again, the test shows too little'
    assert retries['chars']['RLE_STRING_STATS'] > 0, 'RLE_STRING_STATS: no frame was compressed again, the test shows too little'
    assert retries['chars']['RLE_STATS'] == 0, 'the events did not fit either: this run was to show the characters alone'
    # the mask, the planes and the uncertainty map of the first frame at least
    assert retries['tiny']['PNG_STATS'] >= 1 + len(MATTES) * len(LABELS) + 1


@gpu
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_each_family_writes_what_it_writes_alone(runs, family):
    root, dfs, _ = runs
    if family == 'tracks':
        assert _tracks(root / 'tiny') == _tracks(root / 'tracks')
    else:
        subs = {'masks': ('masks',), 'mattes': ('mattes', 'trimaps'), 'uncertainty': ('uncertainty',)}[family]
        alone = _files(root / family, subs)
        assert alone and _files(root / 'tiny', subs) == alone
    shared = [c for c in dfs['tiny'].columns if c in dfs[family].columns]
    assert {'frame', 'mask_provided'} <= set(shared) and dfs['tiny'][shared].equals(dfs[family][shared])


@gpu
@pytest.mark.parametrize('other', ['chars', 'default'])
def test_a_frame_done_again_is_the_same_frame(runs, other):
    root, dfs, _ = runs
    tiny = _files(root / 'tiny', SUBS)
    assert len(tiny) == T_CLIP * (1 + len(MATTES) * len(LABELS) + 1)    # a mask, a matte and a trimap per label, a map
    assert _files(root / other, SUBS) == tiny
    assert _tracks(root / other) == _tracks(root / 'tiny')
    assert dfs[other].equals(dfs['tiny']) and list(dfs[other].attrs) == list(dfs['tiny'].attrs)


@gpu
def test_the_ensemble_rereads_its_own_copy(cfg, net, clip, tmp_path):
    from xmem2_amd.run_on_video import run_on_video_ensemble
    imgs, msks, names = clip
    one = dict(cfg, ensemble=[[-1, True]])
    dfs, retries = {}, {}
    with pytest.MonkeyPatch.context() as mp:
        _tiny(mp)
        before = _retries()
        dfs['tiny'] = run_on_video_ensemble(imgs, msks, str(tmp_path / 'tiny'), overwrite_config=dict(one, **COMBINED), network=net, **COMMON)
        retries = {k: v - before[k] for k, v in _retries().items()}
    dfs['default'] = run_on_video_ensemble(imgs, msks, str(tmp_path / 'default'), overwrite_config=dict(one, **COMBINED), network=net, **COMMON)
    dfs['plain'] = run_on_video_ensemble(imgs, msks, str(tmp_path / 'plain'), overwrite_config=dict(one), network=net, **COMMON)
    print('retries added:', retries)
    for name in ('RLE_STATS', 'RLE_STRING_STATS', 'POLY_STATS', 'PNG_STATS'):
        assert retries[name] > 0, f'{name}: no frame was done again, the test shows too little'
    tiny = _files(tmp_path / 'tiny', SUBS)
    assert len(tiny) == T_CLIP * (1 + len(MATTES) * len(LABELS) + 1) and _files(tmp_path / 'default', SUBS) == tiny
    assert _tracks(tmp_path / 'tiny') == _tracks(tmp_path / 'default')
    assert dfs['tiny'].equals(dfs['default']) and dfs['tiny']['frame'].tolist() == names
    _same_images(_files(tmp_path / 'plain'), _files(tmp_path / 'tiny'))          # the host's files open to the same pixels
    shared = list(dfs['plain'].columns)
    assert dfs['tiny'][shared].equals(dfs['plain'])
