"""The session's feature cache on the device (`config['session_feature_cache_bytes']`): the copy kernel byte for byte, and a session with
the cache on against its twin with the cache off - masks, selector arenas and written PNGs equal after every round, in every order of
travel, under a budget, with two objects, a later reference, two sessions on one network, in the fp16 loop and through the command line.

The clips are those of tests/test_gpu_session.py (its small helpers restated): 9 frames of 96 x 128 with key_batch 4, i.e. the batches
[0-3], [4-7] and a tail [8] at batch 1, mem_every 2.  One network per module and precision."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

T_CLIP, HW = 9, (96, 128)
PALETTES = {1: [0, 0, 0, 255, 255, 255], 2: [0, 0, 0, 200, 0, 0, 0, 200, 0]}
WHOLE_CLIP = 1 << 30                                         # a budget no 9-frame clip of this size reaches


@pytest.fixture(scope='module')
def checkpoint(synth_sd, tmp_path_factory):
    path = tmp_path_factory.mktemp('ckpt') / 'XMem_synth.pth'
    torch.save(synth_sd, path)
    return str(path)


@pytest.fixture(scope='module')
def cfg(checkpoint):
    return {'model': checkpoint, 'size': -1, 'mem_every': 2}


@pytest.fixture(scope='module')
def nets(checkpoint):
    """precision -> the one network of that precision (built on first use)"""
    from xmem2_amd.network import XMem
    made = {}

    def get(precision='fp32'):
        if precision not in made:
            made[precision] = XMem({'precision': precision}, checkpoint).to('cuda').eval()
        return made[precision]
    return get


def _write_clip(root, n_obj, seed=1234, hw=HW, t=T_CLIP, second_object_from=0):
    from PIL import Image
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    imgs, msks = root / 'JPEGImages', root / 'Annotations'
    imgs.mkdir(parents=True); msks.mkdir(parents=True)
    frames, masks = synthetic_frames(t, *hw, seed=seed), synthetic_masks(t, n_obj, *hw)
    pal = PALETTES[n_obj] + [0] * (768 - len(PALETTES[n_obj]))
    for i in range(t):
        rgb = np.clip((frames[i].transpose(1, 2, 0) * 0.229 + 0.45) * 255, 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(imgs / f'frame_{i:06d}.png')
        idx = sum(masks[i, o] * (o + 1) for o in range(n_obj) if o == 0 or i >= second_object_from).astype(np.uint8)
        im = Image.fromarray(idx, mode='P'); im.putpalette(pal); im.save(msks / f'frame_{i:06d}.png')
    return str(imgs), str(msks)


@pytest.fixture(scope='module')
def clips(tmp_path_factory):
    root = tmp_path_factory.mktemp('clips')
    return {'one': _write_clip(root / 'one', 1), 'two': _write_clip(root / 'two', 2), 'other': _write_clip(root / 'other', 1, seed=77),
            'late': _write_clip(root / 'late', 2, second_object_from=3)}


def _mask_bytes(out_dir):
    d = os.path.join(str(out_dir), 'masks')
    return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


def _session(clips, cfg, net, which, cache_bytes=0, **over):
    from xmem2_amd.session import VideoSession
    config = dict(cfg, **over)
    if cache_bytes:
        config['session_feature_cache_bytes'] = cache_bytes
    return VideoSession(*clips[which], overwrite_config=config, network=net)


_saves = [0]


def _state(s, tmp_path, frames=None):
    """What a round leaves behind: the masks arena, the selector's three arenas (rows of the visited frames) and the PNG bytes `save`
    writes."""
    rows = list(range(len(s))) if frames is None else sorted(frames)
    _saves[0] += 1
    out = tmp_path / f'save{_saves[0]}'
    s.save(out, save_overlay=False)
    torch.cuda.synchronize()
    return dict(masks=s.masks[rows].cpu(), key=s.key[rows].cpu(), shrinkage=s.shrinkage[rows].cpu(), selection=s.selection[rows].cpu(),
                png=_mask_bytes(out))


def _assert_same(got, want, what):
    for name in ('masks', 'key', 'shrinkage', 'selection'):
        assert torch.equal(got[name].view(torch.uint8), want[name].view(torch.uint8)), f'{what}: the {name} arena differs'
    assert got['png'] == want['png'], f'{what}: the written masks differ'
    assert not bool(torch.isnan(got['key']).any())


def _spy_stages(monkeypatch):
    from xmem2_amd.network import XMem
    names = []
    orig = XMem._run_stage
    monkeypatch.setattr(XMem, '_run_stage', lambda self, name, *a, **k: (names.append(name), orig(self, name, *a, **k))[1])
    return names


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
GUARD = 256
# (bytes, source offset, destination offset): offsets from a 256-byte base; the issue's lengths first, then fillers up to 16 segments
SEGMENTS = [(0, 0, 2), (1, 2, 0), (2, 4, 18), (15, 8, 8), (16, 16, 0), (17, 18, 2), (4096 + 6, 0, 0), (3 << 20, 2, 16),
            (31, 4, 8), (32, 0, 4), (33, 18, 18), (255, 16, 2), (4096, 8, 0), (6, 2, 4), (1000, 0, 18), (48, 4, 4)]
# offsets no fp16 / fp32 slice has, for the byte-wide loads; and more pairs than one launch carries
ODD_SEGMENTS = [(100, 1, 0), (100, 0, 3), (5000, 3, 1), (4097, 1, 1), (77, 5, 2)]


def _lay_out(segments, seed):
    """Source bytes (random) and the expected destination (a guard pattern with every segment's bytes in place), as numpy arrays, plus
    the (source start, destination start, length) of every segment.  Each segment has a region of its own with GUARD bytes either side."""
    rng = np.random.RandomState(seed)
    places, s_at, d_at = [], 0, 0
    for n, so, do in segments:
        places.append((s_at + GUARD + so, d_at + GUARD + do, n))
        room = -(-(2 * GUARD + n + 32) // 256) * 256
        s_at, d_at = s_at + room, d_at + room
    src = rng.randint(0, 256, s_at, dtype=np.uint8)
    guard = (np.arange(d_at) * 37 + 11).astype(np.uint8)
    want = guard.copy()
    for a, b, n in places:
        want[b:b + n] = src[a:a + n]
    return src, guard, want, places


@pytest.mark.parametrize('name,segments', [('sixteen', SEGMENTS), ('odd_offsets', ODD_SEGMENTS), ('two_launches', SEGMENTS + ODD_SEGMENTS)])
def test_copy_segments_is_byte_exact_and_leaves_the_guards_alone(name, segments):
    from xmem2_amd import _lib, ops
    src_h, guard_h, want_h, places = _lay_out(segments, 3)
    assert name != 'sixteen' or (len(segments) == 16 <= _lib.COPY_MAX_SEGMENTS and {n for n, _, _ in segments} >= {0, 1, 2, 15, 16, 17, 4102, 3 << 20}
                                 and {o for _, so, do in segments for o in (so, do)} == {0, 2, 4, 8, 16, 18})
    src, dst = torch.from_numpy(src_h).cuda(), torch.from_numpy(guard_h).cuda()
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0
    pairs = [(src[a:a + n], dst[b:b + n]) for a, b, n in places]
    launches = []
    lib = _lib.load()
    orig = lib.xmem_copy_segments
    try:
        lib.xmem_copy_segments = lambda *a: (launches.append(a[3]), orig(*a))[1]
        ops.copy_segments(pairs)
    finally:
        lib.xmem_copy_segments = orig
    assert launches == [len(segments)]                       # ONE call; it is one launch per 16 segments inside the library
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != want_h)
    assert bad.size == 0, f'{bad.size} wrong bytes, first at {bad[:5]}'
    assert np.array_equal(src.cpu().numpy(), src_h)
    ops.copy_segments(pairs)                                 # a second launch gives the same bytes
    assert np.array_equal(dst.cpu().numpy(), want_h)
    # typed tensors: equal BYTE counts are what matters
    a = torch.randn(1000, device='cuda')[1:].half()          # a fresh, contiguous half tensor of 999 elements
    b = torch.zeros(999 * 2 + 2, dtype=torch.uint8, device='cuda')
    ops.copy_segments([(a, b[2:])])
    assert torch.equal(b[2:].view(torch.float16), a) and int(b[:2].sum()) == 0


def test_copy_segments_rejects_what_it_cannot_copy():
    from xmem2_amd import ops
    a, b = torch.zeros(64, device='cuda'), torch.zeros(64, device='cuda')
    ops.copy_segments([])                                    # nothing to do
    ops.copy_segments([(a[:0], b[:0])])                      # an empty pair
    with pytest.raises(RuntimeError, match='bytes'):
        ops.copy_segments([(a, b[:63])])
    with pytest.raises(RuntimeError, match='bytes'):
        ops.copy_segments([(a, b.half())])
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.copy_segments([(a.cpu(), b)])
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.copy_segments([(a, b.cpu())])
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.copy_segments([(a[::2], b[:32])])
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.copy_segments([(a.view(8, 8), b.view(8, 8).t())])
    with pytest.raises(RuntimeError):
        ops.copy_segments([(a, a)])                          # a pair that overlaps itself
    assert int(a.sum()) == 0 and int(b.sum()) == 0


# ---- 4. / 7. / 8. forward: cache on == cache off ------------------------------------------------------------------------------
def _forward_comparison(clips, cfg, net, which, tmp_path, monkeypatch, repeats=0, **over):
    """Session A (cache off) and B (a budget for the whole clip) on one network: save_reference(0), full_propagation(),
    save_reference(5), full_propagation(); equal state after each round; B's second round replays no key stage and is served from the
    cache frame by frame; `repeats` more second rounds of B give the same bytes."""
    A = _session(clips, cfg, net, which, **over)
    B = _session(clips, cfg, net, which, WHOLE_CLIP, **over)
    assert A.cache_info() == B.cache_info() == dict(entry_bytes=0, frames=0, bytes=0, hits=0, misses=0)
    for s in (A, B):
        s.save_reference(0)
        s.full_propagation()
    first = _state(A, tmp_path)
    _assert_same(_state(B, tmp_path), first, f'{which}: round 1')
    info = B.cache_info()
    assert info['frames'] == T_CLIP and info['misses'] == T_CLIP and info['hits'] == 0
    assert info['bytes'] == T_CLIP * info['entry_bytes'] > 0 and A.cache_info()['bytes'] == 0
    for s in (A, B):
        s.save_reference(5)
    A.full_propagation()
    second = _state(A, tmp_path)
    assert second['png'] != first['png']                     # the second reference changed something: the rounds are not trivially equal
    names = _spy_stages(monkeypatch)
    B.full_propagation()
    monkeypatch.undo()
    assert 'segment' in names and 'key' not in names, f'stages replayed by the cached round: {sorted(set(names))}'
    assert B.cache_info()['hits'] == T_CLIP and B.cache_info()['misses'] == T_CLIP
    _assert_same(_state(B, tmp_path), second, f'{which}: round 2')
    for r in range(repeats):                                 # the same round again: a race between the streams would show here
        B.full_propagation()
        _assert_same(_state(B, tmp_path), second, f'{which}: round 2, repeat {r + 1}')
        assert B.cache_info()['hits'] == (r + 2) * T_CLIP
    return A, B


def test_a_cached_round_is_bit_identical_and_runs_no_key_stage(clips, cfg, nets, tmp_path, monkeypatch):
    A, B = _forward_comparison(clips, cfg, nets(), 'one', tmp_path, monkeypatch, repeats=3)
    # what an entry holds: fp32 throughout in the default mode, key | shrinkage | selection | f16 | the extras of the hinted key pass
    layout = B._fcache.layout
    gh, gw = B.grid_hw
    assert [d for _, d in layout] == [torch.float32] * len(layout) and len(layout) in (6, 8)
    assert layout[0][0] == (gh * gw, 64) and layout[1][0] == (gh * gw,) and layout[3][0] == (1, gh, gw, 1024)
    # the restored-key slot: stable buffers the decoder stages alias, f8 / f4 without memory behind them
    net = nets()
    slots = [st[2] for k, st in net._stages.items() if k[0] == 'keyr']
    assert slots and all(o[4].stride(-1) == 0 and o[5].stride(-1) == 0 and net._is_stage_output(o[3]) for o in slots)


# ---- 5. other orders ------------------------------------------------------------------------------------------------------
def test_backward_and_partial_propagation_from_the_cache(clips, cfg, nets, tmp_path):
    """After a forward round the entries of frames 0-7 carry the tag 4 and frame 8 the tag 1; every call below runs on both sessions."""
    net = nets()
    A, B = _session(clips, cfg, net, 'one'), _session(clips, cfg, net, 'one', WHOLE_CLIP)
    for s in (A, B):
        s.save_reference(0)
        s.full_propagation()
    for call, hits in ((lambda s: s.propagate(8, 'backward'), 4),           # [8,7,6,5] and [0] run the key pass, [4,3,2,1] is restored
                       (lambda s: s.propagate(2, 'forward', stop=6), 4),    # [2,3,4,5] is restored, the tail [6] (tagged 4) is not
                       (lambda s: s.propagate(8, 'backward'), 5)):          # [8,7,6,5] holds frame 6, now tagged 1; [4,3,2,1] and [0] hit
        before = B.cache_info()['hits']
        order_a, order_b = call(A), call(B)
        assert order_a == order_b
        _assert_same(_state(B, tmp_path, order_b), _state(A, tmp_path, order_a), f'order {order_b}')
        assert B.cache_info()['hits'] - before == hits, order_b


# ---- 6. budget ------------------------------------------------------------------------------------------------------------
def test_a_budget_of_five_entries_still_gives_cache_off_bytes(clips, cfg, nets, tmp_path):
    net = nets()
    probe = _session(clips, cfg, net, 'one', WHOLE_CLIP)
    probe.save_reference(0)
    probe.propagate(0, 'forward', stop=0)                    # one key pass tells the entry size
    entry = probe.cache_info()['entry_bytes']
    assert entry > 0
    budget = 5 * entry + entry // 2
    A, B = _session(clips, cfg, net, 'one'), _session(clips, cfg, net, 'one', budget)
    for r, ref in enumerate((0, 5)):
        for s in (A, B):
            s.save_reference(ref)
            s.full_propagation()
        _assert_same(_state(B, tmp_path), _state(A, tmp_path), f'round {r + 1}')
    info = B.cache_info()
    assert info['bytes'] == 5 * entry <= budget and info['frames'] == 5
    assert info['hits'] == 4 and info['misses'] == T_CLIP + 5         # round 2 restored [0-3]; [4-7] and [8] ran the key pass
    assert sorted(B._fcache._slot) == [0, 1, 2, 3, 4]


def test_cached_rounds_under_a_full_stage_cache(clips, cfg, checkpoint, tmp_path, monkeypatch):
    """MAX_STAGES reached: restored-key slots count as stages, are dropped least recently used first together with the decoder and
    value stages that alias them - also while frames restored into them are still pending - and are made again on demand.  The bytes
    do not change."""
    import xmem2_amd.network as N
    mine = N.XMem({'precision': 'fp32'}, checkpoint).to('cuda').eval()
    A, B = _session(clips, cfg, mine, 'one'), _session(clips, cfg, mine, 'one', WHOLE_CLIP)
    for s in (A, B):
        s.save_reference(0)
        s.full_propagation()
    want = _state(A, tmp_path)
    _assert_same(_state(B, tmp_path), want, 'round 1')
    assert len(mine._stages) > 12
    monkeypatch.setattr(N, 'MAX_STAGES', 12)                 # fewer than the slots and stages one cached round needs
    evicted = []
    orig = N.XMem._evict_lru
    monkeypatch.setattr(N.XMem, '_evict_lru', lambda self: (evicted.append(next(iter(self._stages))[0]), orig(self))[1])
    for r in (2, 3):
        B.full_propagation()
        _assert_same(_state(B, tmp_path), want, f'round {r}')
        assert len(mine._stages) <= 12
    print('evicted:', {k: evicted.count(k) for k in sorted(set(evicted))})
    assert 'keyr' in evicted and B.cache_info()['hits'] == 2 * T_CLIP


# ---- 7. two objects, a later reference, a shared network ----------------------------------------------------------------------
@pytest.mark.parametrize('which', ['two', 'late'])
def test_cached_rounds_with_two_objects_and_a_later_object(clips, cfg, nets, tmp_path, monkeypatch, which):
    _forward_comparison(clips, cfg, nets(), which, tmp_path, monkeypatch)


def test_two_cached_sessions_on_one_network_propagated_alternately(clips, cfg, nets, tmp_path):
    net = nets()
    want = {}
    for which in ('one', 'other'):                           # the cache-off twins, one after the other
        twin = _session(clips, cfg, net, which)
        for ref in (0, 5):
            twin.save_reference(ref)
            twin.full_propagation()
            want[which, ref] = _state(twin, tmp_path)
        del twin
    S = {which: _session(clips, cfg, net, which, WHOLE_CLIP) for which in ('one', 'other')}
    for ref in (0, 5):
        for which in ('one', 'other'):
            S[which].save_reference(ref)
        for turn in range(2):                                # one, other, one, other: the second turn of each is served from its cache
            for which in ('one', 'other'):
                S[which].full_propagation()
                _assert_same(_state(S[which], tmp_path), want[which, ref], f'{which}, reference {ref}, turn {turn}')
    for which in ('one', 'other'):
        assert S[which].cache_info()['hits'] == 3 * T_CLIP and S[which].cache_info()['misses'] == T_CLIP
    assert want['one', 5]['png'] != want['other', 5]['png']


# ---- 8. precision ---------------------------------------------------------------------------------------------------------
def test_cached_rounds_in_the_fp16_loop_hold_halfs(clips, cfg, nets, tmp_path, monkeypatch):
    A, B = _forward_comparison(clips, cfg, nets('fp16'), 'one', tmp_path, monkeypatch, precision='fp16')
    layout = B._fcache.layout
    assert [d for _, d in layout[:3]] == [torch.float32] * 3                    # keys stay fp32 in every mode
    assert all(d == torch.float16 for _, d in layout[3:]) and len(layout) >= 6  # f16 and the extras are activations: halfs
    fp32_entry = sum(int(np.prod(sh)) * 4 for sh, _ in layout)
    assert B.cache_info()['entry_bytes'] < 0.6 * fp32_entry


# ---- 9. the command line --------------------------------------------------------------------------------------------------
def test_session_cli_with_a_feature_cache_writes_the_same_masks(clips, cfg, tmp_path):
    imgs, msks = clips['two']
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = {}
    for name, extra in (('off', []), ('on', ['--feature-cache-gb', '1'])):
        p = subprocess.run([sys.executable, '-m', 'xmem2_amd.session', '--images', imgs, '--masks', msks, '--out', str(tmp_path / name),
                            '--rounds', '2', '--k', '2', '--config', json.dumps(cfg)] + extra, env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        rounds = [json.loads(line) for line in p.stdout.splitlines() if line.startswith('{')]
        assert [r['round'] for r in rounds] == [0, 1]
        out[name] = (rounds, _mask_bytes(tmp_path / name))
    assert out['on'][0] == out['off'][0] and out['on'][1] == out['off'][1] and len(out['on'][1]) == T_CLIP
