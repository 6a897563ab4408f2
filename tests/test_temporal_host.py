"""The temporal majority vote on the host: `temporal.mode_host` against an independent oracle and its pinned cases, `parse_smooth`,
the sixth header with its binding and its place in the build, the entry point's refusals (which touch no GPU), the delay line of the
frame loop with a numpy vote in place of the kernel, and the command line of `python -m xmem2_amd.rle --smooth`."""
import ctypes
import os
import re

import numpy as np
import pytest

import temporal_refs as R
from conftest import ROOT
from xmem2_amd import temporal

HEADER = os.path.join(ROOT, 'include', 'xmem_hip_temporal.h')
BAD_ARG, UNSUPPORTED = -1, -2


def _col(values):
    return np.array(values, np.uint8).reshape(-1, 1, 1)


def _vote(values, r, **kw):
    out, changed = temporal.mode_host(_col(values), r, **kw)
    return out.ravel().tolist(), changed.tolist()


# ---- the definition ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('labels', [(0, 1), (0, 1, 2, 3), (0, 127, 128, 255)])
def test_mode_host_is_the_oracle(labels):
    rng = np.random.default_rng(len(labels) * 1000 + labels[-1])
    changed_any = 0
    for T in range(1, 21):
        for r in range(1, temporal.MAX_R + 1):
            masks = R.flicker_stack(rng, T, 3, 4, labels, flips=0.3, run=4)
            present = rng.random(T) < 0.85 if T % 3 else None
            locked = rng.random(T) < 0.2 if T % 2 else None
            got, got_changed = temporal.mode_host(masks, r, present, locked)
            want, want_changed = R.mode_oracle(masks, r, present, locked)
            np.testing.assert_array_equal(got, want, err_msg=f'T={T} r={r}')
            np.testing.assert_array_equal(got_changed, want_changed, err_msg=f'T={T} r={r}')
            assert got.dtype == np.uint8 and got_changed.dtype == np.int64
            changed_any += int(got_changed.sum())
    assert changed_any > 0


def test_pinned_cases():
    for r in range(1, temporal.MAX_R + 1):
        assert _vote([9], r) == ([9], [0])                                      # T = 1
    assert _vote([1, 2], 1) == ([1, 2], [0, 0])                                 # the tie goes to the centre
    assert _vote([1, 1, 3, 2, 2], 2)[0][2] == 1                                 # the tie excludes the centre: the smaller label
    assert _vote([0, 5, 0], 1) == ([0, 0, 0], [0, 1, 0])
    assert _vote([0, 5, 0], 1, locked=[False, True, False]) == ([0, 5, 0], [0, 0, 0])
    assert _vote([5, 0, 5], 1, locked=[True, False, False])[0][1] == 5          # a locked frame votes
    # an absent frame neither votes nor changes: without frame 1 the window of frame 2 is {7, 3} and the centre keeps its 3
    assert _vote([7, 7, 3, 3], 1, present=[True, False, True, True])[0] == [7, 7, 3, 3]
    assert _vote([7, 7, 3, 7], 1)[0] == [7, 7, 7, 7]
    assert _vote([7, 7, 3, 7], 1, present=[True, True, False, True]) == ([7, 7, 3, 7], [0, 0, 0, 0])
    # nothing exists outside the video: frame 0 at r = 2 sees three frames, not five
    assert _vote([4, 6, 6, 4, 4], 2)[0][0] == 6
    # every output comes from the input: a cascade would turn the whole row to 1
    assert _vote([1, 1, 2, 1, 2, 2], 1)[0] == [1, 1, 1, 2, 2, 2]
    masks = np.zeros((3, 4, 5), np.uint8)
    masks[1, 1, 1:4] = 200
    masks[1, 3, 0] = 128
    out, changed = temporal.mode_host(masks, 1)
    assert not out.any() and changed.tolist() == [0, 4, 0]                      # `changed` counts exactly the differing pixels
    for bad in (0, 8, -1, True, 1.0, None):
        with pytest.raises(ValueError, match='radius'):
            temporal.mode_host(masks, bad)
    with pytest.raises(ValueError):
        temporal.mode_host(masks.astype(np.int32), 1)
    with pytest.raises(ValueError):
        temporal.mode_host(masks, 1, present=[True])


def test_parse_smooth():
    assert temporal.parse_smooth(None) is None and temporal.parse_smooth(False) is None
    assert temporal.parse_smooth(True) == {'radius': 1}
    for r in range(1, temporal.MAX_R + 1):
        assert temporal.parse_smooth(r) == temporal.parse_smooth({'radius': r}) == temporal.parse_smooth(np.int64(r)) == {'radius': r}
    for bad in (0, 8, -2, 1.0, '2', [2], {}, {'radius': 0}, {'radius': 8}, {'radius': True}, {'radius': 2, 'weights': 1}, {'r': 2}):
        with pytest.raises(ValueError, match='temporal_smooth'):
            temporal.parse_smooth(bad)


# ---- the sixth header, its binding, the build ----------------------------------------------------------------------------------------

def test_sixth_header_parses_and_the_library_exports_it():
    from xmem2_amd import _header, _lib, _lib_masks, _lib_matte, _lib_polygons, _lib_raster, _lib_temporal, build
    text = open(HEADER).read()
    constants, structs, sigs = _header.parse(text)
    assert structs == {} and constants == {'XMEM_TEMPORAL_MAX_R': 7, 'XMEM_TEMPORAL_PRESENT': 1, 'XMEM_TEMPORAL_LOCKED': 2,
                                           'XMEM_TEMPORAL_SEGMENT': _lib_temporal.SEGMENT}
    assert (_lib_temporal.MAX_R, _lib_temporal.PRESENT, _lib_temporal.LOCKED) == (7, 1, 2) and temporal.MAX_R == 7
    assert _lib_temporal.SEGMENT >= 1
    declared = sorted(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S))))
    assert sorted(sigs) == declared == sorted(_lib_temporal.EXPORTED_SYMBOLS) == ['xmem_temporal_mode']
    i, p = ctypes.c_int, ctypes.c_void_p
    assert sigs['xmem_temporal_mode'] == (i, [p] + [i] * 7 + [p, p, p, p])
    lib = _lib_temporal.load()
    assert lib is _lib.load()
    fn = lib.xmem_temporal_mode
    assert fn.restype is i and list(fn.argtypes) == sigs['xmem_temporal_mode'][1]
    others = (set(_lib.EXPORTED_SYMBOLS) | set(_lib_masks.EXPORTED_SYMBOLS) | set(_lib_polygons.EXPORTED_SYMBOLS)
              | set(_lib_raster.EXPORTED_SYMBOLS) | set(_lib_matte.EXPORTED_SYMBOLS))
    assert not set(sigs) & others and len(_lib.EXPORTED_SYMBOLS) == 103 and _lib.ABI_VERSION == 5
    assert 'temporal.hip' in build.SOURCES and [os.path.basename(f) for f in build.TEMPORAL_HEADERS] == ['xmem_hip_temporal.h']
    assert np.array_equal(temporal.frame_flags(3, [1, 0, 1], [0, 0, 1]), [_lib_temporal.PRESENT, 0, _lib_temporal.PRESENT | _lib_temporal.LOCKED])


def test_build_tracks_the_sixth_header(tmp_path, monkeypatch):
    from xmem2_amd import build
    assert os.path.samefile(build.TEMPORAL_HEADERS[0], HEADER)
    digest = build.source_digest()
    copy = tmp_path / 'xmem_hip_temporal.h'
    copy.write_bytes(open(HEADER, 'rb').read())
    monkeypatch.setattr(build, 'TEMPORAL_HEADERS', [str(copy)])
    assert build.source_digest() == digest
    assert build.needs_build()                                       # the copy is newer than the library
    copy.write_bytes(copy.read_bytes() + b'\n/* changed */\n')
    assert build.source_digest() != digest


def test_the_entry_point_refuses_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib_temporal
    lib = _lib_temporal.load()
    p = ctypes.c_void_p(4096)                                        # never dereferenced: every call below is refused on the host
    q = ctypes.c_void_p(1 << 30)

    def mode(frames=p, ring=5, H=8, W=8, T=20, t0=2, n=1, radius=2, flags=p, out=q, changed=p):
        return lib.xmem_temporal_mode(frames, ring, H, W, T, t0, n, radius, flags, out, changed, None)

    for name in ('frames', 'flags', 'out', 'changed'):
        assert mode(**{name: None}) == BAD_ARG, name
    for kw in ({'radius': 0}, {'radius': 8}, {'radius': -1}, {'n': 0}, {'n': -3}, {'t0': -1}, {'t0': 20}, {'t0': 18, 'n': 3, 'ring': 20},
               {'ring': 0}, {'ring': -5}, {'ring': 4}, {'n': 4, 'ring': 7}, {'t0': 0, 'ring': 2}, {'t0': 19, 'ring': 2},
               {'changed': ctypes.c_void_p(4098)}):
        assert mode(**kw) == BAD_ARG, kw
    for kw in ({'H': 0}, {'W': 0}, {'H': -1}, {'H': 16385}, {'W': 16385}, {'T': 0}, {'T': 65536}, {'T': -4}):
        assert mode(**kw) == UNSUPPORTED, kw
    for out in (4096, 4096 + 5 * 64 - 1, 4096 - 63):                 # out [1][8][8] overlaps frames [4096, 4096 + 5 * 64)
        assert mode(out=ctypes.c_void_p(out)) == BAD_ARG, out


def test_ops_refuse_host_tensors_and_bad_options():
    import torch
    from xmem2_amd import ops
    host = torch.zeros((4, 8, 8), dtype=torch.uint8)
    flags = torch.ones(4, dtype=torch.uint8)
    for call in (lambda: ops.temporal_mode(host, 1), lambda: ops.temporal_mode_ring(host, 4, 0, 4, 1, flags)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()


# ---- the delay line of the frame loop, on the host ---------------------------------------------------------------------------------------

class _Recorder:
    """what the delay line sees of `_FrameOutputs`: every call, in order"""

    def __init__(self):
        self.calls, self.stats = [], []

    def submit(self, ti, sample, had_mask, out_dev):
        self.calls.append(('submit', ti, sample, had_mask, out_dev.numpy().copy()))

    def deliver(self, last=False):
        self.calls.append(('deliver', last))

    def drain(self):
        self.calls.append(('drain',))

    def close(self):
        self.calls.append(('close',))


def _numpy_vote(calls):
    import torch

    def vote(ring, T, t0, n, radius, flags, out=None, changed=None):
        slots = ring.shape[0]
        first, last = max(0, t0 - radius), min(T - 1, t0 + n - 1 + radius)
        assert n == 1 and slots == 2 * radius + 1 and last - first + 1 <= slots
        window = np.stack([ring[f % slots].numpy() for f in range(first, last + 1)])
        fl = flags.numpy()[first:last + 1]
        got, ch = temporal.mode_host(window, radius, (fl & 1) > 0, (fl & 2) > 0)
        changed.copy_(torch.from_numpy(ch[t0 - first:t0 - first + n].astype(np.int32)))
        calls.append(t0)
        return torch.from_numpy(got[t0 - first:t0 - first + n].copy()), changed
    return vote


@pytest.mark.parametrize('r', [1, 2, 3])
def test_the_delay_line_hands_every_frame_on_once_in_order(r):
    import torch
    rng = np.random.default_rng(r)
    for T in sorted({1, r, r + 1, 2 * r + 1, 12}):
        masks = R.flicker_stack(rng, T, 5, 7, (0, 1, 2), flips=0.3, run=5)
        given = [t in (0, 4) for t in range(T)]
        inner, launches = _Recorder(), []
        line = temporal.DelayLine(inner, {'radius': r}, T, 'cpu', vote=_numpy_vote(launches))
        assert line.stats is inner.stats
        buf = torch.empty((5, 7), dtype=torch.uint8)                             # the caller rewrites its tensor every frame
        for t in range(T):                                                       # as _run_frame_loop calls it
            buf.copy_(torch.from_numpy(masks[t]))
            line.submit(t, f'sample{t}', given[t], buf)
            line.deliver()
        line.drain()
        line.deliver(last=True)
        line.close()
        calls = inner.calls
        submits = [c for c in calls if c[0] == 'submit']
        assert [c[1:4] for c in submits] == [(t, f'sample{t}', given[t]) for t in range(T)], T
        assert launches == list(range(T))
        want, want_changed = temporal.mode_host(masks, r, locked=given)
        for c in submits:
            np.testing.assert_array_equal(c[4], want[c[1]], err_msg=f'T={T} frame {c[1]}')
        for i, c in enumerate(calls):                                            # a deliver follows every submit, delayed ones included
            if c[0] == 'submit':
                assert calls[i + 1] == ('deliver', False), (T, i)
        assert [c[0] for c in calls[-3:]] == ['drain', 'deliver', 'close'] and calls[-2] == ('deliver', True)
        assert sum(1 for c in calls if c[0] == 'drain') == 1
        assert line.report() == {'radius': r, 'pixels_changed': int(want_changed.sum()), 'frames_changed': int((want_changed > 0).sum())}


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def test_the_rle_command_line_takes_smooth_alone():
    from xmem2_amd import rle
    args = rle.parse_args(['--tracks', 't.json', '--smooth', '2', '--lock', '0,17,40', '--out', 'o.json'])
    assert args.smooth == 2 and args.lock == [0, 17, 40]
    assert rle.parse_args(['--tracks', 't.json', '--smooth', '7', '--out', 'o.json']).lock is None
    assert rle.parse_args(['--tracks', 't.json', '--out', 'o']).smooth is None
    base = ['--tracks', 't.json', '--smooth', '2', '--out', 'o.json']
    for extra in (['--clean', '{"min_area": 4}'], ['--grow', '2'], ['--polygons'], ['--polygons', '1.5'], ['--recode', 'compressed'],
                  ['--recode', 'list'], ['--from-polygons'], ['--verify-polygons']):
        with pytest.raises(SystemExit):
            rle.parse_args(base + extra)
    for bad in (['--tracks', 't', '--smooth', '0', '--out', 'o'], ['--tracks', 't', '--smooth', '8', '--out', 'o'],
                ['--tracks', 't', '--smooth', 'x', '--out', 'o'], ['--tracks', 't', '--lock', '1', '--out', 'o'],
                ['--tracks', 't', '--smooth', '1', '--lock', 'a,b', '--out', 'o'], ['--from-labelme', 'd', '--smooth', '1', '--out', 'o'],
                ['--tracks', 't', '--smooth', '1']):
        with pytest.raises(SystemExit):
            rle.parse_args(bad)
