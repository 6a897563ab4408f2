"""Block motion and the motion-compensated vote on the host: `motion.block_motion_host` and `temporal.mode_mc_host` against
independent oracles (motion_refs.py) and their pinned cases, the pan clip, `parse_smooth`'s new forms, the ninth header with its
binding and its place in the build, the entry points' refusals (which touch no GPU), the delay line with numpy stand-ins for the
kernels, and the command line of `python -m xmem2_amd.rle --smooth --motion`."""
import ctypes
import os
import re

import numpy as np
import pytest

import motion_refs as R
import temporal_refs
from conftest import ROOT
from xmem2_amd import motion, temporal

HEADER = os.path.join(ROOT, 'include', 'xmem_hip_motion.h')
BAD_ARG, UNSUPPORTED = -1, -2


# ---- the definitions --------------------------------------------------------------------------------------------------------------------

def test_luma_host():
    rgb = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]]], np.uint8)
    assert motion.luma_host(rgb).tolist() == [[255, 0, (77 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (29 * 255 + 128) >> 8, (77 + 300 + 87 + 128) >> 8]]
    assert motion.luma_host(np.zeros((2, 4, 5, 3), np.uint8)).shape == (2, 4, 5)
    with pytest.raises(ValueError):
        motion.luma_host(np.zeros((4, 5), np.uint8))


def test_block_motion_host_is_the_oracle():
    for name, cur, ref, S, bias in R.search_cases():
        vec, sad = motion.block_motion_host(cur, ref, S, bias)
        want_vec, want_sad = R.motion_oracle(cur, ref, S, bias)
        np.testing.assert_array_equal(vec, want_vec, err_msg=name)
        np.testing.assert_array_equal(sad, want_sad, err_msg=name)
        assert vec.dtype == np.int8 and sad.dtype == np.int32 and vec.shape == motion.blocks_of(*cur.shape) + (2,)


def test_block_motion_host_pinned_cases():
    for H, W in R.SIZES:
        for S in R.SEARCHES:
            dy, dx = R.shift_for(S)
            cur, ref = R.shifted_pair(np.random.default_rng(H * 1000 + W * 10 + S), H, W, dy, dx)
            vec, sad = motion.block_motion_host(cur, ref, S, 1)
            for by in range(vec.shape[0]):
                for bx in range(vec.shape[1]):
                    y0, y1, x0, x1 = by * 16, min(H, by * 16 + 16), bx * 16, min(W, bx * 16 + 16)
                    if y0 + dy >= 0 and y1 + dy <= H and x0 + dx >= 0 and x1 + dx <= W and (y1 - y0) * (x1 - x0) > 4:
                        assert tuple(vec[by, bx]) == (dy, dx) and sad[by, bx] == 0, (H, W, S, by, bx)
            vec, sad = motion.block_motion_host(np.full((H, W), 9, np.uint8), np.full((H, W), 200, np.uint8), S, 1)
            assert not vec.any() and np.array_equal(sad, 191 * motion.block_pixels(H, W))
    # the tie order: d^2 first, then the smaller dy, then the smaller dx
    vec, _ = motion.block_motion_host(R.stripes(48, 48), R.stripes(48, 48, 2), 7, 0)
    assert vec[1].tolist() == [[0, 2], [0, -2], [0, -2]]                         # dx = -2 leaves the image for the first column of blocks
    vec, _ = motion.block_motion_host(R.stripes(48, 48).T.copy(), R.stripes(48, 48, 2).T.copy(), 7, 0)
    assert vec[:, 1].tolist() == [[2, 0], [-2, 0], [-2, 0]]
    # the zero bias: SAD(0, 0) - best == bias * n stays still, one more moves
    vec, sad = motion.block_motion_host(*R.bias_block(0), 7, 2)
    assert tuple(vec[1, 1]) == (0, 0) and sad[1, 1] == 512
    vec, sad = motion.block_motion_host(*R.bias_block(1), 7, 2)
    assert tuple(vec[1, 1]) == (0, 1) and sad[1, 1] == 0
    vec, sad = motion.block_motion_host(*R.bias_block(1), 7, 3)
    assert tuple(vec[1, 1]) == (0, 0) and sad[1, 1] == 513
    a = np.zeros((4, 4), np.uint8)
    for kw in ({'search': 0}, {'search': 33}, {'bias': -1}, {'bias': 256}, {'search': True}, {'search': 2.0}):
        with pytest.raises(ValueError):
            motion.block_motion_host(a, a, **kw)
    for cur, ref in ((a, a[:3]), (a.astype(np.int32), a), (a[0], a[0])):
        with pytest.raises(ValueError):
            motion.block_motion_host(cur, ref)


def _clip(rng, T, H, W, labels):
    base = rng.integers(0, 256, (H + T + 8, W + 2 * T + 8), dtype=np.uint8)
    luma = np.stack([base[t:t + H, 2 * (T - t):2 * (T - t) + W] for t in range(T)])
    luma = (luma.astype(np.int32) + rng.integers(-3, 4, luma.shape)).clip(0, 255).astype(np.uint8)
    return luma, temporal_refs.flicker_stack(rng, T, H, W, labels, flips=0.25)


@pytest.mark.parametrize('T,r', [(1, 1), (3, 1), (9, 3)])
def test_mode_mc_host_is_the_oracle(T, r):
    rng = np.random.default_rng(T * 10 + r)
    luma, masks = _clip(rng, T, 18, 21, (0, 1, 128, 255))
    flags = [(None, None)] if T < 9 else [(None, None), (rng.random(T) < 0.8, rng.random(T) < 0.25)]
    total = 0
    for present, locked in flags:
        for max_sad in (0, 30, 255):
            got, changed = temporal.mode_mc_host(masks, luma, r, search=3, bias=1, max_sad=max_sad, present=present, locked=locked)
            want, want_changed = R.mode_mc_oracle(masks, luma, r, 3, 1, max_sad, present, locked)
            np.testing.assert_array_equal(got, want, err_msg=f'max_sad {max_sad}')
            np.testing.assert_array_equal(changed, want_changed)
            assert got.dtype == np.uint8 and changed.dtype == np.int64
            if max_sad == 0:                                                     # noisy lumas: every neighbour abstains everywhere
                assert not changed.any()
            total += int(changed.sum())
    assert total > 0 or T == 1


def test_mode_mc_host_without_motion_is_mode_host():
    rng = np.random.default_rng(4)
    masks = temporal_refs.flicker_stack(rng, 8, 17, 19, (0, 1, 2))
    luma = np.broadcast_to(rng.integers(0, 256, (17, 19), dtype=np.uint8), (8, 17, 19)).copy()        # a still video
    present, locked = rng.random(8) < 0.8, rng.random(8) < 0.2
    for r in (1, 2):
        got = temporal.mode_mc_host(masks, luma, r, max_sad=0, present=present, locked=locked)
        want = temporal.mode_host(masks, r, present, locked)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    with pytest.raises(ValueError):
        temporal.mode_mc_host(masks, luma[:, :16], 1)
    for kw in ({'search': 0}, {'max_sad': 256}, {'bias': -1}):
        with pytest.raises(ValueError):
            temporal.mode_mc_host(masks, luma, 1, **kw)


@pytest.mark.parametrize('r,plain_damage', [(1, 87), (2, 803)])
def test_the_pan_clip_comes_back_clean(r, plain_damage):
    luma, clean, noisy = R.pan_clip()
    for t in range(5):                               # the object keeps a block and more from every border (24 px in frame 0)
        ys, xs = np.nonzero(clean[t])
        margin = min(ys.min(), xs.min(), 79 - ys.max(), 111 - xs.max())
        assert margin >= (24 if t == 0 else 16), (t, margin)
    assert int((noisy != clean).sum()) == 25 and set(np.unique(clean)) == {0, 1, 2}
    got, changed = temporal.mode_mc_host(noisy, luma, r, search=8)
    np.testing.assert_array_equal(got, clean)
    assert changed.tolist() == [0, 0, 25, 0, 0]
    plain, _ = temporal.mode_host(noisy, r)
    assert int((plain != clean).sum()) == plain_damage


# ---- the options ------------------------------------------------------------------------------------------------------------------------

def test_parse_smooth_with_motion():
    full = {'search': 16, 'bias': 1, 'max_sad': 24}
    assert temporal.parse_smooth({'radius': 2, 'motion': True}) == {'radius': 2, 'motion': full}
    assert temporal.parse_smooth({'radius': 1, 'motion': {}}) == {'radius': 1, 'motion': full}
    assert temporal.parse_smooth({'radius': 7, 'motion': {'search': 32, 'bias': 0, 'max_sad': 255}}) == \
        {'radius': 7, 'motion': {'search': 32, 'bias': 0, 'max_sad': 255}}
    assert temporal.parse_smooth({'radius': 3, 'motion': {'search': np.int64(1)}})['motion'] == dict(full, search=1)
    assert (motion.SEARCH, motion.BIAS, motion.MAX_SAD, motion.BLOCK, motion.MAX_SEARCH) == (16, 1, 24, 16, 32)
    for bad in ({'radius': 2, 'motion': False}, {'radius': 2, 'motion': None}, {'radius': 2, 'motion': 1}, {'radius': 2, 'motion': 'on'},
                {'radius': 2, 'motion': {'search': 0}}, {'radius': 2, 'motion': {'search': 33}}, {'radius': 2, 'motion': {'bias': -1}},
                {'radius': 2, 'motion': {'bias': 256}}, {'radius': 2, 'motion': {'max_sad': 256}}, {'radius': 2, 'motion': {'max_sad': 1.0}},
                {'radius': 2, 'motion': {'block': 8}}, {'radius': 0, 'motion': True}, {'motion': True},
                {'radius': 2, 'motion': True, 'weights': 1}, {'radius': 2, 'motion': {'search': True}}):
        with pytest.raises(ValueError, match='temporal_smooth'):
            temporal.parse_smooth(bad)
    # the forms of before, unchanged
    assert temporal.parse_smooth({'radius': 2}) == {'radius': 2} and temporal.parse_smooth(3) == {'radius': 3}
    with pytest.raises(ValueError, match='temporal_smooth'):
        temporal.parse_smooth({'radius': 2, 'weights': 1})


# ---- the ninth header, its binding, the build ----------------------------------------------------------------------------------------

def test_ninth_header_parses_and_the_library_exports_it():
    from xmem2_amd import _header, _lib, _lib_motion, _lib_temporal, build
    text = open(HEADER).read()
    constants, structs, sigs = _header.parse(text)
    assert structs == {} and constants == {'XMEM_MOTION_BLOCK': 16, 'XMEM_MOTION_MAX_SEARCH': 32, 'XMEM_MOTION_MAX_N': 65535}
    assert (_lib_motion.BLOCK, _lib_motion.MAX_SEARCH) == (motion.BLOCK, motion.MAX_SEARCH)
    declared = sorted(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S))))
    assert sorted(sigs) == declared == sorted(_lib_motion.EXPORTED_SYMBOLS) == ['xmem_block_motion', 'xmem_luma_u8', 'xmem_motion_window',
                                                                                 'xmem_temporal_mode_mc']
    i, p = ctypes.c_int, ctypes.c_void_p
    assert sigs['xmem_luma_u8'] == (i, [p, i, i, i, p, p])
    assert sigs['xmem_block_motion'] == (i, [p, p] + [i] * 5 + [p, p, p])
    assert sigs['xmem_motion_window'] == (i, [p] + [i] * 7 + [p, i, i, p, p, p])
    assert sigs['xmem_temporal_mode_mc'] == (i, [p] + [i] * 7 + [p, p, p, i, p, p, p])
    lib = _lib_motion.load()
    assert lib is _lib.load()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert not set(sigs) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib_temporal.EXPORTED_SYMBOLS))
    assert len(_lib.EXPORTED_SYMBOLS) == 103 and _lib.ABI_VERSION == 5
    assert build.SOURCES[-1] == 'confidence.hip' and build.SOURCES.index('motion.hip') == len(build.SOURCES) - 2
    assert [os.path.basename(f) for f in build.MOTION_HEADERS] == ['xmem_hip_motion.h'] and 'vote_bytes.hpp' in build.HEADERS


def test_build_tracks_the_ninth_header(tmp_path, monkeypatch):
    from xmem2_amd import build
    assert os.path.samefile(build.MOTION_HEADERS[0], HEADER)
    digest = build.source_digest()
    copy = tmp_path / 'xmem_hip_motion.h'
    copy.write_bytes(open(HEADER, 'rb').read())
    monkeypatch.setattr(build, 'MOTION_HEADERS', [str(copy)])
    assert build.source_digest() == digest
    assert build.needs_build()                                       # the copy is newer than the library
    copy.write_bytes(copy.read_bytes() + b'\n/* changed */\n')
    assert build.source_digest() != digest


def test_the_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib_motion
    lib = _lib_motion.load()
    p = ctypes.c_void_p(4096)                                        # never dereferenced: every call below is refused on the host
    q = ctypes.c_void_p(1 << 30)
    odd = ctypes.c_void_p(4098)

    def luma(rgb=p, N=1, H=8, W=8, out=q):
        return lib.xmem_luma_u8(rgb, N, H, W, out, None)

    def pair(cur=p, ref=p, N=1, H=8, W=8, search=4, bias=1, vec=q, sad=q):
        return lib.xmem_block_motion(cur, ref, N, H, W, search, bias, vec, sad, None)

    def window(luma=p, ring=5, H=8, W=8, T=20, t0=2, n=1, radius=2, flags=p, search=4, bias=1, vec=q, sad=q):
        return lib.xmem_motion_window(luma, ring, H, W, T, t0, n, radius, flags, search, bias, vec, sad, None)

    def vote(frames=p, ring=5, H=8, W=8, T=20, t0=2, n=1, radius=2, flags=p, vec=q, sad=q, max_sad=24, out=q, changed=p):
        return lib.xmem_temporal_mode_mc(frames, ring, H, W, T, t0, n, radius, flags, vec, sad, max_sad, out, changed, None)

    sizes = ({'H': 0}, {'W': 0}, {'H': -1}, {'H': 16385}, {'W': 16385})
    searches = ({'search': 0}, {'search': 33}, {'search': -1}, {'bias': -1}, {'bias': 256})
    windows = ({'radius': 0}, {'radius': 8}, {'n': 0}, {'t0': -1}, {'t0': 20}, {'t0': 18, 'n': 3, 'ring': 20}, {'ring': 0}, {'ring': 4},
               {'n': 4, 'ring': 7}, {'t0': 0, 'ring': 2})
    for fn, pointers in ((luma, ('rgb', 'out')), (pair, ('cur', 'ref', 'vec', 'sad')), (window, ('luma', 'flags', 'vec', 'sad')),
                         (vote, ('frames', 'flags', 'vec', 'sad', 'out', 'changed'))):
        for name in pointers:
            assert fn(**{name: None}) == BAD_ARG, (fn.__name__, name)
        for kw in sizes:
            assert fn(**kw) == UNSUPPORTED, (fn.__name__, kw)
    for fn in (luma, pair):
        assert fn(N=0) == BAD_ARG and fn(N=-2) == BAD_ARG and fn(N=65536) == UNSUPPORTED
    for fn in (pair, window):
        for kw in searches + ({'sad': odd},):
            assert fn(**kw) == BAD_ARG, (fn.__name__, kw)
    for fn in (window, vote):
        for kw in windows:
            assert fn(**kw) == BAD_ARG, (fn.__name__, kw)
        for kw in ({'T': 0}, {'T': 65536}):
            assert fn(**kw) == UNSUPPORTED, (fn.__name__, kw)
    for kw in ({'max_sad': -1}, {'max_sad': 256}, {'sad': odd}, {'changed': odd}):
        assert vote(**kw) == BAD_ARG, kw
    for out in (4096, 4096 + 5 * 64 - 1, 4096 - 63):                 # out [1][8][8] overlaps frames [4096, 4096 + 5 * 64)
        assert vote(out=ctypes.c_void_p(out)) == BAD_ARG, out


def test_ops_refuse_host_tensors_and_bad_options():
    import torch
    from xmem2_amd import ops
    host = torch.zeros((4, 8, 8), dtype=torch.uint8)
    flags = torch.ones(4, dtype=torch.uint8)
    for call in (lambda: ops.block_motion(host[0], host[1]), lambda: ops.temporal_mode_mc(host, host, 1),
                 lambda: ops.motion_window(host, 4, 0, 4, 1, flags), lambda: ops.temporal_mode_mc_ring(host, host, 4, 0, 4, 1, flags),
                 lambda: ops.luma_u8(torch.zeros((8, 8, 3), dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()


# ---- the delay line of the frame loop, on the host ---------------------------------------------------------------------------------------

class _Recorder:
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


def _numpy_stand_ins(launches):
    import torch

    def luma(rgb, out=None):
        out.copy_(torch.from_numpy(motion.luma_host(rgb.numpy())))
        return out

    def vote(ring, lumas, T, t0, n, radius, flags, search=16, bias=1, max_sad=24, out=None, changed=None, vec=None, sad=None):
        slots = ring.shape[0]
        first, last = max(0, t0 - radius), min(T - 1, t0 + n - 1 + radius)
        assert n == 1 and slots == 2 * radius + 1 == lumas.shape[0] and vec.shape[:2] == sad.shape[:2] == (1, 2 * radius)
        window = np.stack([ring[f % slots].numpy() for f in range(first, last + 1)])
        luma_window = np.stack([lumas[f % slots].numpy() for f in range(first, last + 1)])
        fl = flags.numpy()[first:last + 1]
        got, ch = temporal.mode_mc_host(window, luma_window, radius, search, bias, max_sad, (fl & 1) > 0, (fl & 2) > 0)
        changed.copy_(torch.from_numpy(ch[t0 - first:t0 - first + n].astype(np.int32)))
        launches.append(t0)
        return torch.from_numpy(got[t0 - first:t0 - first + n].copy()), changed
    return luma, vote


@pytest.mark.parametrize('r', [1, 2, 3])
def test_the_delay_line_with_motion_hands_every_frame_on_once_in_order(r):
    import torch
    rng = np.random.default_rng(r)
    spec = temporal.parse_smooth({'radius': r, 'motion': {'search': 3, 'max_sad': 40}})
    for T in sorted({1, r, r + 1, 2 * r + 1, 9}):
        base = rng.integers(0, 256, (18 + T, 21 + 2 * T, 3), dtype=np.uint8)
        rgb = np.stack([base[t:t + 18, 2 * (T - t):2 * (T - t) + 21] for t in range(T)])
        masks = temporal_refs.flicker_stack(rng, T, 18, 21, (0, 1, 2), flips=0.3, run=5)
        given = [t in (0, 4) for t in range(T)]
        inner, launches = _Recorder(), []
        luma, vote = _numpy_stand_ins(launches)
        line = temporal.DelayLine(inner, spec, T, 'cpu', vote=vote, luma=luma, frame_of=lambda sample: torch.from_numpy(rgb[sample]))
        buf = torch.empty((18, 21), dtype=torch.uint8)                           # the caller rewrites its tensor every frame
        for t in range(T):
            buf.copy_(torch.from_numpy(masks[t]))
            line.submit(t, t, given[t], buf)
            line.deliver()
        line.drain()
        line.deliver(last=True)
        line.close()
        submits = [c for c in inner.calls if c[0] == 'submit']
        assert [c[1:4] for c in submits] == [(t, t, given[t]) for t in range(T)], T
        assert launches == list(range(T))
        want, want_changed = temporal.mode_mc_host(masks, motion.luma_host(rgb), r, 3, 1, 40, locked=given)
        for c in submits:
            np.testing.assert_array_equal(c[4], want[c[1]], err_msg=f'T={T} frame {c[1]}')
        for i, c in enumerate(inner.calls):
            if c[0] == 'submit':
                assert inner.calls[i + 1] == ('deliver', False), (T, i)
        assert [c[0] for c in inner.calls[-3:]] == ['drain', 'deliver', 'close']
        assert line.report() == {'radius': r, 'pixels_changed': int(want_changed.sum()), 'frames_changed': int((want_changed > 0).sum()),
                                 'motion': {'search': 3, 'bias': 1, 'max_sad': 40}}


def test_the_delay_line_refuses_a_frame_of_another_size_and_a_missing_frame_source():
    import torch
    spec = temporal.parse_smooth({'radius': 1, 'motion': True})
    luma, vote = _numpy_stand_ins([])
    with pytest.raises(ValueError, match='frame_of'):
        temporal.DelayLine(_Recorder(), spec, 3, 'cpu', vote=vote, luma=luma)
    line = temporal.DelayLine(_Recorder(), spec, 3, 'cpu', vote=vote, luma=luma, frame_of=lambda s: torch.zeros((6, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask's size"):
        line.submit(0, None, False, torch.zeros((5, 8), dtype=torch.uint8))


def test_the_frame_loops_name_the_two_ways_out_before_they_start():
    from xmem2_amd import run_on_video as rov
    spec = temporal.parse_smooth({'radius': 1, 'motion': True})
    assert rov._motion_frames(None, False, None) is None and rov._motion_frames({'radius': 1}, False, None) is None
    with pytest.raises(ValueError, match=r"resize_on_device.*size'\] = -1"):
        rov._motion_frames(spec, False, None)
    source = lambda sample: sample
    assert rov._motion_frames(spec, False, source) is source
    assert rov._motion_frames(spec, True, None)(type('S', (), {'src_u8': 5})) == 5


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def test_the_rle_command_line_takes_motion_with_smooth():
    from xmem2_amd import rle
    args = rle.parse_args(['--tracks', 't.json', '--smooth', '2', '--motion', 'frames', '--motion-search', '8', '--out', 'o.json'])
    assert (args.smooth, args.motion, args.motion_search) == (2, 'frames', 8)
    args = rle.parse_args(['--tracks', 't.json', '--smooth', '2', '--motion', 'frames', '--out', 'o.json'])
    assert args.motion == 'frames' and args.motion_search is None
    assert rle.parse_args(['--tracks', 't.json', '--smooth', '2', '--out', 'o.json']).motion is None
    for bad in (['--tracks', 't', '--motion', 'd', '--out', 'o'], ['--tracks', 't', '--smooth', '1', '--motion-search', '8', '--out', 'o'],
                ['--tracks', 't', '--smooth', '1', '--motion', 'd', '--motion-search', '0', '--out', 'o'],
                ['--tracks', 't', '--smooth', '1', '--motion', 'd', '--motion-search', '33', '--out', 'o'],
                ['--tracks', 't', '--smooth', '1', '--motion', 'd', '--grow', '2', '--out', 'o']):
        with pytest.raises(SystemExit):
            rle.parse_args(bad)


def test_frame_lumas_reads_a_directory_and_refuses_another_size_or_count(tmp_path):
    from PIL import Image
    from xmem2_amd import rle
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    for t in range(3):
        Image.fromarray(rgb[t]).save(tmp_path / f'{t:05d}.png')
    (tmp_path / '00000.txt').write_text('not a frame')               # ignored, and does not shift the frames
    lumas = rle.frame_lumas(str(tmp_path), 9, 11, 3)
    np.testing.assert_array_equal(lumas(1, 3), motion.luma_host(rgb[1:3]))
    for count in (2, 4):
        with pytest.raises(ValueError, match='3 frames'):
            rle.frame_lumas(str(tmp_path), 9, 11, count)
    with pytest.raises(ValueError, match="masks' size"):
        rle.frame_lumas(str(tmp_path), 9, 12, 3)(0, 1)


def test_the_ensemble_takes_the_unmirrored_pass_at_the_source_size():
    from xmem2_amd import run_on_video as rov
    assert rov._source_pass([(-1, False)]) == 0
    assert rov._source_pass([(480, False), (-1, True), (-1, False), (-1, False)]) == 2
    assert rov._source_pass([(480, False), (-1, True)]) is None and rov._source_pass([]) is None
    spec = temporal.parse_smooth({'radius': 1, 'motion': True})
    sample = type('S', (), {'rgb_u8': ['small', 'mirrored', 'source'], 'src_u8': 'decoded'})
    assert rov._motion_frames(spec, False, rov._pass_frame(2))(sample) == 'source'
    assert rov._motion_frames(spec, True, rov._pass_frame(None))(sample) == 'decoded'
    with pytest.raises(ValueError, match='resize_on_device'):
        rov._motion_frames(spec, False, rov._pass_frame(rov._source_pass([(480, False), (-1, True)])))
