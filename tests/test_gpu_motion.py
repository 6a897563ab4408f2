"""`ops.luma_u8`, `ops.block_motion`, `ops.motion_window` and `ops.temporal_mode_mc` byte for byte against the host definitions
(`motion.luma_host`, `motion.block_motion_host`, `temporal.mode_mc_host`), at the smallest shapes at which the kernels can go wrong:
images of one pixel, cropped last blocks, rows that start off a dword, a search range most of which lies outside the image, rings
that wrap, absent and locked frames, labels on both sides of 0x80.  Every case runs twice and once from a captured graph."""
import numpy as np
import pytest
import torch

import motion_refs as R
import temporal_refs
from xmem2_amd import motion, temporal

pytestmark = pytest.mark.gpu

LABELS = (0, 1, 127, 128, 255)


def _replayed(call, outs):
    """`call(*outs)` captured into a graph and replayed twice -> outs"""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(*outs)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    return outs


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (33, 50)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_luma_is_luma_host(shape):
    from xmem2_amd import ops
    rng = np.random.default_rng(shape[0])
    for lead in ((), (3,)):
        rgb = rng.integers(0, 256, lead + shape + (3,), dtype=np.uint8)
        rgb.reshape(-1, 3)[0] = 255                                              # the largest sum: 256 * 255 + 128 >> 8 = 255
        dev = torch.from_numpy(rgb).cuda()
        want = torch.from_numpy(motion.luma_host(rgb)).cuda()
        got = ops.luma_u8(dev)
        assert got.dtype == torch.uint8 and torch.equal(got, want) and torch.equal(ops.luma_u8(dev), want)
        out, = _replayed(lambda o: ops.luma_u8(dev, out=o), (torch.full_like(want, 9),))
        assert torch.equal(out, want)
    assert motion.luma_host(np.full((1, 1, 3), 255, np.uint8))[0, 0] == 255


def _search_all_ways(cur, ref, S, bias):
    """(vec, sad) of ops.block_motion, after checking that a second run and a replayed graph give the same bytes"""
    from xmem2_amd import ops
    c, r = torch.from_numpy(cur).cuda(), torch.from_numpy(ref).cuda()
    first = ops.block_motion(c, r, S, bias)
    assert _same(first, ops.block_motion(c, r, S, bias))
    spare = (torch.full_like(first[0], 99), torch.full_like(first[1], -7))
    assert _same(first, _replayed(lambda v, s: ops.block_motion(c, r, S, bias, vec=v, sad=s), spare))
    assert first[0].dtype == torch.int8 and first[1].dtype == torch.int32
    return first


def test_block_motion_is_block_motion_host_on_every_host_case():
    for name, cur, ref, S, bias in R.search_cases():
        want_vec, want_sad = motion.block_motion_host(cur, ref, S, bias)
        vec, sad = _search_all_ways(cur, ref, S, bias)
        assert torch.equal(vec.cpu(), torch.from_numpy(want_vec)), name
        assert torch.equal(sad.cpu(), torch.from_numpy(want_sad)), name


def test_block_motion_of_several_noise_pairs():
    rng = np.random.default_rng(8)
    cur = rng.integers(0, 256, (3, 80, 112), dtype=np.uint8)
    ref = rng.integers(0, 256, (3, 80, 112), dtype=np.uint8)
    ref[1] = np.roll(cur[1], (3, -5), (0, 1))                                    # one pair that does move
    want = [motion.block_motion_host(cur[i], ref[i], 8, 0) for i in range(3)]
    vec, sad = _search_all_ways(cur, ref, 8, 0)
    assert vec.shape == (3, 5, 7, 2) and sad.shape == (3, 5, 7)
    assert torch.equal(vec.cpu(), torch.from_numpy(np.stack([w[0] for w in want])))
    assert torch.equal(sad.cpu(), torch.from_numpy(np.stack([w[1] for w in want])))
    assert (want[1][0][1:4, 1:6] == (3, -5)).all() and np.stack([w[0] for w in want])[[0, 2]].any()


def test_block_motion_where_most_candidates_leave_the_image():
    rng = np.random.default_rng(9)
    cur, ref = R.shifted_pair(rng, 40, 70, -20, 31)
    want_vec, want_sad = motion.block_motion_host(cur, ref, 32, 1)
    vec, sad = _search_all_ways(cur, ref, 32, 1)
    assert torch.equal(vec.cpu(), torch.from_numpy(want_vec)) and torch.equal(sad.cpu(), torch.from_numpy(want_sad))
    assert tuple(want_vec[2, 0]) == (-20, 31) and want_sad[2, 0] == 0


def _window_want(luma, r, S, bias, flags, t0, n):
    T, H, W = luma.shape
    By, Bx = motion.blocks_of(H, W)
    vec = np.zeros((n, 2 * r, By, Bx, 2), np.int8)
    sad = np.full((n, 2 * r, By, Bx), -1, np.int32)
    for i in range(n):
        t = t0 + i
        for e, j in enumerate([j for j in range(-r, r + 1) if j]):
            if 0 <= t + j < T and flags[t] == 1 and flags[t + j] & 1:
                vec[i, e], sad[i, e] = motion.block_motion_host(luma[t], luma[t + j], S, bias)
    return vec, sad


@pytest.mark.parametrize('r', [1, 2])
def test_motion_window_is_the_search_of_every_pair(r):
    from xmem2_amd import ops
    rng = np.random.default_rng(r)
    T, H, W, S = 7, 33, 50, 4
    base = rng.integers(0, 256, (H + 40, W + 40), dtype=np.uint8)
    luma = np.stack([base[20 + t:20 + t + H, 20 - 2 * t + 6:20 - 2 * t + 6 + W] for t in range(T)])
    flags = temporal.frame_flags(T, [True, True, False, True, True, True, True], [False, False, False, False, True, False, False])
    fl = torch.from_numpy(flags).cuda()
    dev = torch.from_numpy(luma).cuda()
    for t0, n in ((0, T), (2, 3)):                                               # ring = T
        want = _window_want(luma, r, S, 1, flags, t0, n)
        got = ops.motion_window(dev, T, t0, n, r, fl, S, 1)
        assert _same(got, ops.motion_window(dev, T, t0, n, r, fl, S, 1))
        spare = (torch.full_like(got[0], 5), torch.full_like(got[1], 5))
        assert _same(got, _replayed(lambda v, s: ops.motion_window(dev, T, t0, n, r, fl, S, 1, vec=v, sad=s), spare))
        assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
        assert (want[1] == -1).any() and (want[1] >= 0).any() and want[0].any()
    slots = 2 * r + 1                                                            # ring = 2 r + 1, fed frame by frame
    ring = torch.zeros((slots, H, W), dtype=torch.uint8, device='cuda')
    want = _window_want(luma, r, S, 1, flags, 0, T)
    emitted = []
    for t in range(T + r):
        if t < T:
            ring[t % slots].copy_(dev[t])
        if t >= r:
            emitted.append(ops.motion_window(ring, T, t - r, 1, r, fl, S, 1))
    assert torch.equal(torch.cat([e[0] for e in emitted]).cpu(), torch.from_numpy(want[0]))
    assert torch.equal(torch.cat([e[1] for e in emitted]).cpu(), torch.from_numpy(want[1]))


def _vote_all_ways(masks, luma, r, present=None, locked=None, **kw):
    from xmem2_amd import ops
    T = masks.shape[0]
    m, l = torch.from_numpy(masks).cuda(), torch.from_numpy(luma).cuda()
    first = ops.temporal_mode_mc(m, l, r, present=present, locked=locked, **kw)
    assert _same(first, ops.temporal_mode_mc(m, l, r, present=present, locked=locked, **kw))
    flags = torch.from_numpy(temporal.frame_flags(T, present, locked)).cuda()
    vec, sad = ops.motion_window(l, T, 0, T, r, flags, kw.get('search', 16), kw.get('bias', 1))
    spare = (torch.full_like(m, 77), torch.full((T,), -5, dtype=torch.int32, device='cuda'))
    got = _replayed(lambda o, c: ops.temporal_mode_mc_ring(m, l, T, 0, T, r, flags, out=o, changed=c, vec=vec, sad=sad, **kw), spare)
    assert _same(first, got)
    assert torch.equal(m, torch.from_numpy(masks).cuda())                        # the input is read only
    assert first[0].dtype == torch.uint8 and first[1].dtype == torch.int32 and first[1].shape == (T,)
    return first[0].cpu().numpy(), first[1].cpu().numpy()


def _moving_clip(rng, T, H, W):
    """lumas that pan by (1, -2) a frame with a little noise, and masks that flicker"""
    base = rng.integers(0, 256, (H + 2 * T + 8, W + 4 * T + 8), dtype=np.uint8)
    luma = np.stack([base[t:t + H, 2 * (T - t):2 * (T - t) + W] for t in range(T)])
    luma = (luma.astype(np.int32) + rng.integers(-3, 4, luma.shape)).clip(0, 255).astype(np.uint8)
    return luma, temporal_refs.flicker_stack(rng, T, H, W, LABELS, flips=0.2)


@pytest.mark.parametrize('shape,T,r', [((15, 17), 6, 1), ((9, 3), 6, 2), ((1, 1), 3, 1), ((33, 50), 1, 1), ((20, 36), 16, 1),
                                       ((20, 36), 16, 3), ((20, 36), 16, 7)], ids=str)
def test_compensated_vote_is_mode_mc_host(shape, T, r):
    rng = np.random.default_rng(shape[0] * 100 + T * 10 + r)
    luma, masks = _moving_clip(rng, T, *shape)
    present = rng.random(T) < 0.85 if T > 6 else None
    locked = rng.random(T) < 0.2 if T > 6 else None
    total = 0
    for max_sad in (0, 24, 255):
        kw = {'search': 4, 'bias': 1, 'max_sad': max_sad}
        want, want_changed = temporal.mode_mc_host(masks, luma, r, present=present, locked=locked, **kw)
        got, got_changed = _vote_all_ways(masks, luma, r, present, locked, **kw)
        np.testing.assert_array_equal(got, want, err_msg=f'max_sad {max_sad}')
        np.testing.assert_array_equal(got_changed, want_changed, err_msg=f'max_sad {max_sad}')
        total += int(want_changed.sum())
    assert total > 0 or T == 1 or shape == (1, 1)


def test_the_pan_clip_comes_back_clean():
    luma, clean, noisy = R.pan_clip()
    for r in (1, 2):
        got, changed = _vote_all_ways(noisy, luma, r, search=8)
        np.testing.assert_array_equal(got, clean)
        assert changed.tolist() == [0, 0, 25, 0, 0]


def test_outputs_are_the_callers_tensors_and_bad_ones_are_refused():
    from xmem2_amd import ops
    luma, clean, noisy = R.pan_clip()
    m, l = torch.from_numpy(noisy).cuda(), torch.from_numpy(luma).cuda()
    out = torch.full_like(m, 9)
    got, _ = ops.temporal_mode_mc(m, l, 1, search=8, out=out)
    assert got is out and torch.equal(out.cpu(), torch.from_numpy(clean))
    with pytest.raises(RuntimeError, match='out must be'):
        ops.temporal_mode_mc(m, l, 1, out=torch.empty((5, 80, 113), dtype=torch.uint8, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.temporal_mode_mc(m, l[:, :, :100], 1)
    with pytest.raises(RuntimeError, match='vec must be'):
        ops.block_motion(l[0], l[1], vec=torch.empty((5, 7, 2), dtype=torch.int32, device='cuda'))
    for bad in ({'search': 0}, {'search': 33}, {'bias': 256}, {'max_sad': -1}, {'max_sad': 256}, {'search': True}):
        with pytest.raises(ValueError):
            ops.temporal_mode_mc(m, l, 1, **bad)
