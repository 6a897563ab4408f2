"""`ops.temporal_mode` and `ops.temporal_mode_ring` byte for byte against `temporal.mode_host`, at the smallest shapes at which the
kernel can go wrong: frames of one pixel, of fewer than four, of 35 bytes (every frame after the first starts off a dword), of whole
dwords, of several workgroups; videos shorter than, as long as and just longer than the window and the kernel's time segment; labels on
both sides of 0x80; absent and locked frames.  Every case runs twice and once from a captured graph."""
import numpy as np
import pytest
import torch

import temporal_refs as R
from xmem2_amd import temporal

pytestmark = pytest.mark.gpu

LABELS = (0, 1, 127, 128, 255)
SHAPES = [(1, 1), (1, 3), (5, 7), (4, 8), (33, 67)]
RADII = [1, 2, 3, 7]


def _segment():
    from xmem2_amd import _lib_temporal
    return _lib_temporal.SEGMENT


def _lengths(r):
    seg = _segment()
    return sorted({1, 2, r, r + 1, 2 * r, 2 * r + 1, 2 * r + 2, seg - 1, seg, seg + 1, 2 * seg + 3})


def _flags(rng, T, kind):
    if kind == 'random':
        return rng.random(T) < 0.85, rng.random(T) < 0.2
    if kind == 'plain':
        return None, None
    return (np.zeros(T, bool), None) if kind == 'absent' else (None, np.ones(T, bool))


def _run_all_ways(masks, r, present, locked):
    """(out, changed) of ops.temporal_mode, after checking that a second run and a replayed graph give the same bytes"""
    from xmem2_amd import ops
    T = masks.shape[0]
    dev = torch.from_numpy(masks).cuda()
    out, changed = ops.temporal_mode(dev, r, present, locked)
    again, changed_again = ops.temporal_mode(dev, r, present, locked)
    assert torch.equal(out, again) and torch.equal(changed, changed_again)
    assert out.dtype == torch.uint8 and out.shape == dev.shape and changed.dtype == torch.int32 and changed.shape == (T,)
    flags = torch.from_numpy(temporal.frame_flags(T, present, locked)).cuda()
    g_out = torch.full_like(dev, 77)
    g_changed = torch.full((T,), -5, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.temporal_mode_ring(dev, T, 0, T, r, flags, out=g_out, changed=g_changed)
    for _ in range(2):                                               # replayed twice: `changed` is overwritten, not added to
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, out) and torch.equal(g_changed, changed)
    assert torch.equal(dev, torch.from_numpy(masks).cuda())          # the input is read only
    return out.cpu().numpy(), changed.cpu().numpy()


@pytest.mark.parametrize('r', RADII)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_batch_form_is_mode_host(shape, r):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] * 10 + r)
    total = 0
    for T in _lengths(r):
        for kind in ('random', 'plain'):
            masks = R.flicker_stack(rng, T, *shape, LABELS)
            present, locked = _flags(rng, T, kind)
            want, want_changed = temporal.mode_host(masks, r, present, locked)
            got, got_changed = _run_all_ways(masks, r, present, locked)
            np.testing.assert_array_equal(got, want, err_msg=f'T={T} {kind}')
            np.testing.assert_array_equal(got_changed, want_changed, err_msg=f'T={T} {kind}')
            total += int(want_changed.sum()) if kind == 'plain' else 0
    print('pixels changed in the plain cases:', total)
    assert total > 0 or shape == (1, 1)                              # one pixel may happen to flicker nowhere; every other shape must


def test_one_pixel_changes_too():
    masks = np.array([3, 3, 200, 3, 3, 128, 128, 0, 128], np.uint8).reshape(-1, 1, 1)
    want, want_changed = temporal.mode_host(masks, 1)
    got, got_changed = _run_all_ways(masks, 1, None, None)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_changed, want_changed)
    assert want_changed.sum() == 2


@pytest.mark.parametrize('r', RADII)
def test_several_workgroups_and_segments(r):
    rng = np.random.default_rng(r)
    T = _segment() + 2 * r + 2
    masks = R.flicker_stack(rng, T, 96, 128, LABELS, flips=0.1)
    present, locked = _flags(rng, T, 'random')
    want, want_changed = temporal.mode_host(masks, r, present, locked)
    got, got_changed = _run_all_ways(masks, r, present, locked)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_changed, want_changed)
    assert want_changed.sum() > 0


@pytest.mark.parametrize('kind', ['absent', 'locked'])
def test_all_absent_and_all_locked_change_nothing(kind):
    rng = np.random.default_rng(5)
    for r in RADII:
        masks = R.flicker_stack(rng, 2 * r + 2, 5, 7, LABELS)
        present, locked = _flags(rng, masks.shape[0], kind)
        got, got_changed = _run_all_ways(masks, r, present, locked)
        np.testing.assert_array_equal(got, masks)
        assert not got_changed.any()


@pytest.mark.parametrize('r', RADII)
@pytest.mark.parametrize('shape', [(5, 7), (4, 8)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_ring_form_reproduces_the_batch(shape, r):
    from xmem2_amd import ops
    rng = np.random.default_rng(r * 7 + shape[0])
    T = 3 * (2 * r + 1) + 2                                           # the delay line wraps several times
    masks = R.flicker_stack(rng, T, *shape, LABELS)
    present, locked = _flags(rng, T, 'random')
    want, want_changed = temporal.mode_host(masks, r, present, locked)
    dev = torch.from_numpy(masks).cuda()
    flags = torch.from_numpy(temporal.frame_flags(T, present, locked)).cuda()
    # as the frame loop feeds it: 2 r + 1 slots, one frame in, one frame out
    slots = 2 * r + 1
    ring = torch.zeros((slots,) + shape, dtype=torch.uint8, device='cuda')
    outs, counts = [], []

    def emit(t):
        out, changed = ops.temporal_mode_ring(ring, T, t, 1, r, flags)
        outs.append(out)
        counts.append(changed)
    for t in range(T):
        ring[t % slots].copy_(dev[t])
        if t >= r:
            emit(t - r)
    for t in range(max(0, T - r), T):
        emit(t)
    np.testing.assert_array_equal(torch.cat(outs).cpu().numpy(), want)
    np.testing.assert_array_equal(torch.cat(counts).cpu().numpy(), want_changed)
    # four frames per call from a ring of 4 + 2 r slots
    n, slots = 4, 4 + 2 * r
    ring = torch.zeros((slots,) + shape, dtype=torch.uint8, device='cuda')
    outs, counts, loaded = [], [], 0
    for i in range(0, T, n):
        m = min(n, T - i)
        while loaded <= min(T - 1, i + m - 1 + r):
            ring[loaded % slots].copy_(dev[loaded])
            loaded += 1
        out, changed = ops.temporal_mode_ring(ring, T, i, m, r, flags)
        outs.append(out)
        counts.append(changed)
    np.testing.assert_array_equal(torch.cat(outs).cpu().numpy(), want)
    np.testing.assert_array_equal(torch.cat(counts).cpu().numpy(), want_changed)
    assert want_changed.sum() > 0


def test_out_is_the_callers_tensor():
    from xmem2_amd import ops
    rng = np.random.default_rng(11)
    masks = R.flicker_stack(rng, 9, 5, 7, LABELS)
    dev = torch.from_numpy(masks).cuda()
    out = torch.full_like(dev, 9)
    got, changed = ops.temporal_mode(dev, 2, out=out)
    assert got is out
    want, want_changed = temporal.mode_host(masks, 2)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    np.testing.assert_array_equal(changed.cpu().numpy(), want_changed)
    for bad in (torch.empty((9, 5, 8), dtype=torch.uint8, device='cuda'), torch.empty((9, 5, 7), dtype=torch.int32, device='cuda'),
                torch.empty((9, 5, 7), dtype=torch.uint8), torch.empty((9, 7, 5), dtype=torch.uint8, device='cuda').transpose(1, 2)):
        with pytest.raises(RuntimeError, match='out must be'):
            ops.temporal_mode(dev, 2, out=bad)
