"""ops.components / ops.clean_masks (csrc/components.hip) against the host definition (xmem2_amd/mask_cleanup.py), bit for bit: root,
area, out and stats.  Shapes around the 32 x 32 tile a workgroup resolves, every pattern of cleanup_refs.py, N = 3 frames in one call
and one 480 x 854 frame.  Every case runs twice into fresh outputs: the bytes are the same."""
import numpy as np
import pytest
import torch

import cleanup_refs as R
from xmem2_amd import mask_cleanup as M
from xmem2_amd import ops

pytestmark = pytest.mark.gpu

_HOST = {}


def _host(key, m):
    """the definition of a case, computed once: {4: (root, area), 8: (root, area), args: (out, stats)}"""
    if key not in _HOST:
        ref = {c: M.components_host(m, c) for c in (4, 8)}
        ref.update({a: M.clean_host(m, *a) for a in R.CLEAN_ARGS})
        _HOST[key] = ref
    return _HOST[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(key, m):
    ref = _host(key, m)
    d = _dev(m)
    for conn in (4, 8):
        root, area = ops.components(d, conn)
        root2, area2 = ops.components(d.clone(), conn)
        assert root.dtype == area.dtype == torch.int32 and root.shape == area.shape == d.shape
        assert (root.cpu().numpy() == ref[conn][0]).all(), (key, conn, 'root')
        assert (area.cpu().numpy() == ref[conn][1]).all(), (key, conn, 'area')
        assert torch.equal(root, root2) and torch.equal(area, area2)
    for args in R.CLEAN_ARGS:
        out, stats = ops.clean_masks(d, *args)
        out2, stats2 = ops.clean_masks(d.clone(), *args)
        assert out.dtype == torch.uint8 and out.shape == d.shape and stats.dtype == torch.int32 and tuple(stats.shape) == (4,)
        assert stats.cpu().tolist() == ref[args][1].tolist(), (key, args)
        assert (out.cpu().numpy() == ref[args][0]).all(), (key, args)
        assert torch.equal(out, out2) and torch.equal(stats, stats2)
    assert (d.cpu().numpy() == m).all()                              # the input is read only


@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_random_masks(shape):
    for K, p in R.RANDOM:
        _check(('random', shape, K, p), R.random_mask(*shape, K, p))


@pytest.mark.parametrize('name', sorted(R.patterns()))
def test_patterns(name):
    _check(name, R.patterns()[name])


@pytest.mark.parametrize('shape', ((1, 1), (70, 1), (65, 129)), ids=lambda s: f'{s[0]}x{s[1]}')
def test_uniform_and_checkerboard_at_edge_shapes(shape):
    _check(('zeros', shape), np.zeros(shape, np.uint8))
    _check(('label', shape), np.full(shape, 255, np.uint8))
    _check(('checkerboard', shape), R.checkerboard(*shape))


def test_random_masks_fire_every_rule():
    for K, p in R.RANDOM:
        assert _host(('random', (64, 64), K, p), R.random_mask(64, 64, K, p))[(4, 6, False)][1].min() > 0


def test_three_frames_in_one_call():
    frames = [R.random_mask(65, 129, 3, .5), R.checkerboard(65, 129), R.random_mask(65, 129, 1, .6, seed=5)]
    d = _dev(np.stack(frames))
    for conn in (4, 8):
        root, area = ops.components(d, conn)
        for i, m in enumerate(frames):
            ref = _host(('n3', i), m)
            assert (root[i].cpu().numpy() == ref[conn][0]).all() and (area[i].cpu().numpy() == ref[conn][1]).all(), (i, conn)
    for args in R.CLEAN_ARGS:
        mine = torch.full(d.shape, 9, dtype=torch.uint8, device=d.device)
        out, stats = ops.clean_masks(d, *args, out=mine)
        assert out is mine and tuple(stats.shape) == (3, 4)
        for i, m in enumerate(frames):
            ref = _host(('n3', i), m)
            assert stats[i].cpu().tolist() == ref[args][1].tolist() and (out[i].cpu().numpy() == ref[args][0]).all(), (i, args)
        again = ops.clean_masks(d, *args)
        assert torch.equal(again[0], out) and torch.equal(again[1], stats)


def test_product_size_frame():
    _check('480p', R.blobs_480p())


def test_out_must_not_alias_the_input_and_options_are_validated():
    d = _dev(R.random_mask(33, 65, 3, .5))
    with pytest.raises(RuntimeError, match='status -1'):
        ops.clean_masks(d, min_area=3, out=d)
    with pytest.raises(RuntimeError):
        ops.clean_masks(d, min_area=3, out=torch.empty(33, 64, dtype=torch.uint8, device=d.device))
    with pytest.raises(ValueError):
        ops.clean_masks(d, max_hole=-1)
    with pytest.raises(RuntimeError):
        ops.components(d.to(torch.int32))


def test_call_is_capturable_and_replays_the_same_bytes():
    """No read-back and no host synchronisation inside the call: it can be captured, and the replay on new contents is right."""
    a, b = R.random_mask(65, 129, 3, .5), R.random_mask(65, 129, 3, .8, seed=3)
    d = _dev(a)
    out = torch.empty_like(d)
    ops.clean_masks(d, 4, 6, True, out=out)                           # the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, stats = ops.clean_masks(d, 4, 6, True, out=out)
    for m in (b, a):
        d.copy_(_dev(m))
        g.replay()
        ref_out, ref_stats = M.clean_host(m, 4, 6, True)
        assert (out.cpu().numpy() == ref_out).all() and stats.cpu().tolist() == ref_stats.tolist()
