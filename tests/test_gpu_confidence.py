"""`ops.confidence_stats` byte for byte against `confidence.stats_host`, at the smallest shapes at which the kernel can go wrong: one
pixel, frames whose size is odd (every channel after the first starts off a 16-byte boundary), every length of the vector tail, more
than one workgroup with a ragged last one, every counter row; scores of k / 256 so that ties and the floor, cap and threshold boundaries
occur in numbers; the uint16 route; null outputs; a sum beyond 2^32; refusals; a captured graph.  Every case runs twice."""
import ctypes

import numpy as np
import pytest
import torch

import confidence_refs as R
from xmem2_amd import confidence as CF

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -2
SHAPES = [(1, 1, 1), (2, 1, 1),                                      # one pixel
          (3, 5, 7), (3, 3, 5), (3, 7, 13),                          # H W odd: every channel after the first starts off a 16-byte boundary
          (2, 1, 9), (2, 1, 10), (2, 1, 11), (2, 3, 6),              # widths of 4k + 1, 4k + 2, 4k + 3: the tails of the element route
          (2, 4, 9), (2, 4, 10), (2, 4, 11), (3, 4, 8),              # the same widths with H W a multiple of 4: the 16-byte route
          (2, 65, 129)]                                              # several workgroups, a ragged last one


def _check(got, want, what):
    for name, g, w in zip(('mask', 'plane', 'record'), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        np.testing.assert_array_equal(g, w, err_msg=f'{what}: {name}')


def _twice(prob, tau, passes=None):
    from xmem2_amd import ops
    dev = torch.from_numpy(prob).cuda()
    first = ops.confidence_stats(dev, tau, passes, want_plane=True)
    again = ops.confidence_stats(dev, tau, passes, want_plane=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), 'the same call twice gave other bytes'
    assert np.array_equal(dev.cpu().numpy(), prob)                   # the input is read only
    return first


@pytest.mark.parametrize('tau', [0, 64, 256])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_float_scores_are_stats_host(shape, tau):
    prob = R.scores(np.random.default_rng(sum(shape) * 1000 + tau), *shape)
    want = CF.stats_host(prob, tau)
    if shape[0] > 1 and shape[1] * shape[2] > 30:
        q = 255 - want[1].astype(int)
        assert (q == 0).any() and (q == 255).any() and ((q > 0) & (q < 255)).any(), 'the drawing shows too little'
    _check(_twice(prob, tau), want, f'{shape} tau {tau}')


def test_every_counter_row():
    from xmem2_amd import ops
    rng = np.random.default_rng(255)
    prob = R.scores(rng, 255, 9, 11)
    for c, p in zip(rng.permutation(255)[:99], range(99)):           # 99 pixels, 99 different winners
        prob[c, p // 11, p % 11] = 1.0 + 8 / 256                      # leads a 1.0 by q = 8: low, and somebody's contested
    want = CF.stats_host(prob, 64)
    assert (want[2][:, 0] > 0).sum() == 99 and (want[2][:, 3] > 0).sum() > 5
    _check(_twice(prob, 64), want, 'C = 255')
    with pytest.raises(ValueError, match='classes'):
        ops.confidence_stats(torch.zeros((256, 9, 11), device='cuda'))


def test_all_zeros():
    P = 7 * 13
    for C in (1, 2, 3):
        mask, plane, record = _twice(np.zeros((C, 7, 13), np.float32), 64)
        want = np.zeros((C, 4), np.int64)
        want[0, 0] = want[0, 2] = P                                  # top = 0, q = 0: low[0] = P
        if C > 1:
            want[1, 3] = P                                           # second = 1: contested[1] = P
        assert not mask.any() and bool((plane == 255).all())
        np.testing.assert_array_equal(record.cpu().numpy(), want)


def test_a_sum_beyond_32_bits():
    """4112 x 4112 with planes of 0 and of 1, built on the device: q = 255 everywhere, so margin_sum = 255 * area > 2^32."""
    from xmem2_amd import ops
    side = 4112
    prob = torch.zeros((2, side, side), device='cuda')
    prob[1].fill_(1.0)
    mask, plane, record = ops.confidence_stats(prob, 64, want_plane=True)
    area = side * side
    assert area == 16908544 and 255 * area > 1 << 32
    assert record.cpu().tolist() == [[0, 0, 0, 0], [area, 255 * area, 0, 0]]
    assert bool((mask == 1).all()) and not plane.any()


@pytest.mark.parametrize('passes', [1, 4, 8])
def test_the_integer_route(passes):
    for shape in ((3, 7, 13), (1, 7, 13), (3, 4, 8), (2, 33, 64)):
        for tau in (0, 64, 256):
            acc = R.sums(np.random.default_rng(passes * 100 + tau + shape[1]), *shape, passes)
            _check(_twice(acc, tau, passes), CF.stats_host(acc, tau, passes), f'{shape} passes {passes} tau {tau}')
    acc = np.zeros((2, 1, 1), np.uint16)
    acc[0] = 65535
    _check(_twice(acc, 64, 257), CF.stats_host(acc, 64, 257), 'passes 257')


def test_null_outputs():
    from xmem2_amd import ops
    prob = R.scores(np.random.default_rng(3), 3, 7, 13)
    dev = torch.from_numpy(prob).cuda()
    want = CF.stats_host(prob, 64)
    for want_mask, want_plane in ((True, False), (False, True), (False, False)):
        mask, plane, record = ops.confidence_stats(dev, 64, want_mask=want_mask, want_plane=want_plane)
        assert (mask is not None) == want_mask and (plane is not None) == want_plane
        if want_mask:
            np.testing.assert_array_equal(mask.cpu().numpy(), want[0])
        if want_plane:
            np.testing.assert_array_equal(plane.cpu().numpy(), want[1])
        np.testing.assert_array_equal(record.cpu().numpy(), want[2])
    # the caller's tensors: a row of a wider table, and planes of its own
    table = torch.full((2, 5, 4), -3, dtype=torch.int64, device='cuda')
    mine = torch.full((7, 13), 99, dtype=torch.uint8, device='cuda')
    mask, plane, record = ops.confidence_stats(dev, 64, want_mask=False, record=table[1, :3], plane=mine)
    assert mask is None and plane is mine and record.data_ptr() == table[1].data_ptr()
    np.testing.assert_array_equal(table[1, :3].cpu().numpy(), want[2])
    np.testing.assert_array_equal(mine.cpu().numpy(), want[1])
    assert bool((table[0] == -3).all()) and bool((table[1, 3:] == -3).all())


def test_the_mask_is_argmax_u8_on_ties():
    from xmem2_amd import ops
    rng = np.random.default_rng(11)
    for shape in ((4, 33, 67), (5, 32, 64), (2, 5, 7)):
        prob = torch.from_numpy((rng.integers(0, 3, size=shape) / 2).astype(np.float32)).cuda()      # three values: ties nearly everywhere
        mask, _, record = ops.confidence_stats(prob)
        assert torch.equal(mask, ops.argmax_u8(prob))
        assert int(record[:, 0].sum()) == shape[1] * shape[2]


def test_refusals_launch_nothing():
    from xmem2_amd import _lib_confidence, ops
    from xmem2_amd._lib import ptr, stream_ptr
    lib = _lib_confidence.load()
    prob = torch.rand((3, 6, 5), device='cuda')
    acc = torch.zeros((3, 6, 5), dtype=torch.uint16, device='cuda')
    mask = torch.full((6, 5), 201, dtype=torch.uint8, device='cuda')
    plane = torch.full((6, 5), 202, dtype=torch.uint8, device='cuda')
    record = torch.full((3, 4), -7, dtype=torch.int64, device='cuda')

    def f32(**kw):
        a = dict(prob=ptr(prob), C=3, H=6, W=5, tau=64, mask=ptr(mask), plane=ptr(plane), record=ptr(record))
        a.update(kw)
        return lib.xmem_confidence_f32(a['prob'], a['C'], a['H'], a['W'], a['tau'], a['mask'], a['plane'], a['record'], stream_ptr())

    def u16(**kw):
        a = dict(acc=ptr(acc), passes=2, C=3, H=6, W=5, tau=64, mask=ptr(mask), plane=ptr(plane), record=ptr(record))
        a.update(kw)
        return lib.xmem_confidence_u16(a['acc'], a['passes'], a['C'], a['H'], a['W'], a['tau'], a['mask'], a['plane'], a['record'], stream_ptr())

    for call in (f32, u16):
        for kw in ({'record': None}, {'record': ctypes.c_void_p(record.data_ptr() + 4)}, {'C': 0}, {'C': 256}, {'tau': -1}, {'tau': 257}):
            assert call(**kw) == BAD_ARG, (call.__name__, kw)
        for kw in ({'H': 0}, {'W': 0}, {'H': 16385}, {'W': 16385}, {'H': -2}):
            assert call(**kw) == UNSUPPORTED, (call.__name__, kw)
    assert f32(prob=None) == BAD_ARG and u16(acc=None) == BAD_ARG
    for passes in (0, -1, 258):
        assert u16(passes=passes) == BAD_ARG
    for call in (lambda: ops.confidence_stats(prob, -1), lambda: ops.confidence_stats(prob, 257), lambda: ops.confidence_stats(prob, True),
                 lambda: ops.confidence_stats(acc, 64, 0), lambda: ops.confidence_stats(acc, 64, 258)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: ops.confidence_stats(prob, 64, 2), lambda: ops.confidence_stats(acc), lambda: ops.confidence_stats(prob[0]),
                 lambda: ops.confidence_stats(prob, record=record[:2]), lambda: ops.confidence_stats(prob, record=record.int()),
                 lambda: ops.confidence_stats(prob, mask=mask[:3]), lambda: ops.confidence_stats(prob, plane=plane.cpu())):
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert bool((mask == 201).all()) and bool((plane == 202).all()) and bool((record == -7).all()), 'a refused call wrote'


def test_a_captured_graph_replayed_twice():
    from xmem2_amd import ops
    prob = R.scores(np.random.default_rng(8), 3, 33, 67)
    want = CF.stats_host(prob, 64)
    dev = torch.from_numpy(prob).cuda()
    mask = torch.full((33, 67), 77, dtype=torch.uint8, device='cuda')
    plane = torch.full((33, 67), 78, dtype=torch.uint8, device='cuda')
    record = torch.full((3, 4), -5, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.confidence_stats(dev, 64, record=record, mask=mask, plane=plane)
    for _ in range(2):                                               # replayed twice: the record is overwritten, not added to
        graph.replay()
    torch.cuda.synchronize()
    _check((mask, plane, record), want, 'graph')
