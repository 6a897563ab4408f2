"""Every refusal of xmem_temporal_mode returns its code, or raises from `ops`, and leaves `out` and `changed` as they were."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -2
T, H, W, RING = 20, 6, 5, 5


@pytest.fixture()
def buffers():
    frames = torch.randint(0, 3, (RING, H, W), dtype=torch.uint8, device='cuda')
    flags = torch.ones(T, dtype=torch.uint8, device='cuda')
    out = torch.full((4, H, W), 201, dtype=torch.uint8, device='cuda')
    changed = torch.full((4,), -7, dtype=torch.int32, device='cuda')
    yield frames, flags, out, changed
    torch.cuda.synchronize()
    assert bool((out == 201).all()) and bool((changed == -7).all()), 'a refused call wrote'


def _call(buffers, **kw):
    from xmem2_amd import _lib_temporal
    from xmem2_amd._lib import ptr, stream_ptr
    frames, flags, out, changed = buffers
    a = dict(frames=ptr(frames), ring=RING, H=H, W=W, T=T, t0=2, n=1, radius=2, flags=ptr(flags), out=ptr(out), changed=ptr(changed))
    a.update(kw)
    return _lib_temporal.load().xmem_temporal_mode(a['frames'], a['ring'], a['H'], a['W'], a['T'], a['t0'], a['n'], a['radius'], a['flags'],
                                                   a['out'], a['changed'], stream_ptr())


@pytest.mark.parametrize('kw', [
    {'frames': None}, {'flags': None}, {'out': None}, {'changed': None},
    {'radius': 0}, {'radius': 8}, {'radius': -1},
    {'n': 0}, {'n': -1}, {'t0': -1}, {'t0': T}, {'t0': T - 1, 'n': 2},
    {'ring': 0}, {'ring': -1},
    {'ring': 4}, {'n': 2}, {'n': 4}, {'t0': 0, 'ring': 2}, {'t0': T - 1, 'ring': 2},      # a ring too short for the frames the call reads
], ids=str)
def test_bad_arguments(buffers, kw):
    assert _call(buffers, **kw) == BAD_ARG


def test_out_overlapping_the_ring(buffers):
    frames = buffers[0]
    for offset in (0, H * W - 1, RING * H * W - 1):
        assert _call(buffers, out=ctypes.c_void_p(frames.data_ptr() + offset)) == BAD_ARG
    assert _call(buffers, out=ctypes.c_void_p(frames.data_ptr() - 1)) == BAD_ARG          # out [1][H][W] ends inside the ring


@pytest.mark.parametrize('kw', [{'H': 0}, {'W': 0}, {'H': 16385}, {'W': 16385}, {'H': -2}, {'T': 0}, {'T': 65536}], ids=str)
def test_unsupported_sizes(buffers, kw):
    assert _call(buffers, **kw) == UNSUPPORTED


def test_ops_raise(buffers):
    from xmem2_amd import ops
    frames, flags, out, changed = buffers
    one = out[:1]
    for call in (lambda: ops.temporal_mode_ring(frames, T, 2, 1, 0, flags, out=one), lambda: ops.temporal_mode_ring(frames, T, 2, 1, 8, flags, out=one),
                 lambda: ops.temporal_mode_ring(frames, T, 2, 1, True, flags, out=one), lambda: ops.temporal_mode_ring(frames, T, 2, 0, 2, flags, out=one),
                 lambda: ops.temporal_mode_ring(frames, T, -1, 1, 2, flags, out=one), lambda: ops.temporal_mode_ring(frames, T, T, 1, 2, flags, out=one),
                 lambda: ops.temporal_mode_ring(frames, 0, 0, 1, 2, flags, out=one), lambda: ops.temporal_mode_ring(frames, 65536, 0, 1, 2, flags, out=one),
                 lambda: ops.temporal_mode_ring(frames, T, 2, 2, 2, flags, out=out[:2]),          # six frames in five slots
                 lambda: ops.temporal_mode(frames, 0, out=torch.empty_like(frames)), lambda: ops.temporal_mode(frames, 9),
                 lambda: ops.temporal_mode(frames, 1, present=[True])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: ops.temporal_mode_ring(frames, T, 2, 1, 2, flags[:-1], out=one), lambda: ops.temporal_mode_ring(frames, T, 2, 1, 2, flags.cpu(), out=one),
                 lambda: ops.temporal_mode_ring(frames, T, 2, 1, 2, flags.int(), out=one), lambda: ops.temporal_mode_ring(frames[0], T, 2, 1, 2, flags, out=one),
                 lambda: ops.temporal_mode_ring(frames, T, 2, 1, 2, flags, out=out[:2]), lambda: ops.temporal_mode_ring(frames, T, 2, 1, 2, flags, out=one, changed=changed),
                 lambda: ops.temporal_mode_ring(frames, T, 2, 1, 2, flags, out=one, changed=changed[:1].long()),
                 lambda: ops.temporal_mode(frames[0], 1), lambda: ops.temporal_mode(frames.int(), 1)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError, match='status -1'):                                 # the library's own refusal, through ops
        ops.temporal_mode_ring(frames, RING, 0, RING, 1, torch.ones(RING, dtype=torch.uint8, device='cuda'), out=frames)
