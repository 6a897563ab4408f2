"""Every refusal of xmem_png_encode returns its code, or raises from `ops`, and leaves `meta`, `out` and the workspace as they were."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
N, H, W, CAPACITY = 2, 6, 5, 96


@pytest.fixture()
def buffers():
    from xmem2_amd import _lib_png
    planes = torch.randint(0, 3, (N, H, W), dtype=torch.uint8, device='cuda')
    table = torch.arange(768, dtype=torch.int32, device='cuda').to(torch.uint8)
    meta = torch.full((N, _lib_png.META), -7, dtype=torch.int32, device='cuda')
    out = torch.full((N * CAPACITY,), 201, dtype=torch.uint8, device='cuda')
    ws = torch.full((_lib_png.load().xmem_png_workspace_bytes(N, H, W, 3),), 77, dtype=torch.uint8, device='cuda')
    yield planes, table, meta, out, ws
    torch.cuda.synchronize()
    assert bool((meta == -7).all()) and bool((out == 201).all()) and bool((ws == 77).all()), 'a refused call wrote'


def _call(buffers, **kw):
    from xmem2_amd import _lib_png
    from xmem2_amd._lib import ptr, stream_ptr
    planes, table, meta, out, ws = buffers
    a = dict(planes=ptr(planes), N=N, H=H, W=W, color_type=0, table=None, palette=None, capacity=CAPACITY, meta=ptr(meta), out=ptr(out),
             ws=ptr(ws), nbytes=ws.numel())
    a.update(kw)
    return _lib_png.load().xmem_png_encode(a['planes'], a['N'], a['H'], a['W'], a['color_type'], a['table'], a['palette'], a['capacity'],
                                           a['meta'], a['out'], a['ws'], a['nbytes'], stream_ptr())


def test_the_code_of_a_short_workspace_is_the_librarys():
    from xmem2_amd import _lib
    assert _lib.CONSTANTS['XMEM_ERR_BAD_ARG'] == BAD_ARG and _lib.CONSTANTS['XMEM_ERR_UNSUPPORTED'] == UNSUPPORTED
    assert _lib.CONSTANTS['XMEM_ERR_WORKSPACE'] == WORKSPACE


@pytest.mark.parametrize('kw', [
    {'planes': None}, {'meta': None}, {'out': None}, {'ws': None},
    {'capacity': 0}, {'capacity': -1},
    {'color_type': 1}, {'color_type': 4}, {'color_type': -1}, {'color_type': 6},
    {'color_type': 2}, {'color_type': 3},                                                  # no table
    {'color_type': 3, 'table': 'table'},                                                   # no palette
    {'color_type': 0, 'palette': 'table'}, {'color_type': 2, 'table': 'table', 'palette': 'table'},      # a palette that is not type 3's
], ids=str)
def test_bad_arguments(buffers, kw):
    from xmem2_amd._lib import ptr
    kw = {k: ptr(buffers[1]) if v == 'table' else v for k, v in kw.items()}
    assert _call(buffers, **kw) == BAD_ARG


def test_misaligned_pointers(buffers):
    _, _, meta, out, ws = buffers
    assert _call(buffers, meta=ctypes.c_void_p(meta.data_ptr() + 2)) == BAD_ARG
    assert _call(buffers, out=ctypes.c_void_p(out.data_ptr() + 1)) == BAD_ARG
    assert _call(buffers, ws=ctypes.c_void_p(ws.data_ptr() + 4)) == WORKSPACE


@pytest.mark.parametrize('kw', [{'H': 0}, {'W': 0}, {'H': 16385}, {'W': 16385}, {'H': -2}, {'N': 0}, {'N': 65536}, {'N': -1}], ids=str)
def test_unsupported_sizes(buffers, kw):
    assert _call(buffers, **kw) == UNSUPPORTED


def test_a_short_workspace(buffers):
    from xmem2_amd import _lib_png
    need = _lib_png.load().xmem_png_workspace_bytes(N, H, W, 1)
    assert 0 < need <= buffers[4].numel()
    assert _call(buffers, nbytes=need - 1) == WORKSPACE and _call(buffers, nbytes=0) == WORKSPACE


def test_ops_raise(buffers):
    from xmem2_amd import ops
    planes, table, meta, out, ws = buffers
    rgb, grey = table.reshape(256, 3), table[:256]
    for call in (lambda: ops.png_encode(planes, 'L'), lambda: ops.png_encode(planes, 'rgb'), lambda: ops.png_encode(planes, 'palette', grey),
                 lambda: ops.png_encode(planes, 'grey', palette=rgb), lambda: ops.png_encode(planes, 'rgb', rgb, rgb),
                 lambda: ops.png_encode(planes, 'rgb', grey), lambda: ops.png_encode(planes, 'grey', rgb),
                 lambda: ops.png_encode(planes, 'palette', grey, grey), lambda: ops.png_encode(planes, 'grey', np.zeros(256, np.int32)),
                 lambda: ops.png_encode(planes, 'grey', capacity=0), lambda: ops.png_encode(planes, 'grey', capacity=True),
                 lambda: ops.png_encode(planes, 'grey', capacity=2 ** 31)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: ops.png_encode(planes.cpu(), 'grey'), lambda: ops.png_encode(planes.int(), 'grey'), lambda: ops.png_encode(planes[0, 0], 'grey'),
                 lambda: ops.png_encode(planes[:0], 'grey')):
        with pytest.raises(RuntimeError):
            call()
