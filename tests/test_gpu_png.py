"""csrc/png.hip against `png.encode_host`: the device's files are the definition's, byte for byte, and a second call gives the same
bytes.  The shapes are the smallest that reach each way of going wrong."""
import numpy as np
import pytest
import torch

import png_refs as R
from xmem2_amd import png

pytestmark = pytest.mark.gpu

BYTE_MAP, COLOURS, PALETTE = R.tables()


def _args(mode, table=True):
    if mode == 'grey':
        return (BYTE_MAP if table else None), None
    return (COLOURS, None) if mode == 'rgb' else (BYTE_MAP, PALETTE)


def _same(planes, mode, table=True, capacity=None):
    """encode [N,H,W] twice on the device, compare with the host per frame; -> the files"""
    from xmem2_amd import ops
    tab, pal = _args(mode, table)
    dev = torch.from_numpy(np.ascontiguousarray(planes)).cuda()
    got = ops.png_encode(dev, mode, tab, pal, capacity=capacity)
    again = ops.png_encode(dev, mode, tab, pal, capacity=capacity)
    assert len(got) == len(planes) and got == again
    for n, plane in enumerate(planes):
        want = png.encode_host(plane, mode, tab, pal)
        assert len(got[n]) == len(want), f'frame {n}: {len(got[n])} bytes, the host has {len(want)}'
        diff = np.nonzero(np.frombuffer(got[n], np.uint8) != np.frombuffer(want, np.uint8))[0]
        assert diff.size == 0, f'frame {n}: {diff.size} bytes differ, the first at {diff[0]} of {len(want)}'
    return got


@pytest.mark.parametrize('mode', ['grey', 'rgb', 'palette'])
@pytest.mark.parametrize('hw', [(1, 1), (1, 3), (2, 4), (3, 2)], ids=str)
def test_tiny_planes(hw, mode):
    _same(R.noise((2,) + hw, 1), mode)
    _same(np.zeros((1,) + hw, np.uint8), mode)


@pytest.mark.parametrize('name, row', R.boundary_rows(), ids=[n for n, _ in R.boundary_rows()])
def test_run_and_match_boundaries(name, row):
    _same(row[None], 'grey', table=False)
    _same(np.concatenate([row, row, row[:, ::-1]])[None], 'grey', table=False)      # rows above: all zeros after the filter, then not


@pytest.mark.parametrize('W', [86, 87])
def test_rgb_row_byte_boundaries(W):
    _same(np.full((1, 2, W), 3, np.uint8), 'rgb')
    planes = np.full((1, 2, W), 3, np.uint8)
    planes[0, :, 0] = 4
    _same(planes, 'rgb')


def test_every_length_code():
    rows = R.every_run_length()
    _same(rows[None], 'grey', table=False)
    _same(rows[None, ::-1], 'grey')


@pytest.mark.parametrize('hw', [(96, 96), (33, 70)], ids=str)
def test_noise(hw):
    big = R.noise((1,) + hw, 2, low=144)                             # 9-bit literals; the sums of an unreduced Adler-32 overflow
    files = _same(big, 'grey', table=False)
    R.check_file(files[0], big[0], 'grey')
    _same(R.noise((1,) + hw, 3), 'grey')
    _same(R.noise((1,) + hw, 4), 'rgb')


@pytest.mark.parametrize('mode, W', [('grey', 4099), ('rgb', 1367)])
def test_rows_wider_than_one_pass_of_a_workgroup(mode, W):
    planes = np.zeros((1, 3, W), np.uint8)
    planes[0, 1, 5:W - 7] = 1
    planes[0, 2] = np.arange(W) // 300
    _same(planes, mode)
    _same(R.noise((1, 2, W), 6), mode)


def test_the_row_above():
    H, W = 6, 40
    stripes = np.zeros((H, W), np.uint8)
    stripes[1::2] = 255                                              # Up differences of 255 and 1: wrap-around
    same = np.tile(R.noise((1, W), 7), (H, 1))                       # identical rows: every row but the first is zeros
    first = np.zeros((H, W), np.uint8)
    first[0] = 250                                                   # row 0 against the zeros above it
    _same(np.stack([stripes, same, first]), 'grey', table=False)
    _same(np.stack([stripes, same, first]), 'rgb')


@pytest.mark.parametrize('mode', ['grey', 'rgb', 'palette'])
def test_a_batch_of_different_planes(mode):
    H, W = 17, 45
    planes = np.stack([np.zeros((H, W), np.uint8), R.noise((H, W), 8), np.full((H, W), 255, np.uint8),
                       (np.arange(H * W).reshape(H, W) // 50 % 3).astype(np.uint8), R.noise((H, W), 9, low=200)])
    files = _same(planes, mode)
    assert len({len(f) for f in files}) > 2
    for f, p in zip(files, planes):
        tab, pal = _args(mode)
        R.check_file(f, p, mode, tab, pal)


@pytest.mark.parametrize('table', [True, False])
def test_grey_with_and_without_a_table(table):
    _same(R.noise((2, 9, 31), 10), 'grey', table=table)


@pytest.mark.parametrize('mode', ['grey', 'rgb', 'palette'])
def test_one_real_size(mode):
    from xmem2_amd.synth import synthetic_masks
    m = synthetic_masks(1, 3, 480, 854)[0]
    plane = np.zeros((480, 854), np.uint8)
    for k in range(3):
        plane[m[k] > 0] = k + 1
    files = _same(plane[None], mode)
    print(f'{mode}: {len(files[0])} bytes for a 480 x 854 mask of {len(np.unique(plane))} labels')


def test_capacity_below_the_need():
    from xmem2_amd import _lib_png, ops
    from xmem2_amd._lib import check, ptr, stream_ptr
    H, W, N = 12, 50, 3
    planes = np.stack([np.zeros((H, W), np.uint8), R.noise((H, W), 11), np.ones((H, W), np.uint8)])
    want = [png.encode_host(p, 'grey') for p in planes]
    capacity = (len(want[1]) - 150) | 1                              # the noise frame does not fit, the others do; no multiple of 4
    assert max(len(want[0]), len(want[2])) <= capacity < len(want[1])
    dev = torch.from_numpy(planes).cuda()
    lib = _lib_png.load()
    meta = torch.full((N, _lib_png.META), -1, dtype=torch.int32, device='cuda')
    out = torch.full((N * capacity + 64,), 0xa5, dtype=torch.uint8, device='cuda')
    ws = torch.empty(lib.xmem_png_workspace_bytes(N, H, W, 1), dtype=torch.uint8, device='cuda')
    check(lib.xmem_png_encode(ptr(dev), N, H, W, 0, None, None, capacity, ptr(meta), ptr(out), ptr(ws), ws.numel(), stream_ptr()))
    meta, out = meta.cpu().numpy(), out.cpu().numpy()
    assert meta[:, 0].tolist() == [len(w) for w in want] and meta[:, 1].tolist() == [len(w) - 63 for w in want]
    assert (out[N * capacity:] == 0xa5).all(), 'bytes behind the last frame were written'
    for n in (0, 2):
        assert out[n * capacity:n * capacity + len(want[n])].tobytes() == want[n]
        assert not out[n * capacity + len(want[n]):(n + 1) * capacity].any()
    head = out[capacity:2 * capacity].tobytes()                      # what fits of the frame that does not: all but the IDAT checksum
    assert head == want[1][:capacity]
    # the last frame too small: nothing behind out[N][capacity] changes
    out = torch.full((capacity + 64,), 0xa5, dtype=torch.uint8, device='cuda')
    meta = torch.zeros(_lib_png.META, dtype=torch.int32, device='cuda')
    check(lib.xmem_png_encode(ptr(dev[1:2]), 1, H, W, 0, None, None, capacity, ptr(meta), ptr(out), ptr(ws), ws.numel(), stream_ptr()))
    assert int(meta[0]) == len(want[1]) and bool((out[capacity:] == 0xa5).all())
    before = ops.PNG_STATS['retries']
    assert ops.png_encode(dev, 'grey', capacity=capacity) == want
    assert ops.png_encode(dev, 'grey', capacity=1) == want
    assert ops.PNG_STATS['retries'] == before + 1 + 3


def test_record_without_waiting():
    from xmem2_amd import ops
    planes = R.noise((2, 5, 7), 12)
    capacity = png.worst_case_bytes(5, 7, 'rgb')
    rec = ops.png_encode(torch.from_numpy(planes).cuda(), 'rgb', COLOURS, capacity=capacity, wait=False)
    assert rec.is_cuda and rec.dtype == torch.uint8 and rec.numel() == png.record_bytes(2, capacity)
    meta, data = png.split_record(rec.cpu().numpy(), 2, capacity)
    for n in range(2):
        assert data[n, :meta[n, 0]].tobytes() == png.encode_host(planes[n], 'rgb', COLOURS)
