"""GPU: `ops.signed_edt_sq`, `ops.mask_mattes` (two tables: a feather and a trimap) and `ops.grow_masks` (both signs) byte for byte
against the numpy definitions of xmem2_amd/matte.py (which test_matte_host.py holds to a brute force).

Sizes: one row, one column, widths either side of a wave (63, 64, 65), heights either side of the column pass's segments of 32 rows
(31, 32, 33; 63, 64, 65 - two segments of one thread row; 129 - a second workgroup along y) and more than one workgroup along x
(130 > 64).  R and r in {1, 2, 9, 127}: 127 is larger than both sides of every size here.  The host side of every size is computed
once and shared."""
import functools

import numpy as np
import pytest
import torch

import matte_refs as R
from xmem2_amd import matte, ops

pytestmark = pytest.mark.gpu

SIZES = ((1, 70), (70, 1), (37, 63), (37, 64), (37, 65), (97, 130), (31, 37), (32, 37), (33, 37), (63, 20), (64, 20), (65, 20), (129, 9))
RADII = (1, 2, 9, 127)
K = 3


@functools.lru_cache(maxsize=None)
def _stack(h, w):
    """(names, uint8 [N, h, w]): every content of matte_refs.contents at this size as one batch"""
    c = R.contents(h, w)
    return tuple(c), np.stack(list(c.values()))


@functools.lru_cache(maxsize=None)
def _want_d2(h, w, radius):
    _, maps = _stack(h, w)
    return np.stack([np.stack([matte.signed_d2_host(m, k, radius) for k in range(1, K + 1)]) for m in maps])


def _tables(radius):
    """a feather and a trimap that need the whole reach `radius` between them"""
    feather = matte.feather_table(feather=min(2 * radius - 1, 200), offset=0.5 if radius > 1 else 0, falloff='smooth', R=radius)[0]
    trimap = matte.trimap_table(band=radius - 0.5, R=radius)[0]
    return np.stack([feather, trimap])


def _lookups(tables, s2, radius):
    return np.stack([matte.lookup(table, s2, radius) for table in tables])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('h,w', SIZES)
def test_signed_distance_and_mattes(h, w):
    names, maps = _stack(h, w)
    dev = _dev(maps)
    for radius in RADII:
        want = _want_d2(h, w, radius)
        got = ops.signed_edt_sq(dev, K, radius)
        assert got.dtype == torch.int32 and tuple(got.shape) == (len(maps), K, h, w)
        got = got.cpu().numpy()
        for n, name in enumerate(names):
            assert (got[n] == want[n]).all(), (name, radius, int((got[n] != want[n]).sum()))
        tables = _tables(radius)
        planes = ops.mask_mattes(dev, K, _dev(tables), radius)
        assert planes.dtype == torch.uint8 and tuple(planes.shape) == (2, len(maps), K, h, w)
        planes = planes.cpu().numpy()
        for t in range(2):
            assert (planes[t] == matte.lookup(tables[t], want, radius)).all(), (t, radius)


@pytest.mark.parametrize('h,w', SIZES)
def test_grow_and_shrink(h, w):
    names, maps = _stack(h, w)
    dev = _dev(maps)
    for r in RADII + (1.5, 2.9):                                     # r2 = 2 and 8: radii that are no integers
        for sign in (1, -1):
            got = ops.grow_masks(dev, sign * r)
            assert got.dtype == torch.uint8 and got.shape == dev.shape and got.data_ptr() != dev.data_ptr()
            got = got.cpu().numpy()
            for n, name in enumerate(names):
                assert (got[n] == matte.grow_host(maps[n], sign * r)).all(), (name, sign * r)
    assert (dev.cpu().numpy() == maps).all()                         # the input is left alone


def test_the_border_is_no_edge():
    """a blob that touches all four borders: with a ring of zeros round the image (the click robot's `ops.edt_sq`) its border pixels
    would be at distance 1; here the distance runs to the background inside the image alone"""
    m = R.contents(37, 65)['touching']
    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    got = ops.signed_edt_sq(_dev(m), 1, 127).cpu().numpy()[0]
    ring = np.pad(m, 1)
    ringed = matte.signed_d2_host(ring, 1, 127)[1:-1, 1:-1]
    assert (got == matte.signed_d2_host(m, 1, 127)).all() and (got != ringed).any()
    assert got[0, 32] > 1 and ringed[0, 32] == 1


def test_label_255_alone():
    m = np.zeros((37, 65), np.uint8)
    m[5:20, 30:50] = 255
    m[36, 0] = 255
    got = ops.signed_edt_sq(_dev(m), 255, 9).cpu().numpy()
    assert got.shape == (255, 37, 65)
    assert (got[254] == matte.signed_d2_host(m, 255, 9)).all() and (got[:254] == -100).all()
    tables = _tables(9)
    planes = ops.mask_mattes(_dev(m), 255, _dev(tables), 9).cpu().numpy()
    assert planes.shape == (2, 255, 37, 65) and (planes[:, :254] == 0).all()
    assert (planes[:, 254] == _lookups(tables, got[254], 9)).all()
    for r in (9, -9):
        assert (ops.grow_masks(_dev(m), r).cpu().numpy() == matte.grow_host(m, r)).all()


def test_three_frames_2d_and_strided_inputs():
    c = R.contents(37, 65)
    frames = np.stack([c['blobs'], c['empty'], c['lattice']])        # three different frames, one of them empty
    dev = _dev(frames)
    tables = _tables(9)
    d2 = ops.signed_edt_sq(dev, K, 9).cpu().numpy()
    planes = ops.mask_mattes(dev, K, _dev(tables), 9).cpu().numpy()
    for n in range(3):
        want = np.stack([matte.signed_d2_host(frames[n], k, 9) for k in range(1, K + 1)])
        assert (d2[n] == want).all() and (planes[:, n] == _lookups(tables, want, 9)).all()
        for r in (2, -2):
            assert (ops.grow_masks(dev, r)[n].cpu().numpy() == matte.grow_host(frames[n], r)).all()
    # a 2-D input: the frame dimension is left out of the results
    one = ops.signed_edt_sq(dev[0], K, 9)
    assert tuple(one.shape) == (K, 37, 65) and (one.cpu().numpy() == d2[0]).all()
    two = ops.mask_mattes(dev[2], K, _dev(tables), 9)
    assert tuple(two.shape) == (2, K, 37, 65) and (two.cpu().numpy() == planes[:, 2]).all()
    assert tuple(ops.grow_masks(dev[0], 3).shape) == (37, 65)
    # a non-contiguous input: every other column of a wider batch, and a transposed view
    wide = _dev(np.repeat(frames, 2, axis=2))
    view = wide[:, :, ::2]
    assert not view.is_contiguous() and (ops.signed_edt_sq(view, K, 9).cpu().numpy() == d2).all()
    assert (ops.mask_mattes(view, K, _dev(tables), 9).cpu().numpy() == planes).all()
    assert (ops.grow_masks(view, 2).cpu().numpy() == ops.grow_masks(dev, 2).cpu().numpy()).all()
    turned = _dev(np.ascontiguousarray(frames[0].T)).T
    assert not turned.is_contiguous() and (ops.signed_edt_sq(turned, K, 9).cpu().numpy() == d2[0]).all()
    # out=: a tensor of the caller's; one that overlaps the input is refused
    out = torch.empty_like(dev)
    assert ops.grow_masks(dev, 2, out=out) is out and (out.cpu().numpy() == ops.grow_masks(dev, 2).cpu().numpy()).all()
    with pytest.raises(Exception):
        ops.grow_masks(dev, 2, out=dev)


def test_the_same_input_gives_the_same_bytes():
    _, maps = _stack(97, 130)
    dev = _dev(maps)
    tables = _dev(_tables(9))
    for call in (lambda: ops.signed_edt_sq(dev, K, 9), lambda: ops.mask_mattes(dev, K, tables, 9), lambda: ops.grow_masks(dev, 9),
                 lambda: ops.grow_masks(dev, -9)):
        first = call().clone()
        assert torch.equal(first, call())
