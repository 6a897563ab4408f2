"""Host side of the device frame resize (xmem2_amd/pil_resize.py): the restated tap computation and the integer two-pass emulation
against the installed Pillow, byte for byte; the new C symbols; the reader's `resize_on_device` switch without a device."""
import os

import numpy as np
import pytest
import torch


# (source (h, w), target (th, tw)): 1080p / 720p / 540p to the 480p working size, odd down- and upscales, one axis only, an upscale
# by 14, a single source row, 201 taps
CASES = [((1080, 1920), (480, 853)), ((720, 1280), (480, 853)), ((540, 960), (480, 853)), ((37, 53), (16, 22)), ((16, 22), (37, 53)),
         ((9, 300), (480, 16)), ((481, 641), (480, 639)), ((5, 7), (5, 3)), ((33, 47), (480, 683)), ((1, 9), (4, 3)),
         ((100, 100), (1, 1))]


def _images(hw, seed):
    """seeded noise and a seeded 0/255 image (every sum of taps hits the clamp ends and the rounding of full-scale steps)"""
    g = np.random.default_rng(seed)
    return {'noise': g.integers(0, 256, size=hw + (3,), dtype=np.uint8),
            'binary': (g.integers(0, 2, size=hw + (3,), dtype=np.uint8) * 255).astype(np.uint8)}


def _pillow(a, th, tw):
    from PIL import Image
    return np.array(Image.fromarray(a).resize((tw, th), Image.BILINEAR), dtype=np.uint8)


@pytest.mark.parametrize('src,dst', CASES, ids=[f'{s[0]}x{s[1]}_to_{d[0]}x{d[1]}' for s, d in CASES])
def test_host_emulation_equals_pillow(src, dst):
    from xmem2_amd.pil_resize import resize_u8_host
    for kind, a in _images(src, seed=src[0] * 131 + dst[1]).items():
        want = _pillow(a, *dst)
        got = resize_u8_host(a, *dst)
        assert got.dtype == np.uint8 and got.shape == dst + (3,) and got.flags.c_contiguous
        assert int((got != want).sum()) == 0, f'{kind}: {int((got != want).sum())} bytes differ from Pillow'
        flipped = resize_u8_host(a, *dst, flip=True)
        assert flipped.flags.c_contiguous and np.array_equal(flipped, np.ascontiguousarray(want[:, ::-1])), f'{kind}: mirrored result'


@pytest.mark.parametrize('n_in,n_out', [(1920, 853), (1080, 480), (2160, 480), (22, 53), (100, 1), (1, 4), (641, 639), (7, 3), (16384, 480)])
def test_taps_properties(n_in, n_out):
    from xmem2_amd.pil_resize import PRECISION_BITS, taps
    bounds, coeffs = taps(n_in, n_out)
    ksize = 2 * int(np.ceil(max(n_in / n_out, 1.0))) + 1
    assert bounds.dtype == np.int32 and coeffs.dtype == np.int32
    assert bounds.shape == (n_out, 2) and coeffs.shape == (n_out, ksize)
    first, count = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
    assert (first >= 0).all() and (count >= 1).all() and (count <= ksize).all() and (first + count <= n_in).all()
    assert (coeffs >= 0).all(), 'the triangle filter has no negative lobe'
    sums = coeffs.astype(np.int64).sum(1)
    assert (np.abs(sums - (1 << PRECISION_BITS)) <= ksize).all(), 'one rounding per tap'
    for xx in range(n_out):
        assert not coeffs[xx, count[xx]:].any(), 'unused taps are 0'
    assert 255 * int(sums.max()) + (1 << (PRECISION_BITS - 1)) < 2 ** 31, 'the int32 accumulator cannot overflow'
    assert taps(n_in, n_out)[0] is bounds, 'cached per geometry'


def test_taps_tap_counts_and_identity():
    from xmem2_amd.pil_resize import PRECISION_BITS, taps
    assert taps(22, 53)[1].shape[1] == 3 and taps(2160, 480)[1].shape[1] == 11 and taps(100, 1)[1].shape[1] == 201
    for n in (1, 5, 480):
        bounds, coeffs = taps(n, n)
        assert np.array_equal(bounds[:, 0] + (coeffs.argmax(1)), np.arange(n)), 'the one non-zero tap sits on the sample itself'
        assert (coeffs.max(1) == 1 << PRECISION_BITS).all() and (coeffs.sum(1) == 1 << PRECISION_BITS).all()
    with pytest.raises(ValueError):
        taps(0, 4)


def test_new_symbols_and_abi_version():
    from xmem2_amd import _lib, build
    lib = _lib.load()
    for name in ('xmem_resize_u8_bilinear_aa', 'xmem_resize_u8_workspace_bytes'):
        assert hasattr(lib, name)
    assert 'resize_u8.hip' in build.SOURCES
    assert lib.xmem_version() == _lib.ABI_VERSION == 5
    assert lib.xmem_resize_u8_workspace_bytes(1080, 1920, 480, 853) == 1080 * 853 * 3
    assert lib.xmem_resize_u8_workspace_bytes(480, 1920, 480, 853) == 0 and lib.xmem_resize_u8_workspace_bytes(96, 128, 96, 128) == 0
    assert lib.xmem_resize_u8_workspace_bytes(16385, 4, 4, 4) == 0
    # argument checks run before anything touches a device
    args = (1, 1, 3, 1, 1, 8, 1)                      # tables and workspace: non-null dummies, never dereferenced on these paths
    assert lib.xmem_resize_u8_bilinear_aa(None, 4, 4, 1, 2, 2, 0, *args, 8, None) == -1
    assert lib.xmem_resize_u8_bilinear_aa(1, 16385, 4, 1, 2, 2, 0, *args, 8, None) == -2
    assert lib.xmem_resize_u8_bilinear_aa(1, 4, 4, 1, 2, 16385, 0, *args, 8, None) == -2
    assert lib.xmem_resize_u8_bilinear_aa(1, 4, 4, 1, 2, 2, 0, None, None, 0, 1, 1, 5, 1, 64, None) == -1, 'a changing axis needs its taps'
    assert lib.xmem_resize_u8_bilinear_aa(1, 4, 4, 1, 2, 2, 0, *args, 4 * 2 * 3 - 1, None) == -3


def _write_frames(tmp_path, hw, n=2):
    from PIL import Image
    imgs, msks = tmp_path / 'JPEGImages', tmp_path / 'Annotations'
    imgs.mkdir(); msks.mkdir()
    g = np.random.default_rng(5)
    for i in range(n):
        Image.fromarray(g.integers(0, 256, size=hw + (3,), dtype=np.uint8)).save(imgs / f'f{i:03d}.png')
    idx = np.zeros(hw, np.uint8); idx[10:60, 20:90] = 1
    im = Image.fromarray(idx, mode='P'); im.putpalette([0, 0, 0, 200, 0, 0] + [0] * (256 * 3 - 6)); im.save(msks / 'f000.png')
    return str(imgs), str(msks)


def test_reader_hands_over_the_source_frame_when_asked(tmp_path):
    from PIL import Image
    from xmem2_amd.pil_resize import resize_u8_host
    from xmem2_amd.run_on_video import VideoReader
    imgs, msks = _write_frames(tmp_path, (150, 200))
    decoded = np.array(Image.open(os.path.join(imgs, 'f000.png')).convert('RGB'), dtype=np.uint8)
    off = VideoReader('', imgs, msks, size=96, use_all_masks=True)
    on = VideoReader('', imgs, msks, size=96, use_all_masks=True, resize_on_device=True)
    a, b = off[0], on[0]
    # off: what the sample is today
    assert a.src_u8 is None and a.target_hw is None
    assert a.rgb_u8.dtype == torch.uint8 and tuple(a.rgb_u8.shape) == (96, 128, 3)
    assert np.array_equal(a.rgb_u8.numpy(), _pillow(decoded, 96, 128))
    # on: the decoded frame at its own size and the size the device resizes it to; the rest of the sample is unchanged
    assert b.rgb_u8 is None and b.target_hw == (96, 128)
    assert b.src_u8.dtype == torch.uint8 and tuple(b.src_u8.shape) == (150, 200, 3) and np.array_equal(b.src_u8.numpy(), decoded)
    assert (b.frame, b.shape, b.need_resize, b.save) == (a.frame, a.shape, a.need_resize, a.save) == ('f000.png', (150, 200), True, True)
    assert np.array_equal(a.mask, b.mask) and a.mask is not None and on[1].mask is None
    assert np.array_equal(resize_u8_host(b.src_u8.numpy(), *b.target_hw), a.rgb_u8.numpy())
    assert torch.equal(a.rgb, b.rgb), 'the float view of the sample is the same frame'
    assert tuple(on.resize_mask(torch.zeros(1, 150, 200)).shape) == tuple(off.resize_mask(torch.zeros(1, 150, 200)).shape) == (1, 96, 128)
    # native size: the target is the source size
    native = VideoReader('', imgs, msks, size=-1, resize_on_device=True)[0]
    assert native.target_hw == (150, 200) and native.need_resize is False
    # portrait frames: the shorter side is the width
    assert VideoReader('', imgs, msks, size=96, resize_on_device=True)._target_hw(200, 150) == (128, 96)
