"""`png.encode_host`, the definition of the PNG files built on the device, and what stands round it: the colour table, the sizes, the
record, the option, the seventh header and its place in the build.  No GPU."""
import ctypes
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_refs as R
from xmem2_amd import png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'xmem_hip_png.h')
CHAIR = os.path.join(ROOT, 'tests', 'golden', 'chair', 'Annotations', 'frame_000000.png')
BYTE_MAP, COLOURS, PALETTE = R.tables()
MODES = ('grey', 'rgb', 'palette')


def _args(mode):
    return {'grey': (BYTE_MAP, None), 'rgb': (COLOURS, None), 'palette': (BYTE_MAP, PALETTE)}[mode]


def _planes():
    soft = np.clip(300 - np.hypot(*np.mgrid[-40:40, -60:60]) * 8, 0, 255).astype(np.uint8) // 16 * 16      # a disc with a soft edge
    out = [('1x1', np.array([[7]], np.uint8)), ('1x3', R.noise((1, 3), 1)), ('3x2', R.noise((3, 2), 2)), ('zeros', np.zeros((9, 300), np.uint8)),
           ('noise', R.noise((33, 70), 3)), ('high noise', R.noise((96, 96), 4, low=144)), ('soft disc', soft), ('runs', R.every_run_length())]
    return out + R.boundary_rows()[::5]


@pytest.mark.parametrize('mode', MODES)
def test_files_open_and_hold_the_plane(mode):
    table, palette = _args(mode)
    for name, plane in _planes():
        data = png.encode_host(plane, mode, table, palette)
        D = R.check_file(data, plane, mode, table, palette)
        assert len(data) == png.file_bytes(D, mode) == 57 + 6 + D + (780 if mode == 'palette' else 0), name
        assert len(data) <= png.worst_case_bytes(*plane.shape, mode), name
        assert png.encode_host(plane, mode, table, palette) == data


def test_grey_without_a_table_and_the_arguments():
    plane = R.noise((5, 9), 5)
    R.check_file(png.encode_host(plane, 'grey'), plane, 'grey')
    for bad in (lambda: png.encode_host(plane, 'rgb'), lambda: png.encode_host(plane, 'palette', BYTE_MAP), lambda: png.encode_host(plane, 'grey', None, PALETTE),
                lambda: png.encode_host(plane, 'rgb', BYTE_MAP), lambda: png.encode_host(plane, 'grey', COLOURS), lambda: png.encode_host(plane, 'L'),
                lambda: png.encode_host(plane.astype(np.int32), 'grey'), lambda: png.encode_host(plane[0], 'grey'),
                lambda: png.encode_host(np.zeros((0, 4), np.uint8), 'grey')):
        with pytest.raises(ValueError):
            bad()


def test_the_length_formula_at_its_worst():
    """bytes of 144 and more whose Up differences are 144 and more too and never repeat: every data byte is a 9-bit literal"""
    H, W = 8, 33
    d = np.where((np.arange(W)[None] + np.arange(H)[:, None]) % 2 == 0, 255, 254)
    plane = (np.cumsum(d, axis=0) % 256).astype(np.uint8)
    filt = np.frombuffer(R.filtered_up(plane), np.uint8).reshape(H, W + 1)[:, 1:]
    assert plane.min() >= 144 and filt.min() >= 144 and (filt[:, 1:] != filt[:, :-1]).all()
    for mode, table in (('grey', None), ('rgb', np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1))):
        L = W * png.MODES[mode][1]
        data = png.encode_host(plane, mode, table)
        if mode == 'grey':                                           # rgb repeats every byte three times: two literals and a literal
            D = (3 + H * (8 + 9 * L) + 7 + 7) // 8
            assert len(data) == 63 + D
        assert len(data) <= png.worst_case_bytes(H, W, mode) <= len(data) + H // 8 + 1
        R.check_file(data, plane, mode, table)
    noise = R.noise((33, 70), 6)
    assert len(png.encode_host(noise, 'grey')) <= png.worst_case_bytes(33, 70, 'grey') == 63 + (3 + 9 * 33 * 71 + 14) // 8


def test_the_token_rule_by_hand():
    """a row of 1 + 258 + 2 equal bytes: a literal, one match of 258, two literals; with one byte more the tail is a match of 3"""
    def block(n):
        return dict(R.chunks(png.encode_host(np.full((1, n), 5, np.uint8), 'grey')))[b'IDAT'][2:-4]
    lit2, lit5 = '00110010', '00110101'                              # 0x30 + value, most significant bit first
    m258 = '11000101' + '00000'                                      # code 285, distance code 0
    m3 = '0000001' + '00000'                                         # code 257
    for n, tail in ((261, lit5 + lit5), (262, m3)):
        want = '110' + lit2 + lit5 + m258 + tail + '0000000'
        bits = ''.join(format(b, '08b')[::-1] for b in block(n))
        assert bits[:len(want)] == want and set(bits[len(want):]) <= {'0'} and len(bits) - len(want) < 8, n


def _reader_and_mapper(path):
    from xmem2_amd.mask_mapper import MaskMapper
    from xmem2_amd.run_on_video import VideoReader
    d = os.path.dirname(path)
    reader = VideoReader('chair', d, d)
    mapper = MaskMapper()
    return reader, mapper


def test_the_colour_table_is_the_writers_colours():
    reader, mapper = _reader_and_mapper(CHAIR)
    ann = np.array(Image.open(CHAIR).convert('P'), dtype=np.uint8)
    mapper.convert_mask(ann, exhaustive=True)
    dense = np.asarray(mapper.remap_index_mask(np.arange(256, dtype=np.uint8)))
    table = png.color_table(reader, png.label_map(mapper))
    assert table.shape == (256, 3) and table.dtype == np.uint8
    k = len(mapper.labels)
    ids = (np.arange(ann.size).reshape(ann.shape) // 97 % (k + 1)).astype(np.uint8)          # dense ids, as a frame loop holds them
    full = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for m in (ids, full):
        want = np.array(reader.map_the_colors_back(Image.fromarray(mapper.remap_index_mask(m))))
        np.testing.assert_array_equal(table[m], want)
        np.testing.assert_array_equal(np.array(Image.open(io.BytesIO(png.encode_host(m, 'rgb', table)))), want)
    assert dense.dtype == np.uint8
    # the index PNG: the annotation's palette, pixel values the labels
    im = Image.open(io.BytesIO(png.encode_host(ids, 'palette', png.label_map(mapper), png.reader_palette(reader))))
    np.testing.assert_array_equal(np.array(im), mapper.remap_index_mask(ids))
    assert im.getpalette()[:768] == (reader.reference_mask.getpalette() + [0] * 768)[:768]
    np.testing.assert_array_equal(np.array(im.convert('RGB')), np.array(reader.map_the_colors_back(Image.fromarray(mapper.remap_index_mask(ids)))))


def test_sizes_record_and_option():
    for mode in MODES:
        C = png.MODES[mode][1]
        for H, W in ((1, 1), (480, 854), (1080, 1920)):
            worst = png.worst_case_bytes(H, W, mode)
            assert worst == 63 + (3 + 9 * H * (1 + W * C) + 14) // 8 + (780 if mode == 'palette' else 0)
            assert 64 <= png.default_capacity(H, W, mode) <= worst
    assert png.default_capacity(480, 854, 'rgb') < 480 * 854                # less travels than the mask itself
    N, cap = 3, 10
    buf = np.arange(png.record_bytes(N, cap), dtype=np.uint8)
    assert png.record_bytes(N, cap) == 4 * png.META * N + 32
    meta, data = png.split_record(buf, N, cap)
    assert meta.shape == (N, png.META) and meta.dtype == np.int32 and data.shape == (N, cap)
    assert data[1, 0] == (4 * png.META * N + cap) % 256 and np.shares_memory(data, buf)
    with pytest.raises(ValueError):
        png.split_record(buf[:-1], N, cap)
    assert png.parse_option(None) is None and png.parse_option(False) is None
    assert png.parse_option(True) == {'mode': 'rgb'} == png.parse_option({}) == png.parse_option('rgb')
    assert png.parse_option({'mode': 'palette'}) == {'mode': 'palette'}
    for bad in ('grey', {'mode': 'L'}, {'mod': 'rgb'}, 3):
        with pytest.raises(ValueError):
            png.parse_option(bad)


# ---- the seventh header, its binding, the build ---------------------------------------------------------------------------------------

def test_seventh_header_parses_and_the_library_exports_it():
    from xmem2_amd import _header, _lib, _lib_masks, _lib_matte, _lib_png, _lib_polygons, _lib_raster, _lib_temporal, build
    text = open(HEADER).read()
    constants, structs, sigs = _header.parse(text)
    assert structs == {} and constants == {'XMEM_PNG_META': png.META, 'XMEM_PNG_GREY': 0, 'XMEM_PNG_RGB': 2, 'XMEM_PNG_PALETTE': 3,
                                           'XMEM_PNG_MAX_CAPACITY': 2 ** 31 - 1}
    assert _lib_png.COLOR_TYPES == {m: png.MODES[m][0] for m in MODES} and _lib_png.META == png.META
    declared = sorted(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S))))
    assert sorted(sigs) == declared == sorted(_lib_png.EXPORTED_SYMBOLS) == ['xmem_png_encode', 'xmem_png_workspace_bytes']
    i, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert sigs['xmem_png_workspace_bytes'] == (z, [i] * 4)
    assert sigs['xmem_png_encode'] == (i, [p] + [i] * 4 + [p, p, i, p, p, p, z, p])
    lib = _lib_png.load()
    assert lib is _lib.load()
    others = (set(_lib.EXPORTED_SYMBOLS) | set(_lib_masks.EXPORTED_SYMBOLS) | set(_lib_polygons.EXPORTED_SYMBOLS)
              | set(_lib_raster.EXPORTED_SYMBOLS) | set(_lib_matte.EXPORTED_SYMBOLS) | set(_lib_temporal.EXPORTED_SYMBOLS))
    assert not set(sigs) & others and len(_lib.EXPORTED_SYMBOLS) == 103 and _lib.ABI_VERSION == 5
    assert 'png.hip' in build.SOURCES and [os.path.basename(f) for f in build.PNG_HEADERS] == ['xmem_hip_png.h']


def test_build_tracks_the_seventh_header(tmp_path, monkeypatch):
    from xmem2_amd import build
    assert os.path.samefile(build.PNG_HEADERS[0], HEADER)
    digest = build.source_digest()
    copy = tmp_path / 'xmem_hip_png.h'
    copy.write_bytes(open(HEADER, 'rb').read())
    monkeypatch.setattr(build, 'PNG_HEADERS', [str(copy)])
    assert build.source_digest() == digest
    assert build.needs_build()                                       # the copy is newer than the library
    copy.write_bytes(copy.read_bytes() + b'\n/* changed */\n')
    assert build.source_digest() != digest


def test_the_entry_point_refuses_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib_png
    lib = _lib_png.load()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 30)           # never dereferenced: every call below is refused on the host

    def encode(planes=p, N=1, H=8, W=8, ct=0, table=None, palette=None, capacity=64, meta=p, out=q, ws=p, nbytes=1 << 20):
        return lib.xmem_png_encode(planes, N, H, W, ct, table, palette, capacity, meta, out, ws, nbytes, None)

    for kw in ({'planes': None}, {'meta': None}, {'out': None}, {'ws': None}, {'meta': ctypes.c_void_p(4098)}, {'out': ctypes.c_void_p(4097)},
               {'capacity': 0}, {'capacity': -5}, {'ct': 1}, {'ct': 4}, {'ct': -1}, {'ct': 2}, {'ct': 3}, {'ct': 3, 'table': p},
               {'ct': 3, 'palette': p}, {'ct': 0, 'palette': p}, {'ct': 2, 'table': p, 'palette': p}):
        assert encode(**kw) == -1, kw
    for kw in ({'H': 0}, {'W': 0}, {'H': 16385}, {'W': 16385}, {'N': 0}, {'N': 65536}, {'H': -1}):
        assert encode(**kw) == -2, kw
    need = lib.xmem_png_workspace_bytes(1, 8, 8, 1)
    assert need > 0 and need % 8 == 0 and lib.xmem_png_workspace_bytes(2, 8, 8, 3) > need
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 16385, 1), (65536, 8, 8, 1), (1, 8, 8, 2)):
        assert lib.xmem_png_workspace_bytes(*bad) == 0
    codes = {encode(nbytes=need - 1), encode(ws=ctypes.c_void_p(4100))}
    assert len(codes) == 1 and codes.pop() not in (0, -1, -2)        # XMEM_ERR_WORKSPACE


def test_without_the_key_nothing_is_imported():
    import subprocess
    import sys
    code = ('import sys; import xmem2_amd.run_on_video, xmem2_amd.session, xmem2_amd.rle, xmem2_amd.matte; '
            'assert not {"xmem2_amd.png", "xmem2_amd._lib_png"} & set(sys.modules), "imported without the option"')
    subprocess.run([sys.executable, '-c', code], check=True, cwd=ROOT)
