"""Mattes, trimaps, grow and shrink without a GPU: the numpy definitions (xmem2_amd/matte.py) against a brute force over all pairs of
pixels, the properties of the tables, the parser of config['mattes'], the fifth header with its binding and the build lists, and the
argument checks of the C entry points (which answer before any GPU work)."""
import ctypes
import os
import re

import numpy as np
import pytest

import matte_refs as R
from conftest import ROOT
from xmem2_amd import matte

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # xmem_status (include/xmem_hip.h)
HEADER = os.path.join(ROOT, 'include', 'xmem_hip_matte.h')


def _maps():
    rng = np.random.default_rng(5)
    maps = [np.full((7, 9), 2, np.uint8), np.zeros((6, 5), np.uint8), np.full((1, 1), 1, np.uint8)]       # whole frame, empty, one pixel
    for h, w in ((24, 24), (1, 23), (23, 1), (5, 5), (17, 24), (24, 11)):
        maps.append(R.blob(h, w, rng))
        maps.append((rng.random((h, w)) < 0.15).astype(np.uint8) * rng.integers(1, 4, (h, w)).astype(np.uint8))
    maps += [m for name, m in R.contents(13, 18).items()]
    return maps


MAPS = _maps()


# ---- the definition -------------------------------------------------------------------------------------------------------------------

def test_signed_d2_host_is_the_brute_force():
    for m in MAPS:
        for radius in (1, 3, 5, 127):                                # 127: larger than every map here
            for k in (1, 2, 3):
                got = matte.signed_d2_host(m, k, radius)
                assert got.dtype == np.int32 and got.shape == m.shape
                assert (got == R.signed_d2_brute(m, k, radius)).all(), (m.shape, radius, k)


def test_signed_d2_host_special_cases():
    whole, empty = np.full((7, 9), 2, np.uint8), np.zeros((6, 5), np.uint8)
    assert (matte.signed_d2_host(whole, 2, 3) == 16).all()           # a minimum over no pixel is cap2: no edge at the border
    assert (matte.signed_d2_host(whole, 1, 3) == -16).all()
    assert (matte.signed_d2_host(empty, 1, 127) == -128 * 128).all()
    m = np.zeros((9, 9), np.uint8)
    m[:5, :5] = 1                                                    # touches two borders: the distance is to the background alone
    assert matte.signed_d2_host(m, 1, 10)[0, 0] == 25 and matte.signed_d2_host(m, 1, 2)[0, 0] == 9
    assert matte.signed_d2_host(m, 1, 10)[8, 8] == -(16 + 16) and matte.signed_d2_host(m, 1, 10)[4, 5] == -1
    for bad in ((m, 0, 3), (m, 256, 3), (m, 1, 0), (m, 1, 128), (m, 1, 2.0), (m.astype(np.int32), 1, 3), (m[0], 1, 3)):
        with pytest.raises(ValueError):
            matte.signed_d2_host(*bad)


def test_grow_host_is_the_brute_force():
    for m in MAPS:
        for r in (1, 1.5, 2, 3, 5, 127, -1, -1.5, -2, -3, -127):
            got = matte.grow_host(m, r)
            assert got.dtype == np.uint8 and (got == R.grow_brute(m, r)).all(), (m.shape, r)
    m = MAPS[3]
    assert (matte.grow_host(m, 0) == m).all() and (matte.grow_host(m, 0.9) == m).all()
    for bad in (128, -127.5, float('nan'), True, 'a'):
        with pytest.raises(ValueError):
            matte.grow_host(m, bad)


def test_grow_host_rules():
    m = np.zeros((5, 9), np.uint8)
    m[2, 1], m[2, 7] = 3, 1
    g = matte.grow_host(m, 4)
    assert g[2, 4] == 1 and g[2, 3] == 3 and g[2, 5] == 1            # the tie at equal distance goes to the smaller label
    assert g[2, 1] == 3 and g[2, 7] == 1                             # objects never eat one another
    two = np.array([[1, 1, 2, 2, 0, 0]], np.uint8)
    assert matte.grow_host(two, 1).tolist() == [[1, 1, 2, 2, 2, 0]]
    assert matte.grow_host(two, -1).tolist() == [[1, 0, 0, 0, 0, 0]]          # the other label is an edge, the image border is none


# ---- tables ---------------------------------------------------------------------------------------------------------------------------

WIDTHS = (0, 0.5, 1, 2, 3, 5, 8, 32, 100)
OFFSETS = (0, 0.5, -0.5, 1, -2, 3.25, -10)


def test_feather_tables():
    for falloff in matte.FALLOFFS:
        for w in WIDTHS:
            for o in OFFSETS:
                table, radius = matte.feather_table(feather=w, offset=o, falloff=falloff)
                assert radius == max(1, int(np.ceil(w / 2 + abs(o)))) and table.dtype == np.uint8
                assert table.shape == (2 * (radius + 1) ** 2 + 1,)
                assert (np.diff(table.astype(int)) >= 0).all(), (w, o)                   # monotone
                assert table[0] == 0 and table[-1] == 255                                # saturated at the two caps
                cap2 = (radius + 1) ** 2
                if o == 0:                                                               # symmetric about 127.5 (s2 = 0 is no distance)
                    assert (np.delete(table.astype(int) + table[::-1].astype(int), cap2) == 255).all(), w
                wider, r2 = matte.feather_table(feather=w, offset=o, falloff=falloff, R=radius + 3)
                big = (r2 + 1) ** 2
                assert r2 == radius + 3 and (wider[big - cap2 + 1:big + cap2] == table[1:-1]).all()
                assert (wider[:big - cap2 + 1] == 0).all() and (wider[big + cap2:] == 255).all()       # the cap never shows
    step, radius = matte.feather_table(feather=0, offset=0)
    assert radius == 1 and step.tolist() == [0] * 5 + [255] * 4                          # w = 0 is a step at the edge
    step, radius = matte.feather_table(feather=0, offset=1)                              # moved out by one pixel: s > -1, d > 1.5
    assert radius == 1 and step.tolist() == [0, 0] + [255] * 7
    linear, _ = matte.feather_table(feather=2, offset=0)
    assert linear[4 + 1] == 191 and linear[4 - 1] == 64                   # s = +-1/2: a = 3/4 and 1/4
    for bad in ({'feather': -1}, {'feather': 255}, {'feather': 2, 'offset': 127}, {'falloff': 'cubic'}, {'feather': float('inf')},
                {'feather': 4, 'R': 1}, {'feather': 2, 'R': 128}, {'feather': True}):
        with pytest.raises(ValueError):
            matte.feather_table(**bad)


def test_trimap_tables():
    for t in (0, 0.5, 1, 2, 2.5, 10, 127):
        table, radius = matte.trimap_table(band=t)
        assert radius == max(1, int(np.ceil(t))) and table.shape == (2 * (radius + 1) ** 2 + 1,)
        s2 = np.arange(len(table)) - (radius + 1) ** 2
        assert (table[s2 > t * t] == 255).all() and (table[s2 < -t * t] == 0).all() and (table[np.abs(s2) <= t * t] == 128).all()
        assert table[0] == 0 and table[-1] == 255 and set(np.unique(table)) <= {0, 128, 255}
    for bad in (-1, 128, float('nan'), None):
        with pytest.raises(ValueError):
            matte.trimap_table(band=bad)


def test_parse_mattes():
    assert matte.parse_mattes(None) is None
    assert matte.parse_mattes(True) == {'feather': 2, 'offset': 0, 'falloff': 'linear', 'trimap': None} == matte.parse_mattes({})
    got = matte.parse_mattes({'feather': 3, 'trimap': 2, 'offset': -1, 'falloff': 'smooth'})
    assert got == {'feather': 3.0, 'offset': -1.0, 'falloff': 'smooth', 'trimap': 2.0}
    assert matte.parse_mattes({'feather': None, 'trimap': 4}) == {'feather': None, 'offset': 0, 'falloff': 'linear', 'trimap': 4.0}
    for bad in ({'feather': None}, {'blur': 1}, {'feather': -1}, {'feather': '2'}, {'trimap': -1}, {'trimap': 200}, {'feather': 300},
                {'offset': 127, 'feather': 2}, {'falloff': 'cubic'}, {'feather': True}, {'offset': None}, False, 3, 'on', [2]):
        with pytest.raises(ValueError):
            matte.parse_mattes(bad)
    names, tables, radius = matte.tables_of(matte.parse_mattes({'feather': 3, 'trimap': 4}))
    assert names == ['mattes', 'trimaps'] and radius == 4 and tables.shape == (2, 51) and tables.dtype == np.uint8
    assert (tables[0] == matte.feather_table(3, R=4)[0]).all() and (tables[1] == matte.trimap_table(4)[0]).all()
    names, tables, radius = matte.tables_of(matte.parse_mattes({'feather': None, 'trimap': 1}))
    assert names == ['trimaps'] and radius == 1 and tables.shape == (1, 9)
    m = R.contents(9, 12)['touching']
    planes = matte.planes_host(m, 2, matte.parse_mattes({'feather': 3, 'trimap': 2}))
    assert planes['mattes'].shape == (2, 9, 12) and (planes['mattes'][1] == 0).all() and (planes['trimaps'][1] == 0).all()
    assert planes['mattes'][0][m == 1].min() >= 128 and planes['mattes'][0][m != 1].max() <= 127


# ---- the fifth header, its binding, the build -------------------------------------------------------------------------------------------

def test_fifth_header_parses_and_the_library_exports_it():
    from xmem2_amd import _header, _lib, _lib_masks, _lib_matte, _lib_polygons, _lib_raster, build
    text = open(HEADER).read()
    constants, structs, sigs = _header.parse(text)
    assert structs == {} and constants == {'XMEM_MATTE_MAX_R': 127, 'XMEM_MATTE_MAX_TABLES': 4, 'XMEM_MATTE_MAX_LABELS': 255}
    assert (_lib_matte.MAX_R, _lib_matte.MAX_TABLES, _lib_matte.MAX_LABELS) == (127, 4, 255) and matte.MAX_R == 127
    declared = sorted(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S))))
    assert sorted(sigs) == declared == sorted(_lib_matte.EXPORTED_SYMBOLS) == [
        'xmem_mask_grow', 'xmem_mask_grow_workspace_bytes', 'xmem_mask_matte', 'xmem_mask_matte_workspace_bytes', 'xmem_signed_edt',
        'xmem_signed_edt_workspace_bytes']
    i, p, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert sigs['xmem_signed_edt'] == (i, [p] + [i] * 5 + [p, p, z, p])
    assert sigs['xmem_mask_matte'] == (i, [p] + [i] * 5 + [p, i, p, p, z, p])
    assert sigs['xmem_mask_grow'] == (i, [p] + [i] * 5 + [p, p, z, p])
    assert sigs['xmem_signed_edt_workspace_bytes'] == sigs['xmem_mask_matte_workspace_bytes'] == (z, [i] * 4)
    assert sigs['xmem_mask_grow_workspace_bytes'] == (z, [i] * 3)
    lib = _lib_matte.load()
    assert lib is _lib.load()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib_masks.EXPORTED_SYMBOLS) | set(_lib_polygons.EXPORTED_SYMBOLS) | set(_lib_raster.EXPORTED_SYMBOLS)
    assert not set(sigs) & others and len(others) == 103 + 4 + 2 + 2 and _lib.ABI_VERSION == 5
    assert 'matte.hip' in build.SOURCES and [os.path.basename(f) for f in build.MATTE_HEADERS] == ['xmem_hip_matte.h']
    assert build.PUBLIC_HEADERS == ['xmem_hip.h', 'xmem_hip_masks.h', 'xmem_hip_polygons.h']
    assert [os.path.basename(f) for f in build.LATER_HEADERS] == ['xmem_hip_raster.h']


def test_build_tracks_the_fifth_header(tmp_path, monkeypatch):
    from xmem2_amd import build
    assert os.path.samefile(build.MATTE_HEADERS[0], HEADER)
    digest = build.source_digest()
    copy = tmp_path / 'xmem_hip_matte.h'
    copy.write_bytes(open(HEADER, 'rb').read())
    monkeypatch.setattr(build, 'MATTE_HEADERS', [str(copy)])
    assert build.source_digest() == digest
    assert build.needs_build()                                       # the copy is newer than the library
    copy.write_bytes(copy.read_bytes() + b'\n/* changed */\n')
    assert build.source_digest() != digest


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib_matte
    lib = _lib_matte.load()
    p = ctypes.c_void_p(4096)                                        # never dereferenced: every call below is refused on the host
    q = ctypes.c_void_p(1 << 30)
    big = 1 << 60

    def edt(masks=p, N=1, H=8, W=8, K=2, R=3, out=q, ws=p, nbytes=big):
        return lib.xmem_signed_edt(masks, N, H, W, K, R, out, ws, nbytes, None)

    def mat(masks=p, N=1, H=8, W=8, K=2, R=3, tables=p, T=2, out=q, ws=p, nbytes=big):
        return lib.xmem_mask_matte(masks, N, H, W, K, R, tables, T, out, ws, nbytes, None)

    def grow(masks=p, N=1, H=8, W=8, r2=4, shrink=0, out=q, ws=p, nbytes=big):
        return lib.xmem_mask_grow(masks, N, H, W, r2, shrink, out, ws, nbytes, None)

    for query in (lib.xmem_signed_edt_workspace_bytes, lib.xmem_mask_matte_workspace_bytes):
        assert query(1, 480, 854, 3) >= 3 * 480 * 854 and query(32, 480, 854, 3) >= 32 * 3 * 480 * 854 and query(1, 1, 1, 1) > 0
        assert query(65535, 16384, 16384, 255) >= 65535 * 255 * 16384 * 16384
        for args in ((0, 8, 8, 1), (65536, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 16385, 8, 1), (1, 8, 16385, 1), (1, 8, 8, 0),
                     (1, 8, 8, 256), (-1, 8, 8, 1), (1, 8, 8, -2)):
            assert query(*args) == 0, args
    query = lib.xmem_mask_grow_workspace_bytes
    assert query(1, 480, 854) >= 2 * 480 * 854 and query(1, 1, 1) > 0 and query(65535, 16384, 16384) >= 2 * 65535 * 16384 * 16384
    for args in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 16385, 8), (1, 8, 16385), (-1, 8, 8)):
        assert query(*args) == 0, args

    for fn in (edt, mat):
        for kw in ({'N': 0}, {'N': 65536}, {'K': 0}, {'K': 256}, {'R': 0}, {'R': 128}, {'R': -1}):
            assert fn(**kw) == BAD_ARG, (fn.__name__, kw)
        for kw in ({'H': 0}, {'W': 0}, {'H': -1}, {'H': 16385}, {'W': 16385}):
            assert fn(**kw) == UNSUPPORTED, (fn.__name__, kw)
        for name in ('masks', 'out', 'ws'):
            assert fn(**{name: None}) == BAD_ARG, (fn.__name__, name)
        assert fn(ws=ctypes.c_void_p(4100)) == BAD_ARG               # the workspace is 8-byte aligned
        assert fn(nbytes=0) == WORKSPACE and fn(nbytes=lib.xmem_signed_edt_workspace_bytes(1, 8, 8, 2) - 1) == WORKSPACE
    assert edt(out=ctypes.c_void_p((1 << 30) + 2)) == BAD_ARG        # int32 planes
    for kw in ({'T': 0}, {'T': 5}, {'T': -1}, {'tables': None}):
        assert mat(**kw) == BAD_ARG, kw
    for kw in ({'N': 0}, {'N': 65536}, {'r2': 0}, {'r2': 127 * 127 + 1}, {'r2': -4}, {'masks': None}, {'out': None},
               {'ws': None}, {'ws': ctypes.c_void_p(4100)}):
        assert grow(**kw) == BAD_ARG, kw
        assert grow(shrink=1, **kw) == BAD_ARG, kw
    assert grow(H=0) == UNSUPPORTED and grow(W=-1) == UNSUPPORTED and grow(H=16385) == UNSUPPORTED and grow(W=16385, shrink=1) == UNSUPPORTED
    assert grow(nbytes=0) == WORKSPACE and grow(nbytes=query(1, 8, 8) - 1) == WORKSPACE
    for out in (4096, 4096 + 63, 4096 - 63):                         # out overlaps masks [4096, 4096 + 64)
        assert grow(out=ctypes.c_void_p(out)) == BAD_ARG and grow(out=ctypes.c_void_p(out), shrink=1) == BAD_ARG


def test_ops_refuses_host_tensors_and_bad_options():
    import torch
    from xmem2_amd import ops
    host = torch.zeros((8, 8), dtype=torch.uint8)
    tables = torch.zeros((1, 33), dtype=torch.uint8)
    for call in (lambda: ops.signed_edt_sq(host, 1, 3), lambda: ops.mask_mattes(host, 1, tables, 3), lambda: ops.grow_masks(host, 2)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()
    for call in (lambda: ops.signed_edt_sq(host, 0, 3), lambda: ops.signed_edt_sq(host, 256, 3), lambda: ops.signed_edt_sq(host, 1, 128),
                 lambda: ops.signed_edt_sq(host, 1, 0), lambda: ops.signed_edt_sq(host, True, 3), lambda: ops.mask_mattes(host, 1, tables, 1.5),
                 lambda: ops.grow_masks(host, 0), lambda: ops.grow_masks(host, 0.5), lambda: ops.grow_masks(host, 128),
                 lambda: ops.grow_masks(host, float('nan'))):
        with pytest.raises(ValueError):
            call()


def test_the_command_line_parses():
    args = matte.parse_args(['--tracks', 't.json', '--out', 'o', '--feather', '3', '--trimap', '2', '--offset', '-1', '--falloff', 'smooth'])
    assert args.spec == {'feather': 3.0, 'offset': -1.0, 'falloff': 'smooth', 'trimap': 2.0} and args.tracks == 't.json'
    assert matte.parse_args(['--masks', 'd', '--out', 'o']).spec == {'feather': 2.0, 'offset': 0.0, 'falloff': 'linear', 'trimap': None}
    assert matte.parse_args(['--masks', 'd', '--out', 'o', '--feather', 'none', '--trimap', '1']).spec['feather'] is None
    for bad in (['--out', 'o'], ['--tracks', 't', '--masks', 'd', '--out', 'o'], ['--tracks', 't'], ['--tracks', 't', '--out', 'o', '--feather', '-1'],
                ['--tracks', 't', '--out', 'o', '--feather', 'none'], ['--tracks', 't', '--out', 'o', '--trimap', '300']):
        with pytest.raises(SystemExit):
            matte.parse_args(bad)
