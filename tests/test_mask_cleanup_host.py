"""Mask clean-up without a GPU: the host definition (xmem2_amd/mask_cleanup.py) against the scipy oracle (cleanup_refs.py) on every
pattern of the GPU tests, the chair annotation, `parse_cleanup`, the second header and its binding, the argument checks of the C entry
points (which answer before any GPU work) and the `--clean` option of the rle tool."""
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image

import cleanup_refs as R
from conftest import GOLDEN, ROOT
from xmem2_amd import mask_cleanup as M

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # xmem_status (include/xmem_hip.h)


def _cases():
    cases = dict(R.patterns())
    for K, p in R.RANDOM:
        for h, w in ((64, 64), (33, 65), (1, 70), (70, 1)):
            cases[f'random_K{K}_p{p}_{h}x{w}'] = R.random_mask(h, w, K, p)
    cases['one_pixel'] = np.array([[7]], np.uint8)
    return cases


CASES = _cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_components_host_equals_the_oracle(name):
    m = CASES[name]
    for conn in (4, 8):
        root, area = M.components_host(m, conn)
        ref_root, ref_area = R.components_ref(m, conn)
        assert root.dtype == area.dtype == np.int32 and root.shape == area.shape == m.shape
        assert (root == ref_root).all() and (area == ref_area).all(), (name, conn)


@pytest.mark.parametrize('name', sorted(CASES))
def test_clean_host_equals_the_oracle(name):
    m = CASES[name]
    for args in R.CLEAN_ARGS + ((0, 3, False), (9, 0, False)):
        out, stats = M.clean_host(m, *args)
        ref_out, ref_stats = R.clean_ref(m, *args)
        assert out.dtype == np.uint8 and stats.dtype == np.int32 and stats.shape == (4,)
        assert (out == ref_out).all() and (stats == ref_stats).all(), (name, args, stats, ref_stats)


def test_the_patterns_make_every_rule_fire():
    """What the patterns are there for, from the oracle alone."""
    assert len(np.unique(R.components_ref(R.serpentine(), 8)[0][R.serpentine() > 0])) == 1        # one component, the longest chain
    cb = R.checkerboard()
    assert len(np.unique(R.components_ref(cb, 8)[0])) == 2 and len(np.unique(R.components_ref(cb, 4)[0])) == cb.size
    ring = R.rings()
    out, stats = R.clean_ref(ring, 0, 10 ** 6, False)
    assert stats[2] == 1 and (out == 0).sum() == (ring == 0).sum() - stats[3]     # only the innermost hole (inside label 1 or 2 alone) may go
    out, stats = R.clean_ref(R.border_hole(), 0, 8, False)
    assert list(stats) == [0, 0, 1, 4] and (out[10:12, 0:2] == 0).all() and (out[31:33, 39] == 0).all() and out[-1, -1] == 0
    out, stats = R.clean_ref(R.equal_blobs(), 0, 0, True)
    assert (out[5:11, 60:66] == 2).all() and (out[30:36, 10:16] == 0).all() and list(stats[:2]) == [3, 36 + 9 + 4]
    for K, p in R.RANDOM:
        stats = R.clean_ref(R.random_mask(64, 64, K, p), 4, 6, False)[1]
        assert stats.min() > 0, (K, p, stats)


def test_result_does_not_depend_on_orientation():
    """No traversal order in the definition: the flipped mask has the flipped components (areas; roots are first pixels, so compared
    as partitions)."""
    m = R.random_mask(40, 52, 3, .5)
    root, area = M.components_host(m, 8)
    froot, farea = M.components_host(m[::-1, ::-1].copy(), 8)
    assert (farea[::-1, ::-1] == area).all()
    assert len(np.unique(root)) == len(np.unique(froot)) == len(set(zip(root.reshape(-1).tolist(), froot[::-1, ::-1].reshape(-1).tolist())))


def test_chair_annotation():
    m = (np.array(Image.open(os.path.join(GOLDEN, 'chair', 'Annotations', 'frame_000000.png'))) > 0).astype(np.uint8)
    root, area = M.components_host(m, 8)
    roots = np.unique(root)
    sizes = {int(r): (int(m.reshape(-1)[r]), int(area.reshape(-1)[r])) for r in roots}
    print('chair frame 0, 8-connected components root -> (value, area):', sizes)
    root4, area4 = M.components_host(m, 4)
    print('4-connected zero components:', sorted(int(area4.reshape(-1)[r]) for r in np.unique(root4[m == 0])))
    assert len(roots) == 6                                           # the object, the background, 4 enclosed holes
    assert [a for v, a in sizes.values() if v == 1] == [5233]
    assert (root == R.components_ref(m, 8)[0]).all() and (area == R.components_ref(m, 8)[1]).all()
    out, stats = M.clean_host(m, min_area=64, max_hole=64)
    assert list(stats) == [0, 0, 3, 73]
    assert int((out == 1).sum()) == 5306 and int((out > 0).sum()) == 5306
    ref_out, ref_stats = R.clean_ref(m, 64, 64, False)
    assert (out == ref_out).all() and (stats == ref_stats).all()


def test_definition_refuses_what_is_not_a_mask():
    for bad in (np.zeros((2, 2), np.int32), np.zeros((2, 2, 2), np.uint8), np.zeros((0, 3), np.uint8)):
        with pytest.raises(ValueError):
            M.components_host(bad, 8)
    with pytest.raises(ValueError):
        M.components_host(np.zeros((2, 2), np.uint8), 6)
    with pytest.raises(ValueError):
        M.clean_host(np.zeros((2, 2), np.uint8), min_area=-1)


def test_parse_cleanup():
    assert M.parse_cleanup(None) is None
    assert M.parse_cleanup({}) is None and M.parse_cleanup({'min_area': 0, 'max_hole': 0, 'keep_largest': False}) is None
    assert M.parse_cleanup({'min_area': 1}) is None                  # no component is smaller than one pixel
    assert M.parse_cleanup({'min_area': 16}) == {'min_area': 16, 'max_hole': 0, 'keep_largest': False}
    assert M.parse_cleanup({'max_hole': np.int64(3), 'keep_largest': True}) == {'min_area': 0, 'max_hole': 3, 'keep_largest': True}
    assert M.parse_cleanup({'keep_largest': 1}) == {'min_area': 0, 'max_hole': 0, 'keep_largest': True}
    for bad in ({'min_area': -1}, {'max_hole': -3}, {'min_area': 2.0}, {'max_hole': '4'}, {'min_area': True}, {'keep_largest': 2},
                {'keep_largest': 'yes'}, {'min_size': 3}, {'min_area': 4, 'holes': 1}, [('min_area', 3)], 16, {'min_area': 2 ** 31}):
        with pytest.raises(ValueError):
            M.parse_cleanup(bad)


def test_config_key_is_optional_and_the_default_config_has_none():
    from xmem2_amd.configuration import VIDEO_INFERENCE_CONFIG
    from xmem2_amd.run_on_video import _clean_output
    assert 'mask_cleanup' not in VIDEO_INFERENCE_CONFIG
    marker = object()
    assert _clean_output(None, marker) is marker                     # nothing is loaded, nothing is launched


def _declared(path):
    text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(xmem_[a-z0-9_]+)\s*\(', text)))


def test_second_header_parses_and_the_library_exports_it():
    from xmem2_amd import _header, _lib, _lib_masks, build
    path = os.path.join(ROOT, 'include', 'xmem_hip_masks.h')
    constants, structs, sigs = _header.parse(open(path).read())
    assert structs == {} and constants['XMEM_CLEAN_STATS'] == 4 == _lib_masks.CLEAN_STATS == len(M.STATS)
    assert sorted(sigs) == _declared(path) == sorted(_lib_masks.EXPORTED_SYMBOLS)
    assert sorted(sigs) == ['xmem_components', 'xmem_components_workspace_bytes', 'xmem_mask_clean', 'xmem_mask_clean_workspace_bytes']
    assert sigs['xmem_components'] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 +
                                       [ctypes.c_size_t, ctypes.c_void_p])
    assert sigs['xmem_mask_clean'] == (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3 +
                                       [ctypes.c_size_t, ctypes.c_void_p])
    assert sigs['xmem_mask_clean_workspace_bytes'] == sigs['xmem_components_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    lib = _lib_masks.load()
    assert lib is _lib.load()
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # the first header and what is derived from it stay where they are
    assert len(_lib._SIGS) == 103 and _lib.ABI_VERSION == 5 and not set(sigs) & set(_lib.EXPORTED_SYMBOLS)
    assert 'components.hip' in build.SOURCES and 'xmem_hip_masks.h' in build.PUBLIC_HEADERS


def test_build_tracks_the_second_header(tmp_path, monkeypatch):
    from xmem2_amd import build
    digest = build.source_digest()
    inc = tmp_path / 'include'
    inc.mkdir()
    for f in build.PUBLIC_HEADERS:
        (inc / f).write_bytes(open(os.path.join(build.INCLUDE, f), 'rb').read() + (b'\n/* changed */\n' if f == 'xmem_hip_masks.h' else b''))
    monkeypatch.setattr(build, 'INCLUDE', str(inc))
    assert build.source_digest() != digest
    assert build.needs_build()                                       # the copied headers are newer than the library


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib_masks
    lib = _lib_masks.load()
    p = ctypes.c_void_p(4096)                                        # never dereferenced: every call below is refused on the host
    q = ctypes.c_void_p(1 << 20)
    big = 1 << 40

    def comp(masks=p, N=1, H=8, W=8, conn=8, root=p, area=p, ws=p, nbytes=big):
        return lib.xmem_components(masks, N, H, W, conn, root, area, ws, nbytes, None)

    def clean(masks=p, N=1, H=8, W=8, min_area=1, max_hole=1, keep=0, out=q, stats=p, ws=p, nbytes=big):
        return lib.xmem_mask_clean(masks, N, H, W, min_area, max_hole, keep, out, stats, ws, nbytes, None)

    for query in (lib.xmem_components_workspace_bytes, lib.xmem_mask_clean_workspace_bytes):
        assert query(1, 480, 854) >= 4 * 480 * 854 and query(3, 16384, 16384) >= 3 * 4 * 16384 ** 2
        for N, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 16385, 8), (1, 8, 16385), (1, -4, 8)):
            assert query(N, H, W) == 0, (N, H, W)
    assert lib.xmem_mask_clean_workspace_bytes(2, 100, 100) > lib.xmem_components_workspace_bytes(2, 100, 100)
    for call in (comp, clean):
        assert call(N=0) == BAD_ARG and call(N=-2) == BAD_ARG
        for kw in ({'H': 0}, {'W': 0}, {'H': 16385}, {'W': 16385}, {'H': -1}):
            assert call(**kw) == UNSUPPORTED, kw
        assert call(masks=None) == BAD_ARG and call(ws=None) == BAD_ARG
        assert call(nbytes=0) == WORKSPACE and call(nbytes=8 * 8 * 4 - 1) == WORKSPACE
    for conn in (0, 1, 6, 9, -8):
        assert comp(conn=conn) == BAD_ARG
    assert comp(root=None) == BAD_ARG and comp(area=None) == BAD_ARG
    assert clean(min_area=-1) == BAD_ARG and clean(max_hole=-1) == BAD_ARG
    assert clean(out=None) == BAD_ARG and clean(stats=None) == BAD_ARG
    assert clean(out=p) == BAD_ARG                                   # out aliases masks
    assert clean(out=ctypes.c_void_p(4096 + 63)) == BAD_ARG          # out overlaps masks' last byte
    assert clean(nbytes=lib.xmem_mask_clean_workspace_bytes(1, 8, 8) - 1) == WORKSPACE


def test_ops_refuse_host_tensors_and_bad_options():
    import torch
    from xmem2_amd import ops
    m = torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.components(m)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.clean_masks(m, min_area=2)
    with pytest.raises(ValueError):
        ops.components(m, connectivity=6)
    with pytest.raises(ValueError):
        ops.clean_masks(m, min_area=-2)


def test_rle_tool_parses_clean():
    from xmem2_amd import rle
    args = rle.parse_args(['--tracks', 'a.json', '--clean', '{"min_area": 16, "max_hole": 16}', '--out', 'b.json'])
    assert args.clean == {'min_area': 16, 'max_hole': 16, 'keep_largest': False} and args.tracks == 'a.json' and args.out == 'b.json'
    args = rle.parse_args(['--tracks', 'a.json', '--clean', '{"keep_largest": true}', '--recode', 'compressed', '--out', 'b.json'])
    assert args.clean == {'min_area': 0, 'max_hole': 0, 'keep_largest': True} and args.recode == 'compressed'
    assert rle.parse_args(['--tracks', 'a.json', '--recode', 'list', '--out', 'b.json']).clean is None
    for bad in ('{"min_area": -1}', '{"area": 3}', 'not json', '[1]', '{}'):
        with pytest.raises(SystemExit):
            rle.parse_args(['--tracks', 'a.json', '--clean', bad, '--out', 'b.json'])
    with pytest.raises(SystemExit):
        rle.parse_args(['--tracks', 'a.json', '--clean', '{"min_area": 4}'])      # a cleaned file needs somewhere to go
