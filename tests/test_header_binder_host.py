"""`_lib.bind_header`, the one binder of the headers after include/xmem_hip.h, no GPU: what it refuses, and that `load()` of each of the
four modules it serves sets that header's signatures on the handle of `_lib.load()` - once, and again on another handle."""
import ctypes as C
import os

import pytest

from conftest import ROOT

MODULES = {'_lib_masks': 'xmem_hip_masks.h', '_lib_polygons': 'xmem_hip_polygons.h', '_lib_raster': 'xmem_hip_raster.h',
           '_lib_matte': 'xmem_hip_matte.h'}
PLAIN = '#define XMEM_T_MAX 7\nint xmem_version(void);\n'
WITH_STRUCT = PLAIN + 'typedef struct { int a; } xmem_t_thing;\n'


def _module(name):
    import importlib
    return importlib.import_module('xmem2_amd.' + name)


def _signatures(file_name):
    from xmem2_amd import _header
    with open(os.path.join(ROOT, 'include', file_name)) as fh:
        constants, structs, sigs = _header.parse(fh.read())
    assert structs == {} and sigs
    return constants, sigs


def test_a_header_with_structs_or_without_a_file_is_refused(tmp_path):
    from xmem2_amd import _lib
    path = tmp_path / 'xmem_hip_t.h'
    path.write_text(WITH_STRUCT)
    with pytest.raises(_lib.XMemHipError) as e:
        _lib.bind_header(str(path))
    assert str(e.value) == f"{path} declares structs ['xmem_t_thing']: this header carries functions and #defines only"
    missing = tmp_path / 'xmem_hip_none.h'
    with pytest.raises(_lib.XMemHipError) as e:
        _lib.bind_header(str(missing))
    assert str(e.value) == (f"{missing} cannot be read ([Errno 2] No such file or directory: '{missing}'): "
                            'the ctypes binding is derived from it')
    assert isinstance(e.value.__cause__, OSError)
    with pytest.raises(_lib.XMemHipError, match='cannot be read'):
        _lib.bind_header('xmem_hip_no_such_header.h')                # a bare name is looked for in include/


def test_a_plain_header_gives_its_path_constants_symbols_and_a_load(tmp_path):
    from xmem2_amd import _lib
    path = tmp_path / 'xmem_hip_t.h'
    path.write_text(PLAIN)
    got_path, constants, symbols, load = _lib.bind_header(str(path))
    assert got_path == str(path) and constants == {'XMEM_T_MAX': 7} and symbols == ('xmem_version',) and callable(load)
    assert load() is _lib.load() and load() is load()


@pytest.mark.parametrize('name', MODULES)
def test_module_keeps_its_names_and_binds_its_header(name):
    from xmem2_amd import _lib
    module = _module(name)
    constants, sigs = _signatures(MODULES[name])
    assert os.path.samefile(module.HEADER_PATH, os.path.join(ROOT, 'include', MODULES[name]))
    assert module.CONSTANTS == constants and module.EXPORTED_SYMBOLS == tuple(sigs)
    assert module.XMemHipError is _lib.XMemHipError and module.check is _lib.check and module.ptr is _lib.ptr
    assert module.stream_ptr is _lib.stream_ptr
    lib = module.load()
    assert lib is _lib.load()
    for symbol, (res, args) in sigs.items():
        fn = getattr(lib, symbol)
        assert fn.restype is res and list(fn.argtypes) == args, symbol


def test_lifted_constants():
    lifted = {'_lib_masks': {'CLEAN_STATS': 'XMEM_CLEAN_STATS'},
              '_lib_polygons': {'POLY_META': 'XMEM_POLY_META', 'MAX_CAPACITY': 'XMEM_POLY_MAX_CAPACITY'},
              '_lib_raster': {'MAX_FRAC_BITS': 'XMEM_FILL_MAX_FRAC_BITS', 'COORD_BOUND': 'XMEM_FILL_COORD_BOUND', 'FILL_STATUS': 'XMEM_FILL_STATUS'},
              '_lib_matte': {'MAX_R': 'XMEM_MATTE_MAX_R', 'MAX_TABLES': 'XMEM_MATTE_MAX_TABLES', 'MAX_LABELS': 'XMEM_MATTE_MAX_LABELS'}}
    for name, names in lifted.items():
        module = _module(name)
        for attr, constant in names.items():
            assert getattr(module, attr) == module.CONSTANTS[constant], (name, attr)


def test_another_handle_is_bound_again(monkeypatch):
    """`_lib.load()` hands out `_lib._lib`; a fresh CDLL of the same file in its place has no signature set until the next `load()`."""
    from xmem2_amd import _lib
    first = _lib.load()
    fresh = C.CDLL(_lib.LIB_PATH)
    assert fresh is not first
    monkeypatch.setattr(_lib, '_lib', fresh)                         # restored when the test ends
    for name, header in MODULES.items():
        module, (_, sigs) = _module(name), _signatures(header)
        some = next(s for s, (res, args) in sigs.items() if args)
        assert getattr(fresh, some).argtypes is None                 # ctypes' default: nothing set
        assert module.load() is fresh
        for symbol, (res, args) in sigs.items():
            fn = getattr(fresh, symbol)
            assert fn.restype is res and list(fn.argtypes) == args, (name, symbol)
    monkeypatch.undo()
    assert _lib.load() is first
    for name, header in MODULES.items():
        assert _module(name).load() is first                         # and back: the first handle's signatures are set anew
        _, sigs = _signatures(header)
        for symbol, (res, args) in sigs.items():
            assert list(getattr(first, symbol).argtypes) == args, (name, symbol)
