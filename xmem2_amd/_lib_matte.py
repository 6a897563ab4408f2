"""ctypes binding of include/xmem_hip_matte.h, the fifth header of libxmem_hip.so (signed distances, mattes, trimaps, grow and shrink).

As `_lib_raster`: include/xmem_hip.h and what `_lib` derives from it are frozen at ABI version 5, later entry points are declared
in headers of their own and bound by the same reader (`_header.parse`) on the same `CDLL` that `_lib.load()` returns.
"""
import os

from . import _header, _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'xmem_hip_matte.h')
_bound = None


def _read_header():
    try:
        with open(HEADER_PATH) as fh:
            constants, structs, sigs = _header.parse(fh.read())
    except OSError as e:
        raise XMemHipError(f'{HEADER_PATH} cannot be read ({e}): the ctypes binding is derived from it') from e
    if structs:
        raise XMemHipError(f'{HEADER_PATH} declares structs {sorted(structs)}: this header carries functions and #defines only')
    return constants, sigs


CONSTANTS, _SIGS = _read_header()
EXPORTED_SYMBOLS = tuple(_SIGS)
MAX_R = CONSTANTS['XMEM_MATTE_MAX_R']                         # of the reach R, and of a grow / shrink radius
MAX_TABLES = CONSTANTS['XMEM_MATTE_MAX_TABLES']               # look-up tables one distance pass serves
MAX_LABELS = CONSTANTS['XMEM_MATTE_MAX_LABELS']


def load():
    """`_lib.load()` with this header's signatures set on it (once per handle).  Raises when the library or a symbol is missing."""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)      # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _bound = lib
    return lib
