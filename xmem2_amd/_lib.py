"""ctypes binding of the C-ABI library, derived at import from its one declaration, include/xmem_hip.h (reader: _header.py).

The product path has NO CPU fallback: if the shared library is missing or fails to load, the first
kernel call raises.  PyTorch is used only for device memory and the current HIP stream.
"""
import ctypes as C
import os

import torch

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libxmem_hip.so')
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'xmem_hip.h')
_lib = None


class XMemHipError(RuntimeError):
    pass


def _read_header(path):
    """(constants, structs, signatures) of one header (type rules: _header).  Each header is parsed once per process, at import."""
    try:
        with open(path) as fh:
            return _header.parse(fh.read())
    except OSError as e:
        raise XMemHipError(f'{path} cannot be read ({e}): the ctypes binding is derived from it') from e


def _set_signatures(lib, sigs):
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args


CONSTANTS, _STRUCTS, _SIGS = _read_header(HEADER_PATH)
EXPORTED_SYMBOLS = tuple(_SIGS)

ConvDesc = _STRUCTS['xmem_conv_desc']
ConvPlanInfo = _STRUCTS['xmem_conv_plan_info']
AugDesc = _STRUCTS['xmem_aug_desc']
KeySegment = _STRUCTS['xmem_key_segment']
AffinityHint = _STRUCTS['xmem_affinity_hint']
ValueSegment = _STRUCTS['xmem_value_segment']
CompactArena = _STRUCTS['xmem_compact_arena']

ABI_VERSION = CONSTANTS['XMEM_ABI_VERSION']                  # the layout of ConvDesc belongs to it
UNSUPPORTED = CONSTANTS['XMEM_ERR_UNSUPPORTED']
CONV_SHARED_MAX = CONSTANTS['XMEM_CONV_SHARED_MAX']          # convolutions one xmem_conv2d_shared_input call carries
DILATED_NO_TAP_SKIP = CONSTANTS['XMEM_DILATED_NO_TAP_SKIP']
RLE_META = CONSTANTS['XMEM_RLE_META']                        # int32 values per (frame, label) of xmem_rle_encode's meta
COPY_MAX_SEGMENTS = CONSTANTS['XMEM_COPY_MAX_SEGMENTS']      # (src, dst, bytes) triples one xmem_copy_segments launch carries
COMPACT_MAX_ARENAS = CONSTANTS['XMEM_COMPACT_MAX_ARENAS']    # arena descriptors one xmem_store_compact launch carries
# the XMEM_CONV_* enumerators by value, 0 up: 'gemv', 'direct', 'f2', 'f2_fused', 'f2_f16', 'f4' (XMEM_CONV_SHARED_MAX is a #define)
_FORMS = {v: k[len('XMEM_CONV_'):].lower() for k, v in CONSTANTS.items() if k.startswith('XMEM_CONV_') and k != 'XMEM_CONV_SHARED_MAX'}
CONV_FORMS = tuple(_FORMS[i] for i in range(len(_FORMS)))


def load():
    """Load libxmem_hip.so (once).  Raises loudly when it is absent - there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XMemHipError(
            f'{LIB_PATH} not found: the MI355X kernels are not built. Run `python -m xmem2_amd.build` '
            '(or __graft_entry__.build()). xmem2_amd has no CPU / PyTorch fallback.')
    lib = C.CDLL(LIB_PATH)
    _set_signatures(lib, _SIGS)
    if lib.xmem_version() != ABI_VERSION:
        raise XMemHipError('libxmem_hip.so ABI version mismatch')
    _lib = lib
    return lib


def bind_header(file_name):
    """The binding of a later header of libxmem_hip.so, include/<file_name>: functions and #defines only, since include/xmem_hip.h and
    what this module derives from it are frozen at its ABI version.  Returns (path, constants, exported symbols, load): that `load()`
    returns the handle of `load()` above with this header's signatures set on it - once per handle, and again should the handle ever
    be another.  A `_lib_*` module is one call of this and the constants it lifts out.  (An absolute `file_name` is read as it is.)"""
    path = os.path.join(_HERE, '..', 'include', file_name)
    constants, structs, sigs = _read_header(path)
    if structs:
        raise XMemHipError(f'{path} declares structs {sorted(structs)}: this header carries functions and #defines only')
    bound = None

    def load_bound():
        """`_lib.load()` with this header's signatures set on it (once per handle).  Raises when the library or a symbol is missing."""
        nonlocal bound
        lib = load()
        if bound is not lib:
            _set_signatures(lib, sigs)
            bound = lib
        return lib

    return path, constants, tuple(sigs), load_bound


def check(code):
    if code != 0:
        msg = load().xmem_last_error_string(code).decode()
        raise RuntimeError(f'xmem_hip: {msg} (status {code})')


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())
