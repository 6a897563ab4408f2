"""ctypes binding of include/xmem_hip_matte.h, the fifth header of libxmem_hip.so (signed distances, mattes, trimaps, grow and shrink):
one call of `_lib.bind_header`, as `_lib_masks`."""
from . import _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH, CONSTANTS, EXPORTED_SYMBOLS, load = _lib.bind_header('xmem_hip_matte.h')
MAX_R = CONSTANTS['XMEM_MATTE_MAX_R']                         # of the reach R, and of a grow / shrink radius
MAX_TABLES = CONSTANTS['XMEM_MATTE_MAX_TABLES']               # look-up tables one distance pass serves
MAX_LABELS = CONSTANTS['XMEM_MATTE_MAX_LABELS']
