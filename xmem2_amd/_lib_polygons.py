"""ctypes binding of include/xmem_hip_polygons.h, the third header of libxmem_hip.so (polygon outlines of index masks): one call of
`_lib.bind_header`, as `_lib_masks`."""
from . import _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH, CONSTANTS, EXPORTED_SYMBOLS, load = _lib.bind_header('xmem_hip_polygons.h')
POLY_META = CONSTANTS['XMEM_POLY_META']                      # int32 per (frame, label) of xmem_mask_polygons' meta: corners, rings
MAX_CAPACITY = CONSTANTS['XMEM_POLY_MAX_CAPACITY']
