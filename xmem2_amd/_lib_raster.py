"""ctypes binding of include/xmem_hip_raster.h, the fourth header of libxmem_hip.so (polygons filled back into index masks): one call
of `_lib.bind_header`, as `_lib_masks`."""
from . import _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH, CONSTANTS, EXPORTED_SYMBOLS, load = _lib.bind_header('xmem_hip_raster.h')
MAX_FRAC_BITS = CONSTANTS['XMEM_FILL_MAX_FRAC_BITS']
COORD_BOUND = CONSTANTS['XMEM_FILL_COORD_BOUND']             # of a quantised coordinate's magnitude
FILL_STATUS = CONSTANTS['XMEM_FILL_STATUS']                  # int32 of xmem_polygons_fill's status: edges skipped for plane, for coordinate
