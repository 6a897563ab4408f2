"""ctypes binding of include/xmem_hip_temporal.h, the sixth header of libxmem_hip.so (the temporal majority vote): one call of
`_lib.bind_header`, as `_lib_matte`."""
from . import _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH, CONSTANTS, EXPORTED_SYMBOLS, load = _lib.bind_header('xmem_hip_temporal.h')
MAX_R = CONSTANTS['XMEM_TEMPORAL_MAX_R']                      # of the radius: a window of at most 2 MAX_R + 1 frames
PRESENT = CONSTANTS['XMEM_TEMPORAL_PRESENT']                  # flag bits of a frame
LOCKED = CONSTANTS['XMEM_TEMPORAL_LOCKED']
SEGMENT = CONSTANTS['XMEM_TEMPORAL_SEGMENT']                  # output frames per time segment of one launch
