"""ctypes binding of include/xmem_hip_motion.h, the ninth header of libxmem_hip.so (luma, the block-motion search, the
motion-compensated vote): one call of `_lib.bind_header`, as `_lib_temporal`."""
from . import _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH, CONSTANTS, EXPORTED_SYMBOLS, load = _lib.bind_header('xmem_hip_motion.h')
BLOCK = CONSTANTS['XMEM_MOTION_BLOCK']                        # pixels of a block's side
MAX_SEARCH = CONSTANTS['XMEM_MOTION_MAX_SEARCH']              # of the search range, in pixels either way
MAX_N = CONSTANTS['XMEM_MOTION_MAX_N']                        # images or pairs of one call
