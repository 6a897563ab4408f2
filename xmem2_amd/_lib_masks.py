"""ctypes binding of include/xmem_hip_masks.h, the second header of libxmem_hip.so (connected components, mask clean-up).

include/xmem_hip.h and what `_lib` derives from it are frozen at ABI version 5; what was added after it is declared in a header of
its own and bound by `_lib.bind_header`: the same reader (`_header.parse`), on the same `CDLL` that `_lib.load()` returns.  `check`,
`ptr` and `stream_ptr` are `_lib`'s.
"""
from . import _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH, CONSTANTS, EXPORTED_SYMBOLS, load = _lib.bind_header('xmem_hip_masks.h')
CLEAN_STATS = CONSTANTS['XMEM_CLEAN_STATS']                  # int32 counters per frame of xmem_mask_clean's stats
