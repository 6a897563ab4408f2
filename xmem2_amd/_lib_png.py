"""ctypes binding of include/xmem_hip_png.h, the seventh header of libxmem_hip.so (PNG files built on the device): one call of
`_lib.bind_header`, as `_lib_temporal`."""
from . import _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH, CONSTANTS, EXPORTED_SYMBOLS, load = _lib.bind_header('xmem_hip_png.h')
META = CONSTANTS['XMEM_PNG_META']                             # int32 words per frame of a record's meta
COLOR_TYPES = {'grey': CONSTANTS['XMEM_PNG_GREY'], 'rgb': CONSTANTS['XMEM_PNG_RGB'], 'palette': CONSTANTS['XMEM_PNG_PALETTE']}
MAX_CAPACITY = CONSTANTS['XMEM_PNG_MAX_CAPACITY']
