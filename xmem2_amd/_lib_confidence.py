"""ctypes binding of include/xmem_hip_confidence.h, the eighth header of libxmem_hip.so (confidence and uncertainty maps): one call of
`_lib.bind_header`, as `_lib_temporal`."""
from . import _lib
from ._lib import XMemHipError, check, ptr, stream_ptr      # noqa: F401  (the callers' one import)

HEADER_PATH, CONSTANTS, EXPORTED_SYMBOLS, load = _lib.bind_header('xmem_hip_confidence.h')
MAX_C = CONSTANTS['XMEM_CONFIDENCE_MAX_C']                    # classes, background included
MAX_TAU = CONSTANTS['XMEM_CONFIDENCE_MAX_TAU']                # of the threshold
MAX_PASSES = CONSTANTS['XMEM_CONFIDENCE_MAX_PASSES']          # of the integer route
RECORD = CONSTANTS['XMEM_CONFIDENCE_RECORD']                  # int64 values per label
AREA, MARGIN_SUM, LOW, CONTESTED = (CONSTANTS['XMEM_CONFIDENCE_' + n] for n in ('AREA', 'MARGIN_SUM', 'LOW', 'CONTESTED'))
