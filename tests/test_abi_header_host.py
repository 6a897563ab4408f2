"""The ctypes binding derived from include/xmem_hip.h (xmem2_amd/_header.py), no GPU: the reader on a literal header of its dialect, the
parsed structs against the compiler, the parsed functions against the library, and the facts earlier tests froze family by family."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'xmem_hip.h')
DIALECT = '''/* every construct the reader takes */
#ifndef T_H
#define T_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define XMEM_N 3          // sizes an array below
enum { XMEM_A = 0, XMEM_B = 1 };
typedef enum { XMEM_FINE = 0, XMEM_BAD = -1, XMEM_WORSE = -2 /* xmem_not_a_call( */ } xmem_code;
typedef struct {
    const float* in;  int B, H, ldin;   /* several declarators */
    double m[XMEM_N]; uint8_t flag[2];
} xmem_thing;
int xmem_zero(void);
size_t xmem_many(const xmem_thing* const* things, void* const* bufs, const size_t* sizes, float f, size_t n);
const char* xmem_text(const xmem_thing* t, const uint16_t* dev, uint64_t bits);
#ifdef __cplusplus
}
#endif
#endif
'''
STRUCT_SIZES = dict(xmem_conv_desc=208, xmem_conv_plan_info=28, xmem_aug_desc=80, xmem_key_segment=32, xmem_affinity_hint=40,
                    xmem_affinity_plan=36, xmem_value_segment=16, xmem_compact_arena=32)
ARITIES = dict(xmem_store_compact=7, xmem_copy_segments=5, xmem_rle_decode=11, xmem_selector_prepare_u8=17, xmem_conv2d_m_bytes=1,
               xmem_conv2d_shared_input_workspace_bytes=2, xmem_conv2d_shared_input=7, xmem_conv2d_nhwc_folded=7, xmem_conv2d_output_from_m=4)


def test_reader_takes_its_dialect_and_refuses_everything_else():
    from xmem2_amd._header import parse
    constants, structs, functions = parse(DIALECT)
    assert constants == dict(XMEM_N=3, XMEM_A=0, XMEM_B=1, XMEM_FINE=0, XMEM_BAD=-1, XMEM_WORSE=-2)
    (thing,) = structs.values()
    assert list(structs) == ['xmem_thing'] and issubclass(thing, C.Structure) and C.sizeof(thing) == 56 and thing.flag.offset == 48
    assert thing._fields_ == [('inp', C.c_void_p), ('B', C.c_int), ('H', C.c_int), ('ldin', C.c_int), ('m', C.c_double * 3), ('flag', C.c_uint8 * 2)]
    assert functions == dict(
        xmem_zero=(C.c_int, []),
        xmem_many=(C.c_size_t, [C.POINTER(C.POINTER(thing)), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_float, C.c_size_t]),
        xmem_text=(C.c_char_p, [C.POINTER(thing), C.c_void_p, C.c_uint64]))
    for bad, what in (('long xmem_f(int a);', 'long'), ('int xmem_f(float** rows);', 'float**'),                       # an unknown type
                      ('int xmem_f(int);', "'int'"), ('typedef struct { int a b; } xmem_s;', 'int a'),                 # a declarator that cannot be split
                      ('typedef struct { float v[2.5]; } xmem_s;', '2.5'), ('#define XMEM_HALF 0.5', '0.5'),           # a non-integer size / constant
                      ('typedef struct { float v[XMEM_UNSET]; } xmem_s;', 'XMEM_UNSET'),
                      ('static int counter;', 'static int counter;'), ('int xmem_f(int (*callback)(int));', 'callback')):  # a statement left over
        with pytest.raises(ValueError, match=re.escape(what)):
            parse(DIALECT.replace('int xmem_zero(void);', 'int xmem_zero(void);\n' + bad))


def test_parsed_structs_have_the_compilers_layout(tmp_path):
    """sizeof of every struct and offsetof of every field of the real header, as a host C++ compiler sees them."""
    from xmem2_amd import _lib, build
    from xmem2_amd._header import FIELD_NAMES
    c_name = {v: k for k, v in FIELD_NAMES.items()}
    want = {}
    for name, struct in _lib._STRUCTS.items():
        want[f'sizeof({name})'] = C.sizeof(struct)
        want.update({f'offsetof({name}, {c_name.get(f, f)})': getattr(struct, f).offset for f, _ in struct._fields_})
    src, exe = tmp_path / 'layout.cpp', tmp_path / 'layout'
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "xmem_hip.h"\nint main() {\n'
                   + ''.join(f'    std::printf("%zu\\n", {x});\n' for x in want) + '    return 0;\n}\n')
    subprocess.run([build._hipcc(), '-x', 'c++', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(want) == 8 + 33 + 7 + 4 + 4 + 5 + 9 + 2 + 5 and dict(zip(want, map(int, got))) == want


def test_library_is_bound_as_the_header_declares():
    from xmem2_amd import _lib
    lib = _lib.load()
    for name, (restype, argtypes) in _lib._SIGS.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.xmem_version() == _lib.CONSTANTS['XMEM_ABI_VERSION'] == _lib.ABI_VERSION == 5


def test_frozen_abi_facts():
    from xmem2_amd import _lib, rle
    assert _lib.EXPORTED_SYMBOLS == tuple(_lib._SIGS) and len(_lib._SIGS) == 103
    assert {n: C.sizeof(s) for n, s in _lib._STRUCTS.items()} == STRUCT_SIZES
    assert {n: len(_lib._SIGS[n][1]) for n in ARITIES} == ARITIES
    assert _lib.ConvDesc is _lib._STRUCTS['xmem_conv_desc'] and _lib.ConvDesc._fields_[0] == ('inp', C.c_void_p)
    assert [n for n, _ in _lib.CompactArena._fields_] == ['src', 'dst', 'width', 'n', 'off']
    assert _lib.ABI_VERSION == 5 and _lib.UNSUPPORTED == -2 and _lib.CONV_SHARED_MAX == 3 and _lib.DILATED_NO_TAP_SKIP == 1
    assert _lib.COPY_MAX_SEGMENTS >= 16 and _lib.COMPACT_MAX_ARENAS >= 8 and _lib.RLE_META == rle.META == 6
    assert _lib.CONV_FORMS == ('gemv', 'direct', 'f2', 'f2_fused', 'f2_f16', 'f4')
    assert _lib.CONSTANTS['XMEM_ROWS16_HALFS'] == 144 and _lib.CONSTANTS['XMEM_MAX_SEGMENTS'] == 4 and _lib.CONSTANTS['XMEM_AUG_MAX'] == 32
