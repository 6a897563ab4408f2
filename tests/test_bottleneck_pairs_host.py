"""xmem_conv2d_pointwise_pair on the host: argument validation and the unsupported answers, with dummy operand pointers - every
case here is answered before any GPU work, nothing is launched (the pattern of test_conv_plan_host.py)."""
import ctypes as C

import pytest

_PTR = 0x10000                                                   # nothing is dereferenced: any non-null 16-byte-aligned value
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope='module')
def lib():
    from xmem2_amd import build as B
    from xmem2_amd import _lib
    B.build(force=False, verbose=False)
    return _lib.load()


def pair(k1=64, n2=64, B=1, H=8, W=8, plan_e=(3, 1), plan_r=(3, 1)):
    """(expand, reduce) descriptors of a pair the entry point takes: k1 -> 4 k1 (+ residual, relu) -> n2 (relu)."""
    from xmem2_amd._lib import ConvDesc
    e, r = ConvDesc(), ConvDesc()
    for d, cin, cout, plan in ((e, k1, 4 * k1, plan_e), (r, 4 * k1, n2, plan_r)):
        d.inp, d.w, d.scale, d.shift, d.out = _PTR, _PTR, _PTR, _PTR, _PTR
        d.B, d.H, d.W, d.Cin, d.ldin = B, H, W, cin, cin
        d.Cout, d.KH, d.KW, d.stride, d.pad = cout, 1, 1, 1, 0
        d.ldout = cout
        d.relu_in, d.relu_out = 0, 1
        d.plan_tile, d.plan_splitk = plan
    e.res, e.ldres = _PTR, 4 * k1
    e.out = r.inp = _PTR + 0x100000
    return e, r


def call(lib, e, r):
    return lib.xmem_conv2d_pointwise_pair(C.byref(e), C.byref(r), None)


def test_null_and_invalid_descriptors_are_bad_arguments(lib):
    e, r = pair()
    assert lib.xmem_conv2d_pointwise_pair(None, C.byref(r), None) == BAD_ARG
    assert lib.xmem_conv2d_pointwise_pair(C.byref(e), None, None) == BAD_ARG
    for field in ('inp', 'w', 'scale', 'shift', 'out'):
        for which in (0, 1):
            e, r = pair()
            setattr((e, r)[which], field, None)
            assert call(lib, e, r) == BAD_ARG, (field, which)
    e, r = pair()
    e.plan_tile = 41
    assert call(lib, e, r) == BAD_ARG
    e, r = pair()
    r.B = 0
    assert call(lib, e, r) == BAD_ARG
    e, r = pair()
    e.ldres = 4 * 64 - 4                         # a residual narrower than the output
    assert call(lib, e, r) == BAD_ARG


@pytest.mark.parametrize('field, value', [('inp', _PTR + 0x200000), ('ldin', 4 * 64 + 4), ('Cin', 128), ('B', 2), ('H', 4), ('W', 16)])
def test_reduce_must_read_the_expand_output(lib, field, value):
    e, r = pair()
    setattr(r, field, value)
    if field == 'Cin':
        r.ldin = 4 * 64                          # (still a valid descriptor on its own)
    assert call(lib, e, r) == BAD_ARG


def test_unsupported_answers(lib):
    def changed(which, **fields):
        e, r = pair()
        for k, v in fields.items():
            setattr((e, r)[which], k, v)
        return call(lib, e, r)
    assert changed(0, res=None) == UNSUPPORTED                   # the expand layer has no residual
    assert changed(1, res=_PTR, ldres=64) == UNSUPPORTED         # the reduce layer has one
    assert changed(0, res_broadcast=1) == UNSUPPORTED
    assert changed(0, relu_out=0) == UNSUPPORTED
    assert changed(1, relu_out=0) == UNSUPPORTED
    assert changed(0, relu_in=1) == UNSUPPORTED
    assert changed(1, relu_in=1) == UNSUPPORTED
    assert changed(0, inp=_PTR + 4) == UNSUPPORTED               # the A operand is read as 16-byte groups
    assert changed(1, plan_splitk=2) == UNSUPPORTED              # forced split-K on the reduce layer
    assert changed(0, plan_splitk=2) == UNSUPPORTED
    assert changed(1, plan_tile=35) == UNSUPPORTED               # the streaming kernel
    assert changed(0, plan_tile=35) == UNSUPPORTED
    # the heuristic's own split-K: 1024 -> 256 over 64 pixels is four tiles of a deep K
    e, r = pair(k1=256, n2=256, plan_r=(0, 0))
    assert call(lib, e, r) == UNSUPPORTED
    # the half and split-operand modes
    assert changed(0, arith=1, w_split=_PTR) == UNSUPPORTED
    e, r = pair()
    for d in (e, r):
        d.in_half, d.out_half, d.w_half = 1, 1, _PTR
    assert call(lib, e, r) == UNSUPPORTED


@pytest.mark.parametrize('k1, n2', [(32, 32), (64, 32), (64, 256), (96, 96), (128, 64), (256, 128), (512, 512)])
def test_channel_counts_outside_the_kernel(lib, k1, n2):
    e, r = pair(k1=k1, n2=n2)
    assert call(lib, e, r) == UNSUPPORTED


def test_expand_must_widen_four_times(lib):
    e, r = pair()
    e.Cout = e.ldout = e.ldres = r.Cin = r.ldin = 128
    assert call(lib, e, r) == UNSUPPORTED


def test_strided_and_3x3_layers_are_unsupported(lib):
    e, r = pair(H=8, W=8)
    e.stride = 2
    r.H = r.W = 4                                # the reduce layer then reads the strided output: same B, other H / W
    assert call(lib, e, r) in (BAD_ARG, UNSUPPORTED)
    e, r = pair()
    r.stride = 2
    assert call(lib, e, r) == UNSUPPORTED
    e, r = pair()
    r.KH = r.KW = 3
    r.pad = 1
    assert call(lib, e, r) == UNSUPPORTED


def test_abi_version_agrees_across_header_binding_and_library(lib):
    from xmem2_amd import _lib
    assert _lib.ABI_VERSION == lib.xmem_version()
    assert hasattr(lib, 'xmem_conv2d_pointwise_pair')
