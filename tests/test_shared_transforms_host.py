"""Host side of the shared Winograd transforms: the entry points are declared, bound and exported, the ABI version did not move, and
the size queries cover the layouts the source implies.  No GPU: the queries dereference no pointer of a descriptor."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('xmem_conv2d_shared_input_workspace_bytes', 'xmem_conv2d_m_bytes', 'xmem_conv2d_shared_input', 'xmem_conv2d_nhwc_folded',
       'xmem_conv2d_output_from_m')
F4_64, F4_STREAM, DIRECT_64 = 19, 23, 3
FAKE = 0x10000          # a 16-byte aligned address nobody reads


def test_entry_points_are_declared_bound_and_exported():
    from xmem2_amd import _lib
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW) and _lib.CONV_SHARED_MAX == 3
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert name in doc, f'{name} is not documented in INTEGRATION.md'


def test_abi_version_and_descriptor_did_not_move():
    from xmem2_amd import _lib
    assert 5 == _lib.ABI_VERSION == _lib.load().xmem_version()
    assert C.sizeof(_lib.ConvDesc) == 208


def desc(B, H, W, cin, ldin, cout, plan, relu_in=0, inp=FAKE):
    from xmem2_amd._lib import ConvDesc
    d = ConvDesc()
    d.inp, d.B, d.H, d.W, d.Cin, d.ldin = inp, B, H, W, cin, ldin
    d.w, d.Cout, d.KH, d.KW, d.stride, d.pad = FAKE, cout, 3, 3, 1, 1
    d.scale = d.shift = d.out = d.w_winograd = d.w_winograd4 = FAKE
    d.ldout, d.relu_in, d.plan_tile, d.plan_splitk = cout, relu_in, plan, 1
    return d


def array(ds):
    from xmem2_amd._lib import ConvDesc
    return (C.POINTER(ConvDesc) * len(ds))(*[C.pointer(d) for d in ds])


@pytest.mark.parametrize('B,H,W', [(1, 7, 9), (2, 13, 6), (1, 8, 12), (4, 30, 54)])
@pytest.mark.parametrize('cin,ldin', [(32, 100), (64, 64)])
def test_size_queries_cover_the_layouts(B, H, W, cin, ldin):
    """V [36][P][Cin] per distinct relu_in, then one M [36][P][max Cout]; a deferred M is [36][P][Cout]; P = B ceil(H/4) ceil(W/4)."""
    from xmem2_amd import _lib
    lib = _lib.load()
    P = B * -(-H // 4) * -(-W // 4)
    couts = (32, 132, 64)
    for flags in ((1, 0), (0, 1, 0), (0, 0), (1, 1, 1)):
        ds = [desc(B, H, W, cin, ldin, c, p, relu_in=f) for f, c, p in zip(flags, couts, (F4_64, F4_STREAM, F4_64))]
        need = lib.xmem_conv2d_shared_input_workspace_bytes(array(ds), len(ds))
        assert need >= 36 * P * (len(set(flags)) * cin + max(couts[:len(flags)])) * 4
        for d in ds:
            assert lib.xmem_conv2d_m_bytes(C.byref(d)) >= 36 * P * d.Cout * 4
            assert lib.xmem_conv2d_workspace_bytes(C.byref(d)) >= 36 * P * (cin + d.Cout) * 4      # what the folded entry asks for


def test_ineligible_calls_are_refused_before_any_gpu_work():
    from xmem2_amd import _lib
    lib = _lib.load()
    UNSUPPORTED, BAD_ARG = -2, -1
    mk = lambda **kw: desc(1, 8, 12, kw.pop('cin', 64), kw.pop('ldin', 64), kw.pop('cout', 32), kw.pop('plan', F4_64), **kw)
    no_m, no_b = (C.c_void_p * 3)(), (C.c_size_t * 3)()
    run = lambda ds: lib.xmem_conv2d_shared_input(array(ds), len(ds), no_m, no_b, None, 0, None)
    size = lambda ds: lib.xmem_conv2d_shared_input_workspace_bytes(array(ds), len(ds))
    for ds in ([mk(), mk(plan=DIRECT_64)],                     # one plan is the direct form
               [mk(), mk(plan=9)],                             # F(2x2)
               [mk(cin=36, ldin=100), mk(cin=36, ldin=100)],   # Cin % 32: no Winograd form at all
               [mk(), mk(inp=FAKE + 4096)],                    # not the same tensor
               [mk(), mk(ldin=128)],
               [mk(), mk(cin=32)]):
        assert size(ds) == 0 and run(ds) == UNSUPPORTED
    split = mk()
    split.arith, split.w_split, split.w_winograd_split, split.w_winograd4_split = 1, FAKE, FAKE, FAKE
    assert size([mk(), split]) == 0 and run([mk(), split]) == UNSUPPORTED
    assert lib.xmem_conv2d_m_bytes(C.byref(split)) == 0 and lib.xmem_conv2d_m_bytes(C.byref(mk(plan=DIRECT_64))) == 0
    assert run([mk()]) == BAD_ARG and run([mk()] * 4) == BAD_ARG
    # an eligible call with too small a workspace is refused as well
    assert run([mk(), mk(relu_in=1)]) == -3
    # the fold: both sides F(4x4) on one tile grid, the main convolution without a residual of its own
    fold = lambda d, b: lib.xmem_conv2d_nhwc_folded(C.byref(d), C.byref(b), FAKE, 1 << 40, FAKE, 0, None)
    assert fold(mk(plan=DIRECT_64), mk()) == UNSUPPORTED and fold(mk(), mk(plan=DIRECT_64)) == UNSUPPORTED
    assert fold(mk(), mk(cout=64)) == UNSUPPORTED
    assert fold(mk(), desc(1, 8, 16, 64, 64, 32, F4_64)) == UNSUPPORTED
    with_res = mk()
    with_res.res, with_res.ldres = FAKE, 32
    assert fold(with_res, mk()) == BAD_ARG
    assert fold(mk(), mk()) == -3          # eligible: stops at the empty workspace
