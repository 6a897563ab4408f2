"""Host tests of the convolution plan codes (no GPU: the entry points used here only compute): what the library resolves a
`plan_tile` to, that the Python table of the codes says the same, and that the shipped plan tables survive a round trip."""
import ctypes as C
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_plan_info.npz')

# a layer of the fixture: these integer columns, in this order
LAYER_COLS = ('B', 'H', 'W', 'Cin', 'ldin', 'Cout', 'K', 'stride', 'pad', 'ldout', 'ldres', 'out_off')
OPERANDS = ('all', 'winograd only', 'none')                     # {w_winograd, w_winograd4, w_winograd_f16} | {w_winograd} | {}
MODES = ('fp32', 'fp32x', 'fp32x + w_winograd4_split', 'half, out_half 0', 'half, out_half 1')
TILES, SPLITKS = tuple(range(-1, 43)), (0, 1, 3, 64)
DILATIONS, DILATED_TILES = (1, 2, 6), tuple(range(8))
INFO_COLS = ('rc', 'form', 'bm', 'bn', 'bk', 'splitk', 'stream', 'ring')
_PTR = 0x10000                                                   # nothing is dereferenced: any non-null 16-byte-aligned value


def make_desc(layer, operands=0, mode=0):
    """The descriptor of one layer (dummy operand pointers) with an operand set and a mode (indices of OPERANDS / MODES)."""
    from xmem2_amd._lib import ConvDesc
    r = dict(zip(LAYER_COLS, (int(v) for v in layer)))
    d = ConvDesc()
    d.inp, d.w, d.scale, d.shift = _PTR, _PTR, _PTR, _PTR
    d.B, d.H, d.W, d.Cin, d.ldin = r['B'], r['H'], r['W'], r['Cin'], r['ldin']
    d.Cout, d.KH, d.KW, d.stride, d.pad = r['Cout'], r['K'], r['K'], r['stride'], r['pad']
    d.out, d.ldout = _PTR + r['out_off'], r['ldout']
    if r['ldres']:
        d.res, d.ldres = _PTR, r['ldres']
    if operands <= 1:
        d.w_winograd = _PTR
    if operands == 0:
        d.w_winograd4, d.w_winograd_f16 = _PTR, _PTR
    if mode in (1, 2):
        d.arith, d.w_split = 1, _PTR
        d.w_winograd_split = _PTR if operands <= 1 else None
        d.w_winograd4_split = _PTR if mode == 2 and operands == 0 else None
    if mode >= 3:
        d.in_half, d.out_half, d.w_half = 1, int(mode == 4), _PTR
    return d


def plan_info(d, tile, splitk):
    """(rc, form, bm, bn, bk, splitk, stream, ring) of `d` under plan (tile, splitk); zeros after rc when rc != 0"""
    from xmem2_amd import _lib
    pi = _lib.ConvPlanInfo()
    d.plan_tile, d.plan_splitk = tile, splitk
    rc = _lib.load().xmem_conv2d_plan_info(C.byref(d), C.byref(pi))
    return (rc, pi.form, pi.bm, pi.bn, pi.bk, pi.splitk, pi.stream, pi.ring) if rc == 0 else (rc, 0, 0, 0, 0, 0, 0, 0)


def query(layers):
    """What the loaded library answers over the grid: info [layer, operands, mode, tile, splitk, INFO_COLS], workspace bytes
    [layer, operands, mode, tile, splitk] and the dilated workspace bytes [layer, dilation, tile 0..7, splitk]."""
    from xmem2_amd import _lib
    lib = _lib.load()
    info, ws, dws = [], [], []
    for layer in layers:
        for operands in range(len(OPERANDS)):
            for mode in range(len(MODES)):
                d = make_desc(layer, operands, mode)
                for tile in TILES:
                    for sk in SPLITKS:
                        info.append(plan_info(d, tile, sk))
                        ws.append(lib.xmem_conv2d_workspace_bytes(C.byref(d)))
        d = make_desc(layer)
        for dil in DILATIONS:
            for d.plan_tile in DILATED_TILES:
                for d.plan_splitk in SPLITKS:
                    dws.append(lib.xmem_conv2d_dilated_workspace_bytes(C.byref(d), dil))
    shape = (len(layers), len(OPERANDS), len(MODES), len(TILES), len(SPLITKS))
    return (np.array(info, np.int16).reshape(shape + (len(INFO_COLS),)), np.array(ws, np.int64).reshape(shape),
            np.array(dws, np.int64).reshape(len(layers), len(DILATIONS), len(DILATED_TILES), len(SPLITKS)))


def test_plan_resolution_matches_the_recorded_table():
    """Every descriptor of the grid behind tests/golden/conv_plan_info.npz (make_conv_plan_goldens.py: the layers, and the build it
    was recorded from) resolves to the recorded plan and workspace size - the fallback chain of make_plan, the half tiles, the
    split-K rule and the workspace formulas, pinned across restructurings of the host code."""
    g = np.load(GOLDEN)
    layers = g['layers']
    col = {n: layers[:, i] for i, n in enumerate(LAYER_COLS)}
    # the layers the fixture must cover (the plan values, operand sets, modes and dilations are the constants above)
    l3 = (col['K'] == 3) & (col['stride'] == 1) & (col['pad'] == 1)
    assert {(ci, co, e) for ci in (32, 36, 64) for co in (1, 64, 96, 98) for e in (0, 1)} <= \
        set(zip(col['Cin'][l3], col['Cout'][l3], (col['ldout'] - col['Cout'])[l3]))
    assert (l3 & (col['ldres'] % 4 != 0)).any() and (l3 & (col['out_off'] % 16 != 0)).any()
    assert set(zip(col['K'], col['stride'], col['pad'])) >= {(3, 2, 1), (7, 2, 3), (1, 1, 0), (1, 2, 0), (1, 1, 1)}
    assert (col['Cin'][col['K'] == 7] == 4).all()
    tiles128 = -(-(col['B'] * col['H'] * col['W']) // 128) * -(-col['Cout'] // 128)
    assert (l3 & (tiles128 >= 384)).any() and (l3 & (tiles128 < 384)).any()
    info, ws, dws = query(layers)
    assert info.shape == g['info'].shape and ws.shape == g['workspace'].shape and dws.shape == g['dilated_workspace'].shape
    bad = np.argwhere((info != g['info']).any(-1) | (ws != g['workspace']))
    if len(bad):
        l, o, m, t, k = bad[0]
        raise AssertionError(f'{len(bad)} of {ws.size} descriptors differ, first: layer {dict(zip(LAYER_COLS, layers[l]))}, operands '
                             f'{OPERANDS[o]}, {MODES[m]}, plan ({TILES[t]}, {SPLITKS[k]}): {dict(zip(INFO_COLS, info[l, o, m, t, k]))} '
                             f'workspace {ws[l, o, m, t, k]}; recorded {dict(zip(INFO_COLS, g["info"][l, o, m, t, k]))} workspace '
                             f'{g["workspace"][l, o, m, t, k]}')
    bad = np.argwhere(dws != g['dilated_workspace'])
    assert len(bad) == 0, f'dilated workspace differs at (layer, dilation, tile, splitk) indices {bad[0]}'


def test_planner_alone_under_the_sanitizers_matches_the_recorded_table(tmp_path):
    """csrc/conv_plan.hpp is free of HIP: tools/conv_plan_sweep.cpp, built by the host compiler with AddressSanitizer and
    UndefinedBehaviorSanitizer (a stand-alone program), walks the grid of query() over the fixture's layers and must print the
    recorded plan and workspace of every descriptor - among them plan codes -1, 41 and 42, which validate() has to turn away
    before kPlanCodes is indexed.  Any sanitizer report ends the program with a non-zero status."""
    import shutil
    import subprocess
    import pytest
    cxx = next((c for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++') if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'conv_plan_sweep')
    subprocess.run([cxx, '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', 'conv_plan_sweep.cpp'), '-o', exe], check=True)
    g = np.load(GOLDEN)
    assert len(g['layers']) == 34
    rows = '\n'.join(' '.join(str(int(v)) for v in layer) for layer in g['layers']) + '\n'
    run = subprocess.run([exe], input=rows, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.split('\n')[:-1]
    per_layer = g['workspace'][0].size + g['dilated_workspace'][0].size
    assert len(lines) == len(g['layers']) * per_layer
    info, ws, dws = [], [], []
    for line in lines:
        kind, *vals = line.split()
        if kind == 'I':
            info.append(vals[:len(INFO_COLS)])
            ws.append(vals[len(INFO_COLS)])
        else:
            assert kind == 'D'
            dws.append(vals[0])
    assert (np.array(info, np.int64).reshape(g['info'].shape) == g['info']).all()
    assert (np.array(ws, np.int64).reshape(g['workspace'].shape) == g['workspace']).all()
    assert (np.array(dws, np.int64).reshape(g['dilated_workspace'].shape) == g['dilated_workspace']).all()


def _info_of(code, pointwise, half):
    layer = dict(B=2, H=40, W=40, Cin=64, ldin=64, Cout=64, K=1 if pointwise else 3, stride=1, pad=0 if pointwise else 1, ldout=64,
                 ldres=0, out_off=0)
    info = plan_info(make_desc([layer[c] for c in LAYER_COLS], 0, 3 if half else 0), code, 1)
    assert info[0] == 0
    return dict(zip(INFO_COLS, info))


def test_python_codes_agree_with_the_library():
    """conv_plan.CODES / HALF_CODES against xmem_conv2d_plan_info on a layer every code fully applies to (3x3 s1 p1, 64 -> 64, all
    operands; 1x1 p0 for the pointwise streaming codes): form, GEMM tile, k-tile depth and streaming ring."""
    from xmem2_amd import _lib, conv_plan
    assert sorted(conv_plan.CODES) == list(range(0, 41)) and sorted(conv_plan.HALF_CODES) == [1, 2, 3, 4, 5, 6]
    for half, table in ((False, conv_plan.CODES), (True, conv_plan.HALF_CODES)):
        for code in sorted(table)[0 if half else 1:]:               # (code 0 is the heuristic: no tile of its own)
            got = _info_of(code, pointwise=table[code].form == 'direct' and table[code].ring > 0, half=half)
            assert got['stream'] == (got['ring'] > 0)
            assert tuple(table[code]) == (_lib.CONV_FORMS[got['form']], got['bm'], got['bn'], got['bk'], got['ring']), (half, code)
    assert conv_plan.CODES[0] == ('direct', 0, 0, 32, 0) and _info_of(0, False, False)['form'] == _lib.CONV_FORMS.index('direct')


def test_shipped_tables_round_trip(tmp_path):
    """Every key of the three shipped tables resolves through the pure part of `choose` to its tabled plan; an unlisted key takes
    the documented heuristic; dumping an untouched table reproduces the shipped file."""
    from xmem2_amd import conv_plan
    n = 0
    for mode, table in (('fp32', conv_plan.FP32), ('fp32x', conv_plan.FP32X), ('fp16', conv_plan.FP16)):
        shipped = json.load(open(table.path))
        n += len(shipped)
        for key, plan in shipped.items():
            for eligible in (True, False):
                assert conv_plan.tabled_or_heuristic(key, mode, autotune=False, has_winograd=eligible, wino_ok=eligible,
                                                     pixels=1 << 20) == (tuple(plan), True), (mode, key)
        out = tmp_path / f'{mode}.json'
        assert table.dump(str(out)) == len(shipped)
        assert json.load(open(out)) == shipped and open(out).read() == open(table.path).read()
    assert n == 1843
    key = '3x5x7x64/64->64/64 k3s1p1 r000'                                # no shipped table lists it
    for mode in ('fp32', 'fp32x'):
        pure = lambda **kw: conv_plan.tabled_or_heuristic(key, mode, autotune=False, **kw)
        assert pure(has_winograd=True, wino_ok=True, pixels=4096) == ((19, 1), False)
        assert pure(has_winograd=True, wino_ok=True, pixels=4095) == ((9, 1), False)
        assert pure(has_winograd=True, wino_ok=False, pixels=4096) == ((0, 0), False)
        assert pure(has_winograd=False, wino_ok=True, pixels=4096) == ((0, 0), False)
    assert conv_plan.tabled_or_heuristic('h' + key + 'o1', 'fp16', autotune=False, has_winograd=True, wino_ok=True,
                                         pixels=4096) == ((0, 0), False)
    # fp32x inherits the fp32 entry of a shape its own table lacks, except under the tuner (which measures the split kernels)
    only32 = next(k for k in json.load(open(conv_plan.FP32.path)) if k not in json.load(open(conv_plan.FP32X.path)) and not k.startswith('__'))
    want = tuple(json.load(open(conv_plan.FP32.path))[only32])
    assert conv_plan.tabled_or_heuristic(only32, 'fp32x', autotune=False, has_winograd=False, wino_ok=False, pixels=1) == (want, True)
    assert conv_plan.tabled_or_heuristic(only32, 'fp32x', autotune=True, has_winograd=False, wino_ok=False, pixels=1) == ((0, 0), False)
