"""Edge-shape parity of every convolution plan against float64 references (tests/conv_refs.py): maps smaller than one Winograd or
GEMM tile, ragged channel counts, the k tail of the BK-64 codes, rectangular / unpadded / strided kernels, channel slices and
mis-aligned outputs (the Winograd fallbacks), split-K beyond the k-tile count, the GEMV kernels, the dilated entry.

Every case of conv_refs.cases() is launched through the C ABI with a descriptor of its own (plan 16, mis-aligned `out`, workspace
guards and status codes are not expressible through ops.conv2d; the operands are the ones ops.ConvWeights / ops.winograd*_weights /
ops.split_pack make, and test_ops_conv2d_surface runs a slice of the grid through ops.conv2d itself).  Per case:
  - xmem_conv2d_plan_info must report the form, tile, k-tile and ring the header documents for the code (conv_refs.expected_plan);
  - the output buffer is sentinel-filled and nothing outside out[..., off : off + Cout] may change; the input and residual buffers
    hold a finite junk value outside their slices;
  - the workspace is xmem_conv2d_workspace_bytes + 4096 bytes of 0xFF (NaN as floats and as halfs): the tail must be intact;
  - `exact` regime: the result EQUALS the float64 reference (every form but F(4x4)); otherwise |got - ref| <= the a-priori bound
    of conv_refs (err / bound <= 1).
Run with -s for the table (profiles/r09_conv_edge_tests.txt is one run)."""
import collections
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import conv_refs as R

pytestmark = pytest.mark.gpu
SENTINEL = -777.0                 # exactly representable as a half
JUNK = 7.0                        # outside the input / residual slices: finite, so that a stray read shows as a wrong value
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # xmem_status (include/xmem_hip.h)


def show(name, worst, n=None):
    print(f'\nconvedge | {name:<66s} | {"" if n is None else f"{n:4d} cases | "}max err/bound {worst:.3f}')


_weights = {}


def device_weights(c):
    """ops.ConvWeights of the case's layer on the GPU with every operand a plan may read, built once per layer."""
    from xmem2_amd import ops
    half = c.mode.startswith('half')
    key = (c.regime, half, c.cout, c.kh, c.kw, c.cin)
    if key not in _weights:
        w, scale, shift = R.make_weights(*key)
        cw = ops.ConvWeights(w.float().cuda().contiguous(), scale.float().cuda(), shift.float().cuda(), c.stride, c.pad)
        if not half and (c.kh, c.kw) == (3, 3) and c.cin % 32 == 0 and c.cout % 4 == 0:
            if cw.wu is None:                      # the library takes any Cout % 4 == 0; ConvWeights builds the operand from Cout = 32
                cw.wu = ops.winograd_weights(cw.w)
            if c.cin % 64 == 0 and cw.wu_f16 is None:
                cw.wu_f16 = cw.wu.to(torch.float16).contiguous()
            cw.wu4 = ops.winograd4_weights(cw.w)
        if half:
            cw.half()
        else:
            cw.ensure_split()
        _weights[key] = cw
    return _weights[key]


def _strided(t, ld, off, fill, dtype):
    """t [..., C] float64 on the host -> (device buffer [rows, ld] filled with `fill`, with t at columns off : off + C)"""
    rows = t.reshape(-1, t.shape[-1])
    buf = torch.full((rows.shape[0], ld), fill, dtype=dtype)
    buf[:, off:off + rows.shape[1]] = rows.to(dtype)
    return buf.cuda()


Launch = collections.namedtuple('Launch', 'rc got info need case')


def launch(c, lib, plan_splitk=None, ws_bytes=None):
    """One case through the C ABI.  Returns the status, the output slice (float64, None when refused) and the reported plan, after
    checking the sentinels of the output buffer and of the workspace tail."""
    from xmem2_amd import _lib
    i = R.make_inputs(c)
    cw = device_weights(c)
    half, odt = c.mode.startswith('half'), torch.float16 if c.mode == 'half_f16' else torch.float32
    ldin, in_off, ldout, out_off, ldres = R.layout_of(c)
    Ho, Wo = R.out_dims(c)
    rows = c.B * max(Ho, 0) * max(Wo, 0)
    xbuf = _strided(i['x'], ldin, in_off if c.layout == 'sliced' else 0, JUNK, torch.float16 if half else torch.float32)
    obuf = torch.full((out_off + rows * ldout + 8,), SENTINEL, dtype=odt, device='cuda')
    rbuf = _strided(i['res'], ldres, 0, JUNK, odt) if i['res'] is not None else None
    d = _lib.ConvDesc()
    d.inp = xbuf.data_ptr() + (in_off if c.layout == 'sliced' else 0) * xbuf.element_size()
    d.B, d.H, d.W, d.Cin, d.ldin = c.B, c.H, c.W, c.cin, ldin
    d.w, d.Cout, d.KH, d.KW, d.stride, d.pad = cw.w.data_ptr(), c.cout, c.kh, c.kw, c.stride, c.pad
    d.scale, d.shift = cw.scale.data_ptr(), cw.shift.data_ptr()
    if rbuf is not None:
        d.res, d.ldres = rbuf.data_ptr(), ldres
    d.out, d.ldout = obuf.data_ptr() + out_off * obuf.element_size(), ldout
    d.relu_in, d.relu_out, d.res_broadcast = (int(v) for v in R.epilogue_flags(c))
    d.plan_tile, d.plan_splitk = c.code, c.splitk if plan_splitk is None else plan_splitk
    if half:
        d.in_half, d.out_half, d.w_half = 1, int(odt == torch.float16), cw.w_h.data_ptr()
    else:
        for f, t in (('w_winograd', cw.wu), ('w_winograd4', cw.wu4), ('w_winograd_f16', cw.wu_f16)):
            if t is not None:
                setattr(d, f, t.data_ptr())
        if c.mode == 'fp32x' and c.cout > 1:
            d.arith, d.w_split, d.scale = 1, cw.w_sp.data_ptr(), cw.scale_sp.data_ptr()
            if cw.wu_sp is not None:
                d.w_winograd_split, d.w_winograd4_split = cw.wu_sp.data_ptr(), cw.wu4_sp.data_ptr()
    dilated = c.family == 'dilated'
    info = _lib.ConvPlanInfo()
    rc_info = OK if dilated else lib.xmem_conv2d_plan_info(C.byref(d), C.byref(info))
    need = lib.xmem_conv2d_dilated_workspace_bytes(C.byref(d), c.dil) if dilated else lib.xmem_conv2d_workspace_bytes(C.byref(d))
    given = need if ws_bytes is None else ws_bytes
    ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device='cuda')
    if dilated:
        rc = lib.xmem_conv2d_nhwc_dilated(C.byref(d), c.dil, 0 if c.skip else _lib.DILATED_NO_TAP_SKIP, _lib.ptr(ws), given, _lib.stream_ptr())
    else:
        rc = lib.xmem_conv2d_nhwc(C.byref(d), _lib.ptr(ws), given, _lib.stream_ptr())
        assert rc_info == rc or (rc == WORKSPACE and rc_info == OK), (c, rc_info, rc)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a device fault: nothing more may run on this GPU from this process
        pytest.exit(f'GPU fault at {c}: {e}', returncode=3)
    assert bool((ws[given:] == 0xFF).all()), f'{c}: the kernels wrote past the {need} workspace bytes the library asked for'
    flat = obuf.cpu().double()
    body = flat[out_off:out_off + rows * ldout].reshape(rows, ldout)
    if rc != OK:
        assert bool((flat == SENTINEL).all()), f'{c}: a refused call (status {rc}) wrote to the output'
        return Launch(rc, None, None, need, c)
    keep = torch.ones_like(flat, dtype=torch.bool)
    keep[out_off:out_off + rows * ldout].reshape(rows, ldout)[:, :c.cout] = False
    assert bool((flat[keep] == SENTINEL).all()), f'{c}: wrote outside out[..., {out_off} : {out_off} + {c.cout}]'
    got = body[:, :c.cout].reshape(c.B, Ho, Wo, c.cout)
    form = 'direct' if dilated else _lib.CONV_FORMS[info.form]
    return Launch(rc, got, (form, info.bm, info.bn, info.bk, info.stream, info.ring, info.splitk), need, c)


def check(c, lib, fails, forms=None):
    """Launch a case and hold it to its reference; returns err / bound (0 for an exact match), appends a description of every miss
    to `fails` (the grid goes on: one run shows the whole picture)."""
    if R.refused(c):
        r = launch(c, lib)
        if r.rc != BAD_ARG:
            fails.append(f'{c}: status {r.rc}, expected XMEM_ERR_BAD_ARG')
        return 0.0
    r = launch(c, lib)
    if r.rc != OK:
        fails.append(f'{c}: status {r.rc}')
        return 0.0
    plan = R.expected_plan(c)
    if c.family != 'dilated':
        if r.info[:6] != tuple(plan[:6]):
            fails.append(f'{c}: executed {r.info}, expected {plan}')
            return 0.0
        s = R.expected_splitk(c, plan)
        if not (r.info[6] == s if s is not None else 1 <= r.info[6] <= 16):
            fails.append(f'{c}: split-K {r.info[6]}, expected {s}')
        if forms is not None:
            forms[plan.form] += 1
    i = R.make_inputs(c)
    ref, S, T = R.reference(c, i)
    bound = R.bound_of(c, plan, r.info[6] if c.family != 'dilated' else 16, ref, S, T, i)
    if not bool(torch.isfinite(r.got).all()):
        fails.append(f'{c}: non-finite output')
        return float('inf')
    if bound is None:
        R.assert_exact_representable(c, ref)
        bad = int((r.got != ref).sum())
        if bad:
            fails.append(f'{c} [{plan.form} {plan.bm}x{plan.bn}x{plan.bk}]: {bad} of {ref.numel()} elements differ from the exact reference, '
                         f'max |err| {float((r.got - ref).abs().max()):.3g}')
        return 0.0
    ratio = float(((r.got - ref).abs() / bound).max())
    if not ratio <= 1.0:
        fails.append(f'{c} [{plan.form} {plan.bm}x{plan.bn}x{plan.bk}]: err / bound {ratio:.3g}')
    return ratio


def run_group(name, group, lib=None):
    from xmem2_amd import _lib
    lib = lib or _lib.load()
    fails, forms, worst = [], collections.Counter(), 0.0
    for c in group:
        worst = max(worst, check(c, lib, fails, forms))
    show(f'{name} [{" ".join(f"{k}:{v}" for k, v in sorted(forms.items()))}]', worst, len(group))
    assert not fails, f'{len(fails)} of {len(group)} cases failed:\n' + '\n'.join(fails[:12])
    return worst


def family(name, **match):
    return [c for c in R.cases() if c.family == name and all(getattr(c, k) == v for k, v in match.items())]


@pytest.mark.parametrize('kernel', R.KERNELS, ids=lambda k: 'k%dx%ds%dp%d' % k)
@pytest.mark.parametrize('regime', ['exact', 'sparse'])
@pytest.mark.parametrize('mode', R.MODES)
def test_direct_family(mode, regime, kernel):
    """Every map x channel pair under one kernel geometry, codes 0..6, epilogue / layout / split-K rotated: M < bm, Cout < bn, the
    generic k tail, pad 0 and pad 1 on a 1x1, rectangular and 7x7 / stride 2 kernels, inputs smaller than the kernel (refused)."""
    kh, kw, stride, pad = kernel
    run_group(f'direct {mode} {regime} {kh}x{kw}/{stride}/{pad}', family('direct', mode=mode, regime=regime, kh=kh, kw=kw, stride=stride, pad=pad))


@pytest.mark.parametrize('code', range(41))
def test_every_plan_code(code):
    """3x3 / 1 / 1 on every map x the eligible channel pairs under ONE plan code, fp32 and fp32x (codes 35..40 also on the three 1x1
    kernels, plan 16 also at 64 -> 64): the code runs as itself where the header says it applies, as its documented fallback
    elsewhere (unaligned layouts, fp32x without a split variant, Cin % 64 for plan 16, a padded 1x1 on the streaming kernel).
    F(4x4) codes run the sparse regime against their bound, everything else must be exact."""
    run_group(f'plan code {code:2d} ({R.conv_plan.CODES[code].form})', family('plans', code=code))


@pytest.mark.parametrize('code', range(41))
def test_every_plan_code_dense(code):
    """Realistic accumulation (normal activations and weights) under every code: precision class of the executed form."""
    assert run_group(f'plan code {code:2d} dense', family('dense', code=code)) <= 1.0


def test_small_cout_winograd():
    """The library's own contract, Cout % 4 == 0: F(2x2) (classic, streaming, fused) and F(4x4) at Cout = 4 and 36."""
    run_group('Winograd at Cout 4 / 36', family('small_cout'))


@pytest.mark.parametrize('mode', ['fp32', 'half_f32'])
def test_gemv(mode):
    """Cout = 1 on every map and kernel (one Cin of 260: the general channel loop of a 3x3), the row-of-four kernel at M >= 8192, and
    the half-input GEMV with its fp32 output."""
    run_group(f'GEMV {mode}', family('gemv', mode=mode))


@pytest.mark.parametrize('dil', [1, 2, 5])
def test_dilated_entry(dil):
    """Dilation 1 / 2 / 5 on maps up to 7 x 9 (whole taps outside the map), codes 0..6, exact; tap skip on and off give equal bits."""
    from xmem2_amd import _lib
    lib = _lib.load()
    group = family('dilated', dil=dil)
    run_group(f'dilated entry, dilation {dil}', group, lib)
    for on, off in zip(group[0::2], group[1::2]):
        assert on.skip == 1 and off.skip == 0 and on._replace(skip=0) == off
        a, b = launch(on, lib).got, launch(off, lib).got
        assert np.array_equal(a.float().numpy().view(np.int32), b.float().numpy().view(np.int32)), f'{on}: tap skip changes bits'


def _bits(r):
    return r.got.float().numpy().view(np.int32)


@pytest.mark.parametrize('m', R.MAPS, ids=lambda m: '%dx%dx%d' % m)
def test_streaming_codes_keep_the_bits_of_their_classic_tile(m):
    """23..28 equal 19, 29..34 equal 9 (3x3 / 1 / 1, eligible channel pairs), 35..40 equal 3 (the three 1x1 kernels), on dense data,
    with a residual and both relus."""
    from xmem2_amd import _lib
    lib = _lib.load()
    n = 0
    for ch, (base, codes, kernels) in itertools.product(R.CHANNELS_WINO, ((19, range(23, 29), (R.K3,)), (9, range(29, 35), (R.K3,)),
                                                                          (3, range(35, 41), R.KERNELS[:3]))):
        for k in kernels:
            c0 = R.Case('bits', 'fp32', 'dense', *m, *ch, *k, 'relu_res_relu', 'sliced', 0, base)
            r0 = launch(c0, lib)
            assert r0.rc == OK and r0.info[:6] == tuple(R.expected_plan(c0)[:6])
            for code in codes:
                c = c0._replace(code=code)
                r = launch(c, lib)
                assert r.rc == OK and r.info[:6] == tuple(R.expected_plan(c)[:6]), (c, r.info)
                assert np.array_equal(_bits(r), _bits(r0)), f'{c}: bits differ from code {base}'
                n += 1
    show(f'bit identity of the streaming codes on {m}', 0.0, n)


def test_ops_conv2d_surface():
    """A slice of the grid through ops.conv2d itself (explicit plan, channel slices in and out, residuals): 3x3 / 1 / 1 of the direct
    family, fp32 and both half modes, exact - the result equals the float64 reference and nothing else in the output buffer changes."""
    from xmem2_amd import ops
    n = 0
    for c in family('direct', regime='exact', kh=3, kw=3, stride=1, pad=1):
        if c.mode == 'fp32x' or c.layout == 'unaligned':
            continue
        i, cw = R.make_inputs(c), device_weights(c)
        cw.stride, cw.pad = c.stride, c.pad                   # (the layer's weights are shared with the other 3x3 geometries)
        half, odt = c.mode.startswith('half'), torch.float16 if c.mode == 'half_f16' else torch.float32
        ldin, in_off, ldout, out_off, ldres = R.layout_of(c)
        off = in_off if c.layout == 'sliced' else 0
        xbuf = _strided(i['x'], ldin, off, JUNK, torch.float16 if half else torch.float32).reshape(c.B, c.H, c.W, ldin)
        obuf = torch.full((c.B, c.H, c.W, ldout), SENTINEL, dtype=odt, device='cuda')
        res = None
        if i['res'] is not None:
            res = _strided(i['res'], ldres, 0, JUNK, odt).reshape(*i['res'].shape[:3], ldres)
        relu_in, relu_out, bcast = R.epilogue_flags(c)
        ops.conv2d(xbuf[..., off:off + c.cin], cw, out=obuf[..., out_off:], out_ld=ldout, res=res, relu_in=relu_in, relu_out=relu_out,
                   in_ld=ldin, cin=c.cin, plan=(c.code, c.splitk), res_broadcast=bcast, out_dtype=odt)
        torch.cuda.synchronize()
        got = obuf.cpu().double()
        ref = R.reference(c, i)[0]
        assert bool((got[..., out_off:out_off + c.cout] == ref).all()), c
        rest = torch.ones(ldout, dtype=torch.bool)
        rest[out_off:out_off + c.cout] = False
        assert bool((got[..., rest] == SENTINEL).all()), c
        n += 1
    show('ops.conv2d, 3x3 / 1 / 1 exact, dense and sliced', 0.0, n)


def test_half_slices_are_validated():
    """ops._conv2d_half refuses a channel slice that is not a whole number of 8-half groups, and one that crosses its pixel stride:
    the kernel would read the neighbouring slice or the next pixel against zero weights (0 x Inf = NaN)."""
    from xmem2_amd import ops
    cw = ops.ConvWeights(torch.ones(4, 1, 1, 12, device='cuda'), torch.ones(4, device='cuda'), torch.zeros(4, device='cuda'), 1, 0)
    buf = torch.zeros(1, 2, 2, 24, dtype=torch.float16, device='cuda')
    with pytest.raises(RuntimeError, match='multiple of 8'):
        ops.conv2d(buf[..., :12], cw, in_ld=24, cin=12)
    with pytest.raises(RuntimeError, match='crosses the pixel stride'):
        ops.conv2d(buf[..., 12:], cw, in_ld=24, cin=16)
    cw8 = ops.ConvWeights(torch.ones(4, 1, 1, 8, device='cuda'), torch.ones(4, device='cuda'), torch.zeros(4, device='cuda'), 1, 0)
    out = ops.conv2d(buf[..., 16:], cw8, in_ld=24, cin=8)                    # the valid twin: a whole group that ends with its pixel
    assert out.shape == (1, 2, 2, 4) and bool((out == 0).all())


def test_status_codes_and_workspace_guard():
    """Refusals launch nothing (the output keeps its sentinel): a workspace one byte short of the reported need (split-K, F(2x2),
    F(4x4), plan 16), a plan code of 41, a negative split-K; the valid twins are served."""
    from xmem2_amd import _lib
    lib = _lib.load()
    base = R.Case('status', 'fp32', 'exact', 2, 6, 10, 64, 132, *R.K3, 'relu_res_relu', 'dense', 3, 3)
    for code in (3, 9, 16, 19, 23):
        c = base._replace(code=code)
        r = launch(c, lib)
        assert r.rc == OK and r.need > 0, (code, r.rc, r.need)
        short = launch(c, lib, ws_bytes=r.need - 1)
        assert short.rc == WORKSPACE, (code, short.rc)
    assert launch(base._replace(code=41), lib).rc == BAD_ARG
    assert launch(base, lib, plan_splitk=-1).rc == BAD_ARG
    assert launch(base._replace(H=1, W=1, kh=5, kw=5, pad=1), lib).rc == BAD_ARG          # H + 2 pad < KH
