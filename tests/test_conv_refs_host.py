"""Host tests (no GPU) of tests/conv_refs.py: the float64 convolution reference against a literal loop, the Winograd matrices, the
bounds against fp32 arithmetic on the CPU, the case table of tests/test_gpu_conv_edges.py (pairwise coverage, the plans the library
resolves the cases to) and the SENSITIVITY of the bounds: what a subtly wrong kernel would return must fall outside them."""
import collections
import ctypes as C
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import conv_refs as R

_PTR = 0x10000


def loop_conv(x, w, scale, shift, res, stride, pad, relu_in, relu_out, res_broadcast, dilation=1):
    """The header's formula, one loop per index."""
    B, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    Ho = (H + 2 * pad - dilation * (KH - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dilation * (KW - 1) - 1) // stride + 1
    out = np.zeros((B, Ho, Wo, Cout))
    for b in range(B):
        for oh in range(Ho):
            for ow in range(Wo):
                for n in range(Cout):
                    acc = 0.0
                    for kh in range(KH):
                        for kw in range(KW):
                            ih, iw = oh * stride - pad + kh * dilation, ow * stride - pad + kw * dilation
                            if not (0 <= ih < H and 0 <= iw < W):
                                continue
                            for c in range(Cin):
                                v = x[b, ih, iw, c]
                                acc += (max(v, 0.0) if relu_in else v) * w[n, kh, kw, c]
                    v = acc * scale[n] + shift[n]
                    if res is not None:
                        v += res[0 if res_broadcast else b, oh, ow, n]
                    out[b, oh, ow, n] = max(v, 0.0) if relu_out else v
    return out


def test_conv_ref_equals_a_literal_loop():
    """Three tiny shapes: stride 2 / pad 0, a rectangular kernel with the broadcast residual, a dilated 3x3 with relu on both ends."""
    g = torch.Generator().manual_seed(5)
    for (B, H, W, Cin, Cout, KH, KW, s, p, d, relu_in, relu_out, res, bc) in (
            (2, 5, 6, 3, 4, 3, 3, 2, 0, 1, False, False, False, False),
            (2, 3, 5, 4, 3, 1, 3, 1, 1, 1, False, True, True, True),
            (2, 6, 5, 2, 3, 3, 3, 1, 2, 2, True, True, True, False)):
        x, w = torch.randn(B, H, W, Cin, generator=g).double(), torch.randn(Cout, KH, KW, Cin, generator=g).double()
        scale, shift = torch.randn(Cout, generator=g).double(), torch.randn(Cout, generator=g).double()
        Ho, Wo = (H + 2 * p - d * (KH - 1) - 1) // s + 1, (W + 2 * p - d * (KW - 1) - 1) // s + 1
        r = torch.randn(1 if bc else B, Ho, Wo, Cout, generator=g).double() if res else None
        ref, S, T = R.conv_ref(x, w, scale, shift, r, s, p, relu_in, relu_out, bc, d)
        lit = loop_conv(x.numpy(), w.numpy(), scale.numpy(), shift.numpy(), None if r is None else r.numpy(), s, p, relu_in, relu_out, bc, d)
        assert ref.shape == lit.shape and np.abs(ref.numpy() - lit).max() < 1e-12
        xa = (x.clamp(min=0) if relu_in else x).abs()
        Sl = loop_conv(xa.numpy(), w.abs().numpy(), np.ones(Cout), np.zeros(Cout), None, s, p, False, False, False, d)
        assert np.abs(S.numpy() - Sl).max() < 1e-12
        Tl = np.abs(scale.numpy()) * Sl + np.abs(shift.numpy()) + (0 if r is None else np.abs(r.numpy()))
        assert np.abs(T.numpy() - Tl).max() < 1e-12


def test_winograd_matrices_reproduce_the_convolution():
    """(G, B^T, A^T) as conv_refs derives them (B^T solved, entries asserted dyadic there) against the float64 convolution, on a map
    with partial tiles in both directions; and |.| of the same form dominates it."""
    g = torch.Generator().manual_seed(6)
    x, w = torch.randn(2, 7, 9, 5, generator=g).double(), torch.randn(6, 3, 3, 5, generator=g).double()
    for r in (2, 4):
        G, BT, AT = R.wino_matrices(r)
        assert BT.shape == (r + 2, r + 2) and AT.shape == (r, r + 2)
        y = R.wino_conv(x, w, r)
        assert float((y - R.conv_sum(x, w, 1, 1)).abs().max()) < 1e-12
        assert bool((R.wino_abs(x, w, r) >= y.abs() - 1e-12).all())
    assert np.abs(R.wino_matrices(2)[1]).max() == 1.0 and np.abs(R.wino_matrices(2)[2]).max() == 1.0      # F(2x2): +-1 only


def test_case_table_covers_every_pair_of_axis_values():
    """Every pair of values of any two axes occurs at least once: in the direct family over (kernel, map, channels, code, epilogue,
    layout, split-K) per mode, in the plan family over (code, map, channels, mode, epilogue, layout, split-K)."""
    cs = R.cases()
    axes = dict(kernel=lambda c: (c.kh, c.kw, c.stride, c.pad), map=lambda c: (c.B, c.H, c.W), ch=lambda c: (c.cin, c.cout),
                code=lambda c: c.code, epi=lambda c: c.epi, layout=lambda c: c.layout, splitk=lambda c: c.splitk, mode=lambda c: c.mode,
                regime=lambda c: c.regime)
    values = dict(kernel=R.KERNELS, map=R.MAPS, epi=R.EPILOGUES, layout=R.LAYOUTS, splitk=R.SPLITKS)

    def check(sub, names, **vals):
        v = dict(values, **vals)
        for a, b in itertools.combinations(names, 2):
            seen = {(axes[a](c), axes[b](c)) for c in sub}
            missing = [p for p in itertools.product(v[a], v[b]) if p not in seen]
            assert not missing, (a, b, missing[:5], len(missing))

    for mode in R.MODES:
        ch = R.CHANNELS_HALF if mode.startswith('half') else R.CHANNELS
        check([c for c in cs if c.family == 'direct' and c.mode == mode], ('kernel', 'map', 'ch', 'code', 'epi', 'layout', 'splitk', 'regime'),
              ch=ch, code=range(7), regime=('exact', 'sparse'))
    check([c for c in cs if c.family == 'plans' and (c.kh, c.kw) == (3, 3) and (c.cin, c.cout) != (64, 64)], ('code', 'map', 'ch', 'mode', 'epi', 'layout', 'splitk'),
          code=range(41), ch=R.CHANNELS_WINO, mode=('fp32', 'fp32x'))
    check([c for c in cs if c.family == 'dense'], ('code', 'map', 'ch', 'mode', 'epi', 'layout'), code=range(41), ch=R.CHANNELS_WINO,
          mode=('fp32', 'fp32x'), map=R.DENSE_MAPS)
    check([c for c in cs if c.family == 'dilated'], ('code', 'map', 'layout', 'splitk'), code=range(7), map=R.MAPS[:8])
    dil = [c for c in cs if c.family == 'dilated']
    assert {(c.dil, c.skip, c.code) for c in dil} == set(itertools.product((1, 2, 5), (0, 1), range(7)))
    g = [c for c in cs if c.family == 'gemv']
    assert {((c.kh, c.kw, c.stride, c.pad), (c.B, c.H, c.W)) for c in g if c.mode == 'fp32'} >= set(itertools.product(R.KERNELS, R.MAPS))
    assert any(c.cin > 256 and c.kh == 3 for c in g) and any(c.B * c.H * c.W >= 8192 and c.cin <= 256 for c in g)
    assert sum(R.refused(c) for c in cs) > 0                      # inputs smaller than the kernel are in the table: they must be refused


def make_desc(c, plan_splitk=None):
    """The descriptor of a case with dummy operand pointers of the alignment the layout gives (nothing is dereferenced)."""
    from xmem2_amd._lib import ConvDesc
    ldin, in_off, ldout, out_off, ldres = R.layout_of(c)
    half, esz = c.mode.startswith('half'), 2 if c.mode == 'half_f16' else 4
    d = ConvDesc()
    d.inp, d.w, d.scale, d.shift = _PTR, _PTR, _PTR, _PTR
    d.B, d.H, d.W, d.Cin, d.ldin = c.B, c.H, c.W, c.cin, ldin
    d.Cout, d.KH, d.KW, d.stride, d.pad = c.cout, c.kh, c.kw, c.stride, c.pad
    d.out, d.ldout = _PTR + out_off * esz, ldout
    if R.has_res(c):
        d.res, d.ldres = _PTR, ldres
    d.relu_in, d.relu_out, d.res_broadcast = (int(v) for v in R.epilogue_flags(c))
    d.plan_tile, d.plan_splitk = c.code, c.splitk if plan_splitk is None else plan_splitk
    if half:
        d.in_half, d.out_half, d.w_half = 1, int(c.mode == 'half_f16'), _PTR
    elif (c.kh, c.kw, c.stride, c.pad) == R.K3 and c.cin % 32 == 0 and c.cout % 4 == 0 and c.family != 'dilated':
        d.w_winograd = d.w_winograd4 = _PTR
        if c.cin % 64 == 0:
            d.w_winograd_f16 = _PTR
    if c.mode == 'fp32x':
        d.arith, d.w_split = 1, _PTR
        if d.w_winograd:
            d.w_winograd_split = d.w_winograd4_split = _PTR
    return d


def test_the_library_resolves_every_case_to_the_documented_plan():
    """xmem_conv2d_plan_info (host only) on every case: the form, tile, k-tile and ring that include/xmem_hip.h documents for the code
    and its fallbacks (conv_refs.expected_plan), the split-K clamp, XMEM_ERR_BAD_ARG for an input smaller than the kernel; and each of
    the 41 codes is executed AS ITSELF by at least one fp32 case, each code that has a split-operand form by an fp32x case."""
    from xmem2_amd import _lib
    lib = _lib.load()
    as_itself = collections.defaultdict(set)
    for c in R.cases():
        if c.family == 'dilated':
            continue
        d, pi = make_desc(c), _lib.ConvPlanInfo()
        rc = lib.xmem_conv2d_plan_info(C.byref(d), C.byref(pi))
        if R.refused(c):
            assert rc == -1, (c, rc)
            continue
        assert rc == 0, (c, rc)
        e = R.expected_plan(c)
        got = (_lib.CONV_FORMS[pi.form], pi.bm, pi.bn, pi.bk, pi.stream, pi.ring)
        assert got == tuple(e[:6]), (c, got, e)
        s = R.expected_splitk(c, e)
        assert pi.splitk == s if s is not None else 1 <= pi.splitk <= 16, (c, pi.splitk, s)
        if e.code == c.code and c.cout > 1:
            as_itself[c.mode].add(c.code)
    assert as_itself['fp32'] == set(range(41))
    assert as_itself['fp32x'] == set(range(13)) | set(range(17, 23))
    assert as_itself['half_f32'] == as_itself['half_f16'] == set(range(7))


def _ratio(err, bound):
    return float((err / bound).max())


def test_fp32_arithmetic_on_the_cpu_stays_inside_the_bounds(capsys):
    """The reference alone must satisfy its own bounds: torch's fp32 conv2d inside the direct bound on every problem of the direct
    family (fp32 and half-rounded operands; exact cases must come out equal), a numpy fp32 emulation of the F(2x2) and F(4x4) pipelines
    inside the Winograd bounds on every map x eligible channel pair, sparse and dense."""
    worst = collections.defaultdict(float)
    seen = set()
    for c in R.cases():
        key = (c.regime, c.mode.startswith('half'), c.B, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.stride, c.pad, c.epi)
        if c.family != 'direct' or c.mode in ('fp32x', 'half_f16') or R.refused(c) or key in seen:
            continue
        seen.add(key)
        i = R.make_inputs(c)
        ref, S, T = R.reference(c, i)
        relu_in, relu_out, bcast = R.epilogue_flags(c)
        x = i['x'].float().clamp(min=0) if relu_in else i['x'].float()
        y = F.conv2d(x.permute(0, 3, 1, 2), i['w'].float().permute(0, 3, 1, 2), stride=c.stride, padding=c.pad).permute(0, 2, 3, 1)
        y = y * i['scale'].float() + i['shift'].float()
        if i['res'] is not None:
            y = y + i['res'].float()
        y = (y.clamp(min=0) if relu_out else y).double()
        if c.regime == 'exact':
            R.assert_exact_representable(c, ref)
            assert bool((y == ref).all()), c
        else:
            b = R.bound_direct(T, S, i['scale'], c.kh * c.kw * c.cin, 32, 1)
            worst['direct ' + c.regime] = max(worst['direct ' + c.regime], _ratio((y - ref).abs(), b))
    for regime, m, ch, r in itertools.product(('sparse', 'dense'), R.MAPS, R.CHANNELS_WINO, (2, 4)):
        c = R.Case('plans', 'fp32', regime, *m, *ch, *R.K3, 'relu_res_relu', 'dense', 0, 9 if r == 2 else 19)
        i = R.make_inputs(c)
        ref, S, T = R.reference(c, i)
        y = R.wino_emulate_fp32(i['x'].clamp(min=0), i['w'], r).float()
        y = ((y * i['scale'].float() + i['shift'].float() + i['res'].float()).clamp(min=0)).double()
        b = R.bound_of(c, R.expected_plan(c), 1, ref, S, T, i)
        worst[f'F({r}x{r}) {regime}'] = max(worst[f'F({r}x{r}) {regime}'], _ratio((y - ref).abs(), b))
    with capsys.disabled():
        for k, v in sorted(worst.items()):
            print(f'\nconv refs | fp32 on the CPU, {k:<16s} | max err/bound {v:.2e}', end='')
        print()
    assert len(worst) == 5 and all(v <= 1.0 for v in worst.values()), dict(worst)


# ---------------------------------------------------------------------------------------------------------
# sensitivity: what a subtly wrong kernel would compute
# ---------------------------------------------------------------------------------------------------------
MUTATIONS = ('drop_last_tap', 'ignore_last_channel', 'replicate_right_border', 'residual_of_image_0', 'scale_of_channel_before',
             'shift_of_channel_before', 'skip_relu_in_at_one_pixel')


def has_feature(c, m):
    """Does the case have what the mutation corrupts?  A broadcast or absent residual has no per-image rows to mix up, a case without
    relu_in no relu to skip, pad 0 no border, one output channel no neighbour."""
    return {'residual_of_image_0': c.epi == 'relu_res_relu' and c.B > 1, 'skip_relu_in_at_one_pixel': c.epi == 'relu_res_relu',
            'replicate_right_border': c.pad > 0, 'scale_of_channel_before': c.cout > 1, 'shift_of_channel_before': c.cout > 1}.get(m, True)


def mutate(c, i, m):
    """The output of the case under mutation `m`, float64; None where the mutation cannot apply to the data."""
    relu_in, relu_out, bcast = R.epilogue_flags(c)
    x = i['x'].clamp(min=0) if relu_in else i['x']
    conv = R.conv_parts(c)[0]
    scale, shift, res = i['scale'], i['shift'], i['res']
    B, Ho, Wo, n = conv.shape
    if m == 'drop_last_tap':             # the last in-range tap of the last output pixel of the last image, last channel; where that pixel reads
        ref = R.finish(conv, scale, shift, res, relu_out, bcast)                  # padding or zeros only, or relu_out hides it, the pixel before it
        for oh, ow in itertools.product(reversed(range(Ho)), reversed(range(Wo))):
            pix = [(kh, kw, oh * c.stride - c.pad + kh * c.dil, ow * c.stride - c.pad + kw * c.dil) for kh in range(c.kh) for kw in range(c.kw)]
            pix = [t for t in pix if 0 <= t[2] < c.H and 0 <= t[3] < c.W and bool(x[B - 1, t[2], t[3]].any())]
            if not pix:
                continue
            kh, kw, ih, iw = pix[-1]
            mut = conv.clone()
            mut[B - 1, oh, ow, n - 1] -= x[B - 1, ih, iw] @ i['w'][n - 1, kh, kw]
            mut = R.finish(mut, scale, shift, res, relu_out, bcast)
            if not bool((mut == ref).all()):
                return mut
        return None
    elif m == 'ignore_last_channel':
        conv = conv - R.conv_sum(x[..., -1:], i['w'][..., -1:], c.stride, c.pad, c.dil)
    elif m == 'replicate_right_border':  # the pad columns right of the map hold the last column instead of zeros
        xp = torch.zeros(B, c.H + 2 * c.pad, c.W + 2 * c.pad, c.cin).double()
        xp[:, c.pad:c.pad + c.H, c.pad + c.W:] = x[:, :, -1:]
        conv = conv + R.conv_sum(xp, i['w'], c.stride, 0, c.dil)
    elif m == 'residual_of_image_0':
        res = res.clone()
        res[B - 1] = res[0]
    elif m == 'scale_of_channel_before':
        scale = scale.clone()
        scale[n - 1] = scale[n - 2]
    elif m == 'shift_of_channel_before':
        shift = shift.clone()
        shift[n - 1] = shift[n - 2]
    elif m == 'skip_relu_in_at_one_pixel':   # the last pixel that holds a negative value keeps it
        neg = (i['x'] < 0).any(-1).flatten().nonzero()
        if not len(neg):
            return None
        xm = torch.zeros_like(x).reshape(-1, c.cin)
        xm[neg[-1]] = i['x'].reshape(-1, c.cin)[neg[-1]].clamp(max=0)
        conv = conv + R.conv_sum(xm.reshape(x.shape), i['w'], c.stride, c.pad, c.dil)
    return R.finish(conv, scale, shift, res, relu_out, bcast)


def test_a_subtly_wrong_kernel_falls_outside_the_bounds(capsys):
    """For every sparse GPU case each mutation must push an element past the case's bound; on exact cases it must change the result.
    A (case, mutation) pair is SKIPPED where the case has the feature but the data cannot show the mutation (the mutated output is
    identical: every candidate tap reads zeros, a relu_out clips the change); pairs of a case WITHOUT the feature (has_feature: B = 1
    or no per-image residual, no relu_in, pad 0, Cout = 1) are not pairs at all - with the axes of the grid they alone are a quarter of
    all combinations.  At most 5 % of the pairs may be skipped.  A mutation that stays under an F(4x4) bound is allowed only if the
    same problem also runs under an exact-regime F(2x2) / direct case, where any change is a failure."""
    cs = [c for c in R.cases() if c.regime in ('sparse', 'exact') and not R.refused(c)]
    exact_twins = {(c.B, c.H, c.W, c.cin, c.cout) for c in cs
                   if c.regime == 'exact' and (c.kh, c.kw, c.stride, c.pad) == R.K3 and R.expected_plan(c).form != 'f4'}
    pairs = skipped = without = f4_under = 0
    memo = {}
    for c in cs:
        plan = R.expected_plan(c)
        s = R.expected_splitk(c, plan) or 16
        i = R.make_inputs(c)
        ref, S, T = R.reference(c, i)
        bound = R.bound_of(c, plan, s, ref, S, T, i)
        for m in MUTATIONS:
            if not has_feature(c, m):
                without += 1
                continue
            pairs += 1
            key = (c.regime, c.mode.startswith('half'), R._nnz(c), c.B, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.stride, c.pad, c.dil, c.epi, m)
            if key not in memo:
                mut = mutate(c, i, m)
                memo[key] = None if mut is None or bool((mut == ref).all()) else (mut - ref).abs()
            diff = memo[key]
            if diff is None:
                skipped += 1
            elif bound is None:
                pass                                         # exact regime: unequal is enough, and diff is not None says so
            elif not bool((diff > bound).any()):
                assert plan.form == 'f4', (c, m, _ratio(diff, bound))
                assert (c.B, c.H, c.W, c.cin, c.cout) in exact_twins, (c, m)
                f4_under += 1
    share = skipped / pairs
    with capsys.disabled():
        print(f'\nconv refs | sensitivity: {pairs} (case, mutation) pairs, {skipped} skipped ({100 * share:.2f} %), {f4_under} under an F(4x4) bound '
              f'with an exact twin; {without} combinations of a case without the feature ({100 * (skipped + without) / (pairs + without):.1f} % of all '
              'combinations cannot show a mutation)')
    assert share <= 0.05
