"""tests/elementwise_refs.py on the CPU: (a) every float64 reference agrees with the oracle / torch in fp32 on the GPU test's own
inputs - equal where the operation is exact, and the FP32 ORACLE ITSELF INSIDE THE BOUND where it has one (a bound the reference
implementation cannot meet is wrong); (b) sensitivity: what a subtly wrong kernel would compute falls outside the bound (exact
operations: differs) on those same inputs."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

import elementwise_refs as R
from oracle import cpu_ref

torch.set_grad_enabled(False)
nchw = lambda t: t.permute(0, 3, 1, 2)
nhwc = lambda t: t.permute(0, 2, 3, 1)


def _refnet(w):
    net = object.__new__(cpu_ref.RefNet)
    net.sd = {'a.ChannelGate.mlp.1.weight': w['w1'], 'a.ChannelGate.mlp.1.bias': w['b1'], 'a.ChannelGate.mlp.3.weight': w['w2'],
              'a.ChannelGate.mlp.3.bias': w['b2'], 'a.SpatialGate.spatial.conv.weight': w['sw'][None], 'a.SpatialGate.spatial.conv.bias': w['sb']}
    return net


def oracle32(c, i):
    """The case in fp32 through the oracle / torch, in the reference's logical shape."""
    op = c['op']
    if op == 'maxpool':
        return nhwc(F.max_pool2d(nchw(i['x']), 3, 2, 1))
    if op == 'upsample2x_add':
        return nhwc(F.interpolate(nchw(i['g']), scale_factor=2, mode='bilinear', align_corners=False)) + i['skip']
    if op == 'area_downsample':
        return nhwc(F.interpolate(nchw(i['x']), scale_factor=1 / c['r'], mode='area'))
    if op == 'copy_channels':
        return i['src'][torch.arange(c['B']) % c['srcB']]
    if op == 'hidden_update_gather':
        area = lambda t, r: nhwc(cpu_ref.RefNet._interp_groups(nchw(t)[None], 1 / r, 'area', None)[0])
        return torch.cat([i['g16'], area(i['g8'], 2), area(i['g4'], 4), area(i['logits'][..., None], 4)], -1)
    if op == 'cbam_residual':
        x = nchw(i['g'])
        return nhwc(x + _refnet(i)._cbam(x, 'a'))
    if op == 'gru_gate':
        v, h, hd = i['values'], i['h'], c['Ch']
        forget, update, new_value = torch.sigmoid(v[:, :hd]), torch.sigmoid(v[:, hd:hd * 2]), torch.tanh(v[:, hd * 2:])
        return forget * h * (1 - update) + update * new_value
    if op == 'logits_to_prob':
        lg = F.interpolate(i['logits'][None], scale_factor=4, mode='bilinear', align_corners=False)[0]
        prob = cpu_ref.aggregate(torch.sigmoid(lg), dim=0)
        return prob[:, c['lh']:c['lh'] + c['H'], c['lw']:c['lw'] + c['W']]
    if op == 'aggregate_masks':
        return cpu_ref.aggregate(i['masks'], dim=0).reshape(c['K'] + 1, -1)
    if op == 'resize_bilinear':
        return F.interpolate(i['x'][:, None], (c['Ho'], c['Wo']), mode='bilinear', align_corners=False)[:, 0]
    if op == 'merge_masks':                       # inference_core.py:117-127
        pred, mask = i['pred'].clone(), i['mask']
        pred[:, mask.sum(0) > 0.5] = 0
        for k in range(c['K']):
            if (c['valid_bits'] >> k) & 1:
                pred[k] = mask[k]
        return pred
    if op == 'argmax_u8':
        return torch.argmax(i['prob'], 0)
    raise KeyError(op)


def fp32_cases(op):
    """The cases of `op` with fp32 storage (half storage repeats the arithmetic on rounded inputs)."""
    return [c for c in R.CASES[op]() if not (c.get('in_half') or c.get('out_half') or c.get('half') or c.get('inplace'))]


def test_fp32_oracle_agrees_and_stays_inside_the_bounds(capsys):
    worst = {}
    for op in R.CASES:
        w = 0.0
        for c in fp32_cases(op):
            i = R.make_inputs(c)
            ref, bound = R.reference(c, i)
            got = oracle32(c, i).double()
            assert got.shape == ref.shape, (R.tag(c), got.shape, ref.shape)
            if bound is None:
                assert bool((got == ref.double()).all()), R.tag(c)
            else:
                assert bool(torch.isfinite(got).all()) and bool((bound >= 0).all()), R.tag(c)
                err = (got - ref).abs()
                w = max(w, float((err / bound.clamp(min=1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0)
                if op in ('logits_to_prob', 'aggregate_masks'):
                    assert float((got.sum(0) - 1).abs().max()) <= 4 * R.sum_to_one_bound(c['K']), R.tag(c)   # torch's softmax sums in its own order
        worst[op] = w
    with capsys.disabled():
        for op, w in worst.items():
            print(f'\nelementwise refs | fp32 oracle on the CPU, {op:<22s} | ' + ('equal' if w == 0.0 and op in EXACT else f'max err/bound {w:.3f}'), end='')
        print()
    assert all(w <= 1.0 for w in worst.values()), worst
    assert all(worst[op] > 0.0 for op in worst if op not in EXACT), worst        # a bounded operation whose fp32 oracle shows no error at all would be a wrong test


EXACT = ('maxpool', 'copy_channels', 'merge_masks', 'argmax_u8')


def test_small_exact_references():
    """pack_image, pack_value_input, key_post, add3, the sum-to-one statement and the bilinear index against torch."""
    g = R.rng_of('small')
    img = R.randn(g, 3, 5, 6)
    for Hp, Wp, lh, lw in ((5, 6, 0, 0), (16, 16, 11, 10), (16, 16, 0, 0)):
        want = F.pad(img, (lw, Wp - 6 - lw, lh, Hp - 5 - lh))
        got, _ = R.pack_image_ref(img, Hp, Wp, lh, lw)
        assert bool((got[..., :3] == want.permute(1, 2, 0).double()).all()) and bool((got[..., 3] == 0).all())
    for K in (1, 12):
        masks = (torch.rand(K, 4, 4, generator=g) < 0.4).float()
        im4 = R.randn(g, 4, 4, 4)
        got, _ = R.pack_value_input_ref(im4, masks)
        others = torch.stack([masks.sum(0) - masks[k] for k in range(K)])             # model/network.py:73-81
        assert bool((got[..., 4] == others.double()).all()) and bool((got[..., 3] == masks.double()).all())
        assert bool((got[..., :3] == im4[None, ..., :3].double()).all()) and bool((got[..., 5:] == 0).all())
    proj = R.randn(g, 37, 2 * 64 + 1)
    proj[0, 64:70] = torch.tensor([100.0, -100.0, 100.0, 30.0, -30.0, 0.0])
    (key, _), (shr, bs), (sel, be) = R.key_post_ref(proj, 64)
    assert bool((key == proj[:, :64].double()).all())
    assert bool(((proj[:, 64] ** 2 + 1).double() - shr).abs().le(bs).all())
    assert bool((torch.sigmoid(proj[:, 65:]).double() - sel).abs().le(be).all())
    a, b, c = (R.randn(g, 257) for _ in range(3))
    ref, bound = R.add3_ref(a, b, c)
    assert bool(((a + b + c).double() - ref).abs().le(bound).all())
    for n_in, n_out in ((1, 3), (5, 1), (9, 20), (7, 5), (6, 13), (272, 1088)):       # the fp32 index against ATen's own choice of taps
        i0, i1, l1, dl = R.bilinear_index(n_out, n_in)
        ramp = torch.arange(n_in, dtype=torch.float32)[None, None, :, None]
        want = F.interpolate(ramp, (n_out, 1), mode='bilinear', align_corners=False).flatten().double()
        got = (1 - l1) * i0 + l1 * i1
        assert bool(((got - want).abs() <= dl + 2 * R.U * want.abs()).all())


def test_vector_entries_refuse_a_misaligned_pointer_on_the_host():
    """xmem_maxpool3x3s2_t, xmem_upsample2x_add_t and xmem_cbam_residual_t move 16-byte vectors (8 bytes for halfs).  A pointer off
    that alignment, a channel count off the vector and a workspace one byte short are refused before anything is launched, so the
    status codes can be read without a device (the addresses below are never dereferenced)."""
    import ctypes as C
    from xmem2_amd import _lib
    lib = _lib.load()
    p = C.c_void_p
    UNSUPPORTED, WORKSPACE = _lib.UNSUPPORTED, _lib.CONSTANTS['XMEM_ERR_WORKSPACE']
    a, b, d, w = 0x10000, 0x20000, 0x30000, p(0x40000)
    for half, skew in ((0, 4), (0, 8), (1, 2), (1, 4)):
        assert lib.xmem_maxpool3x3s2_t(p(a + skew), half, p(b), half, 1, 2, 2, 8, None) == UNSUPPORTED
        assert lib.xmem_maxpool3x3s2_t(p(a), half, p(b + skew), half, 1, 2, 2, 8, None) == UNSUPPORTED
        for g, s, o in ((a + skew, b, d), (a, b + skew, d), (a, b, d + skew)):
            assert lib.xmem_upsample2x_add_t(p(g), p(s), p(o), half, 1, 1, 1, 8, None) == UNSUPPORTED
        for g, o in ((a + skew, b), (a, b + skew)):
            assert lib.xmem_cbam_residual_t(p(g), p(o), half, 1, 1, 1, 16, w, w, w, w, w, w, p(d), 1 << 20, None) == UNSUPPORTED
    assert lib.xmem_maxpool3x3s2_t(p(a), 0, p(b), 0, 1, 2, 2, 6, None) == UNSUPPORTED                         # C % 4
    assert lib.xmem_upsample2x_add_t(p(a), p(b), p(d), 0, 1, 1, 1, 6, None) == UNSUPPORTED                    # C % 4
    assert lib.xmem_cbam_residual_t(p(a), p(b), 0, 1, 1, 1, 24, w, w, w, w, w, w, p(d), 1 << 20, None) == UNSUPPORTED        # C % 16
    assert lib.xmem_cbam_residual_t(p(a), p(b), 0, 1, 1, 1, 16, w, w, w, w, w, w, p(d), lib.xmem_cbam_workspace_bytes(1, 1, 16) - 1, None) == WORKSPACE
    assert lib.xmem_area_downsample_t(p(a), 0, 3, p(b), 0, 3, 1, 5, 4, 3, 2, None) == UNSUPPORTED             # H % r


# ---------------------------------------------------------------------------------------------------------
# sensitivity: what a subtly wrong kernel would compute
# ---------------------------------------------------------------------------------------------------------
_clamped = lambda c: c['data'] in ('hard', 'overlap', 'saturated', 'mixed')
MUTATIONS = {          # op -> {mutation: does the case have what the mutation corrupts?}
    'maxpool': {'zero_padding': lambda c: c['data'] == 'negative', 'window_shifted': lambda c: c['H'] >= 3 or c['W'] >= 3},
    'upsample2x_add': {'weights_swapped': lambda c: c['w'] > 1, 'no_clamp_at_0': lambda c: c['h'] > 1 or c['w'] > 1,
                       'skip_per_image': lambda c: c['B'] > 1},
    'area_downsample': {'divided_by_r': lambda c: c['r'] > 1},
    'copy_channels': {'b_not_modulo': lambda c: c['B'] > c['srcB']},
    'cbam_residual': {'mean_over_C_plus_1': lambda c: True, 'max_pooled_from_0': lambda c: c['data'] == 'negative',
                      'one_tap_dropped': lambda c: True, 'gate_channels_swapped': lambda c: True,
                      'avg_over_padded_P': lambda c: c['H'] * c['W'] % 16 != 0},
    'gru_gate': {'f_and_u_swapped': lambda c: True},
    'logits_to_prob': {'background_misses_object_0': lambda c: c['data'] != 'saturated',      # at +-40 another object or nobody holds the background
                       'clamp_constants_in_float64': _clamped, 'numerator_8_recomputed': lambda c: c['K'] > 8,
                       'weights_swapped': lambda c: c['w4'] > 1 and c['data'] == 'randn4',
                       'no_clamp_at_0': lambda c: (c['h4'] > 1 or (c['w4'] > 1 and c['lw'] == 0)) and c['data'] == 'randn4'},   # lw = 2 crops columns 0, 1
    'aggregate_masks': {'background_misses_object_0': lambda c: True, 'clamp_constants_in_float64': _clamped,
                        'numerator_8_recomputed': lambda c: c['K'] > 8},
    'resize_bilinear': {'weights_swapped': lambda c: c['Wi'] > 1,
                        'no_clamp_at_0': lambda c: (c['Ho'] > c['Hi'] > 1) or (c['Wo'] > c['Wi'] > 1)},
    'merge_masks': {'region_greater_equal': lambda c: c['valid_bits'] != (1 << c['K']) - 1},
    'argmax_u8': {'last_maximal_index': lambda c: c['C'] > 1},
}


def _fp32_twin(c):
    return {k: (0 if k in ('in_half', 'out_half', 'half') else v) for k, v in c.items()}


def test_a_subtly_wrong_kernel_falls_outside_the_bounds(capsys):
    """For every GPU case each mutation of the float64 reference must push an element past the case's bound; on exact cases it must
    change the result.  A (case, mutation) pair is SKIPPED where the case has the feature but its data cannot show the mutation
    (a dead hidden unit of CBAM at C = 16, a mean over 528 channels that 1 / 529 does not move past the worst-case bound); pairs of
    a case WITHOUT the feature (the predicates above: B = 1 has no second image, r = 1 no divisor, ...) are not pairs at all.  At
    most 5 % of the pairs may be skipped.  A mutation that stays under the wider bound of a HALF-storage case (+ 2^-11 |ref|) is
    allowed only if the same case with fp32 storage is in the grid and catches it."""
    pairs = skipped = without = half_under = 0
    missed = collections.Counter()
    grid = {op: {R.tag(c) for c in R.CASES[op]()} for op in MUTATIONS}
    memo = {}

    def caught(c, m):
        key = (R.tag(c), m)
        if key not in memo:
            i = R.make_inputs(c)
            ref, bound = R.reference(c, i)
            mut, _ = R.reference(c, i, mut=m)
            diff = (mut.double() - ref.double()).abs()
            assert not bool(torch.isnan(diff).any()), key
            memo[key] = bool((diff > 0).any()) if bound is None else bool((diff > bound).any())
        return memo[key]
    for op, muts in MUTATIONS.items():
        for c in R.CASES[op]():
            for m, has_feature in muts.items():
                if not has_feature(c):
                    without += 1
                    continue
                pairs += 1
                if caught(c, m):
                    continue
                twin = _fp32_twin(c)
                if twin != c and R.tag(twin) in grid[op] and op not in EXACT and caught(twin, m):
                    half_under += 1
                else:
                    skipped += 1
                    missed[(op, m)] += 1
    share = skipped / pairs
    with capsys.disabled():
        print(f'\nelementwise refs | sensitivity: {pairs} (case, mutation) pairs, {skipped} skipped ({100 * share:.2f} %), {half_under} under a '
              f'half-storage bound with an fp32 twin that catches them; {without} combinations of a case without the feature; skipped by '
              f'(operation, mutation): {dict(missed)}')
    assert share <= 0.05
    assert all(n < sum(1 for c in R.CASES[op]() if MUTATIONS[op][m](c)) for (op, m), n in missed.items()), missed   # no mutation goes unseen everywhere
