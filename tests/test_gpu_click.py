"""GPU: click-to-mask kernels and network against float64 torch and the reference's recorded outputs (tests/golden/click.npz)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, load_golden
from xmem2_amd import ops
from xmem2_amd.ops import ConvWeights

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('make_click_goldens', os.path.join(GOLDEN, 'make_click_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, rtol=1e-5, atol=1e-6, msg=''):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), f'{msg}: {int(bad.sum())}/{bad.numel()} out of tolerance, max abs err {float(err.max()):.3e}'


def _ac(x, size):
    """float64 F.interpolate(align_corners=True) of [N,C,H,W]"""
    return F.interpolate(x.double(), size=size, mode='bilinear', align_corners=True)


# ---- click_input ------------------------------------------------------------------------------------------------------
def _rgb_par(seed):
    g = _gen(seed)
    w1, b1 = torch.randn(8, 5, generator=g) * 0.6, torch.randn(8, generator=g) * 0.2
    w2, b2 = torch.randn(3, 8, generator=g) * 0.4, torch.randn(3, generator=g) * 0.1
    return torch.cat([w1.reshape(-1), b1, w2.reshape(-1), b2]), (w1, b1, w2, b2)


def _click_buffers(pos, neg, cap=16):
    buf = np.full((2, cap, 2), -1.0, np.float32)
    buf[0, :len(pos)] = np.array(pos, np.float32).reshape(-1, 2)
    buf[1, :len(neg)] = np.array(neg, np.float32).reshape(-1, 2)
    return torch.from_numpy(buf).cuda(), torch.tensor([len(pos), len(neg)], dtype=torch.int32).cuda()


@pytest.mark.parametrize('case', range(len(G.DIST_CASES)))
def test_click_input_features_vs_cython_goldens(case):
    name, H, W, pos, neg = G.DIST_CASES[case]
    gd = load_golden('click')
    par, _ = _rgb_par(1)
    image = torch.randn(3, H, W, generator=_gen(2))
    clicks, counts = _click_buffers(pos, neg)
    out, feat = ops.click_input(image.cuda(), clicks, counts, par.cuda(), 260.0, with_flip=True, want_features=True)
    _close(feat[0], gd[f'{name}_features64'], msg=name)
    if not pos:
        assert bool((feat[0, 0] == 1.0).all()), 'a polarity without a click must give exactly 1'
    # the counts live on the device: the same buffers with the counts zeroed see no click
    none = ops.click_input(image.cuda(), clicks, torch.zeros(2, dtype=torch.int32).cuda(), par.cuda(), want_features=True)[1]
    assert bool((none == 1.0).all())


def test_click_input_full_output_flip_and_padding():
    H, W = 37, 53
    par, (w1, b1, w2, b2) = _rgb_par(3)
    image = torch.randn(3, H, W, generator=_gen(4))
    pos, neg = [(5.0, 7.0), (30.2, 41.7)], [(18.5, 2.5), (-1.0, -1.0)]
    clicks, counts = _click_buffers(pos, neg)
    out, feat = ops.click_input(image.cuda(), clicks, counts, par.cuda(), want_features=True)
    assert out.shape == (2, H, W, 8) and bool((out[..., 3:] == 0).all()), 'channels 3..7 must be zero'
    # float64 rgb_conv on the kernel's own features (their parity with the reference is the test above)
    x = torch.cat([torch.stack([image, image.flip(2)]).double(), feat.cpu().double()], 1)          # [2,5,H,W]
    y = torch.einsum('jk,bkhw->bjhw', w1.double(), x) + b1.double()[None, :, None, None]
    y = torch.where(y > 0, y, 0.2 * y)
    ref = torch.einsum('mj,bjhw->bmhw', w2.double(), y) + b2.double()[None, :, None, None]
    _close(out[..., :3].permute(0, 3, 1, 2), ref, rtol=2e-4, atol=5e-5, msg='rgb_conv')
    # sample 1 == the kernel on the mirrored image with mirrored clicks, bit for bit
    mirror = lambda cl: [(r, (W - 1) - c) if r >= 0 else (r, c) for r, c in cl]
    clicks_m, _ = _click_buffers(mirror(pos), mirror(neg))
    out_m = ops.click_input(image.flip(2).contiguous().cuda(), clicks_m, counts, par.cuda(), with_flip=False)
    assert out_m.shape == (1, H, W, 8) and torch.equal(out_m[0], out[1])
    assert torch.equal(ops.click_input(image.cuda(), clicks, counts, par.cuda(), with_flip=False)[0], out[0])


def test_click_input_ignores_clicks_outside_the_map():
    par, _ = _rgb_par(5)
    image = torch.zeros(3, 9, 11)
    inside, _ = _click_buffers([(4.0, 5.0)], [])
    wild, counts = _click_buffers([(4.0, 5.0), (9.0, 3.0), (2.0, 11.2), (3.0, -0.6), (-0.51, 2.0)], [])
    a = ops.click_input(image.cuda(), inside, torch.tensor([1, 0], dtype=torch.int32).cuda(), par.cuda(), want_features=True)[1]
    b = ops.click_input(image.cuda(), wild, counts, par.cuda(), want_features=True)[1]
    assert torch.equal(a, b)


# ---- depthwise 3x3 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,W,C', [(2, 1, 1, 64), (1, 3, 5, 160), (2, 25, 33, 160), (1, 60, 60, 128), (3, 7, 6, 4)])
def test_depthwise3x3_vs_float64(B, H, W, C):
    x = torch.randn(B, H, W, C, generator=_gen(C + H))
    w = torch.randn(C, 1, 3, 3, generator=_gen(C)) * 0.5
    wk = w.reshape(C, 9).t().contiguous()
    y = ops.depthwise3x3(x.cuda(), wk.cuda())
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1, groups=C).permute(0, 2, 3, 1)
    _close(y, ref, rtol=2e-4, atol=5e-5, msg=f'depthwise {B}x{H}x{W}x{C}')


def test_depthwise3x3_channel_slices():
    B, H, W, C = 2, 9, 13, 32
    big = torch.randn(B, H, W, 48, generator=_gen(7))
    w = torch.randn(C, 1, 3, 3, generator=_gen(8))
    out = torch.full((B, H, W, 100), 7.0, device='cuda')
    ops.depthwise3x3(big.cuda()[..., 8:40], w.reshape(C, 9).t().contiguous().cuda(), out=out[..., 20:52])
    ref = F.conv2d(big[..., 8:40].double().permute(0, 3, 1, 2), w.double(), padding=1, groups=C).permute(0, 2, 3, 1)
    _close(out[..., 20:52], ref, rtol=2e-4, atol=5e-5, msg='slices')
    assert bool((out[..., :20] == 7.0).all()) and bool((out[..., 52:] == 7.0).all()), 'wrote outside its channel slice'


# ---- align_corners resampling -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('hi,wi,ho,wo', [(13, 17, 25, 33), (1, 17, 25, 33), (13, 1, 25, 33), (13, 17, 1, 33), (25, 33, 13, 17)])
def test_resize_bilinear_ac_nhwc_into_slice(hi, wi, ho, wo):
    x = torch.randn(2, hi, wi, 128, generator=_gen(hi * wi))
    buf = torch.zeros(2, ho, wo, 160, device='cuda')
    ops.resize_bilinear_ac_nhwc(x.cuda(), (ho, wo), out=buf[..., 0:128])
    ref = _ac(x.permute(0, 3, 1, 2), (ho, wo)).permute(0, 2, 3, 1)
    _close(buf[..., :128], ref, msg='resize ac nhwc')
    assert bool((buf[..., 128:] == 0).all())


def test_resize_bilinear_ac_equal_sizes_copy():
    x = torch.randn(2, 13, 17, 128, generator=_gen(9)).cuda()
    assert torch.equal(ops.resize_bilinear_ac_nhwc(x, (13, 17)), x)
    p = torch.randn(3, 21, 34, generator=_gen(10)).cuda()
    assert torch.equal(ops.resize_bilinear_ac(p, (21, 34)), p)


def test_resize_bilinear_ac_crop_paste():
    x = torch.randn(3, 40, 56, generator=_gen(11))
    xd = x.cuda()
    # a crop touching the top and the right border
    roi = (0, 22, 31, 55)
    got = ops.resize_bilinear_ac(xd, (48, 51), crop=roi)
    _close(got, _ac(x[None, :, 0:23, 31:56], (48, 51))[0], msg='crop')
    # paste with zero fill
    small = torch.randn(1, 19, 27, generator=_gen(12))
    out = torch.full((1, 40, 56), 5.0, device='cuda')
    ops.resize_bilinear_ac(small.cuda(), None, out=out, paste=(7, 30, 10, 50), zero_fill=True)
    ref = torch.zeros(1, 40, 56, dtype=torch.float64)
    ref[:, 7:31, 10:51] = _ac(small[None], (24, 41))[0]
    _close(out, ref, msg='paste')
    assert bool((out[:, :7] == 0).all()) and bool((out[:, :, 51:] == 0).all())
    # without the fill the rest of the destination stays
    out = torch.full((1, 40, 56), 5.0, device='cuda')
    ops.resize_bilinear_ac(small.cuda(), None, out=out, paste=(7, 30, 10, 50))
    assert bool((out[:, :7] == 5.0).all()) and bool((out[:, 31:] == 5.0).all()) and bool((out[:, :, :10] == 5.0).all())
    _close(out[:, 7:31, 10:51], ref[:, 7:31, 10:51], msg='paste, no fill')
    # crop -> resize -> paste back: the zoom-in's round trip
    z = ops.resize_bilinear_ac(xd, (48, 51), crop=roi)
    back = torch.empty(3, 40, 56, device='cuda')
    ops.resize_bilinear_ac(z, None, out=back, paste=roi, zero_fill=True)
    ref = torch.zeros(3, 40, 56, dtype=torch.float64)
    ref[:, 0:23, 31:56] = _ac(_ac(x[None, :, 0:23, 31:56], (48, 51)), (23, 25))[0]
    _close(back, ref, msg='round trip')


@pytest.mark.parametrize('flip', [True, False])
def test_click_prob_vs_float64(flip):
    h4, w4, H, W = 25, 33, 97, 131
    lg = torch.randn(2 if flip else 1, h4, w4, generator=_gen(13)) * 3
    p = ops.click_prob(lg.cuda(), H, W)
    up = _ac(lg[None], (H, W))[0]
    ref = torch.sigmoid(0.5 * (up[0] + up[1].flip(1))) if flip else torch.sigmoid(up[0])
    _close(p, ref, msg='click_prob')
    if flip:       # the average is taken on the logits, not on the probabilities
        other = 0.5 * (torch.sigmoid(up[0]) + torch.sigmoid(up[1].flip(1)))
        assert float((other - ref).abs().max()) > 1e-2


# ---- mask_bbox, prob_threshold, click_commit ----------------------------------------------------------------------------------------
def _bbox(prob, thr=0.5, pix=None):
    pixd = torch.tensor(pix, dtype=torch.int32).cuda() if pix else None
    return ops.mask_bbox(prob.cuda(), thr, pixd).cpu().tolist()


def test_mask_bbox_exact():
    from xmem2_amd.click import mask_bbox_host
    H, W = 67, 301
    empty = torch.full((H, W), 0.5)                      # == threshold: not set
    assert _bbox(empty) == [2 ** 31 - 1, -1, 2 ** 31 - 1, -1, 0]
    one = empty.clone()
    one[66, 300] = 0.6
    assert _bbox(one) == [66, 66, 300, 300, 1]
    assert _bbox(torch.ones(H, W)) == [0, H - 1, 0, W - 1, H * W]
    p = torch.rand(H, W, generator=_gen(14))
    p[:5] = 0
    p[:, 290:] = 0
    for thr, pix in ((0.9, None), (0.999, [(2, 3)]), (0.9, [(1, 295), (66, 0)]), (2.0, [(10, 20), (30, 5)])):
        assert tuple(_bbox(p, thr, pix)) == mask_bbox_host(p.numpy(), thr, pix or ())
    big = torch.zeros(1100, 1300)                        # more pixels than one pass of the grid covers
    big[1099, 7] = big[3, 1299] = 1
    assert _bbox(big) == [3, 1099, 7, 1299, 2]


def test_prob_threshold():
    p = torch.tensor([[0.5, 0.50001, 0.2], [1.0, 0.0, 0.49999]])
    assert torch.equal(ops.prob_threshold(p.cuda()).cpu(), (p > 0.5).float())


def _wbg64(prob, hard=True):
    new = torch.cat([torch.prod(1 - prob, 0, keepdim=True), prob], 0).clamp(1e-7, 1 - 1e-7)
    return torch.softmax(torch.log(new / (1 - new)) * (1000 if hard else 1), 0)


@pytest.mark.parametrize('K,tar', [(1, 1), (3, 2)])
def test_click_commit_vs_float64(K, tar):
    H, W = 45, 77
    prev = torch.rand(K + 1, H, W, generator=_gen(15 + K))
    prev[1, :10] = 1.0                                    # a confident earlier object: clamped to 0.9, so that a click can overwrite it
    obj = (torch.rand(H, W, generator=_gen(16)) > 0.5).float()
    out, mask = ops.click_commit(prev.cuda(), obj.cuda(), tar)
    p = prev.double().clamp(max=0.9)
    p[tar] = obj.double()
    w64 = _wbg64(p[1:])
    srt = torch.sort(w64, 0).values
    ok = (srt[-1] - srt[-2]) > 1e-3
    assert float(ok.float().mean()) > 0.9
    assert bool((mask.cpu().long() == w64.argmax(0))[ok].all())
    assert float((out.cpu().double() - w64)[:, ok].abs().max()) < 1e-3
    assert bool((mask[:10][obj[:10].cuda() > 0.5] == tar).all()), 'the click mask must overwrite a saturated earlier object'
    soft, _ = ops.click_commit(prev.cuda(), obj.cuda(), tar, temperature=1.0)
    _close(soft, _wbg64(p[1:], hard=False), msg='soft commit')


# ---- the network --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def click_net():
    from xmem2_amd.click import ClickNet
    from xmem2_amd.synth import synthetic_click_state_dict
    return ClickNet(device='cuda:0').load_weights(synthetic_click_state_dict(0))


def _err32(case, step=None):
    with open(os.path.join(GOLDEN, 'click_fp32_reference.json')) as f:
        d = json.load(f)[case]
    return float(d['max_abs'] if step is None else d['per_step'][step])


def _gate(p, p64, what, err32):
    p, p64 = p.detach().double().cpu(), torch.as_tensor(p64).double()
    err = float((p - p64).abs().max())
    decided = (p64 - 0.5).abs() > 5e-3
    flips = int(((p > 0.5) != (p64 > 0.5))[decided].sum())
    print(f'{what}: max |p - p64| {err:.3e} (fp32 reference {err32:.3e}), decided pixels that flip {flips}')
    assert err <= 2e-3, f'{what}: max |p - p64| = {err:.3e}'
    assert flips == 0, f'{what}: {flips} thresholded pixels disagree with float64'


def _controller(net, name):
    from xmem2_amd.click import FBRSController
    c = G.NET_CASES[name]
    return FBRSController(net, max_size=c['max_size'], zoom_in_params=c['zoom'])


def test_network_n1_intermediates(click_net):
    from xmem2_amd.click import NORM_RADIUS
    gd = load_golden('click')
    c = G.NET_CASES['n1']
    image = torch.from_numpy(G.case_image('n1')).cuda()
    _, x, y, _pos = c['steps'][0]
    clicks, counts = _click_buffers([(y, x)], [], cap=64)
    inp = ops.click_input(image, clicks, counts, click_net._w['rgb_conv'], NORM_RADIUS, True)
    f = click_net.features(inp)
    lg = click_net.head(f['head_input'])
    nchw = lambda t: t.permute(0, 3, 1, 2).cpu()
    ch = click_net.deeplab_ch
    assert f['aspp'].shape[1:3] == (13, 17) and f['head_input'].shape == (2, 25, 33, ch + 32)
    for key, got in (('rgb', nchw(inp[..., :3])), ('skip', nchw(f['head_input'][..., ch:])),
                     ('aspp', nchw(f['aspp'])[:, ::G.ASPP_CHANNEL_STRIDE]),
                     ('head_input', nchw(f['head_input'])[:, ::G.HEAD_CHANNEL_STRIDE]), ('logits', nchw(lg))):
        ref = torch.from_numpy(gd[f'n1_{key}64'])
        err = float((got.double() - ref.double()).abs().max())
        print(f'n1 {key}: max abs err {err:.3e}, scale {float(ref.abs().max()):.3e}')
        _close(got, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()), msg=key)
    ctl = _controller(click_net, 'n1')
    mask = ctl.interact(image[None], x, y, True)
    _gate(ctl.prob, gd['n1_prob64'][0], 'n1 prob', _err32('n1'))
    assert mask.shape == (1, 1, c['H'], c['W']) and torch.equal(mask[0, 0], (ctl.prob > 0.5).float())


def _drive(net, name, gd, probs64):
    """Run the case's steps through FBRSController; check geometry and probability after every click and the undo."""
    c = G.NET_CASES[name]
    ctl = _controller(net, name)
    image = torch.from_numpy(G.case_image(name))[None].cuda()
    k = s = 0                # click index, step index among the recorded probabilities
    kept = []
    for step in c['steps']:
        if step[0] == 'plant':
            states = ctl.predictor.get_states()
            z = list(states['transform_states'][0])
            z[2] = torch.from_numpy(G.planted_probs(name)).cuda()
            states['transform_states'][0] = tuple(z)
            ctl.predictor.set_states(states)
            continue
        if step[0] == 'undo':
            before = kept[-2]
            ctl.undo()
            assert ctl.prob is before[0] and torch.equal(ctl.prob, before[1]), 'undo did not restore the previous probability bit for bit'
            _gate(ctl.prob, probs64[s], f'{name} after undo', 0.0)
            kept.pop()
            s += 1
            continue
        _, x, y, positive = step
        ctl.interact(image, x, y, positive)
        zoom, limit = ctl.predictor.transforms
        size, clicks = ctl.predictor.last_geometry
        assert G._roi_arr(zoom._object_roi).tolist() == gd[f'{name}_rois'][k].tolist(), f'{name} click {k}: ROI'
        assert G._roi_arr(limit._object_roi).tolist() == gd[f'{name}_limit_rois'][k].tolist(), f'{name} click {k}: LimitLongestSide ROI'
        assert list(size) == gd[f'{name}_sizes'][k].tolist(), f'{name} click {k}: working size'
        assert np.array_equal(np.array(clicks, np.float64).reshape(-1, 2), gd[f'{name}_clicks{k}']), f'{name} click {k}: transformed clicks'
        _gate(ctl.prob, probs64[s], f'{name} click {k}', _err32(name, s))
        kept.append((ctl.prob, ctl.prob.clone()))
        k += 1
        s += 1
    return ctl, image


def test_network_n2_controller_sequence(click_net):
    gd = load_golden('click')
    ctl, image = _drive(click_net, 'n2', gd, gd['n2_prob64_u16'].astype(np.float64) / 65535.0)
    # every kept state is a copy: the static buffers of later clicks did not change an earlier probability (checked at the undo);
    # interact after unanchor() starts a fresh session
    first = G.NET_CASES['n2']['steps'][0]
    ctl.unanchor()
    ctl.interact(image, first[1], first[2], first[3])
    assert len(ctl.clicks) == 1 and len(ctl.states) == 1 and ctl.predictor.transforms[0]._object_roi is None
    _gate(ctl.prob, gd['n2_prob64_u16'][0].astype(np.float64) / 65535.0, 'n2 click 0 after unanchor', _err32('n2', 0))
    assert ctl.undo() is None and ctl.prob is None and ctl.undo() is None


def test_network_n3_limit_longest_side_then_zoom(click_net):
    gd = load_golden('click')
    _drive(click_net, 'n3', gd, gd['n3_prob64_u16'].astype(np.float64) / 65535.0)


def test_network_n4_480p_defaults(click_net):
    gd = load_golden('click')
    c = G.NET_CASES['n4']
    rows = gd['n4_prob64_rows_u16'].astype(np.float64) / 65535.0
    ctl = _controller(click_net, 'n4')
    image = torch.from_numpy(G.case_image('n4'))[None].cuda()
    for k, (_, x, y, positive) in enumerate(c['steps']):
        ctl.interact(image, x, y, positive)
        assert list(ctl.predictor.last_geometry[0]) == gd['n4_sizes'][k].tolist()
        assert G._roi_arr(ctl.predictor.transforms[0]._object_roi).tolist() == gd['n4_rois'][k].tolist()
        _gate(ctl.prob[::G.N4_ROW_STRIDE], rows[k], f'n4 click {k} rows', _err32('n4', k))


def test_graph_replay_and_no_torch_arithmetic(click_net):
    from torch.utils._python_dispatch import TorchDispatchMode
    c = G.NET_CASES['n2']
    image = torch.from_numpy(G.case_image('n2'))[None].cuda()
    ctl = _controller(click_net, 'n2')
    ctl.interact(image, 88, 60, True)
    ctl.predictor.transforms[0]._prev_probs = torch.from_numpy(G.planted_probs('n2')).cuda()
    ctl.interact(image, 100, 40, False)                 # zoomed: captures (or finds) the ROI's geometry
    n = click_net.captures
    a = ctl.prob
    ctl.undo()
    ctl.interact(image, 100, 40, False)
    assert click_net.captures == n, 're-captured at the same geometry'
    assert torch.equal(a, ctl.prob), 'the replay differs from the first call'

    allowed = ('empty', 'view', 'copy', 'clone', '_to_copy', 'to', 'detach', 'alias', 'as_strided', 'slice', 'select', 'lift_fresh',
               'unsqueeze', 'squeeze', 'expand', '_unsafe_view', 'reshape', '_local_scalar_dense', 'item')
    seen = []

    class Rec(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func.__name__.split('.')[0])
            return func(*args, **(kwargs or {}))

    with Rec():
        ctl.interact(image, 90, 62, True)               # a third click in the same ROI
    assert click_net.captures == n
    arith = sorted({o for o in seen if not any(o == x or o.startswith(x + '_') or o == x + '_' for x in allowed)})
    assert not arith, f'warm interact() ran torch ops {arith}'


def test_ninth_geometry_evicts_the_first():
    from xmem2_amd.click import MAX_GEOMETRIES, ClickNet
    from xmem2_amd.synth import synthetic_click_state_dict
    net = ClickNet(device='cuda:0').load_weights(synthetic_click_state_dict(0))
    pts = np.array([[4, 5], [-1, -1]], np.float32)
    sizes = [(17 + 2 * i, 23) for i in range(MAX_GEOMETRIES + 1)]
    for h, w in sizes[:MAX_GEOMETRIES]:
        net.run(torch.zeros(3, h, w, device='cuda'), pts)
    net.run(torch.zeros(3, *sizes[0], device='cuda'), pts)           # the first is now the most recently used
    assert net.captures == MAX_GEOMETRIES
    net.run(torch.zeros(3, *sizes[MAX_GEOMETRIES], device='cuda'), pts)
    keys = [k[:2] for k in net._graphs]
    assert len(keys) == MAX_GEOMETRIES and sizes[1] not in keys and sizes[0] in keys and sizes[MAX_GEOMETRIES] in keys
    net.run(torch.zeros(3, *sizes[1], device='cuda'), pts)           # evicted: captured again
    assert net.captures == MAX_GEOMETRIES + 2
    # more clicks than the buffers hold: they grow, with a recapture, and the extra clicks count
    img = torch.randn(3, 17, 23, generator=_gen(20)).cuda()
    many = np.array([[i % 17, (3 * i) % 23] for i in range(70)] + [[-1, -1]] * 70, np.float32)
    few = many.copy()
    few[64:70] = -1
    a = net.run(img, many).clone()
    assert net._cap == 128
    assert not torch.equal(a, net.run(img, few))


# ---- command line on the chair clip -------------------------------------------------------------------------------------
CHAIR = os.path.join(GOLDEN, 'chair')


def test_cli_on_chair_frames(tmp_path):
    import shutil
    import subprocess
    import sys
    from PIL import Image
    from xmem2_amd.click import ClickNet, FBRSController, click_commit
    from xmem2_amd.scribble import IM_MEAN, IM_STD
    from xmem2_amd.synth import synthetic_click_state_dict
    names = sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages')))[:2]
    imgs = tmp_path / 'JPEGImages'
    imgs.mkdir()
    for nm in names:
        shutil.copy(os.path.join(CHAIR, 'JPEGImages', nm), imgs / nm)
    img0 = np.array(Image.open(imgs / names[0]).convert('RGB'), dtype=np.uint8)
    H, W = img0.shape[:2]
    frame = int(''.join(ch for ch in names[0] if ch.isdigit()))
    clicks = [{'object': 1, 'x': W // 3, 'y': H // 2, 'positive': True}, {'object': 1, 'x': W // 3 + 9, 'y': H // 2 - 7, 'positive': True},
              {'object': 1, 'x': 5, 'y': 5, 'positive': False},
              {'object': 2, 'x': 2 * W // 3, 'y': H // 3, 'positive': True}, {'object': 2, 'x': 2 * W // 3 + 4, 'y': H // 3 + 6, 'positive': True},
              {'object': 2, 'x': W - 6, 'y': H - 6, 'positive': False}]
    (tmp_path / 'clicks.json').write_text(json.dumps({str(frame): clicks}))
    r = subprocess.run([sys.executable, '-m', 'xmem2_amd.click', '--images', str(imgs), '--clicks', str(tmp_path / 'clicks.json'),
                        '--out', str(tmp_path / 'masks'), '--synthetic-seed', '0'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    written = Image.open(tmp_path / 'masks' / (os.path.splitext(names[0])[0] + '.png'))
    assert written.mode == 'P' and written.size == (W, H)
    assert sorted(os.listdir(tmp_path / 'masks')) == [os.path.splitext(names[0])[0] + '.png']
    # the controller's own argmax
    image = torch.from_numpy(((img0.astype(np.float32) / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1).copy()).cuda()
    ctl = FBRSController(ClickNet(device='cuda:0').load_weights(synthetic_click_state_dict(0)))
    prob = torch.zeros(3, H, W, device='cuda')
    prob[0] = 1
    for k in (1, 2):
        ctl.unanchor()
        for c in clicks:
            if c['object'] == k:
                obj = ctl.interact(image, c['x'], c['y'], c['positive'])
        assert bool((obj > 0.5).any()), f'object {k}: empty click mask'
        prob, mask = click_commit(prob, obj, k)
    assert np.array_equal(np.array(written), mask.cpu().numpy())
    assert bool((mask == 1).any()) and bool((mask == 2).any()), 'an object mask is empty'
