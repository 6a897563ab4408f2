"""GPU: scribble-to-mask (S2M) kernels and network against float64 torch and the reference's recorded outputs (tests/golden/s2m.npz)."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, load_golden
from xmem2_amd import ops
from xmem2_amd.ops import ConvWeights

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('make_s2m_goldens', os.path.join(GOLDEN, 'make_s2m_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, rtol=2e-4, atol=5e-5, msg=''):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), f'{msg}: {int(bad.sum())}/{bad.numel()} out of tolerance, max abs err {float(err.max()):.3e}'


def _cw(cout, cin, k, pad, seed, stride=1, dilation=1):
    g = _gen(seed)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (k * k * cin)) ** 0.5
    scale = 0.5 + torch.rand(cout, generator=g)
    shift = 0.1 * torch.randn(cout, generator=g)
    cw = ConvWeights(w.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda(), stride, pad, dilation=dilation)
    return cw, w, scale, shift


def _conv_ref(x, w, scale, shift, pad, dil, stride=1, res=None, relu_in=False, relu_out=False):
    """float64 torch: x NHWC cpu -> NHWC"""
    xi = x.double().permute(0, 3, 1, 2)
    if relu_in:
        xi = xi.clamp_min(0)
    y = F.conv2d(xi, w.double(), stride=stride, padding=pad, dilation=dil)
    y = y * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0) if relu_out else y


# ---- dilated convolution -----------------------------------------------------------------------------------------
DIL_CASES = [  # (B, H, W, cin, cout, dilation)
    (1, 30, 54, 64, 64, 1), (1, 30, 54, 64, 64, 2), (2, 30, 54, 64, 128, 6), (1, 30, 54, 96, 64, 12), (1, 30, 54, 64, 64, 18),
    (1, 5, 7, 32, 64, 12),            # map smaller than the dilation: only the centre tap reads the input
    (3, 9, 11, 36, 40, 18),           # B > 1, Cin not a multiple of 32 (generic loader), Cout not a multiple of 64
]


@pytest.mark.parametrize('B,H,W,cin,cout,dil', DIL_CASES)
def test_dilated_conv_vs_float64(B, H, W, cin, cout, dil):
    cw, w, sc, sh = _cw(cout, cin, 3, dil, seed=dil * 100 + cin, dilation=dil)
    x = torch.randn(B, H, W, cin, generator=_gen(1))
    y = ops.conv2d(x.cuda(), cw, relu_out=True)
    _close(y, _conv_ref(x, w, sc, sh, dil, dil, relu_out=True), msg=f'd={dil}')


def test_dilated_conv_res_relu_slices():
    """res + relu_in + relu_out, the input a channel slice of a wider buffer, the output written into a slice of another"""
    cw, w, sc, sh = _cw(64, 32, 3, 6, seed=5, dilation=6)
    big = torch.randn(2, 20, 24, 48, generator=_gen(2))
    res = torch.randn(2, 20, 24, 64, generator=_gen(3))
    out = torch.full((2, 20, 24, 100), 7.0, device='cuda')
    xs = big.cuda()[..., 8:40]
    ops.conv2d(xs, cw, out=out[..., 20:84], out_ld=100, res=res.cuda(), relu_in=True, relu_out=True, in_ld=48)
    ref = _conv_ref(big[..., 8:40], w, sc, sh, 6, 6, res=res, relu_in=True, relu_out=True)
    _close(out[..., 20:84], ref, msg='slices')
    assert bool((out[..., :20] == 7.0).all()) and bool((out[..., 84:] == 7.0).all()), 'wrote outside its channel slice'


@pytest.mark.parametrize('cin,cout,dil,H,W', [(2048, 256, 18, 30, 54), (2048, 256, 6, 30, 54), (512, 512, 2, 30, 54)])
def test_dilated_conv_layer_shapes(cin, cout, dil, H, W):
    """the ASPP branches and layer4's dilated 3x3 at 480p; tap skipping on and off give the same bits"""
    cw, w, sc, sh = _cw(cout, cin, 3, dil, seed=dil, dilation=dil)
    x = torch.rand(1, H, W, cin, generator=_gen(4))
    xd = x.cuda()
    y = ops.conv2d(xd, cw, relu_out=True)
    y_all = ops.conv2d_dilated(xd, cw, relu_out=True, tap_skip=False)
    assert torch.equal(y, y_all), 'tap skipping changed the result'
    _close(y, _conv_ref(x, w, sc, sh, dil, dil, relu_out=True), msg=f'{cin}->{cout} d={dil}')


@pytest.mark.parametrize('plan', [(3, 1), (2, 1), (1, 1), (6, 1), (3, 4)])
def test_dilation_one_is_bit_identical_to_conv2d(plan):
    cw, w, sc, sh = _cw(128, 64, 3, 1, seed=9)
    x = torch.randn(2, 23, 31, 64, generator=_gen(5)).cuda()
    res = torch.randn(2, 23, 31, 128, generator=_gen(6)).cuda()
    a = ops.conv2d(x, cw, res=res, relu_out=True, plan=plan)
    b = ops.conv2d_dilated(x, cw, dilation=1, res=res, relu_out=True, plan=plan)
    assert torch.equal(a, b)


def test_dilated_rejects_unsupported():
    cw, *_ = _cw(1, 32, 3, 2, seed=1, dilation=2)
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros(1, 8, 8, 32, device='cuda'), cw)          # Cout == 1
    cw, *_ = _cw(32, 32, 3, 2, seed=1, dilation=2)
    with pytest.raises(RuntimeError):
        ops.conv2d_dilated(torch.zeros(1, 8, 8, 32, device='cuda'), cw, plan=(9, 1))   # Winograd plan


# ---- other S2M kernels --------------------------------------------------------------------------------------------
def _np_pack(image, prev, scr, K, ignore, Hp, Wp, lh, lw):
    H, W = prev.shape
    out = np.zeros((K, Hp, Wp, 8), np.float32)
    for k in range(1, K + 1):
        out[k - 1, lh:lh + H, lw:lw + W, 0:3] = image.transpose(1, 2, 0)
        out[k - 1, lh:lh + H, lw:lw + W, 3] = prev == k
        out[k - 1, lh:lh + H, lw:lw + W, 4] = scr == k
        out[k - 1, lh:lh + H, lw:lw + W, 5] = (scr != k) & (scr != ignore)
    return out


@pytest.mark.parametrize('case', [0, 1])
def test_s2m_pack_bit_exact(case):
    from xmem2_amd.s2m import pad_divide_by_16
    name, H, W, K, seed = G.CASES[case]
    image, prev, scr = G.case_inputs(H, W, K, seed)
    Hp, Wp, lh, lw = pad_divide_by_16(H, W)
    got = ops.s2m_pack(torch.from_numpy(image).cuda(), torch.from_numpy(prev).cuda(), torch.from_numpy(scr).cuda(), K, 255,
                       Hp, Wp, lh, lw).cpu().numpy()
    assert np.array_equal(got, _np_pack(image, prev, scr, K, 255, Hp, Wp, lh, lw))


def test_channel_mean_and_broadcast():
    x = torch.randn(3, 30, 54, 2048, generator=_gen(7))
    m = ops.channel_mean(x.cuda())
    _close(m, x.double().mean((1, 2)), rtol=1e-5, atol=1e-6, msg='mean')
    assert torch.equal(m, ops.channel_mean(x.cuda())), 'mean not reproducible'
    buf = torch.zeros(3, 30, 54, 1280, device='cuda')
    ops.broadcast_channels(m[:, :256].contiguous(), buf[..., 1024:1280])
    assert torch.equal(buf[..., 1024:].cpu(), m[:, None, None, :256].cpu().expand(3, 30, 54, 256))
    assert bool((buf[..., :1024] == 0).all())


@pytest.mark.parametrize('hi,wi,ho,wo', [(30, 54, 120, 216), (13, 19, 52, 76), (30, 54, 77, 101), (7, 9, 5, 4)])
def test_resize_bilinear_nhwc_into_slice(hi, wi, ho, wo):
    x = torch.randn(2, hi, wi, 256, generator=_gen(8))
    buf = torch.zeros(2, ho, wo, 304, device='cuda')
    ops.resize_bilinear_nhwc(x.cuda(), (ho, wo), out=buf[..., 48:])
    # torch's fp32 interpolate: the source index and weights are fp32 arithmetic there too (a float64 statement moves the
    # weights of a non-integer ratio by ~1e-5)
    ref = F.interpolate(x.permute(0, 3, 1, 2), size=(ho, wo), mode='bilinear', align_corners=False).permute(0, 2, 3, 1)
    _close(buf[..., 48:], ref, rtol=1e-5, atol=1e-6, msg='resize')
    assert bool((buf[..., :48] == 0).all())


def _wbg64(prob, hard=True):
    new = torch.cat([torch.prod(1 - prob, 0, keepdim=True), prob], 0).clamp(1e-7, 1 - 1e-7)
    lg = torch.log(new / (1 - new)) * (1000 if hard else 1)
    return torch.softmax(lg, 0)


@pytest.mark.parametrize('K,H,W', [(1, 64, 96), (3, 200, 300)])
def test_s2m_output_vs_float64(K, H, W):
    from xmem2_amd.s2m import pad_divide_by_16
    Hp, Wp, lh, lw = pad_divide_by_16(H, W)
    lg = torch.randn(K, Hp // 4, Wp // 4, generator=_gen(K)) * 3
    prob, wbg, mask = ops.s2m_output(lg.cuda(), H, W, lh, lw, 1000.0)
    up = F.interpolate(lg.double()[None], size=(Hp, Wp), mode='bilinear', align_corners=False)[0]
    p64 = torch.sigmoid(up)[:, lh:lh + H, lw:lw + W]
    _close(prob, p64, rtol=1e-5, atol=1e-6, msg='prob')
    w64 = _wbg64(p64)
    ok = (torch.sort(w64, 0).values[-1] - torch.sort(w64, 0).values[-2]) > 1e-3 if K > 0 else None
    # hard softmax: compare the argmax (and the values away from ties), where the float64 winner is clear
    assert bool((mask.cpu().long() == w64.argmax(0))[ok].all())
    assert float((wbg.cpu().double() - w64)[:, ok].abs().max()) < 1e-3
    soft = ops.aggregate_wbg(prob, keep_bg=True, temperature=1.0)
    _close(soft, _wbg64(prob.cpu().double(), hard=False), rtol=1e-5, atol=1e-6, msg='soft wbg')


# ---- the network --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def s2m_net():
    from xmem2_amd.s2m import S2M
    from xmem2_amd.synth import synthetic_s2m_state_dict
    return S2M(device='cuda:0').load_weights(synthetic_s2m_state_dict(0))


def _case(i):
    name, H, W, K, seed = G.CASES[i]
    image, prev, scr = G.case_inputs(H, W, K, seed)
    return name, K, torch.from_numpy(image)[None], torch.from_numpy(prev), scr


def _err32(case):
    """the fp32 reference's own max |p - p64| on the host that recorded the goldens (printed for comparison, not gated)"""
    import json
    with open(os.path.join(GOLDEN, 's2m_fp32_reference.json')) as f:
        return float(json.load(f)[case]['max_abs'])


def _gate(p, p64, what, err32):
    p, p64 = p.detach().double().cpu(), torch.as_tensor(p64).double()
    err = float((p - p64).abs().max())
    decided = (p64 - 0.5).abs() > 5e-3
    flips = int(((p > 0.5) != (p64 > 0.5))[decided].sum())
    print(f'{what}: max |p - p64| {err:.3e} (fp32 reference {err32:.3e}), decided pixels that flip {flips}')
    assert err <= 2e-3, f'{what}: max |p - p64| = {err:.3e}'
    assert flips == 0, f'{what}: {flips} thresholded pixels disagree with float64'


def test_network_case1_intermediates(s2m_net):
    from xmem2_amd.s2m import pad_divide_by_16
    gd = load_golden('s2m')
    name, K, image, prev, scr = _case(0)
    H, W = prev.shape
    Hp, Wp, lh, lw = pad_divide_by_16(H, W)
    x = ops.s2m_pack(image[0].cuda(), prev.cuda(), torch.from_numpy(scr).cuda(), K, 255, Hp, Wp, lh, lw)
    f = s2m_net.features(x)
    nchw = lambda t: t.permute(0, 3, 1, 2).cpu()
    for key, got in (('low_level', nchw(f['low_level'])[:, :G.LOW_CHANNELS]), ('aspp', nchw(f['aspp'])), ('logits', nchw(f['logits']))):
        ref = torch.from_numpy(gd[f'c1_{key}64'])
        err = float((got.double() - ref.double()).abs().max())
        print(f'c1 {key}: max abs err {err:.3e}, scale {float(ref.abs().max()):.3e}')
        _close(got, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()), msg=key)
    from xmem2_amd.s2m import S2MController
    p = S2MController(s2m_net, K).interact(image.cuda(), prev.cuda(), scr)
    _gate(p, gd['c1_prob64'], 'c1 prob', _err32('c1'))


def test_network_case2_padded_three_objects(s2m_net):
    from xmem2_amd.s2m import S2MController
    gd = load_golden('s2m')
    name, K, image, prev, scr = _case(1)
    assert np.array_equal(G.pack_channels(prev.numpy(), scr, K), gd['c2_channels'])
    p = S2MController(s2m_net, K).interact(image.cuda(), prev.cuda(), scr)
    _gate(p, gd['c2_prob64_u16'].astype(np.float64) / 65535.0, 'c2 prob', _err32('c2'))
    # batching: K objects in one batch == K single-object calls (object k alone: relabel k -> 1, others -> 0 / > 1 stay negative)
    for k in range(1, K + 1):
        scr_k = np.where(scr == k, 1, np.where((scr != 255), 2, 255)).astype(np.uint8)
        prev_k = (prev == k).float()
        single = S2MController(s2m_net, 1).interact(image.cuda(), prev_k.cuda(), scr_k)
        _gate(single[0], p[k - 1].cpu(), f'c2 object {k} alone vs batched', 0.0)


def test_network_case3_480p(s2m_net):
    from xmem2_amd.s2m import S2MController, pad_divide_by_16
    gd = load_golden('s2m')
    name, K, image, prev, scr = _case(2)
    H, W = prev.shape
    Hp, Wp, lh, lw = pad_divide_by_16(H, W)
    x = ops.s2m_pack(image[0].cuda(), prev.cuda(), torch.from_numpy(scr).cuda(), K, 255, Hp, Wp, lh, lw)
    lg = s2m_net.features(x)['logits'].permute(0, 3, 1, 2).cpu()
    ref = torch.from_numpy(gd['c3_logits64'])
    print(f'c3 logits: max abs err {float((lg.double() - ref.double()).abs().max()):.3e}')
    p = S2MController(s2m_net, K).interact(image.cuda(), prev.cuda(), scr)
    _gate(p[:, ::G.C3_ROW_STRIDE], gd['c3_prob64_rows'], 'c3 prob rows', _err32('c3'))


def test_graph_replay_and_no_torch_arithmetic(s2m_net):
    from torch.utils._python_dispatch import TorchDispatchMode
    from xmem2_amd.s2m import S2MController
    name, K, image, prev, scr = _case(1)
    ctl = S2MController(s2m_net, K)
    img, pv = image.cuda(), prev.cuda()
    a = ctl.interact(img, pv, scr)
    n = s2m_net.captures
    b = ctl.interact(img, pv, scr)
    assert s2m_net.captures == n, 're-captured at the same geometry'
    assert torch.equal(a, b), 'the replay differs from the first call'

    allowed = ('empty', 'view', 'copy', 'clone', '_to_copy', 'to', 'detach', 'alias', 'as_strided', 'slice', 'select', 'lift_fresh',
               'unsqueeze', 'squeeze', 'expand', '_unsafe_view', 'reshape')
    seen = []

    class Rec(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func.__name__.split('.')[0])
            return func(*args, **(kwargs or {}))

    with Rec():
        ctl.interact(img, pv, scr)
    arith = sorted({o for o in seen if not any(o == x or o.startswith(x + '_') or o == x + '_' for x in allowed)})
    assert not arith, f'warm interact() ran torch ops {arith}'


def test_batched_bit_identical_when_plans_pinned(s2m_net):
    """the same object twice in a batch of 2 and alone: each row of the batch equals the single call at fixed tiles"""
    from xmem2_amd.s2m import S2MController
    name, K, image, prev, scr = _case(0)
    img, pv = image.cuda(), prev.cuda()
    scr2 = np.where(scr == 1, 2, scr).astype(np.uint8)
    prev2 = torch.where(prev == 1, torch.tensor(2.0), prev)
    one = S2MController(s2m_net, 2).interact(img, pv, scr)[0]
    two = S2MController(s2m_net, 2).interact(img, prev2.cuda(), scr2)[1]
    assert torch.equal(one, two)


# ---- end to end on the chair clip ---------------------------------------------------------------------------------
CHAIR = os.path.join(GOLDEN, 'chair')


def _strokes(ann):
    """Scribbles derived from an annotation: per object a horizontal stroke through its middle row (inside the object), one
    background stroke along a row away from every object; 255 elsewhere."""
    scr = np.full(ann.shape, 255, np.uint8)
    for k in [int(v) for v in np.unique(ann) if 0 < v < 255]:
        ys, xs = np.nonzero(ann == k)
        y = int(np.median(ys))
        row = np.nonzero(ann[y] == k)[0]
        scr[y, row[len(row) // 4: 3 * len(row) // 4 + 1]] = k
    free = np.nonzero((ann == 0).all(1))[0]
    y = int(free[len(free) // 2]) if len(free) else 2
    scr[y, ann.shape[1] // 8: ann.shape[1] - ann.shape[1] // 8] = 0
    return scr


def test_chair_end_to_end(tmp_path, synth_sd):
    import shutil
    import subprocess
    import sys
    from PIL import Image
    from xmem2_amd import InferenceCore, XMem
    from xmem2_amd.run_on_video import run_on_video
    from xmem2_amd.s2m import S2M, S2MController
    from xmem2_amd.scribble import IM_MEAN, IM_STD
    from xmem2_amd.synth import synthetic_s2m_state_dict
    names = sorted(os.listdir(os.path.join(CHAIR, 'JPEGImages')))
    imgs = tmp_path / 'JPEGImages'
    shutil.copytree(os.path.join(CHAIR, 'JPEGImages'), imgs)
    ann = np.array(Image.open(os.path.join(CHAIR, 'Annotations', names[0][:-4] + '.png')))
    scr = _strokes(ann)
    K = int(scr[scr < 255].max())
    (tmp_path / 'scr').mkdir()
    Image.fromarray(scr, mode='L').save(tmp_path / 'scr' / (names[0][:-4] + '.png'))
    # 1-3: the CLI writes an indexed PNG of the frame's size equal to the API's argmax
    r = subprocess.run([sys.executable, '-m', 'xmem2_amd.scribble', '--images', str(imgs), '--scribbles', str(tmp_path / 'scr'),
                        '--out', str(tmp_path / 'masks'), '--synthetic-seed', '0'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    written = Image.open(tmp_path / 'masks' / (names[0][:-4] + '.png'))
    assert written.mode == 'P' and written.size == (ann.shape[1], ann.shape[0])
    img0 = np.array(Image.open(imgs / names[0]).convert('RGB'), dtype=np.uint8)
    image = torch.from_numpy(((img0.astype(np.float32) / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1).copy())
    net = S2M(device='cuda:0').load_weights(synthetic_s2m_state_dict(0))
    ctl = S2MController(net, K)
    wbg, mask = ctl.predict(image[None].cuda(), torch.zeros(ann.shape).cuda(), scr)
    assert np.array_equal(np.array(written), mask.cpu().numpy())
    assert bool((mask == 1).any()), 'the strokes produced an empty mask'
    # 4: run_on_video takes the written directory as its masks directory
    ckpt = tmp_path / 'xmem.pth'
    torch.save(synth_sd, ckpt)
    run_on_video(str(imgs), str(tmp_path / 'masks'), str(tmp_path / 'out'), frames_with_masks=[0], print_progress=False,
                 overwrite_config={'model': str(ckpt)})
    assert len(os.listdir(tmp_path / 'out' / 'masks')) == len(names)
    # 5: gui.py:851-859 on the device result: one-hot -> [1:] -> put_to_permanent_memory, then step() over the clip
    cfg = dict(mem_every=5, deep_update_every=-1, enable_long_term=True, enable_long_term_count_usage=True, hidden_dim=64,
               key_dim=64, value_dim=512, top_k=30, max_mid_term_frames=10, min_mid_term_frames=5, num_prototypes=128,
               max_long_term_elements=10000)
    xnet = XMem(dict(cfg), None).to('cuda:0').eval()
    xnet.load_weights(synth_sd)
    core = InferenceCore(xnet, cfg)
    core.set_all_labels(list(range(1, K + 1)))
    onehot = F.one_hot(mask.long(), K + 1).permute(2, 0, 1).float()
    core.put_to_permanent_memory(image.cuda(), onehot[1:])
    for t, nm in enumerate(names[1:], 1):
        im = np.array(Image.open(imgs / nm).convert('RGB'), dtype=np.float32)
        frame = torch.from_numpy(((im / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1).copy()).cuda()
        prob = core.step(frame, None, None, end=(t == len(names) - 1))
        assert prob.shape == (K + 1,) + ann.shape and bool(torch.isfinite(prob).all())
