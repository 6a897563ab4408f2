"""The decoder's tail: `ops.mask_head_gather` (mask head + HiddenUpdater input + hidden copy in one launch) against the three launches
it replaces, the fused hidden-update convolution with its Cin padded to the 32-deep k-tile against the unpadded one, and the decoder
stage with the tail switched off and on.  The reference is always the existing path."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def g_(seed):
    return torch.Generator().manual_seed(seed)


def close(a, b, rtol, atol, msg):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), f'{msg}: {int(bad.sum())}/{bad.numel()} out of tol, max abs err {float(err.max()):.3e}'


# (K, h, w, c16, c8, c4, hd)
TAIL_SHAPES = [
    (1, 30, 54, 512, 256, 256, 64),      # the served shape
    (2, 3, 5, 16, 8, 12, 8),             # idle lanes, two objects, borders on every side
    (3, 1, 1, 4, 4, 4, 4),               # every tap but the centre row / column padded
    (1, 2, 3, 8, 4, 256, 4),             # all 64 lanes active on a tiny map
]
# wider tensors than one straight-line pass of the copy covers (the left-over loops): more than 128 / 64 / 64 float4 groups
TAIL_SHAPES_WIDE = [(2, 2, 3, 1032, 520, 8, 264)]
SENTINEL = 7.0


def _tail_inputs(shape):
    from xmem2_amd.ops import ConvWeights
    K, h, w, c16, c8, c4, hd = shape
    r = lambda *s, seed: torch.randn(*s, generator=g_(seed))            # negative values: relu-before-sum and no-relu-in-the-mean differ
    t = dict(g16=r(K, h, w, c16, seed=21), g8=r(K, 2 * h, 2 * w, c8, seed=22), g4=r(K, 4 * h, 4 * w, c4, seed=23),
             hidden=r(K, h, w, hd, seed=24))
    wgt = r(1, c4, 3, 3, seed=25) * (1.0 / (9 * c4)) ** 0.5
    scale, shift = torch.tensor([1.25]), torch.tensor([-0.1])
    cw = ConvWeights(wgt.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda(), 1, 1)
    return t, wgt, scale, shift, cw


def _run_both(shape):
    """(logits, g4d, cat) of the fused launch and of the three existing ops; g4d and cat seeded with a sentinel."""
    from xmem2_amd import ops
    K, h, w, c16, c8, c4, hd = shape
    t, wgt, scale, shift, cw = _tail_inputs(shape)
    d = {k: v.cuda() for k, v in t.items()}
    n = c16 + c8 + c4 + 1
    ld, mid = (n + 31) // 32 * 32 + 4, 12
    out = []
    for fused in (True, False):
        g4d = torch.full((K, h, w, ld), SENTINEL).cuda()
        cat = torch.full((K, h, w, mid + hd + 4), SENTINEL).cuda()
        if fused:
            logits = ops.mask_head_gather(d['g16'], d['g8'], d['g4'], cw, d['hidden'], g4d, cat, mid)
        else:
            logits = ops.conv2d(d['g4'], cw, relu_in=True)
            ops.hidden_update_gather(d['g16'], d['g8'], d['g4'], logits, g4d)
            ops.copy_channels(d['hidden'], cat, mid)
        torch.cuda.synchronize()
        out.append((logits, g4d, cat))
    return t, wgt, scale, shift, out, n, mid


@pytest.mark.parametrize('shape', TAIL_SHAPES + TAIL_SHAPES_WIDE, ids=lambda s: 'x'.join(map(str, s)))
def test_mask_head_gather_is_the_three_launches_in_one(shape):
    """Same bits as conv2d(relu_in) + hidden_update_gather + copy_channels on logits, g4d and cat; the padding channels of g4d and
    everything of cat outside [mid, mid + hd) keep the sentinel."""
    hd = shape[6]
    _, _, _, _, ((la, ga, ca), (lb, gb, cb)), n, mid = _run_both(shape)
    assert tuple(la.shape) == tuple(lb.shape)
    assert torch.equal(la, lb), f'logits: max |diff| {float((la - lb).abs().max()):.3e}'
    assert torch.equal(ga, gb), f'g4d: max |diff| {float((ga - gb).abs().max()):.3e}'
    assert torch.equal(ca, cb), f'cat: max |diff| {float((ca - cb).abs().max()):.3e}'
    assert bool((ga[..., n:] == SENTINEL).all()) and ga.shape[3] > n
    assert bool((ca[..., :mid] == SENTINEL).all()) and bool((ca[..., mid + hd:] == SENTINEL).all())


@pytest.mark.parametrize('shape', TAIL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_mask_head_gather_against_the_cpu(shape):
    """The fused launch alone against torch on the CPU: the logits at test_gpu_ops.py's convolution tolerance, g4d against
    F.interpolate(mode='area') at the gather test's 1e-5 / 1e-6, the hidden copy exactly."""
    from xmem2_amd import ops
    K, h, w, c16, c8, c4, hd = shape
    t, wgt, scale, shift, cw = _tail_inputs(shape)
    n = c16 + c8 + c4 + 1
    g4d = torch.zeros(K, h, w, (n + 3) // 4 * 4).cuda()
    cat = torch.zeros(K, h, w, 8 + hd).cuda()
    logits = ops.mask_head_gather(t['g16'].cuda(), t['g8'].cuda(), t['g4'].cuda(), cw, t['hidden'].cuda(), g4d, cat, 8)
    torch.cuda.synchronize()
    nchw = lambda x: x.permute(0, 3, 1, 2)
    ref_l = F.conv2d(F.relu(nchw(t['g4'])), wgt, None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    close(nchw(logits.cpu()), ref_l, 2e-4, 5e-5, f'logits {shape}')
    ref_g = torch.cat([nchw(t['g16']), F.interpolate(nchw(t['g8']), scale_factor=0.5, mode='area'),
                       F.interpolate(nchw(t['g4']), scale_factor=0.25, mode='area'),
                       F.interpolate(nchw(logits.cpu()), scale_factor=0.25, mode='area')], 1)
    close(nchw(g4d.cpu())[:, :n], ref_g, 1e-5, 1e-6, f'g4d {shape}')
    assert torch.equal(cat.cpu()[..., 8:], t['hidden'])


def test_mask_head_gather_rejects_what_it_cannot_run():
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    K, h, w = 1, 2, 2
    z = lambda *s: torch.zeros(*s).cuda()
    cw = ConvWeights(z(1, 3, 3, 260), torch.ones(1).cuda(), z(1), 1, 1)
    with pytest.raises(RuntimeError):                       # more channels than one float4 per lane
        ops.mask_head_gather(z(K, h, w, 8), z(K, 2 * h, 2 * w, 8), z(K, 4 * h, 4 * w, 260), cw, z(K, h, w, 4), z(K, h, w, 280), z(K, h, w, 8), 4)
    cw = ConvWeights(z(1, 3, 3, 8), torch.ones(1).cuda(), z(1), 1, 1)
    with pytest.raises(RuntimeError):                       # g4d too narrow for [g16 | g8 | g4 | logits]
        ops.mask_head_gather(z(K, h, w, 8), z(K, 2 * h, 2 * w, 8), z(K, 4 * h, 4 * w, 8), cw, z(K, h, w, 4), z(K, h, w, 24), z(K, h, w, 8), 4)


def _plan_info(x, cw, plan):
    from xmem2_amd import _lib, ops
    d = ops.ConvCall(x=x, cw=cw, out=x, plan=plan).d
    info = _lib.ConvPlanInfo()
    assert _lib.load().xmem_conv2d_plan_info(ctypes.byref(d), ctypes.byref(info)) == 0
    return info


@pytest.mark.parametrize('geom', [(1, 30, 54), (2, 5, 7)], ids=lambda s: 'x'.join(map(str, s)))
def test_padded_g_fused_has_the_same_bits_on_the_1x1_loader(geom):
    """The fused hidden-update convolution with Cin 1028 and with zero filter columns + zero input channels up to 1056, both under
    plan (3, 4): the same bits, and only the padded one has a Cin that the plan's k-tile divides (`generic = Cin % bk != 0` in the
    library: the padded call takes the 1x1 operand loader)."""
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    K, h, w = geom
    cin, cpad, cout, ldo = 1028, 1056, 256, 320
    x = torch.randn(K, h, w, cin, generator=g_(31))
    wgt = torch.randn(cout, 1, 1, cin, generator=g_(32)) * (1.0 / cin) ** 0.5
    shift = torch.randn(cout, generator=g_(33)) * 0.1
    outs = []
    for c in (cin, cpad):
        xc, wc = F.pad(x, (0, c - cin)).cuda(), F.pad(wgt, (0, c - cin)).contiguous().cuda()
        cw = ConvWeights(wc, torch.ones(cout).cuda(), shift.cuda(), 1, 0, cin_true=cin)
        out = torch.full((K, h, w, ldo), SENTINEL).cuda()
        ops.RECORD = []
        try:
            ops.conv2d(xc, cw, out=out, out_ld=ldo, plan=(3, 4))
        finally:
            rec, ops.RECORD = ops.RECORD, None
        torch.cuda.synchronize()
        assert rec[0][4][5]['plan'] == (3, 4) and f'x{c}/{c}->256/320' in rec[0][1]
        info = _plan_info(xc, cw, (3, 4))
        assert (info.bm, info.bn, info.bk) == (64, 64, 32) and info.splitk == 4 and info.ring == 0
        assert (c % info.bk == 0) == (c == cpad)            # 1056: the non-generic (1x1) loader; 1028: the general one
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), f'max |diff| {float((outs[0] - outs[1]).abs().max()):.3e}'
    assert bool((outs[1][..., cout:] == SENTINEL).all())
    ref = F.conv2d(x.permute(0, 3, 1, 2), wgt.permute(0, 3, 1, 2), shift)
    close(outs[1][..., :cout].cpu().permute(0, 3, 1, 2), ref, 2e-4, 5e-5, 'padded g_fused vs CPU')


@pytest.fixture(scope='module')
def tail_nets(synth_sd):
    """The network with the tail switched off, on (the shipped size threshold: at 96x128 only the padded Cin is taken) and on with
    the threshold at 0 (the fused launch runs on the 6x8 map too).  One network each: a captured stage is keyed by shapes only."""
    from xmem2_amd.network import XMem
    nets = {}
    for name, on, min_pixels in (('off', False, None), ('on', True, None), ('on0', True, 0)):
        net = XMem({'key_dim': 64, 'value_dim': 512, 'hidden_dim': 64, 'precision': 'fp32'}, None)
        net.fused_tail = on
        if min_pixels is not None:
            net.fused_tail_min_pixels = min_pixels
        net.to('cuda').eval()
        net.load_weights(synth_sd)
        nets[name] = net
    assert nets['off']._w['decoder.hidden_update.g_fused'].cin == 1028 and nets['on']._w['decoder.hidden_update.g_fused'].cin == 1056
    return nets


@pytest.mark.parametrize('K', [1, 2])
@pytest.mark.parametrize('graphs', [True, False], ids=['graphs', 'eager'])
def test_decoder_stage_tail_off_vs_on(tail_nets, graphs, K):
    """segment_nhwc at a 96x128 input over three consecutive frames (the hidden state advances in place): the same prob and the same
    hidden state with the tail off, on, and on with the fused launch forced."""
    from xmem2_amd import ops
    h, w = 6, 8
    r = lambda *s, seed, k=0.5: (torch.randn(*s, generator=g_(seed)) * k).cuda()
    feats = [(r(1, h, w, 1024, seed=40 + f), r(1, 2 * h, 2 * w, 512, seed=50 + f), r(1, 4 * h, 4 * w, 256, seed=60 + f),
              r(K, h, w, 512, seed=70 + f)) for f in range(3)]
    hid0 = r(K, h, w, 64, seed=80, k=0.3)
    runs = {}
    for name, net in tail_nets.items():
        net.use_graphs = graphs
        hidden, frames = hid0.clone(), []
        for f16, f8, f4, ro in feats:
            cat16 = net.new_decoder_input(K, h, w, f16.device)
            ops.copy_channels(ro, cat16, 1024)
            new_hidden, prob, _ = net.segment_nhwc(f16, f8, f4, cat16, hidden, (16 * h, 16 * w), (0, 0), h_out=True)
            torch.cuda.synchronize()
            frames.append((prob.clone(), new_hidden.clone()))
            hidden = new_hidden
        runs[name] = frames
    for f in range(3):
        p0, h0 = runs['off'][f]
        assert bool(torch.isfinite(p0).all()) and bool(torch.isfinite(h0).all())
        for name in ('on', 'on0'):
            p1, h1 = runs[name][f]
            assert torch.equal(p0, p1), f'{name} frame {f}: prob differs, max |diff| {float((p0 - p1).abs().max()):.3e}'
            assert torch.equal(h0, h1), f'{name} frame {f}: hidden differs, max |diff| {float((h0 - h1).abs().max()):.3e}'
    assert not torch.equal(runs['off'][0][1], runs['off'][2][1])       # the state did advance
