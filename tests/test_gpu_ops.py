"""GPU parity (op level): every kernel, called through the C ABI, against the oracle / plain torch-CPU fp32
on the same seeded inputs.  Tolerances are fp32-roundoff class (different summation order only)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def g_(seed):
    return torch.Generator().manual_seed(seed)


def nhwc(x):      # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):      # NHWC cuda -> NCHW cpu
    return x.cpu().permute(0, 3, 1, 2).contiguous()


def close(a, b, rtol=2e-4, atol=2e-5, msg=''):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = err > tol
    assert not bool(bad.any()), f'{msg}: {int(bad.sum())}/{bad.numel()} out of tol, max abs err {float(err.max()):.3e}, ' \
                                f'ref scale {float(b.abs().max()):.3e}, first bad idx {bad.nonzero()[0].tolist()}'


# ---------------------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------------------
CONV_CASES = [
    # B, H, W, Cin, Cout, k, stride, pad, relu_in, relu_out, residual, bn
    (1, 24, 40, 64, 64, 1, 1, 0, False, True, False, True),        # bottleneck conv1
    (1, 24, 40, 64, 64, 3, 1, 1, False, True, False, True),        # bottleneck conv2
    (1, 24, 40, 64, 256, 1, 1, 0, False, True, True, True),        # conv3 + residual + relu
    (1, 24, 40, 256, 128, 3, 2, 1, False, True, False, True),      # strided 3x3
    (1, 24, 40, 256, 512, 1, 2, 0, False, False, False, True),     # strided 1x1 downsample
    (1, 48, 80, 4, 64, 7, 2, 3, False, True, False, True),         # key stem (generic K path)
    (2, 48, 80, 8, 64, 7, 2, 3, False, True, False, True),         # value stem, two objects
    (2, 6, 10, 1600, 512, 3, 1, 1, True, True, False, False),      # fuser block1.conv1 (relu_in/out, split-K)
    (1, 6, 10, 1600, 512, 3, 1, 1, False, False, False, False),    # fuser downsample
    (2, 6, 10, 512, 512, 3, 1, 1, False, False, True, False),      # conv2 + residual
    (1, 30, 54, 1024, 129, 3, 1, 1, False, False, False, False),   # key projection (Cout=129)
    (2, 24, 40, 256, 1, 3, 1, 1, True, False, False, False),       # pred (Cout=1, relu_in)
    (1, 95, 101, 256, 1, 3, 1, 1, True, False, False, False),      # pred on a map of >= 8192 pixels: four pixels per wave, ragged row tail
    (2, 80, 64, 192, 1, 3, 1, 1, False, True, True, False),        # the same kernel with fewer channels than lanes x 4, residual, relu_out
    (2, 6, 10, 260, 256, 1, 1, 0, False, False, True, False),      # g4_conv (generic K, residual chain)
    (1, 60, 108, 256, 256, 3, 1, 1, True, True, False, False),     # decoder up_8_4-like, 128x128 tiles
    (3, 15, 27, 576, 192, 3, 1, 1, False, False, False, False),    # GRU transform, odd spatial size
    (1, 17, 23, 64, 96, 3, 1, 1, False, False, False, False),      # ragged M and N tails
]


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'x'.join(str(int(v)) for v in c))
def test_conv2d(case):
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    B, H, W, Cin, Cout, k, stride, pad, relu_in, relu_out, use_res, bn = case
    gen = g_(hash(case) & 0xffff)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, k, k, generator=gen) * (1.0 / (Cin * k * k)) ** 0.5
    if bn:
        scale = torch.rand(Cout, generator=gen) * 0.5 + 0.75
        shift = torch.randn(Cout, generator=gen) * 0.1
    else:
        scale = torch.ones(Cout)
        shift = torch.randn(Cout, generator=gen) * 0.1
    xin = F.relu(x) if relu_in else x
    ref = F.conv2d(xin, w, None, stride, pad) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    res = torch.randn(ref.shape, generator=gen) if use_res else None
    if use_res:
        ref = ref + res
    if relu_out:
        ref = F.relu(ref)
    cw = ConvWeights(w.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda(), stride, pad)
    out = ops.conv2d(nhwc(x), cw, res=nhwc(res) if use_res else None, relu_in=relu_in, relu_out=relu_out)
    torch.cuda.synchronize()
    close(nchw(out), ref, rtol=2e-4, atol=5e-5, msg=f'conv {case}')


@pytest.mark.parametrize('plan', [(1, 1), (2, 2), (3, 4), (4, 1), (5, 3), (6, 2), (7, 1), (9, 1), (10, 1), (12, 1),
                                  (13, 1), (14, 1), (15, 1), (17, 1), (19, 1), (22, 1),
                                  (23, 1), (24, 1), (25, 1), (26, 1), (27, 1), (28, 1), (29, 1), (30, 1), (31, 1), (32, 1),
                                  (8, 1), (11, 1), (16, 1), (18, 1), (20, 1), (21, 1), (33, 1), (34, 1), (35, 1), (40, 1)])
@pytest.mark.parametrize('shape', [(1, 30, 54, 256, 128), (2, 15, 27, 64, 96), (1, 17, 23, 32, 64)])
def test_conv2d_every_plan(plan, shape):
    """Every tile / split-K / Winograd plan the autotuner may pick computes the same 3x3 convolution - and so does a code that
    does not apply here and falls back: 16 (no fp16 operand in the fp32 mode), 35 / 40 (pointwise streaming codes on a 3x3)."""
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    B, H, W, Cin, Cout = shape
    gen = g_(Cin + Cout + H)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * (1.0 / (Cin * 9)) ** 0.5
    shift = torch.randn(Cout, generator=gen) * 0.1
    scale = torch.rand(Cout, generator=gen) * 0.5 + 0.75
    res = torch.randn(B, Cout, H, W, generator=gen)
    ref = F.relu(F.conv2d(F.relu(x), w, None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res)
    cw = ConvWeights(w.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda(), 1, 1)
    assert cw.wu is not None
    out = ops.conv2d(nhwc(x), cw, res=nhwc(res), relu_in=True, relu_out=True, plan=plan)
    torch.cuda.synchronize()
    close(nchw(out), ref, rtol=2e-4, atol=5e-5, msg=f'conv plan {plan} {shape}')


@pytest.mark.parametrize('shape', [(1, 60, 108, 256, 256), (4, 30, 54, 64, 64), (2, 15, 27, 64, 96), (1, 17, 23, 32, 64),
                                   (3, 9, 13, 96, 192), (1, 120, 216, 64, 64)])
def test_streaming_gemm_plans_are_bit_identical_to_the_classic_tiles(shape):
    """The streaming position GEMM (csrc/gemm_stream.hip: LDS-DMA ring, one flat (unit, k-tile) pipeline per workgroup, counted
    vmcnt waits across unit boundaries) contracts in the classic 64x64 kernel's order: every variant (tile x ring) of plans
    23..28 must reproduce plan 19 bit for bit, 29..34 plan 9 - ragged tile rows, Cout = 96 / 192 (masked column blocks),
    Cin = 32 (ONE k-tile per unit: the ring runs NS - 1 units ahead), many units per workgroup."""
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    B, H, W, Cin, Cout = shape
    gen = g_(Cin * 7 + Cout + H)
    x = torch.randn(B, Cin, H, W, generator=gen)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) * (1.0 / (Cin * 9)) ** 0.5
    shift = torch.randn(Cout, generator=gen) * 0.1
    scale = torch.rand(Cout, generator=gen) * 0.5 + 0.75
    res = nhwc(torch.randn(B, Cout, H, W, generator=gen))
    cw = ConvWeights(w.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda(), 1, 1)
    xin = nhwc(x)
    for base, variants in ((19, range(23, 29)), (9, range(29, 35))):
        want = ops.conv2d(xin, cw, res=res, relu_in=True, relu_out=True, plan=(base, 1)).clone()
        for t in variants:
            got = ops.conv2d(xin, cw, res=res, relu_in=True, relu_out=True, plan=(t, 1))
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
                f'plan {t} differs from plan {base} on {shape}: max |d| {float((got - want).abs().max()):.3e}'


@pytest.mark.parametrize('case', [(4, 24, 40, 64, 256, 1, True, True, True), (1, 30, 54, 1024, 256, 1, True, False, True),
                                  (2, 24, 40, 256, 512, 2, False, False, False), (1, 17, 23, 64, 96, 1, False, True, True),
                                  (3, 9, 13, 32, 48, 1, True, True, False)])
def test_streaming_gemm_pointwise_plans(case):
    """Plans 35..40: the pointwise convolution itself on the streaming kernel with the fused epilogue (scale / shift / residual /
    relu, relu-on-load, stride 2) - bit-identical to the classic 64x64 tile (plan 3: same k order, same epilogue arithmetic);
    also through a channel slice of a wider input buffer and with a broadcast residual."""
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    B, H, W, Cin, Cout, stride, relu_in, use_res, relu_out = case
    gen = g_(Cin + 3 * Cout + H)
    wide = torch.randn(B, H, W, Cin + 32, generator=gen).cuda()
    w = torch.randn(Cout, 1, 1, Cin, generator=gen) * (1.0 / Cin) ** 0.5
    cw = ConvWeights(w.cuda(), (torch.rand(Cout, generator=gen) * 0.5 + 0.75).cuda(), (torch.randn(Cout, generator=gen) * 0.1).cuda(), stride, 0)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    for bcast in (False, True):
        res = torch.randn(1 if bcast else B, Ho, Wo, Cout, generator=gen).cuda() if use_res else None
        kw = dict(res=res, relu_in=relu_in, relu_out=relu_out, in_ld=Cin + 32, cin=Cin, res_broadcast=bcast)
        want = ops.conv2d(wide, cw, plan=(3, 1), **kw).clone()
        for t in range(35, 41):
            got = ops.conv2d(wide, cw, plan=(t, 1), **kw)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
                f'plan {t} differs from plan 3 on {case} (broadcast residual {bcast}): max |d| {float((got - want).abs().max()):.3e}'
        if not use_res:
            break


def test_winograd_f4_accuracy_at_a_large_layer():
    """F(4x4,3x3) is what the large 3x3 layers run by default.  With the interpolation points {0, +-3/4, +-3/2, inf} (round 5; the
    textbook +-1, +-2 gave ~1e-5) its error against a fp64 convolution is a few 1e-6 of the output scale - the class of F(2x2) and of
    the direct form's own fp32 summation - and gated there: the 3-object parity clip showed that 1e-5 is NOT harmless
    (profiles/r05_c3_parity_by_plan.txt).  Odd sizes exercise the partial border tiles."""
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    gen = g_(5)
    for (B, H, W, Cin, Cout) in [(1, 60, 108, 256, 256), (2, 61, 107, 64, 128)]:
        x = F.relu(torch.randn(B, Cin, H, W, generator=gen))
        w = torch.randn(Cout, Cin, 3, 3, generator=gen) * (2.0 / (Cin * 9)) ** 0.5
        ref = F.conv2d(x.double(), w.double(), None, 1, 1)
        cw = ConvWeights(w.permute(0, 2, 3, 1).contiguous().cuda(), torch.ones(Cout).cuda(), torch.zeros(Cout).cuda(), 1, 1)
        scale = float(ref.abs().max())
        errs = {}
        for name, plan in (('direct', (3, 1)), ('F2', (9, 1)), ('F4', (19, 1)), ('default', None)):
            out = nchw(ops.conv2d(nhwc(x), cw, plan=plan)).double()
            errs[name] = float((out - ref).abs().max()) / scale
        print(f'{(B, H, W, Cin, Cout)}: max err / scale {errs}')
        assert errs['direct'] < 2e-6 and errs['F2'] < 5e-6 and errs['F4'] < 8e-6 and errs['default'] < 8e-6


def test_conv2d_into_channel_slice_and_strided_input():
    """ldin / ldout: read a channel slice of a wider buffer and write into the middle of a concat buffer."""
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    gen = g_(5)
    wide = torch.randn(1, 12, 20, 96, generator=gen)           # NHWC buffer; conv reads channels [0, 64)
    w = torch.randn(32, 64, 3, 3, generator=gen) * 0.05
    ref = F.conv2d(wide[..., :64].permute(0, 3, 1, 2), w, None, 1, 1)
    cw = ConvWeights(w.permute(0, 2, 3, 1).contiguous().cuda(), torch.ones(32).cuda(), torch.zeros(32).cuda(), 1, 1)
    dst = torch.full((1, 12, 20, 80), 7.0).cuda()
    import ctypes
    from xmem2_amd import _lib
    d = _lib.ConvDesc()
    xw = wide.cuda()
    d.inp = xw.data_ptr(); d.B, d.H, d.W, d.Cin, d.ldin = 1, 12, 20, 64, 96
    d.w = cw.w.data_ptr(); d.Cout, d.KH, d.KW, d.stride, d.pad = 32, 3, 3, 1, 1
    d.scale = cw.scale.data_ptr(); d.shift = cw.shift.data_ptr(); d.res = None; d.ldres = 0
    d.out = dst.data_ptr() + 4 * 16; d.ldout = 80
    lib = _lib.load()
    need = lib.xmem_conv2d_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device='cuda')
    _lib.check(lib.xmem_conv2d_nhwc(ctypes.byref(d), _lib.ptr(ws), need, _lib.stream_ptr()))
    torch.cuda.synchronize()
    got = dst.cpu()
    close(got[..., 16:48].permute(0, 3, 1, 2), ref, msg='slice conv')
    assert bool((got[..., :16] == 7.0).all()) and bool((got[..., 48:] == 7.0).all()), 'neighbouring channels were clobbered'


# ---------------------------------------------------------------------------------------------------------
# pooling / resampling / gates
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 48, 80, 64), (2, 15, 27, 64), (1, 7, 9, 8)])
def test_maxpool(shape):
    from xmem2_amd import ops
    x = torch.randn(*shape, generator=g_(1))
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1)
    close(nchw(ops.maxpool3x3s2(x.cuda())), ref, 0, 0, 'maxpool')


@pytest.mark.parametrize('shape', [(2, 6, 10, 512), (1, 15, 27, 256), (3, 5, 7, 8)])
def test_upsample2x_add(shape):
    from xmem2_amd import ops
    B, h, w, C = shape
    g = torch.randn(*shape, generator=g_(2))
    skip = torch.randn(1, 2 * h, 2 * w, C, generator=g_(3))
    ref = F.interpolate(g.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear', align_corners=False) + skip.permute(0, 3, 1, 2)
    close(nchw(ops.upsample2x_add(g.cuda(), skip.cuda())), ref, 1e-5, 1e-5, 'upsample2x_add')


@pytest.mark.parametrize('r', [2, 4])
def test_area_downsample(r):
    from xmem2_amd import ops
    x = torch.randn(2, 24, 40, 36, generator=g_(4))
    ref = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=1 / r, mode='area')
    close(nchw(ops.area_downsample(x.cuda(), r)), ref, 1e-5, 1e-6, 'area')
    # strided destination (cat(g4, logits) builder)
    dst = torch.zeros(2, 24 // r, 40 // r, 40).cuda()
    ops.area_downsample(x.cuda(), r, out=dst, out_ld=40, out_off=4)
    close(nchw(dst)[:, 4:40], ref, 1e-5, 1e-6, 'area strided')
    assert float(dst[..., :4].abs().max()) == 0.0


def test_copy_channels_broadcast():
    from xmem2_amd import ops
    src = torch.randn(1, 5, 7, 16, generator=g_(6))
    g = torch.randn(3, 5, 7, 8, generator=g_(7))
    dst = torch.zeros(3, 5, 7, 24).cuda()
    ops.copy_channels(src.cuda(), dst, 0)
    ops.copy_channels(g.cuda(), dst, 16)
    ref = torch.cat([src.expand(3, -1, -1, -1), g], 3)
    close(dst, ref, 0, 0, 'copy_channels')


@pytest.mark.parametrize('shape', [(1, 30, 54, 512, 256, 256), (3, 5, 7, 16, 8, 12), (2, 9, 4, 4, 4, 4)])
def test_hidden_update_gather_is_the_four_launches_in_one(shape):
    """HiddenUpdater's concatenated input [g16 | area2(g8) | area4(g4) | area4(logits)] (model/modules.py:49-57) from ONE launch: the
    same bits as copy_channels + three area_downsample calls, F.interpolate(mode='area') within rounding, padding channels untouched."""
    from xmem2_amd import ops
    K, h, w, c16, c8, c4 = shape
    g16 = torch.randn(K, h, w, c16, generator=g_(11)).cuda(); g8 = torch.randn(K, 2 * h, 2 * w, c8, generator=g_(12)).cuda()
    g4 = torch.randn(K, 4 * h, 4 * w, c4, generator=g_(13)).cuda(); lg = torch.randn(K, 4 * h, 4 * w, 1, generator=g_(14)).cuda()
    ld = (c16 + c8 + c4 + 1 + 3) // 4 * 4 + 4
    a = torch.full((K, h, w, ld), 7.0).cuda(); b = a.clone()
    ops.hidden_update_gather(g16, g8, g4, lg, a)
    ops.copy_channels(g16, b, 0)
    ops.area_downsample(g8, 2, out=b, out_ld=ld, out_off=c16)
    ops.area_downsample(g4, 4, out=b, out_ld=ld, out_off=c16 + c8)
    ops.area_downsample(lg, 4, out=b, out_ld=ld, out_off=c16 + c8 + c4)
    assert torch.equal(a, b), f'max |diff| {float((a - b).abs().max()):.3e}'
    n = c16 + c8 + c4 + 1
    assert bool((a[..., n:] == 7.0).all())
    ref = torch.cat([g16.permute(0, 3, 1, 2), F.interpolate(g8.permute(0, 3, 1, 2), scale_factor=0.5, mode='area'),
                     F.interpolate(g4.permute(0, 3, 1, 2), scale_factor=0.25, mode='area'),
                     F.interpolate(lg.permute(0, 3, 1, 2), scale_factor=0.25, mode='area')], 1)
    close(nchw(a)[:, :n], ref.cpu(), 1e-5, 1e-6, 'hidden_update_gather')


@pytest.mark.parametrize('B', [1, 2])
def test_cbam_residual(B, synth_sd, ref_net):
    from xmem2_amd import ops
    p = 'decoder.fuser.attention'
    g = torch.randn(B, 512, 15, 27, generator=g_(8)) * 0.5
    ref = g + ref_net._cbam(g, p)
    params = dict(w1=synth_sd[p + '.ChannelGate.mlp.1.weight'].cuda(), b1=synth_sd[p + '.ChannelGate.mlp.1.bias'].cuda(),
                  w2=synth_sd[p + '.ChannelGate.mlp.3.weight'].cuda(), b2=synth_sd[p + '.ChannelGate.mlp.3.bias'].cuda(),
                  sw=synth_sd[p + '.SpatialGate.spatial.conv.weight'].reshape(2, 7, 7).contiguous().cuda(),
                  sb=synth_sd[p + '.SpatialGate.spatial.conv.bias'].cuda())
    out = ops.cbam_residual(nhwc(g), params)
    close(nchw(out), ref, 1e-4, 1e-5, 'cbam')


def test_gru_gate():
    from xmem2_amd import ops
    v = torch.randn(2, 6, 10, 192, generator=g_(9))
    h = torch.randn(2, 6, 10, 64, generator=g_(10))
    f, u, n = torch.sigmoid(v[..., :64]), torch.sigmoid(v[..., 64:128]), torch.tanh(v[..., 128:])
    ref = f * h * (1 - u) + u * n
    close(ops.gru_gate(v.cuda(), h.cuda()), ref, 1e-5, 1e-6, 'gru')


def test_pack_image_and_value_input():
    from xmem2_amd import ops
    from xmem2_amd.tensor_util import pad_amounts
    img = torch.randn(3, 50, 70, generator=g_(11))
    lw, uw, lh, uh = pad_amounts(50, 70)
    padded, _ = R.pad_divide_by(img, 16)
    out = ops.pack_image(img.cuda(), 50 + lh + uh, 70 + lw + uw, lh, lw)
    close(out[0, ..., :3].permute(2, 0, 1), padded, 0, 0, 'pack_image')
    assert float(out[..., 3].abs().max()) == 0
    masks = (torch.rand(3, 64, 80, generator=g_(12)) > 0.7).float()
    v = ops.pack_value_input(out, masks.cuda()).cpu()
    others = torch.stack([masks[[j for j in range(3) if j != i]].sum(0) for i in range(3)])
    close(v[..., 3], masks, 0, 0, 'mask channel')
    close(v[..., 4], others, 0, 0, 'others channel')
    close(v[..., :3], out[0, ..., :3].cpu().expand(3, -1, -1, -1), 0, 0, 'rgb channels')
    assert float(v[..., 5:].abs().max()) == 0


def test_key_post():
    from xmem2_amd import ops
    proj = torch.randn(1, 6, 10, 132, generator=g_(13))
    key, shr, sel = ops.key_post(proj.cuda(), 64)
    flat = proj.view(60, 132)
    close(key, flat[:, :64], 0, 0, 'key')
    close(shr, flat[:, 64] ** 2 + 1, 1e-6, 1e-6, 'shrinkage')
    close(sel, torch.sigmoid(flat[:, 65:129]), 1e-6, 1e-6, 'selection')


@pytest.mark.parametrize('K', [1, 3])
def test_logits_to_prob_and_aggregate(K):
    from xmem2_amd import ops
    from xmem2_amd.tensor_util import pad_amounts
    H, W = 50, 70
    lw, uw, lh, uh = pad_amounts(H, W)
    h4, w4 = (H + lh + uh) // 4, (W + lw + uw) // 4
    logits = torch.randn(K, h4, w4, generator=g_(14)) * 4
    up = F.interpolate(logits.unsqueeze(0), scale_factor=4, mode='bilinear', align_corners=False)
    _, ref = R.aggregate(torch.sigmoid(up), dim=1, return_logits=True)
    prob, padded = ops.logits_to_prob(logits.cuda(), H, W, lh, lw)
    close(padded, ref[0], 1e-4, 1e-6, 'prob padded')
    close(prob, R.unpad(ref[0], (lw, uw, lh, uh)), 1e-4, 1e-6, 'prob cropped')
    masks = (torch.rand(K, 32, 48, generator=g_(15)) > 0.6).float()
    close(ops.aggregate_masks(masks.cuda()), R.aggregate(masks, dim=0), 1e-5, 1e-7, 'aggregate masks')
    soft = torch.rand(K, 32, 48, generator=g_(16))
    close(ops.aggregate_masks(soft.cuda()), R.aggregate(soft, dim=0), 1e-4, 1e-6, 'aggregate soft')


def test_merge_masks_and_argmax_and_resize():
    from xmem2_amd import ops
    K, H, W = 3, 32, 48
    pred = torch.rand(K, H, W, generator=g_(17))
    mask = (torch.rand(K, H, W, generator=g_(18)) > 0.8).float()
    valid = [1, 3]
    ref_pred = pred.clone()
    ref_pred[:, mask.sum(0) > 0.5] = 0
    ref = mask.clone()
    keep = [i for i in range(K) if (i + 1) not in valid]
    ref[keep] = ref_pred[keep]
    bits = sum(1 << i for i in range(K) if (i + 1) in valid)
    close(ops.merge_masks(pred.cuda(), mask.cuda(), bits), ref, 0, 0, 'merge_masks')
    prob = torch.rand(K + 1, H, W, generator=g_(19))
    assert np.array_equal(ops.argmax_u8(prob.cuda()).cpu().numpy(), torch.argmax(prob, 0).numpy().astype(np.uint8))
    big = F.interpolate(prob.unsqueeze(1), (45, 80), mode='bilinear', align_corners=False)[:, 0]
    close(ops.resize_bilinear(prob.cuda(), (45, 80)), big, 1e-5, 1e-6, 'resize')


def test_layout_transposes():
    from xmem2_amd import ops
    x = torch.randn(2, 37, 9, 11, generator=g_(20))         # NCHW
    y = ops.nchw_to_nhwc(x.cuda())
    close(y, x.permute(0, 2, 3, 1), 0, 0, 'nchw_to_nhwc')
    close(ops.nhwc_to_nchw(y), x, 0, 0, 'nhwc_to_nchw')


# ---------------------------------------------------------------------------------------------------------
# affinity / readout / usage
# ---------------------------------------------------------------------------------------------------------
def _check_topk(w, idx, sim_ref, top_k, tag):
    """Compare as sets: the k-th / (k+1)-th values may tie or be within roundoff, so membership is checked by value."""
    w, idx = w.cpu(), idx.cpu().long()
    HW = sim_ref.shape[2]
    vals_ref, idx_ref = torch.topk(sim_ref[0], top_k, dim=0)              # [k, HW]
    x = vals_ref.exp(); w_ref = (x / x.sum(0, keepdim=True)).t()        # [HW, k] sorted desc
    assert int(idx.min()) >= 0 and int(idx.max()) < sim_ref.shape[1]
    picked = sim_ref[0].t().gather(1, idx)                               # similarity (oracle) of the picked elements
    kth = vals_ref[-1].unsqueeze(1)
    assert bool((picked >= kth - 1e-4 * (1 + kth.abs())).all()), f'{tag}: picked an element below the k-th value'
    for q in range(0, HW, max(1, HW // 50)):
        assert len(set(idx[q].tolist())) == top_k, f'{tag}: duplicate index for query {q}'
    same = (torch.sort(idx, 1)[0] == torch.sort(idx_ref.t(), 1)[0]).all(1).float().mean()
    assert float(same) > 0.97, f'{tag}: only {float(same):.3f} of queries have the identical index set'
    close(torch.sort(w, 1, descending=True)[0], w_ref, 2e-3, 1e-6, tag + ' weights')
    assert float((w.sum(1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize('tag', ['small', 'mid'])
def test_affinity_topk_golden(tag):
    from xmem2_amd import ops
    g = load_golden('op_' + tag)
    mk, ms, qk, qe, mv = (T(g[k]) for k in ('mk', 'ms', 'qk', 'qe', 'mv'))
    sim = R.get_similarity(mk, ms, qk, qe)
    rows = lambda t: t[0].t().contiguous().cuda()
    w, idx, sims = ops.affinity_topk([(rows(mk), ms.view(-1).cuda())], rows(qk), rows(qe), 30, want_sim=True)
    torch.cuda.synchronize()
    _check_topk(w, idx, sim, 30, 'affinity ' + tag)
    close(sims, sim[0].t().gather(1, idx.cpu().long()), 1e-4, 1e-4, 'raw similarities')
    # golden sparse form from the reference run
    close(torch.sort(w.cpu(), 1, descending=True)[0], T(g['topk_w'])[0].t(), 2e-3, 1e-6, 'weights vs golden')
    # sparse readout == dense v @ affinity
    n_obj, cv = mv.shape[0], mv.shape[1]
    out = torch.zeros(n_obj, qk.shape[2], cv).cuda()
    vrows = [[mv[o].t().contiguous().cuda()] for o in range(n_obj)]
    ops.readout_sparse(vrows, w, idx, cv, out, cv, qk.shape[2] * cv)
    close(out.permute(0, 2, 1), T(g['readout']), 2e-3, 2e-4, 'readout vs golden')
    # usage
    n = mk.shape[2]
    use = torch.zeros(n).cuda(); life = torch.full((n,), 1e-7).cuda()
    ops.usage_update(w, idx, 0, n, use, life)
    close(use, T(g['usage'])[0], 2e-3, 1e-5, 'usage vs golden')
    close(life, torch.full((n,), 1.0 + 1e-7), 0, 0, 'life')


@pytest.mark.parametrize('variant', ['se', 's', 'e', 'none'])
def test_affinity_variants_and_segments(variant):
    """selection / shrinkage optional; three ragged segments must behave as their concatenation."""
    from xmem2_amd import ops
    gen = g_(21)
    n_seg, hw, ck = (128, 405 * 3 + 7, 50), 405, 64
    n = sum(n_seg)
    mk = torch.randn(1, ck, n, generator=gen) * 0.9
    ms = torch.rand(1, 1, n, generator=gen) * 3 + 1
    qk = torch.randn(1, ck, hw, generator=gen) * 0.9
    qe = torch.rand(1, ck, hw, generator=gen) * 0.9 + 0.05
    use_s, use_e = variant in ('se', 's'), variant in ('se', 'e')
    sim = R.get_similarity(mk, ms if use_s else None, qk, qe if use_e else None)
    segs, a = [], 0
    for c in n_seg:
        segs.append((mk[0, :, a:a + c].t().contiguous().cuda(), ms[0, 0, a:a + c].contiguous().cuda() if use_s else None))
        a += c
    w, idx, _ = ops.affinity_topk(segs, qk[0].t().contiguous().cuda(), qe[0].t().contiguous().cuda() if use_e else None, 30)
    torch.cuda.synchronize()
    _check_topk(w, idx, sim, 30, 'affinity ' + variant)


@pytest.mark.parametrize('n,hw,k', [(51840, 1620, 30), (30, 40, 30), (8100 + 128, 1350, 30), (5000, 100, 8), (3000, 70, 64)])
def test_affinity_sizes(n, hw, k):
    """The benchmark size (32 frames x 1620), N == top_k, other top_k values."""
    from xmem2_amd import ops
    gen = g_(n + hw)
    mk = torch.randn(1, 64, n, generator=gen) * 0.9
    ms = torch.rand(1, 1, n, generator=gen) * 3 + 1
    qk = torch.randn(1, 64, hw, generator=gen) * 0.9
    qe = torch.rand(1, 64, hw, generator=gen) * 0.9 + 0.05
    sim = R.get_similarity(mk, ms, qk, qe)
    w, idx, _ = ops.affinity_topk([(mk[0].t().contiguous().cuda(), ms.view(-1).cuda())], qk[0].t().contiguous().cuda(),
                                  qe[0].t().contiguous().cuda(), k)
    torch.cuda.synchronize()
    _check_topk(w, idx, sim, k, f'affinity n={n}')


def test_affinity_errors():
    from xmem2_amd import ops
    k = torch.randn(20, 64).cuda()
    with pytest.raises(RuntimeError):
        ops.affinity_topk([(k, None)], torch.randn(10, 64).cuda(), None, 30)      # N < top_k, like torch.topk


def test_affinity_ties_are_exact():
    """Duplicate memory rows give exactly tied similarities; the result must still be a valid top-k set."""
    from xmem2_amd import ops
    gen = g_(33)
    base = torch.randn(40, 64, generator=gen)
    mk = base.repeat(4, 1)                                  # every row appears 4 times
    qk = torch.randn(50, 64, generator=gen)
    w, idx, sims = ops.affinity_topk([(mk.cuda(), None)], qk.cuda(), None, 30, want_sim=True)
    sim = R.get_similarity(mk.t().unsqueeze(0), None, qk.t().unsqueeze(0), None)
    vals_ref = torch.topk(sim[0], 30, dim=0)[0].t()
    close(torch.sort(sims.cpu(), 1, descending=True)[0], vals_ref, 1e-5, 1e-5, 'tied values')
    for q in range(50):
        assert len(set(idx[q].tolist())) == 30


def test_affinity_optimistic_overflow_falls_back_exactly():
    """>56 near-duplicates of a query inside one split of a large memory overflow the optimistic candidate buffers; the
    flagged query tiles are redone by the safe kernel (global-scratch buffers) and the result stays exact."""
    from xmem2_amd import ops
    gen = g_(77)
    n, hw = 16384, 200
    mk = torch.randn(n, 64, generator=gen) * 0.9
    ms = torch.rand(n, generator=gen) + 1
    qk = torch.randn(hw, 64, generator=gen) * 0.9
    qe = torch.rand(hw, 64, generator=gen) * 0.9 + 0.05
    for j, q in enumerate((3, 70, 150)):                       # three queries in three different query tiles
        lo = 2000 + 4000 * j
        mk[lo:lo + 120] = qk[q] + torch.randn(120, 64, generator=gen) * 0.02
    w, idx, sims = ops.affinity_topk([(mk.cuda(), ms.cuda())], qk.cuda(), qe.cuda(), 30, want_sim=True)
    sim = R.get_similarity(mk.t().unsqueeze(0), ms.view(1, 1, -1), qk.t().unsqueeze(0), qe.t().unsqueeze(0))[0]   # [n, hw]
    rv, ri = torch.topk(sim, 30, dim=0)
    close(sims, rv.t(), 1e-4, 1e-4, 'top-k values after fallback')
    for q in (3, 70, 150, 0, 199):
        assert set(idx[q].tolist()) == set(ri[:, q].tolist())
    aff = R.do_softmax(sim.unsqueeze(0), top_k=30)[0]            # [n, hw]
    dense = torch.zeros(hw, n)
    dense.scatter_(1, idx.cpu().long(), w.cpu())
    close(dense, aff.t(), 2e-4, 1e-7, 'affinity after fallback')


@pytest.mark.parametrize('filter16', ['1', '0'])
def test_affinity_hint_never_changes_the_result(filter16, monkeypatch):
    """xmem_affinity_topk_hinted: the hint (previous top-k indices) only bounds the k-th similarity from below.  Results
    with a perfect hint, a hint from a DIFFERENT segment layout, a hint of k' > k indices, a garbage hint (all zeros:
    fewer than k distinct elements -> no bound -> full exact scan) and a misleading hint (the WORST elements: a very loose
    bound -> candidate lists overflow -> self-tightening lists / full exact scan) must all equal the un-hinted result BIT FOR
    BIT - with the fp16-filter + exact-refine pipeline (default for hinted calls) and with the fp32 select (FILTER16=0)."""
    from xmem2_amd import ops
    monkeypatch.setenv('XMEM_AFFINITY_FILTER16', filter16)
    gen = g_(91)
    n, hw, gw = 20000, 300, 20
    mk = torch.randn(n, 64, generator=gen) * 0.9
    ms = torch.rand(n, generator=gen) * 3 + 1
    qk = torch.randn(hw, 64, generator=gen) * 0.9
    qe = torch.rand(hw, 64, generator=gen) * 0.9 + 0.05
    cuts = [0, 7000, 7000, 20000]                                  # three slots, the middle one empty
    segs = [(mk[a:b].cuda() if b > a else None, ms[a:b].cuda() if b > a else None) for a, b in zip(cuts[:-1], cuts[1:])]
    sizes = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    w0, i0, s0 = ops.affinity_topk(segs, qk.cuda(), qe.cuda(), 30, want_sim=True)
    sim = R.get_similarity(mk.t().unsqueeze(0), ms.view(1, 1, -1), qk.t().unsqueeze(0), qe.t().unsqueeze(0))
    _check_topk(w0, i0, sim, 30, 'un-hinted')
    worst = torch.topk(sim[0], 40, dim=0, largest=False)[1].t().contiguous().int().cuda()       # [hw, 40]
    _, i64, _ = ops.affinity_topk(segs, qk.cuda(), qe.cuda(), 64)
    hints = {
        'perfect': (i0, sizes, gw),
        'perfect, no neighbours': (i0, sizes, 0),
        'k=64 hint': (i64, sizes, gw),
        'other layout': (i0, [5000, 3000, 12000], gw),
        'garbage': (torch.zeros_like(i0), sizes, gw),
        'misleading': (worst, sizes, 0),
    }
    for name, h in hints.items():
        w, i, sv = ops.affinity_topk(segs, qk.cuda(), qe.cuda(), 30, want_sim=True, hint=h)
        torch.cuda.synchronize()
        assert torch.equal(sv, s0), f'{name}: similarities differ from the un-hinted call'
        assert torch.equal(i, i0) and torch.equal(w, w0), f'{name}: indices / weights differ from the un-hinted call'


@pytest.mark.parametrize('case', ['fp16 overflow', 'fp16 subnormal', 'huge shrinkage', 'ties', 'no selection'])
def test_affinity_filter16_is_exact_on_hostile_values(case):
    """The fp16 filter may only DROP a pair when a rigorous bound proves it is outside the top-k.  Values beyond the fp16 range
    (x^2 > 65504), in its subnormal range (x^2 ~ 1e-6), shrinkages that blow the bound up, and exact ties (every element a
    candidate) must still give the un-hinted fp32 result bit for bit."""
    from xmem2_amd import ops
    gen = g_(93)
    n, hw, gw, k = 12000, 260, 20, 30
    mk = torch.randn(n, 64, generator=gen) * 0.9
    ms = torch.rand(n, generator=gen) * 3 + 1
    qk = torch.randn(hw, 64, generator=gen) * 0.9
    qe = torch.rand(hw, 64, generator=gen) * 0.9 + 0.05
    if case == 'fp16 overflow':
        mk[::7] *= 400.0                                           # x^2 up to ~1e6: inf in fp16
        qk[::5] *= 300.0
    elif case == 'fp16 subnormal':
        mk *= 1e-3; qk *= 1e-3; qe *= 1e-2
    elif case == 'huge shrinkage':
        ms[::11] = 5e4
    elif case == 'ties':
        mk[:] = mk[:40].repeat(n // 40, 1)                          # 300 copies of 40 rows: every query has 300-fold ties
        ms[:] = 2.0
    qe_arg = None if case == 'no selection' else qe.cuda()
    segs = [(mk[:5000].cuda(), ms[:5000].cuda()), (mk[5000:].cuda(), ms[5000:].cuda())]
    sizes = [5000, n - 5000]
    w0, i0, s0 = ops.affinity_topk(segs, qk.cuda(), qe_arg, k, want_sim=True)
    for name, h in {'perfect': (i0, sizes, gw), 'shifted': (torch.roll(i0, 1, 0).contiguous(), sizes, 0)}.items():
        w, i, sv = ops.affinity_topk(segs, qk.cuda(), qe_arg, k, want_sim=True, hint=h)
        torch.cuda.synchronize()
        assert torch.equal(sv, s0), f'{case} / {name}: similarities differ from the un-hinted call'
        assert torch.equal(i, i0), f'{case} / {name}: indices differ'
        same = torch.equal(w, w0) or bool(((w == w0) | (torch.isnan(w) & torch.isnan(w0))).all())
        assert same, f'{case} / {name}: weights differ'


# ---------------------------------------------------------------------------------------------------------
# consolidation kernels
# ---------------------------------------------------------------------------------------------------------
def test_similarity_dense_softmax_weighted_rows():
    from xmem2_amd import ops
    gen = g_(40)
    n, P, cv = 2500, 64, 128
    mk = torch.randn(1, 64, n, generator=gen) * 0.9
    ms = torch.rand(1, 1, n, generator=gen) * 3 + 1
    pk = torch.randn(1, 64, P, generator=gen) * 0.9
    pe = torch.rand(1, 64, P, generator=gen) * 0.9 + 0.05
    sim = R.get_similarity(mk, ms, pk, pe)                        # [1, n, P]
    got = ops.similarity_dense(mk[0].t().contiguous().cuda(), ms.view(-1).cuda(), pk[0].t().contiguous().cuda(),
                               pe[0].t().contiguous().cuda())
    close(got, sim[0].t(), 1e-4, 1e-4, 'similarity_dense')
    cnt = 1700
    aff_ref = R.do_softmax(sim[:, -cnt:])                          # softmax over candidates
    aff = ops.softmax_rows_suffix(got.clone(), cnt)
    close(aff[:, n - cnt:], aff_ref[0].t(), 2e-3, 1e-9, 'softmax suffix')
    assert float(aff[:, :n - cnt].abs().max()) == 0
    V = torch.randn(cnt, cv, generator=gen)
    ref = (V.t() @ aff_ref[0]).t()                                 # gv @ affinity
    close(ops.weighted_rows(aff, cnt, V.cuda()), ref, 2e-3, 1e-5, 'weighted rows')
    s = ms.view(-1)[n - cnt:]
    close(ops.weighted_rows(aff, cnt, s.cuda()).view(-1), (s.view(1, -1) @ aff_ref[0]).view(-1), 2e-3, 1e-5, 'weighted shrinkage')


def test_topk_1d_and_select_and_gather():
    from xmem2_amd import ops
    gen = g_(41)
    v = torch.rand(8100, generator=gen)
    vals, idx = ops.topk_1d(v.cuda(), 128, largest=True)
    rv, ri = torch.topk(v, 128)
    close(vals, rv, 0, 0, 'topk values'); assert idx.cpu().tolist() == ri.tolist()
    vals, idx = ops.topk_1d(v.cuda(), 77, largest=False)
    rv, ri = torch.topk(v, 77, largest=False)
    close(vals, rv, 0, 0, 'bottomk values'); assert idx.cpu().tolist() == ri.tolist()
    thr = vals[76:77]
    sel, cnt = ops.select_greater(v.cuda(), thr)
    keep = (v > rv[-1]).nonzero().flatten()
    assert int(cnt.item()) == keep.numel() and sel[:keep.numel()].cpu().tolist() == keep.tolist()
    src = torch.randn(500, 24, generator=gen)
    pick = torch.randint(0, 500, (77,), generator=gen).to(torch.int32)
    close(ops.gather_rows(src.cuda(), pick.cuda()), src[pick.long()], 0, 0, 'gather')
    u, l = torch.rand(100, generator=gen), torch.rand(100, generator=gen) + 0.5
    close(ops.usage_ratio(u.cuda(), l.cuda()), u / l, 1e-6, 0, 'usage ratio')


# ---------------------------------------------------------------------------------------------------------
# BASELINE configs 4 / 5 sizes: the oracle cannot materialise N x HW (13 GB / 136 GB), so a random subset of the
# queries is checked exactly and size-independent properties are checked for all of them.
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,hw,nseg', [(921600, 3600, 3), (4177920, 8160, 2)], ids=['C4_720p_256frames', 'C5_1080p_512frames'])
def test_affinity_large_memory(n, hw, nseg):
    from xmem2_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(n)
    mk = torch.randn(n, 64, generator=gen, device='cuda') * 0.9
    ms = torch.rand(n, generator=gen, device='cuda') * 3 + 1
    qk = torch.randn(hw, 64, generator=gen, device='cuda') * 0.9
    qe = torch.rand(hw, 64, generator=gen, device='cuda') * 0.9 + 0.05
    cuts = [0] + sorted(torch.randint(1, n, (nseg - 1,)).tolist()) + [n]
    segs = [(mk[a:b], ms[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    w, idx, sims = ops.affinity_topk(segs, qk, qe, 30, want_sim=True)
    torch.cuda.synchronize()
    w, idx, sims = w.cpu(), idx.cpu().long(), sims.cpu()
    assert float((w.sum(1) - 1).abs().max()) < 1e-5
    assert bool((sims[:, :-1] >= sims[:, 1:]).all()), 'top-k not sorted'
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    assert all(len(set(idx[q].tolist())) == 30 for q in range(0, hw, 97))
    pick = torch.randperm(hw)[:48]
    mkc, msc = mk.cpu(), ms.cpu()
    sim = R.get_similarity(mkc.t().unsqueeze(0), msc.view(1, 1, -1), qk.cpu()[pick].t().unsqueeze(0), qe.cpu()[pick].t().unsqueeze(0))
    vals_ref, idx_ref = torch.topk(sim[0], 30, dim=0)
    close(sims[pick], vals_ref.t(), 1e-4, 1e-4, 'large-N top-k values')
    same = (torch.sort(idx[pick], 1)[0] == torch.sort(idx_ref.t(), 1)[0]).all(1).float().mean()
    assert float(same) > 0.9, f'only {float(same):.2f} of the sampled queries have the identical index set'
    # the readout stays sparse: k rows per query regardless of N
    out = torch.zeros(1, hw, 512).cuda()
    V = torch.randn(n, 512, device='cuda', generator=gen) if n < 2_000_000 else None
    if V is not None:
        ops.readout_sparse([[V[a:b] for a, b in zip(cuts[:-1], cuts[1:])]], w.cuda(), idx.int().cuda(), 512, out, 512, hw * 512)
        q0 = int(pick[0])
        ref = (w[q0].unsqueeze(1) * V[idx[q0].cuda()].cpu()).sum(0)
        close(out[0, q0], ref, 1e-3, 1e-5, 'large-N readout')


@pytest.mark.parametrize('plan', [(0, 0), (3, 1), (6, 2), (9, 1), (14, 1)], ids=['auto', 'direct', 'splitk', 'winograd', 'wino_fused'])
def test_conv_broadcast_residual_and_channel_slice_input(plan):
    """res_broadcast: one [1,Ho,Wo,C] image added to every batch element; input = a channel slice of a wider buffer
    (the per-object half of the fuser convolutions): equals the convolution over the concatenation."""
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    gen = g_(91)
    K, h, w, cx, cg, co = 3, 12, 20, 64, 96, 64
    x = torch.randn(1, h, w, cx, generator=gen)
    g = torch.randn(K, h, w, cg, generator=gen)
    wt = torch.randn(co, cx + cg, 3, 3, generator=gen) * 0.05
    bias = torch.randn(co, generator=gen)
    cat = torch.cat([x.expand(K, -1, -1, -1), g], 3)                                   # [K,h,w,cx+cg]
    ref = F.conv2d(F.relu(cat.permute(0, 3, 1, 2)), wt, bias, padding=1).relu().permute(0, 2, 3, 1)
    wk = wt.permute(0, 2, 3, 1).contiguous().cuda()
    ones, zeros = torch.ones(co).cuda(), torch.zeros(co).cuda()
    wx = ConvWeights(wk[..., :cx].contiguous(), ones, zeros, 1, 1)
    wg = ConvWeights(wk[..., cx:].contiguous(), ones, bias.cuda(), 1, 1)
    catd = cat.cuda().contiguous()
    sx = ops.conv2d(x.cuda(), wx, relu_in=True, plan=plan)
    got = ops.conv2d(catd[..., cx:], wg, relu_in=True, relu_out=True, res=sx, res_broadcast=True, in_ld=cx + cg, cin=cg, plan=plan)
    close(got, ref, 2e-4, 2e-4, f'broadcast residual plan {plan}')


def test_pack_image_u8_matches_totensor_normalize():
    """Device ingest (xmem_pack_image_u8) == ToTensor + Normalize + pad_divide_by on the host, bit for bit, and step() on a
    uint8 H x W x 3 frame == step() on the reference-format float frame."""
    from xmem2_amd import ops
    from xmem2_amd.tensor_util import pad_amounts
    g = torch.Generator().manual_seed(0)
    H, W = 50, 70
    u8 = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)
    u8[0, 0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    mean = np.array(ops.IM_MEAN, np.float32); std = np.array(ops.IM_STD, np.float32)
    want = (u8.numpy().astype(np.float32) / np.float32(255.0) - mean) / std                # H x W x 3
    tw = (u8.permute(2, 0, 1).float().div(255)).sub_(torch.tensor(ops.IM_MEAN).view(3, 1, 1)).div_(torch.tensor(ops.IM_STD).view(3, 1, 1))
    assert np.array_equal(want, tw.permute(1, 2, 0).numpy())                               # numpy == torchvision's op order
    lw, uw, lh, uh = pad_amounts(H, W, 16)
    got = ops.pack_image_u8(u8.cuda(), H + lh + uh, W + lw + uw, lh, lw).cpu().numpy()[0]
    ref = np.zeros((H + lh + uh, W + lw + uw, 4), np.float32)
    ref[lh:lh + H, lw:lw + W, :3] = want
    assert np.array_equal(got, ref)
    flt = ops.pack_image(tw.cuda().contiguous(), H + lh + uh, W + lw + uw, lh, lw).cpu().numpy()[0]
    assert np.array_equal(got, flt)
    with pytest.raises(RuntimeError):
        ops.pack_image_u8(u8, 64, 80, 0, 0)                                                 # host tensor: no CPU path
