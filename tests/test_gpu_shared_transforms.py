"""Shared Winograd transforms (ops.conv2d_shared / ops.conv2d_folded, include/xmem_hip.h SHARED WINOGRAD TRANSFORMS) against the
same convolutions issued one by one with ops.conv2d under the same plans.  Storing and reloading an fp32 value is lossless and the
shared kernels perform, per channel, the operations of the separate transforms in their order, so every comparison is torch.equal.

Geometries: 1 x 7 x 9 and 2 x 13 x 6 (ragged in both directions: edge tiles clamped), 1 x 8 x 12 (whole tiles).  Inputs: 64 channels
contiguous, and a channel slice at offset 64 of a 100-channel buffer - 36 channels wide (the Winograd forms need Cin % 32 == 0, so this
one resolves to the direct form under any plan code and the wrapper must decline and still give the same bits) and 32 channels wide
(so that a slice also goes through the shared kernel).  F(4x4) is forced with `plan=`: these maps are far below the size at which
the heuristic picks it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GEOMETRIES = [(1, 7, 9), (2, 13, 6), (1, 8, 12)]
INPUTS = [(36, 100, 64), (32, 100, 64), (64, 64, 0)]          # Cin, in_ld, channel offset
F4_PLANS = [(19, 1), (23, 1), (17, 1)]                        # F(4x4): 64x64 tile, 64x64 streaming ring 3, 128x128 tile
JUNK = 7.0

_cache = {}


def weights(cout, cin, seed):
    from xmem2_amd import ops
    key = (cout, cin, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * seed + cout + cin)
        w = (torch.randn(cout, 3, 3, cin, generator=g) * (2.0 / (9 * cin)) ** 0.5).cuda().contiguous()
        scale = (1.0 + 0.25 * torch.randn(cout, generator=g)).cuda()
        shift = (0.1 * torch.randn(cout, generator=g)).cuda()
        _cache[key] = ops.ConvWeights(w, scale, shift, 1, 1)
    return _cache[key]


def make_input(B, H, W, cin, ld, off, seed):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((B, H, W, ld), JUNK)
    buf[..., off:off + cin] = torch.randn(B, H, W, cin, generator=g)
    buf = buf.cuda()
    return buf[..., off:off + cin], ld


def rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def stats():
    from xmem2_amd import ops
    return dict(ops.SHARED_STATS)


@pytest.mark.parametrize('flags', [(True, False), (False, True, False)], ids=['relu-raw', 'raw-relu-raw'])
@pytest.mark.parametrize('cin,ld,off', INPUTS, ids=['slice36', 'slice32', 'cin64'])
@pytest.mark.parametrize('B,H,W', GEOMETRIES, ids=['1x7x9', '2x13x6', '1x8x12'])
def test_shared_input_transform_equals_separate_convolutions(B, H, W, cin, ld, off, flags):
    from xmem2_amd import ops
    x, in_ld = make_input(B, H, W, cin, ld, off, seed=B * 100 + H)
    couts = (32, 132, 64)[:len(flags)]
    res1 = rand((B, H, W, couts[1]), 5)
    convs = []
    for i, (relu_in, cout) in enumerate(zip(flags, couts)):
        kw = dict(cw=weights(cout, cin, i), relu_in=relu_in, relu_out=(i == 0), plan=F4_PLANS[i])
        if i == 1:
            kw['res'] = res1
        convs.append(kw)
    ref = [ops.conv2d(x, in_ld=in_ld, cin=cin, **kw) for kw in convs]
    before = stats()
    got = ops.conv2d_shared(x, convs, in_ld=in_ld, cin=cin)
    after = stats()
    took = after['shared_input'] - before['shared_input']
    assert took == (1 if cin % 32 == 0 else 0) and after['separate'] - before['separate'] == 1 - took
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and torch.equal(a, b), f'convolution {i}: {int((a != b).sum())} of {a.numel()} values differ'


def test_shared_input_declines_when_one_plan_is_direct():
    from xmem2_amd import ops
    B, H, W, cin = 2, 13, 6, 64
    x, _ = make_input(B, H, W, cin, cin, 0, seed=3)
    convs = [dict(cw=weights(32, cin, 0), relu_in=True, plan=(19, 1)), dict(cw=weights(132, cin, 1), plan=(3, 1))]     # code 3: direct
    ref = [ops.conv2d(x, **kw) for kw in convs]
    before = stats()
    got = ops.conv2d_shared(x, convs)
    after = stats()
    assert after['shared_input'] == before['shared_input'] and after['separate'] == before['separate'] + 1
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_shared_input_same_flag_shares_one_v():
    """Both consumers raw: the plain input transform once, one V."""
    from xmem2_amd import ops
    x, _ = make_input(1, 7, 9, 64, 64, 0, seed=4)
    convs = [dict(cw=weights(32, 64, 0), plan=(19, 1)), dict(cw=weights(64, 64, 2), plan=(23, 1), relu_out=True)]
    ref = [ops.conv2d(x, **kw) for kw in convs]
    before = stats()
    got = ops.conv2d_shared(x, convs)
    assert stats()['shared_input'] == before['shared_input'] + 1
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize('relu_out', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('branch_res', ['plain', 'broadcast', 'none'])
@pytest.mark.parametrize('B,H,W', GEOMETRIES, ids=['1x7x9', '2x13x6', '1x8x12'])
def test_folded_branch_equals_separate_convolutions(B, H, W, branch_res, relu_out):
    """conv2(relu(conv1(relu(x)))) + downsample(x): the block of network._group_res / _fusion, written into a channel slice."""
    from xmem2_amd import ops
    cin, mid, cout, out_ld, out_off = 64, 32, 132, 200, 60
    x, _ = make_input(B, H, W, cin, cin, 0, seed=7 + H)
    conv1, down, conv2 = weights(mid, cin, 0), weights(cout, cin, 1), weights(cout, mid, 2)
    res = None if branch_res == 'none' else rand((1 if branch_res == 'broadcast' else B, H, W, cout), 11)
    bkw = dict(cw=down, res=res, res_broadcast=(branch_res == 'broadcast'), plan=(23, 1))
    ckw = dict(cw=conv1, relu_in=True, relu_out=True, plan=(19, 1))

    def out_buffer():
        buf = torch.full((B, H, W, out_ld), JUNK, device='cuda')
        return buf, buf[..., out_off:out_off + cout]

    o = ops.conv2d(x, **ckw)
    r = ops.conv2d(x, **bkw)
    ref_buf, ref_view = out_buffer()
    ops.conv2d(o, conv2, res=r, relu_out=relu_out, out=ref_view, out_ld=out_ld, plan=(17, 1))
    before = stats()
    o2, branch = ops.conv2d_shared(x, [ckw, bkw], defer=1)
    assert isinstance(branch, ops.DeferredConv) and torch.equal(o2, o)
    got_buf, got_view = out_buffer()
    ops.conv2d_folded(o2, conv2, branch, relu_out=relu_out, out=got_view, out_ld=out_ld, plan=(17, 1))
    after = stats()
    assert after['shared_input'] == before['shared_input'] + 1 and after['folded'] == before['folded'] + 1
    assert after['separate'] == before['separate']
    assert torch.equal(got_buf, ref_buf), f'{int((got_buf != ref_buf).sum())} of {got_buf.numel()} values differ'
    assert bool((got_buf[..., :out_off] == JUNK).all()) and bool((got_buf[..., out_off + cout:] == JUNK).all())


def test_folded_declines_a_main_convolution_that_is_not_f4():
    """The branch was deferred, the main convolution runs the direct form: the branch is finished by its own output transform."""
    from xmem2_amd import ops
    B, H, W, cin, mid, cout = 2, 13, 6, 64, 32, 132
    x, _ = make_input(B, H, W, cin, cin, 0, seed=9)
    conv1, down, conv2 = weights(mid, cin, 0), weights(cout, cin, 1), weights(cout, mid, 2)
    ckw, bkw = dict(cw=conv1, relu_in=True, relu_out=True, plan=(19, 1)), dict(cw=down, plan=(19, 1))
    ref = ops.conv2d(ops.conv2d(x, **ckw), conv2, res=ops.conv2d(x, **bkw), plan=(3, 1))
    o, branch = ops.conv2d_shared(x, [ckw, bkw], defer=1)
    before = stats()
    got = ops.conv2d_folded(o, conv2, branch, plan=(3, 1))
    after = stats()
    assert after['folded'] == before['folded'] and after['separate'] == before['separate'] + 1
    assert torch.equal(got, ref)


# ---- network level ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net_f4_everywhere(synth_sd):
    """A network of its own at the 96 x 128 size of tests/golden/net_96x128.npz.  Its maps (6 x 8 at 1/16) are below the size from which
    the heuristic picks F(4x4), and the shared transforms apply to F(4x4) plans: for this module the heuristic picks it from one pixel
    (on both sides of every comparison), and the plans chosen meanwhile are forgotten afterwards."""
    from xmem2_amd import conv_plan
    from xmem2_amd.network import XMem
    saved, saved_min = conv_plan.FP32.chosen, conv_plan.F4_MIN_PIXELS
    conv_plan.FP32.chosen, conv_plan.F4_MIN_PIXELS = {}, 1
    try:
        net = XMem({'key_dim': 64, 'value_dim': 512, 'hidden_dim': 64, 'precision': 'fp32'}, None).to('cuda').eval()
        net.load_weights(synth_sd)
        yield net
    finally:
        conv_plan.FP32.chosen, conv_plan.F4_MIN_PIXELS = saved, saved_min


def _spy(monkeypatch):
    from xmem2_amd import ops
    calls = {'shared': 0, 'folded': 0}
    shared, folded = ops.conv2d_shared, ops.conv2d_folded

    def spy_shared(*a, **k):
        calls['shared'] += 1
        return shared(*a, **k)

    def spy_folded(*a, **k):
        calls['folded'] += 1
        return folded(*a, **k)

    monkeypatch.setattr(ops, 'conv2d_shared', spy_shared)
    monkeypatch.setattr(ops, 'conv2d_folded', spy_folded)
    return calls


def _flat(out):
    flat = []
    for t in out:
        if isinstance(t, (tuple, list)):
            flat += _flat(t)
        elif t is not None:
            flat.append(t.clone())
    return flat


def _key_pass(net, on, batch=2):
    from conftest import load_golden
    from xmem2_amd import ops
    frame = torch.from_numpy(load_golden('net_96x128')['frame']).cuda()[0]        # [3, 96, 128]
    image4 = torch.cat([ops.pack_image((frame * (1.0 - 0.25 * i)).contiguous(), 96, 128, 0, 0) for i in range(batch)], 0)
    net.shared_transforms = on
    # a slot per side: each side captures stages of its own
    return net.encode_key_nhwc(image4, need_sk=True, need_ek=True, with_skips=True, slot=4 + int(on), inline_skips=True)


def test_network_key_pass_is_bit_identical_with_shared_transforms(net_f4_everywhere, monkeypatch):
    from xmem2_amd import ops
    net = net_f4_everywhere
    calls, before = _spy(monkeypatch), stats()
    on = _flat(_key_pass(net, True))
    after = stats()
    assert calls['shared'] == 2 and after['shared_input'] - before['shared_input'] == 2      # warm-up + capture
    assert after['separate'] == before['separate'], 'the key pass went through a fallback'
    off = _flat(_key_pass(net, False))
    assert calls['shared'] == 2 and stats() == after
    assert len(on) == len(off) == 10          # key, shrinkage, selection, f16, f8, f4 + the four extras
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and torch.equal(a, b), f'output {i} differs'


@pytest.mark.parametrize('prefetched', [True, False], ids=['prefetched', 'unhinted'])
@pytest.mark.parametrize('K', [1, 2])
def test_network_segment_is_bit_identical_with_shared_transforms(net_f4_everywhere, monkeypatch, K, prefetched):
    """Prefetched: the f16 half of the fuser arrives from the key pass (network._fusion, `pre`); un-hinted with two objects: the
    shared-x path; un-hinted with one object: block1 as a plain residual block over the whole concatenation."""
    net = net_f4_everywhere
    calls = _spy(monkeypatch)
    h, w = 6, 8
    results = {}
    for on in (True, False):
        key, shr, sel, f16, f8, f4, extras = _key_pass(net, on, batch=1)
        f16, f8, f4 = f16.clone(), f8.clone(), f4.clone()
        skips = tuple(t.clone() for t in extras) if prefetched else None
        net.shared_transforms = on
        cat16 = torch.zeros((K, h, w, 1024 + 512 + 64), device='cuda')
        cat16[..., 1024:1536] = rand((K, h, w, 512), 21)
        hidden = 0.3 * rand((K, h, w, 64), 22)
        n0, before = dict(calls), stats()
        new_hidden, prob, prob_padded = net.segment_nhwc(f16, f8, f4, cat16, hidden, (96, 128), (0, 0), h_out=True, skips=skips,
                                                         slot=6 + int(on), owner=0)
        after = stats()
        if on:
            # fuser block1 and up_16_8.out_conv: one shared input transform and one folded output transform each, warm-up + capture
            assert calls['shared'] - n0['shared'] == 4 and calls['folded'] - n0['folded'] == 4
            assert after['shared_input'] - before['shared_input'] == 4 and after['folded'] - before['folded'] == 4
            assert after['separate'] == before['separate'], 'the decoder went through a fallback'
        else:
            assert calls == n0 and after == before
        results[on] = (new_hidden.clone(), prob.clone(), prob_padded.clone())
    for a, b, name in zip(results[True], results[False], ('hidden', 'prob', 'prob_padded')):
        assert torch.equal(a, b), name
