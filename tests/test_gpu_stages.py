"""Weights replaced -> captured stages dropped (hipnet.HipNet._weights_replaced), for the three networks: a network that has captured a
stage and then loads other weights must compute what a fresh network with those weights computes, bit for bit.  A stage that survived
the reload would replay kernels holding the addresses of the freed weight tensors."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _shifted(sd, shifts):
    sd2 = dict(sd)
    for name, by in shifts.items():
        sd2[name] = sd[name] + by
    return sd2


def _reload_check(make, run, sd, sd2, cache='_stages'):
    """A: load sd, run twice (one capture, one replay), load sd2, run.  B: fresh, loads sd2 only.  `run(net)` -> tuple of tensors (clones)."""
    a = make().load_weights(sd)
    stages = getattr(a, cache)
    first = run(a)
    again = run(a)
    assert a.captures == 1 and len(stages) == 1
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    a.load_weights(sd2)
    assert len(stages) == 0, 'a captured stage outlived the weights it was captured against'
    got = run(a)
    assert a.captures == 2 and len(stages) == 1, 'the reload costs exactly one new capture of the stage'
    want = run(make().load_weights(sd2))
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), f'output {i}: the reloaded network differs from a fresh one with the same weights'
    assert not torch.equal(got[0], first[0]), 'the new weights must change the output, or the test shows nothing'
    return a, first, got


def test_xmem_reload_recaptures(synth_sd):
    from xmem2_amd import ops
    from xmem2_amd.network import XMem
    sd2 = _shifted(synth_sd, {'key_proj.key_proj.bias': 0.25, 'key_proj.e_proj.bias': 0.125})
    g = torch.Generator().manual_seed(7)
    image4 = ops.pack_image(torch.randn(3, 64, 96, generator=g).cuda(), 64, 96, 0, 0)       # a 4 x 6 map at 1/16 resolution
    make = lambda: XMem({'key_dim': 64, 'value_dim': 512, 'hidden_dim': 64, 'precision': 'fp32'}, None).to('cuda').eval()
    run = lambda net: tuple(t.clone() for t in net.encode_key_nhwc(image4)[:3])             # key, shrinkage, selection
    a, first, got = _reload_check(make, run, synth_sd, sd2)
    assert a.captures == a._stages.captures
    assert not torch.equal(got[2], first[2]) and torch.equal(got[1], first[1])              # e_proj moved, d_proj did not
    # to() uploads again as well: back to the first weights through it
    a._sd = {k: v.clone() for k, v in synth_sd.items()}
    assert a.to('cuda') is a and len(a._stages) == 0
    back = run(a)
    assert a.captures == 3 and len(a._stages) == 1
    assert all(torch.equal(x, y) for x, y in zip(back, first))


def test_s2m_reload_recaptures():
    from xmem2_amd.s2m import S2M
    from xmem2_amd.synth import synthetic_s2m_state_dict
    sd = synthetic_s2m_state_dict(0)
    sd2 = _shifted(sd, {'classifier.classifier.3.bias': 0.25})
    g = torch.Generator().manual_seed(8)
    image = torch.randn(3, 32, 48, generator=g).cuda()
    prev = torch.zeros(32, 48).cuda()
    scr = np.zeros((32, 48), np.uint8)
    scr[10:14, 8:30], scr[24:27, 30:44] = 1, 2
    scr = torch.from_numpy(scr).cuda()
    run = lambda net: tuple(t.clone() for t in net.run(image, prev, scr, 2))
    _reload_check(lambda: S2M(device='cuda:0'), run, sd, sd2, '_graphs')


def test_click_reload_recaptures():
    from xmem2_amd.click import ClickNet
    from xmem2_amd.synth import synthetic_click_state_dict
    sd = synthetic_click_state_dict(0)
    sd2 = _shifted(sd, {'head.layers.2.bias': 0.5})
    g = torch.Generator().manual_seed(9)
    image = torch.randn(3, 32, 48, generator=g).cuda()
    pts = np.array([[12, 20], [-1, -1]], np.float32)
    run = lambda net: (net.run(image, pts).clone(),)
    a, _, _ = _reload_check(lambda: ClickNet(device='cuda:0'), run, sd, sd2, '_graphs')
    assert not a._brs
