"""GPU: the f-BRS refinement kernels against float64 torch (tests/brs_refs.py), the objective and the controllers against the
reference's recorded float64 runs (tests/golden/brs.npz)."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from xmem2_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brs_refs                                                   # noqa: E402

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('make_brs_goldens', os.path.join(GOLDEN, 'make_brs_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, rtol=1e-5, atol=1e-6, msg=''):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), f'{msg}: {int(bad.sum())}/{bad.numel()} out of tolerance, max abs err {float(err.max()):.3e}'


def _fp32_reference():
    with open(os.path.join(GOLDEN, 'brs_fp32_reference.json')) as f:
        return json.load(f)


# ---- kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 5, 7, 160), (1, 1, 1, 8)])
def test_affine_and_relu_gates(shape):
    C = shape[3]
    x = torch.randn(shape, generator=_gen(1))
    sb = torch.randn(2 * C, generator=_gen(2)) * 0.3
    y = ops.brs_affine(x.cuda(), sb.cuda())
    _close(y, x.double() * (1 + sb[:C].double()) + sb[C:].double(), msg='affine')
    zero = torch.zeros(2 * C).cuda()
    assert torch.equal(ops.brs_affine(x.cuda(), zero).cpu(), x), 'scale 0, bias 0 must be the identity'
    kept = torch.relu(torch.randn(shape, generator=_gen(3)))              # a ReLU output: about half zeros
    g = torch.randn(shape, generator=_gen(4))
    out = ops.relu_gate(kept.cuda(), g.cuda())
    assert torch.equal(out.cpu(), torch.where(kept > 0, g, torch.zeros(()))), 'the gate selects: bit-exact'
    gc = g.cuda()
    assert ops.relu_gate(kept.cuda(), gc, out=gc) is gc and torch.equal(gc.cpu(), out.cpu()), 'in place'
    g1, w = torch.randn(shape[:3], generator=_gen(5)), torch.randn(C, generator=_gen(6))
    outer = ops.relu_gate_outer(kept.cuda(), g1.cuda(), w.cuda())
    _close(outer, torch.where(kept > 0, g1.double()[..., None] * w.double(), torch.zeros((), dtype=torch.float64)), msg='outer gate')


@pytest.mark.parametrize('shape', [(2, 25, 33, 160), (1, 3, 5, 128), (1, 1, 1, 8)])
def test_param_grad_within_the_fp32_summation_bound(shape):
    B, h, w, C = shape
    n = B * h * w
    g, x = torch.randn(shape, generator=_gen(7)), torch.randn(shape, generator=_gen(8)) * 1.5
    sb = torch.randn(2 * C, generator=_gen(9)) * 0.1
    record = torch.zeros(ops.BRS_RECORD + 2 * C)
    record[0] = 0.37
    record = record.cuda()
    ops.brs_param_grad(g.cuda(), x.cuda(), sb.cuda(), record, record[ops.BRS_RECORD:], 1e-3, 10.0)
    again = record.clone()
    ops.brs_param_grad(g.cuda(), x.cuda(), sb.cuda(), record, record[ops.BRS_RECORD:], 1e-3, 10.0)
    assert torch.equal(record, again), 'the reduction must be bit-reproducible'
    got = record.cpu().double()
    gd, xd, sd = g.double().reshape(n, C), x.double().reshape(n, C), sb.double()
    terms = torch.cat([gd * xd, gd], 1)                                  # [n, 2C]: column c of the scale half, then of the bias half
    reg = torch.cat([2e-3 * sd[:C], 2e-2 * sd[C:]])
    ref = terms.sum(0) + reg
    # n + 1 terms added in fp32 in any order, each product rounded once: |error| <= (n + 1) 2^-24 sum |terms| to first order
    bound = (n + 1) * 2.0 ** -24 * (terms.abs().sum(0) + reg.abs()) + 1e-30
    err = (got[ops.BRS_RECORD:] - ref).abs()
    print(f'param_grad {shape}: max err / bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all()), f'max err / bound {float((err / bound).max()):.3f}'
    f = 0.37 + 1e-3 * float((sd[:C] ** 2).sum() + 10.0 * (sd[C:] ** 2).sum())
    assert abs(float(got[3]) - f) <= (2 * C + 2) * 2.0 ** -24 * f


LOSS_H4, LOSS_W4, LOSS_H, LOSS_W = 25, 33, 97, 131
LOSS_CLICKS = [(True, (0.0, 40.0)), (False, (50.0, 0.0)), (True, (96.0, 130.0)), (False, (96.0, 3.0)), (True, (10.5, 20.5)), (False, (11.5, 70.5)),
               (True, (40.0, 60.0)), (True, (41.0, 61.0)), (False, (60.0, 100.0)), (False, (61.0, 99.0)), (True, (3.0, 130.0)), (True, (40.0, 60.0))]


@pytest.fixture(scope='module')
def loss_logits():
    """Random logits [2,25,33] whose float64 upsample to 97 x 131 stays 1e-4 away from 0, so that the mask bit is decided alike in
    fp32 (the interpolation of values <= 4 in magnitude errs by < 1e-5 there)."""
    logits = (torch.randn(2, LOSS_H4, LOSS_W4, generator=_gen(631)) * 1.5).clamp(-4, 4)     # the seed whose upsample stays farthest from 0
    up = torch.nn.functional.interpolate(logits.double()[:, None], size=(LOSS_H, LOSS_W), mode='bilinear', align_corners=True)[:, 0]
    assert float(up.abs().min()) > 1e-4, 'an upsampled logit lies within 1e-4 of zero: pick another seed'
    return logits


@pytest.mark.parametrize('clicks', [LOSS_CLICKS, [c for c in LOSS_CLICKS if c[0]]], ids=['both', 'positive_only'])
def test_brs_loss_vs_float64(loss_logits, clicks):
    from xmem2_amd.click import Click
    from xmem2_amd.click_brs import click_squares, flipped_clicks
    ours = [Click(p, c) for p, c in clicks]
    lists = [ours, flipped_clicks(ours, LOSS_W)]
    rects = click_squares(lists, (LOSS_H, LOSS_W))
    pos, neg = brs_refs.click_maps([[(c.is_positive, c.coords) for c in cl] for cl in lists], (LOSS_H, LOSS_W))
    ref = brs_refs.loss_and_gradient(loss_logits.numpy(), pos, neg, (LOSS_H, LOSS_W))
    assert np.abs(ref['up']).min() > 1e-4
    cap = 16
    host = np.zeros((2, cap, 5), np.int32)
    host[:, :rects.shape[1]] = rects
    last = (torch.rand(2, LOSS_H, LOSS_W, generator=_gen(12)) > 0.5).to(torch.uint8)
    last[1, :40] = 0
    mask = torch.full((2, LOSS_H, LOSS_W), 7, dtype=torch.uint8).cuda()
    record = torch.full((ops.BRS_RECORD,), -1.0).cuda()
    count = torch.tensor([rects.shape[1]], dtype=torch.int32).cuda()
    args = (loss_logits.cuda(), LOSS_H, LOSS_W, torch.from_numpy(host).cuda(), count, last.cuda(), mask, record)
    dlogit = ops.brs_loss(*args)
    rec = record.cpu().numpy()
    again = ops.brs_loss(*args)
    assert torch.equal(again, dlogit) and np.array_equal(record.cpu().numpy().view(np.int32), rec.view(np.int32)), 'not bit-reproducible'
    ref_mask = ref['up'] > 0
    assert np.array_equal(mask.cpu().numpy(), ref_mask.astype(np.uint8)), 'mask'
    counts = rec[4:8].view(np.int32)
    lm = last.numpy().astype(bool)
    assert counts.tolist() == [int((ref_mask[b] & lm[b]).sum()) if k == 0 else int((ref_mask[b] | lm[b]).sum()) for b in range(2) for k in range(2)]
    print(f'loss {rec[0]:.6f} (float64 {ref["loss"]:.6f}) maxima {rec[1]:.6f} {rec[2]:.6f} (float64 {ref["f_max_pos"]:.6f} {ref["f_max_neg"]:.6f})')
    _close(rec[0], ref['loss'], msg='loss')
    _close(rec[1], ref['f_max_pos'], msg='f_max_pos')
    _close(rec[2], ref['f_max_neg'], msg='f_max_neg')
    _close(dlogit, ref['dlogit'], msg='dlogit')
    assert np.abs(ref['dlogit']).max() > 1e-3, 'the case has no gradient to speak of'


# ---- the objective and the controllers against the recorded runs ---------------------------------------------------------------
@pytest.fixture(scope='module')
def click_net():
    from xmem2_amd.click import ClickNet
    from xmem2_amd.synth import synthetic_click_state_dict
    net = ClickNet(device='cuda')
    net.load_state_dict(synthetic_click_state_dict(0))
    return net


def _controller(net, name):
    from xmem2_amd.click_brs import FeatureBRSController
    c = G.BRS_CASES[name]
    return FeatureBRSController(net, max_size=800, brs_mode=c['mode'], zoom_in_params=c['zoom'], net_clicks_limit=c['limit'])


_RUNS = {}


def _drive(net, name):
    """Run the case once through FeatureBRSController; per step what the tests below check.  After every refined click the objective is
    also evaluated at the reference's recorded iterates (the click's squares and input_data are still in the graph's buffers)."""
    if name in _RUNS:
        return _RUNS[name]
    gd = load_golden('brs')
    c = G.BRS_CASES[name]
    ctl = _controller(net, name)
    image = torch.from_numpy(G.case_image(name))[None].cuda()
    out, kept, k = [], [], 0
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
            out.append(dict(undo=True, same_tensor=ctl.prob is before[0], same_bits=torch.equal(ctl.prob, before[1]), prob=ctl.prob.cpu().numpy()))
            kept.pop()
            continue
        _, x, y, positive = step
        ctl.interact(image, x, y, positive)
        pred = ctl.predictor
        zoom, limit = pred.transforms
        size, clicks = pred.last_geometry
        rec = dict(roi=G._roi_arr(zoom._object_roi).tolist(), limit_roi=G._roi_arr(limit._object_roi).tolist(), size=list(size), clicks=clicks,
                   evals=[dict(e) for e in pred.opt_functor.evaluations], prob=ctl.prob.cpu().numpy(), click=k, at_recorded=[])
        if f'{name}_x{k}' in gd.files:
            obj = pred.engine.objective(tuple(pred.input_data.shape), size[0], size[1], len(clicks), 1e-3, 10.0)
            for xr in gd[f'{name}_x{k}']:
                a = obj.evaluate(xr)
                b = obj.evaluate(xr)
                rec['at_recorded'].append(dict(f=float(a['f']), grad=a['grad'].astype(np.float64),
                                               same_bits=a['f'] == b['f'] and np.array_equal(a['grad'].view(np.int32), b['grad'].view(np.int32))))
        kept.append((ctl.prob, ctl.prob.clone()))
        out.append(rec)
        k += 1
    _RUNS[name] = out
    return out


@pytest.mark.parametrize('name', ['b1', 'c1'])
def test_objective_at_the_recorded_iterates(click_net, name):
    """f and grad at x = 0 (the first evaluation of click 2) and at every iterate the reference's float64 run visited: within 1e-3 of
    max |golden|, the allowance of the click network's feature gates; two evaluations at one x are bit-identical."""
    gd = load_golden('brs')
    ref32 = _fp32_reference()[name]
    worst_f = worst_g = 0.0
    n = 0
    for rec in (r for r in _drive(click_net, name) if not r.get('undo')):
        k = rec['click']
        if not rec['at_recorded']:
            continue
        if k == 1:
            assert not gd[f'{name}_x{k}'][0].any(), 'the first evaluation of the second click is at x = 0'
        for j, got in enumerate(rec['at_recorded']):
            f64, g64, stop = float(gd[f'{name}_f{k}'][j]), gd[f'{name}_grad{k}'][j].astype(np.float64), int(gd[f'{name}_stop{k}'][j])
            ef = abs(got['f'] - f64) / abs(f64)
            worst_f = max(worst_f, ef)
            line = f'{name} click {k} evaluation {j}: |f - f64| / |f64| {ef:.2e} (fp32 reference {ref32["eval_f"][n]:.2e})'
            assert got['same_bits'], f'{name} click {k} evaluation {j}: two evaluations at the same x differ'
            assert ef <= 1e-3, line
            if stop == 0:               # on a stop the reference hands L-BFGS zeros and never computes the gradient
                eg = float(np.abs(got['grad'] - g64).max() / np.abs(g64).max())
                worst_g = max(worst_g, eg)
                line += f', max |grad - grad64| / max |grad64| {eg:.2e} (fp32 reference {ref32["eval_grad"][n]:.2e})'
                assert eg <= 1e-3, line
            print(line)
            n += 1
    assert n == int(sum(gd[f'{name}_eval_counts'])) > 0
    print(f'{name}: worst f {worst_f:.2e}, worst grad {worst_g:.2e} over {n} evaluations')


@pytest.mark.parametrize('name', ['b1', 'b2', 'c1'])
def test_controller_vs_reference(click_net, name):
    from xmem2_amd.click import FBRSController
    gd = load_golden('brs')
    ref32 = _fp32_reference()[name]
    c = G.BRS_CASES[name]
    probs64 = gd[f'{name}_prob64_u16'].astype(np.float64) / 65535.0
    run = _drive(click_net, name)
    assert len(run) == len(probs64)
    for s, rec in enumerate(run):
        p64 = probs64[s]
        tol = max(2e-3, 2.0 * ref32['perturbed_max_abs'][s])
        err = float(np.abs(rec['prob'] - p64).max())
        flips = int(((rec['prob'] > 0.5) != (p64 > 0.5)).sum())
        undecided = int((np.abs(p64 - 0.5) <= tol).sum())
        what = f'{name} step {s}' + (' (undo)' if rec.get('undo') else f' (click {rec["click"]}, {len(rec["evals"])} evaluations)')
        print(f'{what}: max |p - p64| {err:.3e} (fp32 reference {ref32["per_step"][s]:.3e}, allowed {tol:.3e}), mask mismatches {flips} (allowed {undecided})')
        if rec.get('undo'):
            assert rec['same_tensor'] and rec['same_bits'], f'{what}: undo did not restore the previous probability bit for bit'
        else:
            k = rec['click']
            assert rec['roi'] == gd[f'{name}_rois'][k].tolist(), f'{what}: ROI'
            assert rec['limit_roi'] == gd[f'{name}_limit_rois'][k].tolist(), f'{what}: LimitLongestSide ROI'
            assert rec['size'] == gd[f'{name}_sizes'][k].tolist(), f'{what}: working size'
            np.testing.assert_allclose(np.array(rec['clicks'], np.float64).reshape(-1, 2), gd[f'{name}_clicks{k}'], rtol=0, atol=1e-9)
            assert len(rec['evals']) == int(gd[f'{name}_eval_counts'][k]), f'{what}: the reference ran {int(gd[f"{name}_eval_counts"][k])} evaluations'
            if len(rec['evals']):
                assert [e['stop'] for e in rec['evals']] == gd[f'{name}_stop{k}'].tolist(), f'{what}: stops'
        assert err <= tol, what
        assert flips <= undecided, what
    # the first click runs no optimisation: bit-equal to the NoBRS controller's
    first = next(s for s in c['steps'] if s[0] == 'click')
    plain = FBRSController(click_net, max_size=800, zoom_in_params=c['zoom'])
    plain.interact(torch.from_numpy(G.case_image(name))[None].cuda(), first[1], first[2], first[3])
    assert np.array_equal(plain.prob.cpu().numpy(), run[0]['prob']), f'{name}: the first click differs from NoBRS'
    assert any(len(r.get('evals', [])) > 1 for r in run), f'{name}: no click was optimised'


def test_refinement_changes_the_mask(click_net):
    """From the second click on f-BRS-B and NoBRS give different masks - the reference flips 8980 of this image's 12707 pixels at the
    second click of b1: the refinement is not a no-op."""
    from xmem2_amd.click import FBRSController
    c = G.BRS_CASES['b1']
    plain = FBRSController(click_net, max_size=800, zoom_in_params=c['zoom'], net_clicks_limit=c['limit'])
    image = torch.from_numpy(G.case_image('b1'))[None].cuda()
    run = _drive(click_net, 'b1')
    for s, step in enumerate(c['steps'][:2]):
        plain.interact(image, step[1], step[2], step[3])
    flips = int(((plain.prob.cpu().numpy() > 0.5) != (run[1]['prob'] > 0.5)).sum())
    print(f'b1 click 2: f-BRS-B flips {flips} pixels against NoBRS')
    assert flips > 1000


def test_cli_brs_mode(tmp_path, click_net):
    """`python -m xmem2_amd.click --brs-mode f-BRS-B` writes the mask FeatureBRSController gives for the same clicks."""
    import subprocess
    from PIL import Image
    from conftest import ROOT
    from xmem2_amd.click import click_commit
    from xmem2_amd.scribble import IM_MEAN, IM_STD
    frames = tmp_path / 'frames'
    frames.mkdir()
    f = G.case_image('b1').transpose(1, 2, 0)
    img = np.clip((f * IM_STD + IM_MEAN) * 255.0, 0, 255).astype(np.uint8)
    Image.fromarray(img).save(frames / '00000.png')
    steps = G.BRS_CASES['b1']['steps'][:2]
    clicks = [{'object': 1, 'x': s[1], 'y': s[2], 'positive': s[3]} for s in steps]
    (tmp_path / 'clicks.json').write_text(json.dumps({'0': clicks}))
    r = subprocess.run([sys.executable, '-m', 'xmem2_amd.click', '--images', str(frames), '--clicks', str(tmp_path / 'clicks.json'),
                        '--out', str(tmp_path / 'masks'), '--synthetic-seed', '0', '--brs-mode', 'f-BRS-B'], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    written = np.array(Image.open(tmp_path / 'masks' / '00000.png'))
    from xmem2_amd.click_brs import FeatureBRSController
    image = torch.from_numpy(((img.astype(np.float32) / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1).copy()).cuda()
    ctl = FeatureBRSController(click_net)
    for s in steps:
        obj = ctl.interact(image, s[1], s[2], s[3])
    assert len(ctl.predictor.opt_functor.evaluations) > 0, 'the second click was not refined'
    prob = torch.zeros(2, *img.shape[:2], device='cuda')
    prob[0] = 1
    _, mask = click_commit(prob, obj, 1)
    assert np.array_equal(written, mask.cpu().numpy())
