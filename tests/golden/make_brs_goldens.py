"""Record tests/golden/brs.npz: the reference's f-BRS click refinement (FeatureBRSPredictor, ScaleBiasOptimizer, BRSMaskLoss) on
conditioned synthetic weights.

    python tests/golden/make_brs_goldens.py --reference PATH [--check]

Imports the reference's fbrs package as make_click_goldens.py does, loads xmem2_amd.synth.synthetic_click_state_dict(0) and drives
InteractiveController with the reference controller's parameters (inference/interact/fbrs_controller.py:17-27) through each case
three times on the CPU: in fp32, with the model and image cast to float64 (the golden), and in float64 with the optimised feature
map (`input_data`) perturbed by 1e-3 of its largest magnitude (uniform noise of that amplitude, seeded) - the allowance the
project's feature gates give an intermediate tensor of the click network.  The optimisation amplifies such a perturbation a lot
(p moves by up to 0.1 in the recorded cases): the perturbed run decides which clicks are fit to be a golden at all, see BRS_CASES.  `np.float`, which the reference's optimiser still names, is set to `float` here and only here.

Every evaluation of the objective is recorded (x as the float32 vector the objective sees, f, the float32 gradient L-BFGS was
handed, the two maxima, the per-sample IoU list and which stop fired), and every click (geometry, probability map, number of
evaluations).  The generator asserts what the tests then rely on: the three runs take the same geometries, evaluation counts and
stops, and every quantity that decides a stop stays `MARGIN` from its threshold.  A mask-IoU stop is decided by pixel counts: its
margin is measured where it can be - on the IoU when the stop does not fire, and by the stop firing alike in all three runs when it
does (an IoU of 1 is 1e-3 from the threshold by construction).

brs.npz holds the float64 run: probability maps as uint16 steps of 1/65535, float64 scalars on a 20-bit significand (`grid20`), and
the optimiser's exchange (x, gradient: float32 values in the reference itself; f: float64) as it was, because the host-loop test
replays it through scipy and must see the values scipy saw.  --check regenerates and compares: the exchange to 1e-5 relative
(float64 convolutions differ between CPU kernels in the last bits), everything else array for array.  The fp32 run's own distance
from float64 and the perturbed run's go to brs_fp32_reference.json, which --check does not compare.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'brs.npz')
OUT_FP32 = os.path.join(HERE, 'brs_fp32_reference.json')
sys.path.insert(0, HERE)

from make_click_goldens import RADIUS, ZOOM_DEFAULTS, grid20, u16      # noqa: E402

MARGIN = 0.02                   # distance every stop-deciding quantity keeps from its threshold
PERTURB = 1e-3                  # of max |input_data|: tests/test_gpu_click.py gates head_input at that
PERTURB_SEED = 0
PROB_THRESH = 0.5
MIN_IOU_DIFF = 1e-3

# steps: ('click', x, y, positive) | ('plant',) the synthetic ellipse as the zoom-in's previous probabilities | ('undo',)
_B1_STEPS = [('click', 60, 45, True), ('click', 100, 20, False), ('click', 0, 0, True), ('click', 30, 80, False), ('click', 64, 50, True)]
BRS_CASES = {
    'b1': dict(H=97, W=131, seed=21, mode='f-BRS-B', limit=8, zoom=dict(target_size=128, min_crop_size=32), steps=_B1_STEPS),
    # f-BRS-C on b1's clicks.  With all five the reference takes 6 / 1 / 7 / 7 evaluations, but clicks 4 and 5 do not survive the
    # perturbed run (7 becomes 6 to 10 evaluations and p moves by 0.15 to 0.4, whatever the noise: uniform with any seed, constant,
    # alternating, a tenth of the amplitude), so the case ends after the third click: 6 / 1 evaluations, the empty border square included.
    'c1': dict(H=97, W=131, seed=21, mode='f-BRS-C', limit=8, zoom=dict(target_size=128, min_crop_size=32), steps=_B1_STEPS[:3]),
    # a planted previous mask (a proper sub-ROI), click 3 outside it (the ROI changes between two refined clicks), an undo, and
    # net_clicks_limit=2: clicks 3 and 3' act through the loss only, and 3' - back in the planted ROI without an image change -
    # optimises the input_data click 3 left behind at ANOTHER geometry, as the reference does (input_data is not part of the states)
    'b2': dict(H=120, W=176, seed=22, mode='f-BRS-B', limit=2, zoom=dict(target_size=192, min_crop_size=48),
               steps=[('click', 88, 60, True), ('plant',), ('click', 100, 45, True), ('click', 13, 27, True), ('undo',), ('click', 53, 92, True)]),
}


# The objective on its own (tests/brs_refs.py against the reference's modules): a seeded random input_data [2,C,7,9] and x, working
# size 25 x 33, clicks (positive, (row, col)) with a row-0 square (empty), a far-corner square (clipped), a half-to-even centre and two
# overlapping positive squares
RESTATEMENT = dict(h4=7, w4=9, H=25, W=33, clicks=[(True, (12.0, 16.0)), (False, (0.0, 5.0)), (True, (24.0, 32.0)), (False, (2.5, 3.5)),
                                                   (True, (13.0, 17.0)), (False, (20.0, 6.0))])
RESTATEMENT_MODES = {'rb': 'after_aspp', 'rc': 'after_deeplab'}


def restatement_inputs(name, deeplab_ch=128):
    """(input_data [2,C,h4,w4] float64, x [2C] float32) of a restatement case."""
    C = deeplab_ch + (32 if RESTATEMENT_MODES[name] == 'after_aspp' else 0)
    rng = np.random.RandomState({'rb': 5, 'rc': 6}[name])
    feat = rng.standard_normal((2, C, RESTATEMENT['h4'], RESTATEMENT['w4']))
    return feat, (0.1 * rng.standard_normal(2 * C)).astype(np.float32)


def case_image(name):
    """image [3,H,W] float32 (normalised scale) of a case."""
    sys.path.insert(0, ROOT)
    from xmem2_amd.synth import synthetic_frames
    c = BRS_CASES[name]
    return synthetic_frames(1, c['H'], c['W'], seed=c['seed'])[0]


def planted_probs(name):
    sys.path.insert(0, ROOT)
    from xmem2_amd.synth import synthetic_masks
    c = BRS_CASES[name]
    return synthetic_masks(1, 1, c['H'], c['W'])[0, 0].astype(np.float32)


def zoom_params(name):
    zoom = dict(ZOOM_DEFAULTS)
    zoom.update(BRS_CASES[name]['zoom'])
    return zoom


def _reference(path):
    np.float = float                                                          # brs_functors.py:75
    sys.path.insert(0, path)
    from inference.interact.fbrs.utils.cython import get_dist_maps            # noqa: F401  (pyximport: stops here without Cython)
    from inference.interact.fbrs.inference.utils import load_is_model
    from inference.interact.fbrs.controller import InteractiveController
    from inference.interact.fbrs.inference.predictors import brs_functors
    return load_is_model, InteractiveController, brs_functors


def _params(name):
    c = BRS_CASES[name]
    return {'brs_mode': c['mode'], 'prob_thresh': PROB_THRESH, 'zoom_in_params': zoom_params(name),
            'predictor_params': {'net_clicks_limit': c['limit'], 'max_size': 800},
            'brs_opt_func_params': {'min_iou_diff': MIN_IOU_DIFF}, 'lbfgs_params': {'maxfun': 20}}


def _instrument(brs_functors, functor, log):
    """Record every evaluation of `functor` into `log` (a list the caller swaps per click)."""
    cap = {}
    inner_loss = functor.brs_loss

    def loss(result, pos, neg):
        out = inner_loss(result, pos, neg)
        cap['fmax'], cap['iou'] = (float(out[1]), float(out[2])), None
        return out
    functor.brs_loss = loss
    inner_iou = brs_functors._compute_iou

    def iou(a, b):
        r = inner_iou(a, b)
        cap['iou'] = [float(v) for v in r]
        return r
    brs_functors._compute_iou = iou
    cls = type(functor)
    inner_call = cls.__call__

    class Logged(cls):
        def __call__(self, x):
            f, g = inner_call(self, x)
            g = np.asarray(g)
            fmp, fmn = cap['fmax']
            stop = 0
            if fmp < 1 - self.prob_thresh and fmn < self.prob_thresh:
                stop = 1
            elif cap['iou'] is not None and len(cap['iou']) > 0 and np.mean(np.array(cap['iou'], np.float32)) > 1 - self.min_iou_diff:
                stop = 2
            assert (stop != 0) == (not g.any()), 'the stop bookkeeping of the generator lost track of the reference'
            log[0].append(dict(x=np.asarray(x, np.float64).astype(np.float32), f=float(f), grad=g.astype(np.float32), fmax=(fmp, fmn),
                               iou=cap['iou'], stop=stop))
            return [f, g]
    functor.__class__ = Logged
    return lambda: setattr(brs_functors, '_compute_iou', inner_iou)


def _perturb_scale(t):
    return t.abs().max()


def _run_case(torch, Controller, brs_functors, model, name, dtype, perturb=0.0):
    """One record per step: dict(roi, limit_roi, size, clicks, prob, evals) per click, dict(undo, prob) per undo."""
    c = BRS_CASES[name]
    ctl = Controller(model, 'cpu', _params(name))
    ctl.set_image(torch.from_numpy(case_image(name)).to(dtype))
    pred = ctl.predictor
    seen, log = [], [[]]
    inner = pred._get_prediction

    def logged(image_nd, clicks_lists, is_image_changed):
        seen.append((tuple(image_nd.shape[2:]), [tuple(float(v) for v in k.coords) for k in clicks_lists[0]]))
        return inner(image_nd, clicks_lists, is_image_changed)
    pred._get_prediction = logged
    if perturb:
        head_input = pred._get_head_input
        gen = torch.Generator().manual_seed(PERTURB_SEED)

        def perturbed(image_nd, points):
            t = head_input(image_nd, points)
            return t + perturb * _perturb_scale(t) * (2.0 * torch.rand(t.shape, generator=gen, dtype=t.dtype) - 1.0)
        pred._get_head_input = perturbed
    restore = _instrument(brs_functors, pred.opt_functor, log)
    out = []
    try:
        for step in c['steps']:
            if step[0] == 'plant':
                states = pred.get_states()
                z = list(states['transform_states'][0])
                z[2] = planted_probs(name)[None, None].astype(np.float64 if dtype == torch.float64 else np.float32)
                states['transform_states'][0] = tuple(z)
                pred.set_states(states)
                continue
            if step[0] == 'undo':
                ctl.undo_click()
                out.append(dict(undo=True, prob=ctl.probs_history[-1][1][0, 0].double().numpy()))
                continue
            _, x, y, positive = step
            log[0] = []
            ctl.add_click(x, y, positive)
            size, clicks = seen[-1]
            zoom, limit = pred.transforms[0], pred.transforms[1]
            out.append(dict(roi=zoom._object_roi, limit_roi=limit._object_roi, size=size, clicks=clicks, evals=log[0],
                            opt_data=np.array(pred.opt_data, np.float32), prob=ctl.probs_history[-1][1][0, 0].double().numpy()))
    finally:
        restore()
    return out


def _restatement(torch, reference, brs_functors, net64, name):
    """f and grad of the reference's ScaleBiasOptimizer on a restatement case, its modules called as FeatureBRSPredictor's closure
    calls them (brs.py:82-103)."""
    from inference.interact.fbrs.inference.clicker import Click
    from inference.interact.fbrs.inference.predictors import get_predictor
    from inference.interact.fbrs.inference.transforms import AddHorizontalFlip
    R, mode = RESTATEMENT, RESTATEMENT_MODES[name]
    feat, x = restatement_inputs(name)
    input_data = torch.from_numpy(feat)
    pred = get_predictor(net64, 'f-BRS-B', 'cpu', prob_thresh=PROB_THRESH, zoom_in_params=None)
    clicks = [Click(is_positive=p, coords=c) for p, c in R['clicks']]
    _, lists = AddHorizontalFlip().transform(torch.zeros(1, 3, R['H'], R['W']), [clicks])
    pos, neg = pred._get_clicks_maps_nd(lists, (R['H'], R['W']))

    def logits(scale, bias):
        y = input_data * scale.view(1, -1, 1, 1).repeat(2, 1, 1, 1) + bias.view(1, -1, 1, 1).repeat(2, 1, 1, 1)
        if mode == 'after_aspp':
            y = net64.feature_extractor.head(y)
        return torch.nn.functional.interpolate(net64.head(y), size=(R['H'], R['W']), mode='bilinear', align_corners=True)
    functor = brs_functors.ScaleBiasOptimizer(prob_thresh=PROB_THRESH, with_flip=True, optimizer_params={}, min_iou_diff=MIN_IOU_DIFF)
    functor.init_click(logits, pos, neg, 'cpu')
    f, g = functor(x.astype(np.float64))
    g = np.asarray(g)
    assert g.any(), f'{name}: the restatement case stops at once'
    assert float(pos.sum()) > 18 and float(neg.sum()) > 9, f'{name}: the click maps are emptier than planned'
    return float(f), g.astype(np.float32), float(pos.sum()), float(neg.sum())


def _roi_arr(roi):
    return np.array([-1, -1, -1, -1] if roi is None else [int(v) for v in roi], np.int32)


def _margins(ev):
    """Distances of the stop-deciding quantities of one evaluation from their thresholds."""
    fmp, fmn = ev['fmax']
    out = []
    if ev['stop'] == 1:
        out.append(min((1 - PROB_THRESH) - fmp, PROB_THRESH - fmn))
    else:
        out.append(max(fmp - (1 - PROB_THRESH), fmn - PROB_THRESH))
        if ev['iou'] and ev['stop'] == 0:
            out.append((1 - MIN_IOU_DIFF) - float(np.mean(ev['iou'])))
    return out


def generate(reference):
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    load_is_model, Controller, brs_functors = _reference(reference)
    sys.path.insert(0, ROOT)
    from xmem2_amd.synth import synthetic_click_state_dict
    sd = synthetic_click_state_dict(0)
    net32 = load_is_model(dict(sd), 'cpu', cpu_dist_maps=True, norm_radius=RADIUS)
    net64 = load_is_model(dict(sd), 'cpu', cpu_dist_maps=True, norm_radius=RADIUS).double()
    rec, fp32 = {}, {}
    for name in RESTATEMENT_MODES:
        f, g, npos, nneg = _restatement(torch, reference, brs_functors, net64, name)
        print(f'{name}: f {f:.6f} max |grad| {float(np.abs(g).max()):.3e} positive / negative pixels {npos:.0f} / {nneg:.0f}')
        rec[f'{name}_f'], rec[f'{name}_grad'], rec[f'{name}_pixels'] = np.array(f, np.float64), g, np.array([npos, nneg], np.int32)
    for name, c in BRS_CASES.items():
        r64 = _run_case(torch, Controller, brs_functors, net64, name, torch.float64)
        r32 = _run_case(torch, Controller, brs_functors, net32, name, torch.float32)
        rpt = _run_case(torch, Controller, brs_functors, net64, name, torch.float64, perturb=PERTURB)
        info = dict(per_step=[], perturbed_max_abs=[], eval_f=[], eval_grad=[])
        worst = np.inf
        for i, (a, b, p) in enumerate(zip(r64, r32, rpt)):
            err, dev = float(np.abs(b['prob'] - a['prob']).max()), float(np.abs(p['prob'] - a['prob']).max())
            info['per_step'].append(err)
            info['perturbed_max_abs'].append(dev)
            if a.get('undo'):
                print(f'{name} step {i}: undo, fp32 vs float64 {err:.2e}, perturbed {dev:.2e}')
                continue
            for other, what in ((b, 'fp32'), (p, 'perturbed')):
                assert a['roi'] == other['roi'] and a['limit_roi'] == other['limit_roi'] and a['size'] == other['size'] \
                    and a['clicks'] == other['clicks'], f'{name} step {i}: the {what} run took another geometry'
                assert [e['stop'] for e in a['evals']] == [e['stop'] for e in other['evals']], \
                    f'{name} step {i}: the {what} run took {[e["stop"] for e in other["evals"]]} evaluations / stops, float64 {[e["stop"] for e in a["evals"]]}'
                for e in other['evals']:
                    worst = min([worst] + _margins(e))
            for e, e32 in zip(a['evals'], b['evals']):
                worst = min([worst] + _margins(e))
                info['eval_f'].append(abs(e32['f'] - e['f']) / max(abs(e['f']), 1e-30))
                gmax = float(np.abs(e['grad']).max())
                info['eval_grad'].append(float(np.abs(e32['grad'].astype(np.float64) - e['grad']).max()) / gmax if gmax > 0 else 0.0)
            best = int(np.argmin([e['f'] for e in a['evals']])) if a['evals'] else -1
            print(f'{name} step {i}: roi {a["roi"]} size {a["size"]} evals {len(a["evals"])} stops {[e["stop"] for e in a["evals"]]} best {best} '
                  f'mask {float((a["prob"] > 0.5).mean()):.3f} fp32 vs float64 {err:.2e} perturbed {dev:.2e}')
            assert err <= 2e-4, f'{name} step {i}: the fp32 reference is {err:.2e} from float64'
        print(f'{name}: the closest stop-deciding quantity is {worst:.4f} from its threshold')
        assert worst >= MARGIN, f'{name}: a stop is decided within {worst:.4f} of its threshold: pick other clicks'
        info['max_abs'], info['stop_margin'] = max(info['per_step']), float(worst)
        fp32[name] = info
        clicks = [s for s in r64 if not s.get('undo')]
        rec[f'{name}_rois'] = np.stack([_roi_arr(s['roi']) for s in clicks])
        rec[f'{name}_limit_rois'] = np.stack([_roi_arr(s['limit_roi']) for s in clicks])
        rec[f'{name}_sizes'] = np.array([s['size'] for s in clicks], np.int32)
        rec[f'{name}_eval_counts'] = np.array([len(s['evals']) for s in clicks], np.int32)
        rec[f'{name}_prob64_u16'] = u16(np.stack([s['prob'] for s in r64]))          # undo steps included, in step order
        for i, s in enumerate(clicks):
            rec[f'{name}_clicks{i}'] = np.array(s['clicks'], np.float64).reshape(-1, 2)
            rec[f'{name}_opt_data{i}'] = s['opt_data']
            ev = s['evals']
            if not ev:
                continue
            rec[f'{name}_x{i}'] = np.stack([e['x'] for e in ev])
            rec[f'{name}_f{i}'] = np.array([e['f'] for e in ev], np.float64)
            rec[f'{name}_grad{i}'] = np.stack([e['grad'] for e in ev])
            rec[f'{name}_fmax{i}'] = grid20(np.array([e['fmax'] for e in ev], np.float64))
            rec[f'{name}_stop{i}'] = np.array([e['stop'] for e in ev], np.int32)
            rec[f'{name}_iou{i}'] = grid20(np.array([(e['iou'] + [-1.0, -1.0])[:2] if e['iou'] is not None else [-2.0, -2.0] for e in ev],
                                                    np.float64))
        if name == 'b1':
            assert rec['b1_eval_counts'][0] == 0 and all(n > 0 for n in rec['b1_eval_counts'][1:]), 'the first click must not optimise'
        if name == 'b2':
            H, W = c['H'], c['W']
            planted = rec['b2_rois'][1]
            assert planted[0] > 0 and planted[1] < H - 1 and planted[2] > 0 and planted[3] < W - 1, f'b2: the planted ROI {planted} is not a proper sub-rectangle'
            assert tuple(rec['b2_rois'][2]) != tuple(rec['b2_rois'][1]), 'b2: click 3 did not move the ROI'
            assert tuple(rec['b2_rois'][3]) == tuple(rec['b2_rois'][1]) and tuple(rec['b2_sizes'][3]) != tuple(rec['b2_sizes'][2]), \
                "b2: click 3' after the undo should run in the planted ROI"
            assert rec['b2_eval_counts'][1] > 0 and rec['b2_eval_counts'][2] > 0, 'b2: the clicks around the ROI change were not refined'
    return rec, fp32


EXCHANGE = ('_x', '_f', '_grad', '_opt_data')        # what L-BFGS exchanged with the objective, and where it ended


def _is_exchange(key):
    tail = key.split('_', 1)[1].rstrip('0123456789')
    return '_' + tail in EXCHANGE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('XMEM_REFERENCE'), required='XMEM_REFERENCE' not in os.environ,
                    help='checkout of the reference project (default: $XMEM_REFERENCE)')
    ap.add_argument('--check', action='store_true', help='compare with the committed file instead of writing it')
    args = ap.parse_args()
    rec, fp32 = generate(args.reference)
    if args.check:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(rec), (sorted(old.files), sorted(rec))
        for k in rec:
            assert old[k].dtype == rec[k].dtype and old[k].shape == rec[k].shape, f'{k} differs in type or shape'
            if _is_exchange(k):
                scale = max(float(np.abs(old[k]).max()), 1e-30)
                assert float(np.abs(old[k].astype(np.float64) - rec[k]).max()) <= 1e-5 * scale, f'{k} differs'
            else:
                assert np.array_equal(old[k], rec[k]), f'{k} differs'
        print('brs.npz reproduced')
        return
    np.savez_compressed(OUT, **rec)
    with open(OUT_FP32, 'w') as f:
        json.dump(fp32, f, indent=1, sort_keys=True)
        f.write('\n')
    size = os.path.getsize(OUT)
    assert size < 1 << 20, f'brs.npz is {size} bytes: over the size limit of a committed file'
    print('wrote', OUT, size, 'bytes, and', OUT_FP32)


if __name__ == '__main__':
    main()
