"""Record tests/golden/click_eval.npz: the reference's robot user (fbrs Clicker), its IoU and NoC helpers and evaluate_sample runs.

    python tests/golden/make_click_eval_goldens.py --reference PATH [--check]

Imports the reference's fbrs package as make_click_goldens.py does.  `np.bool` and `np.int`, which the reference's clicker.py and
utils.py still name, are set to `bool` and `int` here and only here, where numpy lacks them.

(a) CLICKER_CASES: (gt, pred) pairs without a network (gt: 1 object, 0 background, -1 ignore); per case the reference Clicker's next
    three clicks on that prediction and get_iou.  `clicker_case` rebuilds every pair from its name; the pairs are stored as well.
(b) EVAL_CASES: evaluate_sample with the NoBRS predictor on xmem2_amd.synth.synthetic_click_state_dict(0), the model and image cast
    to float64 on the CPU.  The reference's predictor hands back a tensor [1,1,H,W] where its evaluate_sample expects the map, so
    the predictor is wrapped to return `[0, 0]` as numpy (and to log every map).  Per step: the click, the float64 probability map
    in uint16 steps of 1/65535, the float64 IoU, intersection and union, and the number of NEAR pixels |p64 - 0.49| <= NEAR - the
    allowance tests/test_gpu_click.py gives the click network's probabilities.  The generator asserts what lets the GPU tests
    demand equal clicks: the fp32 reference run takes the same clicks and stops alike; the reference clicker's next choice is the
    same with every near pixel forced to 1 and forced to 0; every IoU is further from max_iou_thr than near / union.  A candidate of
    EVAL_CANDIDATES that fails one of them is passed over (and reported), never tolerated; the first three that hold are recorded,
    and among them one must stop early and one must run out of clicks.
(c) NOC_CASES: compute_noc_metric, get_time_metrics and get_results_table on a few IoU lists.

--check regenerates and compares with the committed click_eval.npz array for array.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'click_eval.npz')
sys.path.insert(0, HERE)

from make_click_goldens import RADIUS, ZOOM_DEFAULTS, u16      # noqa: E402

NEAR = 2e-3                     # tests/test_gpu_click.py: max |p - p64| of the click network
PRED_THR = 0.49
MAX_CLICKS = 6
N_SUCCESSIVE = 3
EVAL_ZOOM = dict(target_size=128, min_crop_size=32)
N_EVAL = 3


# ---- (a) clicker cases ------------------------------------------------------------------------------------------------------
def _ellipse(H, W, cy, cx, ay, ax):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return ((yy - cy) / ay) ** 2 + ((xx - cx) / ax) ** 2 <= 1.0


def _runs(n, seed):
    """a 0/1 sequence of random runs"""
    rng = np.random.RandomState(seed)
    out = np.zeros(n, np.int8)
    i, v = 0, 0
    while i < n:
        k = int(rng.randint(1, 12))
        out[i:i + k] = v
        i, v = i + k, 1 - v
    return out


def _c_1x1():
    return np.ones((1, 1), np.int8), np.zeros((1, 1), bool)


def _c_1x70():
    gt = _runs(70, 1)[None]
    return gt, np.roll(gt, 3, 1).astype(bool)


def _c_70x1():
    gt = _runs(70, 2)[:, None]
    return gt, np.roll(gt, -2, 0).astype(bool)


def _c_5x300():          # fn wider than 256 columns
    gt = np.zeros((5, 300), np.int8)
    gt[:, 10:290] = 1
    pred = np.zeros((5, 300), bool)
    pred[0, 295:] = True
    return gt, pred


def _c_300x5():          # fp taller than 256 rows
    gt = np.zeros((300, 5), np.int8)
    gt[296:, 0] = 1
    pred = np.zeros((300, 5), bool)
    pred[7:291, :] = True
    return gt, pred


def _c_all_fn():
    return np.ones((37, 53), np.int8), np.zeros((37, 53), bool)


def _c_equal():
    gt = _ellipse(37, 53, 18, 26, 9, 14).astype(np.int8)
    return gt, gt.astype(bool)


def _c_corners():
    gt = np.ones((37, 53), np.int8)
    gt[0, 0] = gt[0, -1] = gt[-1, 0] = gt[-1, -1] = 0
    return gt, np.zeros((37, 53), bool)


def _c_checker():
    yy, xx = np.mgrid[0:37, 0:53]
    gt = ((yy + xx) % 2).astype(np.int8)
    return gt, gt == 0


def _c_rect_ties():      # a symmetric rectangle: a whole medial segment of tied maxima
    gt = np.zeros((97, 131), np.int8)
    gt[20:60, 30:100] = 1
    return gt, np.zeros((97, 131), bool)


def _c_fn_fp_tie():      # equal squares of fn and fp: fn_max == fp_max -> a negative click
    gt = np.zeros((97, 131), np.int8)
    gt[10:31, 15:36] = 1
    pred = np.zeros((97, 131), bool)
    pred[50:71, 80:101] = True
    return gt, pred


def _c_border():         # an error region on the border: the ring of zeros moves the maximum inwards
    gt = np.zeros((97, 131), np.int8)
    gt[0:30, 0:40] = 1
    gt[70:97, 100:131] = 1
    pred = np.zeros((97, 131), bool)
    pred[70:97, 100:131] = True
    pred[60:97, 0:20] = True
    return gt, pred


def _c_blobs_ignore():
    gt = _ellipse(97, 131, 48, 65, 20, 30).astype(np.int8)
    gt[40:56, 60:64] = -1
    gt[0:97, 120:131] = -1
    pred = _ellipse(97, 131, 52, 75, 22, 26) | _ellipse(97, 131, 15, 20, 8, 8)
    return gt, pred


def _c_noise_ignore():
    rng = np.random.RandomState(7)
    gt = (rng.rand(64, 256) < 0.6).astype(np.int8)
    gt[rng.rand(64, 256) < 0.05] = -1
    return gt, rng.rand(64, 256) < 0.4


def _c_wide_ignore():
    gt = np.zeros((64, 256), np.int8)
    gt[4:60, 8:250] = 1
    gt[30:34, :] = -1
    pred = np.zeros((64, 256), bool)
    pred[20:44, 100:140] = True
    return gt, pred


CLICKER_CASES = {'k_1x1': _c_1x1, 'k_1x70': _c_1x70, 'k_70x1': _c_70x1, 'k_5x300': _c_5x300, 'k_300x5': _c_300x5, 'k_all_fn': _c_all_fn,
                 'k_equal': _c_equal, 'k_corners': _c_corners, 'k_checker': _c_checker, 'k_rect_ties': _c_rect_ties,
                 'k_fn_fp_tie': _c_fn_fp_tie, 'k_border': _c_border, 'k_blobs_ignore': _c_blobs_ignore, 'k_noise_ignore': _c_noise_ignore,
                 'k_wide_ignore': _c_wide_ignore}


def clicker_case(name):
    """(gt int8 [H,W] with -1 = ignore, pred bool [H,W])"""
    gt, pred = CLICKER_CASES[name]()
    return np.ascontiguousarray(gt, np.int8), np.ascontiguousarray(pred, bool)


# ---- (b) evaluate_sample candidates -----------------------------------------------------------------------------------------------
# ground truth: the synthetic ellipse of synthetic_masks plus a second blob (cy, cx, ay, ax)
# With the synthetic weights the first click's mask is the best of a run (IoU 0.16 to 0.49) and every later one is worse, so a run
# either stops at its first click or runs out: max_iou_thr is set below the first IoU in one case and out of reach in the others.
EVAL_CANDIDATES = (
    dict(H=97, W=131, seed=21, blob=(20, 25, 9, 12), max_iou_thr=0.60),        # passed over: near pixels move its second click
    dict(H=97, W=131, seed=22, blob=(75, 105, 10, 14), max_iou_thr=0.95),
    dict(H=90, W=120, seed=23, blob=(22, 95, 10, 11), max_iou_thr=0.15),
    dict(H=97, W=131, seed=25, blob=(40, 50, 38, 48), max_iou_thr=0.99),
    dict(H=97, W=131, seed=24, blob=(78, 22, 9, 13), max_iou_thr=0.70),
)


def eval_image(c):
    sys.path.insert(0, ROOT)
    from xmem2_amd.synth import synthetic_frames
    return synthetic_frames(1, c['H'], c['W'], seed=c['seed'])[0]


def eval_gt(c):
    sys.path.insert(0, ROOT)
    from xmem2_amd.synth import synthetic_masks
    gt = synthetic_masks(1, 1, c['H'], c['W'])[0, 0] > 0.5
    return (gt | _ellipse(c['H'], c['W'], *c['blob'])).astype(np.int32)


def eval_zoom():
    zoom = dict(ZOOM_DEFAULTS)
    zoom.update(EVAL_ZOOM)
    return zoom


# ---- (c) NoC helpers -----------------------------------------------------------------------------------------------------------
NOC_CASES = {
    'm_mixed': dict(ious=[[0.3, 0.7, 0.82, 0.91], [0.85], [0.1, 0.2, 0.3], [0.5, 0.86, 0.84, 0.95, 0.99]], thrs=[0.8, 0.85, 0.9], max_clicks=20,
                    elapsed=12.5),
    'm_never': dict(ious=[[0.1, 0.2], [0.3, 0.4, 0.5]], thrs=[0.8, 0.85, 0.9], max_clicks=5, elapsed=3661.0),
    'm_one_thr': dict(ious=[[0.9], [0.2, 0.9]], thrs=[0.9], max_clicks=20, elapsed=0.75),
    'm_exact': dict(ious=[[0.8, 0.85, 0.9], [np.float32(0.85), 0.9]], thrs=[0.8, 0.85, 0.9], max_clicks=3, elapsed=100.0),
}


def noc_ious(name):
    return [np.array(v, np.float32) for v in NOC_CASES[name]['ious']]


def _reference(path):
    for name, kind in (('bool', bool), ('int', int)):                         # clicker.py:87, utils.py:122
        if not hasattr(np, name):                                             # (numpy 2 has np.bool again, as its own scalar type)
            setattr(np, name, kind)
    sys.path.insert(0, path)
    from inference.interact.fbrs.utils.cython import get_dist_maps            # noqa: F401  (pyximport: stops here without Cython)
    from inference.interact.fbrs.inference import utils
    from inference.interact.fbrs.inference.clicker import Clicker
    from inference.interact.fbrs.inference.evaluation import evaluate_sample
    from inference.interact.fbrs.inference.predictors import get_predictor
    return utils, Clicker, evaluate_sample, get_predictor


class _MapPredictor:
    """The reference predictor with get_prediction returning the map [H,W] as float64 numpy, every map kept."""

    def __init__(self, predictor, dtype):
        self.predictor, self.dtype, self.maps = predictor, dtype, []

    def set_input_image(self, image):
        self.predictor.set_input_image(image.to(self.dtype))

    def get_prediction(self, clicker):
        p = self.predictor.get_prediction(clicker).double().cpu().numpy()[0, 0]
        self.maps.append(p)
        return p


def _run_eval(torch, ref, model, c, dtype):
    utils, Clicker, evaluate_sample, get_predictor = ref
    pred = _MapPredictor(get_predictor(model, 'NoBRS', 'cpu', prob_thresh=PRED_THR, zoom_in_params=eval_zoom(),
                                       predictor_params={'net_clicks_limit': None, 'max_size': 800}), dtype)
    gt = eval_gt(c)
    clicks, ious, _ = evaluate_sample(torch.from_numpy(eval_image(c)), gt, pred, c['max_iou_thr'], pred_thr=PRED_THR, max_clicks=MAX_CLICKS)
    assert len(clicks) == len(ious) == len(pred.maps)
    return [(int(bool(k.is_positive)), int(k.coords[0]), int(k.coords[1])) for k in clicks], pred.maps


def _try_candidate(torch, ref, net32, net64, c):
    """-> (record dict, None) or (None, why the candidate is unfit)"""
    utils, Clicker = ref[0], ref[1]
    gt = eval_gt(c)
    clicks, maps = _run_eval(torch, ref, net64, c, torch.float64)
    clicks32, maps32 = _run_eval(torch, ref, net32, c, torch.float32)
    if clicks32 != clicks:
        return None, f'the fp32 run clicks {clicks32}, the float64 run {clicks}'
    err32 = max(float(np.abs(a - b).max()) for a, b in zip(maps, maps32))
    ious, inters, unions, nears = [], [], [], []
    for k, p in enumerate(maps):
        mask = p > PRED_THR
        near = np.abs(p - PRED_THR) <= NEAR
        inter, union = int((mask & (gt == 1)).sum()), int((mask | (gt == 1)).sum())
        iou = float(utils.get_iou(gt, mask))
        assert iou == inter / union
        n = int(near.sum())
        if not abs(iou - c['max_iou_thr']) > n / union:
            return None, f'step {k}: IoU {iou:.4f} is within near / union = {n}/{union} of the threshold {c["max_iou_thr"]}'
        if k + 1 < len(maps):
            for forced in (True, False):
                alt = Clicker(gt_mask=gt, init_clicks=[_click(Clicker, t) for t in clicks[:k + 1]])
                alt.make_next_click(np.where(near, forced, mask))
                got = alt.get_clicks()[-1]
                if (int(bool(got.is_positive)), int(got.coords[0]), int(got.coords[1])) != clicks[k + 1]:
                    return None, f'step {k}: with the {n} near pixels forced to {int(forced)} the next click moves'
        ious.append(iou), inters.append(inter), unions.append(union), nears.append(n)
    stopped = ious[-1] >= c['max_iou_thr']
    assert stopped or len(clicks) == MAX_CLICKS
    print(f'  clicks {clicks}\n  ious {[round(v, 4) for v in ious]} near {nears} union {unions} stop {"early" if len(clicks) < MAX_CLICKS else "at the limit"}'
          f' fp32 vs float64 {err32:.2e}')
    return dict(clicks=np.array(clicks, np.int32).reshape(-1, 3), prob64_u16=u16(np.stack(maps)), iou64=np.array(ious, np.float64),
                inter=np.array(inters, np.int32), union=np.array(unions, np.int32), near=np.array(nears, np.int32),
                geometry=np.array([c['H'], c['W'], c['seed']], np.int32), blob=np.array(c['blob'], np.float64),
                max_iou_thr=np.array(c['max_iou_thr'], np.float64), gt=gt.astype(np.int8)), None


def _click(Clicker, t):
    from inference.interact.fbrs.inference.clicker import Click
    return Click(is_positive=bool(t[0]), coords=(t[1], t[2]))


def generate(reference):
    import torch
    torch.set_grad_enabled(False)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = _reference(reference)
    utils, Clicker = ref[0], ref[1]
    rec = {}

    # (a)
    for name in CLICKER_CASES:
        gt, pred = clicker_case(name)
        clicker = Clicker(gt_mask=gt.astype(np.int32))
        for _ in range(N_SUCCESSIVE):
            clicker.make_next_click(pred)
        clicks = np.array([(int(bool(k.is_positive)), int(k.coords[0]), int(k.coords[1])) for k in clicker.get_clicks()], np.int32)
        with np.errstate(invalid='ignore', divide='ignore'):
            iou = np.float64(utils.get_iou(gt.astype(np.int32), pred))
        print(f'{name} {gt.shape}: clicks {clicks.tolist()} iou {iou:.4f}')
        rec[f'{name}_gt'], rec[f'{name}_pred'] = gt, pred.astype(np.uint8)
        rec[f'{name}_clicks'], rec[f'{name}_iou'] = clicks, np.array(iou, np.float64)

    # (c)
    for name, c in NOC_CASES.items():
        ious = noc_ious(name)
        noc, over = utils.compute_noc_metric(ious, c['thrs'], max_clicks=c['max_clicks'])
        spc, spi = utils.get_time_metrics(ious, c['elapsed'])
        header, row = utils.get_results_table(noc, over, 'NoBRS', 'synthetic', spc, c['elapsed'], n_clicks=c['max_clicks'], model_name='m')
        rec[f'{name}_noc'], rec[f'{name}_over'] = np.array(noc, np.float64), np.array(over, np.int64)
        rec[f'{name}_time'] = np.array([spc, spi], np.float64)
        rec[f'{name}_table'] = np.array([header, row])

    # (b)
    from xmem2_amd.synth import synthetic_click_state_dict
    sd = synthetic_click_state_dict(0)
    net32 = utils.load_is_model(dict(sd), 'cpu', cpu_dist_maps=True, norm_radius=RADIUS)
    net64 = utils.load_is_model(dict(sd), 'cpu', cpu_dist_maps=True, norm_radius=RADIUS).double()
    kept = []
    for i, c in enumerate(EVAL_CANDIDATES):
        if len(kept) == N_EVAL:
            break
        print(f'candidate {i}: {c}')
        out, why = _try_candidate(torch, ref, net32, net64, c)
        if out is None:
            print(f'  passed over: {why}')
            continue
        out['candidate'] = np.array(i, np.int32)
        kept.append(out)
    assert len(kept) == N_EVAL, f'only {len(kept)} of the candidates hold the stability conditions'
    lengths = [len(k['clicks']) for k in kept]
    assert min(lengths) < MAX_CLICKS and max(lengths) == MAX_CLICKS and any(k['iou64'][-1] < k['max_iou_thr'] for k in kept), \
        f'one run must stop early and one must run out of clicks: lengths {lengths}'
    for j, k in enumerate(kept):
        for key, v in k.items():
            rec[f'e{j}_{key}'] = v
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('XMEM_REFERENCE'), required='XMEM_REFERENCE' not in os.environ,
                    help='checkout of the reference project (default: $XMEM_REFERENCE)')
    ap.add_argument('--check', action='store_true', help='compare with the committed file instead of writing it')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec = generate(args.reference)
    if args.check:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(rec), (sorted(old.files), sorted(rec))
        for k in rec:
            assert old[k].dtype == rec[k].dtype and np.array_equal(old[k], rec[k], equal_nan=old[k].dtype.kind == 'f'), f'{k} differs'
        print('click_eval.npz reproduced array for array')
        return
    np.savez_compressed(OUT, **rec)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, f'click_eval.npz is {size} bytes: over the size limit of a committed file'
    print('wrote', OUT, size, 'bytes')


if __name__ == '__main__':
    main()
