"""GPU: the robot user of click evaluation (csrc/edt.hip, xmem2_amd/click_eval.py) against the integer / scipy restatements of
tests/click_eval_refs.py and the reference's recorded clicks and runs (tests/golden/click_eval.npz).  Everything the robot computes
is integer arithmetic: every comparison of its own outputs is exact."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import click_eval_refs as R
from conftest import GOLDEN, load_golden
from xmem2_amd import ops

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('make_click_eval_goldens', os.path.join(GOLDEN, 'make_click_eval_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

THR32 = np.float32(G.PRED_THR)


def _planes(name):
    gt, pred = G.clicker_case(name)
    return np.stack(R.error_planes(gt, pred)).astype(np.uint8)


# ---- kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(G.CLICKER_CASES))
def test_edt_sq_equals_the_integer_restatement(name):
    planes = _planes(name)
    got = ops.edt_sq(torch.from_numpy(planes).cuda())
    want = np.stack([R.edt_sq_int(p) for p in planes])
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(ops.edt_sq(torch.from_numpy(planes[0]).cuda()).cpu(), torch.from_numpy(want[0]))      # [H,W]


def test_edt_sq_batch_of_different_planes():
    planes = np.stack([_planes('k_all_fn')[0], _planes('k_corners')[0], _planes('k_checker')[1]])
    assert planes.shape == (3, 37, 53)
    got = ops.edt_sq(torch.from_numpy(planes).cuda())
    assert torch.equal(got.cpu(), torch.from_numpy(np.stack([R.edt_sq_int(p) for p in planes])))


def test_click_errors_planes_and_counts():
    for name in ('k_blobs_ignore', 'k_noise_ignore', 'k_1x1', 'k_300x5'):
        gt, pred = G.clicker_case(name)
        gt8 = np.where(gt == -1, 255, gt).astype(np.uint8)
        prob = np.where(pred, np.float32(0.8), np.float32(0.2))
        prob[~pred & (np.arange(pred.size).reshape(pred.shape) % 3 == 0)] = THR32         # == threshold: not set
        want = np.stack(R.error_planes(gt, pred)).astype(np.uint8)
        for arg, thr in ((torch.from_numpy(prob).cuda(), G.PRED_THR), (torch.from_numpy(pred.astype(np.uint8)).cuda(), None)):
            planes, counts = ops.click_errors(arg, torch.from_numpy(gt8).cuda(), thr)
            assert torch.equal(planes.cpu(), torch.from_numpy(want)), name
            assert tuple(counts.cpu().tolist()) == R.iou_counts(gt, pred), name


# ---- the clicker ---------------------------------------------------------------------------------------------------------------
def _pred_forms(pred):
    prob = np.where(pred, np.float32(0.8), np.float32(0.2))
    return {'prob': (torch.from_numpy(prob).cuda(), G.PRED_THR), 'mask_u8': (torch.from_numpy(pred.astype(np.uint8)).cuda(), None),
            'mask_bool_host': (pred, None)}


@pytest.mark.parametrize('form', ['prob', 'mask_u8', 'mask_bool_host'])
@pytest.mark.parametrize('name', list(G.CLICKER_CASES))
def test_clicker_equals_the_reference(name, form):
    from xmem2_amd.click_eval import Clicker
    gd = load_golden('click_eval')
    gt, pred = G.clicker_case(name)
    arg, thr = _pred_forms(pred)[form]
    clicker = Clicker(gt_mask=gt.astype(np.int32))
    for _ in range(G.N_SUCCESSIVE):
        clicker.make_next_click(arg, thr)
        assert clicker.last_iou == gd[f'{name}_iou']
    got = [(int(c.is_positive), c.coords[0], c.coords[1]) for c in clicker.get_clicks()]
    assert got == [tuple(r) for r in gd[f'{name}_clicks'].tolist()]
    assert all(type(c.is_positive) is bool and type(c.coords[0]) is int and type(c.coords[1]) is int for c in clicker.get_clicks())
    assert len(clicker) == 3 and clicker.num_pos_clicks + clicker.num_neg_clicks == 3
    assert clicker.num_pos_clicks == int(gd[f'{name}_clicks'][:, 0].sum())
    want_nc = np.ones(gt.shape, np.uint8)
    for _p, r, c in got:
        want_nc[r, c] = 0
    assert torch.equal(clicker.not_clicked_map.cpu(), torch.from_numpy(want_nc))


def test_clicker_empty_union_is_nan_and_a_negative_click_at_the_origin():
    from xmem2_amd.click_eval import Clicker, get_iou
    gt = torch.zeros(9, 11, dtype=torch.uint8).cuda()
    clicker = Clicker(gt_mask=gt, ignore_label=255)
    clicker.make_next_click(torch.zeros(9, 11, dtype=torch.bool).cuda())
    assert clicker.get_clicks() == [(False, (0, 0))] and np.isnan(clicker.last_iou)
    assert np.isnan(get_iou(gt, torch.zeros(9, 11).cuda(), ignore_label=255, pred_thr=0.49))


def test_device_get_iou_and_ignore_label_of_a_device_ground_truth():
    from xmem2_amd.click_eval import Clicker, get_iou
    gd = load_golden('click_eval')
    gt, pred = G.clicker_case('k_blobs_ignore')
    gt8 = torch.from_numpy(np.where(gt == -1, 255, gt).astype(np.uint8)).cuda()
    assert get_iou(gt8, torch.from_numpy(pred).cuda(), ignore_label=255) == gd['k_blobs_ignore_iou']
    assert get_iou(gt.astype(np.int32), torch.from_numpy(pred).cuda()) == gd['k_blobs_ignore_iou']
    clicker = Clicker(gt_mask=gt8, ignore_label=255)
    clicker.make_next_click(torch.from_numpy(pred).cuda())
    assert (int(clicker.get_clicks()[0].is_positive),) + clicker.get_clicks()[0].coords == tuple(gd['k_blobs_ignore_clicks'][0].tolist())


def test_remove_last_click_and_set_state_restore_not_clicked():
    from xmem2_amd.click_eval import Clicker
    gt, pred = G.clicker_case('k_noise_ignore')
    predd = torch.from_numpy(pred).cuda()
    clicker = Clicker(gt_mask=gt.astype(np.int32))
    clicker.make_next_click(predd)
    state = clicker.get_state()
    clicker.make_next_click(predd)
    second = clicker.get_clicks()[-1]
    clicker.make_next_click(predd)
    third = clicker.get_clicks()[-1]
    assert third != second
    clicker._remove_last_click()
    clicker.make_next_click(predd)
    assert clicker.get_clicks()[-1] == third and len(clicker) == 3
    clicker.set_state(state)
    assert len(clicker) == 1 and int(clicker.not_clicked_map.sum()) == gt.size - 1
    clicker.make_next_click(predd)
    assert clicker.get_clicks()[-1] == second
    # clicks given at construction count as clicked
    other = Clicker(gt_mask=gt.astype(np.int32), init_clicks=clicker.get_clicks())
    other.make_next_click(predd)
    assert other.get_clicks()[-1] == third and other.num_pos_clicks + other.num_neg_clicks == 3
    other.reset_clicks()
    assert len(other) == 0 and bool((other.not_clicked_map == 1).all())


# ---- evaluate_sample against the reference's recorded runs -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def click_net():
    from xmem2_amd.click import ClickNet
    from xmem2_amd.synth import synthetic_click_state_dict
    return ClickNet(device='cuda:0').load_weights(synthetic_click_state_dict(0))


def _nobrs(net):
    from xmem2_amd.click import NoBRSPredictor, ZoomIn
    return NoBRSPredictor(net, None, True, ZoomIn(prob_thresh=0.5, **G.eval_zoom()), 800)


def _run(gd, j):
    c = G.EVAL_CANDIDATES[int(gd[f'e{j}_candidate'])]
    image = torch.from_numpy(G.eval_image(c)).cuda()
    return c, image, gd[f'e{j}_gt'].astype(np.int32)


def _clicks_of(rows):
    from xmem2_amd.click import Click
    return [Click(bool(p), (int(r), int(c))) for p, r, c in rows]


@pytest.mark.parametrize('j', range(G.N_EVAL))
def test_teacher_forced_masks_and_next_clicks(click_net, j):
    """with the reference's clicks so far, the HIP predictor's mask differs from the float64 mask only on near pixels, and the robot's
    next click on the device's own mask is the scipy restatement's on that mask"""
    from xmem2_amd.click_eval import Clicker
    gd = load_golden('click_eval')
    c, image, gt = _run(gd, j)
    clicks = _clicks_of(gd[f'e{j}_clicks'])
    predictor = _nobrs(click_net)
    predictor.set_input_image(image)
    for k in range(len(clicks)):
        prob = predictor.get_prediction(clicks[:k + 1])
        p64 = gd[f'e{j}_prob64_u16'][k].astype(np.float64) / 65535.0
        mine = prob.cpu().numpy() > THR32
        near = np.abs(p64 - G.PRED_THR) <= G.NEAR
        differ = mine != (p64 > G.PRED_THR)
        print(f'run {j} step {k}: {int(differ.sum())} pixels differ, {int(near.sum())} near (recorded {int(gd[f"e{j}_near"][k])}), '
              f'max |p - p64| {float(np.abs(prob.cpu().numpy() - p64).max()):.3e}')
        assert not (differ & ~near).any(), f'run {j} step {k}: {int((differ & ~near).sum())} decided pixels differ from float64'
        clicker = Clicker(gt_mask=gt, init_clicks=clicks[:k + 1])
        clicker.make_next_click(prob, G.PRED_THR)
        got = clicker.get_clicks()[-1]
        want = R.successive_clicks(gt, mine, 1, R.next_click_scipy, clicks=clicks[:k + 1])[0]
        assert (int(got.is_positive),) + got.coords == tuple(want.tolist()), f'run {j} step {k}'
        assert clicker.last_iou == R.get_iou(gt, mine)


@pytest.mark.parametrize('j', range(G.N_EVAL))
def test_evaluate_sample_follows_the_reference(click_net, j):
    from xmem2_amd.click_eval import evaluate_sample
    gd = load_golden('click_eval')
    c, image, gt = _run(gd, j)
    clicks, ious, prob = evaluate_sample(image, gt, _nobrs(click_net), c['max_iou_thr'], pred_thr=G.PRED_THR, max_clicks=G.MAX_CLICKS)
    got = [[int(k.is_positive), k.coords[0], k.coords[1]] for k in clicks]
    print(f'run {j}: clicks {got}\n ious {ious.tolist()}\n ious64 {gd[f"e{j}_iou64"].tolist()}')
    assert got == gd[f'e{j}_clicks'].tolist(), 'the click list or the stopping click differs from the reference'
    assert ious.dtype == np.float32 and len(ious) == len(got)
    bound = gd[f'e{j}_near'] / gd[f'e{j}_union']
    assert (np.abs(ious.astype(np.float64) - gd[f'e{j}_iou64']) <= bound).all()
    assert tuple(prob.shape) == gt.shape and prob.is_cuda
    assert float(ious[-1]) == np.float32(R.get_iou(gt, prob.cpu().numpy() > THR32))


class _Logged:
    """a predictor that keeps the mask of every answer on the host"""

    def __init__(self, predictor):
        self.predictor, self.masks = predictor, []

    def set_input_image(self, image):
        self.predictor.set_input_image(image)

    def get_prediction(self, clicks):
        prob = self.predictor.get_prediction(clicks)
        self.masks.append(prob.cpu().numpy() > THR32)
        return prob


def test_evaluate_sample_with_feature_brs(click_net):
    from xmem2_amd.click import ZoomIn
    from xmem2_amd.click_brs import FeatureBRSPredictor
    from xmem2_amd.click_eval import evaluate_sample
    gd = load_golden('click_eval')
    c, image, gt = _run(gd, 0)
    predictor = _Logged(FeatureBRSPredictor(click_net, 'after_aspp', 8, True, ZoomIn(prob_thresh=0.5, **G.eval_zoom()), 800,
                                            prob_thresh=0.5, min_iou_diff=1e-3, lbfgs={'maxfun': 20}))
    clicks, ious, prob = evaluate_sample(image, gt, predictor, 2.0, pred_thr=G.PRED_THR, max_clicks=3)
    assert len(clicks) == 3 and len(ious) == 3 and np.isfinite(ious).all() and len(predictor.masks) == 3
    masks = [np.zeros(gt.shape, bool)] + predictor.masks
    for k in range(3):
        want = R.successive_clicks(gt, masks[k], 1, R.next_click_scipy, clicks=[(q.is_positive, q.coords) for q in clicks[:k]])[0]
        assert (int(clicks[k].is_positive),) + clicks[k].coords == tuple(want.tolist()), f'click {k}'
        assert ious[k] == np.float32(R.get_iou(gt, predictor.masks[k]))


# ---- command line on a chair frame -------------------------------------------------------------------------------------------
def test_cli_clicks_reproduce_its_masks(click_net, tmp_path, capsys):
    """`run` (the command line behind its argument parser and weight loading) on one chair frame: the results table, and the clicks
    file replayed through FBRSController as `python -m xmem2_amd.click` does gives the mask it wrote"""
    import shutil
    from PIL import Image
    from xmem2_amd import click_eval as E
    from xmem2_amd.click import FBRSController, click_commit, load_clicks
    from xmem2_amd.scribble import IM_MEAN, IM_STD
    chair = os.path.join(GOLDEN, 'chair')
    (tmp_path / 'im').mkdir()
    (tmp_path / 'gt').mkdir()
    shutil.copy(os.path.join(chair, 'JPEGImages', 'frame_000000.jpg'), tmp_path / 'im')
    shutil.copy(os.path.join(chair, 'Annotations', 'frame_000000.png'), tmp_path / 'gt')
    args = E.parse_args(['--images', str(tmp_path / 'im'), '--masks', str(tmp_path / 'gt'), '--synthetic-seed', '0', '--max-clicks', '3',
                         '--clicks-out', str(tmp_path / 'clicks.json'), '--out', str(tmp_path / 'masks')])
    assert E.run(args, click_net) == 0
    table = capsys.readouterr().out
    assert 'NoC@85%' in table and '|    NoBRS    |' in table and '>=3@90%' in table
    clicks = load_clicks(str(tmp_path / 'clicks.json'))
    assert list(clicks) == [0] and 1 <= len(clicks[0]) <= 3 and all(c[0] == 1 for c in clicks[0])
    gt = np.array(Image.open(tmp_path / 'gt' / 'frame_000000.png'))
    first = R.successive_clicks((gt == 1).astype(np.int32), np.zeros(gt.shape, bool), 1, R.next_click_scipy)[0]
    assert (int(clicks[0][0][3]), clicks[0][0][2], clicks[0][0][1]) == tuple(first.tolist())
    img = np.array(Image.open(tmp_path / 'im' / 'frame_000000.jpg').convert('RGB'), dtype=np.uint8)
    image = torch.from_numpy(((img.astype(np.float32) / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1).copy()).cuda()
    ctl = FBRSController(click_net)
    for _k, x, y, positive in clicks[0]:
        obj = ctl.interact(image, x, y, positive)
    prob = torch.zeros(2, *gt.shape, device='cuda')
    prob[0] = 1
    _, mask = click_commit(prob, obj, 1)
    written = Image.open(tmp_path / 'masks' / 'frame_000000.png')
    assert written.mode == 'P' and np.array_equal(np.array(written), mask.cpu().numpy())
