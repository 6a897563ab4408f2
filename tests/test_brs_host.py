"""Host side of the f-BRS click refinement: the float64 restatement against the reference's recorded objective, the click squares,
the controllers' validation, and the optimiser loop replayed on the recorded evaluations of the golden cases (no GPU)."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brs_refs                                                   # noqa: E402

_spec = importlib.util.spec_from_file_location('make_brs_goldens', os.path.join(GOLDEN, 'make_brs_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

NEW_SYMBOLS = ('xmem_brs_affine_nhwc', 'xmem_relu_gate_nhwc', 'xmem_relu_gate_outer_nhwc', 'xmem_brs_loss', 'xmem_brs_param_grad')


@pytest.fixture(scope='module')
def click_sd():
    from xmem2_amd.synth import synthetic_click_state_dict
    return synthetic_click_state_dict(0)


def _restatement_lists():
    R = G.RESTATEMENT
    cl = list(R['clicks'])
    return [cl, [(p, (r, R['W'] - c - 1)) for p, (r, c) in cl]], (R['H'], R['W'])


@pytest.mark.parametrize('name', sorted(G.RESTATEMENT_MODES))
def test_restatement_reproduces_the_recorded_objective(click_sd, name):
    gd = load_golden('brs')
    lists, size = _restatement_lists()
    pos, neg = brs_refs.click_maps(lists, size)
    assert [int(pos.sum()), int(neg.sum())] == gd[f'{name}_pixels'].tolist()
    feat, x = G.restatement_inputs(name)
    got = brs_refs.objective(click_sd, feat, x, pos, neg, size, G.RESTATEMENT_MODES[name])
    f, grad = float(gd[f'{name}_f']), gd[f'{name}_grad'].astype(np.float64)
    # the reference's float64 run keeps float32 pieces: x and the click maps are float32 tensors, so the mask sums + 1e-5 and the
    # regulariser are rounded to float32 (2^-24 relative each, two of them in f), and the gradient is handed over as float32
    assert abs(got['f'] - f) <= 4 * 2.0 ** -24 * abs(f), (got['f'], f)
    assert np.abs(got['grad'] - grad).max() <= 4 * 2.0 ** -24 * np.abs(grad).max()


def test_click_squares_match_numpy_slicing():
    from xmem2_amd.click import Click
    from xmem2_amd.click_brs import click_squares, flipped_clicks
    H, W = 25, 33
    clicks = [(True, (0.0, 0.0)), (True, (12.0, 16.0)), (False, (0.5, 7.0)), (False, (1.5, 7.5)), (True, (2.5, 3.5)), (False, (24.0, 32.0)),
              (True, (24.4, 0.6)), (True, (13.0, 17.0)), (False, (5.0, 0.4)), (True, (23.5, 31.5))]
    ours = [Click(p, c) for p, c in clicks]
    lists = [ours, flipped_clicks(ours, W)]
    assert [c.coords for c in lists[1]] == [(r, W - c - 1) for _, (r, c) in clicks]
    rects = click_squares(lists, (H, W))
    assert rects.dtype == np.int32 and rects.shape == (2, len(clicks), 5)
    pos, neg = brs_refs.maps_from_squares(rects, (H, W))
    ref_pos, ref_neg = brs_refs.click_maps([[(c.is_positive, c.coords) for c in cl] for cl in lists], (H, W))
    assert np.array_equal(pos, ref_pos) and np.array_equal(neg, ref_neg)
    assert rects[0, 0, 0] == rects[0, 0, 1] or rects[0, 0, 2] == rects[0, 0, 3], 'the square of a click at (0, 0) is empty in numpy'
    before = brs_refs.click_maps([[(True, (12.0, 16.0))]], (H, W))[0].sum()
    assert brs_refs.click_maps([[(True, (12.0, 16.0)), (True, (0.0, 0.0))]], (H, W))[0].sum() == before == 9
    # half to even: rows 0.5 -> 0 (empty), 1.5 -> 2, 2.5 -> 2
    assert rects[0, 2, 0] == rects[0, 2, 1] and rects[0, 3, :2].tolist() == [1, 4] and rects[0, 4, :2].tolist() == [1, 4]
    assert rects[0, 5].tolist() == [23, 25, 31, 33, 0], 'clipped at the far edges'
    assert (rects[:, :, 1] - rects[:, :, 0]).max() <= 3 and (rects[:, :, 3] - rects[:, :, 2]).max() <= 3
    assert (rects[:, :, :4] >= 0).all() and (rects[:, :, 1] <= H).all() and (rects[:, :, 3] <= W).all()


def test_controller_validation(monkeypatch):
    from xmem2_amd import click_brs
    from xmem2_amd.click import FBRSController
    for mode in ('f-BRS-A', 'RGB-BRS', 'DistMap-BRS'):
        with pytest.raises(NotImplementedError, match='not built'):
            click_brs.FeatureBRSController(None, brs_mode=mode)
    with pytest.raises(ValueError):
        click_brs.FeatureBRSController(None, brs_mode='nonsense')
    with pytest.raises(ValueError):
        click_brs.FeatureBRSController(None, brs_opt_func_params={'no_such': 1})
    with pytest.raises(NotImplementedError, match='first click is identical') as e:
        FBRSController(None, brs_mode='f-BRS-B')
    assert 'FeatureBRSController' in str(e.value)
    assert click_brs.lbfgs_params({'maxfun': 20}) == {'m': 20, 'factr': 0, 'pgtol': 1e-8, 'maxfun': 20, 'maxiter': 40}
    assert click_brs.lbfgs_params({'maxfun': 7, 'm': 3})['maxiter'] == 14
    import inspect
    sig = inspect.signature(click_brs.FeatureBRSController.__init__).parameters
    assert sig['brs_mode'].default == 'f-BRS-B' and sig['net_clicks_limit'].default == 8 and sig['optimize_after_n_clicks'].default == 1
    assert inspect.signature(FBRSController.__init__).parameters['brs_mode'].default == 'NoBRS'
    monkeypatch.setitem(sys.modules, 'scipy.optimize', None)
    with pytest.raises(ImportError, match='scipy'):
        click_brs.FeatureBRSController(None, brs_mode='f-BRS-B')
    with pytest.raises(ImportError, match='scipy'):
        click_brs.BRSOptimizer()


def test_cli_brs_mode_flag(tmp_path):
    from xmem2_amd import click as C
    clicks = tmp_path / 'c.json'
    clicks.write_text('{"0": [{"object": 1, "x": 1, "y": 1, "positive": true}]}')
    base = ['--images', str(tmp_path), '--clicks', str(clicks), '--out', str(tmp_path / 'o'), '--synthetic-seed', '0']
    assert C.parse_args(base).brs_mode == 'NoBRS'
    assert C.parse_args(base + ['--brs-mode', 'f-BRS-B']).brs_mode == 'f-BRS-B'
    assert C.parse_args(base + ['--brs-mode', 'f-BRS-C']).brs_mode == 'f-BRS-C'
    with pytest.raises(SystemExit):
        C.parse_args(base + ['--brs-mode', 'f-BRS-A'])


def test_new_symbols_and_abi_version():
    from xmem2_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.xmem_version() == _lib.ABI_VERSION == 5


# ---- the optimiser loop on the recorded evaluations ------------------------------------------------------------------------------

class _Replay:
    """An objective (and engine) that answers every evaluation with the reference's recorded one."""

    def __init__(self, C):
        self.num_channels, self.C = C, C
        self.logits = self.best_logits = torch.zeros(2, 1, 1)
        self.records, self.asked, self.forwards, self.best_at, self.kept_masks = None, [], [], None, 0

    # engine
    def features(self, image, points, with_flip=True):
        return torch.zeros(2, 1, 1, self.C)

    def objective(self, feat_shape, H, W, num_clicks, reg_weight, reg_bias_weight):
        assert (reg_weight, reg_bias_weight) == (1e-3, 10.0)
        return self

    # objective
    def begin(self, input_data, rects):
        self.asked, self.forwards, self.best_at, self.kept_masks = [], [], None, 0

    def evaluate(self, x32):
        assert x32.dtype == np.float32
        if self.records is None:            # a click without optimisation: the predictor runs one forward at opt_data
            self.forwards.append(x32.copy())
            return dict(f=np.float32(0), f_max_pos=1.0, f_max_neg=1.0, inter=[0, 0], union=[0, 0], grad=np.zeros(2 * self.C, np.float32))
        k = len(self.asked)
        assert k < len(self.records['f']), 'the loop asks for more evaluations than the reference ran'
        self.asked.append(x32.copy())
        r = self.records
        iou = r['iou'][k]
        scale = 10 ** 6
        inter = [int(round(float(v) * scale)) if v >= 0 else 0 for v in iou]
        union = [scale if v >= 0 else 0 for v in iou]
        return dict(f=np.float64(r['f'][k]), f_max_pos=r['fmax'][k, 0], f_max_neg=r['fmax'][k, 1], inter=inter, union=union,
                    grad=r['grad'][k].copy())

    def keep_best(self):
        self.best_at = len(self.asked) - 1

    def keep_mask(self):
        self.kept_masks += 1


def _records(gd, name, i):
    if f'{name}_f{i}' not in gd.files:
        return None
    return {k: gd[f'{name}_{k}{i}'] for k in ('x', 'f', 'grad', 'fmax', 'stop', 'iou')}


@pytest.mark.parametrize('name', ['b1', 'c1'])
def test_host_loop_replays_the_recorded_optimisation(monkeypatch, name):
    from xmem2_amd import click_brs
    from xmem2_amd.click import Click
    gd = load_golden('brs')
    c = G.BRS_CASES[name]
    C = 128 + (32 if c['mode'] == 'f-BRS-B' else 0)
    monkeypatch.setattr(click_brs.ops, 'click_prob', lambda logits, H, W: torch.zeros(H, W))
    stub = _Replay(C)
    pred = click_brs.FeatureBRSPredictor(None, click_brs.INSERTION_MODES[c['mode']], net_clicks_limit=c['limit'], zoom_in=None, max_size=None,
                                         prob_thresh=0.5, min_iou_diff=1e-3, lbfgs={'maxfun': 20}, engine=stub)
    pred.set_input_image(torch.zeros(3, c['H'], c['W']))
    clicks, states, opt_after = [], [], []

    def click(i, step):
        stub.records = _records(gd, name, i)
        states.append(pred.get_states())
        clicks.append(Click(step[3], (step[2], step[1])))
        pred.get_prediction(clicks)
        n = int(gd[f'{name}_eval_counts'][i])
        assert len(stub.asked) == n == len(pred.opt_functor.evaluations), f'{name} click {i}: {len(stub.asked)} evaluations, the reference ran {n}'
        if n:
            r = stub.records
            assert np.abs(np.stack(stub.asked) - r['x']).max() <= 1e-6, f'{name} click {i}: the loop asked for other iterates'
            assert [e['stop'] for e in pred.opt_functor.evaluations] == r['stop'].tolist(), f'{name} click {i}: stops'
            assert stub.best_at == int(np.argmin(r['f'])), f'{name} click {i}: best evaluation'          # argmin: the first minimum, as strict <
            assert stub.kept_masks == int((r['stop'] == 0).sum())
            assert not stub.forwards, 'the best prediction is the result: no further forward'
        else:
            assert not pred.opt_functor.has_best and len(stub.forwards) == 1 and not stub.forwards[0].any()
        assert np.abs(np.asarray(pred.opt_data, np.float64) - gd[f'{name}_opt_data{i}']).max() <= 1e-6, f'{name} click {i}: opt_data'
        opt_after.append(np.array(pred.opt_data, np.float64))

    steps = [s for s in c['steps'] if s[0] == 'click']
    for i, step in enumerate(steps):
        click(i, step)
    assert np.abs(opt_after[1]).max() > 0 and not opt_after[0].any(), 'the first click must leave opt_data at zero, the second must move it'
    # undo the last two clicks: opt_data is the earlier one again, and the next click replays from it
    for _ in range(2):
        pred.set_states(states.pop())
        clicks.pop()
    assert np.array_equal(np.asarray(pred.opt_data, np.float64), opt_after[len(clicks) - 1])
    i = len(clicks)
    del opt_after[i:]
    click(i, steps[i])
    pred.set_input_image(torch.zeros(3, c['H'], c['W']))
    assert pred.opt_data is None and pred.input_data is None
