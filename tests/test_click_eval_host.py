"""Host side of robot-click evaluation: the restatements of the robot against the reference's recorded clicks
(tests/golden/click_eval.npz), the NoC helpers against the reference's recorded outputs, the command line and the ABI.  No device."""
import importlib.util
import json
import os

import numpy as np
import pytest

import click_eval_refs as R
from conftest import GOLDEN, load_golden

_spec = importlib.util.spec_from_file_location('make_click_eval_goldens', os.path.join(GOLDEN, 'make_click_eval_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

NEW_SYMBOLS = ('xmem_click_errors', 'xmem_edt_sq', 'xmem_next_click_workspace_bytes', 'xmem_next_click')


@pytest.mark.parametrize('name', list(G.CLICKER_CASES))
def test_restatements_equal_the_reference_clicker(name):
    """both forms of the robot - scipy's float64 distances and the integer squared distances of the kernels - make the reference's
    three clicks, and the squared integer distance is the square of scipy's, everywhere"""
    from scipy.ndimage import distance_transform_edt
    gd = load_golden('click_eval')
    gt, pred = G.clicker_case(name)
    assert np.array_equal(gt, gd[f'{name}_gt']) and np.array_equal(pred, gd[f'{name}_pred'].astype(bool)), 'the case builder drifted'
    want = gd[f'{name}_clicks']
    assert want.shape == (G.N_SUCCESSIVE, 3)
    assert np.array_equal(R.successive_clicks(gt, pred, G.N_SUCCESSIVE, R.next_click_scipy), want)
    assert np.array_equal(R.successive_clicks(gt, pred, G.N_SUCCESSIVE, R.next_click_int), want)
    for plane in R.error_planes(gt, pred):
        edt = distance_transform_edt(np.pad(plane, 1))[1:-1, 1:-1]
        assert np.array_equal(np.rint(edt ** 2).astype(np.int32), R.edt_sq_int(plane))
    iou, want_iou = R.get_iou(gt, pred), gd[f'{name}_iou']
    assert (np.isnan(iou) and np.isnan(want_iou)) or iou == want_iou


def test_recorded_cases_hold_what_they_are_for():
    gd = load_golden('click_eval')
    assert gd['k_equal_clicks'].tolist() == [[0, 0, 0]] * 3                     # pred == gt: 0 > 0 is false, the first pixel
    assert gd['k_equal_iou'] == 1.0
    assert gd['k_fn_fp_tie_clicks'][0].tolist() == [0, 60, 90]                  # fn_max == fp_max: negative
    assert gd['k_fn_fp_tie_clicks'][1, 0] == 1                                  # ... and with that maximum clicked away, positive
    assert gd['k_1x1_clicks'].tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert gd['k_border_clicks'][0].tolist() == [1, 14, 14]                     # a 30 x 40 corner block: the ring moves the maximum inwards
    lengths = [len(gd[f'e{j}_clicks']) for j in range(G.N_EVAL)]
    assert min(lengths) < G.MAX_CLICKS == max(lengths)
    for j in range(G.N_EVAL):
        n = lengths[j]
        assert gd[f'e{j}_prob64_u16'].shape[0] == n and len(gd[f'e{j}_iou64']) == n
        thr = float(gd[f'e{j}_max_iou_thr'])
        margins = np.abs(gd[f'e{j}_iou64'] - thr) - gd[f'e{j}_near'] / gd[f'e{j}_union']
        assert (margins > 0).all()
        assert (gd[f'e{j}_iou64'][:-1] < thr).all() and (n == G.MAX_CLICKS or gd[f'e{j}_iou64'][-1] >= thr)


@pytest.mark.parametrize('j', range(G.N_EVAL))
def test_restatement_follows_the_recorded_runs(j):
    """on the recorded float64 maps the restatement makes every recorded click, with the near pixels forced either way"""
    gd = load_golden('click_eval')
    gt = gd[f'e{j}_gt'].astype(np.int32)
    c = G.EVAL_CANDIDATES[int(gd[f'e{j}_candidate'])]
    assert np.array_equal(gt, G.eval_gt(c))
    clicks = [(bool(p), (int(r), int(col))) for p, r, col in gd[f'e{j}_clicks']]
    assert R.successive_clicks(gt, np.zeros(gt.shape, bool), 1)[0].tolist() == gd[f'e{j}_clicks'][0].tolist()
    for k in range(len(clicks) - 1):
        p = gd[f'e{j}_prob64_u16'][k].astype(np.float64) / 65535.0
        mask = p > G.PRED_THR
        near = np.abs(p - G.PRED_THR) <= G.NEAR - 1.0 / 65535.0             # inside the recorded band whatever the uint16 rounding did
        for forced in (mask, mask | near, mask & ~near):
            got = R.successive_clicks(gt, forced, 1, clicks=clicks[:k + 1])[0]
            assert got.tolist() == gd[f'e{j}_clicks'][k + 1].tolist(), f'run {j} step {k}'


@pytest.mark.parametrize('name', list(G.NOC_CASES))
def test_noc_helpers_equal_the_reference(name):
    from xmem2_amd import click_eval as E
    gd = load_golden('click_eval')
    c = G.NOC_CASES[name]
    ious = G.noc_ious(name)
    noc, over = E.compute_noc_metric(ious, c['thrs'], max_clicks=c['max_clicks'])
    assert np.array_equal(np.array(noc, np.float64), gd[f'{name}_noc']) and np.array_equal(np.array(over, np.int64), gd[f'{name}_over'])
    spc, spi = E.get_time_metrics(ious, c['elapsed'])
    assert np.array_equal(np.array([spc, spi], np.float64), gd[f'{name}_time'])
    header, row = E.get_results_table(noc, over, 'NoBRS', 'synthetic', spc, c['elapsed'], n_clicks=c['max_clicks'], model_name='m')
    assert [header, row] == [str(s) for s in gd[f'{name}_table']]
    assert E.get_results_table(noc, over, 'NoBRS', 'synthetic', spc, c['elapsed'])[0].startswith('---')


def test_never_reached_counts_max_clicks():
    from xmem2_amd import click_eval as E
    gd = load_golden('click_eval')
    assert gd['m_never_noc'].tolist() == [5.0, 5.0, 5.0] and gd['m_never_over'].tolist() == [2, 2, 2]
    noc, over = E.compute_noc_metric([np.array([0.1, 0.95], np.float32), np.array([0.2], np.float32)], [0.9], max_clicks=7)
    assert noc == [4.5] and over == [1]


def test_get_iou_on_the_host():
    from xmem2_amd import click_eval as E
    gd = load_golden('click_eval')
    for name in ('k_blobs_ignore', 'k_noise_ignore', 'k_equal', 'k_all_fn'):
        gt, pred = G.clicker_case(name)
        assert E.get_iou(gt, pred) == gd[f'{name}_iou']
    assert np.isnan(E.get_iou(np.zeros((3, 4), np.int32), np.zeros((3, 4), bool)))
    assert E.get_iou(np.array([[1, 0]]), np.array([[0.6, 0.3]]), pred_thr=0.49) == 1.0


def test_oracle_eval_is_refused():
    from xmem2_amd import click_eval as E
    with pytest.raises(NotImplementedError, match='oracle_eval'):
        E.evaluate_dataset([], None, oracle_eval=True)


def test_cli_validation(tmp_path):
    from xmem2_amd import click_eval as E
    (tmp_path / 'im').mkdir()
    (tmp_path / 'gt').mkdir()
    base = ['--images', str(tmp_path / 'im'), '--masks', str(tmp_path / 'gt')]
    args = E.parse_args(base + ['--synthetic-seed', '0'])
    assert args.brs_mode == 'NoBRS' and args.max_clicks == 20 and args.iou_thrs == [0.8, 0.85, 0.9] and args.clicks_out is None and args.out is None
    args = E.parse_args(base + ['--synthetic-seed', '1', '--brs-mode', 'f-BRS-B', '--max-clicks', '5', '--iou-thrs', '0.5', '--out', 'o'])
    assert args.brs_mode == 'f-BRS-B' and args.max_clicks == 5 and args.iou_thrs == [0.5] and args.out == 'o'
    for argv in (base, base + ['--synthetic-seed', '0', '--model', 'x.pth'], base + ['--model', str(tmp_path / 'missing.pth')],
                 base + ['--synthetic-seed', '0', '--max-clicks', '0'], base + ['--synthetic-seed', '0', '--brs-mode', 'f-BRS-A'],
                 base + ['--synthetic-seed', '0', '--iou-thrs', '0.9', '0.8'], base + ['--synthetic-seed', '0', '--iou-thrs', '1.5'],
                 base + ['--synthetic-seed', '0', '--iou-thrs', '0.1', '0.2', '0.3', '0.4'],
                 ['--images', str(tmp_path / 'none'), '--masks', str(tmp_path / 'gt'), '--synthetic-seed', '0'],
                 ['--images', str(tmp_path / 'im'), '--masks', str(tmp_path / 'none'), '--synthetic-seed', '0']):
        with pytest.raises(SystemExit):
            E.parse_args(argv)


def test_clicks_json_round_trip(tmp_path):
    from xmem2_amd import click as C
    from xmem2_amd import click_eval as E
    per_frame = {7: [(2, C.Click(True, (4, 9))), (2, C.Click(False, (0, 0)))], 0: [(1, C.Click(np.bool_(True), (np.int32(3), np.int64(5))))],
                 3: []}
    doc = E.clicks_json(per_frame)
    assert list(doc) == ['0', '7']
    path = tmp_path / 'clicks.json'
    path.write_text(json.dumps(doc))
    assert C.load_clicks(str(path)) == {0: [(1, 5, 3, True)], 7: [(2, 9, 4, True), (2, 0, 0, False)]}


def test_new_symbols_and_abi_version():
    from xmem2_amd import _lib, build
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert 'edt.hip' in build.SOURCES
    assert lib.xmem_version() == _lib.ABI_VERSION == 5
    assert lib.xmem_next_click_workspace_bytes(480, 854) == 256 * 2 * 8 and lib.xmem_next_click_workspace_bytes(1, 1) == 16
    assert lib.xmem_next_click_workspace_bytes(16385, 4) == 0
    # argument checks run before anything touches a device
    assert lib.xmem_edt_sq(None, 1, 4, 4, None, None) == -1
    assert lib.xmem_edt_sq(1, 1, 16385, 4, 1, None) == -2 and lib.xmem_click_errors(None, 0.5, 1, 1, 4, 16385, 1, 1, None) == -2
    assert lib.xmem_click_errors(1, 0.5, 1, 1, 4, 4, 1, 1, None) == -1, 'both a probability map and a mask'
    assert lib.xmem_next_click(1, 1, None, 4, 4, 1, 8, 8, None) == -3
