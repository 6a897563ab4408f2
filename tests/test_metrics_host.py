"""DAVIS J&F (xmem2_amd/metrics.py, `xmem_jf_counts`) without a GPU: the host arithmetic against the reference's values
(tests/golden/jf.npz, written by make_jf_goldens.py from util/metrics.py itself), a numpy restatement of the kernel's counts that the
GPU tests (tests/test_gpu_metrics.py) compare the kernel against, the object-id and radius logic, the C ABI's argument checks and the
command-line surfaces."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

SLOTS = ('gt_area', 'pred_area', 'inter', 'n_gt', 'n_pred', 'gt_match', 'pred_match')


def golden_cases():
    z = np.load(os.path.join(GOLDEN, 'jf.npz'), allow_pickle=False)
    names = sorted({k.split('/')[0] for k in z.files})
    out = {}
    for n in names:
        nb = int(z[f'{n}/nb_objects'])
        out[n] = dict(gt=z[f'{n}/gt'], pred=z[f'{n}/pred'], bound_th=float(z[f'{n}/bound_th']), nb_objects=None if nb < 0 else nb,
                      J_obj=z[f'{n}/J_obj'], F_obj=z[f'{n}/F_obj'], J_avg=z[f'{n}/J_avg'], F_avg=z[f'{n}/F_avg'],
                      counts=z[f'{n}/counts'])
    return out


# ---- numpy restatement of xmem_jf_counts -----------------------------------------------------------------------------------------
def seg2bmap(m):
    """util/metrics.py _seg2bmap, width=None: (m^E) | (m^S) | (m^SE), last row m^E, last column m^S, bottom-right 0."""
    m = np.asarray(m, bool)
    e, s, se = np.zeros_like(m), np.zeros_like(m), np.zeros_like(m)
    e[:, :-1] = m[:, 1:]
    s[:-1, :] = m[1:, :]
    se[:-1, :-1] = m[1:, 1:]
    b = (m ^ e) | (m ^ s) | (m ^ se)
    b[-1, :] = m[-1, :] ^ e[-1, :]
    b[:, -1] = m[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def _shift(b, dy, dx):
    """out[y, x] = b[y + dy, x + dx], False outside the image."""
    H, W = b.shape
    out = np.zeros_like(b)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if H - abs(dy) > 0 and W - abs(dx) > 0:
        out[yd, xd] = b[ys, xs]
    return out


def dilate_disk(b, r):
    """cv2.dilate(b, disk(r)): OR of b shifted by every offset with dy^2 + dx^2 <= r^2 (rows first: the horizontal run of half-width
    floor(sqrt(r^2 - dy^2)) is built by shift-and-OR, then shifted by dy)."""
    runs = [b.copy()]
    for w in range(1, r + 1):
        runs.append(runs[-1] | _shift(b, 0, w) | _shift(b, 0, -w))
    out = np.zeros_like(b)
    for dy in range(-r, r + 1):
        out |= _shift(runs[math.isqrt(r * r - dy * dy)], dy, 0)
    return out


def jf_counts_reference(gt, pred, r, lut=None):
    """[B,256,7] int64 counts of xmem_jf_counts: labels 1..254, pred through `lut` first."""
    gt, pred = np.asarray(gt, np.uint8), np.asarray(pred, np.uint8)
    if gt.ndim == 2:
        gt, pred = gt[None], pred[None]
    if lut is not None:
        pred = np.asarray(lut, np.uint8)[pred]
    out = np.zeros((gt.shape[0], 256, 7), np.int64)
    for b in range(gt.shape[0]):
        for k in np.union1d(np.unique(gt[b]), np.unique(pred[b])):
            if k == 0 or k == 255:
                continue
            mg, mp = gt[b] == k, pred[b] == k
            bg, bp = seg2bmap(mg), seg2bmap(mp)
            dg, dp = dilate_disk(bg, r), dilate_disk(bp, r)
            out[b, k] = [mg.sum(), mp.sum(), (mg & mp).sum(), bg.sum(), bp.sum(), (bg & dp).sum(), (bp & dg).sum()]
    return out


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_host_formula_from_golden_counts_reproduces_the_reference():
    from xmem2_amd.metrics import object_ids, scores_from_counts
    for name, c in golden_cases().items():
        ids = object_ids(c['gt'], c['nb_objects'])
        J, F = scores_from_counts(c['counts'], ids)
        np.testing.assert_array_equal(J, c['J_obj'], err_msg=name)
        np.testing.assert_array_equal(F, c['F_obj'], err_msg=name)
        assert J.dtype == np.float64 and F.dtype == np.float64
        np.testing.assert_array_equal(J.mean(axis=1), c['J_avg'], err_msg=name)
        np.testing.assert_array_equal(F.mean(axis=1), c['F_avg'], err_msg=name)


def test_counts_restatement_equals_the_reference_counts():
    from xmem2_amd.metrics import bound_pix
    for name, c in golden_cases().items():
        r = bound_pix(c['bound_th'], c['gt'].shape[1:])
        np.testing.assert_array_equal(jf_counts_reference(c['gt'], c['pred'], r), c['counts'], err_msg=name)


def test_golden_cases_cover_what_they_claim():
    cases = golden_cases()
    from xmem2_amd.metrics import bound_pix
    assert bound_pix(0.008, cases['p480']['gt'].shape[1:]) == 8 and bound_pix(0.008, cases['p1080']['gt'].shape[1:]) == 18
    assert cases['bound3']['bound_th'] == 3.0 and cases['multi_nb8']['nb_objects'] == 8
    assert set(np.unique(cases['multi']['gt'])) == {0, 1, 3, 7}
    assert (cases['empty_pred']['pred'] == 0).all() and 255 in cases['absent_void']['gt']
    assert 5 in cases['absent_void']['pred'] and 5 not in cases['absent_void']['gt']
    assert cases['chair_shift']['gt'].shape == (10, 480, 720)


def test_object_ids_and_nb_objects():
    from xmem2_amd.metrics import object_ids
    gt = np.zeros((2, 4, 4), np.uint8)
    gt[0, 0, 0], gt[1, 1, 1], gt[1, 2, 2], gt[0, 3, 3] = 7, 3, 255, 3
    assert object_ids(gt).tolist() == [3, 7]                       # whole sequence, 0 and 255 excluded
    assert object_ids(gt, nb_objects=2).tolist() == [1, 2]
    assert object_ids(torch.from_numpy(gt)).tolist() == [3, 7]
    with pytest.raises(ValueError):
        object_ids(np.zeros((1, 3, 3), np.uint8))
    with pytest.raises(ValueError):
        object_ids(np.full((1, 3, 3), 255, np.uint8))
    with pytest.raises(ValueError):
        object_ids(gt, nb_objects=0)
    with pytest.raises(ValueError):
        object_ids(gt, nb_objects=255)


def test_reference_value_errors_come_before_the_gpu():
    from xmem2_amd.metrics import batched_f_measure, batched_jaccard
    for fn in (batched_jaccard, batched_f_measure):
        with pytest.raises(ValueError, match='y_true array must have 3 dimensions'):
            fn(np.zeros((4, 4), np.uint8), np.zeros((1, 4, 4), np.uint8))
        with pytest.raises(ValueError, match='y_pred array must have 3 dimensions'):
            fn(np.zeros((1, 4, 4), np.uint8), np.zeros((4, 4), np.uint8))
        with pytest.raises(ValueError, match='same shape'):
            fn(np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 5), np.uint8))
        with pytest.raises(ValueError, match='higher than 0'):
            fn(np.zeros((1, 4, 4), np.uint8), np.zeros((1, 4, 4), np.uint8))
        with pytest.raises(ValueError):
            fn(np.full((1, 4, 4), 300), np.zeros((1, 4, 4), np.int64))
    with pytest.raises(ValueError):
        batched_f_measure(np.ones((1, 4, 4), np.uint8), np.ones((1, 4, 4), np.uint8), bound_th=2.5)
    with pytest.raises(ValueError):
        batched_f_measure(np.ones((1, 4, 4), np.uint8), np.ones((1, 4, 4), np.uint8), bound_th=64)


def test_bound_pix():
    from xmem2_amd.metrics import bound_pix
    for shape in ((480, 854), (1080, 1920), (480, 720), (1, 50), (40, 1), (2, 2), (240, 427), (2160, 3840)):
        assert bound_pix(0.008, shape) == int(np.ceil(0.008 * np.linalg.norm(shape))), shape
    assert [bound_pix(0.008, s) for s in ((480, 854), (1080, 1920), (480, 720), (1, 50), (2, 2))] == [8, 18, 7, 1, 1]
    assert bound_pix(3, (10, 10)) == 3 and bound_pix(1.0, (10, 10)) == 1 and bound_pix(0, (10, 10)) == 0
    for bad in (1.5, 2.25, -0.1):
        with pytest.raises(ValueError):
            bound_pix(bad, (10, 10))


def test_restatement_on_hand_built_masks():
    m = np.zeros((4, 5), bool)
    m[1:3, 1:4] = True
    b = seg2bmap(m)
    # offset by 1/2 pixel towards the origin: the pixel above / left of an edge is marked, the last object row too
    assert b.astype(int).tolist() == [[1, 1, 1, 1, 0], [1, 0, 0, 1, 0], [1, 1, 1, 1, 0], [0, 0, 0, 0, 0]]
    full = np.ones((3, 3), bool)
    assert not seg2bmap(full).any()                                # the image border is not a boundary
    one = np.zeros((5, 5), bool)
    one[2, 2] = True
    assert dilate_disk(one, 1).astype(int).tolist() == [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0],
                                                        [0, 0, 0, 0, 0]]
    assert dilate_disk(one, 2).sum() == 13 and (dilate_disk(one, 0) == one).all()
    c = jf_counts_reference(np.array([[1, 1], [0, 2]], np.uint8), np.array([[2, 1], [0, 0]], np.uint8), 1,
                            lut=np.r_[[0, 1, 1], np.zeros(253, np.uint8)])
    assert c[0, 1].tolist() == [2, 2, 2, 2, 2, 2, 2]                  # the LUT maps pred's 2 to 1
    assert c[0, 2].tolist() == [1, 0, 0, 3, 0, 0, 0]                  # a bottom-right pixel marks its three up/left neighbours


def test_jf_counts_abi_rejects_bad_arguments_without_touching_the_gpu():
    from xmem2_amd import _lib
    lib = _lib.load()
    p = __import__('ctypes').c_void_p(16)        # never dereferenced: every call below fails its argument check first
    f = lib.xmem_jf_counts
    assert f(None, p, None, 1, 8, 8, 3, p, None) == -1                  # gt NULL
    assert f(p, None, None, 1, 8, 8, 3, p, None) == -1                  # pred NULL
    assert f(p, p, None, 1, 8, 8, 3, None, None) == -1                  # counts NULL
    for B, H, W, r in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, -1, 3), (-2, 8, 8, 3), (1, 8, 8, -1)):
        assert f(p, p, p, B, H, W, r, p, None) == -1
    assert f(p, p, None, 1, 8, 8, 64, p, None) == -2                    # radius beyond one neighbour word
    assert f(p, p, None, 1, 16385, 8, 3, p, None) == -2
    assert f(p, p, None, 1, 8, 16385, 3, p, None) == -2


def test_jf_counts_binding_rejects_cpu_and_mismatched_tensors():
    from xmem2_amd import ops
    with pytest.raises(RuntimeError):
        ops.jf_counts(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8), 1)


def test_evaluate_cli_arguments():
    from xmem2_amd.evaluate import parse_args
    a = parse_args(['--gt', 'A', '--pred', 'R'])
    assert (a.gt, a.pred, a.csv, a.workers) == ('A', 'R', None, 8)
    a = parse_args(['--gt', 'A', '--pred', 'R', '--csv', 'out.csv', '--workers', '3'])
    assert (a.csv, a.workers) == ('out.csv', 3)
    with pytest.raises(SystemExit):
        parse_args(['--gt', 'A'])
    with pytest.raises(SystemExit):
        parse_args(['--pred', 'R'])


def test_launcher_jf_means_and_summary(tmp_path):
    import json
    import pandas as pd
    from xmem2_amd.launch import jf_means, merge
    df = pd.DataFrame({'frame': ['a', 'b', 'c'], 'mask_provided': [True, False, False], 'J': [1.0, 0.5, np.nan], 'F': [0.5, 0.25, np.nan]})
    assert jf_means(df) == dict(mean_J=0.75, mean_F=0.375, mean_JF=0.5625)
    assert jf_means(df.drop(columns=['J', 'F'])) == dict(mean_J=None, mean_F=None, mean_JF=None)
    rows = [dict(name='v0', frames=3, seconds=1.0, fps=3.0, rank=0, mean_J=0.75, mean_F=0.375, mean_JF=0.5625),
            dict(name='v1', frames=2, seconds=1.0, fps=2.0, rank=0, mean_J=0.25, mean_F=0.125, mean_JF=0.1875)]
    with open(tmp_path / '_rank0.json', 'w') as f:
        json.dump(dict(rank=0, world=1, nonce='n', videos=rows), f)
    s = merge(str(tmp_path), 1, 2.0, 'n')
    assert (s['mean_J'], s['mean_F'], s['mean_JF']) == (0.5, 0.25, 0.375)
    with open(tmp_path / '_rank0.json', 'w') as f:                  # without --compute-jf the summary keeps today's keys
        json.dump(dict(rank=0, world=1, nonce='m', videos=[{k: v for k, v in r.items() if not k.startswith('mean')} for r in rows]), f)
    assert 'mean_J' not in merge(str(tmp_path), 1, 2.0, 'm')


def test_launcher_flag():
    import argparse
    from xmem2_amd import launch
    seen = {}
    orig = argparse.ArgumentParser.parse_args

    def spy(self, argv=None, namespace=None):
        a = orig(self, argv, namespace)
        seen.update(vars(a))
        raise SystemExit(0)
    argparse.ArgumentParser.parse_args = spy
    try:
        for argv, want in ((['--videos', 'v', '--out', 'o'], False), (['--videos', 'v', '--out', 'o', '--compute-jf'], True)):
            with pytest.raises(SystemExit):
                launch.main(argv)
            assert seen['compute_jf'] is want
    finally:
        argparse.ArgumentParser.parse_args = orig
