"""Host side of click-to-mask: architecture table, synthetic weights, ABI, the predictor's ROI / click arithmetic against the
reference's recorded sequences (tests/golden/click.npz), the command line's validation.  No device is involved."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

_spec = importlib.util.spec_from_file_location('make_click_goldens', os.path.join(GOLDEN, 'make_click_goldens.py'))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

NEW_SYMBOLS = ('xmem_click_input', 'xmem_depthwise3x3_nhwc', 'xmem_resize_bilinear_ac_nhwc', 'xmem_resize_bilinear_ac',
               'xmem_click_prob', 'xmem_mask_bbox', 'xmem_prob_threshold', 'xmem_click_commit')


def test_spec_matches_the_reference():
    from xmem2_amd.arch import click_state_dict_spec
    from xmem2_amd.click import state_dict_spec
    gd = load_golden('click')
    spec = click_state_dict_spec()
    assert len(spec) == 413 and spec == state_dict_spec()
    assert list(spec) == [str(n) for n in gd['spec_names']]
    assert [str(tuple(v)) for v in spec.values()] == [str(s) for s in gd['spec_shapes']]
    n_param = sum(int(np.prod(v)) for k, v in spec.items() if not re.search(r'running_|num_batches', k))
    assert n_param == 31396604            # the reference model's sum(p.numel() for p in parameters())
    wide = click_state_dict_spec(256)
    assert wide['feature_extractor.aspp.project.0.weight'] == (256, 1280, 1, 1) and wide['head.layers.2.weight'] == (1, 128, 1, 1)


def test_synthetic_state_dict_is_deterministic():
    from xmem2_amd.arch import click_state_dict_spec
    from xmem2_amd.synth import synthetic_click_state_dict
    a, b = synthetic_click_state_dict(0, as_torch=False), synthetic_click_state_dict(0, as_torch=False)
    spec = click_state_dict_spec()
    assert list(a) == list(spec) and all(tuple(a[k].shape) == tuple(spec[k]) for k in spec)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    other = synthetic_click_state_dict(1, as_torch=False)
    assert not np.array_equal(a['rgb_conv.0.weight'], other['rgb_conv.0.weight'])
    w = a['rgb_conv.0.weight'][:, :, 0, 0]
    assert np.abs(w[:, 3:]).mean() > 5 * np.abs(w[:, :3]).mean(), 'the click channels are not conditioned'
    assert np.isfinite(np.concatenate([v.reshape(-1) for v in a.values()]).astype(np.float64)).all()


def test_new_symbols_and_abi_version():
    from xmem2_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.xmem_version() == _lib.ABI_VERSION == 5


def test_load_refuses_other_architectures():
    from xmem2_amd.click import ClickNet
    net = ClickNet.__new__(ClickNet)           # the checks run before anything touches a device
    with pytest.raises(NotImplementedError, match='HRNet'):
        net.load_state_dict({'feature_extractor.stage2.0.branches.0.0.conv1.weight': np.zeros(1)})
    r34 = {f'feature_extractor.backbone.x{i}.weight': np.zeros(1) for i in range(180)}
    with pytest.raises(NotImplementedError, match='resnet34'):
        net.load_state_dict(r34)
    r101 = {f'feature_extractor.backbone.x{i}.weight': np.zeros(1) for i in range(500)}
    with pytest.raises(NotImplementedError, match='resnet101'):
        net.load_state_dict(r101)


def _clicks_of(name, upto):
    from xmem2_amd.click import Click
    out = []
    for step in G.NET_CASES[name]['steps'][:upto]:
        if step[0] == 'click':
            out.append(Click(step[3], (step[2], step[1])))
        elif step[0] == 'undo':
            out.pop()
    return out


def _prob(gd, name, i):
    return gd[f'{name}_prob64_u16'][i].astype(np.float64) / 65535.0


def test_roi_helpers_reproduce_n2():
    """from the recorded probabilities alone: the planted ROI, the recomputed ROI of click 3, working sizes and transformed clicks"""
    from xmem2_amd import click as C
    gd = load_golden('click')
    zoom = dict(G.ZOOM_DEFAULTS)
    zoom.update(G.NET_CASES['n2']['zoom'])
    H, W = G.NET_CASES['n2']['H'], G.NET_CASES['n2']['W']
    # click 2: the previous probabilities are the planted ellipse
    clicks = _clicks_of('n2', 3)
    box = C.mask_bbox_host(G.planted_probs('n2'), 0.5, C.positive_click_pixels(clicks))
    roi = C.get_object_roi(box, (H, W), zoom['expansion_ratio'], zoom['min_crop_size'])
    assert roi == tuple(gd['n2_rois'][1])
    size = C.roi_image_size(roi, zoom['target_size'])
    assert size == tuple(gd['n2_sizes'][1])
    assert np.array_equal(np.array([c.coords for c in C.transform_clicks(clicks, roi, size)], np.float64), gd['n2_clicks1'])
    # click 3 lies outside that ROI: recomputed from the result of click 2 (probability index 1)
    clicks = _clicks_of('n2', 4)
    assert not C.check_object_roi(roi, clicks)
    box = C.mask_bbox_host(_prob(gd, 'n2', 1), 0.5, C.positive_click_pixels(clicks))
    roi3 = C.get_object_roi(box, (H, W), zoom['expansion_ratio'], zoom['min_crop_size'])
    assert roi3 == tuple(gd['n2_rois'][2]) and roi3 != roi
    size3 = C.roi_image_size(roi3, zoom['target_size'])
    assert size3 == tuple(gd['n2_sizes'][2])
    assert np.array_equal(np.array([c.coords for c in C.transform_clicks(clicks, roi3, size3)], np.float64), gd['n2_clicks2'])
    # click 3' after the undo stays inside the planted ROI, whose IoU with the ROI of its own previous probabilities is high
    clicks = _clicks_of('n2', 6)
    assert C.check_object_roi(roi, clicks) and tuple(gd['n2_rois'][3]) == roi


def test_roi_helpers_reproduce_n3():
    from xmem2_amd import click as C
    gd = load_golden('click')
    c = G.NET_CASES['n3']
    zoom = dict(G.ZOOM_DEFAULTS)
    zoom.update(c['zoom'])
    full = (0, c['H'] - 1, 0, c['W'] - 1)
    assert tuple(gd['n3_limit_rois'][0]) == full
    size = C.roi_image_size(full, c['max_size'])                 # LimitLongestSide
    assert size == tuple(gd['n3_sizes'][0])
    clicks = _clicks_of('n3', 1)
    assert np.array_equal(np.array([k.coords for k in C.transform_clicks(clicks, full, size)], np.float64), gd['n3_clicks0'])
    clicks = _clicks_of('n3', 2)
    box = C.mask_bbox_host(_prob(gd, 'n3', 0), 0.5, C.positive_click_pixels(clicks))
    roi = C.get_object_roi(box, (c['H'], c['W']), zoom['expansion_ratio'], zoom['min_crop_size'])
    assert roi == tuple(gd['n3_rois'][1])
    size = C.roi_image_size(roi, zoom['target_size'])
    assert size == tuple(gd['n3_sizes'][1]) and max(size) <= c['max_size']      # LimitLongestSide returns early: the double resize
    assert np.array_equal(np.array([k.coords for k in C.transform_clicks(clicks, roi, size)], np.float64), gd['n3_clicks1'])


def test_bbox_helpers():
    from xmem2_amd import click as C
    assert C.expand_bbox((10, 19, 20, 39), 1.4) == (8, 22, 16, 44)             # 14.5 +- 7 -> round half to even: 8 (7.5), 22 (21.5)
    assert C.expand_bbox((10, 19, 20, 39), 1.0, 30) == (0, 30, 14, 44)
    assert C.clamp_bbox((-3, 50, 2, 99), 0, 40, 0, 60) == (0, 40, 2, 60)
    assert C.get_bbox_iou((0, 9, 0, 9), (0, 9, 0, 9)) == 1.0 and C.get_bbox_iou((0, 9, 0, 9), (10, 19, 0, 9)) == 0.0
    assert C.get_bbox_iou((0, 9, 0, 9), (5, 14, 0, 9)) == pytest.approx(5 / 15)
    pos = C.Click(True, (5.0, 7.9))
    assert C.check_object_roi((0, 10, 0, 10), [pos, C.Click(False, (50, 50))])
    assert not C.check_object_roi((0, 5, 0, 10), [pos])                       # the upper bounds are exclusive
    assert C.positive_click_pixels([pos, C.Click(False, (1, 1))]) == [(5, 7)]
    empty = C.mask_bbox_host(np.zeros((4, 5)), 0.5)
    assert empty[4] == 0 and empty[1] == -1
    assert C.mask_bbox_host(np.zeros((4, 5)), 0.5, [(2, 3)]) == (2, 2, 3, 3, 0)
    assert C.roi_image_size((0, 149, 0, 259), 200) == (115, 200)


def test_get_points_nd_padding_and_truncation():
    from xmem2_amd.click import Click, get_points_nd
    cl = [Click(True, (1, 2)), Click(False, (3, 4)), Click(True, (5, 6)), Click(True, (7, 8))]
    p = get_points_nd([cl])
    assert p.shape == (1, 6, 2) and p.dtype == np.float32
    assert p[0].tolist() == [[1, 2], [5, 6], [7, 8], [3, 4], [-1, -1], [-1, -1]]
    assert get_points_nd([[]])[0].tolist() == [[-1, -1], [-1, -1]]            # at least one (padding) point per polarity
    # net_clicks_limit keeps the FIRST clicks of the list, whatever their polarity
    p = get_points_nd([cl], net_clicks_limit=2)
    assert p[0].tolist() == [[1, 2], [-1, -1], [3, 4], [-1, -1]]
    p = get_points_nd([cl], net_clicks_limit=3)
    assert p[0].tolist() == [[1, 2], [5, 6], [-1, -1], [3, 4], [-1, -1], [-1, -1]]     # n = min(limit, max(3 positive, 1 negative))


def test_distance_closed_form_rounds_half_to_even():
    name, H, W, pos, neg = G.DIST_CASES[0]
    d = G.dist_closed_form(H, W, pos, neg)
    assert d[0, 0, 2] == 0 and d[0, 2, 10] == 0 and d[1, 11, 3] == 0
    assert d[0, 0, 1] > 0 and d[0, 2, 11] > 0 and d[1, 10, 3] > 0


def test_cli_validation(tmp_path):
    from xmem2_amd import click as C
    good = tmp_path / 'ok.json'
    good.write_text(json.dumps({'0': [{'object': 1, 'x': 3, 'y': 4.5, 'positive': True}], '7': [{'object': 2, 'x': 0, 'y': 0, 'positive': False}]}))
    assert C.load_clicks(str(good)) == {0: [(1, 3, 4.5, True)], 7: [(2, 0, 0, False)]}
    bad = [[1], {'a': []}, {'0': []}, {'0': [{'object': 0, 'x': 1, 'y': 1, 'positive': True}]},
           {'0': [{'object': 1, 'x': -1, 'y': 1, 'positive': True}]}, {'0': [{'object': 1, 'x': 1, 'y': 1, 'positive': 1}]},
           {'0': [{'object': 1, 'x': 1, 'y': 1}]}, {'0': [{'object': True, 'x': 1, 'y': 1, 'positive': True}]}]
    for i, doc in enumerate(bad):
        f = tmp_path / f'bad{i}.json'
        f.write_text(json.dumps(doc))
        with pytest.raises(ValueError):
            C.load_clicks(str(f))
    base = ['--images', str(tmp_path), '--clicks', str(good), '--out', str(tmp_path / 'o')]
    args = C.parse_args(base + ['--synthetic-seed', '0', '--num-objects', '3'])
    assert args.synthetic_seed == 0 and args.num_objects == 3 and args.model is None
    for argv in (base, base + ['--synthetic-seed', '0', '--model', 'x.pth'], base + ['--model', str(tmp_path / 'missing.pth')],
                 base + ['--synthetic-seed', '0', '--num-objects', '0'],
                 ['--images', str(tmp_path), '--clicks', str(tmp_path / 'none.json'), '--out', 'o', '--synthetic-seed', '0']):
        with pytest.raises(SystemExit):
            C.parse_args(argv)


def test_brs_modes_are_refused():
    from xmem2_amd.click import FBRSController
    for mode in ('f-BRS-A', 'f-BRS-B', 'f-BRS-C', 'RGB-BRS', 'DistMap-BRS'):
        with pytest.raises(NotImplementedError, match='first click is identical'):
            FBRSController(None, brs_mode=mode)
    with pytest.raises(ValueError):
        FBRSController(None, brs_mode='nonsense')
