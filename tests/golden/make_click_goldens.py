"""Record tests/golden/click.npz: the reference's click network (f-BRS model, NoBRS predictor) on conditioned synthetic weights.

    python tests/golden/make_click_goldens.py --reference PATH [--check]

Imports the reference's fbrs package (inference/interact/fbrs/: load_is_model, InteractiveController, the Cython get_dist_maps the
controller's cpu_dist_maps=True uses), loads xmem2_amd.synth.synthetic_click_state_dict(0) and runs each case in fp32 and with the
model and image cast to float64 (CPU).  The generator needs Cython: if the reference's get_dist_maps does not import, it stops.
Frames are regenerated from their seeds by `case_image` (this module is imported by the tests for that and for the case tables;
nothing here touches the reference at import time).

click.npz holds only what every host computes alike (see make_s2m_goldens.py): float64 results on a 20-bit significand (`grid20`),
or uint16 steps of 1/65535 for the full-size probability maps of the controller sequences; case n4 keeps every 16th row.  The fp32
reference's own distance from float64 goes to click_fp32_reference.json, which the GPU tests print next to their own distance
and which --check does not compare.  --check regenerates and compares with the committed click.npz array for array.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'click.npz')
OUT_FP32 = os.path.join(HERE, 'click_fp32_reference.json')

RADIUS = 260.0
N4_ROW_STRIDE = 16
ASPP_CHANNEL_STRIDE = 2         # n1 stores every 2nd channel of the ASPP output
HEAD_CHANNEL_STRIDE = 8         # and every 8th of head_input (channels of the upsampled ASPP half and of the skip half)

# ---- distance-map cases: (name, H, W, positive clicks, negative clicks), clicks (row, col) ------------------------------
DIST_CASES = (
    ('d_round', 16, 16, [(0.5, 1.5), (2.5, 10.49)], [(10.51, 3.0)]),                  # half to even: 0, 2, 2, 10 | 11
    ('d_neg_only', 97, 131, [], [(5.0, 7.0), (90.0, 120.0), (40.2, 64.8)]),
    ('d_one', 97, 131, [(48.0, 65.0)], []),
    ('d_nine', 97, 131, [(3 + 10 * i, (51 * i + 5) % 131) for i in range(9)], [((29 * i + 11) % 97, 125 - 14 * i) for i in range(9)]),
    ('d_corners', 33, 47, [(0.0, 0.0)], [(32.0, 46.0)]),
    ('d_negative_row', 33, 47, [(-3.0, 5.0), (20.0, 30.0)], [(-0.6, 4.0)]),         # a negative rounded row is ignored
)

# The reference's BFS is a flood fill that only advances through pixels it improves, so in a crowded layout a pixel can keep a
# non-minimal distance: with the positive columns (17 i^2 + 5) % 131 in d_nine, pixel (75, 14) of the positive map holds 0.015163
# where the closed form gives 0.014985.  The kernel computes the closed form; the recorded layouts are ones on which both agree.

# ---- network cases ------------------------------------------------------------------------------------------------------
# steps: ('click', x, y, positive) | ('plant',) the synthetic ellipse as the zoom-in's previous probabilities | ('undo',)
NET_CASES = {
    'n1': dict(H=97, W=131, seed=21, max_size=800, zoom={}, steps=[('click', 60, 45, True)]),
    'n2': dict(H=120, W=176, seed=22, max_size=800, zoom=dict(target_size=192, min_crop_size=48),
               steps=[('click', 88, 60, True), ('plant',), ('click', 100, 40, False), ('click', 20, 10, True), ('undo',),
                      ('click', 80, 70, True)]),
    'n3': dict(H=150, W=260, seed=23, max_size=200, zoom=dict(target_size=192, min_crop_size=48),
               steps=[('click', 130, 75, True), ('click', 150, 60, False)]),
    'n4': dict(H=480, W=854, seed=24, max_size=800, zoom={},
               steps=[('click', 427, 240, True), ('click', 600, 200, False), ('click', 380, 300, True)]),
}
ZOOM_DEFAULTS = dict(skip_clicks=1, target_size=480, expansion_ratio=1.4)       # fbrs_controller.py:11-15


def case_image(name):
    """image [3,H,W] float32 (normalised scale) of a network case."""
    sys.path.insert(0, ROOT)
    from xmem2_amd.synth import synthetic_frames
    c = NET_CASES[name]
    return synthetic_frames(1, c['H'], c['W'], seed=c['seed'])[0]


def planted_probs(name):
    """The probabilities the 'plant' step writes: the synthetic ellipse, [H,W] float32 of 0 / 1."""
    sys.path.insert(0, ROOT)
    from xmem2_amd.synth import synthetic_masks
    c = NET_CASES[name]
    return synthetic_masks(1, 1, c['H'], c['W'])[0, 0].astype(np.float32)


def grid20(a):
    """float64 -> float32 rounded to a 20-bit significand (relative step 2^-20 ~ 1e-6): host-independent storage of float64 results."""
    m, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.round(m * 2.0 ** 20) / 2.0 ** 20, e).astype(np.float32)


def u16(p):
    return np.round(np.asarray(p, np.float64) * 65535.0).astype(np.uint16)


def dist_closed_form(H, W, pos, neg, radius=RADIUS):
    """[2,H,W] float32: min over the valid clicks of ((r - rint(r_i)) / R)^2 + ((c - rint(c_i)) / R)^2, 1e6 without one (float32
    arithmetic in the order of _get_dist_maps.pyx; np.rint rounds half to even).  Every click must lie inside the map unless its
    rounded row is negative."""
    out = np.full((2, H, W), 1e6, np.float32)
    rr, cc = np.mgrid[0:H, 0:W].astype(np.float32)
    R = np.float32(radius)
    for layer, clicks in enumerate((pos, neg)):
        for r, c in clicks:
            r, c = np.rint(np.float32(r)), np.rint(np.float32(c))
            if r < 0:
                continue
            assert 0 <= r < H and 0 <= c < W, 'the goldens hold no click outside the map'
            d = ((rr - r) / R) ** 2 + ((cc - c) / R) ** 2
            out[layer] = np.minimum(out[layer], d.astype(np.float32))
    return out


def points_of(pos, neg):
    """get_points_nd's layout of one clicks list: n positive then n negative entries, (-1, -1) padding; float32 [2n,2]."""
    n = max(1, len(pos), len(neg))
    return np.array(list(pos) + [(-1, -1)] * (n - len(pos)) + list(neg) + [(-1, -1)] * (n - len(neg)), np.float32)


def _reference(path):
    sys.path.insert(0, path)
    from inference.interact.fbrs.utils.cython import get_dist_maps            # pyximport: stops here without Cython
    from inference.interact.fbrs.inference.utils import load_is_model
    from inference.interact.fbrs.controller import InteractiveController
    return get_dist_maps, load_is_model, InteractiveController


def _params(c):
    zoom = dict(ZOOM_DEFAULTS)
    zoom.update(c['zoom'])
    return {'brs_mode': 'NoBRS', 'prob_thresh': 0.5, 'zoom_in_params': zoom,
            'predictor_params': {'net_clicks_limit': None, 'max_size': c['max_size']}}


def _no_click_prob(torch, model, image_nd):
    """the flip-averaged probability of the network on image_nd [1,3,h,w] without any click"""
    x = torch.cat([image_nd, torch.flip(image_nd, dims=[3])], 0)
    pts = torch.full((2, 2, 2), -1.0)
    lg = model(x, pts)['instances']
    return torch.sigmoid(0.5 * (lg[:1] + torch.flip(lg[1:], dims=[3])))[0, 0].double().numpy()


def _run_case(torch, Controller, model, name, dtype, hooks=None):
    """Drive InteractiveController through the case's steps; returns one record per click: dict(roi, limit_roi, size, clicks, prob)."""
    c = NET_CASES[name]
    ctl = Controller(model, 'cpu', _params(c))
    ctl.set_image(torch.from_numpy(case_image(name)).to(dtype))
    seen = []

    def wrap(pred):
        inner = pred._get_prediction

        def logged(image_nd, clicks_lists, is_image_changed):
            lg = inner(image_nd, clicks_lists, is_image_changed)
            work = torch.sigmoid(0.5 * (lg[:1] + torch.flip(lg[1:], dims=[3])))[0, 0].double().numpy()
            seen.append((tuple(image_nd.shape[2:]), [tuple(float(v) for v in k.coords) for k in clicks_lists[0]], image_nd, work))
            return lg
        pred._get_prediction = logged
    wrap(ctl.predictor)
    out, first = [], True
    for step in c['steps']:
        if step[0] == 'plant':
            states = ctl.predictor.get_states()['transform_states']
            z = list(states[0])
            z[2] = planted_probs(name)[None, None].astype(np.float64 if dtype == torch.float64 else np.float32)
            states[0] = tuple(z)
            ctl.predictor.set_states({'transform_states': states})
            continue
        if step[0] == 'undo':
            ctl.undo_click()
            out.append(dict(undo=True, prob=ctl.probs_history[-1][1][0, 0].double().numpy()))
            continue
        _, x, y, positive = step
        if first and hooks:
            hooks(True)
        ctl.add_click(x, y, positive)
        if first and hooks:
            hooks(False)
        size, clicks, image_nd, work = seen[-1]
        zoom, limit = ctl.predictor.transforms[0], ctl.predictor.transforms[1]
        rec = dict(roi=zoom._object_roi, limit_roi=limit._object_roi, size=size, clicks=clicks,
                   prob=ctl.probs_history[-1][1][0, 0].double().numpy())
        if first:
            rec['moved'] = float(np.abs(_no_click_prob(torch, model, image_nd[:1]) - work).max())
        out.append(rec)
        first = False
    return out


def _roi_arr(roi):
    return np.array([-1, -1, -1, -1] if roi is None else [int(v) for v in roi], np.int32)


def generate(reference):
    import torch
    torch.set_grad_enabled(False)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    get_dist_maps, load_is_model, Controller = _reference(reference)
    from xmem2_amd.click import state_dict_spec
    from xmem2_amd.synth import synthetic_click_state_dict
    sd = synthetic_click_state_dict(0)
    net32 = load_is_model(dict(sd), 'cpu', cpu_dist_maps=True, norm_radius=RADIUS)
    net64 = load_is_model(dict(sd), 'cpu', cpu_dist_maps=True, norm_radius=RADIUS).double()
    ref_sd = net32.state_dict()
    names = list(ref_sd)
    spec = state_dict_spec()
    assert names == list(spec) and all(tuple(ref_sd[k].shape) == tuple(spec[k]) for k in names), 'click_state_dict_spec drifted'
    assert all(torch.equal(ref_sd[k], sd[k]) for k in names), 'the reference did not take every synthetic tensor'
    rec = {'spec_names': np.array(names), 'spec_shapes': np.array([str(tuple(ref_sd[k].shape)) for k in names])}
    fp32 = {}

    # distance maps: the reference's Cython BFS equals the closed form, bit for bit
    for name, H, W, pos, neg in DIST_CASES:
        bfs = get_dist_maps(points_of(pos, neg), H, W, RADIUS)
        closed = dist_closed_form(H, W, pos, neg)
        assert bfs.dtype == np.float32 and np.array_equal(bfs, closed), f'{name}: the BFS result differs from the closed form'
        feat = np.tanh(2.0 * np.sqrt(bfs.astype(np.float64)))
        if not pos:
            assert np.all(feat[0] == 1.0)
        rec[f'{name}_features64'] = grid20(feat)

    for name, c in NET_CASES.items():
        grabs = {}
        handles = []

        def hooks(on, grabs=grabs, handles=handles):
            if not on:
                for h in handles:
                    h.remove()
                return
            fe = net64.feature_extractor
            keep = lambda key: (lambda _m, _i, o: grabs.__setitem__(key, o.double().numpy()))
            handles.append(net64.rgb_conv.register_forward_hook(keep('rgb')))
            handles.append(fe.skip_project.register_forward_hook(keep('skip')))
            handles.append(fe.aspp.register_forward_hook(keep('aspp')))
            handles.append(fe.head.register_forward_pre_hook(lambda _m, i: grabs.__setitem__('head_input', i[0].double().numpy())))
            handles.append(net64.head.register_forward_hook(keep('logits')))
        r64 = _run_case(torch, Controller, net64, name, torch.float64, hooks if name == 'n1' else None)
        r32 = _run_case(torch, Controller, net32, name, torch.float32)
        errs = []
        for i, (a, b) in enumerate(zip(r64, r32)):
            p64, p32 = a['prob'], b['prob']
            err = float(np.abs(p32 - p64).max())
            errs.append(err)
            mid = float(((p64 >= 0.05) & (p64 <= 0.95)).mean())
            undecided = float((np.abs(p64 - 0.5) <= 5e-3).mean())
            print(f'{name} step {i}: roi {a.get("roi")} size {a.get("size")} mid {mid:.3f} undecided {undecided:.4f} '
                  f'mask {float((p64 > 0.5).mean()):.3f} fp32 vs float64 {err:.2e}')
            if a.get('undo'):
                continue
            assert a['roi'] == b['roi'] and a['limit_roi'] == b['limit_roi'] and a['size'] == b['size'] and a['clicks'] == b['clicks'], \
                f'{name} step {i}: the fp32 and float64 runs took different geometries'
            assert mid >= 0.20, f'{name} step {i}: degenerate output (only {mid:.3f} of the pixels in [0.05, 0.95])'
            assert undecided <= 0.02, f'{name} step {i}: {undecided:.3f} of the pixels undecided'
            assert err <= 2e-4, f'{name} step {i}: the fp32 reference is {err:.2e} from float64'
            h, w = a['size']
            assert all(0 <= r <= h - 1 and 0 <= x <= w - 1 for r, x in a['clicks']), f'{name} step {i}: a transformed click left its map'
        moved = r64[0]['moved']
        print(f'{name}: removing the click moves p by {moved:.3f}')
        assert moved > 0.05, f'{name}: the clicks barely matter (max |dp| {moved:.4f})'
        fp32[name] = {'max_abs': max(errs), 'per_step': errs}
        clicks = [s for s in r64 if not s.get('undo')]
        rec[f'{name}_rois'] = np.stack([_roi_arr(s['roi']) for s in clicks])
        rec[f'{name}_limit_rois'] = np.stack([_roi_arr(s['limit_roi']) for s in clicks])
        rec[f'{name}_sizes'] = np.array([s['size'] for s in clicks], np.int32)
        for i, s in enumerate(clicks):
            rec[f'{name}_clicks{i}'] = np.array(s['clicks'], np.float64).reshape(-1, 2)
        probs = np.stack([s['prob'] for s in r64])          # undo steps included, in step order
        if name == 'n1':
            rec['n1_prob64'] = grid20(probs)
            rec['n1_rgb64'] = grid20(grabs['rgb'])
            rec['n1_skip64'] = grid20(grabs['skip'])
            rec['n1_aspp64'] = grid20(grabs['aspp'][:, ::ASPP_CHANNEL_STRIDE])
            rec['n1_head_input64'] = grid20(grabs['head_input'][:, ::HEAD_CHANNEL_STRIDE])
            rec['n1_logits64'] = grid20(grabs['logits'])
        elif name == 'n4':
            rec['n4_prob64_rows_u16'] = u16(probs[:, ::N4_ROW_STRIDE])
        else:
            rec[f'{name}_prob64_u16'] = u16(probs)
        if name == 'n2':
            planted = _roi_arr(clicks[1]['roi'])
            H, W = c['H'], c['W']
            assert planted[0] > 0 and planted[1] < H - 1 and planted[2] > 0 and planted[3] < W - 1, f'n2: the planted ROI {planted} is not a proper sub-rectangle'
            assert clicks[2]['roi'] != clicks[1]['roi'], 'n2: click 3 did not move the ROI'
            assert clicks[3]['roi'] == clicks[1]['roi'], "n2: click 3' after the undo should run in the planted ROI"
        if name == 'n3':
            assert clicks[0]['limit_roi'] is not None and clicks[1]['roi'] is not None, 'n3: LimitLongestSide or the zoom-in stayed idle'
            assert clicks[1]['size'] != clicks[0]['size'], 'n3: the zoomed click did not change the working size'
    return rec, fp32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('XMEM_REFERENCE'), required='XMEM_REFERENCE' not in os.environ,
                    help='checkout of the reference project (default: $XMEM_REFERENCE)')
    ap.add_argument('--check', action='store_true', help='compare with the committed file instead of writing it')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec, fp32 = generate(args.reference)
    if args.check:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(rec), (sorted(old.files), sorted(rec))
        for k in rec:
            assert old[k].dtype == rec[k].dtype and np.array_equal(old[k], rec[k]), f'{k} differs'
        print('click.npz reproduced array for array')
        return
    np.savez_compressed(OUT, **rec)
    with open(OUT_FP32, 'w') as f:
        json.dump(fp32, f, indent=1, sort_keys=True)
        f.write('\n')
    size = os.path.getsize(OUT)
    assert size < 1 << 20, f'click.npz is {size} bytes: over the size limit of a committed file'
    print('wrote', OUT, size, 'bytes, and', OUT_FP32)


if __name__ == '__main__':
    main()
