"""Record tests/golden/s2m.npz: the reference's scribble-to-mask network on conditioned synthetic weights.

    python tests/golden/make_s2m_goldens.py [--reference PATH] [--check]

Imports the reference's `s2m_network` and `S2MController` arithmetic (inference/interact/s2m/, s2m_controller.py,
util/tensor_util.py), loads xmem2_amd.synth.synthetic_s2m_state_dict(0) and runs each case in fp32 and with the model and inputs
cast to float64 (CPU).  Frames, previous masks and scribbles are regenerated from their seeds by `case_inputs` (this module is
imported by the tests for that; nothing here touches the reference at import time).

s2m.npz holds only what every host computes alike: the binary channels of the packed input (uint8) and the float64 outputs on a
coarse grid - a 20-bit significand (`grid20`, stored as float32), or uint16 steps of 1/65535 for the 200x300 case to keep the
file small.  Float64 convolutions differ between CPU kernels (AVX2 / AVX-512 BLAS paths) by ~1e-15 relative; a value rounded
straight to float32 can land on either side of a rounding boundary, one 2^20 times coarser almost never does (~1e-9 per value).
The fp32 reference's own distance from float64 does depend on the host's fp32 kernels: it goes to s2m_fp32_reference.json, which
the GPU tests print next to their own distance and which --check does not compare.
--check regenerates and compares with the committed s2m.npz array for array.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 's2m.npz')
OUT_FP32 = os.path.join(HERE, 's2m_fp32_reference.json')

# (name, H, W, K, seed): case 1 with layer intermediates, case 2 padded (not a multiple of 16) with three objects, case 3 480p
CASES = (('c1', 64, 96, 1, 11), ('c2', 200, 300, 3, 12), ('c3', 480, 854, 1, 13))
IGNORE = 255
C3_ROW_STRIDE = 16          # case 3 stores every 16th row of the full-resolution probabilities
LOW_CHANNELS = 64           # case 1 stores the first 64 of layer1's 256 channels


def case_inputs(H, W, K, seed):
    """(image [3,H,W] float32 normalised, prev_mask [H,W] float32 index, scr [H,W] uint8) of one case.
    prev_mask: ellipse = 1, rectangles = 2..K (synthetic_masks).  Scribbles (255 = no stroke): per object k a horizontal
    stroke inside it, a background (0) stroke along the bottom; K >= 3: object 3 has NO positive stroke, the ignore value
    also appears inside a stroke row, and a label K + 1 (> K: a negative stroke for every object) is drawn."""
    sys.path.insert(0, ROOT)
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    image = synthetic_frames(1, H, W, seed=seed)[0]
    m = synthetic_masks(1, K, H, W)[0]
    prev = np.zeros((H, W), np.float32)
    for k in range(K):
        prev[m[k] > 0.5] = k + 1
    scr = np.full((H, W), IGNORE, np.uint8)
    y, x0, x1 = H // 2, W // 3, W // 2
    scr[y - 1:y + 2, x0:x1] = 1                                  # object 1: the ellipse's centre row
    scr[H - 5:H - 2, 2:W // 3] = 0                               # background stroke
    if K >= 2:
        ys, xs = np.nonzero(m[1] > 0.5)
        if len(ys):
            scr[ys.min() + 1, xs.min():xs.max()] = 2
    if K >= 3:
        scr[H // 4, W - W // 4:W - 2] = K + 1                    # label > K
        scr[y - 1:y + 2, (x0 + x1) // 2:(x0 + x1) // 2 + 4] = IGNORE
    return image, prev, scr


def grid20(a):
    """float64 -> float32 rounded to a 20-bit significand (relative step 2^-20 ~ 1e-6): host-independent storage of float64 results."""
    m, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.round(m * 2.0 ** 20) / 2.0 ** 20, e).astype(np.float32)


def pack_channels(prev, scr, K, ignore=IGNORE):
    """The reference's three per-object binary channels (prev == k, scr == k, scr != k and scr != ignore), unpadded: [K][3][H][W]."""
    out = np.zeros((K, 3) + prev.shape, np.uint8)
    for k in range(1, K + 1):
        out[k - 1, 0] = prev == k
        out[k - 1, 1] = scr == k
        out[k - 1, 2] = (scr != k) & (scr != ignore)
    return out


def _reference(path):
    sys.path.insert(0, path)
    from inference.interact.s2m.s2m_network import deeplabv3plus_resnet50
    from util.tensor_util import pad_divide_by, unpad
    return deeplabv3plus_resnet50, pad_divide_by, unpad


def _run(net, torch, pad_divide_by, unpad, image, prev, scr, K, dtype, zero_scribbles=False, hooks=None):
    """s2m_controller.py:21-38 with the model and its input in `dtype`; returns prob [K,H,W] (float64 numpy)."""
    img = torch.from_numpy(image)[None].to(dtype)
    pm = torch.from_numpy(prev)[None]
    out = []
    for ki in range(1, K + 1):
        p_srb = (scr == ki).astype(np.uint8)
        n_srb = ((scr != ki) * (scr != IGNORE)).astype(np.uint8)
        Rs = torch.from_numpy(np.stack([p_srb, n_srb], 0)).unsqueeze(0).to(dtype)
        if zero_scribbles:
            Rs = Rs * 0
        inputs = torch.cat([img, (pm == ki).to(dtype).unsqueeze(0), Rs], 1)
        inputs, pads = pad_divide_by(inputs, 16)
        out.append(unpad(torch.sigmoid(net(inputs)), pads)[0, 0].double().numpy())
    return np.stack(out)


def generate(reference):
    import torch
    torch.set_grad_enabled(False)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    S2M, pad_divide_by, unpad = _reference(reference)
    from xmem2_amd.synth import synthetic_s2m_state_dict
    from xmem2_amd.s2m import state_dict_spec
    sd = synthetic_s2m_state_dict(0)
    net32 = S2M().eval()
    net32.load_state_dict(sd)
    net64 = S2M().eval().double()
    net64.load_state_dict(sd)
    ref_sd = net32.state_dict()
    names = list(ref_sd)
    spec = state_dict_spec()
    assert names == list(spec) and all(tuple(ref_sd[k].shape) == tuple(spec[k]) for k in names), 'state_dict_spec drifted'
    fp32 = {}
    rec = {'spec_names': np.array(names), 'spec_shapes': np.array([str(tuple(ref_sd[k].shape)) for k in names])}

    for name, H, W, K, seed in CASES:
        image, prev, scr = case_inputs(H, W, K, seed)
        rec[f'{name}_channels'] = pack_channels(prev, scr, K)
        grabs = {}
        hooks = []
        if name in ('c1', 'c3'):
            def grab(key):
                def f(_m, _i, o):
                    grabs.setdefault(key, []).append(o.double().numpy())
                return f
            for net in (net64,):
                hooks.append(net.backbone.layer1.register_forward_hook(grab('low_level')))
                hooks.append(net.classifier.aspp.register_forward_hook(grab('aspp')))
                hooks.append(net.classifier.register_forward_hook(grab('logits')))
        p64 = _run(net64, torch, pad_divide_by, unpad, image, prev, scr, K, torch.float64)
        for h in hooks:
            h.remove()
        p32 = _run(net32, torch, pad_divide_by, unpad, image, prev, scr, K, torch.float32)
        pz = _run(net32, torch, pad_divide_by, unpad, image, prev, scr, K, torch.float32, zero_scribbles=True)
        mid = float(((p32 >= 0.05) & (p32 <= 0.95)).mean())
        dscr = float(np.abs(p32 - pz).max())
        err32 = float(np.abs(p32 - p64).max())
        print(f'{name}: {H}x{W} K={K}: p in [0.05, 0.95] {mid:.3f}, scribbles move p by {dscr:.3f}, fp32 reference vs float64 {err32:.2e}')
        assert mid >= 0.20, f'{name}: degenerate output (only {mid:.3f} of pixels in [0.05, 0.95])'
        assert dscr > 0.05, f'{name}: the scribbles barely matter (max |dp| {dscr:.4f})'
        fp32[name] = {'max_abs': err32, 'mean_abs': float(np.abs(p32 - p64).mean())}
        if name == 'c1':
            rec['c1_prob64'] = grid20(p64)
            rec['c1_low_level64'] = grid20(grabs['low_level'][0][:, :LOW_CHANNELS])
            rec['c1_aspp64'] = grid20(grabs['aspp'][0])
            rec['c1_logits64'] = grid20(grabs['logits'][0])
        elif name == 'c2':
            rec['c2_prob64_u16'] = np.round(p64 * 65535.0).astype(np.uint16)
        else:
            rec['c3_logits64'] = grid20(grabs['logits'][0])
            rec['c3_prob64_rows'] = grid20(p64[:, ::C3_ROW_STRIDE])
    return rec, fp32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('XMEM_REFERENCE', '/root/reference'))
    ap.add_argument('--check', action='store_true', help='compare with the committed file instead of writing it')
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    rec, fp32 = generate(args.reference)
    if args.check:
        old = np.load(OUT)
        assert sorted(old.files) == sorted(rec), (sorted(old.files), sorted(rec))
        for k in rec:
            assert old[k].dtype == rec[k].dtype and np.array_equal(old[k], rec[k]), f'{k} differs'
        print('s2m.npz reproduced array for array')
        return
    np.savez_compressed(OUT, **rec)
    with open(OUT_FP32, 'w') as f:
        json.dump(fp32, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', OUT, os.path.getsize(OUT), 'bytes, and', OUT_FP32)


if __name__ == '__main__':
    main()
