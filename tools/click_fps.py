"""Click-to-mask cost at 854x480 (profiles/r07_click.txt).

    python tools/click_fps.py [--out FILE]             # latency of interact(): first click, zoomed click, first call; depthwise bandwidth
    python tools/click_fps.py --kernel-only            # one capture + 40 zoomed clicks: run it under rocprofv3 --kernel-trace --stats
    python tools/click_fps.py --kernel-stats CSV [--out FILE]    # share per kernel family of that run (appended to FILE)

Latency: `FBRSController.interact` on a synthetic 480p frame with conditioned synthetic weights and the controller's defaults
(with_flip: a batch of 2).  The frame is wider than max_size = 800, so the first click runs at 450x800; the zoom-in's previous
probabilities are planted with the synthetic ellipse, so the zoomed clicks run on its ROI at longest side 480.  First call: wall clock
around a synchronize (eager warm-up + graph capture + replay).  Warm calls: wall clock per call over 40 calls, each ended by a
synchronize - a click is a user action, so the host work of the transforms (the 20-byte ROI read-back among it) belongs to it -
reached by undo + the same click again.  Depthwise: `ops.depthwise3x3` alone at 2x120x120x160, 50 launches between device events,
bytes = one read and one write of the tensor.
"""
import argparse
import csv
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 854
HBM_TBPS = 8.0            # MI355X HBM3E peak (a float4 copy reaches about 6.3 TB/s of it)


def _setup():
    from xmem2_amd.click import ClickNet, FBRSController
    from xmem2_amd.synth import synthetic_click_state_dict, synthetic_frames
    torch.set_grad_enabled(False)
    net = ClickNet(device='cuda:0').load_weights(synthetic_click_state_dict(0))
    image = torch.from_numpy(synthetic_frames(1, H, W, seed=5)[0])[None].cuda()
    return net, FBRSController(net), image


def _plant(ctl):
    from xmem2_amd.synth import synthetic_masks
    ctl.predictor.transforms[0]._prev_probs = torch.from_numpy(synthetic_masks(1, 1, H, W)[0, 0]).cuda()


def _warm(ctl, image, x, y, positive, n=40):
    """ms per interact() of the same click repeated after an undo (the undo is outside the clock)"""
    total = 0.0
    for i in range(n + 5):
        ctl.undo()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctl.interact(image, x, y, positive)
        torch.cuda.synchronize()
        if i >= 5:
            total += time.perf_counter() - t0
    return total / n * 1e3


def latency(lines):
    from xmem2_amd import ops
    net, ctl, image = _setup()
    lines.append(f'click-to-mask interact() at {W}x{H}, fp32, with_flip (batch 2), conditioned synthetic weights; {torch.cuda.get_device_name(0)}')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ctl.interact(image, W // 2, H // 2, True)
    torch.cuda.synchronize()
    first_call = (time.perf_counter() - t0) * 1e3
    size1 = ctl.predictor.last_geometry[0]
    first = _warm(ctl, image, W // 2, H // 2, True)
    _plant(ctl)
    t0 = time.perf_counter()
    ctl.interact(image, W // 2 + 40, H // 2 - 30, True)
    torch.cuda.synchronize()
    zoom_capture = (time.perf_counter() - t0) * 1e3
    size2, roi = ctl.predictor.last_geometry[0], ctl.predictor.transforms[0]._object_roi
    zoomed = _warm(ctl, image, W // 2 + 40, H // 2 - 30, True)
    lines.append(f'  first call (eager warm-up + capture + replay), working size {size1[1]}x{size1[0]}: {first_call:8.1f} ms')
    lines.append(f'  first click, warm (LimitLongestSide: {size1[1]}x{size1[0]}):                    {first:8.3f} ms')
    lines.append(f'  first zoomed click (capture of the ROI geometry {size2[1]}x{size2[0]}, ROI {roi}): {zoom_capture:8.1f} ms')
    lines.append(f'  zoomed click, warm ({size2[1]}x{size2[0]}):                                      {zoomed:8.3f} ms')
    lines.append(f'  graphs captured: {net.captures}')
    # depthwise 3x3 alone
    B, h, w, C = 2, 120, 120, 160
    x = torch.randn(B, h, w, C, device='cuda')
    wk = torch.randn(9, C, device='cuda')
    out = torch.empty_like(x)
    for _ in range(5):
        ops.depthwise3x3(x, wk, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        ops.depthwise3x3(x, wk, out=out)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1) / reps
    nbytes = 2.0 * x.numel() * 4
    lines.append(f'  depthwise3x3 at {B}x{h}x{w}x{C}: {ms * 1e3:.1f} us per launch (launch overhead included), {nbytes / 1e6:.1f} MB read + written: '
                 f'{nbytes / ms / 1e9:.2f} TB/s of {HBM_TBPS} TB/s HBM peak, ~6.3 TB/s for a plain copy (the 18 MB tensor fits the last-level cache)')
    return lines


def kernel_only():
    net, ctl, image = _setup()
    ctl.interact(image, W // 2, H // 2, True)
    _plant(ctl)
    ctl.interact(image, W // 2 + 40, H // 2 - 30, True)
    for _ in range(40):
        ctl.undo()
        ctl.interact(image, W // 2 + 40, H // 2 - 30, True)
    torch.cuda.synchronize()
    print(f'kernel-only: 1 full-frame click + 41 zoomed clicks ({net.captures} captures)')


def family(name):
    n = name.replace('void ', '')
    if n.startswith('conv_mfma_kernel') and n.rstrip().endswith('true>(ConvArgs)'):
        return 'convolutions, dilated (direct, DIL)'
    if n.startswith('conv_') or n.startswith('wino') or 'gemm_stream' in n:
        return 'convolutions, other (direct, pointwise, Winograd)'
    if 'depthwise3x3' in n:
        return 'depthwise 3x3'
    if n.startswith('__amd_rocclr'):
        return 'runtime copies / fills'
    return 'elementwise (input, pool, mean, resize, output, bbox)'


def kernel_stats(path, lines):
    rows = list(csv.DictReader(open(path)))
    fam, total = {}, 0.0
    for r in rows:
        d = fam.setdefault(family(r['Name']), [0, 0.0])
        d[0] += int(r['Calls'])
        d[1] += float(r['TotalDurationNs'])
        total += float(r['TotalDurationNs'])
    lines.append('')
    lines.append('rocprofv3 --kernel-trace --stats of `click_fps.py --kernel-only` (2 eager warm-ups, 1 full-frame and 41 zoomed replays; '
                 'share of the kernel time of the whole run):')
    for f, (c, ns) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        lines.append(f'  {f:52s} launches {c:6d}   {ns / 1e6:9.2f} ms   {ns / total:6.1%}')
    lines.append('  top kernels:')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:10]:
        short = r['Name'].replace('void ', '').split('(')[0]
        lines.append(f'    {short[:90]:90s} {int(r["Calls"]):6d} x {float(r["AverageNs"]) / 1e3:8.1f} us')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    if args.kernel_only:
        kernel_only()
        return
    lines = kernel_stats(args.kernel_stats, []) if args.kernel_stats else latency([])
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a' if args.kernel_stats else 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
