"""Cost of the robot user of click evaluation at 854x480 (profiles/r07_click_eval.txt).

    python tools/click_eval_bench.py [--out FILE]                  # robot step on the device and on the host; a 20-click evaluate_sample
    python tools/click_eval_bench.py --kernel-only                 # 50 robot steps: run it under rocprofv3 --kernel-trace --stats
    python tools/click_eval_bench.py --kernel-stats CSV [--out FILE]    # per-kernel times of that run (appended to FILE)

Robot step: `Clicker.make_next_click(prob, 0.49)` - five launches, one fill, the copy of the 32-byte record and its synchronise -
wall clock per call, median of 50 after 10 warm-up calls.  Ground truth: the synthetic ellipse plus a disc; prediction: a smooth
probability map of a shifted ellipse, so both error planes are large regions (the distances are tens of pixels, which is what the row
pass's outward search pays for).  Host formulation on the same machine: the probability map copied to the host, thresholded, and the
reference's wording of the choice (two float64 scipy distance transforms of the padded planes).  evaluate_sample: NoBRSPredictor with
the controller's defaults, max_iou_thr out of reach, 20 clicks, second run (graphs captured), with the time inside make_next_click
summed.
"""
import argparse
import csv
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 854
THR = 0.49
KERNELS = ('click_errors_kernel', 'edt_cols_kernel', 'edt_rows_kernel', 'next_click_partial_kernel', 'next_click_final_kernel')


def _case():
    from xmem2_amd.synth import synthetic_masks
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = (synthetic_masks(1, 1, H, W)[0, 0] > 0.5) | ((yy - 90) ** 2 + (xx - 150) ** 2 <= 60 ** 2)
    r = np.sqrt(((yy - 270) / 120.0) ** 2 + ((xx - 500) / 170.0) ** 2)
    prob = (1.0 / (1.0 + np.exp(8.0 * (r - 1.0)))).astype(np.float32)
    return gt.astype(np.int32), prob


def _host_step(gt, prob_dev, not_clicked):
    from scipy.ndimage import distance_transform_edt
    pred = prob_dev.cpu().numpy() > np.float32(THR)
    obj = gt == 1
    d = [distance_transform_edt(np.pad(p, 1))[1:-1, 1:-1] * not_clicked for p in (obj & ~pred, ~obj & pred)]
    positive = d[0].max() > d[1].max()
    ys, xs = np.where(d[0] == d[0].max()) if positive else np.where(d[1] == d[1].max())
    not_clicked[ys[0], xs[0]] = False
    return bool(positive), (int(ys[0]), int(xs[0]))


def _median_ms(fn, n=50, warm=10):
    times = []
    for i in range(n + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def measure(lines):
    from xmem2_amd import click_eval as E
    from xmem2_amd.click import ClickNet, FBRSController
    from xmem2_amd.synth import synthetic_click_state_dict, synthetic_frames
    torch.set_grad_enabled(False)
    gt, prob = _case()
    prob_dev = torch.from_numpy(prob).cuda()
    lines.append(f'robot step of click evaluation at {W}x{H}; {torch.cuda.get_device_name(0)}')
    clicker = E.Clicker(gt_mask=gt)
    dev = _median_ms(lambda: clicker.make_next_click(prob_dev, THR))
    not_clicked = np.ones((H, W), bool)
    host_clicks = []
    host = _median_ms(lambda: host_clicks.append(_host_step(gt, prob_dev, not_clicked)), n=10, warm=2)
    same = [(c.is_positive, c.coords) for c in clicker.get_clicks()[:len(host_clicks)]] == host_clicks
    lines.append(f'  device: launches + 32-byte record copy + synchronise, median of 50: {dev[0]:8.3f} ms (min {dev[1]:.3f}, max {dev[2]:.3f})')
    lines.append(f'  host:   map copy + threshold + scipy formulation, median of 10:      {host[0]:8.3f} ms (min {host[1]:.3f}, max {host[2]:.3f})')
    lines.append(f'  the first {len(host_clicks)} clicks of both are {"equal" if same else "DIFFERENT"}; '
                 f'first click {clicker.get_clicks()[0]}, record {clicker.last_record}')
    # a 20-click NoBRS run
    net = ClickNet(device='cuda:0').load_weights(synthetic_click_state_dict(0))
    ctl = FBRSController(net)
    ctl._reset_predictor()
    image = torch.from_numpy(synthetic_frames(1, H, W, seed=5)[0]).cuda()
    robot = [0.0]
    inner = E.Clicker.make_next_click

    def timed(self, pred, pred_thr=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inner(self, pred, pred_thr)
        robot[0] += time.perf_counter() - t0
    E.Clicker.make_next_click = timed
    try:
        for run in range(2):
            robot[0] = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            clicks, ious, _ = E.evaluate_sample(image, gt, ctl.predictor, 2.0, max_clicks=20)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
    finally:
        E.Clicker.make_next_click = inner
    lines.append(f'  evaluate_sample, NoBRS, {len(clicks)} clicks (second run, {net.captures} graphs captured before it): {wall * 1e3:8.1f} ms wall, '
                 f'{robot[0] * 1e3:.2f} ms of it in {len(clicks)} robot steps ({robot[0] / wall:.1%}); last IoU {float(ious[-1]):.4f}')
    return lines


def kernel_only():
    from xmem2_amd import click_eval as E
    gt, prob = _case()
    prob_dev = torch.from_numpy(prob).cuda()
    clicker = E.Clicker(gt_mask=gt)
    for _ in range(50):
        clicker.make_next_click(prob_dev, THR)
    torch.cuda.synchronize()
    print('kernel-only: 50 robot steps')


def kernel_stats(path, lines):
    rows = [r for r in csv.DictReader(open(path)) if any(k in r['Name'] for k in KERNELS)]
    lines.append('')
    lines.append('rocprofv3 --kernel-trace --stats of `click_eval_bench.py --kernel-only` (50 robot steps):')
    total = 0.0
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs'])):
        name = next(k for k in KERNELS if k in r['Name'])
        total += float(r['AverageNs'])
        lines.append(f'  {name:28s} {int(r["Calls"]):5d} x {float(r["AverageNs"]) / 1e3:8.2f} us (min {float(r["MinNs"]) / 1e3:.2f}, max {float(r["MaxNs"]) / 1e3:.2f})')
    lines.append(f'  sum of the averages: {total / 1e3:.2f} us of kernel time per robot step')
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
    lines = kernel_stats(args.kernel_stats, []) if args.kernel_stats else measure([])
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a' if args.kernel_stats else 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
