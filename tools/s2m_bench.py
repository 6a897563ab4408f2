"""Scribble-to-mask (S2M) cost at 854x480 for K = 1, 2, 3 objects (profiles/r07_s2m.txt).

    python tools/s2m_bench.py [--out FILE]            # latency table + dilated-layer table (device events)
    python tools/s2m_bench.py --kernel-only           # K = 1: capture + 60 replays only: run it under rocprofv3 --kernel-trace --stats
    python tools/s2m_bench.py --kernel-stats CSV [--out FILE]   # per-kernel-family times of that run (appended to FILE)

Latency: `S2MController.interact` on a synthetic 480p frame (conditioned synthetic weights): the first call (eager warm-up + graph
capture + replay, wall clock around a synchronize) and the warm call (device events over 60 calls after 5 warm-up calls).  The
dilated layers (layer4 blocks 1-2, ASPP rates 6 / 12 / 18) are timed alone at the network's shapes with tap skipping on and off
(20 back-to-back launches between events); their share is taken of the warm latency.  Conv FLOP/s: the algorithmic FLOPs of every
convolution of one forward (ops.RECORD) over the conv family's kernel time from the rocprofv3 run, against the fp32 MFMA peak.
"""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 854
PEAK_FP32_TFLOPS = 157.3          # v_mfma_f32_32x32x2_f32 dense peak (MI355X)


def _inputs(K):
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    image = torch.from_numpy(synthetic_frames(1, H, W, seed=5)[0])[None].cuda()
    m = synthetic_masks(1, K, H, W)[0]
    prev = np.zeros((H, W), np.float32)
    for k in range(K):
        prev[m[k] > 0.5] = k + 1
    scr = np.full((H, W), 255, np.uint8)
    for k in range(K):
        ys, xs = np.nonzero(m[k] > 0.5)
        scr[int(np.median(ys)), xs.min():xs.max()] = k + 1
    scr[H - 8:H - 5, 10:W // 3] = 0
    return image, torch.from_numpy(prev).cuda(), scr


def _net():
    from xmem2_amd.s2m import S2M
    from xmem2_amd.synth import synthetic_s2m_state_dict
    return S2M(device='cuda:0').load_weights(synthetic_s2m_state_dict(0))


def _conv_flops(net, K):
    """algorithmic conv FLOPs of one forward (eager, ops.RECORD), and those of the dilated layers"""
    from xmem2_amd import ops
    from xmem2_amd.s2m import pad_divide_by_16
    image, prev, scr = _inputs(K)
    Hp, Wp, lh, lw = pad_divide_by_16(H, W)
    x = ops.s2m_pack(image[0], prev, torch.from_numpy(scr).cuda(), K, 255, Hp, Wp, lh, lw)
    ops.RECORD = []
    try:
        net.features(x)
        rec = ops.RECORD
    finally:
        ops.RECORD = None
    torch.cuda.synchronize()
    total = sum(r[2] for r in rec)
    dil = sum(r[2] for r in rec if 'dilation' in r[4][5] and r[4][5]['dilation'] > 1)
    return total, dil, len(rec)


def _time_dilated(K, reps=20):
    """ms per launch of each dilated layer of the network at this K, tap skipping on / off"""
    from xmem2_amd import ops
    from xmem2_amd.ops import ConvWeights
    rows = []
    g = torch.Generator().manual_seed(0)
    for name, cin, cout, d in (('layer4.{1,2}.conv2', 512, 512, 2), ('aspp.convs.1', 2048, 256, 6), ('aspp.convs.2', 2048, 256, 12),
                               ('aspp.convs.3', 2048, 256, 18)):
        w = (torch.randn(cout, 3, 3, cin, generator=g) * 0.01).cuda()
        cw = ConvWeights(w, torch.ones(cout).cuda(), torch.zeros(cout).cuda(), 1, d, dilation=d)
        x = torch.rand(K, 30, 54, cin, generator=g).cuda()
        out = torch.empty(K, 30, 54, cout, device='cuda')
        ms = []
        for skip in (True, False):
            for _ in range(3):
                ops.conv2d_dilated(x, cw, out=out, relu_out=True, tap_skip=skip)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.conv2d_dilated(x, cw, out=out, relu_out=True, tap_skip=skip)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        rows.append((name, d, cin, cout, 2.0 * K * 30 * 54 * cout * 9 * cin, ms[0], ms[1], 2 if d == 2 else 1))
    return rows


def latency(out_lines):
    from xmem2_amd.s2m import S2MController
    torch.set_grad_enabled(False)
    out_lines.append(f'S2M interact() at {W}x{H} (padded 864x480), fp32, conditioned synthetic weights; {torch.cuda.get_device_name(0)}')
    out_lines.append('')
    out_lines.append(f'{"K":>2} {"first call ms":>14} {"warm ms":>9} {"warm ms/object":>15} {"conv GFLOP":>11} {"dilated GFLOP":>14} '
                     f'{"dilated ms (skip on)":>21} {"(skip off)":>11} {"dilated share":>14}')
    tables = []
    for K in (1, 2, 3):
        net = _net()
        image, prev, scr = _inputs(K)
        ctl = S2MController(net, K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctl.interact(image, prev, scr)
        torch.cuda.synchronize()
        first = (time.perf_counter() - t0) * 1e3
        for _ in range(5):
            ctl.interact(image, prev, scr)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 60
        e0.record()
        for _ in range(n):
            ctl.interact(image, prev, scr)
        e1.record()
        e1.synchronize()
        warm = e0.elapsed_time(e1) / n
        flops, dflops, nconv = _conv_flops(net, K)
        rows = _time_dilated(K)
        don = sum(r[5] * r[7] for r in rows)
        doff = sum(r[6] * r[7] for r in rows)
        out_lines.append(f'{K:>2} {first:14.1f} {warm:9.3f} {warm / K:15.3f} {flops / 1e9:11.1f} {dflops / 1e9:14.1f} {don:21.3f} '
                         f'{doff:11.3f} {don / warm:14.1%}')
        tables.append((K, rows, nconv))
        del ctl, net
    out_lines.append('')
    out_lines.append('dilated layers alone (ms per launch, 20 launches between events; layer4 runs its dilated 3x3 twice):')
    for K, rows, nconv in tables:
        for name, d, cin, cout, fl, on, off, cnt in rows:
            out_lines.append(f'  K={K} {name:20s} d={d:2d} {cin:4d}->{cout:3d}  skip on {on:7.3f}  off {off:7.3f}  '
                             f'saved {1 - on / off:6.1%}  {fl / on / 1e9:7.1f} TFLOP/s alg. (skip on)')
    return out_lines


def kernel_only():
    from xmem2_amd.s2m import S2MController
    torch.set_grad_enabled(False)
    net = _net()
    image, prev, scr = _inputs(1)
    ctl = S2MController(net, 1)
    for _ in range(60):
        ctl.interact(image, prev, scr)
    torch.cuda.synchronize()
    print('kernel-only: 60 interact() calls at K = 1 (1 capture)')


def family(name):
    n = name.replace('void ', '')
    if n.startswith('conv_mfma_kernel') and n.rstrip().endswith('true>(ConvArgs)'):
        return 'conv dilated (direct, DIL)'
    if n.startswith('conv_mfma_kernel') or n.startswith('conv_splitk') or n.startswith('conv_cout1'):
        return 'conv direct / pointwise / Winograd GEMM'
    if n.startswith('wino') or 'gemm_stream' in n:
        return 'conv Winograd transforms / streaming GEMM'
    if n.startswith('__amd_rocclr'):
        return 'runtime copies / fills'
    return 'elementwise (pack, pool, mean, resize, output)'


def kernel_stats(path, out_lines, forwards=61):
    rows = [r for r in csv.DictReader(open(path))]
    fam = {}
    for r in rows:
        f = family(r['Name'])
        d = fam.setdefault(f, [0, 0.0])
        d[0] += int(r['Calls'])
        d[1] += float(r['TotalDurationNs'])
    net = _net()
    flops, dflops, _ = _conv_flops(net, 1)
    out_lines.append('')
    out_lines.append(f'rocprofv3 --kernel-trace --stats of `s2m_bench.py --kernel-only` (K = 1: the eager warm-up + 60 replays = {forwards} '
                     f'executed forwards - the capture launches nothing; per forward = total / {forwards}):')
    conv_ns = 0.0
    for f, (c, ns) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
        out_lines.append(f'  {f:45s} launches {c:6d}   {ns / forwards / 1e3:9.1f} us per forward')
        if f.startswith('conv'):
            conv_ns += ns / forwards
    out_lines.append(f'  conv family {conv_ns / 1e3:.1f} us per forward for {flops / 1e9:.1f} GFLOP (algorithmic): '
                     f'{flops / conv_ns / 1e3:.1f} TFLOP/s = {flops / conv_ns / 1e3 / PEAK_FP32_TFLOPS:.2f} of the fp32 MFMA peak '
                     f'({PEAK_FP32_TFLOPS} TF)')
    out_lines.append('  top kernels:')
    for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:12]:
        short = r['Name'].replace('void ', '').split('(')[0]
        out_lines.append(f'    {short[:90]:90s} {int(r["Calls"]):6d} x {float(r["AverageNs"]) / 1e3:8.1f} us')
    return out_lines


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
