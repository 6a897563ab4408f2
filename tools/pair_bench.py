"""Isolated timing of the bottleneck pair (ops.conv2d_pointwise_pair) against its two separate launches, at the key pass's shapes and
under the plans conv2d chooses for them (the shipped table).  Each side is a HIP graph of 20 calls, replayed alternately over 7 rounds
(after one untimed replay each); the figure is the median over the rounds of replay time / 20.  The two sides' outputs are compared
(torch.equal) at every shape before anything is timed.

    python tools/pair_bench.py [--calls 20] [--rounds 7] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xmem2_amd import ops                                          # noqa: E402

SHAPES = [  # (B, H, W), (Cmid, 4 Cmid, Cmid')
    ((4, 120, 216), (64, 256, 64)), ((4, 120, 216), (64, 256, 128)), ((4, 60, 108), (128, 512, 128)), ((4, 60, 108), (128, 512, 256)),
    ((4, 30, 54), (256, 1024, 256)),
    ((1, 120, 216), (64, 256, 64)), ((1, 120, 216), (64, 256, 128)), ((1, 60, 108), (128, 512, 128)), ((1, 60, 108), (128, 512, 256)),
    ((1, 30, 54), (256, 1024, 256)),
]


def layer(cin, cout, g):
    w = torch.randn((cout, 1, 1, cin), generator=g) * (2.0 / cin) ** 0.5
    return ops.ConvWeights(w.cuda().contiguous(), (0.6 + 0.9 * torch.rand(cout, generator=g)).cuda(),
                           (0.2 * (torch.rand(cout, generator=g) - 0.5)).cuda(), 1, 0)


def graph_of(fn, calls):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'pair_bench needs the GPU'
    lines = [f'{"shape":<14s} {"channels":<14s} {"pixels":>7s} {"separate us":>12s} {"pair us":>9s} {"pair/sep":>9s} {"sep min..max":>15s} '
             f'{"pair min..max":>15s}  path']
    print(lines[0], flush=True)
    gen = torch.Generator().manual_seed(0)
    for (B, H, W), (k1, n1, n2) in SHAPES:
        o = torch.relu(torch.randn((B, H, W, k1), generator=gen)).cuda()
        res = torch.relu(torch.randn((B, H, W, n1), generator=gen)).cuda()
        e, r = layer(k1, n1, gen), layer(n1, n2, gen)
        y0, y1 = (torch.empty((B, H, W, n1), device='cuda') for _ in range(2))
        z0, z1 = (torch.empty((B, H, W, n2), device='cuda') for _ in range(2))

        def separate():
            ops.conv2d(o, e, out=y0, res=res, relu_out=True)
            ops.conv2d(y0, r, out=z0, relu_out=True)

        def pair():
            ops.conv2d_pointwise_pair(o, e, res, r, y=y1, z=z1)

        before = dict(ops.PAIR_STATS)
        separate()
        pair()
        torch.cuda.synchronize()
        path = 'pair kernel' if ops.PAIR_STATS['pair'] > before['pair'] else 'FELL BACK'
        same = torch.equal(y0, y1) and torch.equal(z0, z1)
        gs, gp = graph_of(separate, a.calls), graph_of(pair, a.calls)
        ts, tp = [], []
        for _ in range(a.rounds):
            ts.append(timed(gs) / a.calls)
            tp.append(timed(gp) / a.calls)
        ms, mp = statistics.median(ts), statistics.median(tp)
        lines.append(f'{B}x{H}x{W:<8d} {k1}-{n1}-{n2:<6d} {B * H * W:7d} {ms:12.1f} {mp:9.1f} {mp / ms:9.3f} '
                     f'{min(ts):7.1f}..{max(ts):<6.1f} {min(tp):7.1f}..{max(tp):<6.1f}  {path}, bits {"equal" if same else "DIFFER"}')
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
