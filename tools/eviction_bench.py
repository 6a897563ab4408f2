"""Time ONE least-used eviction of a long-term store (KeyValueMemoryStore.remove_obsolete_features) on the GPU.

    python tools/eviction_bench.py [--elements 10000] [--prototypes 128] [--reps 40] [--warmup 5]

Layouts: one group of 1 object, one group of 3 objects, and two groups (2 objects + 1 object that appeared later and holds 60 % of the
elements).  For the single-group layouts the path this one replaced - one `ops.gather_rows` plus a copy per arena and per object, as
the parent commit's `_Arena.take` ran it - is restated below and timed in the same process, alternating with the new path rep by rep;
the parent refused several groups, so the two-group layout has no baseline.  A time is the host clock around a call that ends in the
transfer of the new row counts (a device synchronise); the store is rebuilt, untimed, before every rep.  Prints the median, the 10th and
90th percentile and the extremes per variant, and one JSON line.  There is no CPU path: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYOUTS = {'1 group x 1 object': [(1, 1.0)], '1 group x 3 objects': [(3, 1.0)], '2 groups (2 + 1 objects)': [(2, 1.0), (1, 0.6)]}


def build(tensors, layout):
    from xmem2_amd.kv_memory_store import KeyValueMemoryStore
    key, shr, val, use = tensors
    N = key.shape[0]
    st = KeyValueMemoryStore(count_usage=True)
    st.add(key, [val[:n_obj, N - int(N * part):] for n_obj, part in layout], shr, None, None)
    st._use.rows().copy_(use)
    st._life.rows().fill_(1.0)
    return st


def evict_gather(st, max_size):
    """The parent commit's single-group eviction: a gather and a copy back per arena and per object."""
    from xmem2_amd import ops
    assert st.num_groups == 1
    k = st.size - max_size
    usage = st.get_usage_rows()
    vals, _ = ops.topk_1d(usage, k, largest=False)
    index, count = ops.select_greater(usage, vals[k - 1:k])
    m = int(count.item())
    index = index[:m]
    for arena in [st._k, st._use, st._life, st._s, st._r16] + list(st._v):
        if arena.lead:
            for i in range(arena.lead[0]):
                arena.buf[i, :m].copy_(ops.gather_rows(arena.buf[i, :arena.n], index))
        else:
            arena.buf[:m].copy_(ops.gather_rows(arena.buf[:arena.n], index))
        arena.n = m
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--elements', type=int, default=10000)
    ap.add_argument('--prototypes', type=int, default=128)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eviction_bench: no GPU - nothing is measured without one')
    N, max_size = a.elements, a.elements - a.prototypes
    g = torch.Generator(device='cuda').manual_seed(0)
    tensors = (torch.randn(N, 64, generator=g, device='cuda'), torch.rand(N, generator=g, device='cuda') * 3 + 1,
               torch.randn(3, N, 512, generator=g, device='cuda'), torch.rand(N, generator=g, device='cuda'))
    result = {'elements': N, 'max_size': max_size, 'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'ms': {}}
    for name, layout in LAYOUTS.items():
        variants = [('store_compact', lambda st: st.remove_obsolete_features(max_size))]
        if len(layout) == 1:
            variants.append(('gather per arena (parent)', lambda st: evict_gather(st, max_size)))
        times = {v: [] for v, _ in variants}
        sizes = set()
        for rep in range(a.warmup + a.reps):
            for v, fn in variants:                          # alternating: both see the same neighbours on the machine
                st = build(tensors, layout)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(st)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                sizes.add((st.size,) + tuple(st.get_v_size(gi) for gi in range(st.num_groups)))
                if rep >= a.warmup:
                    times[v].append(dt * 1e3)
        assert len(sizes) == 1, f'{name}: the variants disagree on the sizes {sizes}'
        for v, ts in times.items():
            ts = np.array(ts)
            stats = dict(median=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)),
                         min=float(ts.min()), max=float(ts.max()))
            result['ms'][f'{name} / {v}'] = stats
            print(f'{name:28s} {v:28s} median {stats["median"]:.3f} ms  p10 {stats["p10"]:.3f}  p90 {stats["p90"]:.3f}  '
                  f'min {stats["min"]:.3f}  max {stats["max"]:.3f}  -> sizes {sorted(sizes)[0]}')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
