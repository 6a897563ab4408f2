"""bench.py's command line and output dump (no GPU): a plain run is lean unless --full, --dump-outputs writes float32 arrays within
its byte budget, and a dump that must be sampled takes the same elements every time."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_full_and_dump_outputs_are_opt_in():
    import bench
    a = bench.parse_args(['--steps', '7', '--warmup', '3'])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = bench.parse_args(['--full', '--dump-outputs', 'out'])
    assert a.full is True and a.dump_outputs == 'out'


def test_dump_outputs_writes_float32_within_budget(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    prob = rng.random((2, 48, 64)).astype(np.float64)
    mask = rng.integers(0, 2, (48, 64)).astype(np.uint8)
    bench.dump_outputs(str(tmp_path / 'a'), dict(last_step_prob=prob, last_step_mask=mask))
    p, m = np.load(tmp_path / 'a' / 'last_step_prob.npy'), np.load(tmp_path / 'a' / 'last_step_mask.npy')
    assert p.dtype == np.float32 and m.dtype == np.float32
    assert np.array_equal(p, prob.astype(np.float32)) and np.array_equal(m, mask)
    # over the budget: the same seeded sample of every array, no more bytes than allowed
    budget = 4096
    for d in ('b', 'c'):
        bench.dump_outputs(str(tmp_path / d), dict(last_step_prob=prob, last_step_mask=mask), budget=budget)
    sizes = [os.path.getsize(tmp_path / 'b' / f) - 128 for f in ('last_step_prob.npy', 'last_step_mask.npy')]
    assert 0 < sum(sizes) <= budget
    for f in ('last_step_prob.npy', 'last_step_mask.npy'):
        x, y = np.load(tmp_path / 'b' / f), np.load(tmp_path / 'c' / f)
        assert x.dtype == np.float32 and np.array_equal(x, y)
    assert set(np.unique(np.load(tmp_path / 'b' / 'last_step_mask.npy'))) <= {0.0, 1.0}
