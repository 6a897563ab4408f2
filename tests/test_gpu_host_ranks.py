"""8-GPU readiness that a 1-GPU box CAN measure: the HOST side of a rank.  north_star wants >= 7x at 8 GPUs; the device side scales by
construction (independent streams, no collective), so what can break it is the host: ~85 kernel launches / graph replays per 1.7 ms frame
from Python, times 8 ranks on one node.  This test runs 8 rank processes of `bench.py --scale-only`, each confined to its own
<= 8-CPU slice of the 8-way split exactly as `xmem2_amd.launch.pin_rank` confines a rank (they share the one GPU here, so their DEVICE
time says nothing), in waves of CONCURRENT processes: a shared GPU box may cap how many processes open the device at once (this test's
own process holds it too).  It asserts on the host time a frame costs: the time spent inside step() + the batched hint + the argmax launch, excluding
the wait for the mask of two frames ago (bench.py, XMEM_BENCH_HOST_TIMES).  If that stays well under the 1-GPU frame time with other
ranks' hosts busy beside it, eight ranks on eight GPUs are device-bound like one is."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = 8
CONCURRENT = 4                  # rank processes alive at once: with this test's own process, at most 5 hold the GPU
FRAME_MS_1GPU = 1.75            # B32 on one MI355X (BENCH_r05: 1.766 ms); the host must stay well below it
HOST_BUDGET_MS = 0.70 * FRAME_MS_1GPU

WRAP = ("import os, sys, runpy\n"
        "cpus = sorted(os.sched_getaffinity(0)); r, n = int(sys.argv[1]), int(sys.argv[2])\n"
        "per = max(1, min(8, len(cpus) // n))\n"
        "mine = cpus[r * per:(r + 1) * per] or cpus\n"
        "os.sched_setaffinity(0, mine)\n"
        "import torch; torch.set_num_threads(min(8, len(mine)))\n"
        "sys.argv = ['bench.py', '--scale-only', '--steps', '60', '--warmup', '5']\n"
        "runpy.run_path(os.path.join(os.getcwd(), 'bench.py'), run_name='__main__')\n")


def _host_ms(stderr):
    """mean over the phases of a key batch of the median host ms per frame: step + hint + argmax launch"""
    rows = re.findall(r'frame i%KB=(\d+): median host ms\s+step ([\d.]+)\s+hint ([\d.]+)\s+argmax launch ([\d.]+)\s+submit/wait ([\d.]+)', stderr)
    assert rows, 'bench.py printed no host-time table:\n' + stderr[-1500:]
    per_phase = [float(s) + float(h) + float(a) for _, s, h, a, _ in rows]
    return sum(per_phase) / len(per_phase), per_phase


def _run_wave(ranks, env):
    """the rank processes of `ranks` at the same time; stderr of each.  Every one of them is gone when this returns."""
    procs = [subprocess.Popen([sys.executable, '-c', WRAP, str(r), str(RANKS)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in ranks]
    try:
        outs = [p.communicate(timeout=900) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-2000:]            # a failed wave ends the test: the next one is not started
    return [se for _, se in outs]


def test_host_time_per_frame_under_8_concurrent_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    env.update(XMEM_BENCH_HOST_TIMES='1', PYTHONPATH=ROOT)
    errs = []
    for first in range(0, RANKS, CONCURRENT):
        errs += _run_wave(range(first, min(first + CONCURRENT, RANKS)), env)
    host = [_host_ms(se) for se in errs]
    means = [h[0] for h in host]
    print(f'host ms per frame (step + hint + argmax launch) of {RANKS} rank processes, {CONCURRENT} at a time, each on its own <= 8-CPU slice: '
          + ' '.join(f'{m:.3f}' for m in means) + f'; budget {HOST_BUDGET_MS:.2f} ms (0.7 x the 1-GPU frame of {FRAME_MS_1GPU} ms)')
    assert max(means) <= HOST_BUDGET_MS, f'the host side of a rank costs {max(means):.3f} ms per frame with {CONCURRENT} ranks busy at once: 8 GPUs would be host-bound'
