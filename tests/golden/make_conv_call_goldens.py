"""Records tests/golden/conv_call_trace.json: what the convolution front end of xmem2_amd/ops.py hands to the library in the scenarios
of tests/test_gpu_conv_call_trace.py (the proxy and the scenarios live there; this script only runs them and writes the file).

THE SHIPPED FIXTURE WAS RECORDED AT THE COMMIT BEFORE `ops.ConvCall` EXISTED, with the front end still made of three positional helpers
(descriptor, preparation, run): it pins the descriptors, plan keys, RECORD entries and fall-backs of that front end.  Re-record only
when a scenario is ADDED or the library's interface changes, never to make a restructuring of ops.py pass.

    python tests/golden/make_conv_call_goldens.py [OUTPUT.json]        # needs the built library and an MI355X
"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_gpu_conv_call_trace as T  # noqa: E402


if __name__ == '__main__':
    from xmem2_amd.synth import synthetic_state_dict
    torch.set_grad_enabled(False)
    out = {}
    for name, scenario in T.SCENARIOS.items():
        with pytest.MonkeyPatch.context() as mp:
            out[name] = T.trace(mp, scenario)
    sd = synthetic_state_dict(0)
    for mode in T.NETWORK_MODES:
        with pytest.MonkeyPatch.context() as mp:
            out['network_' + mode] = T.trace(mp, T.network, sd, mode)
    path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    with open(path, 'w') as f:          # one scenario per line
        f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + '\n}\n')
    calls = sum(len(v['calls']) + len(v.get('extra') or []) * k.startswith('network_') for k, v in out.items())
    print(f'{len(out)} scenarios, {calls} library calls, {os.path.getsize(path)} bytes -> {path}')
