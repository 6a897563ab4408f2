"""Records tests/golden/conv_plan_info.npz: for a grid of convolution descriptors, what xmem_conv2d_plan_info,
xmem_conv2d_workspace_bytes and xmem_conv2d_dilated_workspace_bytes answer (host-only entry points: runs without a GPU).

THE SHIPPED FIXTURE WAS RECORDED BEFORE THE PLAN CODE TABLE EXISTED: from a build whose make_plan / half_view / make_plan_half were
still the text of the commit before the table was introduced (the cascade of `t -= 10`, `t -= 6`, ... and the private half tile
value), with only the copy-out export xmem_conv2d_plan_info added.  It therefore pins that commit's fallback chain, split-K rule
and workspace formulas; its workspace columns equal what that commit's library returns for the same descriptors.  Re-record only
when a plan code is ADDED (new rows), never to make a restructuring pass.

    python tests/golden/make_conv_plan_goldens.py        # needs the built library, no GPU

The grid (all sizes are free, nothing launches):
  plan_tile -1..42 x plan_splitk {0, 1, 3, 64}
  x operand sets {w_winograd + w_winograd4 + w_winograd_f16, w_winograd only, none}
  x modes {fp32, fp32x, fp32x with w_winograd4_split, half with out_half 0, half with out_half 1}
  x layers: 3x3 s1 p1 with Cin {32, 36, 64} x Cout {1, 64, 96, 98} x ldout {Cout, Cout + 1}; the 64 -> 64 one also with a residual
    (ldres 64 and 66) and with an `out` pointer 4 bytes off 16-byte alignment; 3x3 s2; 7x7 s2 p3 with Cin 4; 1x1 p0 at stride 1 and
    2; 1x1 p1; two batches past the heuristic's 384-tile thresholds (128x128: 4x80x80, 64 -> 256; 128x64: 8x80x80, 64 -> 64), every
    other layer below them (its split-K branch)
  and the dilated query: dilation {1, 2, 6} x plan_tile 0..7 x plan_splitk as above x the same layers (fp32, all operands).
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import test_conv_plan_host as T  # noqa: E402


def layers():
    """rows of test_conv_plan_host.LAYER_COLS"""
    out = []
    for cin, cout, extra in itertools.product((32, 36, 64), (1, 64, 96, 98), (0, 1)):
        out.append((1, 17, 23, cin, cin, cout, 3, 1, 1, cout + extra, 0, 0))
    out += [(1, 17, 23, 64, 64, 64, 3, 1, 1, 64, 64, 0), (1, 17, 23, 64, 64, 64, 3, 1, 1, 64, 66, 0), (1, 17, 23, 64, 64, 64, 3, 1, 1, 64, 0, 4),
            (2, 30, 54, 64, 64, 64, 3, 2, 1, 64, 0, 0), (1, 96, 128, 4, 4, 64, 7, 2, 3, 64, 0, 0),
            (2, 30, 54, 256, 256, 64, 1, 1, 0, 64, 0, 0), (2, 30, 54, 256, 256, 128, 1, 2, 0, 128, 0, 0), (2, 30, 54, 64, 64, 64, 1, 1, 1, 64, 0, 0),
            (4, 80, 80, 64, 64, 256, 3, 1, 1, 256, 0, 0), (8, 80, 80, 64, 64, 64, 3, 1, 1, 64, 0, 0)]
    return out


if __name__ == '__main__':
    rows = np.array(layers(), np.int32)
    info, ws, dws = T.query(rows)
    np.savez_compressed(T.GOLDEN, layers=rows, info=info, workspace=ws, dilated_workspace=dws)
    print(f'{ws.size} + {dws.size} descriptors ({int((info[..., 0] == 0).sum())} resolved, '
          f'{len(np.unique(info.reshape(-1, info.shape[-1]), axis=0))} distinct plans), {os.path.getsize(T.GOLDEN)} bytes -> {T.GOLDEN}')
