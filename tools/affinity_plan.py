"""Which pipeline xmem_affinity_topk_hinted runs for a memory, and with what grid (host only, xmem_affinity_plan_info).

    python tools/affinity_plan.py 8161 129 30            one segment of 8161 elements, HW = 129, top_k = 30
    python tools/affinity_plan.py 1,1,1,8100 129 30 --hint 30
XMEM_AFFINITY_FILTER16=0 in the environment moves hinted calls to the fp32 select, as it does for the call itself.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
ROUTES = ('small', 'large-sampled', 'large-hinted-fp32', 'large-hinted-filter16')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('segments', help='segment sizes, comma separated (at most 4)')
    ap.add_argument('HW', type=int)
    ap.add_argument('top_k', type=int)
    ap.add_argument('--hint', type=int, default=None, help="top_k of a hint from an earlier call (same number of segments)")
    a = ap.parse_args()
    from xmem2_amd import _lib
    lib = _lib.load()
    sizes = [int(s) for s in a.segments.split(',')]
    arr = (C.c_int * len(sizes))(*sizes)
    hp = None
    if a.hint is not None:
        h = _lib.AffinityHint()
        h.idx, h.top_k, h.n_seg = 0x10, a.hint, len(sizes)          # the address is compared with NULL, never dereferenced
        hp = C.byref(h)
    out = _lib._STRUCTS['xmem_affinity_plan']()
    _lib.check(lib.xmem_affinity_plan_info(C.cast(arr, C.c_void_p), len(sizes), a.HW, a.top_k, hp, C.byref(out)))
    fields = {f: getattr(out, f) for f, _ in out._fields_}
    print(ROUTES[fields.pop('route')], ' '.join(f'{k}={v}' for k, v in fields.items()))


if __name__ == '__main__':
    main()
