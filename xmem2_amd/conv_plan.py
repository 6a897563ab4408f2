"""Which plan a convolution runs under: the plan codes, the shipped plan tables, the tuner, and the order they are consulted in.

A plan is (code, split-K).  The code is `xmem_conv_desc.plan_tile` (include/xmem_hip.h documents the numbering, kPlanCodes in
csrc/conv_plan.hpp is the library's table); CODES below is the same table for Python, and everything here that needs the meaning
of a code reads it from there.  tests/test_conv_plan_host.py holds CODES against what the library reports.
"""
import collections
import ctypes as C
import json
import os
import sys

import torch

from ._lib import ptr, stream_ptr

Code = collections.namedtuple('Code', 'form bm bn bk ring')
# form: 'direct' | 'f2' (Winograd F(2x2,3x3)) | 'f2_fused' (output transform fused into the GEMM) | 'f2_f16' (fp16 operands, the
# 'fp16w' mode) | 'f4' (F(4x4,3x3)); bm x bn: GEMM tile, 0 x 0 = chosen by the library from the size; bk: k-tile depth;
# ring: 0 = the implicit-GEMM kernel, 3 / 4 = the streaming kernel with that many LDS stages
_TILES3 = ((128, 128), (128, 64), (64, 64))
_STREAM3 = ((64, 64), (128, 64), (128, 128))
CODES = {0: Code('direct', 0, 0, 32, 0), 13: Code('f2_fused', 128, 64, 32, 0), 14: Code('f2_fused', 64, 64, 32, 0),
         15: Code('f2_fused', 64, 128, 32, 0), 16: Code('f2_f16', 0, 0, 32, 0)}
for _first, _form in ((1, 'direct'), (7, 'f2'), (17, 'f4')):
    CODES.update({_first + 3 * j + i: Code(_form, bm, bn, bk, 0) for j, bk in enumerate((32, 64)) for i, (bm, bn) in enumerate(_TILES3)})
for _first, _form in ((23, 'f4'), (29, 'f2'), (35, 'direct')):
    CODES.update({_first + 3 * j + i: Code(_form, bm, bn, 32, ring) for j, ring in enumerate((3, 4)) for i, (bm, bn) in enumerate(_STREAM3)})
# a half-typed call (the fp16 loop) runs the direct BK-32 tiles only; its own 256x128 tile is code 4; any other code: the heuristic
HALF_CODES = {1: CODES[1], 2: CODES[2], 3: CODES[3], 4: Code('direct', 256, 128, 32, 0), 5: CODES[2], 6: CODES[3]}
_BY_MEANING = {c: code for code, c in CODES.items()}


def code_of(form, bm, bn, bk=32, ring=0):
    return _BY_MEANING[Code(form, bm, bn, bk, ring)]


HEURISTIC, DIRECT_64, F2_64, F2_F16, F4_64 = 0, code_of('direct', 64, 64), code_of('f2', 64, 64), code_of('f2_f16', 0, 0), code_of('f4', 64, 64)


def reads_f4_operand(code):
    return code in CODES and CODES[code].form == 'f4'


def as_f2(code):
    """The F(2x2) code with the GEMM tile and kernel of an F(4x4) code."""
    return code_of('f2', *CODES[code][1:])


def executed_mfma_flops(B, Ho, Wo, cin, cout, kh, kw, stride, pad, code, winograd_ok, half=False):
    """MFMA FLOPs the library issues for one conv2d call under plan code `code` (what an EXECUTED roofline fraction must count,
    bench.py conv_roofline): the direct form contracts 2 * M * Cout * KH * KW * Cin with M / Cout padded to the tile and K to the
    32-deep k-tile; F(2x2) runs 16 position GEMMs over ceil(Ho/2) * ceil(Wo/2) tiles per image (1/2.25 of the direct FLOPs before
    padding), F(4x4) 36 over ceil(Ho/4) * ceil(Wo/4) (1/4).  Cout = 1 is a VALU GEMV: no MFMA work.  Conventions: a tile the
    library chooses itself (the heuristic, the fp16-operand form) is counted as 64x64, the half 256x128 tile as 128x128, and the
    code is taken as given (`winograd_ok` False turns a Winograd code into the direct form; no other fallback is followed)."""
    if cout == 1:
        return 0.0
    c = HALF_CODES.get(int(code), CODES[0]) if half else CODES.get(int(code), CODES[0])
    bm, bn = min(c.bm, 128) or 64, c.bn or 64
    up = lambda a, b: -(-a // b) * b
    if c.form == 'direct' or not winograd_ok:
        return 2.0 * up(B * Ho * Wo, bm) * up(cout, bn) * up(kh * kw * cin, 32)
    r, npos = (4, 36) if c.form == 'f4' else (2, 16)
    tiles = B * (-(-Ho // r)) * (-(-Wo // r))
    return npos * 2.0 * up(tiles, bm) * up(cout, bn) * up(cin, 32)


# ---- plan tables ---------------------------------------------------------------------------------------------
# Plans measured on an MI355X are shipped in conv_plans*.json (deterministic: the same plan -> the same summation order); shapes
# not listed there take a deterministic heuristic (same shape -> same tiles -> same summation order on every machine).
class PlanTable:
    """The plans of one kind of kernels: the shipped file (read on first use), then the plans this process chose."""

    def __init__(self, filename, inherit=None, f4_marker=False):
        self.path = os.path.join(os.path.dirname(os.path.abspath(__file__)), filename)
        self.inherit = inherit            # table asked for a shape this one lacks (not under AUTOTUNE: the tuner measures these kernels)
        self.f4_marker = f4_marker
        self.chosen = {}
        self._shipped = None

    @property
    def shipped(self):
        if self._shipped is None:
            self._shipped = {}
            if os.path.exists(self.path):
                try:
                    self._shipped = {k: tuple(v) for k, v in json.load(open(self.path)).items()}
                except Exception:
                    pass
        return self._shipped

    def forget_shipped(self):
        """A full retune (tools/tune_convs.py, XMEM_RETUNE_ALL): every shape is measured again."""
        self._shipped = {}

    def get(self, key, autotune=False):
        plan = self.shipped.get(key) or self.chosen.get(key)
        if plan is None and self.inherit is not None and not autotune:
            plan = self.inherit.get(key)
        return plan

    def dump(self, path):
        """Write every plan known to this process (shipped + chosen now) in the format of the shipped files; returns their number."""
        allp = dict(self.shipped)
        allp.update(self.chosen)
        if self.f4_marker and (os.environ.get('XMEM_RETUNE_ALL') or '__tuned_with_f4__' in allp):
            allp['__tuned_with_f4__'] = (1, 0)       # EVERY entry was measured against the F(4x4) candidates (full retune only)
        with open(path, 'w') as f:
            json.dump({k: list(v) for k, v in sorted(allp.items())}, f, indent=0)
        return len(allp)


FP32 = PlanTable('conv_plans.json', f4_marker=True)
FP32X = PlanTable('conv_plans_fp32x.json', inherit=FP32)      # split-operand kernels: the GEMMs are ~4x cheaper, other tiles win
FP16 = PlanTable('conv_plans_fp16.json')                      # the half kernels of the fp16 loop
TABLES = {'fp32': FP32, 'fp32x': FP32X, 'fp16': FP16}

# The heuristic plan (shapes the table does not list) takes F(4x4,3x3) from this many output pixels (1/8 resolution of 480p and
# up), F(2x2,3x3) below: there the 36 tile-position GEMMs are too small to fill the chip.
F4_MIN_PIXELS = 4096
# XMEM_CONV_AUTOTUNE=1 opts in to timing the candidates at first use (tools/tune_convs.py does, to refresh conv_plans.json).
AUTOTUNE = os.environ.get('XMEM_CONV_AUTOTUNE', '0') == '1'
# Tools knob (parity attribution, tests/parity_by_plan.py): 'direct' runs every convolution in the direct implicit-GEMM form,
# 'f2' replaces F(4x4) by F(2x2), 'direct_sk2' / 'direct_sk3' = the direct form summed in 2 / 3 slabs; None / '' = the shipped plan
# table.  Read at call time so that a tool can switch it.
CONV_FORM = os.environ.get('XMEM_CONV_FORM') or None
# the CONV_FORM forms that fix the plan outright: the library's deterministic direct-form heuristic; the direct form with every
# contraction cut into 2 / 3 slabs summed afterwards (the SAME products in another fp32 summation order)
_DIRECT_FORMS = {'direct': (HEURISTIC, 0), 'direct_sk2': (DIRECT_64, 2), 'direct_sk3': (DIRECT_64, 3)}
# Tools (tools/tune_convs.py): XMEM_RETUNE_MARGIN=0.05 re-measures every TABLED shape against its candidates and replaces the tabled
# plan only when a candidate is more than that fraction faster (12-launch timings, best of two): a table refresh after a kernel
# change without the churn of equal-within-noise entries.
RETUNE_MARGIN = float(os.environ.get('XMEM_RETUNE_MARGIN', '0') or 0)
# Streaming-GEMM variants of a tabled Winograd plan (csrc/gemm_stream.hip): XMEM_TUNE_STREAM=1 (tools/tune_convs.py) times the
# tabled plan against them once per shape and keeps a variant only when it is at least 3 % faster (same arithmetic, same
# summation order: results are bit-identical either way).
TUNE_STREAM = os.environ.get('XMEM_TUNE_STREAM', '0') == '1'
_STREAM_VARIANTS = {F4_64: [code_of('f4', bm, bn, ring=r) for bm, bn, r in ((64, 64, 3), (64, 64, 4), (128, 64, 3))],
                    F2_64: [code_of('f2', 64, 64, ring=r) for r in (3, 4)]}
_retuned, _stream_checked = set(), set()


def tabled_or_heuristic(key, mode, autotune, has_winograd, wino_ok, pixels):
    """(plan, tabled): the plan of layer `key` in the table of `mode` ('fp32' | 'fp32x' | 'fp16'), else the deterministic
    heuristic: a 3x3 stride-1 layer with its Winograd operand (`has_winograd`) and 4-aligned channel strides (`wino_ok`) still
    takes Winograd with the 64x64 GEMM tile - F(4x4) from F4_MIN_PIXELS output pixels - anything else the library's direct-form
    heuristic.  No GPU, no state but the tables."""
    plan = TABLES[mode].get(key, autotune)
    if plan is not None:
        return plan, True
    if mode != 'fp16' and has_winograd and wino_ok:
        return (F4_64 if pixels >= F4_MIN_PIXELS else F2_64, 1), False
    return (HEURISTIC, 0), False


# ---- tuner ---------------------------------------------------------------------------------------------------
def _time_plan(lib, d, dev, plan, warmup=3, reps=12, rounds=2):
    """ms per launch of `d` under `plan` (best of `rounds` timings of `reps` launches), None when the library refuses it."""
    from .ops import workspace
    d.plan_tile, d.plan_splitk = plan
    need = lib.xmem_conv2d_workspace_bytes(C.byref(d))
    ws = workspace(need, dev, 'conv') if need else None
    st = stream_ptr()
    for _ in range(warmup):
        if lib.xmem_conv2d_nhwc(C.byref(d), ptr(ws), need, st) != 0:
            return None
    best = None
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            lib.xmem_conv2d_nhwc(C.byref(d), ptr(ws), need, st)
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1) / reps
        best = t if best is None or t < best else best
    return best


def _fastest(lib, d, dev, plans, **timing):
    best, best_t = (HEURISTIC, 0), None
    for plan in plans:
        t = _time_plan(lib, d, dev, plan, **timing)
        if t is not None and (best_t is None or t < best_t):
            best, best_t = plan, t
    return best, best_t


def _tune_conv(lib, call, incumbent=None):
    """Time the candidate plans for this call's descriptor; returns the fastest (or `incumbent` unless beaten by RETUNE_MARGIN).
    `call.f4_operand()` points the descriptor at the F(4x4) operand of a layer that has the F(2x2) one."""
    d, dev = call.d, call.x.device
    M, K = d.B * call.Ho * call.Wo, d.KH * d.KW * d.Cin
    forms = ['direct']
    if d.w_winograd and d.ldout % 4 == 0 and (not d.res or d.ldres % 4 == 0):
        forms += ['f2', 'f2_fused']
        if call.Ho * call.Wo >= 256:          # F(4x4,3x3): the same GEMM tiles over 36 positions
            call.f4_operand()
            forms.append('f4')
    plans = []
    for code, c in sorted(CODES.items()):
        if c.form not in forms or c.ring or not c.bm:
            continue
        if c.bn == 128 and d.Cout <= 64 and c.form != 'f2_fused':
            continue
        nt = -(-M // c.bm) * -(-d.Cout // c.bn)
        nk = -(-K // c.bk)
        for sk in ((1, 2, 3, 4, 6, 8, 12, 16) if c.form == 'direct' else (1,)):
            if c.form == 'f4' and nt * 36 < 128:
                continue
            if sk > 1 and (nt * sk > 2048 or nk // sk < 2):
                continue
            if sk == 1 and nt < 48 and nk >= 16:
                continue
            plans.append((code, sk))
    if incumbent is None:
        return _fastest(lib, d, dev, plans, warmup=2, reps=4, rounds=1)[0]
    best, best_t = _fastest(lib, d, dev, plans)
    t_inc = _time_plan(lib, d, dev, tuple(incumbent))
    if t_inc is not None and (best_t is None or best_t > (1.0 - RETUNE_MARGIN) * t_inc):
        return tuple(incumbent)
    print(f'[retune] {tuple(incumbent)} {t_inc and round(t_inc * 1e3, 1)} us -> {best} {best_t and round(best_t * 1e3, 1)} us', file=sys.stderr)
    return best


def _tune_conv_half(lib, d, dev):
    """The same for the half kernels: their four tiles, split-K 1..8."""
    tiles = sorted({c: code for code, c in sorted(HALF_CODES.items(), reverse=True)}.values())    # one code per distinct tile
    return _fastest(lib, d, dev, [(code, sk) for code in tiles for sk in (1, 2, 4, 8)], reps=8)[0]


def _tune_stream(lib, d, dev, plan):
    base = _time_plan(lib, d, dev, plan)
    best, best_t = plan, base
    if base is not None:
        for code in _STREAM_VARIANTS[plan[0]]:
            t = _time_plan(lib, d, dev, (code, 1))
            if t is not None and t < 0.97 * base and t < best_t:
                best, best_t = (code, 1), t
    return best


def choose(lib, call, plan):
    """(code, split-K) of one conv2d call (`call`: its ops.ConvCall, `plan`: what the caller asked for), with the call's descriptor
    pointed at the F(4x4) operand (`call.f4_operand()`) when the plan reads it.  The plan is, in this order:
    1. the caller's plan, taken literally (tests, tools, the fp16w mode);
    2. a CONV_FORM attribution form (fp32 mode);
    3. the plan table of the mode (the shipped conv_plans*.json, then the plans this process chose before);
    4. the tuner: AUTOTUNE times the candidates of a shape the table lacks (with RETUNE_MARGIN also those of a tabled shape),
       TUNE_STREAM tries the streaming-GEMM variants of a Winograd plan;
    5. the deterministic heuristic: same shape -> same plan -> same summation order on every machine.
    CONV_FORM 'f2' then runs the GEMM tile of an F(4x4) plan under F(2x2).  Steps 3 and 5 are `tabled_or_heuristic`."""
    d, key, has_winograd = call.d, call.key, call.cw.wu is not None
    half, split = call.half, d.arith == 1
    fp32 = not half and call.precision == 'fp32'
    explicit = plan is not None or (fp32 and CONV_FORM in _DIRECT_FORMS)
    capturing = torch.cuda.is_current_stream_capturing()
    if explicit:
        plan = tuple(plan) if plan is not None else _DIRECT_FORMS[CONV_FORM]
    else:
        mode = 'fp16' if half else 'fp32x' if split else 'fp32'
        tune = AUTOTUNE and call.cw.cout > 1 and not capturing
        plan, tabled = tabled_or_heuristic(key, mode, AUTOTUNE, has_winograd, call.wino_ok, call.B * call.Ho * call.Wo)
        if tabled and tune and fp32 and RETUNE_MARGIN > 0 and key not in _retuned:
            _retuned.add(key)                     # tools: the tabled plan against its candidates, replaced only when clearly beaten
            if reads_f4_operand(plan[0]) and has_winograd:
                call.f4_operand()
            new_plan = _tune_conv(lib, call, incumbent=plan)
            if new_plan != plan:
                plan = TABLES[mode].chosen[key] = new_plan
        if not tabled:
            if tune:
                plan = _tune_conv_half(lib, d, call.x.device) if half else _tune_conv(lib, call)
            TABLES[mode].chosen[key] = plan
        if CONV_FORM == 'f2' and reads_f4_operand(plan[0]):
            plan = (as_f2(plan[0]), plan[1])
    d.w_winograd4 = None
    if not half and reads_f4_operand(plan[0]) and has_winograd:
        call.f4_operand()
    if TUNE_STREAM and not (explicit or half or split) and plan[0] in _STREAM_VARIANTS and key not in _stream_checked and not capturing:
        _stream_checked.add(key)
        plan = FP32.chosen[key] = _tune_stream(lib, d, call.x.device, plan)
    return plan
