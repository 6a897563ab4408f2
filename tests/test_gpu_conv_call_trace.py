"""What the convolution front end of xmem2_amd/ops.py hands to the library, call by call, against tests/golden/conv_call_trace.json.

The bit-exact tests pin what the convolutions compute.  A changed plan key (the string that indexes conv_plans*.json), descriptor
field or fall-back changes no bit: it costs speed.  So this module replaces `ops.load` by a proxy around the real library that records
every `xmem_conv2d_*` and `xmem_mask_head_gather` call - the symbol, every integer field of each descriptor, each pointer as null /
non-null, the scalar arguments, the answer - and forwards it; the plan keys that were looked up (`conv_plan.tabled_or_heuristic`) since the
previous call ride on the next one.  Per scenario it also keeps the movement of SHARED_STATS and PAIR_STATS, the (kind, key, flops,
info) of every RECORD entry, the number of operand builds (`split_pack`, `winograd4_weights`) and the text of every refusal.

The golden was recorded by tests/golden/make_conv_call_goldens.py (this module's scenarios) on an MI355X from the commit before the
front end was rebuilt around `ops.ConvCall`; every scenario must reproduce it exactly.  Re-record only when a scenario is ADDED or the
library's interface changes, never to make a restructuring of ops.py pass."""
import contextlib
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_call_trace.json')
TRACED = lambda name: name.startswith('xmem_conv2d_') or name == 'xmem_mask_head_gather'
OPERANDS = ('wu', 'wu_f16', 'wu4', 'w_sp', 'wu_sp', 'wu4_sp', 'w_h')


def _desc(d):
    from xmem2_amd._lib import ConvDesc
    return {name: (int(getattr(d, name)) if typ is C.c_int else bool(getattr(d, name))) for name, typ in ConvDesc._fields_}


def _arg(argtype, a):
    from xmem2_amd._lib import ConvDesc
    if argtype is C.POINTER(ConvDesc):
        return _desc(a._obj if hasattr(a, '_obj') else a.contents)
    if argtype is C.POINTER(C.POINTER(ConvDesc)):
        return [_desc(p.contents) for p in a]
    if argtype is C.POINTER(C.c_void_p):
        return [bool(v) for v in a]
    if argtype is C.POINTER(C.c_size_t):
        return [int(v) for v in a]
    if argtype is C.c_void_p:
        return bool(a.value if isinstance(a, C.c_void_p) else a)
    return int(a.value if hasattr(a, 'value') else a)


class Tracer:
    """The proxy library (`lib()` returns it) and what one scenario left behind (`result()`)."""

    def __init__(self, ops, real):
        self.ops, self.real = ops, real
        self.calls, self.pending, self.records, self.errors = [], [], [], []
        self.builds = {'split_pack': 0, 'winograd4_weights': 0}
        self.stats0 = (dict(ops.SHARED_STATS), dict(ops.PAIR_STATS))
        self._wrapped = {}

    def __getattr__(self, name):                    # only what the instance lacks: the library's symbols
        fn = getattr(self.real, name)
        if not TRACED(name):
            return fn
        if name not in self._wrapped:
            from xmem2_amd._lib import _SIGS
            argtypes = _SIGS[name][1]

            def call(*args):
                entry = {'symbol': name, 'keys': self.pending or None, 'args': [_arg(t, a) for t, a in zip(argtypes, args)]}
                self.pending = []
                self.calls.append(entry)            # before the call: a launch that raises is still on the list
                entry['ret'] = int(fn(*args))
                return entry['ret']
            self._wrapped[name] = call
        return self._wrapped[name]

    def looked_up(self, inner):
        def tabled_or_heuristic(key, *args, **kw):
            self.pending.append(key)
            return inner(key, *args, **kw)
        return tabled_or_heuristic

    def counted(self, name, inner):
        def build(*args, **kw):
            self.builds[name] += 1
            return inner(*args, **kw)
        return build

    @contextlib.contextmanager
    def recording(self):
        """`ops.RECORD` on for the calls inside; their entries without the launch closure and the tensors."""
        self.ops.RECORD = []
        try:
            yield
        finally:
            rec, self.ops.RECORD = self.ops.RECORD, None
            self.records += [[kind, key, flops, keep[5]] for kind, key, flops, _, keep in rec]

    def refused(self, fn):
        with pytest.raises(RuntimeError) as e:
            fn()
        self.errors.append(str(e.value))

    def operands(self, cw):
        """Which lazily built operands a ConvWeights holds by now."""
        return {n: getattr(cw, n) is not None for n in OPERANDS}

    def result(self, extra=None):
        shared, pair = ({k: d[k] - d0[k] for k in d} for d, d0 in zip((self.ops.SHARED_STATS, self.ops.PAIR_STATS), self.stats0))
        out = dict(calls=self.calls, shared_stats=shared, pair_stats=pair, record=self.records, builds=self.builds, errors=self.errors)
        if extra is not None:
            out['extra'] = extra
        return json.loads(json.dumps(out))          # tuples -> lists, as the golden file holds them


def trace(mp, scenario, *args):
    """Run `scenario(tracer, *args)` with the proxy in place (`mp`: a pytest MonkeyPatch, undone by its owner) -> Tracer.result()."""
    from xmem2_amd import conv_plan, ops
    t = Tracer(ops, ops.load())
    mp.setattr(ops, 'load', lambda: t)
    mp.setattr(conv_plan, 'tabled_or_heuristic', t.looked_up(conv_plan.tabled_or_heuristic))
    for name in t.builds:
        mp.setattr(ops, name, t.counted(name, getattr(ops, name)))
    assert ops.RECORD is None
    extra = scenario(t, *args)
    torch.cuda.synchronize()
    return t.result(extra)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def weights(cout, cin, k, stride=1, pad=None, seed=0, dilation=1):
    from xmem2_amd.ops import ConvWeights
    g = torch.Generator().manual_seed(7919 * seed + 31 * cout + cin + k)
    w = torch.randn(cout, k, k, cin, generator=g) * (1.0 / (cin * k * k)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) * 0.5 + 0.75, torch.randn(cout, generator=g) * 0.1
    return ConvWeights(w.cuda(), scale.cuda(), shift.cuda(), stride, k // 2 if pad is None else pad, dilation=dilation)


def act(*shape, seed=1, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda().to(dtype)


# ---- scenarios: f(tracer) --------------------------------------------------------------------------------------------------------
def plain(t):
    ops = t.ops
    x, cw = act(2, 9, 11, 32), weights(32, 32, 3)
    res = act(2, 9, 11, 32, seed=2)
    ops.conv2d(x, cw)
    ops.conv2d(x, cw, res=res)
    ops.conv2d(x, cw, relu_in=True)
    ops.conv2d(x, cw, relu_out=True)
    ops.conv2d(x, cw, res=res, relu_in=True, relu_out=True)
    wide = act(2, 9, 11, 48, seed=3)
    ops.conv2d(x, cw, out=wide[..., 8:40], out_ld=48)
    ops.conv2d(x, cw, res=wide[..., 8:40], res_ld=48, relu_out=True)
    ops.conv2d(x, cw, res=act(1, 9, 11, 32, seed=4), res_broadcast=True)
    return t.operands(cw)


def plain_explicit_plans(t):
    from xmem2_amd import conv_plan
    x, cw = act(2, 9, 11, 32), weights(32, 32, 3)
    for plan in ((conv_plan.DIRECT_64, 2), (conv_plan.F2_64, 1), (conv_plan.F4_64, 1)):
        t.ops.conv2d(x, cw, plan=plan)
    return t.operands(cw)


def stem_pointwise_gemv(t):
    t.ops.conv2d(act(1, 18, 22, 4), weights(64, 4, 7, stride=2, pad=3))
    t.ops.conv2d(act(2, 9, 11, 64), weights(128, 64, 1, stride=2, pad=0))
    t.ops.conv2d(act(2, 12, 16, 32), weights(1, 32, 3), relu_in=True)


def half(t):
    ops = t.ops
    h = torch.float16
    c3, c1 = weights(32, 32, 3), weights(128, 64, 1, stride=2, pad=0)
    with ops.precision('fp16'):
        ops.conv2d(act(2, 9, 11, 32, dtype=h), c3)
        ops.conv2d(act(2, 9, 11, 64, dtype=h), c1)
        ops.conv2d(act(2, 9, 11, 32, dtype=h), c3, out_dtype=torch.float32)
        ops.conv2d(act(2, 9, 11, 64, dtype=h), c1, out_dtype=torch.float32, relu_out=True)
        wide = act(2, 9, 11, 48, dtype=h)
        ops.conv2d(wide[..., 8:40], c3, in_ld=48, cin=32)
        t.refused(lambda: ops.conv2d(wide[..., 8:28], weights(32, 20, 3), in_ld=48, cin=20))       # not a multiple of 8
        t.refused(lambda: ops.conv2d(wide[..., 24:], c3, in_ld=48, cin=32))                        # crosses the pixel stride
    return t.operands(c3)


def split_and_fp16w(t):
    ops = t.ops
    x, cw = act(2, 9, 11, 32), weights(32, 32, 3)
    seen = []
    with ops.precision('fp32x'):
        for _ in range(2):
            ops.conv2d(x, cw)
            seen.append(dict(t.builds, **t.operands(cw)))
    cw64 = weights(64, 64, 3)
    with ops.precision('fp16w'):
        ops.conv2d(act(2, 9, 11, 64), cw64)
    return seen + [t.operands(cw64)]


def dilated(t):
    ops = t.ops
    x = act(1, 13, 17, 32)
    cw2, cw3 = (weights(32, 32, 3, pad=d, dilation=d) for d in (2, 3))
    ops.conv2d(x, cw2, relu_out=True)
    ops.conv2d(x, cw3, res=act(1, 13, 17, 32, seed=2))
    with t.recording():
        ops.conv2d(x, cw2, relu_in=True)
    ops.conv2d_dilated(x, weights(32, 32, 3, pad=2), dilation=2, plan=(3, 1), tap_skip=False)


def shared(t):
    from xmem2_amd.conv_plan import F4_64
    ops = t.ops
    x = act(1, 16, 20, 32)
    a, b, c = (weights(32, 32, 3, seed=s) for s in (1, 2, 3))
    kw = lambda cw, **more: dict(cw=cw, plan=(F4_64, 1), **more)
    ops.conv2d_shared(x, [kw(a, relu_in=True, relu_out=True), kw(b)])
    ops.conv2d_shared(x, [kw(a, relu_in=True), kw(b, res=act(1, 16, 20, 32, seed=2)), kw(c, relu_out=True)])


def deferred_and_folded(t):
    from xmem2_amd.conv_plan import F2_64, F4_64
    ops = t.ops
    x = act(1, 16, 20, 32)
    a, b, c = (weights(32, 32, 3, seed=s) for s in (1, 2, 3))
    kw = lambda cw, **more: dict(cw=cw, plan=(F4_64, 1), **more)
    o, branch = ops.conv2d_shared(x, [kw(a, relu_in=True, relu_out=True), kw(b)], defer=1)
    ops.conv2d_folded(o, c, branch, relu_out=True, plan=(F4_64, 1))
    o, branch = ops.conv2d_shared(x, [kw(a, relu_in=True, relu_out=True), kw(b)], defer=1)
    branch.finish()
    o, branch = ops.conv2d_shared(x, [kw(a, relu_in=True, relu_out=True), kw(b)], defer=1)
    ops.conv2d_folded(o, c, branch, plan=(F2_64, 1))                   # not F(4x4): the library declines, the branch finishes itself


def shared_fallbacks(t):
    from xmem2_amd.conv_plan import F4_64
    ops = t.ops
    x = act(1, 16, 20, 32)
    a, b = weights(32, 32, 3, seed=1), weights(32, 32, 3, seed=2)
    kw = lambda cw, **more: dict(cw=cw, plan=(F4_64, 1), **more)
    with t.recording():
        ops.conv2d_shared(x, [kw(a), kw(b)])
    with ops.precision('fp16'):
        ops.conv2d_shared(x.half(), [kw(a), kw(b)])
    ops.conv2d_shared(x, [kw(a), dict(cw=weights(32, 32, 3, pad=2, dilation=2))])


def pair(t):
    ops = t.ops
    o = act(2, 8, 12, 64)
    expand, reduce = weights(256, 64, 1, pad=0, seed=1), weights(64, 256, 1, pad=0, seed=2)
    ops.conv2d_pointwise_pair(o, expand, act(2, 8, 12, 256, seed=2), reduce)
    wide = act(2, 8, 12, 320, seed=3)
    ops.conv2d_pointwise_pair(o, expand, wide[..., 32:288], reduce)
    ops.conv2d_pointwise_pair(o, expand, act(1, 8, 12, 256, seed=4), reduce, res_broadcast=True)
    with t.recording():
        ops.conv2d_pointwise_pair(o, expand, act(2, 8, 12, 256, seed=2), reduce)
    ops.conv2d_pointwise_pair(o, expand, act(2, 8, 12, 256, seed=2), weights(64, 256, 1, stride=2, pad=0, seed=2))


def mask_head(t):
    K, h, w = 2, 3, 4
    cw = weights(1, 32, 3)
    for on in (False, True):
        args = (act(K, h, w, 32, seed=1), act(K, 2 * h, 2 * w, 32, seed=2), act(K, 4 * h, 4 * w, 32, seed=3), cw, act(K, h, w, 64, seed=4),
                torch.zeros(K, h, w, 100).cuda(), torch.zeros(K, h, w, 72).cuda(), 4)
        with (t.recording() if on else contextlib.nullcontext()):
            t.ops.mask_head_gather(*args)


def tabled(t):
    """The one place the shipped tables are hit: the keys below are copied from conv_plans.json, conv_plans_fp32x.json and
    conv_plans_fp16.json, and the descriptors must carry THEIR plans, not the heuristic's."""
    from xmem2_amd import conv_plan
    ops = t.ops
    key, key_h = '1x120x216x256/256->256/256 k3s1p1 r000', 'h1x120x216x256/256->256/256 k3s1p1 r000o1'
    plans = [conv_plan.FP32.shipped[key], conv_plan.FP32X.shipped[key], conv_plan.FP16.shipped[key_h]]
    x, cw = act(1, 120, 216, 256), weights(256, 256, 3)
    ops.conv2d(x, cw)
    with ops.precision('fp32x'):
        ops.conv2d(x, cw)
    with ops.precision('fp16'):
        ops.conv2d(x.half(), cw)
    launches = [c for c in t.calls if c['symbol'] == 'xmem_conv2d_nhwc']
    got = [(c['args'][0]['plan_tile'], c['args'][0]['plan_splitk']) for c in launches]
    assert got == [tuple(p) for p in plans], (got, plans)
    assert got[0] != (conv_plan.F4_64, 1) and got[2] != (conv_plan.HEURISTIC, 0)       # what the heuristic would have said
    return [list(p) for p in plans]


def network(t, sd, mode):
    """One pass of XMem at 96x128 with two objects (key, value, one segment step), eager; only the order of the calls and their
    plans are kept.  The pair and tail kernels are switched on at this small size, as their own tests do."""
    from xmem2_amd.network import XMem
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    ops = t.ops
    net = XMem({'key_dim': 64, 'value_dim': 512, 'hidden_dim': 64, 'precision': mode}, None)
    net.use_graphs = False
    net.fused_tail_min_pixels = net.fused_bottleneck_min_pixels = 0
    net.to('cuda').eval()
    net.load_weights(sd)
    fr = torch.from_numpy(synthetic_frames(1, 96, 128)).cuda()
    mk = torch.from_numpy(synthetic_masks(1, 2, 96, 128)).cuda()
    img4 = ops.pack_image(fr[0], 96, 128, 0, 0)
    key, shr, sel, f16, f8, f4 = net.encode_key_nhwc(img4, True, True)
    hidden = (act(2, 6, 8, 64, seed=5) * 0.3)
    value, hidden = net.encode_value_nhwc(img4, f16, hidden, mk[0], True)
    cat16 = net.new_decoder_input(2, 6, 8, f16.device)
    ops.copy_channels(act(2, 6, 8, 512, seed=6), cat16, 1024)
    net.segment_nhwc(f16, f8, f4, cat16, hidden, (96, 128), (0, 0), h_out=True)
    torch.cuda.synchronize()
    descs = lambda c: [a for arg in c['args'] for a in (arg if isinstance(arg, list) else [arg]) if isinstance(a, dict)]
    short = [[c['symbol'], c['keys'], [[d['plan_tile'], d['plan_splitk']] for d in descs(c)]] for c in t.calls]
    t.calls = []
    return short


SCENARIOS = {f.__name__: f for f in (plain, plain_explicit_plans, stem_pointwise_gemv, half, split_and_fp16w, dilated, shared,
                                     deferred_and_folded, shared_fallbacks, pair, mask_head, tabled)}
NETWORK_MODES = ('fp32', 'fp16', 'fp32x', 'fp16w')


# ---- the test --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def first_difference(got, want, path=''):
    if type(got) is not type(want):
        return f'{path}: {got!r} != {want!r}'
    if isinstance(got, dict):
        for k in sorted(set(got) | set(want)):
            if k not in got or k not in want:
                return f'{path}/{k}: only in the ' + ('golden' if k in want else 'trace')
            d = first_difference(got[k], want[k], f'{path}/{k}')
            if d:
                return d
        return None
    if isinstance(got, list):
        if len(got) != len(want):
            return f'{path}: {len(got)} entries, the golden has {len(want)}'
        for i, (a, b) in enumerate(zip(got, want)):
            d = first_difference(a, b, f'{path}[{i}]')
            if d:
                return d
        return None
    return None if got == want else f'{path}: {got!r} != {want!r}'


@pytest.mark.parametrize('name', list(SCENARIOS))
def test_front_end_hands_the_library_what_it_did(name, golden, monkeypatch):
    got = trace(monkeypatch, SCENARIOS[name])
    assert got['calls'], 'the proxy saw no call'
    assert got == golden[name], first_difference(got, golden[name], name)


@pytest.mark.parametrize('mode', NETWORK_MODES)
def test_network_pass_issues_the_same_calls_under_the_same_plans(mode, golden, monkeypatch, synth_sd):
    got = trace(monkeypatch, network, synth_sd, mode)
    assert len(got['extra']) > 50
    assert got == golden['network_' + mode], first_difference(got, golden['network_' + mode], 'network_' + mode)
