"""Tensor-level wrappers over the C-ABI kernels.

Everything here takes / returns torch CUDA tensors in the kernels' native layouts (NHWC activations
``[B,H,W,C]``, row-major memory rows ``[N,C]``) and launches on torch's current HIP stream.
torch is plumbing only: allocation, streams.  No torch compute op is used on the product path.
"""
import contextlib
import ctypes as C
import math
import os
import threading

import torch

from . import _lib, conv_plan
from .pil_resize import MAX_SIDE, taps
from ._lib import AffinityHint, CompactArena, ConvDesc, KeySegment, ValueSegment, check, load, ptr, stream_ptr

_workspaces = {}
_retired = {}                  # key -> outgrown buffers that captured HIP graphs may still point into
_tls = threading.local()       # .suffix: scratch scope of the calling thread (see ws_scope)
_scope_free, _scope_next = [], [0]


def new_scope():
    """Small recycled integer naming one owner of scoped scratch (an XMem instance: its side-stream key-encoder stages).
    `release_scope` drops every workspace of the scope when the owner dies, so a process that builds one network per video
    (run_on_video, launch.py) does not keep ~100 MB of conv scratch per dead network."""
    if _scope_free:
        return _scope_free.pop()
    _scope_next[0] += 1
    return _scope_next[0]


@contextlib.contextmanager
def ws_scope(suffix):
    """Kernels launched inside take their scratch from buffers tagged `suffix` (per host thread, nestable): stages that may
    run concurrently with the main stream (the side-stream key encoder) never share scratch with it."""
    prev = getattr(_tls, 'suffix', '')
    _tls.suffix = suffix
    try:
        yield
    finally:
        _tls.suffix = prev


def release_scope(scope):
    mark = f'#{scope}#'
    for d in (_workspaces, _retired):
        for key in [k for k in d if mark in k[1]]:
            del d[key]
    _scope_free.append(scope)

# Optional live kernel timing for bench.py.  RECORD = [] makes conv2d / affinity_topk append a re-launchable
# closure for every call of one (eager) frame; time_recorded() then times each distinct launch back to back between
# two HIP events (torch events record on the current stream, which is the stream every kernel here is launched on).
RECORD = None
# EVENT_TAP = [] makes the memory-readout launches (which stay eager between the captured stages) bracket themselves with
# HIP events ON THEIR LAUNCH STREAM inside whatever region is running - bench.py's instrumented pass of the timed region.
EVENT_TAP = None


def _tap_begin():
    if EVENT_TAP is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _tap_end(kind, e0, flop):
    if e0 is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        EVENT_TAP.append((kind, e0, e1, flop))


def eager_only():
    return RECORD is not None


def time_recorded(records, reps=10):
    """{kind: {ms, flop, launches}} for ONE frame: sum over the frame's launches of the average duration of that
    launch (measured over `reps` back-to-back repetitions)."""
    groups = {}
    for kind, key, flop, fn, keep in records:
        g = groups.setdefault((kind, key), [0, flop, fn, keep])
        g[0] += 1
    out = {}
    for (kind, key), (count, flop, fn, keep) in groups.items():
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        d = out.setdefault(kind, dict(ms=0.0, flop=0.0, launches=0))
        d['ms'] += e0.elapsed_time(e1) / reps * count
        d['flop'] += flop * count
        d['launches'] += count
    return out


def workspace(nbytes, device, tag='default'):
    """Grow-only scratch buffer per (device, tag + scope suffix); kernels on one stream run in order so reuse is safe.
    The scope suffix (`ws_scope`, entered by XMem around its side-stream key-encoder stages, unique per network instance and
    graph slot) keeps concurrently running streams on separate scratch.
    CONTRACT: one host thread drives this module per process (as the reference's InferenceCore is single-threaded).
    The scope suffix is thread-local, but the precision mode (`ops.precision`) is a process-wide switch and un-scoped scratch
    ('conv', 'affinity', 'augment', ... without a scope) is shared per device by every caller on every stream: two host threads
    calling into ops concurrently would clobber each other's mode and scratch.  Run one process per stream of videos (launch.py)."""
    key = (str(device), tag + getattr(_tls, 'suffix', ''))      # kernels on a side stream get their own scratch
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _retired.setdefault(key, []).append(buf)   # captured HIP graphs may still hold the old pointer: kept while the scope lives
        grow = max(int(nbytes), 2 * (buf.numel() if buf is not None else 0), 1 << 20)
        buf = torch.empty(grow, dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def _req(t, name, half_ok=False):
    if not t.is_cuda:
        raise RuntimeError(f'{name}: expected a CUDA (HIP) tensor - xmem2_amd has no CPU path')
    if t.dtype != torch.float32 and not (half_ok and t.dtype == torch.float16):
        raise RuntimeError(f'{name}: expected float32' + (' or float16' if half_ok else ''))
    return t


def _h(t):
    """storage flag of the `_t` entry points: 1 = IEEE half, 0 = float"""
    return int(t.dtype == torch.float16)


# Arithmetic mode of the 3x3 / stride-1 convolutions.  'fp32' (default, the parity contract) or 'fp16': OPT-IN reduced
# precision - the Winograd-domain operands are rounded to fp16 and multiplied on the fp16 MFMA with fp32 accumulation (the
# counterpart of the reference's autocast loop, inference/run_on_video.py:76).  Set per call tree by XMem (`precision`).
_PRECISION = 'fp32'
_DRIVER = threading.RLock()          # held while a thread is inside `precision` (a network stage): see precision.__enter__
# held while a stage is being captured into a HIP graph, and by helper threads around calls the runtime forbids while ANY thread captures
# (torch captures in the 'global' error mode): pinning host memory makes the pinned allocator query its events, which invalidates a capture
# in progress on another thread (hipErrorStreamCaptureInvalidated).  Captures are rare (once per stage and shape), so nobody waits long.
CAPTURE_LOCK = threading.Lock()
PRECISIONS = ('fp32', 'fp16', 'fp16w', 'fp32x')
# 'fp16' (opt-in): THE FP16 LOOP - the counterpart of the reference's GPU mode (torch.cuda.amp.autocast around the frame loop,
# inference/run_on_video.py:76; fp32 preload :59-66): activations are IEEE halfs in HBM, every convolution contracts half
# operands on v_mfma_f32_32x32x16_f16 in the direct form with fp32 accumulation and an fp32 epilogue, elementwise kernels
# compute in fp32 on half storage; stems, key projection output, memory (keys, values, readout weights), GRU state, logits and
# probabilities stay fp32.  'fp16w' is round 2's experiment (only the F(2x2) Winograd-domain operands in fp16), kept runnable.
# 'fp32x' (opt-in, separately reported): SPLIT-OPERAND arithmetic - every fp32 operand of every GEMM-shaped convolution is
# carried as two halfs (x = hi + lo, <= 2^-21 relative) and the four partial products run on v_mfma_f32_32x32x16_f16 with fp32
# accumulation (csrc/conv_mfma.hip, SPLIT kernels).  Same tensors, same bytes, fp32-class results; 1/4 of the fp32 MFMA cycles.


def act_dtype():
    """Storage type of the activations the network allocates in the current mode: halfs in the fp16 loop, floats otherwise."""
    return torch.float16 if _PRECISION == 'fp16' else torch.float32


class precision:
    def __init__(self, mode):
        if mode not in PRECISIONS:
            raise ValueError(f'unknown precision {mode!r} ({" | ".join(PRECISIONS)})')
        self.mode = mode

    def __enter__(self):
        global _PRECISION
        # the mode is a process-wide switch and un-scoped scratch is shared per device: ONE host thread may be inside a network stage
        # at a time (the reference's InferenceCore is single-threaded too).  A second thread entering concurrently is a
        # contract violation and fails loudly instead of silently flipping the other thread's arithmetic mode; the same thread
        # may nest, and different threads may take turns.  InferenceCore's public calls (step, prefetch_keys, put_*) hold the same
        # lock for their WHOLE duration with a blocking acquire (inference_core._on_network_device), replays and eager readout
        # included: threads that drive cores of one process are serialised call by call; only a thread that calls into `ops` /
        # XMem stages directly while another is inside one trips this check.
        if not _DRIVER.acquire(blocking=False):
            raise RuntimeError('xmem2_amd.ops: another host thread is inside a network stage - one thread drives the kernels of a process at a '
                               'time (run one process per stream of videos, xmem2_amd.launch)')
        self.prev, _PRECISION = _PRECISION, self.mode

    def __exit__(self, *exc):
        global _PRECISION
        _PRECISION = self.prev
        _DRIVER.release()


class ConvWeights:
    """Device-resident convolution parameters in kernel layout: w [Cout][KH][KW][Cin_pad], scale, shift."""
    __slots__ = ('w', 'scale', 'shift', 'cout', 'cin', 'kh', 'kw', 'stride', 'pad', 'cin_true', 'wu', 'wu_f16', 'wu4',
                 'sp_shift', 'scale_sp', 'w_sp', 'wu_sp', 'wu4_sp', 'w_h', 'dilation')

    def __init__(self, w, scale, shift, stride, pad, cin_true=None, winograd=True, dilation=1):
        self.w, self.scale, self.shift = w, scale, shift
        self.cout, self.kh, self.kw, self.cin = w.shape
        self.stride, self.pad = stride, pad
        self.dilation = dilation         # > 1: conv2d runs the dilated direct form (xmem_conv2d_nhwc_dilated)
        winograd = winograd and dilation == 1
        self.cin_true = cin_true if cin_true is not None else self.cin     # un-padded Cin (algorithmic FLOPs)
        self.wu = None
        self.wu_f16 = None
        self.wu4 = None                  # F(4x4,3x3) operand, built on first use (only the large layers take that path)
        self.sp_shift = None             # 'fp32x' mode only: split operands (built on first use), see ensure_split
        self.scale_sp = self.w_sp = self.wu_sp = self.wu4_sp = None
        self.w_h = None                  # 'fp16' loop: the weights as halfs [Cout][KH][KW][Cin pad 8], built on first use (half())
        if winograd and self.kh == 3 and self.kw == 3 and stride == 1 and pad == 1 and self.cin % 32 == 0 \
                and self.cout % 4 == 0 and self.cout >= 32:
            self.wu = winograd_weights(w)
            if self.cin % 64 == 0:
                self.wu_f16 = self.wu.to(torch.float16).contiguous()      # reduced-precision mode only


    def half(self):
        """[Cout][KH][KW][Cin'] IEEE halfs, Cin' = Cin padded to a multiple of 8 with zero channels (a 16-byte operand chunk is 8
        halfs); rounded once to nearest even, as autocast casts fp32 weights."""
        if self.w_h is None:
            w = self.w
            if w.shape[3] % 8:
                w = torch.nn.functional.pad(w, (0, 8 - w.shape[3] % 8))
            self.w_h = w.to(torch.float16).contiguous()
        return self.w_h

    def ensure_split(self):
        """Split-operand forms of the weights for the 'fp32x' mode: every array the kernels may contract (direct, F(2x2), F(4x4))
        times ONE power of two 2^s per layer (so that the low halves stay in fp16's normal range), each group of four input
        channels stored as [hi x 4 | lo x 4] halfs; `scale_sp` = scale * 2^-s undoes the factor exactly in the epilogue."""
        if self.sp_shift is None:
            forms = [t for t in (self.w, self.wu, self.wu4) if t is not None]
            amax = max(float(t.abs().max()) for t in forms)
            s = 0 if not (amax > 0 and math.isfinite(amax)) else max(-8, min(24, int(math.floor(math.log2(1024.0 / amax)))))
            self.sp_shift = s
            self.scale_sp = (self.scale * (2.0 ** -s)).contiguous()
            self.w_sp = split_pack(self.w, s)
            self.wu_sp = split_pack(self.wu, s) if self.wu is not None else None
        if self.wu4 is not None and self.wu4_sp is None:
            if float(self.wu4.abs().max()) * 2.0 ** self.sp_shift > 3.0e4:      # built after the shift was chosen and larger than planned
                raise RuntimeError('split operand out of the fp16 range: build the F(4x4) operand before ensure_split()')
            self.wu4_sp = split_pack(self.wu4, self.sp_shift)


def split_pack(w, shift=0):
    """float32 [..., C] (C % 4 == 0) -> float16 [..., 2C]: per four channels [hi0..hi3 | lo0..lo3] of w * 2^shift, hi = the
    nearest half, lo = the nearest half of the remainder (|w 2^shift - hi - lo| <= 2^-22 |w 2^shift| or 3e-8 absolute)."""
    ws = w.float() * (2.0 ** shift)
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    c = w.shape[-1]
    hi4 = hi.reshape(*w.shape[:-1], c // 4, 4)
    lo4 = lo.reshape(*w.shape[:-1], c // 4, 4)
    return torch.cat([hi4, lo4], -1).reshape(*w.shape[:-1], 2 * c).contiguous()


_WINO_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])


# F(4x4,3x3) with the interpolation points {0, +-3/4, +-3/2, inf} (csrc/conv_winograd.hip: why, and what the transforms look like).
# Row i of G = (1, p_i, p_i^2) / N_i with N_i = prod_{k != i} (p_i - p_k) over the finite points; the row of infinity is (0, 0, 1).
def _wino4_g(a=0.75, b=1.5):
    from fractions import Fraction as Fr
    a, b = Fr(a), Fr(b)
    na, nb = 2 * a * a * (a * a - b * b), 2 * b * b * (b * b - a * a)
    rows = [[1 / (a * a * b * b), 0, 0], [1 / na, a / na, a * a / na], [1 / na, -a / na, a * a / na],
            [1 / nb, b / nb, b * b / nb], [1 / nb, -b / nb, b * b / nb], [0, 0, 1]]
    return torch.tensor([[float(v) for v in r] for r in rows], dtype=torch.float64)       # exact rationals rounded once to fp64


_WINO4_G = _wino4_g()


def winograd4_weights(w):
    """[Cout][3][3][Cin] -> G g G^T of F(4x4,3x3) as [36][Cout][Cin] (load-time, formed in fp64 and rounded once to fp32)."""
    g = _WINO4_G.to(w.device)
    u = torch.einsum('ia,nabc,jb->ijnc', g, w.double(), g)
    return u.reshape(36, w.shape[0], w.shape[3]).to(torch.float32).contiguous()


def winograd_weights(w):
    """[Cout][3][3][Cin] -> G g G^T as [16][Cout][Cin] (load-time, fp32; F(2x2,3x3) of Lavin & Gray)."""
    g = _WINO_G.to(w.device)
    u = torch.einsum('ia,nabc,jb->ijnc', g, w, g)
    return u.reshape(16, w.shape[0], w.shape[3]).contiguous()


# ---- convolutions ---------------------------------------------------------------------------------------------
# Which plan (tile / algorithm / split-K) a call runs under is decided in conv_plan.py: plan tables, tuner, heuristic.
class ConvCall:
    """One prepared convolution, built once per call from keyword arguments (conv2d's, under its names): the operands, the epilogue, the
    descriptor `d` handed to the library, and what is derived from them exactly once - the geometry, `wino_ok`, the plan key (the string
    that indexes conv_plans*.json and names the RECORD entry) and the plan.  Every entry point below builds its calls from this.
    `dilation` None: the plain entry point, with the operands of the precision mode and the plan of conv_plan.choose; an integer: the
    dilated direct form (`plan` as given, None = the library's heuristic; `flags` passed on).  `folded`: the residual arrives inside the
    output transform (conv2d_folded) - keyed and planned as the convolution with a residual that it is.  `alloc` False: a missing `out`
    stays None until `alloc_out`."""
    __slots__ = ('x', 'cin', 'ldin', 'cw', 'out', 'out_ld', 'out_dtype', 'res', 'res_ld', 'res_broadcast', 'relu_in', 'relu_out', 'dilation',
                 'flags', 'half', 'folded', 'precision', 'd', 'B', 'H', 'W', 'Ho', 'Wo', 'wino_ok', 'key', 'plan', 'need', 'ws')

    def __init__(self, *, x, cw, cin=None, in_ld=None, out=None, out_ld=None, out_dtype=torch.float32, res=None, res_ld=None, res_broadcast=False,
                 relu_in=False, relu_out=False, plan=None, half=False, folded=False, dilation=None, flags=0, alloc=True):
        B, H, W, dense_ld = x.shape
        cin, ldin = cw.cin if cin is None else cin, dense_ld if in_ld is None else in_ld
        self.x, self.cw, self.cin, self.ldin, self.out, self.out_dtype = x, cw, cin, ldin, out, out_dtype
        self.res, self.res_broadcast, self.relu_in, self.relu_out = res, res_broadcast, relu_in, relu_out
        self.dilation, self.flags, self.half, self.folded, self.precision = dilation, flags, half, folded, _PRECISION
        self.B, self.H, self.W, self.need, self.ws = B, H, W, 0, None            # need, ws: the workspace `run` takes
        dil = 1 if dilation is None else dilation
        self.Ho = (H + 2 * cw.pad - dil * (cw.kh - 1) - 1) // cw.stride + 1
        self.Wo = (W + 2 * cw.pad - dil * (cw.kw - 1) - 1) // cw.stride + 1
        out_ld = self.out_ld = cw.cout if out is None else out.shape[-1] if out_ld is None else out_ld
        d = self.d = ConvDesc()
        d.inp = x.data_ptr(); d.B, d.H, d.W, d.Cin, d.ldin = B, H, W, cin, ldin
        d.w = cw.w.data_ptr(); d.Cout, d.KH, d.KW, d.stride, d.pad = cw.cout, cw.kh, cw.kw, cw.stride, cw.pad
        d.scale = cw.scale.data_ptr(); d.shift = cw.shift.data_ptr()
        d.res = res.data_ptr() if res is not None else None
        # `res_ld`: the residual is a channel slice of a wider buffer; `res_broadcast`: res [1,Ho,Wo,C] added to every batch element
        self.res_ld = d.ldres = 0 if res is None else res_ld if res_ld is not None else res.shape[-1]
        d.res_broadcast = int(bool(res_broadcast and res is not None))
        d.out = out.data_ptr() if out is not None else None; d.ldout = out_ld
        d.relu_in, d.relu_out = int(relu_in), int(relu_out)
        self.wino_ok = out_ld % 4 == 0 and d.ldres % 4 == 0
        key = f'{B}x{H}x{W}x{cin}/{ldin}->{cw.cout}/{out_ld} k{cw.kh}s{cw.stride}p{cw.pad}{"" if dilation is None else f"d{dilation}"} ' \
              f'r{int(res is not None or folded)}{int(relu_in)}{int(relu_out)}'
        self.key = f'h{key}o{int(out_dtype == torch.float16)}' if half else key
        if alloc and out is None:
            self.alloc_out()
        if dilation is None:
            self.plan = conv_plan.choose(load(), self, self._mode_operands(plan))
        else:
            self.plan = tuple(plan) if plan is not None else (conv_plan.HEURISTIC, 0)
        d.plan_tile, d.plan_splitk = self.plan

    def _mode_operands(self, plan):
        """Point the descriptor at the operands of the precision mode -> `plan`, or the plan the 'fp16w' mode puts in its place."""
        d, cw = self.d, self.cw
        if self.half:
            d.in_half, d.out_half, d.w_half = 1, int(self.out_dtype == torch.float16), cw.half().data_ptr()
            return plan
        d.w_winograd = cw.wu.data_ptr() if cw.wu is not None else None
        if self.precision == 'fp16w' and cw.wu_f16 is not None and plan is None and self.wino_ok:
            d.w_winograd_f16 = cw.wu_f16.data_ptr()
            plan = (conv_plan.F2_F16, 1)         # the library falls back to the fp32 Winograd tile if its own conditions fail
        if self.precision == 'fp32x' and cw.cout > 1:
            # split-operand arithmetic for every GEMM-shaped path (the Cout = 1 mask head is a GEMV on the fp32 VALU)
            if cw.sp_shift is None or (cw.wu4 is not None and cw.wu4_sp is None):
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError('conv2d: split operands must be built before graph capture (run the stage eagerly once)')
                if cw.sp_shift is None and cw.wu is not None and cw.wu4 is None:
                    cw.wu4 = winograd4_weights(cw.w)          # so that ONE power of two covers every form of this layer
                cw.ensure_split()
            d.arith = 1
            d.w_split = cw.w_sp.data_ptr()
            d.w_winograd_split = cw.wu_sp.data_ptr() if cw.wu_sp is not None else None
            d.w_winograd4_split = cw.wu4_sp.data_ptr() if cw.wu4_sp is not None else None    # taken only by an F(4x4) plan
            d.scale = cw.scale_sp.data_ptr()
        return plan

    def f4_operand(self):
        """Point the descriptor at the F(4x4,3x3) operand of the weights (and at its split form in 'fp32x'), built on first use."""
        d, cw = self.d, self.cw
        if cw.wu4 is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('conv2d: the F(4x4) operand must be built before graph capture (run the stage eagerly once)')
            cw.wu4 = winograd4_weights(cw.w)
        d.w_winograd4 = cw.wu4.data_ptr()
        if d.arith == 1:
            cw.ensure_split()
            d.w_winograd4_split = cw.wu4_sp.data_ptr()

    def alloc_out(self):
        """A fresh output buffer of the convolution's own shape (the caller gave none), entered into the descriptor -> out."""
        self.out = torch.empty((self.B, self.Ho, self.Wo, self.cw.cout), dtype=self.out_dtype, device=self.x.device)
        self.d.out = self.out.data_ptr()
        return self.out

    def workspace_bytes(self):
        lib, d = load(), C.byref(self.d)
        return lib.xmem_conv2d_workspace_bytes(d) if self.dilation is None else lib.xmem_conv2d_dilated_workspace_bytes(d, self.dilation)

    def launch(self):
        """The plain or the dilated entry point on the current stream, with the workspace `run` took: re-launchable -> status."""
        if self.dilation is None:
            return load().xmem_conv2d_nhwc(C.byref(self.d), ptr(self.ws), self.need, stream_ptr())
        return load().xmem_conv2d_nhwc_dilated(C.byref(self.d), self.dilation, self.flags, ptr(self.ws), self.need, stream_ptr())

    def run(self):
        """Output buffer, workspace, launch, and the RECORD entry -> out."""
        if self.out is None:
            self.alloc_out()
        self.need = self.workspace_bytes()
        self.ws = workspace(self.need, self.x.device, 'conv') if self.need else None
        check(self.launch())
        if RECORD is not None:
            self.record(self.launch)
        return self.out

    def record(self, launch):
        """The RECORD entry of this convolution, `launch` being what runs it again (bench.py and tools/*_table.py read the entries)."""
        cw, plan = self.cw, self.plan
        info = dict(dilation=self.dilation) if self.dilation is not None else \
            dict(relu_in=bool(self.relu_in), relu_out=bool(self.relu_out), in_ld=self.ldin, cin=self.cin, out_ld=self.out_ld,
                 res_broadcast=bool(self.res_broadcast), plan=tuple(plan),
                 executed_mfma_flops=conv_plan.executed_mfma_flops(self.B, self.Ho, self.Wo, self.cin, cw.cout, cw.kh, cw.kw, cw.stride, cw.pad,
                                                                   plan[0], bool(self.d.w_winograd) and self.wino_ok, half=self.half))
        RECORD.append(('conv', self.key, 2.0 * self.B * self.Ho * self.Wo * cw.cout * cw.kh * cw.kw * cw.cin_true, launch,
                       (self.x, self.out, self.res, cw, self.ws, info)))


def _conv2d_half(x, cw, *, out, out_ld, res, relu_in, relu_out, in_ld, cin, plan, res_broadcast, out_dtype):
    """The fp16 loop's convolution: x [B,H,W,C] halfs (pixel stride in_ld halfs), half weights, direct implicit GEMM on the fp16
    MFMA, fp32 accumulation + epilogue; output (and residual) halfs, or float32 with out_dtype=torch.float32 (key projection,
    mask head).  Input channels beyond the layer's own (a buffer padded to a multiple of 8) must be zero: the half weights are
    zero there."""
    ldin = in_ld if in_ld is not None else x.shape[3]
    cin_h = cw.half().shape[3]                            # the layer's Cin padded to 8
    cin = cin if cin is not None else cin_h
    if cin != cin_h and cin != cw.cin:
        raise RuntimeError(f'conv2d (half): weight expects Cin={cw.cin} (padded {cin_h}), got {cin}')
    if cin_h > ldin:
        raise RuntimeError(f'conv2d (half): the input buffer has {ldin} channels per pixel, the layer reads {cin_h} (pad to a multiple of 8)')
    if in_ld is not None:
        # a channel SLICE of a wider buffer: the kernel reads cin_h (= Cin padded to 8) halfs from the slice start whatever `cin` says,
        # and only the zero WEIGHTS mask the tail - 0 x Inf/NaN from a neighbouring slice or an uninitialised tail would be NaN.
        # So a slice must be a whole number of 8-half groups and must end inside its pixel (include/xmem_hip.h, xmem_conv_desc.in_half).
        # (A whole, zero-padded buffer - in_ld None - is not a slice: its padding channels are the caller's zeros.)
        if cin % 8 != 0:
            raise RuntimeError(f'conv2d (half): a channel slice must hold a multiple of 8 channels, got cin={cin} '
                               '(pad the slice and zero-fill the padding channels)')
        base = x._base
        if base is not None and base.dim() == 4 and base.shape[3] == ldin and base.is_contiguous():
            # offset of the slice inside its pixel, measured from the PARENT buffer (which may itself sit anywhere in a workspace)
            inpix = (x.storage_offset() - base.storage_offset()) % ldin
            if inpix + cin_h > ldin:
                raise RuntimeError(f'conv2d (half): the slice [{inpix}, +{cin_h}) crosses the pixel stride {ldin}')
    odt = out_dtype if out_dtype is not None else (out.dtype if out is not None else torch.float16)
    if out is not None and out.dtype != odt:
        raise RuntimeError('conv2d (half): out buffer dtype does not match out_dtype')
    if res is not None and res.dtype != odt:
        raise RuntimeError('conv2d (half): the residual must have the output storage type')
    return ConvCall(x=x, cw=cw, cin=cin_h, in_ld=ldin, out=out, out_ld=out_ld, out_dtype=odt, res=res, res_broadcast=res_broadcast,
                    relu_in=relu_in, relu_out=relu_out, plan=plan, half=True).run()


def conv2d(x, cw, out=None, out_ld=None, res=None, relu_in=False, relu_out=False, in_ld=None, cin=None, plan=None,
           res_broadcast=False, out_dtype=None, res_ld=None):
    """x [B,H,W,C] NHWC (or any buffer whose pixel stride is `in_ld`) -> out [B,Ho,Wo,Cout].  `res_ld`: the pixel stride of a residual
    that is a channel slice of a wider buffer (fp32 direct and Winograd forms; default: its last dimension)."""
    _req(x, 'conv2d input', half_ok=True)
    if res_ld is not None and res is not None and res_ld != res.shape[-1] and (x.dtype == torch.float16 or cw.dilation != 1):
        raise RuntimeError('conv2d: a residual with its own pixel stride is taken by the fp32, dilation-1 forms only')
    if x.dtype == torch.float16:
        return _conv2d_half(x, cw, out=out, out_ld=out_ld, res=res, relu_in=relu_in, relu_out=relu_out, in_ld=in_ld, cin=cin, plan=plan,
                            res_broadcast=res_broadcast, out_dtype=out_dtype)
    if out_dtype is not None and out_dtype != torch.float32:
        raise RuntimeError('conv2d: a float32 input gives a float32 output (the fp16 loop converts at the max-pool after the stems)')
    if cw.dilation != 1:
        if res_broadcast:
            raise RuntimeError('conv2d: a dilated convolution takes no broadcast residual')
        return conv2d_dilated(x, cw, out=out, out_ld=out_ld, res=res, relu_in=relu_in, relu_out=relu_out, in_ld=in_ld, cin=cin, plan=plan)
    if cin is not None and cin != cw.cin:
        raise RuntimeError(f'conv2d: weight expects Cin={cw.cin}, got {cin}')
    return ConvCall(x=x, cw=cw, in_ld=in_ld, out=out, out_ld=out_ld, res=res, res_ld=res_ld, res_broadcast=res_broadcast,
                    relu_in=relu_in, relu_out=relu_out, plan=plan).run()


# ---- shared Winograd transforms (include/xmem_hip.h: SHARED WINOGRAD TRANSFORMS) -------------------------------------------------
# conv2d_shared: sibling convolutions of one tensor behind ONE input transform; conv2d_folded: a deferred sibling finished inside the
# output transform of the convolution it is the residual of.  Both give the bits of the separate conv2d calls under the same plans,
# and both fall back to exactly those calls where the library declines (a plan that is not F(4x4), the half / split modes) - and
# while RECORD is on, so that bench.py's per-layer survey times every convolution as its own re-launchable call.
SHARED_STATS = {'shared_input': 0, 'folded': 0, 'separate': 0}      # calls that took the shared kernels / calls issued one by one


class DeferredConv:
    """A convolution of `conv2d_shared` that stopped after its position GEMMs: its call and its M, for `conv2d_folded`."""
    __slots__ = ('call', 'm', 'm_bytes')

    def __init__(self, call, m, m_bytes):
        self.call, self.m, self.m_bytes = call, m, m_bytes

    def finish(self):
        """The convolution's own output transform (the fold did not apply) -> its output tensor."""
        out = self.call.alloc_out()
        check(load().xmem_conv2d_output_from_m(C.byref(self.call.d), ptr(self.m), self.m_bytes, stream_ptr()))
        return out


def conv2d_shared(x, convs, in_ld=None, cin=None, defer=None):
    """x as for conv2d; convs: 2 or 3 dicts of conv2d's keyword arguments, each with its weights under 'cw' (3x3, stride 1, the same
    Cin).  -> the list of outputs.  `defer` (an index): that convolution may stop after its GEMMs and come back as a DeferredConv
    (which only `conv2d_folded` takes) instead of a tensor."""
    _req(x, 'conv2d_shared input', half_ok=True)
    separate = lambda: [conv2d(x, in_ld=in_ld, cin=cin, **kw) for kw in convs]
    if x.dtype != torch.float32 or _PRECISION != 'fp32' or RECORD is not None or not 2 <= len(convs) <= _lib.CONV_SHARED_MAX \
            or any(kw['cw'].dilation != 1 or kw.get('out_dtype') not in (None, torch.float32) for kw in convs):
        SHARED_STATS['separate'] += 1
        return separate()
    lib = load()
    calls = []
    for kw in convs:
        cw = kw['cw']
        if cin is not None and cin != cw.cin:
            raise RuntimeError(f'conv2d_shared: weight expects Cin={cw.cin}, got {cin}')
        calls.append(ConvCall(x=x, cw=cw, in_ld=in_ld, out=kw.get('out'), out_ld=kw.get('out_ld'), res=kw.get('res'),
                              res_broadcast=kw.get('res_broadcast', False), relu_in=kw.get('relu_in', False),
                              relu_out=kw.get('relu_out', False), plan=kw.get('plan'), alloc=False))
    n = len(calls)
    descs = (C.POINTER(ConvDesc) * n)(*[C.pointer(c.d) for c in calls])
    for c in calls:
        if c.out is None:
            c.d.out = x.data_ptr()       # a placeholder: the size query reads no `out`; a descriptor without one is invalid
    need = lib.xmem_conv2d_shared_input_workspace_bytes(descs, n)
    if not need:
        SHARED_STATS['separate'] += 1
        return separate()
    outs = []
    dm, dmb = (C.c_void_p * n)(), (C.c_size_t * n)()
    for i, c in enumerate(calls):
        if i == defer and c.out is None:
            m_bytes = lib.xmem_conv2d_m_bytes(C.byref(c.d))
            m = workspace(m_bytes, x.device, 'conv_m')       # a buffer of its own: the convolutions in between reuse 'conv'
            dm[i], dmb[i] = m.data_ptr(), m_bytes
            c.d.out = m.data_ptr()                           # never written
            outs.append(DeferredConv(c, m, m_bytes))
        else:
            outs.append(c.out if c.out is not None else c.alloc_out())
    ws = workspace(need, x.device, 'conv')
    check(lib.xmem_conv2d_shared_input(descs, n, dm, dmb, ptr(ws), need, stream_ptr()))
    SHARED_STATS['shared_input'] += 1
    return outs


def conv2d_folded(x, cw, branch, out=None, out_ld=None, relu_in=False, relu_out=False, plan=None):
    """conv2d(x, cw, res=branch) where `branch` is what conv2d_shared returned for its `defer` convolution: a DeferredConv, whose output
    transform is then formed inside this convolution's (one launch, the branch result never stored), or already a tensor."""
    if not isinstance(branch, DeferredConv):
        return conv2d(x, cw, out=out, out_ld=out_ld, res=branch, relu_in=relu_in, relu_out=relu_out, plan=plan)
    _req(x, 'conv2d_folded input')
    call = ConvCall(x=x, cw=cw, out=out, out_ld=out_ld, relu_in=relu_in, relu_out=relu_out, plan=plan, folded=True)
    need = call.workspace_bytes()
    ws = workspace(need, x.device, 'conv') if need else None
    rc = load().xmem_conv2d_nhwc_folded(C.byref(call.d), C.byref(branch.call.d), ptr(branch.m), branch.m_bytes, ptr(ws), need, stream_ptr())
    if rc == _lib.UNSUPPORTED:
        SHARED_STATS['separate'] += 1
        return conv2d(x, cw, out=call.out, out_ld=call.out_ld, res=branch.finish(), relu_in=relu_in, relu_out=relu_out, plan=call.plan)
    check(rc)
    SHARED_STATS['folded'] += 1
    return call.out


# ---- bottleneck pair (include/xmem_hip.h: BOTTLENECK PAIR) -----------------------------------------------------------------------
# conv2d_pointwise_pair: a bottleneck's expand 1x1 (+ residual, relu) and the next block's reduce 1x1 (relu) in one launch; the bits of
# the two conv2d calls under the same plans, and exactly those calls wherever the library declines, outside fp32 and while RECORD is on.
PAIR_STATS = {'pair': 0, 'separate': 0}          # calls that took the pair kernel / calls issued as two convolutions


def _pixel_strided(t):
    """(tensor, pixel stride) of a residual: a channel slice of a dense NHWC buffer is read in place, any other view is copied once."""
    B, H, W, Cc = t.shape
    ld = t.stride(2)
    if t.stride(3) == 1 and ld >= Cc and t.stride(1) == W * ld and t.stride(0) == H * W * ld:
        return t, ld
    t = t.contiguous()
    return t, Cc


def conv2d_pointwise_pair(o, cw_expand, res, cw_reduce, y=None, y_ld=None, z=None, z_ld=None, in_ld=None, plans=(None, None),
                          res_broadcast=False):
    """o [B,H,W,Cmid] (pixel stride `in_ld`), res [B,H,W,4 Cmid] (fp32: a channel slice of a wider buffer is read in place) ->
    y = relu(conv1x1(o, cw_expand) + res) [B,H,W,4 Cmid], z = relu(conv1x1(y, cw_reduce)) [B,H,W,Cmid'].  `y` / `z` with `y_ld` / `z_ld`:
    output buffers and their pixel strides, as conv2d's `out` / `out_ld`; `plans`: conv2d's `plan` of the two layers; `res_broadcast` as
    in conv2d (always two launches)."""
    _req(o, 'conv2d_pointwise_pair input', half_ok=True)
    res_ld = None
    if res is not None and o.dtype == torch.float32 and res.dim() == 4:
        res, res_ld = _pixel_strided(res)
    fusable = o.dtype == torch.float32 and _PRECISION == 'fp32' and RECORD is None and res is not None and res.dtype == torch.float32 \
        and not res_broadcast and all(cw.dilation == 1 and cw.stride == 1 for cw in (cw_expand, cw_reduce))
    if not fusable:
        PAIR_STATS['separate'] += 1
        yy = conv2d(o, cw_expand, out=y, out_ld=y_ld, res=res, relu_out=True, in_ld=in_ld, plan=plans[0], res_broadcast=res_broadcast,
                    res_ld=res_ld)
        zz = conv2d(yy, cw_reduce, out=z, out_ld=z_ld, relu_out=True, in_ld=y_ld, plan=plans[1])
        return yy, zz
    e = ConvCall(x=o, cw=cw_expand, in_ld=in_ld, out=y, out_ld=y_ld, res=res, res_ld=res_ld, relu_out=True, plan=plans[0])
    r = ConvCall(x=e.out, cw=cw_reduce, in_ld=e.out_ld, out=z, out_ld=z_ld, relu_out=True, plan=plans[1])
    rc = load().xmem_conv2d_pointwise_pair(C.byref(e.d), C.byref(r.d), stream_ptr())
    if rc == _lib.UNSUPPORTED:
        # (e.out / r.out were allocated above when the caller gave none: the separate calls fill the same buffers)
        PAIR_STATS['separate'] += 1
        conv2d(o, cw_expand, out=e.out, out_ld=e.out_ld, res=res, relu_out=True, in_ld=in_ld, plan=plans[0], res_ld=res_ld)
        conv2d(e.out, cw_reduce, out=r.out, out_ld=r.out_ld, relu_out=True, in_ld=e.out_ld, plan=plans[1])
        return e.out, r.out
    check(rc)
    PAIR_STATS['pair'] += 1
    return e.out, r.out


def conv2d_dilated(x, cw, dilation=None, out=None, out_ld=None, res=None, relu_in=False, relu_out=False, in_ld=None, cin=None, plan=None,
                   tap_skip=True):
    """Dilated (atrous) convolution, fp32: x [B,H,W,C] NHWC (pixel stride `in_ld`) -> out [B,Ho,Wo,Cout], Ho = (H + 2 pad -
    dilation (KH - 1) - 1) / stride + 1.  `dilation` defaults to cw.dilation; `plan` = (tile 0..6, split-K) of the direct form (None:
    the library's heuristic); tap_skip=False keeps every tap (measurement only: the same bits)."""
    _req(x, 'conv2d_dilated input')
    dil = int(cw.dilation if dilation is None else dilation)
    if cin is not None and cin != cw.cin:
        raise RuntimeError(f'conv2d_dilated: weight expects Cin={cw.cin}, got {cin}')
    call = ConvCall(x=x, cw=cw, in_ld=in_ld, out=out, out_ld=out_ld, res=res, relu_in=relu_in, relu_out=relu_out, plan=plan,
                    dilation=dil, flags=0 if tap_skip else _lib.DILATED_NO_TAP_SKIP, alloc=False)
    if call.Ho <= 0 or call.Wo <= 0:
        raise RuntimeError(f'conv2d_dilated: empty output for a {call.H}x{call.W} input (pad {cw.pad}, dilation {dil})')
    return call.run()


_HIPRT = None


def masked_stream(device, n_cus, first=0):
    """A HIP stream whose kernels may only run on `n_cus` compute units (hipExtStreamCreateWithCUMask), wrapped for torch.
    The mask's bits are dealt round-robin over the 8 XCDs by the driver, so the low n_cus bits are n_cus / 8 CUs of every XCD.
    Measurement knob for the frame pipeline's side stream (XMEM_SIDE_CUS); the default stream of a core is unmasked."""
    global _HIPRT
    if _HIPRT is None:
        _HIPRT = C.CDLL('libamdhip64.so')
    words = (first + n_cus + 31) // 32
    mask = (C.c_uint32 * words)()
    for b in range(first, first + n_cus):
        mask[b // 32] |= (1 << (b % 32))
    st = C.c_void_p()
    with torch.cuda.device(device):
        rc = _HIPRT.hipExtStreamCreateWithCUMask(C.byref(st), C.c_uint32(words), mask)
    if rc != 0:
        raise RuntimeError(f'hipExtStreamCreateWithCUMask failed with status {rc}')
    return torch.cuda.ExternalStream(st.value, device=device)


def side_stream(device):
    """The stream `InferenceCore.prefetch_keys` runs the batched key encoder on."""
    n = int(os.environ.get('XMEM_SIDE_CUS', '0') or 0)
    return masked_stream(device, n) if n > 0 else torch.cuda.Stream(device=device)


def readout_stream(device):
    """The stream the early readout (the NEXT hinted frame's select + readout) runs on, under the current frame's decoder, at normal
    priority (high priority measured no faster: profiles/HISTORY.md step 26)."""
    return torch.cuda.Stream(device=device)


def trace_marker(tag=0):
    """Empty kernel `xmem_trace_marker_kernel` on the current stream: cuts a rocprofv3 kernel trace to a region."""
    check(load().xmem_trace_marker(int(tag), stream_ptr()))


# The elementwise wrappers take float32 or (the fp16 loop) float16 activations: the `_t` entry points carry the storage type of
# every tensor; outputs follow the input's type unless `out_dtype` says otherwise.
def maxpool3x3s2(x, out_dtype=None):
    B, H, W, Cc = x.shape
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), dtype=out_dtype or x.dtype, device=x.device)
    check(load().xmem_maxpool3x3s2_t(ptr(x), _h(x), ptr(out), _h(out), B, H, W, Cc, stream_ptr()))
    return out


def upsample2x_add(g, skip):
    B, h, w, Cc = g.shape
    if skip.dtype != g.dtype:
        raise RuntimeError('upsample2x_add: g and skip must share a storage type')
    out = torch.empty((B, 2 * h, 2 * w, Cc), dtype=g.dtype, device=g.device)
    check(load().xmem_upsample2x_add_t(ptr(g), ptr(skip), ptr(out), _h(g), B, h, w, Cc, stream_ptr()))
    return out


def area_downsample(x, r, out=None, out_ld=None, out_off=0, c=None, in_ld=None):
    B, H, W = x.shape[:3]
    c = c if c is not None else x.shape[3]
    in_ld = in_ld if in_ld is not None else x.shape[3]
    if out is None:
        out = torch.empty((B, H // r, W // r, c), dtype=x.dtype, device=x.device)
        out_ld = c
    check(load().xmem_area_downsample_t(ptr(x), _h(x), in_ld, C.c_void_p(out.data_ptr() + out.element_size() * out_off), _h(out), out_ld,
                                        B, H, W, c, r, stream_ptr()))
    return out


def copy_channels(src, dst, dst_off, c=None, src_off=0):
    """dst[b, p, dst_off:dst_off+c] = src[b % srcB, p, src_off:src_off+c]; src/dst are [B,H,W,C] buffers (float32 or float16 each:
    the copy converts)."""
    B = dst.shape[0]
    P = dst.shape[1] * dst.shape[2]
    c = c if c is not None else src.shape[3]
    check(load().xmem_copy_channels_t(C.c_void_p(src.data_ptr() + src.element_size() * src_off), _h(src), src.shape[3], src.shape[0],
                                      C.c_void_p(dst.data_ptr() + dst.element_size() * dst_off), _h(dst), dst.shape[3], B, P, c, stream_ptr()))
    return dst


def hidden_update_gather(g16, g8, g4, logits, out):
    """out[..., :c16+c8+c4+1] = [g16 | area2(g8) | area4(g4) | area4(logits)] in one launch (float32 NHWC; HiddenUpdater's input,
    model/modules.py:49-57); the same bits as copy_channels + three area_downsample calls."""
    K, h, w, c16 = g16.shape
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in (g16, g8, g4, logits, out)):
        raise RuntimeError('hidden_update_gather: contiguous float32 tensors only')
    if tuple(g8.shape[:3]) != (K, 2 * h, 2 * w) or tuple(g4.shape[:3]) != (K, 4 * h, 4 * w) or tuple(logits.shape) != (K, 4 * h, 4 * w, 1) \
            or tuple(out.shape[:3]) != (K, h, w):
        raise RuntimeError('hidden_update_gather: shapes do not belong to one decoder pass')
    check(load().xmem_hidden_update_gather(ptr(g16), c16, ptr(g8), g8.shape[3], ptr(g4), g4.shape[3], ptr(logits), ptr(out), out.shape[3],
                                           K, h, w, stream_ptr()))
    return out


def mask_head_gather_ok(g16, g8, g4, cw, hidden, g4d, cat, cat_off):
    """True when `mask_head_gather` takes these tensors: float32 mode, contiguous float32 NHWC tensors of one decoder pass, a 3x3 /
    stride 1 / pad 1 mask head over at most 256 channels, 4-float channel counts and offsets."""
    ts = (g16, g8, g4, hidden, g4d, cat)
    if _PRECISION != 'fp32' or any(t is None or t.dtype != torch.float32 or not t.is_contiguous() for t in ts):
        return False
    K, h, w, c16 = g16.shape
    c8, c4, hd = g8.shape[3], g4.shape[3], hidden.shape[3]
    return (tuple(g8.shape[:3]) == (K, 2 * h, 2 * w) and tuple(g4.shape[:3]) == (K, 4 * h, 4 * w)
            and tuple(hidden.shape[:3]) == (K, h, w) and tuple(g4d.shape[:3]) == (K, h, w) and tuple(cat.shape[:3]) == (K, h, w)
            and (cw.cout, cw.kh, cw.kw, cw.stride, cw.pad, cw.dilation, cw.cin) == (1, 3, 3, 1, 1, 1, c4) and c4 <= 256
            and not (c16 % 4 or c8 % 4 or c4 % 4 or hd % 4 or cat_off % 4 or cat.shape[3] % 4 or g4d.shape[3] % 4)
            and g4d.shape[3] >= c16 + c8 + c4 + 1 and cat_off + hd <= cat.shape[3])


def mask_head_gather(g16, g8, g4, cw, hidden, g4d, cat, cat_off):
    """The end of the decoder in one launch, g4 read once: logits = conv2d(g4, cw, relu_in=True) (the mask head `cw`: 3x3, Cout 1),
    g4d[..., :c16+c8+c4+1] = [g16 | area2(g8) | area4(g4) | area4(logits)] and cat[..., cat_off:cat_off+hd] = hidden.  The same bits
    as conv2d + hidden_update_gather + copy_channels.  Returns logits [K,4h,4w,1]."""
    if not mask_head_gather_ok(g16, g8, g4, cw, hidden, g4d, cat, cat_off):
        raise RuntimeError('mask_head_gather: float32 mode, contiguous float32 tensors of one decoder pass and a 3x3 mask head over <= 256 channels only')
    K, h, w, c16 = g16.shape
    c8, c4, hd = g8.shape[3], g4.shape[3], hidden.shape[3]
    logits = torch.empty((K, 4 * h, 4 * w, 1), dtype=torch.float32, device=g4.device)
    dst = C.c_void_p(cat.data_ptr() + 4 * cat_off)
    launch = lambda: load().xmem_mask_head_gather(ptr(g16), c16, ptr(g8), c8, ptr(g4), c4, ptr(cw.w), ptr(cw.scale), ptr(cw.shift),
                                                  ptr(hidden), hd, ptr(logits), ptr(g4d), g4d.shape[3], dst, cat.shape[3], K, h, w,
                                                  stream_ptr())
    check(launch())
    if RECORD is not None:
        # the mask head's own entry (key, FLOPs, plan) as conv2d writes it: the survey of the convolutions still counts the layer
        ConvCall(x=g4, cw=cw, out=logits, relu_in=True, plan=(conv_plan.HEURISTIC, 0)).record(launch)
    return logits


def cbam_residual(g, p):
    """out = g + CBAM(g); p = dict(w1,b1,w2,b2,sw,sb) device tensors (float32); g float32 or float16."""
    lib = load()
    B, H, W, Cc = g.shape
    out = torch.empty_like(g)
    need = lib.xmem_cbam_workspace_bytes(B, H * W, Cc)
    ws = workspace(need, g.device, 'cbam')
    check(lib.xmem_cbam_residual_t(ptr(g), ptr(out), _h(g), B, H, W, Cc, ptr(p['w1']), ptr(p['b1']), ptr(p['w2']), ptr(p['b2']),
                                   ptr(p['sw']), ptr(p['sb']), ptr(ws), need, stream_ptr()))
    return out


def gru_gate(values, h, out=None):
    """out may be h itself (in-place update of the hidden state).  The state is float32; `values` float32 or float16."""
    B, H, W, Ch = h.shape
    if out is None:
        out = torch.empty_like(h)
    check(load().xmem_gru_gate_t(ptr(values), _h(values), ptr(h), ptr(out), B, H * W, Ch, stream_ptr()))
    return out


def pack_image(img, Hp, Wp, lh, lw, out=None):
    """img [3,H,W] -> [1,Hp,Wp,4] zero padded NHWC (into `out` when given: one frame of a batched buffer)."""
    _req(img, 'image')
    if not img.is_contiguous():
        img = img.contiguous()
    if out is None:
        out = torch.empty((1, Hp, Wp, 4), dtype=torch.float32, device=img.device)
    check(load().xmem_pack_image(ptr(img), ptr(out), img.shape[1], img.shape[2], Hp, Wp, lh, lw, stream_ptr()))
    return out


IM_MEAN = (0.485, 0.456, 0.406)      # dataset/range_transform.py:5-8
IM_STD = (0.229, 0.224, 0.225)


def pack_image_u8(img, Hp, Wp, lh, lw, mean=IM_MEAN, std=IM_STD, out=None):
    """decoded frame uint8 [H,W,3] -> normalised, zero padded [1,Hp,Wp,4] (ToTensor + Normalize + pad in one kernel)."""
    if not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise RuntimeError('pack_image_u8: expected a CUDA (HIP) uint8 tensor of shape [H, W, 3]')
    if not img.is_contiguous():
        img = img.contiguous()
    if out is None:
        out = torch.empty((1, Hp, Wp, 4), dtype=torch.float32, device=img.device)
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    check(load().xmem_pack_image_u8(ptr(img), ptr(out), img.shape[0], img.shape[1], Hp, Wp, lh, lw, m3, s3, stream_ptr()))
    return out


_resize_taps = {}       # (device, in, out) -> (bounds, coeffs, ksize) on the device: uploaded once per geometry


def _device_taps(device, in_size, out_size):
    key = (str(device), int(in_size), int(out_size))
    t = _resize_taps.get(key)
    if t is None:
        bounds, coeffs = taps(in_size, out_size)
        # a blocking copy: the tables are complete before any stream reads them, whichever stream is current now
        t = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coeffs.copy()).to(device), int(coeffs.shape[1]))
        _resize_taps[key] = t
    return t


def resize_u8(src, size, flip=False, out=None):
    """decoded frame uint8 [H,W,3] -> uint8 [th,tw,3]: `Image.resize((tw, th), Image.BILINEAR)` of the host library byte for byte
    (xmem2_amd/pil_resize.py states the arithmetic), columns mirrored when `flip`.  `out`: a contiguous uint8 [th,tw,3] tensor, e.g.
    one frame of a batched buffer.  Launched on the current stream; the intermediate of the horizontal pass comes from the stream's
    own allocator pool, so calls on different streams share no scratch."""
    if not src.is_cuda or src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous():
        raise RuntimeError('resize_u8: expected a contiguous CUDA (HIP) uint8 tensor of shape [H, W, 3]')
    th, tw = int(size[0]), int(size[1])
    if th < 1 or tw < 1:
        raise RuntimeError(f'resize_u8: target size {(th, tw)} must be positive')
    Hs, Ws = int(src.shape[0]), int(src.shape[1])
    if max(Hs, Ws, th, tw) > MAX_SIDE:                 # what the C entry point answers, before any table is built or uploaded
        check(_lib.UNSUPPORTED)
    if out is None:
        out = torch.empty((th, tw, 3), dtype=torch.uint8, device=src.device)
    elif not out.is_cuda or out.device != src.device or out.dtype != torch.uint8 or tuple(out.shape) != (th, tw, 3) \
            or not out.is_contiguous() or (out.data_ptr() < src.data_ptr() + src.numel() and src.data_ptr() < out.data_ptr() + out.numel()):
        raise RuntimeError(f'resize_u8: out must be a contiguous uint8 CUDA (HIP) tensor of shape {(th, tw, 3)} that does not overlap '
                           'the input')
    lib = load()
    xb, xc, xk = _device_taps(src.device, Ws, tw) if Ws != tw else (None, None, 0)
    yb, yc, yk = _device_taps(src.device, Hs, th) if Hs != th else (None, None, 0)
    nbytes = lib.xmem_resize_u8_workspace_bytes(Hs, Ws, th, tw)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device) if nbytes else None
    check(lib.xmem_resize_u8_bilinear_aa(ptr(src), Hs, Ws, ptr(out), th, tw, int(bool(flip)), ptr(xb), ptr(xc), xk, ptr(yb), ptr(yc), yk,
                                         ptr(ws), nbytes, stream_ptr()))
    return out


def copy_segments(pairs):
    """Every (src, dst) pair of `pairs` copied byte for byte, dst <- src, in ONE launch per `_lib.COPY_MAX_SEGMENTS` pairs on the
    current stream (the feature cache of a session: one frame's key-encoder outputs <-> its cache entry).  The addresses travel in the
    kernel arguments: nothing is uploaded, nothing is captured, so they may differ from call to call.  Both sides of a pair are
    contiguous tensors on one HIP device with the same number of BYTES (the dtypes and shapes may differ); empty pairs are allowed."""
    pairs = list(pairs)
    n = len(pairs)
    if n == 0:
        return
    device = None
    for i, (src, dst) in enumerate(pairs):
        if not (torch.is_tensor(src) and torch.is_tensor(dst)) or not src.is_cuda or not dst.is_cuda:
            raise RuntimeError(f'copy_segments: pair {i}: expected CUDA (HIP) tensors - xmem2_amd has no CPU path')
        if src.device != dst.device or (device is not None and src.device != device):
            raise RuntimeError(f'copy_segments: pair {i}: every tensor of a call must live on one device')
        device = src.device
        if not src.is_contiguous() or not dst.is_contiguous():
            raise RuntimeError(f'copy_segments: pair {i}: both sides must be contiguous')
        if src.numel() * src.element_size() != dst.numel() * dst.element_size():
            raise RuntimeError(f'copy_segments: pair {i}: {src.numel() * src.element_size()} source bytes for '
                               f'{dst.numel() * dst.element_size()} destination bytes')
    srcs = (C.c_void_p * n)(*[s.data_ptr() for s, _ in pairs])
    dsts = (C.c_void_p * n)(*[d.data_ptr() for _, d in pairs])
    sizes = (C.c_size_t * n)(*[s.numel() * s.element_size() for s, _ in pairs])
    with torch.cuda.device(device):
        check(load().xmem_copy_segments(srcs, dsts, sizes, n, stream_ptr()))


def pack_value_input(image4, masks):
    """image4 [1,Hp,Wp,4], masks [K,Hp,Wp] -> [K,Hp,Wp,8]."""
    K, Hp, Wp = masks.shape
    out = torch.empty((K, Hp, Wp, 8), dtype=torch.float32, device=masks.device)
    check(load().xmem_pack_value_input(ptr(image4), ptr(masks), ptr(out), K, Hp, Wp, stream_ptr()))
    return out


def key_post(proj, ck, need_s=True, need_e=True):
    """proj [1,h,w,ld] -> key [h*w,ck], shrinkage [h*w] | None, selection [h*w,ck] | None."""
    P = proj.shape[0] * proj.shape[1] * proj.shape[2]
    key = torch.empty((P, ck), dtype=torch.float32, device=proj.device)
    shr = torch.empty((P,), dtype=torch.float32, device=proj.device) if need_s else None
    sel = torch.empty((P, ck), dtype=torch.float32, device=proj.device) if need_e else None
    check(load().xmem_key_post(ptr(proj), proj.shape[3], ptr(key), ptr(shr), ptr(sel), P, ck, stream_ptr()))
    return key, shr, sel


def logits_to_prob(logits, H, W, lh, lw, want_padded=True):
    """logits [K,h4,w4] -> prob [K+1,H,W] (cropped) and [K+1,4h4,4w4] (padded)."""
    K, h4, w4 = logits.shape
    prob = torch.empty((K + 1, H, W), dtype=torch.float32, device=logits.device)
    padded = torch.empty((K + 1, 4 * h4, 4 * w4), dtype=torch.float32, device=logits.device) if want_padded else None
    check(load().xmem_logits_to_prob(ptr(logits), ptr(prob), ptr(padded), K, h4, w4, H, W, lh, lw, stream_ptr()))
    return prob, padded


def aggregate_masks(masks):
    K, H, W = masks.shape
    if not masks.is_contiguous():
        masks = masks.contiguous()
    prob = torch.empty((K + 1, H, W), dtype=torch.float32, device=masks.device)
    check(load().xmem_aggregate_masks(ptr(_req(masks, 'masks')), ptr(prob), K, H, W, stream_ptr()))
    return prob


def merge_masks(pred_no_bg, mask, valid_bits):
    K, H, W = mask.shape
    out = torch.empty_like(mask)
    check(load().xmem_merge_masks(ptr(pred_no_bg), ptr(mask), valid_bits, ptr(out), K, H, W, stream_ptr()))
    return out


def resize_bilinear(prob, shape):
    Cc, Hi, Wi = prob.shape
    if not prob.is_contiguous():
        prob = prob.contiguous()
    out = torch.empty((Cc, int(shape[0]), int(shape[1])), dtype=torch.float32, device=prob.device)
    check(load().xmem_resize_bilinear(ptr(prob), ptr(out), Cc, Hi, Wi, int(shape[0]), int(shape[1]), stream_ptr()))
    return out


def argmax_u8(prob):
    Cc, H, W = prob.shape
    if not prob.is_contiguous():
        prob = prob.contiguous()
    out = torch.empty((H, W), dtype=torch.uint8, device=prob.device)
    check(load().xmem_argmax_u8(ptr(_req(prob, 'prob')), ptr(out), Cc, H, W, stream_ptr()))
    return out


def ensemble_accumulate(prob, shape, mirror, acc, first, out=None):
    """One pass of the test-time ensemble into `acc` (uint16 [C,H,W], `shape` = (H, W), the original resolution): bilinear resize of
    prob [C,Hi,Wi] (when its size differs), horizontal flip if `mirror`, (uint8)(p * 255), acc = q if `first` else acc + q.  With
    `out` (uint8 [H,W]) the first-index argmax of the updated sum is written there too.  Returns `out` (or `acc` without it)."""
    Cc, Hi, Wi = prob.shape
    H, W = int(shape[0]), int(shape[1])
    _req(prob, 'prob')
    if not prob.is_contiguous():
        prob = prob.contiguous()
    if not acc.is_cuda or acc.dtype != torch.uint16 or tuple(acc.shape) != (Cc, H, W) or not acc.is_contiguous():
        raise RuntimeError(f'acc: expected a contiguous uint16 CUDA (HIP) tensor of shape {(Cc, H, W)}')
    if out is not None and (not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != (H, W) or not out.is_contiguous()):
        raise RuntimeError(f'out: expected a contiguous uint8 CUDA (HIP) tensor of shape {(H, W)}')
    check(load().xmem_ensemble_accumulate(ptr(prob), Cc, Hi, Wi, int(bool(mirror)), ptr(acc), H, W, int(bool(first)), ptr(out),
                                          stream_ptr()))
    return out if out is not None else acc


JF_SLOTS = ('gt_area', 'pred_area', 'inter', 'n_gt', 'n_pred', 'gt_match', 'pred_match')
JF_MAX_RADIUS = 63


def jf_counts(gt, pred, radius, lut=None, out=None):
    """DAVIS J&F counts of uint8 label maps `gt`, `pred` ([H,W] or [B,H,W], same shape) into int32 `out` [B,256,7] (allocated if None):
    per frame and label k in 1..254 the JF_SLOTS counts, boundaries dilated by the disk of `radius` (0..63).  `lut` (uint8 [256]) maps
    pred's labels first.  `out` is zeroed and filled on the current stream; returns it."""
    gt, pred = _req_u8(gt, 'gt', frames='B'), _req_u8(pred, 'pred', frames='B')
    if tuple(gt.shape) != tuple(pred.shape):
        raise RuntimeError(f'gt and pred differ in shape: {tuple(gt.shape)} != {tuple(pred.shape)}')
    B, H, W = (1,) + tuple(gt.shape) if gt.dim() == 2 else tuple(gt.shape)
    if lut is not None:
        if not lut.is_cuda or lut.dtype != torch.uint8 or tuple(lut.shape) != (256,):
            raise RuntimeError('lut: expected a uint8 CUDA (HIP) tensor of shape (256,)')
        lut = lut.contiguous()
    if out is None:
        out = torch.empty((B, 256, len(JF_SLOTS)), dtype=torch.int32, device=gt.device)
    elif (not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != (B, 256, len(JF_SLOTS)) or not out.is_contiguous()):
        raise RuntimeError(f'out: expected a contiguous int32 CUDA (HIP) tensor of shape {(B, 256, len(JF_SLOTS))}')
    check(load().xmem_jf_counts(ptr(gt), ptr(pred), ptr(lut), B, H, W, int(radius), ptr(out), stream_ptr()))
    return out


def nhwc_to_nchw(x, c=None, off=0):
    """x [B,H,W,ld] (channels off..off+c) -> contiguous [B,c,H,W]."""
    B, H, W, ld = x.shape
    c = c if c is not None else ld
    out = torch.empty((B, c, H, W), dtype=torch.float32, device=x.device)
    check(load().xmem_nhwc_to_nchw(C.c_void_p(x.data_ptr() + 4 * off), ld, ptr(out), B, H * W, c, stream_ptr()))
    return out


def nchw_to_nhwc(x):
    B, c, H, W = x.shape
    if not x.is_contiguous():
        x = x.contiguous()
    out = torch.empty((B, H, W, c), dtype=torch.float32, device=x.device)
    check(load().xmem_nchw_to_nhwc(ptr(_req(x, 'tensor')), ptr(out), c, B, H * W, c, stream_ptr()))
    return out


# ---------------------------------------------------------------------------------------------
# memory readout
# ---------------------------------------------------------------------------------------------

ROWS16_FLOATS = _lib.CONSTANTS['XMEM_ROWS16_HALFS'] // 2      # one fp16 filter operand row (144 halfs = 288 bytes) counted in floats
MAX_SEGMENTS = _lib.CONSTANTS['XMEM_MAX_SEGMENTS']            # segments one affinity hint describes


def affinity_rows16(key, shrinkage, out):
    """Filter operand rows of the memory elements `key` [n,Ck] / `shrinkage` [n] | None into out [n, 72] (float32-typed storage
    of 144 halfs per row).  Stores call this when elements are added or replaced (kv_memory_store.py) and hand the rows to
    affinity_topk, so the per-frame rows kernel and its N x 288 bytes of writes are gone."""
    n = key.shape[0]
    if n == 0:
        return out
    if out.shape[0] != n or out.shape[1] != ROWS16_FLOATS or not out.is_contiguous() or not key.is_contiguous():
        raise RuntimeError('affinity_rows16: expected contiguous key [n, Ck] and out [n, 72]')
    check(load().xmem_affinity_rows16(ptr(_req(key, 'key')), ptr(shrinkage), n, ptr(out), stream_ptr()))
    return out


def affinity_topk(segments, qk, qe, top_k, want_sim=False, hint=None):
    """segments: list of (key [n,Ck], shrinkage [n] | None[, rows16 [n,72] | None]).  Returns w [HW,k], idx [HW,k] (int32), sim | None.
    hint: None or (idx [HW,k'] int32 of an earlier call on the same list of stores, its segment sizes, grid width) - only
    tightens the internal lower bound of the k-th similarity (xmem_affinity_topk_hinted); results do not depend on it."""
    lib = load()
    HW, ck = qk.shape
    segs = [(sg[0], sg[1], sg[2] if len(sg) > 2 else None) if (sg[0] is not None and sg[0].shape[0] > 0) else (None, None, None)
            for sg in segments]                                            # empty stores keep their slot
    n_total = sum(k.shape[0] for k, _, _ in segs if k is not None)
    if n_total < top_k:
        raise RuntimeError(f'selected index k out of range: top_k={top_k} > {n_total} memory elements')
    arr = (KeySegment * max(len(segs), 1))()
    for i, (k, s, r16) in enumerate(segs):
        arr[i].key = k.data_ptr() if k is not None else None
        arr[i].shrinkage = s.data_ptr() if s is not None else None
        arr[i].n = k.shape[0] if k is not None else 0
        arr[i].rows16 = r16.data_ptr() if (r16 is not None and k is not None and r16.shape[0] == k.shape[0]) else None
    w = torch.empty((HW, top_k), dtype=torch.float32, device=qk.device)
    idx = torch.empty((HW, top_k), dtype=torch.int32, device=qk.device)
    sim = torch.empty((HW, top_k), dtype=torch.float32, device=qk.device) if want_sim else None
    need = lib.xmem_affinity_topk_workspace_bytes(n_total, HW, top_k)
    ws = workspace(need, qk.device, 'affinity')
    h, hp = None, None
    if hint is not None:
        h_idx, h_sizes, h_gw = hint
        if h_idx is not None and h_idx.is_cuda and tuple(h_idx.shape[:1]) == (HW,) and h_idx.dtype == torch.int32 \
                and len(h_sizes) == len(segs) <= MAX_SEGMENTS:
            h = AffinityHint()
            h.idx = h_idx.data_ptr(); h.top_k = h_idx.shape[1]; h.n_seg = len(h_sizes)
            for i, n in enumerate(h_sizes):
                h.seg_n[i] = int(n)
            h.grid_w = int(h_gw or 0)
            hp = C.byref(h)
    e0 = _tap_begin()
    check(lib.xmem_affinity_topk_hinted(arr, len(segs), ptr(qk), ptr(qe), ck, HW, top_k, hp, ptr(w), ptr(idx), ptr(sim),
                                        ptr(ws), need, stream_ptr()))
    _tap_end('affinity', e0, 4.0 * ck * n_total * HW)
    if RECORD is not None:
        RECORD.append(('affinity', f'{n_total}x{HW}k{top_k}', 4.0 * ck * n_total * HW,
                       lambda: lib.xmem_affinity_topk_hinted(arr, len(segs), ptr(qk), ptr(qe), ck, HW, top_k, hp, ptr(w), ptr(idx),
                                                             ptr(sim), ptr(ws), need, stream_ptr()), (segs, qk, qe, w, idx, sim, ws, h, hint)))
    return w, idx, sim


def usage_update(w, idx, first, count, use_count, life_count):
    if count <= 0:
        return
    HW, k = w.shape
    fx = workspace(8 * count, w.device, 'usage_fx')
    check(load().xmem_usage_update(ptr(w), ptr(idx), HW, k, first, count, ptr(use_count), ptr(life_count), ptr(fx), stream_ptr()))


def readout_sparse(value_segments, w, idx, cv, out, out_ld, obj_stride, out_off=0):
    """value_segments[obj][seg] = tensor [n_seg, Cv] (n may be 0).  Writes out[obj][q][out_off:out_off+Cv]."""
    n_obj = len(value_segments)
    n_seg = len(value_segments[0])
    arr = (ValueSegment * (n_obj * n_seg))()
    for o, segs in enumerate(value_segments):
        for s, v in enumerate(segs):
            arr[o * n_seg + s].value = v.data_ptr() if v is not None and v.shape[0] > 0 else None
            arr[o * n_seg + s].n = v.shape[0] if v is not None else 0
    HW, k = w.shape
    e0 = _tap_begin()
    check(load().xmem_readout_sparse_t(arr, n_obj, n_seg, ptr(w), ptr(idx), HW, k, cv,
                                       C.c_void_p(out.data_ptr() + out.element_size() * out_off), _h(out), out_ld, obj_stride, stream_ptr()))
    _tap_end('readout', e0, 2.0 * cv * k * HW * n_obj)


def similarity_dense(key, shrinkage, qk, qe):
    """key [n,Ck], qk/qe [P,Ck] -> sim [P,n]."""
    n, ck = key.shape
    P = qk.shape[0]
    out = torch.empty((P, n), dtype=torch.float32, device=key.device)
    check(load().xmem_similarity_dense(ptr(key), ptr(shrinkage), n, ptr(qk), ptr(qe), P, ck, ptr(out), stream_ptr()))
    return out


def selector_prepare(key_rows, sel_rows, mask, h, w, alpha, eps, Mexp, Qexp, bsq, presence):
    """One frame of the candidate selector (frame_selection.py:156-186): key_rows/sel_rows [HW,Ck], mask [C,H,W] | None,
    outputs are views into the per-video operand arrays (Mexp/Qexp [HW,2Ck], bsq [HW], presence int32[1])."""
    hw, ck = key_rows.shape
    if hw != h * w:
        raise ValueError('key rows do not match h*w')
    if mask is not None:
        Cm, H, W = mask.shape
        mask = _req(mask, 'mask')
    else:
        Cm = H = W = 0
    check(load().xmem_selector_prepare(ptr(_req(key_rows, 'key')), ptr(_req(sel_rows, 'selection')), ptr(mask), Cm, H, W,
                                       h, w, ck, float(alpha), float(1 - alpha), float(eps),
                                       ptr(Mexp), ptr(Qexp), ptr(bsq), ptr(presence), stream_ptr()))


def selector_prepare_u8(key_rows, sel_rows, mask_u8, lut, h, w, alpha, eps, Mexp, Qexp, bsq, presence):
    """`selector_prepare` for a mask held as a uint8 label plane [H,W] and a float32 table lut[256]: the mask value of a pixel is
    lut[label].  Bit-identical to `selector_prepare` on the float mask `lut[mask_u8][None]`."""
    hw, ck = key_rows.shape
    if hw != h * w:
        raise ValueError('key rows do not match h*w')
    if mask_u8.dim() != 2:
        raise ValueError('mask must be a uint8 [H, W] label plane')
    if lut.dtype != torch.float32 or lut.numel() != 256:
        raise ValueError('lut must hold 256 float32 entries')
    H, W = mask_u8.shape
    check(load().xmem_selector_prepare_u8(ptr(_req(key_rows, 'key')), ptr(_req(sel_rows, 'selection')), ptr(_req_u8(mask_u8, 'mask')),
                                          ptr(_req(lut, 'lut')), H, W, h, w, ck, float(alpha), float(1 - alpha), float(eps),
                                          ptr(Mexp), ptr(Qexp), ptr(bsq), ptr(presence), stream_ptr()))


def cycle_dissimilarity(Mexp, Qexp, bsq, shrinkage, chosen, valid=None):
    """Score every frame against frame `chosen` (frame_selection.py:218-226).  Mexp/Qexp [F,HW,2Ck]; bsq/shrinkage [F,HW];
    valid uint8 [F] | None.  Returns float64 [F]."""
    F, HW, k2 = Mexp.shape
    out = torch.empty((F,), dtype=torch.float64, device=Mexp.device)
    nbytes = load().xmem_cycle_dissimilarity_workspace_bytes(F, HW)
    ws = workspace(nbytes, Mexp.device, 'selector')
    check(load().xmem_cycle_dissimilarity(ptr(_req(Mexp, 'Mexp')), ptr(_req(Qexp, 'Qexp')), ptr(_req(bsq, 'bsq')),
                                          ptr(_req(shrinkage, 'shrinkage')), F, HW, k2 // 2, int(chosen), ptr(valid),
                                          ptr(out), ptr(ws), nbytes, stream_ptr()))
    return out


def usage_ratio(use, life):
    out = torch.empty_like(use)
    check(load().xmem_usage_ratio(ptr(use), ptr(life), ptr(out), use.numel(), stream_ptr()))
    return out


def topk_1d(values, k, largest=True):
    idx = torch.empty((k,), dtype=torch.int32, device=values.device)
    val = torch.empty((k,), dtype=torch.float32, device=values.device)
    check(load().xmem_topk_1d(ptr(values), values.numel(), k, int(largest), ptr(idx), ptr(val), stream_ptr()))
    return val, idx


def gather_rows(src, index):
    """src [n,C] (or [n]) rows at int32 `index` [m] -> [m,C]."""
    cdim = src.shape[1] if src.dim() == 2 else 1
    m = index.numel()
    out = torch.empty((m, cdim) if src.dim() == 2 else (m,), dtype=torch.float32, device=src.device)
    if m > 0:
        check(load().xmem_gather_rows(ptr(src), cdim, ptr(index), m, ptr(out), stream_ptr()))
    return out


def softmax_rows_suffix(sim, count):
    P, n = sim.shape
    check(load().xmem_softmax_rows_suffix(ptr(sim), P, n, count, stream_ptr()))
    return sim


def softmax_rows_topk(sim, k):
    """In place on contiguous rows [P, n]: softmax over each row's k largest entries (no max shift, memory_util.py:45-54),
    zeros elsewhere."""
    P, n = sim.shape
    if not sim.is_contiguous():
        raise RuntimeError('softmax_rows_topk: rows must be contiguous')
    check(load().xmem_softmax_rows_topk(ptr(_req(sim, 'sim')), P, n, k, stream_ptr()))
    return sim


def weighted_rows(aff, count, V):
    """aff [P,n]; V [count,C] -> [P,C] using the last `count` columns of aff."""
    P, n = aff.shape
    cdim = V.shape[1] if V.dim() == 2 else 1
    out = torch.empty((P, cdim), dtype=torch.float32, device=aff.device)
    check(load().xmem_weighted_rows(ptr(aff), P, n, count, ptr(V), cdim, ptr(out), stream_ptr()))
    return out


def select_greater(usage, threshold_dev):
    n = usage.numel()
    idx = torch.empty((n,), dtype=torch.int32, device=usage.device)
    cnt = torch.empty((1,), dtype=torch.int32, device=usage.device)
    check(load().xmem_select_greater(ptr(usage), n, ptr(threshold_dev), ptr(idx), ptr(cnt), stream_ptr()))
    return idx, cnt


def store_compact(arenas, keep, count):
    """Every arena of a store compacted by one index of surviving key elements (csrc/store_compact.hip), one launch per
    `_lib.COMPACT_MAX_ARENAS` arenas.  arenas: (src, dst) pairs of contiguous float32 tensors, src [n, C] or [n] holding the LAST n of
    the store's N = keep.numel() elements, dst of the same row width with room for n rows and not overlapping any src; keep / count:
    what `select_greater` returned (int32 [N] ascending, int32 [1] on the device).  dst row j - j0 receives src row keep[j] - (N - n)
    for j0 <= j < count, j0 the first j with keep[j] >= N - n.  Returns the kept row counts, int32 [len(arenas)] on the device."""
    arenas = list(arenas)
    n_ar, N = len(arenas), keep.numel()
    if keep.dtype != torch.int32 or count.dtype != torch.int32 or not keep.is_cuda or not count.is_cuda or not keep.is_contiguous():
        raise RuntimeError('store_compact: keep and count must be int32 CUDA (HIP) tensors')
    kept = torch.empty((max(n_ar, 1),), dtype=torch.int32, device=keep.device)
    arr = (CompactArena * max(n_ar, 1))()
    for i, (src, dst) in enumerate(arenas):
        _req(src, f'arena {i} source'); _req(dst, f'arena {i} destination')
        n = src.shape[0]
        width = src.shape[1] if src.dim() == 2 else 1
        if src.dim() not in (1, 2) or dst.dim() != src.dim() or (dst.shape[1] if dst.dim() == 2 else 1) != width or dst.shape[0] < n \
                or not src.is_contiguous() or not dst.is_contiguous() or n > N:
            raise RuntimeError(f'store_compact: arena {i}: source {tuple(src.shape)} / destination {tuple(dst.shape)} of a store of {N}')
        arr[i].src, arr[i].dst = (src.data_ptr(), dst.data_ptr()) if n else (None, None)
        arr[i].width, arr[i].n, arr[i].off = width, n, N - n
    check(load().xmem_store_compact(arr, n_ar, ptr(keep), ptr(count), N, ptr(kept), stream_ptr()))
    return kept[:n_ar]


# ---- scribble-to-mask (S2M) ---------------------------------------------------------------------------------

def s2m_pack(image, prev_mask, scr, K, ignore_class, Hp, Wp, lh, lw, out=None):
    """image [3,H,W] float, prev_mask [H,W] float (object index), scr [H,W] uint8 -> [K,Hp,Wp,8] (the S2M input of every object)."""
    _req(image, 'image')
    _req(prev_mask, 'prev_mask')
    if not scr.is_cuda or scr.dtype != torch.uint8:
        raise RuntimeError('s2m_pack: expected a CUDA (HIP) uint8 scribble map')
    H, W = image.shape[-2:]
    if tuple(prev_mask.shape[-2:]) != (H, W) or tuple(scr.shape[-2:]) != (H, W):
        raise RuntimeError(f's2m_pack: image {H}x{W}, prev_mask {tuple(prev_mask.shape)} and scribbles {tuple(scr.shape)} differ in size')
    image, prev_mask, scr = image.contiguous(), prev_mask.contiguous(), scr.contiguous()
    if out is None:
        out = torch.empty((K, Hp, Wp, 8), dtype=torch.float32, device=image.device)
    check(load().xmem_s2m_pack(ptr(image), ptr(prev_mask), ptr(scr), int(ignore_class), int(K), H, W, Hp, Wp, lh, lw, ptr(out), stream_ptr()))
    return out


def channel_mean(x, out=None):
    """x [B,H,W,C] NHWC -> [B,C], the mean over the pixels (fixed summation order)."""
    B, H, W, Cc = _req(x, 'channel_mean input').shape
    if out is None:
        out = torch.empty((B, Cc), dtype=torch.float32, device=x.device)
    check(load().xmem_channel_mean(ptr(x), x.stride(2), B, H * W, Cc, ptr(out), stream_ptr()))
    return out


def broadcast_channels(vec, out):
    """vec [B,C] -> every pixel of `out` [B,H,W,C] (a channel slice of a wider NHWC buffer: pixel stride out.stride(2))."""
    B, H, W, Cc = out.shape
    check(load().xmem_broadcast_channels(ptr(_req(vec, 'vec').contiguous()), ptr(out), out.stride(2), B, H * W, Cc, stream_ptr()))
    return out


def resize_bilinear_nhwc(x, shape, out=None):
    """F.interpolate(x, size=shape, mode='bilinear', align_corners=False) on NHWC x [B,Hi,Wi,C] (pixel stride x.stride(2)) into
    `out` [B,Ho,Wo,C] (may be a channel slice of a wider buffer)."""
    B, Hi, Wi, Cc = _req(x, 'resize_bilinear_nhwc input').shape
    Ho, Wo = int(shape[0]), int(shape[1])
    if out is None:
        out = torch.empty((B, Ho, Wo, Cc), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (B, Ho, Wo, Cc):
        raise RuntimeError(f'resize_bilinear_nhwc: out has shape {tuple(out.shape)}, expected {(B, Ho, Wo, Cc)}')
    check(load().xmem_resize_bilinear_nhwc(ptr(x), x.stride(2), B, Hi, Wi, Cc, ptr(out), out.stride(2), Ho, Wo, stream_ptr()))
    return out


def s2m_output(logits, H, W, lh, lw, temperature=1000.0, want_wbg=True, prob=None, wbg=None, mask=None):
    """logits [K,h4,w4] -> prob [K,H,W] (sigmoid of the x4 bilinear upsample, cropped at lh, lw) and, with want_wbg,
    aggregate_wbg(prob, keep_bg=True) at `temperature` [K+1,H,W] and its argmax (uint8 [H,W])."""
    K, h4, w4 = _req(logits, 'logits').shape
    dev = logits.device
    if prob is None:
        prob = torch.empty((K, H, W), dtype=torch.float32, device=dev)
    if want_wbg and wbg is None:
        wbg = torch.empty((K + 1, H, W), dtype=torch.float32, device=dev)
    if want_wbg and mask is None:
        mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    check(load().xmem_s2m_output(ptr(logits.contiguous()), K, h4, w4, H, W, lh, lw, ptr(prob), ptr(wbg), ptr(mask),
                                 float(temperature), stream_ptr()))
    return prob, wbg, mask


def aggregate_wbg(prob, keep_bg=False, temperature=1.0, want_mask=False):
    """interaction.py aggregate_wbg: prob [K,H,W] -> [K+1,H,W] (keep_bg) or [K,H,W]; with want_mask also the uint8 argmax of
    the K + 1 softmax values."""
    K, H, W = _req(prob, 'prob').shape
    out = torch.empty((K + 1 if keep_bg else K, H, W), dtype=torch.float32, device=prob.device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=prob.device) if want_mask else None
    check(load().xmem_aggregate_wbg(ptr(prob.contiguous()), K, H, W, int(bool(keep_bg)), float(temperature), ptr(out), ptr(mask),
                                    stream_ptr()))
    return (out, mask) if want_mask else out


# ---- click-to-mask (the f-BRS click network) --------------------------------------------------------------------

def click_input(image, clicks, counts, rgb_conv, radius=260.0, with_flip=True, out=None, want_features=False):
    """image [3,H,W] at the working size, clicks [2,cap,2] float (row, col; positives first), counts [2] int32 (device), rgb_conv
    [75] (w1 [8,5], b1 [8], w2 [3,8], b2 [3], BatchNorm folded) -> the network input [B,H,W,8] NHWC, B = 2 with_flip (sample 1:
    mirrored image and clicks); with want_features also the distance features [B,2,H,W]."""
    _req(image, 'image'); _req(clicks, 'clicks'); _req(rgb_conv, 'rgb_conv')
    if not counts.is_cuda or counts.dtype != torch.int32 or counts.numel() != 2:
        raise RuntimeError('click_input: counts must be two int32 on the device')
    if clicks.dim() != 3 or clicks.shape[0] != 2 or clicks.shape[2] != 2 or not clicks.is_contiguous():
        raise RuntimeError(f'click_input: clicks must be a contiguous [2, cap, 2] tensor, got {tuple(clicks.shape)}')
    if image.dim() != 3 or image.shape[0] != 3 or rgb_conv.numel() != 75:
        raise RuntimeError('click_input: expected an image [3,H,W] and 75 rgb_conv parameters')
    image = image.contiguous()
    H, W = image.shape[-2:]
    B = 2 if with_flip else 1
    if out is None:
        out = torch.empty((B, H, W, 8), dtype=torch.float32, device=image.device)
    feat = torch.empty((B, 2, H, W), dtype=torch.float32, device=image.device) if want_features else None
    check(load().xmem_click_input(ptr(image), ptr(clicks), clicks.shape[1], ptr(counts), float(radius), ptr(rgb_conv.contiguous()),
                                  H, W, int(bool(with_flip)), ptr(out), ptr(feat), stream_ptr()))
    return (out, feat) if want_features else out


def depthwise3x3(x, w, out=None):
    """Depthwise 3x3 (pad 1, stride 1, no bias) on NHWC x [B,H,W,C] (pixel stride x.stride(2)) with w [9,C] -> out [B,H,W,C]
    (may be a channel slice of a wider buffer)."""
    B, H, W, Cc = _req(x, 'depthwise3x3 input').shape
    if tuple(_req(w, 'depthwise3x3 weight').shape) != (9, Cc) or not w.is_contiguous():
        raise RuntimeError(f'depthwise3x3: weight must be a contiguous [9, {Cc}] tensor, got {tuple(w.shape)}')
    if out is None:
        out = torch.empty((B, H, W, Cc), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (B, H, W, Cc):
        raise RuntimeError(f'depthwise3x3: out has shape {tuple(out.shape)}, expected {(B, H, W, Cc)}')
    check(load().xmem_depthwise3x3_nhwc(ptr(x), x.stride(2), ptr(w), ptr(out), out.stride(2), B, H, W, Cc, stream_ptr()))
    return out


def resize_bilinear_ac_nhwc(x, shape, out=None):
    """F.interpolate(x, size=shape, mode='bilinear', align_corners=True) on NHWC, otherwise as resize_bilinear_nhwc."""
    B, Hi, Wi, Cc = _req(x, 'resize_bilinear_ac_nhwc input').shape
    Ho, Wo = int(shape[0]), int(shape[1])
    if out is None:
        out = torch.empty((B, Ho, Wo, Cc), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (B, Ho, Wo, Cc):
        raise RuntimeError(f'resize_bilinear_ac_nhwc: out has shape {tuple(out.shape)}, expected {(B, Ho, Wo, Cc)}')
    check(load().xmem_resize_bilinear_ac_nhwc(ptr(x), x.stride(2), B, Hi, Wi, Cc, ptr(out), out.stride(2), Ho, Wo, stream_ptr()))
    return out


def resize_bilinear_ac(x, size, crop=None, out=None, paste=None, zero_fill=False):
    """align_corners=True bilinear resize of planar x [C,Hi,Wi].  crop = (rmin, rmax, cmin, cmax), inclusive as the reference's ROIs: the
    source rectangle (default: all of x).  Without `out` the result is [C, size]; with out [C,Ho,Wo] and paste = (rmin, rmax, cmin,
    cmax) the crop is resized to the paste rectangle's size and written there, zeros elsewhere with zero_fill."""
    Cc, Hi, Wi = _req(x, 'resize_bilinear_ac input').shape
    x = x.contiguous()
    r0, r1, c0, c1 = (0, Hi - 1, 0, Wi - 1) if crop is None else [int(v) for v in crop]
    if out is None:
        Hd, Wd = int(size[0]), int(size[1])
        out = torch.empty((Cc, Hd, Wd), dtype=torch.float32, device=x.device)
        pr0, pc0 = 0, 0
    else:
        if out.dim() != 3 or out.shape[0] != Cc or not out.is_contiguous() or paste is None:
            raise RuntimeError('resize_bilinear_ac: out must be a contiguous [C,Ho,Wo] tensor given together with paste')
        pr0, pr1, pc0, pc1 = [int(v) for v in paste]
        Hd, Wd = pr1 - pr0 + 1, pc1 - pc0 + 1
    check(load().xmem_resize_bilinear_ac(ptr(x), Cc, Hi, Wi, r0, c0, r1 - r0 + 1, c1 - c0 + 1, ptr(_req(out, 'out')), out.shape[1],
                                         out.shape[2], pr0, pc0, Hd, Wd, int(bool(zero_fill)), stream_ptr()))
    return out


def click_prob(logits, H, W, out=None):
    """logits [B,h4,w4] (B = 2: plain and mirrored sample) -> prob [H,W] = sigmoid of the (flip-averaged) align_corners upsample."""
    B, h4, w4 = _req(logits, 'logits').shape
    if B not in (1, 2) or not logits.is_contiguous():
        raise RuntimeError(f'click_prob: expected contiguous logits [1 or 2, h4, w4], got {tuple(logits.shape)}')
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=logits.device)
    check(load().xmem_click_prob(ptr(logits), h4, w4, int(H), int(W), int(B == 2), ptr(out), stream_ptr()))
    return out


def mask_bbox(prob, threshold=0.5, click_pixels=None, out=None):
    """prob [H,W] -> int32 [5] on the device: (rmin, rmax, cmin, cmax) of prob > threshold joined with click_pixels (int32 [n,2]
    row, col on the device), and the number of pixels above the threshold."""
    H, W = _req(prob, 'prob').shape
    n = 0
    if click_pixels is not None:
        if not click_pixels.is_cuda or click_pixels.dtype != torch.int32 or click_pixels.dim() != 2 or click_pixels.shape[1] != 2:
            raise RuntimeError('mask_bbox: click_pixels must be an int32 [n, 2] tensor on the device')
        click_pixels, n = click_pixels.contiguous(), click_pixels.shape[0]
    if out is None:
        out = torch.empty(5, dtype=torch.int32, device=prob.device)
    check(load().xmem_mask_bbox(ptr(prob.contiguous()), H, W, float(threshold), ptr(click_pixels) if n else ptr(None), n, ptr(out),
                                stream_ptr()))
    return out


def prob_threshold(prob, threshold=0.5):
    """(prob > threshold).float() of a contiguous float tensor."""
    if not _req(prob, 'prob').is_contiguous():
        raise RuntimeError('prob_threshold: expected a contiguous tensor')
    out = torch.empty_like(prob)
    check(load().xmem_prob_threshold(ptr(prob), prob.numel(), float(threshold), ptr(out), stream_ptr()))
    return out


def click_commit(prev_prob, obj_mask, tar_obj, temperature=1000.0):
    """ClickInteraction.predict: prev_prob [K+1,H,W], obj_mask [H,W], tar_obj in 1..K -> (aggregate_wbg of the clamped maps with row
    tar_obj replaced [K+1,H,W], its argmax uint8 [H,W])."""
    K1, H, W = _req(prev_prob, 'prev_prob').shape
    if tuple(_req(obj_mask, 'obj_mask').shape[-2:]) != (H, W) or obj_mask.numel() != H * W:
        raise RuntimeError(f'click_commit: prev_prob {tuple(prev_prob.shape)} and obj_mask {tuple(obj_mask.shape)} differ in size')
    out = torch.empty((K1, H, W), dtype=torch.float32, device=prev_prob.device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=prev_prob.device)
    check(load().xmem_click_commit(ptr(prev_prob.contiguous()), ptr(obj_mask.contiguous()), K1 - 1, H, W, int(tar_obj), float(temperature),
                                   ptr(out), ptr(mask), stream_ptr()))
    return out, mask


# ---- robot-click evaluation (csrc/edt.hip): integer arithmetic, bit-reproducible -------------------------------------

CLICK_RECORD = 8        # int32 values of xmem_next_click's record (include/xmem_hip.h)


def _req_u8(t, name, shape=None, frames=None):
    """`t`, contiguous: a uint8 device tensor - of `shape`, or with `frames` ('B' or 'N', the letter the message names the leading
    dimension by) maps [H,W] or [frames,H,W]"""
    if (not t.is_cuda or t.dtype != torch.uint8 or (shape is not None and tuple(t.shape) != tuple(shape))
            or (frames is not None and t.dim() not in (2, 3))):
        raise RuntimeError(f'{name}: expected a uint8 CUDA (HIP) tensor' + (f' of shape {tuple(shape)}' if shape is not None else '')
                           + (f' [H,W] or [{frames},H,W]' if frames is not None else '') + ' - xmem2_amd has no CPU path')
    return t.contiguous()


def _map_dims(masks, fn):
    """(B, H, W) of maps [H,W] or [B,H,W], none of them 0"""
    if masks.numel() == 0:
        raise RuntimeError(f'{fn}: empty input {tuple(masks.shape)}')
    return (1,) + tuple(masks.shape) if masks.dim() == 2 else tuple(masks.shape)


def _index_maps(masks, fn):
    masks = _req_u8(masks, fn, frames='N')
    return masks, _map_dims(masks, fn)


def _int_arg(fn, name, v, low, top=None, numpy_ok=True):
    """`v` as an int: an integer, not a bool, in low..top (no `top`: at least `low`).  numpy_ok=False takes Python integers only.
    Which sites take numpy's is history, not design: rle_encode, mask_polygons and the mattes refuse them, rle_decode,
    rle_compress, rle_decompress and fill_edges accept them.  Each keeps what it did."""
    kinds = int
    if numpy_ok:
        import numpy as np
        kinds = (int, np.integer)
    if isinstance(v, bool) or not isinstance(v, kinds) or not (low <= v and (top is None or v <= top)):
        raise ValueError(f'{fn}: {name} = {v!r} must be an integer ' + (f'in {low}..{top}' if top is not None else f'of at least {low}'))
    return int(v)


def _out_like(out, masks, fn):
    """`out` for uint8 maps shaped like `masks`: the caller's tensor, or a new one"""
    if out is None:
        return torch.empty(masks.shape, dtype=torch.uint8, device=masks.device)
    if not out.is_cuda or out.dtype != torch.uint8 or out.shape != masks.shape or not out.is_contiguous() or out.device != masks.device:
        raise RuntimeError(f'{fn}: out must be a contiguous uint8 CUDA (HIP) tensor of shape {tuple(masks.shape)} on the masks\' device')
    return out


def edt_sq(mask, out=None):
    """Exact squared Euclidean distance transform of uint8 planes `mask` [H,W] or [B,H,W] (non-zero = inside) within one ring of
    zeros -> int32 of the same shape: rint(distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1] ** 2), exactly."""
    if mask.dim() not in (2, 3):
        raise RuntimeError(f'edt_sq: expected [H,W] or [B,H,W], got {tuple(mask.shape)}')
    mask = _req_u8(mask, 'mask')
    B, H, W = (1,) + tuple(mask.shape) if mask.dim() == 2 else tuple(mask.shape)
    if out is None:
        out = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    elif not out.is_cuda or out.dtype != torch.int32 or tuple(out.shape) != tuple(mask.shape) or not out.is_contiguous():
        raise RuntimeError(f'edt_sq: out must be a contiguous int32 CUDA (HIP) tensor of shape {tuple(mask.shape)}')
    check(load().xmem_edt_sq(ptr(mask), B, H, W, ptr(out), stream_ptr()))
    return out


def click_errors(pred, gt, threshold=None, planes=None, counts=None):
    """The robot's error planes: gt uint8 [H,W] (1 object, 255 ignore, else background) against `pred`, a float32 probability map
    with `threshold` (pred > threshold) or a uint8 mask (non-zero) -> (planes uint8 [2,H,W] = (fn, fp), counts int32 [2] =
    (intersection, union) under the ignore mask), both on the device."""
    if gt.dim() != 2:
        raise RuntimeError(f'click_errors: gt must be [H,W], got {tuple(gt.shape)}')
    gt = _req_u8(gt, 'gt')
    H, W = gt.shape
    if pred.dtype == torch.float32:
        if threshold is None:
            raise RuntimeError('click_errors: a probability map needs its threshold')
        if tuple(_req(pred, 'pred').shape) != (H, W):
            raise RuntimeError(f'click_errors: pred {tuple(pred.shape)} and gt {(H, W)} differ in shape')
        prob, mask = pred.contiguous(), None
    else:
        prob, mask = None, _req_u8(pred, 'pred', (H, W))
    if planes is None:
        planes = torch.empty((2, H, W), dtype=torch.uint8, device=gt.device)
    else:
        planes = _req_u8(planes, 'planes', (2, H, W))
    if counts is None:
        counts = torch.empty(2, dtype=torch.int32, device=gt.device)
    check(load().xmem_click_errors(ptr(prob), float(threshold or 0.0), ptr(mask), ptr(gt), H, W, ptr(planes), ptr(counts), stream_ptr()))
    return planes, counts


def next_click(d2, not_clicked, counts=None, record=None):
    """d2 int32 [2,H,W] (fn, fp), not_clicked uint8 [H,W] -> record int32 [CLICK_RECORD] on the device: (is_positive, row, col,
    fn_max_d2, fp_max_d2, counts[0], counts[1], 0); not_clicked[row, col] is cleared in place."""
    if not d2.is_cuda or d2.dtype != torch.int32 or d2.dim() != 3 or d2.shape[0] != 2 or not d2.is_contiguous():
        raise RuntimeError('next_click: d2 must be a contiguous int32 CUDA (HIP) tensor [2,H,W]')
    H, W = int(d2.shape[1]), int(d2.shape[2])
    if not not_clicked.is_cuda or not_clicked.dtype != torch.uint8 or tuple(not_clicked.shape) != (H, W) or not not_clicked.is_contiguous():
        raise RuntimeError(f'next_click: not_clicked must be a contiguous uint8 CUDA (HIP) tensor of shape {(H, W)} (it is written)')
    if record is None:
        record = torch.empty(CLICK_RECORD, dtype=torch.int32, device=d2.device)
    lib = load()
    nbytes = lib.xmem_next_click_workspace_bytes(H, W)
    ws = workspace(nbytes, d2.device, 'next_click')
    check(lib.xmem_next_click(ptr(d2), ptr(not_clicked), ptr(counts), H, W, ptr(record), ptr(ws), ws.numel(), stream_ptr()))
    return record


# ---- run-length track export (csrc/rle.hip): integer arithmetic, bit-reproducible -------------------------------------

RLE_STATS = {'launches': 0, 'retries': 0}      # calls of xmem_rle_encode / frames encoded again because their events did not fit
RLE_STRING_STATS = {'launches': 0, 'retries': 0}       # calls of xmem_rle_compress / frames compressed again: their characters did not fit


def _exact_fit(again, stats, split, rec, masks, K, capacity, refusal):
    """The wait=True tail of rle_encode and mask_polygons: the device record `rec` of `masks` on the host as (meta, list of each
    frame's words).  The counts in `meta` are the true ones, so a frame whose words did not fit `capacity` goes through `again`
    (the caller, by its name in this module) once more on its own with room for all of them, and must count the same."""
    B = masks.shape[0] if masks.dim() == 3 else 1
    meta, words = split(rec.cpu().numpy(), B, K, capacity)
    out = []
    for b in range(B):
        total = int(meta[b, :, 0].sum())
        if total > capacity:
            stats['retries'] += 1
            meta_b, words_b = again(masks[b:b + 1], K, capacity=total)
            if (meta_b[0] != meta[b]).any():
                raise RuntimeError(refusal)
            out.append(words_b[0])
        else:
            out.append(words[b, :total].copy())
    return meta.copy(), out


def rle_encode(masks, K, capacity=None, wait=True):
    """Run boundaries, areas and boxes of the labels 1..K of uint8 label maps `masks` [H,W] or [B,H,W] in the COCO order x * H + y
    (xmem2_amd/rle.py has the definitions).  `capacity`: events per frame there is room for (default `rle.default_capacity`).
    wait=True: returns (meta int32 [B,K,6] = events, area, x0, y0, x1, y1 per label, list of B uint32 arrays: the frame's events of
    label 1, 2, ... back to back) on the HOST; a frame whose events did not fit is encoded again with exactly its size - nothing is
    ever cut off.  wait=False: one launch sequence on the current stream and no synchronisation; returns the int32 device tensor
    `rle.split_record(., B, K, capacity)` takes apart, whose true counts tell the caller which frames to encode again."""
    from . import rle
    masks = _req_u8(masks, 'masks', frames='B')
    K = _int_arg('rle_encode', 'K', K, 1, 254, numpy_ok=False)
    B, H, W = _map_dims(masks, 'rle_encode')
    capacity = rle.default_capacity(H, W) if capacity is None else int(capacity)
    if capacity < 1:
        raise ValueError(f'rle_encode: capacity = {capacity} must be at least 1')
    lib = load()
    rec = torch.empty(B * K * rle.META + B * capacity, dtype=torch.int32, device=masks.device)
    ws = workspace(lib.xmem_rle_workspace_bytes(B, W, K), masks.device, 'rle')
    RLE_STATS['launches'] += 1
    check(lib.xmem_rle_encode(ptr(masks), B, H, W, K, capacity, ptr(rec), C.c_void_p(rec.data_ptr() + 4 * B * K * rle.META), ptr(ws),
                              ws.numel(), stream_ptr()))
    if not wait:
        return rec
    return _exact_fit(rle_encode, RLE_STATS, rle.split_record, rec, masks, K, capacity, 'rle_encode: a frame encoded again gave other counts')


def _frames_fit(B, fn):
    if B > 65535:
        raise ValueError(f'{fn}: {B} frames in one launch, at most 65535')


def _record_frames(record, K, capacity, fn):
    """B of `record`, the int32 device tensor of rle_encode(wait=False) with this `capacity`: a whole number of frames of
    K * META + capacity words, at most 65535"""
    from . import rle
    if not torch.is_tensor(record) or not record.is_cuda or record.dtype != torch.int32 or record.dim() != 1 or not record.is_contiguous():
        raise RuntimeError('record: expected the contiguous int32 CUDA (HIP) tensor of rle_encode(wait=False) - xmem2_amd has no CPU path')
    if capacity is None:
        raise ValueError(f'{fn}: a device record needs the capacity it was encoded with')
    per_frame = K * rle.META + capacity
    B = record.numel() // per_frame
    if B < 1 or B * per_frame != record.numel():
        raise ValueError(f'{fn}: a record of {record.numel()} words is not a whole number of frames of K = {K}, capacity = {capacity}')
    _frames_fit(B, fn)
    return B


def rle_decode(record, H, W, K, capacity=None, values=None, out=None, check=True):
    """The inverse of `rle_encode`: uint8 label maps [B,H,W] on the device from a record.  `record`: the int32 device tensor
    `rle_encode(..., wait=False)` returns (B follows from its length; `capacity` is the one it was encoded with; no host step), or a
    host pair (meta [B,K,>=1] whose field 0 is the rows' event counts, list of B packed event arrays) as wait=True returns, which is
    packed and uploaded - with the capacity the frames need unless `capacity` says otherwise (events beyond it are cut, as the
    encoder does not write them).  A pixel gets values[k - 1] (default k) of the highest row that contains it, else 0.
    check=True reads the per-frame status (one synchronisation) and raises for a frame whose counts exceed the capacity;
    check=False returns (masks, status int32 [B] on the device) without synchronising: such a frame is all zero, status 1."""
    import numpy as np
    from . import rle
    H, W, K = (_int_arg('rle_decode', n, v, 1, top) for n, v, top in (('H', H, 16384), ('W', W, 16384), ('K', K, 254)))
    if capacity is not None:
        capacity = _int_arg('rle_decode', 'capacity', capacity, 1)
    if torch.is_tensor(record):
        B, device = _record_frames(record, K, capacity, 'rle_decode'), record.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError('rle_decode: needs an MI355X (HIP) device - xmem2_amd has no CPU path')
        meta, events = record
        meta = np.asarray(meta)
        if meta.ndim != 3 or meta.shape[0] < 1 or meta.shape[1] != K or meta.shape[2] < 1 or len(events) != meta.shape[0]:
            raise ValueError(f'rle_decode: expected (meta [B, {K}, >= 1], B event arrays), got meta {meta.shape} and {len(events)} arrays')
        B = meta.shape[0]
        events = [np.asarray(e).reshape(-1) for e in events]
        if capacity is None:
            capacity = max(1, max(len(e) for e in events))
        buf = np.zeros(B * K * rle.META + B * capacity, np.int32)
        m, ev = rle.split_record(buf, B, K, capacity)
        m[:, :, 0] = meta[:, :, 0]
        for b, e in enumerate(events):
            n = min(len(e), capacity)
            ev[b, :n] = e[:n]
        device = values.device if torch.is_tensor(values) and values.is_cuda else torch.device('cuda', torch.cuda.current_device())
        record = torch.from_numpy(buf).to(device)
        _frames_fit(B, 'rle_decode')
    if values is not None:
        if not torch.is_tensor(values):
            v = np.asarray(values)
            if v.shape != (K,) or v.dtype.kind not in 'iu' or (v.size and (v.min() < 0 or v.max() > 255)):
                raise ValueError(f'rle_decode: values must be {K} integers in 0..255')
            values = torch.from_numpy(v.astype(np.uint8))
        if values.dtype != torch.uint8 or tuple(values.shape) != (K,):
            raise ValueError(f'rle_decode: values must be uint8 [{K}]')
        values = values.to(device).contiguous()
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.uint8, device=device)
    elif not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W) or not out.is_contiguous():
        raise RuntimeError(f'rle_decode: out must be a contiguous uint8 CUDA (HIP) tensor {(B, H, W)}')
    status = torch.empty(B, dtype=torch.int32, device=device)
    _lib.check(load().xmem_rle_decode(ptr(record), C.c_void_p(record.data_ptr() + 4 * B * K * rle.META), B, H, W, K, capacity,
                                      ptr(values) if values is not None else None, ptr(out), ptr(status), stream_ptr()))
    if not check:
        return out, status
    bad = torch.nonzero(status).reshape(-1).tolist()
    if bad:
        raise RuntimeError(f'rle_decode: the events of frame(s) {bad} do not fit the capacity {capacity}')
    return out


def rle_compress(record, H, W, K, capacity, char_capacity=None, wait=True):
    """The compressed COCO strings (`rle.compress_counts` is the definition) of a record: `record` is the int32 device tensor
    `rle_encode(..., wait=False)` returns, `capacity` the one it was encoded with, `char_capacity` the bytes per frame there is room
    for (default `rle.default_char_capacity`).  wait=False: one launch sequence on the current stream and no synchronisation; returns
    the uint8 device tensor [B * K int32 string lengths | B * char_capacity characters] that `rle.split_string_record(., B, K,
    char_capacity)` takes apart - the lengths are the true ones, -1 in a frame whose EVENTS did not fit `capacity`.  wait=True: returns
    a list of B lists of K str on the HOST ('' for a label without event); a frame whose characters did not fit is compressed again
    with exactly its size; a frame whose events did not fit the record is None - only the masks can be encoded again."""
    from . import rle
    H, W, K = (_int_arg('rle_compress', n, v, 1, top) for n, v, top in (('H', H, 16384), ('W', W, 16384), ('K', K, 254)))
    capacity = _int_arg('rle_compress', 'capacity', capacity, 1, 1 << 28)
    B = _record_frames(record, K, capacity, 'rle_compress')
    char_capacity = rle.default_char_capacity(H, W, capacity) if char_capacity is None \
        else _int_arg('rle_compress', 'char_capacity', char_capacity, 1, (1 << 31) - 1)
    lib = load()
    out = torch.zeros(4 * B * K + B * char_capacity, dtype=torch.uint8, device=record.device)
    ws = workspace(lib.xmem_rle_compress_workspace_bytes(B, K, capacity), record.device, 'rle')
    RLE_STRING_STATS['launches'] += 1
    check(lib.xmem_rle_compress(ptr(record), C.c_void_p(record.data_ptr() + 4 * B * K * rle.META), B, H, W, K, capacity, char_capacity,
                                ptr(out), C.c_void_p(out.data_ptr() + 4 * B * K), ptr(ws), ws.numel(), stream_ptr()))
    if not wait:
        return out
    str_len, chars = rle.split_string_record(out.cpu().numpy(), B, K, char_capacity)
    strings = []
    for b in range(B):
        if (str_len[b] < 0).any():
            strings.append(None)
            continue
        total = int(str_len[b].sum())
        if total > char_capacity:                                 # the lengths are the true ones: once more, with room for all of them
            RLE_STRING_STATS['retries'] += 1
            meta_b = record[b * K * rle.META:(b + 1) * K * rle.META]
            ev_b = record[B * K * rle.META + b * capacity:B * K * rle.META + (b + 1) * capacity]
            again = rle_compress(torch.cat([meta_b, ev_b]), H, W, K, capacity, char_capacity=total)[0]
            if [len(v) for v in again] != str_len[b].tolist():
                raise RuntimeError('rle_compress: a frame compressed again gave other lengths')
            strings.append(again)
        else:
            strings.append(rle.label_strings(str_len[b], chars[b]))
    return strings


def rle_string_offsets(string_record, B, K, char_capacity):
    """The device pair (chars, str_ofs int32 [B, K + 1]) `rle_decompress` takes, from the tensor `rle_compress(..., wait=False)` returned:
    a cumulative sum of the lengths on the device, no host step.  A frame with lengths of -1 (its events did not fit) has no string."""
    if not string_record.is_cuda or string_record.dtype != torch.uint8 or string_record.numel() != 4 * B * K + B * char_capacity:
        raise ValueError(f'rle_string_offsets: expected the uint8 device tensor of rle_compress(wait=False) for {B} frames, K = {K}, '
                         f'char_capacity = {char_capacity}')
    if B * char_capacity >= 1 << 31:
        raise ValueError('rle_string_offsets: the characters do not fit int32 offsets')
    lens = string_record[:4 * B * K].view(torch.int32).reshape(B, K).clamp(min=0)
    ofs = torch.zeros((B, K + 1), dtype=torch.int32, device=string_record.device)
    ofs[:, 1:] = torch.cumsum(lens, 1).clamp(max=char_capacity)       # a frame that did not fit: its tail reads as malformed, in range
    ofs += torch.arange(B, dtype=torch.int32, device=string_record.device)[:, None] * char_capacity
    return string_record[4 * B * K:], ofs


def rle_decompress(strings, H, W, K, capacity=None, check=True):
    """Compressed COCO strings (`rle.decompress_counts` is the definition) -> the int32 device record `rle_decode(record, H, W, K,
    capacity)` takes (field 0 of `meta` holds the rows' event counts, the rest is 0).  `strings`: a list of B frames, each a list of K
    str / ASCII bytes / None (a row without string) - joined into one byte buffer and an offsets table and uploaded, with the
    capacity every frame is sure to fit (its number of characters) unless `capacity` says otherwise; or the device pair (chars uint8
    [n], str_ofs int32 [B, K + 1]) of `rle_string_offsets`, which needs `capacity`.  check=True reads the status (one synchronisation)
    and raises ValueError naming the frame and row of a string that is malformed (1), describes no H x W plane (2) or belongs to a
    frame whose events exceed the capacity (3); check=False returns (record, status int32 [B, K] on the device) without
    synchronising: such a row has no events in the record, its neighbours are exact."""
    import numpy as np
    from . import rle
    H, W, K = (_int_arg('rle_decompress', n, v, 1, top) for n, v, top in (('H', H, 16384), ('W', W, 16384), ('K', K, 254)))
    if capacity is not None:
        capacity = _int_arg('rle_decompress', 'capacity', capacity, 1, (1 << 31) - 1)
    if isinstance(strings, tuple) and len(strings) == 2 and torch.is_tensor(strings[0]):
        chars, ofs = strings
        if not chars.is_cuda or chars.dtype != torch.uint8 or chars.dim() != 1 or not chars.is_contiguous():
            raise RuntimeError('rle_decompress: chars must be a contiguous uint8 CUDA (HIP) tensor - xmem2_amd has no CPU path')
        if (not torch.is_tensor(ofs) or ofs.device != chars.device or ofs.dtype != torch.int32 or ofs.dim() != 2 or ofs.shape[1] != K + 1
                or not ofs.is_contiguous()):
            raise ValueError(f'rle_decompress: str_ofs must be a contiguous int32 tensor [B, {K + 1}] on the device of chars')
        if capacity is None:
            raise ValueError('rle_decompress: a device record needs a capacity')
        B, device = ofs.shape[0], chars.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError('rle_decompress: needs an MI355X (HIP) device - xmem2_amd has no CPU path')
        B = len(strings)
        if B < 1:
            raise ValueError('rle_decompress: no frames')
        table = np.zeros((B, K + 1), np.int64)
        parts = []
        for b, frame in enumerate(strings):
            if len(frame) != K:
                raise ValueError(f'rle_decompress: frame {b} has {len(frame)} rows, expected {K}')
            for k, v in enumerate(frame):
                if v is None:
                    continue
                if isinstance(v, str):
                    try:
                        v = v.encode('ascii')
                    except UnicodeEncodeError:
                        raise ValueError(f'rle_decompress: frame {b}, row {k}: a character outside 48..111') from None
                if not isinstance(v, (bytes, bytearray)):
                    raise ValueError(f'rle_decompress: frame {b}, row {k}: expected str, bytes or None, got {type(v).__name__}')
                if len(v) == 0:
                    raise ValueError(f'rle_decompress: frame {b}, row {k}: an empty string holds no counts')
                table[b, k] = len(v)
                parts.append(v)
        per_frame = table.sum(1)
        if capacity is None:
            capacity = max(1, int(per_frame.max()))                   # every value takes a character: events < characters
        table = np.concatenate((np.zeros((B, 1), np.int64), np.cumsum(table[:, :K], 1)), 1) + (np.cumsum(per_frame) - per_frame)[:, None]
        if int(table[-1, -1]) >= 1 << 31:
            raise ValueError('rle_decompress: more than 2^31 characters in one launch')
        device = torch.device('cuda', torch.cuda.current_device())
        joined = b''.join(parts) or b'0'                              # never an empty allocation; no offset reaches the filler
        chars = torch.frombuffer(bytearray(joined), dtype=torch.uint8).to(device)
        ofs = torch.from_numpy(table.astype(np.int32)).to(device)
    if B < 1 or B > 65535:
        raise ValueError(f'rle_decompress: {B} frames in one launch, 1..65535 fit')
    n_chars = chars.numel()
    lib = load()
    record = torch.zeros(B * K * rle.META + B * capacity, dtype=torch.int32, device=device)
    status = torch.empty((B, K), dtype=torch.int32, device=device)
    ws = workspace(lib.xmem_rle_decompress_workspace_bytes(B, K), device, 'rle')
    with torch.cuda.device(device):
        _lib.check(lib.xmem_rle_decompress(ptr(chars), n_chars, ptr(ofs), B, H, W, K, capacity, ptr(record),
                                           C.c_void_p(record.data_ptr() + 4 * B * K * rle.META), ptr(status), ptr(ws), ws.numel(),
                                           stream_ptr()))
    if not check:
        return record, status
    bad = status.cpu().numpy()
    if bad.any():
        b, k = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f'rle_decompress: frame {b}, row {k}: {rle.STRING_STATUS[int(bad[b, k])]}')
    return record


# ---- f-BRS click refinement (csrc/brs.hip): every kernel bit-reproducible --------------------------------------------

BRS_RECORD = 8          # floats of the evaluation record ahead of the gradient (include/xmem_hip.h, xmem_brs_loss)


def brs_affine(x, scale_bias, out=None):
    """y = x (1 + s[c]) + b[c] on contiguous NHWC x [B,h,w,C]; scale_bias [2C] float32 on the device (scale then bias)."""
    B, h, w, Cc = _req(x, 'brs_affine input').shape
    if not x.is_contiguous() or _req(scale_bias, 'scale_bias').numel() != 2 * Cc or not scale_bias.is_contiguous():
        raise RuntimeError(f'brs_affine: expected a contiguous input and {2 * Cc} scale / bias values')
    if out is None:
        out = torch.empty_like(x)
    if tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
        raise RuntimeError('brs_affine: out must be contiguous and shaped like the input')
    check(load().xmem_brs_affine_nhwc(ptr(x), ptr(scale_bias), ptr(_req(out, 'out')), B, h, w, Cc, stream_ptr()))
    return out


def relu_gate(y, g, out=None):
    """g where the kept ReLU output y is positive, else 0 (the ReLU's adjoint); out may be g."""
    if tuple(_req(y, 'relu_gate y').shape) != tuple(_req(g, 'relu_gate g').shape) or not y.is_contiguous() or not g.is_contiguous():
        raise RuntimeError('relu_gate: y and g must be contiguous tensors of one shape')
    if out is None:
        out = torch.empty_like(g)
    if tuple(out.shape) != tuple(g.shape) or not out.is_contiguous():
        raise RuntimeError('relu_gate: out must be contiguous and shaped like g')
    check(load().xmem_relu_gate_nhwc(ptr(y), ptr(g), ptr(_req(out, 'out')), g.numel(), stream_ptr()))
    return out


def relu_gate_outer(y, g1, w, out=None):
    """out[..., c] = y[..., c] > 0 ? g1[...] w[c] : 0 for y [B,h,w,C], g1 [B,h,w] (or [B,h,w,1]) and w [C]: the adjoint of a
    single-output pointwise layer, gated by the ReLU that produced its input y."""
    Cc = _req(y, 'relu_gate_outer y').shape[-1]
    pixels = y.numel() // Cc
    if _req(g1, 'g1').numel() != pixels or _req(w, 'w').numel() != Cc or not (y.is_contiguous() and g1.is_contiguous() and w.is_contiguous()):
        raise RuntimeError('relu_gate_outer: expected contiguous y [..., C], g1 with one value per pixel and w [C]')
    if out is None:
        out = torch.empty_like(y)
    if tuple(out.shape) != tuple(y.shape) or not out.is_contiguous():
        raise RuntimeError('relu_gate_outer: out must be contiguous and shaped like y')
    check(load().xmem_relu_gate_outer_nhwc(ptr(y), ptr(g1), ptr(w), ptr(_req(out, 'out')), pixels, Cc, stream_ptr()))
    return out


def brs_loss(logits, H, W, rects, count, last_mask, mask, record, dlogit=None):
    """BRSMaskLoss on the align_corners upsample of logits [B,h4,w4] to H x W with the evaluation's bookkeeping.  rects [B,cap,5] int32
    (r0, r1, c0, c1, positive) and count [1] int32 on the device; last_mask (read) and mask (written: upsampled logit > 0) uint8
    [B,H,W]; record: at least BRS_RECORD floats, written as include/xmem_hip.h lays them out -> dlogit [B,h4,w4]."""
    B, h4, w4 = _req(logits, 'logits').shape
    if not logits.is_contiguous() or B not in (1, 2):
        raise RuntimeError(f'brs_loss: expected contiguous logits [1 or 2, h4, w4], got {tuple(logits.shape)}')
    if not rects.is_cuda or rects.dtype != torch.int32 or rects.dim() != 3 or rects.shape[0] != B or rects.shape[2] != 5 or not rects.is_contiguous():
        raise RuntimeError(f'brs_loss: rects must be a contiguous int32 [{B}, cap, 5] tensor on the device')
    if not count.is_cuda or count.dtype != torch.int32 or count.numel() != 1:
        raise RuntimeError('brs_loss: count must be one int32 on the device')
    for name, m in (('last_mask', last_mask), ('mask', mask)):
        if not m.is_cuda or m.dtype != torch.uint8 or tuple(m.shape) != (B, int(H), int(W)) or not m.is_contiguous():
            raise RuntimeError(f'brs_loss: {name} must be a contiguous uint8 [{B}, {H}, {W}] tensor on the device')
    if mask.data_ptr() == last_mask.data_ptr():
        raise RuntimeError('brs_loss: mask and last_mask must be different buffers')
    if _req(record, 'record').numel() < BRS_RECORD or not record.is_contiguous():
        raise RuntimeError(f'brs_loss: record needs {BRS_RECORD} contiguous floats')
    if dlogit is None:
        dlogit = torch.empty_like(logits)
    if tuple(_req(dlogit, 'dlogit').shape) != (B, h4, w4) or not dlogit.is_contiguous():
        raise RuntimeError('brs_loss: dlogit must be contiguous and shaped like the logits')
    lib, cap = load(), rects.shape[1]
    need = lib.xmem_brs_loss_workspace_bytes(B, cap)
    ws = workspace(need, logits.device, 'brs_loss')
    check(lib.xmem_brs_loss(ptr(logits), B, h4, w4, int(H), int(W), ptr(rects), ptr(count), cap, ptr(last_mask), ptr(mask), ptr(record),
                            ptr(dlogit), ptr(ws), need, stream_ptr()))
    return dlogit


def brs_param_grad(g, x, scale_bias, record, grad, reg_weight=1e-3, reg_bias_weight=10.0):
    """The feature gradient g and the un-scaled features x (contiguous NHWC [B,h,w,C]) -> grad [2C] (sum g x + 2 reg_weight s | sum g +
    2 reg_weight reg_bias_weight b) and record[3] = record[0] + the regulariser: the objective's value."""
    B, h, w, Cc = _req(g, 'brs_param_grad g').shape
    if tuple(_req(x, 'x').shape) != (B, h, w, Cc) or not g.is_contiguous() or not x.is_contiguous():
        raise RuntimeError('brs_param_grad: g and x must be contiguous tensors of one shape')
    if _req(scale_bias, 'scale_bias').numel() != 2 * Cc or _req(grad, 'grad').numel() != 2 * Cc or not grad.is_contiguous() \
            or not scale_bias.is_contiguous():
        raise RuntimeError(f'brs_param_grad: scale_bias and grad hold {2 * Cc} contiguous floats')
    if _req(record, 'record').numel() < BRS_RECORD or not record.is_contiguous():
        raise RuntimeError(f'brs_param_grad: record needs {BRS_RECORD} contiguous floats')
    lib = load()
    need = lib.xmem_brs_param_grad_workspace_bytes(Cc)
    ws = workspace(need, g.device, 'brs_param')
    check(lib.xmem_brs_param_grad(ptr(g), ptr(x), B, h, w, Cc, ptr(scale_bias), float(reg_weight), float(reg_bias_weight), ptr(record),
                                  ptr(grad), ptr(ws), need, stream_ptr()))
    return grad


# ---- connected components and mask clean-up (csrc/components.hip, include/xmem_hip_masks.h): integer, bit-reproducible --------

def components(masks, connectivity=8):
    """Connected components of uint8 maps `masks` [H,W] or [N,H,W] on the device -> (root, area), int32 tensors of that shape:
    `mask_cleanup.components_host` per frame, bit for bit (a component is a maximal 4- / 8-connected set of pixels of EQUAL value, 0
    included; root = the row-major index of its first pixel within the frame, area = its size).  A fixed sequence of launches on
    the current stream, no synchronisation."""
    from . import _lib_masks
    if connectivity not in (4, 8):
        raise ValueError(f'components: connectivity = {connectivity!r} must be 4 or 8')
    masks, (N, H, W) = _index_maps(masks, 'components')
    lib = _lib_masks.load()
    root = torch.empty(masks.shape, dtype=torch.int32, device=masks.device)
    area = torch.empty(masks.shape, dtype=torch.int32, device=masks.device)
    ws = workspace(lib.xmem_components_workspace_bytes(N, H, W), masks.device, 'components')
    check(lib.xmem_components(ptr(masks), N, H, W, int(connectivity), ptr(root), ptr(area), ptr(ws), ws.numel(), stream_ptr()))
    return root, area


def clean_masks(masks, min_area=0, max_hole=0, keep_largest=False, out=None):
    """`mask_cleanup.clean_host` of every frame of the uint8 index maps `masks` [H,W] or [N,H,W] on the device -> (out, stats):
    `out` uint8 of that shape (a tensor of the caller's that does not overlap `masks`, or a new one), `stats` int32 [4] or [N,4] on
    the device (components removed, pixels removed, holes filled, pixels filled).  Objects: 8-connected components smaller than
    `min_area`, and with `keep_largest` all but the largest of each label, become 0; then enclosed 4-connected holes of at most
    `max_hole` pixels with one label all around take that label.  One launch sequence on the current stream, no synchronisation."""
    from . import _lib_masks
    from .mask_cleanup import parse_cleanup
    spec = parse_cleanup({'min_area': min_area, 'max_hole': max_hole, 'keep_largest': keep_largest}) or {}
    masks, (N, H, W) = _index_maps(masks, 'clean_masks')
    out = _out_like(out, masks, 'clean_masks')
    lib = _lib_masks.load()
    stats = torch.empty((N, _lib_masks.CLEAN_STATS) if masks.dim() == 3 else (_lib_masks.CLEAN_STATS,), dtype=torch.int32, device=masks.device)
    ws = workspace(lib.xmem_mask_clean_workspace_bytes(N, H, W), masks.device, 'mask_clean')
    check(lib.xmem_mask_clean(ptr(masks), N, H, W, spec.get('min_area', 0), spec.get('max_hole', 0), int(spec.get('keep_largest', False)),
                              ptr(out), ptr(stats), ptr(ws), ws.numel(), stream_ptr()))
    return out, stats


# ---- polygon outlines (csrc/polygons.hip, include/xmem_hip_polygons.h): integer, bit-reproducible ------------------------------

POLY_STATS = {'launches': 0, 'retries': 0}     # calls of xmem_mask_polygons / frames traced again because their corners did not fit


def mask_polygons(masks, K, capacity=None, wait=True):
    """Polygon outlines of the labels 1..K of uint8 index maps `masks` [H,W] or [B,H,W] on the device: `polygons.record_host` per
    frame, word for word (xmem2_amd/polygons.py has the definition).  `capacity`: corners per frame there is room for (default
    `polygons.default_capacity`).  wait=True: returns (meta int32 [B,K,2] = corners, rings per label, list of B uint32 arrays: the
    frame's corner words of label 1, 2, ... back to back, x | y << 16 | first of its ring << 31) on the HOST; a frame whose corners did
    not fit is traced again with exactly its size.  wait=False: one launch sequence on the current stream and no synchronisation;
    returns the int32 device tensor `polygons.split_record(., B, K, capacity)` takes apart, whose true counts tell the caller which
    frames to trace again."""
    from . import _lib_polygons, polygons
    masks = _req_u8(masks, 'masks', frames='B')
    K = _int_arg('mask_polygons', 'K', K, 1, 254, numpy_ok=False)
    B, H, W = _map_dims(masks, 'mask_polygons')
    capacity = polygons.default_capacity(H, W) if capacity is None else int(capacity)
    if not 1 <= capacity <= _lib_polygons.MAX_CAPACITY:
        raise ValueError(f'mask_polygons: capacity = {capacity} must be in 1..{_lib_polygons.MAX_CAPACITY}')
    lib = _lib_polygons.load()
    rec = torch.empty(B * K * polygons.META + B * capacity, dtype=torch.int32, device=masks.device)
    ws = workspace(lib.xmem_mask_polygons_workspace_bytes(B, H, W, K, capacity), masks.device, 'polygons')
    POLY_STATS['launches'] += 1
    check(lib.xmem_mask_polygons(ptr(masks), B, H, W, K, capacity, ptr(rec), C.c_void_p(rec.data_ptr() + 4 * B * K * polygons.META),
                                 ptr(ws), ws.numel(), stream_ptr()))
    if not wait:
        return rec
    return _exact_fit(mask_polygons, POLY_STATS, polygons.split_record, rec, masks, K, capacity,
                      'mask_polygons: a frame traced again gave other counts')


# ---- polygons filled back into masks (csrc/polygons_fill.hip, include/xmem_hip_raster.h): integer, bit-reproducible ------------

FILL_STATS = {'launches': 0}                   # calls of xmem_polygons_fill
FILL_WORKSPACE_CAP = 256 << 20                 # bytes of toggle bit-planes one call may ask for: larger jobs go in chunks of frames and rows
FILL_MAX_ROWS = 254


def fill_edges(edges, plane, N, H, W, R, values=None, frac_bits=8, out=None, overlay=False, check=True):
    """`xmem_polygons_fill` on a packed edge list: `edges` int32 [E,4] = xa, ya, xb, yb in units of 1 / 2**frac_bits pixel with
    ya < yb, `plane` int32 [E] = frame * R + row, as `polygons.pack_edges` gives them (host arrays; uploaded once).  `R` may exceed
    254 and the planes `FILL_WORKSPACE_CAP`: the rows are then layered in chunks, lowest first, each over the ones before it, and the
    frames go in chunks - every edge still goes up once, sorted by chunk.  Returns what `fill_polygons` returns."""
    import numpy as np
    from . import _lib_raster
    N, H, W, R, frac_bits = (_int_arg('fill_polygons', n, v, low, top) for n, v, low, top in (
        ('N', N, 1, 1 << 30), ('H', H, 1, 16384), ('W', W, 1, 16384), ('R', R, 1, 1 << 20), ('frac_bits', frac_bits, 0, _lib_raster.MAX_FRAC_BITS)))
    edges, plane = np.ascontiguousarray(edges, np.int32).reshape(-1, 4), np.ascontiguousarray(plane, np.int32).reshape(-1)
    if len(edges) != len(plane):
        raise ValueError(f'fill_polygons: {len(edges)} edges, {len(plane)} plane indices')
    if values is None:
        if R > 255:
            raise ValueError(f'fill_polygons: {R} rows need a values table, row + 1 does not fit a byte')
        values = np.arange(1, R + 1)
    values = np.asarray(values)
    if values.shape != (R,) or values.dtype.kind not in 'iu' or values.min() < 0 or values.max() > 255:
        raise ValueError(f'fill_polygons: values must be {R} integers in 0..255')
    if out is None:
        if overlay:
            raise ValueError('fill_polygons: overlay needs the planes to lay over (out)')
        if not torch.cuda.is_available():
            raise RuntimeError('fill_polygons: needs an MI355X (HIP) device - xmem2_amd has no CPU path')
        out = torch.empty((N, H, W), dtype=torch.uint8, device=torch.device('cuda', torch.cuda.current_device()))
    elif not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W) or not out.is_contiguous():
        raise RuntimeError(f'fill_polygons: out must be a contiguous uint8 CUDA (HIP) tensor {(N, H, W)} - xmem2_amd has no CPU path')
    device = out.device
    lib = _lib_raster.load()
    per_plane = 4 * H * ((W + 1 + 31) // 32)
    cap = max(int(FILL_WORKSPACE_CAP), per_plane)
    rc = min(FILL_MAX_ROWS, R, cap // per_plane)                      # rows, then frames, of one call
    fc = min(N, 65535, max(1, cap // (per_plane * rc)))
    n_rc, n_fc = -(-R // rc), -(-N // fc)
    # an edge whose plane is outside [0, N R) keeps an index no call accepts, and goes with the first call: the device counts it
    ok = (plane >= 0) & (plane < N * R)
    f, row = np.where(ok, plane // R, 0), np.where(ok, plane % R, 0)
    chunk = (row // rc) * n_fc + f // fc
    local = np.where(ok, (f % fc) * np.minimum(rc, R - row // rc * rc) + row % rc, -1).astype(np.int32)
    order = np.argsort(chunk, kind='stable')
    starts = np.searchsorted(chunk[order], np.arange(n_rc * n_fc + 1))
    E = len(edges)
    up = torch.from_numpy(np.concatenate([edges[order].reshape(-1), local[order], np.zeros(1, np.int32)])).to(device)
    table = torch.from_numpy(values.astype(np.uint8)).to(device)
    status = torch.empty((n_rc * n_fc, _lib_raster.FILL_STATUS), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        for i in range(n_rc):
            rows = min(rc, R - i * rc)
            for j in range(n_fc):
                nf = min(fc, N - j * fc)
                a, b = int(starts[i * n_fc + j]), int(starts[i * n_fc + j + 1])
                ws = workspace(lib.xmem_polygons_fill_workspace_bytes(nf, H, W, rows), device, 'polygons_fill')
                FILL_STATS['launches'] += 1
                _lib.check(lib.xmem_polygons_fill(C.c_void_p(up.data_ptr() + 16 * a), C.c_void_p(up.data_ptr() + 16 * E + 4 * a), b - a, nf, H, W,
                                                  rows, frac_bits, C.c_void_p(table.data_ptr() + i * rc), int(bool(overlay) or i > 0),
                                                  C.c_void_p(out.data_ptr() + j * fc * H * W), C.c_void_p(status.data_ptr() + 8 * (i * n_fc + j)),
                                                  ptr(ws), ws.numel(), stream_ptr()))
    status = status[0] if len(status) == 1 else status.sum(0, dtype=torch.int32)
    if not check:
        return out, status
    bad = status.cpu().tolist()
    if any(bad):
        raise ValueError(f'fill_polygons: {bad[0]} edges name a plane outside the {N} x {R} there are, {bad[1]} have a coordinate beyond '
                         f'{_lib_raster.COORD_BOUND} / 2^{frac_bits} pixels; they were skipped')
    return out


def fill_polygons(frames, H, W, values=None, frac_bits=8, out=None, overlay=False, check=True):
    """Polygons -> uint8 index maps [N,H,W] on the device, `polygons.fill_rows_host` per frame, byte for byte.  `frames`: a list of N
    frames, each a list of rows, each a list of rings ((x, y) lists or flat lists, ints or floats); R is the longest frame's number
    of rows.  A row is filled even-odd on its own; a pixel takes values[row] (default row + 1) of the highest row that contains it,
    else 0 - or, with overlay=True, what `out` held.  The host packs the edges (`polygons.pack_edges`, work per vertex), uploads them
    once and launches; more than 254 rows, or more bit-planes than `FILL_WORKSPACE_CAP` bytes, go in chunks (`fill_edges`).
    check=True reads the status (one synchronisation) and raises if an edge was skipped; check=False returns (masks, status int32 [2]
    on the device) without synchronising."""
    from . import polygons
    frames = list(frames)
    if not frames:
        raise ValueError('fill_polygons: no frames')
    R = max(1, max(len(rows) for rows in frames))
    edges, plane = polygons.pack_edges(frames, R, frac_bits)
    return fill_edges(edges, plane, len(frames), H, W, R, values=values, frac_bits=frac_bits, out=out, overlay=overlay, check=check)


# ---- signed distances, mattes, trimaps, grow / shrink (csrc/matte.hip, include/xmem_hip_matte.h): integer, bit-reproducible -------

def _matte_labels(fn, K, R):
    from . import _lib_matte
    for name, v, top in (('K', K, _lib_matte.MAX_LABELS), ('R', R, _lib_matte.MAX_R)):
        _int_arg(fn, name, v, 1, top, numpy_ok=False)


def signed_edt_sq(masks, K, R):
    """`matte.signed_d2_host(m, k, R)` of every frame of the uint8 index maps `masks` [H,W] or [N,H,W] and every label k = 1..K on the
    device -> int32 [K,H,W] or [N,K,H,W]: the squared distance to the nearest pixel on the other side of `m == k`, capped at
    (R + 1)^2, positive inside the label; nothing exists outside the image.  Two launches on the current stream, no synchronisation."""
    from . import _lib_matte
    _matte_labels('signed_edt_sq', K, R)
    masks, (N, H, W) = _index_maps(masks, 'signed_edt_sq')
    lib = _lib_matte.load()
    out = torch.empty((N, K, H, W) if masks.dim() == 3 else (K, H, W), dtype=torch.int32, device=masks.device)
    ws = workspace(lib.xmem_signed_edt_workspace_bytes(N, H, W, K), masks.device, 'matte')
    check(lib.xmem_signed_edt(ptr(masks), N, H, W, K, R, ptr(out), ptr(ws), ws.numel(), stream_ptr()))
    return out


def mask_mattes(masks, K, tables, R):
    """Look-ups in that distance: `tables` uint8 [T, 2 (R + 1)^2 + 1] on the masks' device (`matte.feather_table`, `matte.trimap_table`,
    T in 1..4) -> uint8 [T,K,H,W] or [T,N,K,H,W] = tables[t][s2 + (R + 1)^2].  One distance computation serves all T tables and no
    int32 plane is written.  Two launches on the current stream, no synchronisation."""
    from . import _lib_matte
    _matte_labels('mask_mattes', K, R)
    masks, (N, H, W) = _index_maps(masks, 'mask_mattes')
    if not torch.is_tensor(tables) or tables.dtype != torch.uint8 or tables.dim() != 2 or tables.device != masks.device:
        raise RuntimeError('mask_mattes: tables must be a uint8 tensor [T, 2 (R + 1)^2 + 1] on the masks\' device')
    T, length = tables.shape
    if not 1 <= T <= _lib_matte.MAX_TABLES or length != 2 * (R + 1) ** 2 + 1:
        raise ValueError(f'mask_mattes: tables {tuple(tables.shape)}: expected 1..{_lib_matte.MAX_TABLES} rows of {2 * (R + 1) ** 2 + 1} for R = {R}')
    tables = tables.contiguous()
    lib = _lib_matte.load()
    out = torch.empty((T, N, K, H, W) if masks.dim() == 3 else (T, K, H, W), dtype=torch.uint8, device=masks.device)
    ws = workspace(lib.xmem_mask_matte_workspace_bytes(N, H, W, K), masks.device, 'matte')
    check(lib.xmem_mask_matte(ptr(masks), N, H, W, K, R, ptr(tables), T, ptr(out), ptr(ws), ws.numel(), stream_ptr()))
    return out


def grow_masks(masks, r, out=None):
    """`matte.grow_host(m, r)` of every frame of the uint8 index maps `masks` [H,W] or [N,H,W] on the device -> `out`, uint8 of that
    shape (a tensor of the caller's that does not overlap `masks`, or a new one).  r > 0 grows every object by r pixels into the
    background - objects never eat one another, ties go to the smaller label -, r < 0 shrinks; |r| in 1..127.  Two launches on the
    current stream, no synchronisation."""
    from . import _lib_matte
    from .matte import radius2
    r2, shrink = radius2(r)
    if r2 < 1:
        raise ValueError(f'grow_masks: r = {r!r} changes nothing (|r| must be at least 1)')
    masks, (N, H, W) = _index_maps(masks, 'grow_masks')
    out = _out_like(out, masks, 'grow_masks')
    lib = _lib_matte.load()
    ws = workspace(lib.xmem_mask_grow_workspace_bytes(N, H, W), masks.device, 'matte')
    check(lib.xmem_mask_grow(ptr(masks), N, H, W, r2, int(shrink), ptr(out), ptr(ws), ws.numel(), stream_ptr()))
    return out


# ---- temporal majority vote (csrc/temporal.hip, include/xmem_hip_temporal.h): integer, bit-reproducible ---------------------------

def temporal_mode_ring(ring, T, t0, n, radius, flags, out=None, changed=None):
    """`temporal.mode_host` of the frames t0 .. t0 + n - 1 of a video of T frames whose frame t lives in slot t % ring.shape[0] of
    `ring`, uint8 [slots,H,W] on the device; `flags` uint8 [T] on that device (1 present, 2 locked: `temporal.frame_flags`).
    -> (`out` uint8 [n,H,W] - a tensor of the caller's that does not overlap `ring`, or a new one -, `changed` int32 [n], likewise,
    overwritten).  The ring must hold the frames max(0, t0 - radius) .. min(T - 1, t0 + n - 1 + radius) at once.  One launch on the
    current stream, no synchronisation."""
    from . import _lib_temporal
    ring = _req_u8(ring, 'temporal_mode_ring', frames='slots')
    if ring.dim() != 3 or ring.numel() == 0:
        raise RuntimeError(f'temporal_mode_ring: expected a ring [slots,H,W], got {tuple(ring.shape)}')
    slots, H, W = ring.shape
    T = _int_arg('temporal_mode_ring', 'T', T, 1, 65535)
    n = _int_arg('temporal_mode_ring', 'n', n, 1, T)
    t0 = _int_arg('temporal_mode_ring', 't0', t0, 0, T - n)
    radius = _int_arg('temporal_mode_ring', 'radius', radius, 1, _lib_temporal.MAX_R)
    held = min(T - 1, t0 + n - 1 + radius) - max(0, t0 - radius) + 1
    if slots < held:
        raise ValueError(f'temporal_mode_ring: a ring of {slots} slots cannot hold the {held} frames that frames {t0}..{t0 + n - 1} read')
    if not torch.is_tensor(flags) or flags.dtype != torch.uint8 or tuple(flags.shape) != (T,) or flags.device != ring.device \
            or not flags.is_contiguous():
        raise RuntimeError(f'temporal_mode_ring: flags must be a contiguous uint8 tensor [{T}] on the ring\'s device')
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.uint8, device=ring.device)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (n, H, W) or out.device != ring.device \
            or not out.is_contiguous():
        raise RuntimeError(f'temporal_mode_ring: out must be a contiguous uint8 CUDA (HIP) tensor of shape {(n, H, W)} on the ring\'s device')
    if changed is None:
        changed = torch.empty(n, dtype=torch.int32, device=ring.device)
    elif not torch.is_tensor(changed) or changed.dtype != torch.int32 or tuple(changed.shape) != (n,) or changed.device != ring.device \
            or not changed.is_contiguous():
        raise RuntimeError(f'temporal_mode_ring: changed must be a contiguous int32 tensor [{n}] on the ring\'s device')
    check(_lib_temporal.load().xmem_temporal_mode(ptr(ring), slots, H, W, T, t0, n, radius, ptr(flags), ptr(out), ptr(changed),
                                                  stream_ptr()))
    return out, changed


def temporal_mode(masks, radius, present=None, locked=None, out=None):
    """`temporal.mode_host(masks, radius, present, locked)` on the device: `masks` uint8 [T,H,W], `present` and `locked` bool [T]
    (sequences or arrays on the host; default all present, none locked) -> (`out` uint8 [T,H,W], a tensor of the caller's that does
    not overlap `masks`, or a new one; `changed` int32 [T]).  One launch on the current stream, no synchronisation (the T flag bytes
    are uploaded from pageable memory, as any small argument is)."""
    from .temporal import frame_flags
    masks = _req_u8(masks, 'temporal_mode', frames='T')
    if masks.dim() != 3 or masks.numel() == 0:
        raise RuntimeError(f'temporal_mode: expected masks [T,H,W], got {tuple(masks.shape)}')
    T = masks.shape[0]
    flags = torch.from_numpy(frame_flags(T, present, locked)).to(masks.device)
    return temporal_mode_ring(masks, T, 0, T, radius, flags, out=_out_like(out, masks, 'temporal_mode'))


# ---- block motion and the motion-compensated vote (csrc/motion.hip, include/xmem_hip_motion.h): integer, bit-reproducible ----------

def _given(fn, name, t, dtype, shape, device):
    """`t` for an output of `fn`: the caller's contiguous tensor of that dtype and shape on `device`, or a new one"""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        raise RuntimeError(f'{fn}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on the input\'s device')
    return t


def _ring_args(fn, ring, T, t0, n, radius, flags):
    """the arguments every call on a ring [slots,H,W] shares, checked as `temporal_mode_ring` checks them -> (ring, T, t0, n, radius)"""
    from . import _lib_temporal
    ring = _req_u8(ring, fn, frames='slots')
    if ring.dim() != 3 or ring.numel() == 0:
        raise RuntimeError(f'{fn}: expected a ring [slots,H,W], got {tuple(ring.shape)}')
    T = _int_arg(fn, 'T', T, 1, 65535)
    n = _int_arg(fn, 'n', n, 1, T)
    t0 = _int_arg(fn, 't0', t0, 0, T - n)
    radius = _int_arg(fn, 'radius', radius, 1, _lib_temporal.MAX_R)
    held = min(T - 1, t0 + n - 1 + radius) - max(0, t0 - radius) + 1
    if ring.shape[0] < held:
        raise ValueError(f'{fn}: a ring of {ring.shape[0]} slots cannot hold the {held} frames that frames {t0}..{t0 + n - 1} read')
    if not torch.is_tensor(flags) or flags.dtype != torch.uint8 or tuple(flags.shape) != (T,) or flags.device != ring.device \
            or not flags.is_contiguous():
        raise RuntimeError(f'{fn}: flags must be a contiguous uint8 tensor [{T}] on the ring\'s device')
    return ring, T, t0, n, radius


def luma_u8(rgb, out=None):
    """`motion.luma_host` on the device: uint8 [H,W,3] or [N,H,W,3] -> uint8 [H,W] or [N,H,W].  One launch, no synchronisation."""
    from . import _lib_motion
    if not torch.is_tensor(rgb) or not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.dim() not in (3, 4) or rgb.shape[-1] != 3 or rgb.numel() == 0:
        raise RuntimeError('luma_u8: expected a uint8 CUDA (HIP) tensor [H,W,3] or [N,H,W,3] - xmem2_amd has no CPU path')
    rgb = rgb.contiguous()
    out = _given('luma_u8', 'out', out, torch.uint8, rgb.shape[:-1], rgb.device)
    N, H, W = (1,) + tuple(rgb.shape[:2]) if rgb.dim() == 3 else tuple(rgb.shape[:3])
    check(_lib_motion.load().xmem_luma_u8(ptr(rgb), N, H, W, ptr(out), stream_ptr()))
    return out


def block_motion(cur, ref, search=16, bias=1, vec=None, sad=None):
    """`motion.block_motion_host(cur, ref, search, bias)` on the device: uint8 [H,W] or N independent pairs [N,H,W] -> (vec int8
    [(N,)By,Bx,2] as (dy, dx), sad int32 [(N,)By,Bx]).  One launch, no synchronisation."""
    from . import _lib_motion
    cur = _req_u8(cur, 'block_motion', frames='N')
    ref = _req_u8(ref, 'block_motion', shape=cur.shape)
    if ref.device != cur.device:
        raise RuntimeError('block_motion: cur and ref must be on one device')
    N, H, W = _map_dims(cur, 'block_motion')
    search = _int_arg('block_motion', 'search', search, 1, _lib_motion.MAX_SEARCH)
    bias = _int_arg('block_motion', 'bias', bias, 0, 255)
    lead = tuple(cur.shape[:-2]) + (-(-H // _lib_motion.BLOCK), -(-W // _lib_motion.BLOCK))
    vec = _given('block_motion', 'vec', vec, torch.int8, lead + (2,), cur.device)
    sad = _given('block_motion', 'sad', sad, torch.int32, lead, cur.device)
    check(_lib_motion.load().xmem_block_motion(ptr(cur), ptr(ref), N, H, W, search, bias, ptr(vec), ptr(sad), stream_ptr()))
    return vec, sad


def motion_window(luma, T, t0, n, radius, flags, search=16, bias=1, vec=None, sad=None):
    """The block motion of the frames t0 .. t0 + n - 1 of a video of T frames towards each of their 2 `radius` neighbours, frame t
    in slot t % luma.shape[0] of `luma`, uint8 [slots,H,W]; `flags` as `temporal_mode_ring` takes them -> (vec int8
    [n,2 radius,By,Bx,2], sad int32 [n,2 radius,By,Bx]); entry e is the offset e - radius for e < radius, e - radius + 1 after it.
    sad = -1 and vec = 0 where the neighbour is outside the video or not present and where the frame itself is absent or locked.
    One launch, no synchronisation."""
    from . import _lib_motion
    luma, T, t0, n, radius = _ring_args('motion_window', luma, T, t0, n, radius, flags)
    slots, H, W = luma.shape
    search = _int_arg('motion_window', 'search', search, 1, _lib_motion.MAX_SEARCH)
    bias = _int_arg('motion_window', 'bias', bias, 0, 255)
    lead = (n, 2 * radius, -(-H // _lib_motion.BLOCK), -(-W // _lib_motion.BLOCK))
    vec = _given('motion_window', 'vec', vec, torch.int8, lead + (2,), luma.device)
    sad = _given('motion_window', 'sad', sad, torch.int32, lead, luma.device)
    check(_lib_motion.load().xmem_motion_window(ptr(luma), slots, H, W, T, t0, n, radius, ptr(flags), search, bias, ptr(vec), ptr(sad),
                                                stream_ptr()))
    return vec, sad


def temporal_mode_mc_ring(ring, luma, T, t0, n, radius, flags, search=16, bias=1, max_sad=24, out=None, changed=None, vec=None, sad=None):
    """`temporal.mode_mc_host` of the frames t0 .. t0 + n - 1 of a video of T frames: `ring` (masks) and `luma`, both uint8
    [slots,H,W] with frame t in slot t % slots, `flags` uint8 [T]; everything else as `temporal_mode_ring` -> (out uint8 [n,H,W],
    changed int32 [n]).  `motion_window` (into `vec` and `sad`, the caller's or new ones) and the vote: two launches and a memset node
    on the current stream, no synchronisation."""
    from . import _lib_motion
    ring, T, t0, n, radius = _ring_args('temporal_mode_mc_ring', ring, T, t0, n, radius, flags)
    luma = _req_u8(luma, 'temporal_mode_mc_ring', shape=ring.shape)
    if luma.device != ring.device:
        raise RuntimeError('temporal_mode_mc_ring: the masks and the lumas must be on one device')
    max_sad = _int_arg('temporal_mode_mc_ring', 'max_sad', max_sad, 0, 255)
    slots, H, W = ring.shape
    out = _given('temporal_mode_mc_ring', 'out', out, torch.uint8, (n, H, W), ring.device)
    changed = _given('temporal_mode_mc_ring', 'changed', changed, torch.int32, (n,), ring.device)
    vec, sad = motion_window(luma, T, t0, n, radius, flags, search, bias, vec, sad)
    check(_lib_motion.load().xmem_temporal_mode_mc(ptr(ring), slots, H, W, T, t0, n, radius, ptr(flags), ptr(vec), ptr(sad), max_sad,
                                                   ptr(out), ptr(changed), stream_ptr()))
    return out, changed


def temporal_mode_mc(masks, luma, radius, search=16, bias=1, max_sad=24, present=None, locked=None, out=None):
    """`temporal.mode_mc_host(masks, luma, radius, search, bias, max_sad, present, locked)` on the device: masks and luma uint8
    [T,H,W] -> (out uint8 [T,H,W], changed int32 [T])."""
    from .temporal import frame_flags
    masks = _req_u8(masks, 'temporal_mode_mc', frames='T')
    if masks.dim() != 3 or masks.numel() == 0:
        raise RuntimeError(f'temporal_mode_mc: expected masks [T,H,W], got {tuple(masks.shape)}')
    T = masks.shape[0]
    flags = torch.from_numpy(frame_flags(T, present, locked)).to(masks.device)
    return temporal_mode_mc_ring(masks, luma, T, 0, T, radius, flags, search, bias, max_sad, out=_out_like(out, masks, 'temporal_mode_mc'))


# ---- PNG files built on the device (csrc/png.hip, include/xmem_hip_png.h): integer, bit-reproducible ------------------------------

PNG_STATS = {'launches': 0, 'retries': 0}      # calls of xmem_png_encode / frames encoded again because their file did not fit


def _png_table(t, shape, device, what):
    """a table of png_encode on the device: a uint8 tensor or array of `shape`, or None"""
    if t is None:
        return None
    if not torch.is_tensor(t):
        import numpy as np
        t = torch.from_numpy(np.ascontiguousarray(t))
    if t.dtype != torch.uint8 or tuple(t.shape) != shape:
        raise ValueError(f'png_encode: {what} must be uint8 {list(shape)}')
    return t.to(device).contiguous()


def png_encode(planes, mode, table=None, palette=None, capacity=None, wait=True):
    """`png.encode_host(plane, mode, table, palette)` of uint8 planes [H,W] or [N,H,W] on the device, byte for byte.  `mode`: 'grey'
    (`table`: an optional uint8 [256] byte map), 'palette' (`table`: the byte map, `palette`: uint8 [256, 3]) or 'rgb' (`table`: uint8
    [256, 3]); tables are tensors on the planes' device, or host arrays that are uploaded.  `capacity`: bytes per file there is room
    for (default `png.default_capacity`).  wait=False: one launch sequence on the current stream and no synchronisation; returns the
    uint8 device tensor `png.split_record(., N, capacity)` takes apart, whose meta holds every file's true length.  wait=True: returns
    a list of N `bytes` on the HOST; a frame whose file did not fit is encoded again at its true length - nothing is ever cut off."""
    from . import _lib_png, png
    if mode not in png.MODES:
        raise ValueError(f'png_encode: mode = {mode!r}: expected one of {sorted(png.MODES)}')
    planes = _req_u8(planes, 'png_encode', frames='N')
    N, H, W = _map_dims(planes, 'png_encode')
    _frames_fit(N, 'png_encode')
    if H > png.MAX_SIDE or W > png.MAX_SIDE:
        raise ValueError(f'png_encode: planes of {H} x {W}: at most {png.MAX_SIDE} on a side')
    channels = png.MODES[mode][1]
    if table is None and mode != 'grey':
        raise ValueError(f'png_encode: mode {mode!r} needs a table')
    if (palette is not None) != (mode == 'palette'):
        raise ValueError("png_encode: mode 'palette', and no other, takes a palette")
    table = _png_table(table, (256,) if channels == 1 else (256, 3), planes.device, f'the table of mode {mode!r}')
    palette = _png_table(palette, (256, 3), planes.device, 'the palette')
    capacity = png.default_capacity(H, W, mode) if capacity is None else _int_arg('png_encode', 'capacity', capacity, 1, _lib_png.MAX_CAPACITY)
    lib = _lib_png.load()
    rec = torch.empty(png.record_bytes(N, capacity), dtype=torch.uint8, device=planes.device)
    ws = workspace(lib.xmem_png_workspace_bytes(N, H, W, channels), planes.device, 'png')
    PNG_STATS['launches'] += 1
    check(lib.xmem_png_encode(ptr(planes), N, H, W, _lib_png.COLOR_TYPES[mode], ptr(table), ptr(palette), capacity, ptr(rec),
                              C.c_void_p(rec.data_ptr() + 4 * png.META * N), ptr(ws), ws.numel(), stream_ptr()))
    if not wait:
        return rec
    meta, data = png.split_record(rec.cpu().numpy(), N, capacity)
    files = []
    for n in range(N):
        length = int(meta[n, 0])
        if length > capacity:                                        # the length is the true one: once more, with room for all of it
            PNG_STATS['retries'] += 1
            again = png_encode(planes[n] if planes.dim() == 3 else planes, mode, table, palette, capacity=length)[0]
            if len(again) != length:
                raise RuntimeError('png_encode: a frame encoded again gave another length')
            files.append(again)
        else:
            files.append(data[n, :length].tobytes())
    return files


# ---- confidence and uncertainty maps (csrc/confidence.hip, include/xmem_hip_confidence.h): integer sums, bit-reproducible ----------

def _confidence_out(t, shape, dtype, device, fn, what):
    """an output of confidence_stats: the caller's contiguous tensor of that shape, dtype and device, or a new one"""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        raise RuntimeError(f'{fn}: {what} must be a contiguous {dtype} CUDA (HIP) tensor of shape {tuple(shape)} on the scores\' device')
    return t


def confidence_stats(prob, tau=64, passes=None, want_mask=True, want_plane=False, record=None, mask=None, plane=None):
    """`confidence.stats_host(prob, tau, passes)` on the device, byte for byte: `prob` [C,H,W], float32 with passes=None (the tensor
    `argmax_u8` sees), or the ensemble's uint16 sums of `passes` bytes.  -> (mask uint8 [H,W] == `argmax_u8(prob)`, or None without
    want_mask; plane uint8 [H,W] = 255 - q, or None without want_plane; record int64 [C,4]: area, margin_sum, low, contested per
    class).  `record`, `mask`, `plane`: tensors of the caller's to write into (a given `mask` or `plane` is wanted).  One memset and
    one launch on the current stream, no synchronisation."""
    from . import _lib_confidence
    fn = 'confidence_stats'
    want = torch.float32 if passes is None else torch.uint16
    if not torch.is_tensor(prob) or not prob.is_cuda or prob.dtype != want or prob.dim() != 3 or prob.numel() == 0:
        raise RuntimeError(f'{fn}: expected {want} CUDA (HIP) scores [C,H,W]' + (' with passes' if passes is not None else '')
                           + ' - xmem2_amd has no CPU path')
    prob = prob.contiguous()
    Cc, H, W = prob.shape
    if Cc > _lib_confidence.MAX_C:
        raise ValueError(f'{fn}: {Cc} classes, at most {_lib_confidence.MAX_C} (a label fits a byte)')
    tau = _int_arg(fn, 'tau', tau, 0, _lib_confidence.MAX_TAU)
    record = _confidence_out(record, (Cc, _lib_confidence.RECORD), torch.int64, prob.device, fn, 'record')
    mask = _confidence_out(mask, (H, W), torch.uint8, prob.device, fn, 'mask') if (want_mask or mask is not None) else None
    plane = _confidence_out(plane, (H, W), torch.uint8, prob.device, fn, 'plane') if (want_plane or plane is not None) else None
    lib = _lib_confidence.load()
    if passes is None:
        check(lib.xmem_confidence_f32(ptr(prob), Cc, H, W, tau, ptr(mask), ptr(plane), ptr(record), stream_ptr()))
    else:
        passes = _int_arg(fn, 'passes', passes, 1, _lib_confidence.MAX_PASSES)
        check(lib.xmem_confidence_u16(ptr(prob), passes, Cc, H, W, tau, ptr(mask), ptr(plane), ptr(record), stream_ptr()))
    return mask, plane, record
