"""Float64 references, a-priori round-off bounds, input regimes and the case table of the convolution edge-shape tests.  No GPU.

Written from the contract in include/xmem_hip.h (xmem_conv_desc, the plan codes and their fallbacks), not from the kernels.
Activations are NHWC [B, H, W, C], weights [Cout, KH, KW, Cin], as the C ABI takes them.  tests/test_conv_refs_host.py ties
everything here to a literal loop convolution on the CPU; tests/test_gpu_conv_edges.py holds the kernels to it.

BOUNDS, per output element, u = 2^-24 (fp32, round to nearest).  With x' = relu(x) if relu_in,
    S = sum |x'| |w|  (the same convolution on absolute values),   T = |scale| S + |shift| + |res|.

Direct form, GEMV, streaming pointwise, dilated entry:  (K_pad + splitk + 4) u T.
  An fp32 sum of n terms in ANY order (a chain of fused multiply-adds on the matrix pipe, lane partial sums, a tree over lanes,
  slabs of a split contraction) errs by at most (n - 1) u sum |terms| to first order: each term passes through at most n - 1
  additions, each of relative error u.  The kernels contract K_pad = KH KW Cin rounded up to the k-tile (the padding terms are
  exact zeros but take part in the chain), split-K adds `splitk` additions of slab sums, and the epilogue rounds three more times
  (times scale, plus shift, plus residual); one more is margin for the first-order statement.  Every intermediate is bounded by
  T, so (K_pad + splitk + 4) u T holds for any summation order a kernel may choose.
Split operands ('fp32x'):  (4 K_pad + splitk + 4) u T + 2^-20 |scale| S.
  Each product is four partial products hi hi + hi lo + lo hi + lo lo in the same accumulator: four times the terms.  x = hi + lo
  is represented to 2^-21 relative (header), for both operands: (1 + 2^-21)^2 - 1 < 2^-20 of every |x'| |w|.
Half inputs: the reference takes the half-rounded operands; a product of two halfs has 22 significant bits and is exact in the fp32
  accumulator, so the fp32 bound holds.  A half OUTPUT is rounded once more: + 2^-11 |ref| + 2^-25 (half of the last normal place,
  half of the smallest subnormal).
Winograd F(r x r, 3x3), W_abs = |A^T| ( sum_c (|G| |g_c| |G^T|) o (|B^T| |d_c| |B|) ) |A|  (wino_abs below):
    F(2x2): (Cin + 24) u |scale| W_abs2 + 4 u T            F(4x4): (Cin + 48) u |scale| W_abs4 + 4 u T
  Every rounding of the pipeline acts on a quantity whose propagated magnitude at the output is bounded by W_abs: the operand
  U = G g G^T is rounded once (1), the input transform is two passes of rows of B^T with at most 4 non-zero coefficients
  (<= 4 multiplies + 3 additions per pass: 14), the position GEMM is a sum of Cin terms (Cin), the output transform two passes of
  rows of A^T with at most 5 non-zero coefficients (<= 5 multiplies + 5 additions per pass: 20): Cin + 35 <= Cin + 48 for F(4x4).
  F(2x2) has coefficients +-1 only (no multiplies: 2 x 2 additions in, 2 x 3 out, 1 operand: Cin + 11 <= Cin + 24).  The epilogue
  is the direct form's: 4 u T.  Split operands add 2^-20 |scale| W_abs; fp16 operands (plan 16) are rounded to 2^-11 relative
  each: (1 + 2^-11)^2 - 1 < 2^-10, so + 2^-10 |scale| W_abs2.
These constants follow from the counts above; they are not fitted to any measured error.
"""
import collections
import functools
import itertools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from xmem2_amd import conv_plan, ops

U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def conv_sum(x, w, stride, pad, dilation=1):
    """sum_{kh,kw,c} x[b, oh s - p + kh d, ow s - p + kw d, c] w[n, kh, kw, c] in float64, NHWC in and out."""
    y = F.conv2d(_nchw(x.double()), _nchw(w.double()), stride=stride, padding=pad, dilation=dilation)
    return y.permute(0, 2, 3, 1).contiguous()


def finish(conv, scale, shift, res, relu_out, res_broadcast):
    """The epilogue on a float64 convolution sum: conv * scale + shift (+ res, one image for all when res_broadcast), relu."""
    v = conv * scale.double() + shift.double()
    if res is not None:
        r = res.double()
        assert r.shape[0] == (1 if res_broadcast else conv.shape[0]) and r.shape[1:] == conv.shape[1:]
        v = v + r
    return v.clamp(min=0) if relu_out else v


def conv_ref(x, w, scale, shift, res, stride, pad, relu_in, relu_out, res_broadcast, dilation=1):
    """(ref, S, T): the convolution of the header in float64, S = sum |x'| |w| and T = |scale| S + |shift| + |res|."""
    xd = x.double().clamp(min=0) if relu_in else x.double()
    ref = finish(conv_sum(xd, w, stride, pad, dilation), scale, shift, res, relu_out, res_broadcast)
    S = conv_sum(xd.abs(), w.double().abs(), stride, pad, dilation)
    T = scale.double().abs() * S + shift.double().abs()
    if res is not None:
        T = T + res.double().abs()
    return ref, S, T


def _dyadic(m, bits=20):
    """m with every entry rounded to a multiple of 2^-bits, after asserting that it is one (to 1e-12)."""
    q = np.round(m * 2.0 ** bits) / 2.0 ** bits
    assert np.abs(q - m).max() < 1e-12, 'a Winograd transform entry is not a dyadic rational'
    return q


@functools.lru_cache(None)
def wino_matrices(r):
    """(G, B^T, A^T) of F(r x r, 3x3), r in {2, 4}, float64 numpy.  G is the library's (ops._WINO_G / ops._wino4_g()); the points are
    read off its rows (p_i = G[i][1] / G[i][0], the row (0, 0, 1) is infinity); A^T[k][i] = p_i^k with the column of infinity
    (0, .., 0, 1); B^T solves sum_i A^T[k,i] G[i,a] B^T[i,j] = [j == k + a]."""
    G = (ops._WINO_G if r == 2 else ops._wino4_g()).double().numpy()
    n = r + 2
    assert G.shape == (n, 3)
    AT = np.zeros((r, n))
    for i in range(n):
        if G[i, 0] == 0.0:
            assert G[i, 1] == 0.0 and G[i, 2] == 1.0
            AT[r - 1, i] = 1.0
        else:
            AT[:, i] = (G[i, 1] / G[i, 0]) ** np.arange(r)
    lhs = (AT[:, None, :] * G.T[None, :, :]).reshape(r * 3, n)              # rows (k, a), columns i
    rhs = np.zeros((r * 3, n))
    for k in range(r):
        for a in range(3):
            rhs[k * 3 + a, k + a] = 1.0
    BT, _, rank, _ = np.linalg.lstsq(lhs, rhs, rcond=None)
    assert rank == n and np.abs(lhs @ BT - rhs).max() < 1e-12, 'the system for B^T has no unique exact solution'
    return G, _dyadic(BT), _dyadic(AT)


def _wino_tiles(x, r):
    """x [B, H, W, C] -> the (r+2)^2 input tiles [B, th, tw, C, r+2, r+2] of the grid the library uses: tiles of r x r outputs from
    output (0, 0), pad 1, zeros beyond the map."""
    B, H, W, C = x.shape
    th, tw = -(-H // r), -(-W // r)
    xp = x.new_zeros((B, r * th + 2, r * tw + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    return xp.unfold(1, r + 2, r).unfold(2, r + 2, r)


def _wino_eval(x, w, r, absolute):
    G, BT, AT = (torch.from_numpy(np.abs(m) if absolute else m) for m in wino_matrices(r))
    xd, wd = x.double(), w.double()
    if absolute:
        xd, wd = xd.abs(), wd.abs()
    B, H, W, _ = x.shape
    Uw = torch.einsum('ia,nabc,jb->nijc', G, wd, G)
    V = torch.einsum('ip,btucpq,jq->btuijc', BT, _wino_tiles(xd, r), BT)
    M = torch.einsum('btuijc,nijc->btunij', V, Uw)
    Y = torch.einsum('ki,btunij,lj->btkuln', AT, M, AT)                        # [B, th, r, tw, r, Cout]
    return Y.reshape(B, Y.shape[1] * r, Y.shape[3] * r, -1)[:, :H, :W].contiguous()


def wino_conv(x, w, r):
    """The 3x3 / stride 1 / pad 1 convolution sum through the Winograd matrices, float64 (equals conv_sum to round-off)."""
    return _wino_eval(x, w, r, False)


def wino_abs(x, w, r):
    """|A^T| ( sum_c (|G| |g_c| |G^T|) o (|B^T| |d_c| |B|) ) |A| per output element, float64; x is the input the transform sees
    (after relu_in)."""
    return _wino_eval(x, w, r, True)


def wino_emulate_fp32(x, w, r):
    """The pipeline in fp32 on the CPU: U = G g G^T rounded once, fp32 input transform, sequential fp32 accumulation over the input
    channels, fp32 output transform.  Returns the convolution sum as float64 [B, H, W, Cout]."""
    G, BT, AT = wino_matrices(r)
    B, H, W, C = x.shape
    Uw = np.einsum('ia,nabc,jb->nijc', G, w.double().numpy(), G).astype(np.float32)
    t = _wino_tiles(x.float(), r).numpy()
    BT32, AT32 = BT.astype(np.float32), AT.astype(np.float32)
    V = np.einsum('ip,btucpq->btuciq', BT32, t, dtype=np.float32)
    V = np.einsum('btuciq,jq->btucij', V, BT32, dtype=np.float32)
    M = np.zeros(V.shape[:3] + (Uw.shape[0], r + 2, r + 2), np.float32)
    for c in range(C):
        M += V[:, :, :, None, c] * Uw[None, None, None, :, :, :, c]
    Y = np.einsum('ki,btunij->btunkj', AT32, M, dtype=np.float32)
    Y = np.einsum('btunkj,lj->btkuln', Y, AT32, dtype=np.float32)
    Y = Y.reshape(B, Y.shape[1] * r, Y.shape[3] * r, -1)[:, :H, :W]
    return torch.from_numpy(np.ascontiguousarray(Y)).double()


# ---------------------------------------------------------------------------------------------------------
# bounds (module docstring)
# ---------------------------------------------------------------------------------------------------------
def k_pad(K, bk):
    return -(-K // bk) * bk


def bound_direct(T, S, scale, K, bk, splitk, fp32x=False):
    b = ((4 if fp32x else 1) * k_pad(K, bk) + splitk + 4) * U * T
    return b + 2.0 ** -20 * scale.double().abs() * S if fp32x else b


def bound_wino(r, cin, scale, Wabs, T, fp32x=False, f16=False):
    sw = scale.double().abs() * Wabs
    b = (cin + (24 if r == 2 else 48)) * U * sw + 4 * U * T
    if fp32x:
        b = b + 2.0 ** -20 * sw
    if f16:
        assert r == 2
        b = b + 2.0 ** -10 * sw
    return b


def half_out_extra(ref):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25


# ---------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------
MAPS = ((1, 1, 1), (1, 1, 9), (2, 2, 2), (1, 3, 5), (3, 4, 4), (1, 5, 7), (2, 6, 10), (1, 7, 9), (3, 9, 13))
CHANNELS = ((4, 3), (12, 36), (36, 68), (32, 32), (64, 132), (96, 64))          # fp32 and fp32x; the last three Winograd-eligible
CHANNELS_WINO = CHANNELS[3:]
CHANNELS_HALF = ((8, 3), (24, 36), (40, 68), (64, 132))
KERNELS = ((1, 1, 1, 0), (1, 1, 2, 0), (1, 1, 1, 1), (3, 3, 1, 1), (3, 3, 2, 1), (3, 3, 1, 0), (1, 3, 1, 1), (5, 5, 1, 2), (7, 7, 2, 3))
K3 = (3, 3, 1, 1)
EPILOGUES = ('none', 'relu_res_relu', 'bcast_relu')
LAYOUTS = ('dense', 'sliced', 'unaligned')
SPLITKS = (0, 1, 2, 3, 5, 16, 1000)
MODES = ('fp32', 'fp32x', 'half_f32', 'half_f16')           # half input with fp32 / half output
DENSE_MAPS = ((3, 4, 4), (1, 7, 9), (3, 9, 13))

Case = collections.namedtuple('Case', 'family mode regime B H W cin cout kh kw stride pad epi layout splitk code dil skip var')
Case.__new__.__defaults__ = (1, 1, 0)                        # dilation, tap skip (dilated entry only), layout variant


def out_dims(c):
    return ((c.H + 2 * c.pad - c.dil * (c.kh - 1) - 1) // c.stride + 1, (c.W + 2 * c.pad - c.dil * (c.kw - 1) - 1) // c.stride + 1)


def refused(c):
    """The header's XMEM_ERR_BAD_ARG: an input that is smaller than the (dilated) kernel even with its padding."""
    return c.H + 2 * c.pad < c.dil * (c.kh - 1) + 1 or c.W + 2 * c.pad < c.dil * (c.kw - 1) + 1


def _rot(i):
    """epilogue, layout, split-K and layout variant of the i-th case of a family: three strides that are pairwise coprime with the
    axis lengths, so that pairs of values meet (tests/test_conv_refs_host.py asserts that they all do)."""
    return EPILOGUES[(i + i // 3 + i // 63) % 3], LAYOUTS[(i // 3 + i // 7 + i // 27) % 3], SPLITKS[(i + i // 9 + i // 49) % 7], (i // 5) % 2


@functools.lru_cache(None)
def cases():
    out, count = [], collections.Counter()

    def add(family, mode, regime, m, ch, k, code, **kw):
        i = count[family]
        count[family] += 1
        epi, layout, splitk, var = _rot(i)
        if kw.get('dil', 1) != 1 or family == 'dilated':
            epi = EPILOGUES[i % 2]                            # the dilated entry takes no broadcast residual
        out.append(Case(family, mode, regime, *m, *ch, *k, kw.pop('epi', epi), kw.pop('layout', layout), kw.pop('splitk', splitk), code,
                        kw.pop('dil', 1), kw.pop('skip', 1), kw.pop('var', var)))

    # direct family: every kernel x map x channel pair, codes 0..6 rotated, every mode, exact and sparse
    i = 0
    for regime in ('exact', 'sparse'):
        for mode in MODES:
            for k, m, ch in itertools.product(KERNELS, MAPS, CHANNELS_HALF if mode.startswith('half') else CHANNELS):
                add('direct', mode, regime, m, ch, k, (i + i // 7) % 7)
                i += 1
    # every plan code on 3x3 / 1 / 1, the eligible channel pairs; F(4x4) codes in the sparse regime
    for code in range(41):
        f4 = conv_plan.CODES[code].form == 'f4'
        for mode in ('fp32', 'fp32x'):
            for m, ch in itertools.product(MAPS, CHANNELS_WINO):
                add('plans', mode, 'sparse' if f4 else 'exact', m, ch, K3, code)
            if code >= 35:
                for k, m, ch in itertools.product(KERNELS[:3], MAPS, CHANNELS_WINO):
                    add('plans', mode, 'exact', m, ch, k, code)
    for m in MAPS:                                            # plan 16 at Cin % 64 == 0
        for ch in ((64, 132), (64, 64)):
            add('plans', 'fp32', 'exact', m, ch, K3, 16)
    for code in range(41):
        for mode in ('fp32', 'fp32x'):
            for m, ch in itertools.product(DENSE_MAPS, CHANNELS_WINO):
                add('dense', mode, 'dense', m, ch, K3, code)
    # the library's own Winograd contract: Cout % 4 == 0, below the 32 that ConvWeights asks for
    for cout in (4, 36):
        for code, regime in ((9, 'exact'), (9, 'sparse'), (29, 'exact'), (14, 'exact'), (19, 'sparse'), (23, 'sparse')):
            add('small_cout', 'fp32', regime, (2, 6, 10), (32, cout), K3, code, layout='dense')
    # Cout = 1: the GEMV on every map and kernel (one Cin above 256: the general channel loop), the row-of-four kernel, half input
    for j, (k, m) in enumerate(itertools.product(KERNELS, MAPS)):
        add('gemv', 'fp32', 'exact', m, (260 if j == 30 else CHANNELS[j % 6][0], 1), k, 0)
        add('gemv', 'half_f32', 'exact', m, (CHANNELS_HALF[j % 4][0], 1), k, 0)
    for regime in ('exact', 'sparse'):
        add('gemv', 'fp32', regime, (1, 91, 93), (8, 1), K3, 0, layout='dense')
    # the dilated entry: whole taps outside the map
    for dil in (1, 2, 5):
        for m in MAPS[:8]:
            for code in range(7):
                j = count['dilated'] // 2
                for skip in (1, 0):
                    add('dilated', 'fp32', 'exact', m, CHANNELS[(j + j // 6) % 6], (3, 3, 1 + j % 2, dil), code, dil=dil, skip=skip,
                        layout=LAYOUTS[(j + j // 7) % 3], splitk=SPLITKS[(j + j // 7) % 7], epi=EPILOGUES[(j // 2) % 2], var=(j // 3) % 2)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------
# the plan a case must execute (include/xmem_hip.h, xmem_conv_desc.plan_tile: codes and FALLBACKS)
# ---------------------------------------------------------------------------------------------------------
Plan = collections.namedtuple('Plan', 'form bm bn bk stream ring code')


def layout_of(c):
    """(ldin, in_off, ldout, out_off, ldres) in elements of the storage types, and whether `out` stays 16-byte aligned."""
    half_in = c.mode.startswith('half')
    ldin = c.cin + (-c.cin % 8 if half_in else 0)
    if c.layout == 'sliced':
        return ((c.cin + 8, 8) if half_in else (c.cin + 8, 4)) + (c.cout + 12, 4, c.cout + 4)
    if c.layout == 'unaligned':
        return (ldin, 0) + ((c.cout + 1, 0) if c.var == 0 else (c.cout, 1)) + (c.cout + 3,)
    return ldin, 0, c.cout, 0, c.cout


def has_res(c):
    return c.epi != 'none'


def wino_eligible(c, have_operand=True):
    _, _, ldout, out_off, ldres = layout_of(c)
    return (have_operand and (c.kh, c.kw, c.stride, c.pad) == K3 and c.dil == 1 and c.cin % 32 == 0 and c.cout % 4 == 0 and ldout % 4 == 0
            and out_off % 4 == 0 and (not has_res(c) or ldres % 4 == 0))


def expected_plan(c):
    """The form, tile, k-tile and ring the header documents for the case (every Winograd operand of the layer is passed; plan 16's
    only where Cin % 64 == 0, as ConvWeights builds it)."""
    if c.cout == 1:
        return Plan('gemv', 0, 0, 32, 0, 0, c.code)
    if c.mode.startswith('half'):
        t = conv_plan.HALF_CODES.get(c.code)
        return Plan('direct', t.bm, t.bn, 32, 0, 0, c.code) if t else Plan('direct', 64, 64, 32, 0, 0, 0)
    fp32x, code = c.mode == 'fp32x', c.code
    wok = wino_eligible(c) and c.family != 'dilated'
    while True:
        t = conv_plan.CODES[code]
        if t.ring:
            if not fp32x and c.cin % 32 == 0 and ((c.kh, c.kw, c.pad) == (1, 1, 0) if t.form == 'direct' else wok):
                break
            code = {'f4': 19, 'f2': 9, 'direct': 3}[t.form]
        elif t.form == 'f4':
            if wok:
                break
            code -= 10
        elif t.form == 'f2_f16':
            if wok and not fp32x and c.cin % 64 == 0:
                break
            code = 9
        elif t.form == 'f2_fused':
            if wok and not fp32x:
                break
            code = {13: 8, 14: 9, 15: 9}[code]
        elif t.form == 'f2':
            if wok:
                break
            code -= 6
        else:
            break
    t = conv_plan.CODES[code]
    bm, bn = (t.bm, t.bn) if code else (64, 64)                # the heuristic: fewer than 384 tiles at these sizes -> 64 x 64
    return Plan(t.form, bm, bn, t.bk, int(t.ring > 0), t.ring, code)


def expected_splitk(c, plan):
    """Slabs of the contraction for an explicit plan_splitk (clamped to the k-tile count, empty slabs dropped); None for the
    heuristic (plan_splitk = 0: anything in 1..16)."""
    if plan.form != 'direct' or plan.ring:
        return 1
    if c.splitk == 0:
        return None
    cin = c.cin // 2 if c.mode.startswith('half') else c.cin      # half operands: a k-tile of 32 four-byte units holds 64 halfs
    cin += -cin % 4 if c.mode.startswith('half') else 0
    nk = -(-(c.kh * c.kw * cin) // plan.bk)
    s = min(c.splitk, nk)
    return -(-nk // -(-nk // s))


# ---------------------------------------------------------------------------------------------------------
# input regimes
# ---------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _sign(shape, g):
    return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


def _h(t):
    return t.to(torch.float16).double()


@functools.lru_cache(256)
def make_weights(regime, half, cout, kh, kw, cin):
    """(w, scale, shift) float64 holding values of the storage types: w [Cout, KH, KW, Cin]; scale per channel from {0.5, 1, 2};
    shift distinct per channel."""
    g = _gen('w', regime, half, cout, kh, kw, cin)
    K = kh * kw * cin
    n = torch.arange(cout).double()
    scale = torch.tensor([0.5, 1.0, 2.0]).double()[torch.arange(cout) % 3]
    if regime == 'exact':
        w, shift = _sign((cout, kh, kw, cin), g), n - cout // 2
    else:
        mag = 0.5 + torch.rand((cout, kh, kw, cin), generator=g).double() if regime == 'sparse' else torch.randn((cout, kh, kw, cin), generator=g).double().abs()
        w = _sign((cout, kh, kw, cin), g) * mag / K ** 0.5
        shift = 0.25 + 0.5 * n / cout
    w = _h(w) if half else w.float().double()
    return w, scale, shift.float().double()


def _nnz(c):
    """exact regime, half output: non-zero channels per pixel (None: all), so that 4 taps nnz + 66 + 8 <= 1024"""
    return max(1, 237 // (c.kh * c.kw)) if c.regime == 'exact' and c.mode == 'half_f16' else None


@functools.lru_cache(512)
def _make_x(regime, half, nnz, B, H, W, cin):
    g = _gen('x', regime, half, nnz, B, H, W, cin)
    shape = (B, H, W, cin)
    if regime == 'exact':
        x = _sign(shape, g) * torch.randint(1, 3, shape, generator=g).double()
        if nnz is not None and nnz < cin:
            x = x * (torch.rand(shape, generator=g).argsort(-1) < nnz)
    elif regime == 'sparse':
        b, h, ww = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing='ij')
        ch = (7 * h + 3 * ww + b + cin - 1 - (7 * (H - 1) + 3 * (W - 1) + B - 1)) % cin
        x = torch.zeros(shape).double()
        v = _sign(shape[:3], g) * (0.5 + torch.rand(shape[:3], generator=g).double())
        v[-1, -1, -1] = v[-1, -1, -1].abs()                   # the last channel survives a relu_in
        x.scatter_(3, ch[..., None], v[..., None])
    else:
        x = torch.randn(shape, generator=g).double()
    return _h(x) if half else x.float().double()


def make_inputs(c):
    """dict(x, w, scale, shift, res) of a case, float64 tensors whose values are exactly representable in the storage types
    (fp32, or half for the operands of the half modes and the residual of a half output).
      exact   x in {+-1, +-2}, w in {+-1}, shift = n - Cout / 2, res in -8..8.  A half output keeps only `nnz` channels per pixel
              non-zero, so that |ref| <= 4 taps nnz + 66 + 8 <= 1024 stays exactly representable with scale 0.5.
      sparse  one non-zero channel per pixel, c = (7 h + 3 w + b + b0) mod Cin with b0 chosen so that the LAST pixel of the last
              image carries the last channel with a positive value (the k tail is always read, also behind relu_in), magnitude in
              [0.5, 1.5], random sign elsewhere; dense weights of
              magnitude in [0.5, 1.5] / sqrt(K).
      dense   normal activations, normal weights / sqrt(K)."""
    half, half_out = c.mode.startswith('half'), c.mode == 'half_f16'
    w, scale, shift = make_weights(c.regime, half, c.cout, c.kh, c.kw, c.cin)
    x = _make_x(c.regime, half, _nnz(c), c.B, c.H, c.W, c.cin)
    res = None
    if has_res(c) and not refused(c):
        Ho, Wo = out_dims(c)
        rs = (1 if c.epi == 'bcast_relu' else c.B, Ho, Wo, c.cout)
        g = _gen('res', c.regime, rs)
        res = torch.randint(-8, 9, rs, generator=g).double() if c.regime == 'exact' else 0.5 * torch.randn(rs, generator=g).double()
        res = _h(res) if half_out else res.float().double()
    return dict(x=x, w=w, scale=scale, shift=shift, res=res)


@functools.lru_cache(512)
def _conv_parts(regime, half, nnz, B, H, W, cin, cout, kh, kw, stride, pad, dil, relu_in):
    """(conv, S) in float64: shared by the cases that differ in plan code, layout, split-K or residual only"""
    w = make_weights(regime, half, cout, kh, kw, cin)[0]
    x = _make_x(regime, half, nnz, B, H, W, cin)
    x = x.clamp(min=0) if relu_in else x
    return conv_sum(x, w, stride, pad, dil), conv_sum(x.abs(), w.abs(), stride, pad, dil)


@functools.lru_cache(512)
def _wino_abs_parts(regime, B, H, W, cin, cout, relu_in, r):
    w = make_weights(regime, False, cout, 3, 3, cin)[0]
    x = _make_x(regime, False, None, B, H, W, cin)
    return wino_abs(x.clamp(min=0) if relu_in else x, w, r)


def conv_parts(c):
    return _conv_parts(c.regime, c.mode.startswith('half'), _nnz(c), c.B, c.H, c.W, c.cin, c.cout, c.kh, c.kw, c.stride, c.pad, c.dil,
                       c.epi == 'relu_res_relu')


def epilogue_flags(c):
    """(relu_in, relu_out, res_broadcast)"""
    return c.epi == 'relu_res_relu', c.epi != 'none', c.epi == 'bcast_relu'


def reference(c, inputs=None):
    """(ref, S, T) of a case: conv_ref on its inputs (the convolution sums are shared between the cases that have them in common)."""
    i = inputs or make_inputs(c)
    conv, S = conv_parts(c)
    _, relu_out, bcast = epilogue_flags(c)
    T = i['scale'].abs() * S + i['shift'].abs() + (i['res'].abs() if i['res'] is not None else 0.0)
    return finish(conv, i['scale'], i['shift'], i['res'], relu_out, bcast), S, T


def bound_of(c, plan, splitk, ref, S, T, inputs=None):
    """The bound of the module docstring for the form `plan` executes; None in the exact regime where equality is asked (every
    form but F(4x4), whose G is not dyadic)."""
    if c.regime == 'exact' and plan.form != 'f4':
        return None
    i = inputs or make_inputs(c)
    fp32x, half = c.mode == 'fp32x', c.mode.startswith('half')
    if plan.form in ('gemv', 'direct'):
        b = bound_direct(T, S, i['scale'], c.kh * c.kw * c.cin, 2 * plan.bk if half else plan.bk, splitk, fp32x and plan.form == 'direct')
    else:
        r = 4 if plan.form == 'f4' else 2
        b = bound_wino(r, c.cin, i['scale'], _wino_abs_parts(c.regime, c.B, c.H, c.W, c.cin, c.cout, epilogue_flags(c)[0], r), T, fp32x,
                       plan.form == 'f2_f16')
    return b + half_out_extra(ref) if c.mode == 'half_f16' else b


def assert_exact_representable(c, ref):
    """The exact regime's premise: the float64 reference is a value of the output storage type."""
    dt = torch.float16 if c.mode == 'half_f16' else torch.float32
    assert bool((ref.to(dt).double() == ref).all()), f'{c}: the reference of an exact case is not representable in {dt}'
    assert float(ref.abs().max()) <= (1024.0 if c.mode == 'half_f16' else 2.0 ** 23)
