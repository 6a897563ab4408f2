"""Plain float64 statements of the frame-loop elementwise operations (csrc/elementwise.hip), the a-priori round-off bounds the GPU
tests hold the kernels to, and the grid of edge cases both test files walk.

Written from the header comments of include/xmem_hip.h and from the oracle (oracle/cpu_ref.py), not from the kernels.  Operands are in
the C ABI's logical layout: NHWC activations [B][H][W][C] (the GPU test embeds them in buffers with pixel strides and offsets), NCHW
planes [K][H][W] for the probability operations.  Inputs are fp32 / half tensors and are taken EXACTLY (converted to float64, no
rounding).  Every reference returns the value and the bound per output element (None: the operation is exact, the result must EQUAL
the value; for a half output the value rounded once to half).

Semantics that belong to the operation's definition (the reference project computes them so):
  - the bilinear source index is computed in fp32 as ATen does, src = scale * (dst + 0.5) - 0.5 clamped at 0, i0 = int(src),
    l1 = src - i0, scale = float32(in / out) (0.5 / 0.25 for the x2 / x4 upsamples); the blend itself is float64;
  - the aggregation clamps at float32(1e-7) and float32(1) - float32(1e-7) (the oracle clamps in fp32), everything else is float64
    and the output is odds_k / sum odds;
  - max-pool pads with -inf, argmax picks the first maximal index, the merge_masks region test is `sum > 0.5` on the fp32 sum.

`mut=` on a reference selects what a plausible kernel mistake would compute instead (tests/test_elementwise_refs_host.py: a bound
counts only if such a kernel falls outside it); the GPU test never passes it.

tests/test_elementwise_refs_host.py ties every function here to the oracle / torch on the CPU; tests/test_gpu_elementwise_edges.py
compares the kernels with them.
"""
import itertools
import zlib

import numpy as np
import torch

U = 2.0 ** -24            # unit round-off of fp32 (round to nearest)
UH = 2.0 ** -11           # unit round-off of half
TINY = 2.0 ** -126        # smallest normal fp32: a result below it may be flushed to zero (exp overflows past 88.7)
C_EXP = 4                 # relative error of exp / tanh in units of u: within 2 ulp (the device library documents 1 ulp)
C_BLEND = 7               # roundings a tap of hy * (hx * a + lx * b) + ly * (...) passes: 1 - l twice, two products, two sums, +1 for
                          # second-order terms; a fused multiply-add only removes roundings
CLAMP_LO = float(np.float32(1e-7))
CLAMP_HI = float(np.float32(1) - np.float32(1e-7))
SENTINEL = -777.0         # what the GPU test fills output buffers with; exactly representable as a half
JUNK = 7.0                # what the GPU test puts outside input slices; the `skip_per_image` mutation reads it

GRID_BLOCK, GRID_CAP = 256, 8192          # grid_for() in csrc/elementwise.hip: workgroup size and the cap on workgroups
GRID_ITEMS = GRID_BLOCK * GRID_CAP        # work items one trip of a grid-stride loop covers (2,097,152)


def d64(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double()


def half_bound(bound, ref):
    """Half storage of the output: the fp32 bound + one rounding to half, 2^-11 |ref| + 2^-25 (the subnormal spacing of halfs is 2^-24)."""
    return bound + UH * ref.abs() + 2.0 ** -25


def round_to(ref, half):
    """The float64 value rounded ONCE to the storage type, as float64 (exact operations must return exactly this)."""
    return (ref.half() if half else ref.float()).double()


def rng_of(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def randn(g, *shape, half=False):
    """fp32 normal values; half=True: values a half holds exactly (so that the half-storage input is the same number)."""
    t = torch.randn(*shape, generator=g)
    return t.half().float() if half else t


# ---------------------------------------------------------------------------------------------------------
# max pool 3x3 / stride 2 / pad 1
# ---------------------------------------------------------------------------------------------------------
def maxpool_ref(x, mut=None):
    """nn.MaxPool2d(3, 2, 1) on x [B][H][W][C] with -inf padding -> [B][Ho][Wo][C], Ho = (H - 1) // 2 + 1.  Exact."""
    x = d64(x)
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.full((B, H + 3, W + 3, C), 0.0 if mut == 'zero_padding' else -np.inf, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    o = 1 if mut == 'window_shifted' else 0            # the window starts at 2 oh instead of 2 oh - 1
    taps = [xp[:, dy + o:dy + o + 2 * Ho:2, dx + o:dx + o + 2 * Wo:2] for dy in range(3) for dx in range(3)]
    return torch.stack(taps).max(0)[0], None


# ---------------------------------------------------------------------------------------------------------
# bilinear resampling
# ---------------------------------------------------------------------------------------------------------
def bilinear_index(n_out, n_in, scale=None, mut=None):
    """ATen's area_pixel_compute_source_index (align_corners=False) in fp32 -> (i0, i1 int64 [n_out], l1, dl float64 [n_out]).
    dl: how far l1 may move when the product scale * (dst + 0.5) is not rounded before the subtraction (a fused multiply-add, as
    ATen's own vectorised CPU kernel and a contracting device compiler emit): u * (src + 0.5).  Zero for the x2 / x4 upsamples, whose
    scale is a power of two: the product is exact either way."""
    s = np.float32(n_in) / np.float32(n_out) if scale is None else np.float32(scale)
    src = s * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    assert src.dtype == np.float32
    if mut != 'no_clamp_at_0':
        src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)            # truncation, as a C cast
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float64)
    dl = U * (np.abs(src.astype(np.float64)) + 0.5) * (0.0 if np.log2(float(s)).is_integer() else 1.0)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1), torch.from_numpy(dl)


def blend_ref(x, Ho, Wo, scale=None, mut=None):
    """x [B][Hi][Wi][C] -> (value, magnitude), float64 [B][Ho][Wo][C]; magnitude = sum over the four taps |w v|, plus
    (dlx |d value / d lx| + dly |d value / d ly|) / (C_BLEND u) so that blend_bound carries the index term of bilinear_index."""
    x = d64(x)
    y0, y1, ly, dly = bilinear_index(Ho, x.shape[1], scale, mut)
    x0, x1, lx, dlx = bilinear_index(Wo, x.shape[2], scale, mut)
    hy, hx = 1.0 - ly, 1.0 - lx
    if mut == 'weights_swapped':
        lx, hx = hx, lx
    ly, hy, lx, hx = ly[None, :, None, None], hy[None, :, None, None], lx[None, None, :, None], hx[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    v00, v01, v10, v11 = r0[:, :, x0], r0[:, :, x1], r1[:, :, x0], r1[:, :, x1]
    val = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)
    mag = (hy * (hx * v00).abs()).abs() + (hy * (lx * v01).abs()).abs() + (ly * (hx * v10).abs()).abs() + (ly * (lx * v11).abs()).abs()
    slope_x = hy.abs() * (v01 - v00).abs() + ly.abs() * (v11 - v10).abs()
    slope_y = hx.abs() * (v10 - v00).abs() + lx.abs() * (v11 - v01).abs()
    index = dlx[None, None, :, None] * slope_x + dly[None, :, None, None] * slope_y
    return val, mag + index / (C_BLEND * U)


def blend_bound(val, mag):
    """C_BLEND u sum |w v| + u |ref| (+ the index term folded into `mag`): every tap's term passes at most C_BLEND - 1 roundings
    (C_BLEND above), the last sum one more."""
    return C_BLEND * U * mag + U * val.abs()


def upsample2x_add_ref(g, skip, mut=None):
    """F.interpolate(g, scale_factor=2, bilinear, align_corners=False) + skip: g [B][h][w][C], skip [2h][2w][C] is ONE image shared by
    every b.  The x2 weights 0.25 / 0.75 are exact.  Bound: the blend's + u |ref| for the addition of the skip."""
    g, skip = d64(g), d64(skip)
    B, h, w, C = g.shape
    v, m = blend_ref(g, 2 * h, 2 * w, 0.5, mut)
    s = skip[None].expand(B, -1, -1, -1).clone()
    if mut == 'skip_per_image':                       # skip[b] instead of skip: past the one image the buffer holds JUNK
        s[1:] = JUNK
    ref = v + s
    return ref, blend_bound(v, m) + U * ref.abs()


def resize_bilinear_ref(x, Ho, Wo, mut=None):
    """F.interpolate(x[:, None], (Ho, Wo), bilinear, align_corners=False) on planes x [C][Hi][Wi] -> [C][Ho][Wo]."""
    v, m = blend_ref(d64(x)[..., None], Ho, Wo, None, mut)
    return v[..., 0], blend_bound(v, m)[..., 0]


# ---------------------------------------------------------------------------------------------------------
# area downsample, channel copies, the HiddenUpdater gather
# ---------------------------------------------------------------------------------------------------------
def area_ref(x, r, mut=None):
    """F.interpolate(mode='area') by the integer ratio r: the mean of each r x r window of x [B][H][W][C].
    Bound (r^2 + 1) u sum|x| / r^2: r^2 - 1 additions in any order, one multiplication by 1 / r^2, one for second-order terms
    (1 / r^2 is a power of two for r = 1, 2, 4)."""
    x = d64(x)
    B, H, W, C = x.shape
    t = x.reshape(B, H // r, r, W // r, r, C)
    div = r if mut == 'divided_by_r' else r * r
    return t.sum((2, 4)) / div, (r * r + 1) * U * t.abs().sum((2, 4)) / (r * r)


def copy_channels_ref(src, B, mut=None):
    """dst[b] = src[b % srcB]: src [srcB][P][C] -> [B][P][C].  Exact (a half destination: one rounding)."""
    src = d64(src)
    out = src[[b % src.shape[0] for b in range(B)]]
    if mut == 'b_not_modulo':                          # src[b]: past the srcB images the buffer holds JUNK
        out[src.shape[0]:] = JUNK
    return out, None


def hidden_gather_ref(g16, g8, g4, logits):
    """[ g16 | area2(g8) | area4(g4) | area4(logits) ] over channels: g16 [K][h][w][c16], g8 [K][2h][2w][c8], g4 [K][4h][4w][c4],
    logits [K][4h][4w].  The g16 part is a copy (bound 0), the others carry area_ref's bound."""
    parts = [(d64(g16), torch.zeros(g16.shape, dtype=torch.float64)), area_ref(g8, 2), area_ref(g4, 4), area_ref(d64(logits)[..., None], 4)]
    return torch.cat([p[0] for p in parts], -1), torch.cat([p[1] for p in parts], -1)


# ---------------------------------------------------------------------------------------------------------
# CBAM + residual
# ---------------------------------------------------------------------------------------------------------
def sigmoid_err(x):
    """|computed - true| of sigmoid(x) evaluated as 1 / (1 + exp(-x)), p the true value and e = exp(-x) = (1 - p) / p:
      - exp is relatively off by C_EXP u, which moves p by C_EXP u e p^2 = C_EXP u p (1 - p);
      - the addition 1 + e and the division each round once: u p relative to the result, but never further than the distance to
        the representable neighbour 1.0 - so min(u, e) p each.  That ABSOLUTE term of about u is what the form leaves of 1 - p when the
        gate saturates at 1; towards 0 the error stays relative;
      - 2 u p (1 - p) for second-order terms, TINY for a result flushed to zero (exp overflows past 88.7)."""
    p = torch.sigmoid(x)
    e = torch.exp(-x)
    return (C_EXP + 2) * U * p * (1 - p) + 2 * torch.minimum(torch.full_like(e, U), e) * p + TINY


def tanh_err(n):
    """|computed - true| of a tanh whose true value is n: (C_EXP + 2) u |n| + TINY."""
    return (C_EXP + 2) * U * n.abs() + TINY


def cbam_ref(g, w1, b1, w2, b2, sw, sb, mut=None):
    """out = g + SpatialGate(ChannelGate(g)) (model/cbam.py through the oracle's RefNet._cbam): g [B][H][W][C], w1 [C/16][C], b1, w2
    [C][C/16], b2, sw [2][7][7] (channel 0 = max, 1 = mean), sb [1].  Returns (value, bound, intermediates).

    The bound is propagated through the five steps from the reference's own magnitudes (n terms summed in ANY order carry at most
    n u sum|terms| to first order; relu, max and the clamp are 1-Lipschitz; sigmoid's slope is at most 1/4):
      1. E_avg = (P + 1) u mean|g| (P - 1 additions, one division, one spare); the pooled max is exact;
      2. hidden pre-activation: sum_c |w1| E_pool + (C + 1) u (sum_c |w1 pool| + |b1|); attention of one path: sum_j |w2| E_hid +
         (Cr + 1) u (sum_j |w2 hid| + |b2|); the two paths are added: + u (|att_avg| + |att_max| + |att|);
      3. channel scale cs = sigmoid(att): E_cs = E_att / 4 + sigmoid_err;  xs = g cs: E_xs = |g| E_cs + u |xs|;
      4. compressed max: max_c E_xs; compressed mean: mean_c E_xs + (C + 1) u mean_c |xs|;
      5. gate pre-activation over the 98 taps: sum |sw| E_comp + 99 u (sum |sw comp| + |sb|); sg = sigmoid: E_sg = E_gate / 4 + sigmoid_err;
      out = g + xs sg: E = |xs| E_sg + sg E_xs + u |xs sg| + u |out|, times 1.01 for second-order terms."""
    g, w1, b1, w2, b2, sw, sb = (d64(t) for t in (g, w1, b1, w2, b2, sw, sb))
    B, H, W, C = g.shape
    P, Cr = H * W, w1.shape[0]
    x = g.reshape(B, P, C)
    n_avg = 16 * ((P + 15) // 16) if mut == 'avg_over_padded_P' else P
    avg = x.sum(1) / n_avg
    mx = x.max(1)[0].clamp(min=0) if mut == 'max_pooled_from_0' else x.max(1)[0]
    e_avg = (P + 1) * U * x.abs().mean(1)

    def mlp(p, e_p):
        pre = p @ w1.t() + b1
        e_pre = e_p @ w1.abs().t() + (C + 1) * U * (p.abs() @ w1.abs().t() + b1.abs())
        hid = pre.clamp(min=0)
        att = hid @ w2.t() + b2
        e_att = e_pre @ w2.abs().t() + (Cr + 1) * U * (hid @ w2.abs().t() + b2.abs())
        return att, e_att
    att_a, e_a = mlp(avg, e_avg)
    att_m, e_m = mlp(mx, torch.zeros_like(mx))
    att = att_a + att_m
    e_att = e_a + e_m + U * (att_a.abs() + att_m.abs() + att.abs())
    cs = torch.sigmoid(att)                                             # [B][C]
    e_cs = e_att / 4 + sigmoid_err(att)
    xs = x * cs[:, None, :]
    e_xs = x.abs() * e_cs[:, None, :] + U * xs.abs()
    cmax = xs.max(2)[0].clamp(min=0) if mut == 'max_pooled_from_0' else xs.max(2)[0]
    cmean = xs.sum(2) / (C + 1 if mut == 'mean_over_C_plus_1' else C)
    e_cmax = e_xs.max(2)[0]
    e_cmean = e_xs.mean(2) + (C + 1) * U * xs.abs().mean(2)
    comp = torch.stack([cmax, cmean], 1).reshape(B, 2, H, W)
    e_comp = torch.stack([e_cmax, e_cmean], 1).reshape(B, 2, H, W)
    k = sw.reshape(1, 2, 7, 7).clone()
    if mut == 'gate_channels_swapped':
        k = k.flip(1)
    if mut == 'one_tap_dropped':
        k[0, 0, 3, 3] = 0.0                                             # the centre tap of the max channel: inside on every map
    conv = torch.nn.functional.conv2d
    gate = (conv(comp, k, padding=3) + sb).reshape(B, P)
    e_gate = (conv(e_comp, k.abs(), padding=3) + 99 * U * (conv(comp.abs(), k.abs(), padding=3) + sb.abs())).reshape(B, P)
    sg = torch.sigmoid(gate)
    e_sg = e_gate / 4 + sigmoid_err(gate)
    y = xs * sg[:, :, None]
    out = x + y
    bound = 1.01 * (xs.abs() * e_sg[:, :, None] + sg[:, :, None] * e_xs + U * y.abs() + U * out.abs())
    aux = dict(avg=avg, max=mx, att=att, cs=cs, comp=comp, gate=gate, e_att=e_att, e_gate=e_gate)
    return out.reshape(B, H, W, C), bound.reshape(B, H, W, C), aux


# ---------------------------------------------------------------------------------------------------------
# GRU gate, add3, key post-processing
# ---------------------------------------------------------------------------------------------------------
def gru_gate_ref(values, h, mut=None):
    """new_h = f h (1 - u) + u n with f = sigmoid(values[..., :Ch]), u = sigmoid(values[..., Ch:2Ch]), n = tanh(values[..., 2Ch:]):
    values [N][3 Ch], h [N][Ch].
    Bound from the magnitudes of the terms: E_f, E_u = sigmoid_err, E_n = tanh_err; the computed 1 - u is off by
    E_u + u (1 - u) ABSOLUTELY - that is the term the 1 + exp(-x) form leaves when the update gate saturates at 1;
    t1 = f h (1 - u): |h| (1 - u) E_f + |f h| (E_u + u (1 - u)) + 2 u |t1|;  t2 = u n: |n| E_u + u E_n + u |t2|;
    the sum: u (|t1| + |t2|); times 1.01 for second-order terms."""
    v, h = d64(values), d64(h)
    Ch = h.shape[-1]
    xf, xu = (v[..., Ch:2 * Ch], v[..., :Ch]) if mut == 'f_and_u_swapped' else (v[..., :Ch], v[..., Ch:2 * Ch])
    f, u, n = torch.sigmoid(xf), torch.sigmoid(xu), torch.tanh(v[..., 2 * Ch:])
    one_u = torch.sigmoid(-xu)                                                                          # 1 - u without cancellation
    t1, t2 = f * h * one_u, u * n
    e_f, e_u, e_n = sigmoid_err(xf), sigmoid_err(xu), tanh_err(n)
    bound = (h.abs() * one_u * e_f + (f * h).abs() * (e_u + U * one_u) + 2 * U * t1.abs()
             + n.abs() * e_u + u * e_n + U * t2.abs() + U * (t1.abs() + t2.abs()))
    return t1 + t2, 1.01 * bound


def add3_ref(a, b, c):
    """a + b + c: two additions, 2 u (|a| + |b| + |c|)."""
    a, b, c = d64(a), d64(b), d64(c)
    return a + b + c, 2 * U * (a.abs() + b.abs() + c.abs())


def key_post_ref(proj, Ck):
    """proj [P][2 Ck + 1] = (key | d | e) -> key (exact), shrinkage = d^2 + 1 (two roundings: 2 u (d^2 + 1)), selection = sigmoid(e)
    (sigmoid_err).  Returns ((key, None), (shrinkage, bound), (selection, bound))."""
    p = d64(proj)
    key, dd, e = p[:, :Ck], p[:, Ck], p[:, Ck + 1:2 * Ck + 1]
    shr = dd * dd + 1.0
    return (key, None), (shr, 2 * U * shr), (torch.sigmoid(e), sigmoid_err(e))


# ---------------------------------------------------------------------------------------------------------
# input packing
# ---------------------------------------------------------------------------------------------------------
def pack_image_ref(img, Hp, Wp, lh, lw):
    """img [3][H][W] -> [Hp][Wp][4]: zero padded (top lh, left lw), 4th channel zero.  Exact."""
    img = d64(img)
    out = torch.zeros(Hp, Wp, 4, dtype=torch.float64)
    out[lh:lh + img.shape[1], lw:lw + img.shape[2], :3] = img.permute(1, 2, 0)
    return out, None


def pack_value_input_ref(image4, masks):
    """image4 [Hp][Wp][4], masks [K][Hp][Wp] -> [K][Hp][Wp][8] = (r, g, b, mask_k, sum_{j != k} mask_j, 0, 0, 0).
    Exact on 0 / 1 masks (the sum is a small integer)."""
    im, m = d64(image4), d64(masks)
    K = m.shape[0]
    out = torch.zeros(K, *m.shape[1:], 8, dtype=torch.float64)
    out[..., :3] = im[None, ..., :3]
    out[..., 3] = m
    out[..., 4] = m.sum(0, keepdim=True) - m
    return out, None


# ---------------------------------------------------------------------------------------------------------
# soft aggregation
# ---------------------------------------------------------------------------------------------------------
def aggregate_ref(p, dp=None, mut=None):
    """STM soft aggregation (model/aggregate.py through the oracle's aggregate): p [K][...] -> (prob [K+1][...], bound).
    new = clamp(cat(prod_k (1 - p_k), p), CLAMP_LO, CLAMP_HI), odds = new / (1 - new), prob = odds / sum odds.

    The operation is ill-conditioned where a probability saturates, so the bound follows its conditioning.  dp (default 0) is the
    ABSOLUTE error the caller's p already carries (logits_to_prob: the blend and the sigmoid).
      - a_k = 1 - p_k is off by da_k = dp_k + u a_k; the background product prod a_k by dbg = prod (a_k + da_k) (1 + K u) - prod a_k
        (K - 1 products, one spare);
      - the clamp is 1-Lipschitz and ABSORBS an error that stays beyond it: dq = 0 where q -+ dq stays clamped, else dp (dbg);
      - odds = q / (1 - q) is relatively off by dq / (q (1 - q)) (that is the u / (1 - q) of a saturated probability) + 2 u for the
        subtraction and the division;
      - the kernels go through l = log(odds) and exp(l - max l) as the oracle's softmax does: the logarithm is off by 2 u |l| (1 ulp),
        the subtraction by u |l - mx|, both ABSOLUTE errors of exp's argument and so relative errors of its value, + 4 u for exp
        itself (2 ulp); the error of mx is common to every term and cancels in the quotient.
        E_k = dq_k / (q_k (1 - q_k)) + (2 |l_k| + |l_k - mx| + 6) u.
      - prob_k = odds_k (1 + e_k) / sum_j odds_j (1 + e_j), |e_j| <= E_j: with S = sum_j prob_j E_j the relative error is at most
        (E_k + S) / (1 - S) (to first order E_k + S <= 2 max E); the denominator's K additions and the division add (K + 3) u.
        Where S >= 1/2 nothing is claimed beyond 0 <= prob <= 1 (bound 1): the data, not the kernel, decides there."""
    p = d64(p)
    K = p.shape[0]
    dp = torch.zeros_like(p) if dp is None else d64(dp)
    lo, hi = (1e-7, 1.0 - 1e-7) if mut == 'clamp_constants_in_float64' else (CLAMP_LO, CLAMP_HI)
    a = 1.0 - p
    bg = (a[1:] if mut == 'background_misses_object_0' else a).prod(0, keepdim=True)
    da = dp + U * a.abs()
    dbg = (a.abs() + da).prod(0, keepdim=True) * (1 + K * U) - a.abs().prod(0, keepdim=True)
    new, dnew = torch.cat([bg, p], 0), torch.cat([dbg, dp], 0)
    q = new.clamp(lo, hi)
    dq = torch.where((new - dnew >= hi) | (new + dnew <= lo), torch.zeros_like(dnew), dnew)
    odds = q / (1.0 - q)
    l = odds.log()
    mx = l.max(0, keepdim=True)[0]
    E = dq / (q * (1.0 - q)) + (2 * l.abs() + (l - mx).abs() + 6) * U
    num = odds.clone()
    if mut == 'numerator_8_recomputed' and K > 8:                       # object 9's numerator is not the value the denominator summed
        num[9] = num[9] * (1 + 1e-4)
    prob = num / odds.sum(0, keepdim=True)
    S = (prob * E).sum(0, keepdim=True)
    rel = torch.where(S < 0.5, (E + S) / (1.0 - S).clamp(min=0.5), torch.full_like(E, np.inf)) + (K + 3) * U
    return prob, (prob * rel).clamp(max=1.0)


def sum_to_one_bound(K):
    """|sum_c prob_c - 1| <= (K + 2) u: K additions in the denominator and one rounding per quotient, GIVEN that every numerator is
    the value the denominator summed."""
    return (K + 2) * U


def logits_to_prob_ref(logits, H, W, lh, lw, mut=None):
    """Decoder tail: logits [K][h4][w4] -> x4 bilinear -> sigmoid -> aggregation -> (cropped [K+1][H][W], padded [K+1][4 h4][4 w4]),
    each as (value, bound).  The blend's error dx (blend_bound) moves p = sigmoid(x) by at most sigmoid(x + dx) - sigmoid(x - dx)
    (monotone), the sigmoid itself adds sigmoid_err; aggregate_ref turns that dp into its conditioning bound."""
    lg = d64(logits)
    K, h4, w4 = lg.shape
    x, m = blend_ref(lg[..., None], 4 * h4, 4 * w4, 0.25, mut)
    x, dx = x[..., 0], blend_bound(x, m)[..., 0]
    p = torch.sigmoid(x)
    dp = (torch.sigmoid(x + dx) - torch.sigmoid(x - dx)) + sigmoid_err(x)
    prob, bound = aggregate_ref(p, dp, mut)
    crop = lambda t: t[:, lh:lh + H, lw:lw + W]
    return (crop(prob), crop(bound)), (prob, bound)


def merge_masks_ref(pred, mask, valid_bits, mut=None):
    """region = sum_k mask_k > 0.5 on the fp32 sum (k ascending); out_k = mask_k if bit k of valid_bits else (region ? 0 : pred_k)."""
    pred, mask = d64(pred), d64(mask)
    s = np.zeros(mask.shape[1:], np.float32)
    for k in range(mask.shape[0]):
        s = s + mask[k].numpy().astype(np.float32)
    region = torch.from_numpy(s >= np.float32(0.5) if mut == 'region_greater_equal' else s > np.float32(0.5))
    out = torch.where(region[None], torch.zeros_like(pred), pred)
    for k in range(mask.shape[0]):
        if (valid_bits >> k) & 1:
            out[k] = mask[k]
    return out, None


def argmax_ref(prob, mut=None):
    """torch.argmax(prob, 0) of prob [C][P]: the FIRST maximal index."""
    p = d64(prob).numpy()
    if mut == 'last_maximal_index':
        return torch.from_numpy(p.shape[0] - 1 - np.argmax(p[::-1], 0)), None
    return torch.from_numpy(np.argmax(p, 0)), None


# ---------------------------------------------------------------------------------------------------------
# the grid of cases (shared by the host and the GPU test) and their inputs
# ---------------------------------------------------------------------------------------------------------
STORAGE = ((0, 0), (0, 1), (1, 0), (1, 1))                 # (input is half, output is half)


def case(op, **kw):
    return dict(op=op, **kw)


def tag(c):
    return c['op'] + '(' + ', '.join(f'{k}={v}' for k, v in c.items() if k != 'op') + ')'


def maxpool_cases():
    for (H, W), C, B, data, (ih, oh) in itertools.product(itertools.product((1, 2, 3, 4, 5), (1, 2, 7, 8)), (4, 8, 68), (1, 3),
                                                          ('randn', 'negative'), STORAGE):
        yield case('maxpool', B=B, H=H, W=W, C=C, data=data, in_half=ih, out_half=oh)


def upsample_cases():
    for h, w, C, B, half in itertools.product((1, 2, 3), (1, 2, 3), (4, 12), (1, 3), (0, 1)):
        yield case('upsample2x_add', B=B, h=h, w=w, C=C, half=half)


def area_cases():
    for r, mult, C, (ih, oh), strided in itertools.product((1, 2, 4), ((1, 1), (2, 3)), (1, 3, 36), STORAGE, (0, 1)):
        yield case('area_downsample', B=2, H=mult[0] * r, W=mult[1] * r, C=C, r=r, in_half=ih, out_half=oh,
                   ldin=C + 5 * strided, in_off=2 * strided, ldout=C + 3 * strided, out_off=1 * strided)


def copy_cases():
    for (srcB, B), C, (ih, oh) in itertools.product(((1, 1), (1, 3), (3, 3), (2, 4)), (4, 20), STORAGE):
        yield case('copy_channels', srcB=srcB, B=B, P=5, C=C, in_half=ih, out_half=oh, ldsrc=C + 8, src_off=4, lddst=C + 12, dst_off=8)


def hidden_cases():
    for (K, h, w), (c16, c8, c4), spare in itertools.product(((1, 1, 1), (3, 2, 3)), ((4, 4, 4), (16, 8, 12)), (3, 7)):
        yield case('hidden_update_gather', K=K, h=h, w=w, c16=c16, c8=c8, c4=c4, ldout=c16 + c8 + c4 + 1 + spare)


def cbam_cases():
    for (H, W), C, B, data, half in itertools.product(((1, 1), (2, 3), (4, 4), (1, 17), (17, 1), (5, 7)), (16, 48, 64, 528), (1, 3),
                                                      ('randn', 'negative'), (0, 1)):
        yield case('cbam_residual', B=B, H=H, W=W, C=C, data=data, half=half)


def gru_cases():
    for Ch, N, inplace, data, half in itertools.product((1, 3, 64), (1, 35), (0, 1), ('randn', 'saturated'), (0, 1)):
        yield case('gru_gate', Ch=Ch, N=N, inplace=inplace, data=data, half=half)


def logits_cases():
    for K, (h4, w4), crop, pad, data in itertools.product((1, 8, 9, 12), ((1, 1), (1, 3), (2, 2), (5, 7)), (0, 1), (0, 1),
                                                          ('randn4', 'saturated', 'mixed')):
        H, W, lh, lw = (4 * h4 - 2, 4 * w4 - 3, 1, 2) if crop else (4 * h4, 4 * w4, 0, 0)
        yield case('logits_to_prob', K=K, h4=h4, w4=w4, H=H, W=W, lh=lh, lw=lw, padded=pad, data=data)


def aggregate_cases():
    for K, data in itertools.product((1, 8, 9, 12), ('hard', 'uniform', 'overlap')):
        yield case('aggregate_masks', K=K, H=9, W=13, data=data)


def resize_cases():
    for (i, o), C in itertools.product((((1, 1), (3, 5)), ((3, 5), (1, 1)), ((4, 6), (4, 6)), ((7, 9), (5, 4)), ((1, 9), (4, 20)),
                                        ((6, 1), (13, 3))), (1, 3)):
        yield case('resize_bilinear', C=C, Hi=i[0], Wi=i[1], Ho=o[0], Wo=o[1])


def merge_cases():
    for K, valid in itertools.product((1, 3, 64), ('none', 'all', 'bit0', 'last')):
        bits = {'none': 0, 'all': (1 << K) - 1, 'bit0': 1, 'last': 1 << (K - 1)}[valid]
        yield case('merge_masks', K=K, H=5, W=11, valid_bits=bits)


def argmax_cases():
    for C, P in itertools.product((1, 2, 255), (1, 300)):
        yield case('argmax_u8', C=C, P=P)


CASES = dict(maxpool=maxpool_cases, upsample2x_add=upsample_cases, area_downsample=area_cases, copy_channels=copy_cases,
             hidden_update_gather=hidden_cases, cbam_residual=cbam_cases, gru_gate=gru_cases, logits_to_prob=logits_cases,
             aggregate_masks=aggregate_cases, resize_bilinear=resize_cases, merge_masks=merge_cases, argmax_u8=argmax_cases)


def cbam_weights(C):
    """Seeded float32 CBAM weights at the checkpoint's scales (std: mlp.1 0.044 / 0.017, mlp.3 0.18 / 0.02, spatial 0.10 / 0.02)."""
    g = rng_of('cbam_weights', C)
    Cr = C // 16
    return dict(w1=randn(g, Cr, C) * 0.044, b1=randn(g, Cr) * 0.017, w2=randn(g, C, Cr) * 0.18, b2=randn(g, C) * 0.02,
                sw=randn(g, 2, 7, 7) * 0.10, sb=randn(g, 1) * 0.02)


def make_inputs(c):
    """The case's input tensors (float32; for half storage values a half holds exactly), seeded by the case."""
    g = rng_of(tag({k: v for k, v in c.items() if k not in ('in_half', 'out_half', 'half', 'inplace', 'padded')}))
    op = c['op']
    ih = bool(c.get('in_half', c.get('half', 0)))
    if op == 'maxpool':
        x = randn(g, c['B'], c['H'], c['W'], c['C'])
        x = -x.abs() - 0.5 if c['data'] == 'negative' else x
        return dict(x=x.half().float() if ih else x)
    if op == 'upsample2x_add':
        return dict(g=randn(g, c['B'], c['h'], c['w'], c['C'], half=ih), skip=randn(g, 2 * c['h'], 2 * c['w'], c['C'], half=ih))
    if op == 'area_downsample':
        return dict(x=randn(g, c['B'], c['H'], c['W'], c['C'], half=ih))
    if op == 'copy_channels':
        return dict(src=randn(g, c['srcB'], c['P'], c['C'], half=ih))
    if op == 'hidden_update_gather':
        K, h, w = c['K'], c['h'], c['w']
        return dict(g16=randn(g, K, h, w, c['c16']), g8=randn(g, K, 2 * h, 2 * w, c['c8']), g4=randn(g, K, 4 * h, 4 * w, c['c4']),
                    logits=randn(g, K, 4 * h, 4 * w) * 4)
    if op == 'cbam_residual':
        x = randn(g, c['B'], c['H'], c['W'], c['C']) * 0.5
        x = -x.abs() - 0.25 if c['data'] == 'negative' else x
        return dict(g=x.half().float() if ih else x, **cbam_weights(c['C']))
    if op == 'gru_gate':
        v = randn(g, c['N'], 3 * c['Ch'])
        if c['data'] == 'saturated':                   # every gate at +-30 / +-100, with a few ordinary values left in
            pick = torch.randint(0, 5, v.shape, generator=g)
            v = torch.where(pick == 4, v, torch.tensor([30.0, -30.0, 100.0, -100.0])[pick.clamp(max=3)])
        return dict(values=v.half().float() if ih else v, h=randn(g, c['N'], c['Ch']))
    if op == 'logits_to_prob':
        K, h4, w4 = c['K'], c['h4'], c['w4']
        x = randn(g, K, h4, w4) * 4
        if c['data'] == 'saturated':
            x = torch.where(x > 0, torch.full_like(x, 40.0), torch.full_like(x, -40.0))
        elif c['data'] == 'mixed':                     # object 0 and the background both saturate on part of the map; the rest ordinary
            sat, up = torch.rand(h4, w4, generator=g) < 0.5, torch.rand(h4, w4, generator=g) < 0.5
            sat[0, 0] = up[0, 0] = True                # the first pixel always: object 0 at +40 over a background at its floor
            x = torch.where(sat[None], torch.full_like(x, -40.0), x)
            x[0] = torch.where(sat, torch.where(up, torch.tensor(40.0), torch.tensor(-40.0)), x[0])
        return dict(logits=x)
    if op == 'aggregate_masks':
        K, H, W = c['K'], c['H'], c['W']
        if c['data'] == 'uniform':
            return dict(masks=torch.rand(K, H, W, generator=g))
        owner = torch.randint(0, K + 1, (H, W), generator=g)          # K = nobody
        m = torch.stack([(owner == k).float() for k in range(K)])
        if c['data'] == 'overlap' and K > 1:                            # two objects both 1 on a third of the pixels
            both = torch.rand(H, W, generator=g) < 0.33
            m[0] = torch.where(both, torch.tensor(1.0), m[0])
            m[K - 1] = torch.where(both, torch.tensor(1.0), m[K - 1])
        return dict(masks=m)
    if op == 'resize_bilinear':
        return dict(x=torch.rand(c['C'], c['Hi'], c['Wi'], generator=g))
    if op == 'merge_masks':
        K, H, W = c['K'], c['H'], c['W']
        pred = torch.rand(K, H, W, generator=g)
        owner = torch.randint(0, K + 1, (H, W), generator=g)
        m = torch.stack([(owner == k).float() for k in range(K)])
        m[:, 0, :] = 0.0
        m[0, 0, 0::2] = 0.25 if K > 1 else 0.5                          # row 0: sums of exactly 0.5 (two 0.25s; K = 1: one 0.5) ...
        m[K - 1, 0, 0::2] += 0.25 if K > 1 else 0.0
        m[0, 0, 1::2] = 0.5 + 2.0 ** -20                                # ... and just above
        return dict(pred=pred, mask=m)
    if op == 'argmax_u8':
        C, P = c['C'], c['P']
        p = torch.rand(C, P, generator=g).mul(64).floor() / 64          # well separated: multiples of 1/64, many natural ties at C = 255
        if C > 1:
            p[:, 0] = 0.5                                               # every channel equal
            if P > 2:
                p[:, 1] = 0.0
                p[C // 2, 1] = p[C - 1, 1] = 2.0                        # two channels equal
        return dict(prob=p)
    raise KeyError(op)


def reference(c, i, mut=None):
    """(value, bound | None) of the case in the destination's logical shape; bound already includes the half-storage term."""
    op = c['op']
    oh = bool(c.get('out_half', c.get('half', 0)))
    kw = {} if mut is None else dict(mut=mut)
    if op == 'maxpool':
        ref, b = maxpool_ref(i['x'], **kw)
    elif op == 'upsample2x_add':
        ref, b = upsample2x_add_ref(i['g'], i['skip'], **kw)
    elif op == 'area_downsample':
        ref, b = area_ref(i['x'], c['r'], **kw)
    elif op == 'copy_channels':
        ref, b = copy_channels_ref(i['src'], c['B'], **kw)
    elif op == 'hidden_update_gather':
        ref, b = hidden_gather_ref(i['g16'], i['g8'], i['g4'], i['logits'])
    elif op == 'cbam_residual':
        ref, b, _ = cbam_ref(i['g'], i['w1'], i['b1'], i['w2'], i['b2'], i['sw'], i['sb'], **kw)
    elif op == 'gru_gate':
        ref, b = gru_gate_ref(i['values'], i['h'], **kw)
        oh = False                                                      # the state stays fp32
    elif op == 'logits_to_prob':
        ref, b = logits_to_prob_ref(i['logits'], c['H'], c['W'], c['lh'], c['lw'], **kw)[0]
    elif op == 'aggregate_masks':
        ref, b = aggregate_ref(i['masks'].reshape(c['K'], -1), **kw)
    elif op == 'resize_bilinear':
        ref, b = resize_bilinear_ref(i['x'], c['Ho'], c['Wo'], **kw)
    elif op == 'merge_masks':
        ref, b = merge_masks_ref(i['pred'], i['mask'], c['valid_bits'], **kw)
    elif op == 'argmax_u8':
        ref, b = argmax_ref(i['prob'], **kw)
    else:
        raise KeyError(op)
    if b is None:
        return (round_to(ref, oh) if ref.dtype == torch.float64 else ref), None
    return ref, (half_bound(b, ref) if oh else b)
