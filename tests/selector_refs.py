"""Plain float64 statement of the annotation-candidate selector (xmem_selector_prepare / xmem_selector_prepare_u8 /
xmem_cycle_dissimilarity), its data regimes and the bounds its tests hold the kernels to.

Written from the header comments of include/xmem_hip.h, from the oracle (oracle/cpu_ref.py: composite_keys_and_validity,
cycle_dissimilarity, get_similarity) and from the operand layout csrc/selector.hip documents, not from the kernel bodies.  No GPU.
Row-major operands, as the C ABI takes them: key / sel [HW, Ck] per frame, Mexp / Qexp [F, HW, 2 Ck], bsq / shrinkage [F, HW].
tests/test_selector_refs_host.py ties everything here to the oracle on the CPU; tests/test_gpu_selector_edges.py runs the kernels.

Regimes
  exact   the operand sets of affinity_refs' exact regime: keys multiples of 1/2 in [-2, 2], e multiples of 1/4 in [0, 1], shrinkage in
          {1/2, 1, 2, 4}, mask weights in {0, 1}, alpha in {0, 1/2, 1}.  The composite key is then a multiple of 1/4 in [-2, 2], every
          product c^2 e, 2 c e and e c^2 a multiple of 1/64, every partial sum of the 128-term dot and b_sq a multiple of 1/64 below
          2^10, the scale shrinkage / 8 a power of two, so vf, vr and vf - vr are multiples of 2^-Q (Q = 10) below 2^10: exact in fp32 in
          any order.  is_exact_regime checks the set membership and, on the data, that 64 max term 2^Q < 2^24, so the fp32 sum of any 64
          terms is exact too.  The kernel's per-tile float64 partials and its scores must EQUAL the reference.
  dense   normal keys (x 0.9), e in [0.05, 0.95], shrinkage in [1, 4], float mask weights in [0, 1], any alpha; held to
          score_tile_bound.

Conditions that keep the exact cases from being vacuous (assert_not_vacuous, called by make_inputs for the exact regime)
  (a) the share of strictly positive relu terms of every scored frame (f != chosen) lies in [0.25, 0.75];
  (b) every tile partial of every scored frame is non-zero;
  (c) the F scores of one chosen frame are pairwise different.
  One case cannot meet them as stated: terms(chosen = a, f = b)[i][j] = relu(x) and terms(chosen = b, f = a)[i][j] = relu(-x) for the
  same x, so a tile of ONE element (the corner tile when HW = 1 mod 128, HW = 1 included) is zero in one of the two directions whatever
  the data.  There the condition is x != 0: the tile is non-zero in exactly one direction, and the tests score every frame in turn
  as `chosen`, so both signs are seen.  At HW = 1 a frame has one term: (a) is waived and (c) asks that the non-zero scores differ.
"""
import numpy as np
import torch
import torch.nn.functional as F

import affinity_refs as A
import memory_kernel_refs as M

U = M.U
CK = 64            # the only width the score kernel serves
TILE = 128         # output block of one workgroup: one float64 partial per tile, row tile major, column tile minor
Q_BITS = 10        # exact regime: every relu term is a multiple of 2^-Q_BITS (1/64 from the products, 1/2 the least shrinkage, 1/8)
EXACT_ALPHAS = (0.0, 0.5, 1.0)
f32 = np.float32


def _np(t, dtype):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=dtype)


def n_tiles(hw):
    return -(-hw // TILE)


# ---------------------------------------------------------------------------------------------------------
# prepare
# ---------------------------------------------------------------------------------------------------------
def nearest(planes, h, w):
    """[C, H, W] float32 -> [C, h, w]: the pixels torch.nn.functional.interpolate(mode='nearest') reads on the CPU (the oracle's call)."""
    return F.interpolate(torch.as_tensor(planes).detach().cpu().float()[None], size=(h, w), mode='nearest')[0]


def prepare_ref(key_rows, sel_rows, mask, h, w, alpha, eps=0.5):
    """One frame.  key_rows / sel_rows [h w, Ck] float32; mask [C, H, W] float32 | None.  Returns a dict:
      ck [HW, Ck] float32      fl(fl(fl(k m) a) + fl(k fl(1 - a))), m = max over the channels at the nearest-resize source pixel, a = fl(alpha),
                               1 - alpha taken in double and rounded once (the Python wrapper passes float(1 - alpha)); mask None: ck = key
      Mexp, Qexp [HW, 2 Ck]    float32 [ck^2, ck] and [-e, 2 (ck e)]: every entry one rounded operation (2 x is exact)
      bsq [HW] float64         sum_c e ck^2 of the float32 ck and e;  bsq_bound = (Ck + 2) u sum_c |e ck^2|
      presence int             #{pixels of the full-resolution mask with max_c mask > fl(eps)}, strictly greater (0 without a mask)"""
    k, e = _np(key_rows, f32), _np(sel_rows, f32)
    hw, ck_w = k.shape
    assert hw == h * w and e.shape == k.shape
    if mask is None:
        ck, presence = k.copy(), 0
    else:
        mk = torch.as_tensor(mask).detach().cpu().float()
        assert mk.dim() == 3
        presence = int((mk.max(0).values.numpy() > f32(eps)).sum())
        m = nearest(mk, h, w).max(0).values.reshape(hw, 1).numpy()
        a, b = f32(alpha), f32(1.0 - float(alpha))
        ck = (k * m) * a + k * b
    assert ck.dtype == f32
    Mexp = np.concatenate([ck * ck, ck], 1)
    Qexp = np.concatenate([-e, f32(2) * (ck * e)], 1)
    assert Mexp.dtype == f32 and Qexp.dtype == f32
    t = e.astype(np.float64) * ck.astype(np.float64) ** 2
    return dict(ck=ck, Mexp=Mexp, Qexp=Qexp, bsq=t.sum(1), bsq_bound=(ck_w + 2) * U * np.abs(t).sum(1), presence=presence)


# ---------------------------------------------------------------------------------------------------------
# score
# ---------------------------------------------------------------------------------------------------------
def pair_terms(Mexp, Qexp, bsq, shr, chosen, f):
    """relu(fwd - rev) [HW, HW] float64 of frame f against frame `chosen` (A = chosen, B = f):
       fwd[i][j] = (sum_k MA[i,k] QB[j,k] - bsqB[j]) sA[i] / sqrt(Ck),  rev[i][j] = (sum_k MB[i,k] QA[j,k] - bsqA[j]) sB[i] / sqrt(Ck)."""
    Mx, Qx, b, s = _np(Mexp, np.float64), _np(Qexp, np.float64), _np(bsq, np.float64), _np(shr, np.float64)
    rs = np.sqrt(Mx.shape[2] // 2)
    fwd = (Mx[chosen] @ Qx[f].T - b[f][None, :]) * s[chosen][:, None] / rs
    rev = (Mx[f] @ Qx[chosen].T - b[chosen][None, :]) * s[f][:, None] / rs
    return np.maximum(fwd - rev, 0.0)


def tile_sums(x):
    """[HW, HW] -> [tiles, tiles]: the sums over TILE x TILE blocks (the last row and column of tiles may be partial)."""
    hw = x.shape[0]
    t = n_tiles(hw)
    p = np.zeros((t * TILE, t * TILE), np.float64)
    p[:hw, :hw] = x
    return p.reshape(t, TILE, t, TILE).sum((1, 3))


def score_ref(Mexp, Qexp, bsq, shr, chosen, valid=None):
    """float64 from the float32 operands the score kernel is given.  Returns (tiles [F, t, t], scores [F]): the per-tile sums of
    relu(fwd - rev) in the layout the kernel leaves in its workspace, and their total / HW^2.  valid[f] == 0: zeros."""
    nf, hw = np.shape(Mexp)[0], np.shape(Mexp)[1]
    t = n_tiles(hw)
    tiles = np.zeros((nf, t, t), np.float64)
    for f in range(nf):
        if valid is None or int(valid[f]):
            tiles[f] = tile_sums(pair_terms(Mexp, Qexp, bsq, shr, chosen, f))
    return tiles, tiles.sum((1, 2)) / (float(hw) * float(hw))


def score_tile_bound(Mexp, Qexp, bsq, shr, chosen, valid=None):
    """Dense regime.  Per element and direction e = (2 Ck + 4) u (sum_k |M| |Q| + |bsq|) s / sqrt(Ck) (the constant of
    memory_kernel_refs.similarity_dense_bound; relu is 1-Lipschitz, so a term is off by at most e_fwd + e_rev); per tile
    sum (e_fwd + e_rev) + 66 u sum relu terms (the fp32 sum of a lane's 64 terms and the cast).  Returns (tile bounds [F, t, t],
    score bounds [F] = their total / HW^2).  Derived, nothing measured."""
    Mx, Qx = np.abs(_np(Mexp, np.float64)), np.abs(_np(Qexp, np.float64))
    b, s = np.abs(_np(bsq, np.float64)), np.abs(_np(shr, np.float64))
    nf, hw, k2 = Mx.shape
    ck = k2 // 2
    c = (2 * ck + 4) * U / np.sqrt(ck)
    t = n_tiles(hw)
    out = np.zeros((nf, t, t), np.float64)
    for f in range(nf):
        if valid is None or int(valid[f]):
            e_fwd = c * (Mx[chosen] @ Qx[f].T + b[f][None, :]) * s[chosen][:, None]
            e_rev = c * (Mx[f] @ Qx[chosen].T + b[chosen][None, :]) * s[f][:, None]
            out[f] = tile_sums(e_fwd + e_rev) + 66 * U * tile_sums(pair_terms(Mexp, Qexp, bsq, shr, chosen, f))
    return out, out.sum((1, 2)) / (float(hw) * float(hw))


# ---------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------
def make_inputs(regime, nf, hw, seed, alpha=0.5, ck=CK, vacuity=True):
    """dict of CPU float32 tensors: key / sel [F, HW, ck], shr / m [F, HW] (m: the mask weight of each key pixel), alpha, the score
    kernel's operands Mexp / Qexp [F, HW, 2 ck] and bsq [F, HW] (prepare_ref of every frame, bsq rounded to float32) and, per chosen
    frame, the reference d['tiles'][chosen] [F, t, t] and d['scores'][chosen] [F] (valid = None).  Computed once; never modified.
    vacuity=False leaves assert_not_vacuous out (for callers that take only the draws and bring their own masks)."""
    gen = torch.Generator().manual_seed(seed)
    if regime == 'exact':
        assert alpha in EXACT_ALPHAS
        key = A._draw(A._HALVES, A._HALF_P, (nf, hw, ck), gen)
        ev = torch.arange(0, 5, dtype=torch.float32) * 0.25
        sel = A._draw(ev, torch.ones(ev.numel()), (nf, hw, ck), gen)
        shr = A._draw(torch.tensor([0.5, 1., 2., 4.]), torch.ones(4), (nf, hw), gen)
        m = torch.randint(0, 2, (nf, hw), generator=gen).float()
    elif regime == 'dense':
        key = torch.randn(nf, hw, ck, generator=gen) * 0.9
        sel = torch.rand(nf, hw, ck, generator=gen) * 0.9 + 0.05
        shr = torch.rand(nf, hw, generator=gen) * 3 + 1
        m = torch.rand(nf, hw, generator=gen)
    else:
        raise ValueError(regime)
    prep = [prepare_ref(key[f], sel[f], m[f].view(1, hw, 1), hw, 1, alpha) for f in range(nf)]
    d = dict(regime=regime, alpha=alpha, key=key, sel=sel, shr=shr, m=m,
             Mexp=torch.from_numpy(np.stack([p['Mexp'] for p in prep])), Qexp=torch.from_numpy(np.stack([p['Qexp'] for p in prep])),
             bsq=torch.from_numpy(np.stack([p['bsq'] for p in prep]).astype(f32)), bsq64=np.stack([p['bsq'] for p in prep]))
    d['tiles'], d['scores'] = {}, {}
    for c in range(nf):
        d['tiles'][c], d['scores'][c] = score_ref(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], c)
    if regime == 'exact':
        assert is_exact_regime(d), 'operands outside the exact regime'
        if vacuity:
            assert_not_vacuous(d)
    return d


def exact_bits(d):
    """(all terms multiples of 2^-Q_BITS, log2(64 max term 2^Q_BITS)) over every ordered pair of frames."""
    nf = d['Mexp'].shape[0]
    ok, top = True, 0.0
    for c in range(nf):
        for f in range(nf):
            if f != c:
                t = pair_terms(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], c, f) * 2.0 ** Q_BITS
                ok = ok and bool(np.all(t == np.round(t)))
                top = max(top, float(t.max()))
    return ok, float(np.log2(max(64.0 * top, 1.0)))


def is_exact_regime(d):
    """The premise of the exact regime's argument, on the data: operand membership, bsq exactly representable, every relu term a
    multiple of 2^-Q_BITS, and 64 max term 2^Q_BITS < 2^24 (any lane's fp32 sum of 64 terms is exact)."""
    on = lambda t, step, lo, hi: bool(((t / step) == (t / step).round()).all() and t.min() >= lo and t.max() <= hi)
    sets = (on(d['key'], 0.5, -2, 2) and on(d['sel'], 0.25, 0, 1) and bool(torch.isin(d['shr'], torch.tensor([0.5, 1., 2., 4.])).all())
            and bool(torch.isin(d['m'], torch.tensor([0., 1.])).all()) and d['alpha'] in EXACT_ALPHAS
            and on(d['Mexp'][..., d['Mexp'].shape[2] // 2:], 0.25, -2, 2) and np.array_equal(d['bsq'].numpy().astype(np.float64), d['bsq64']))
    if not sets:
        return False
    unit, bits = exact_bits(d)
    return unit and bits < 24.0


def assert_not_vacuous(d):
    """Conditions (a) - (c) of the module docstring; returns the (least, largest) share of positive terms."""
    nf, hw = d['Mexp'].shape[0], d['Mexp'].shape[1]
    one = hw % TILE == 1                                         # the corner tile holds one element
    lo, hi, nonzero_scores = 1.0, 0.0, []
    for c in range(nf):
        for f in range(nf):
            if f == c:
                continue
            t = pair_terms(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], c, f)
            tiles = d['tiles'][c][f].copy()
            if one:
                back = pair_terms(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], f, c)
                assert (t[-1, -1] > 0) != (back[-1, -1] > 0), f'HW={hw}: corner term of frames {c},{f} is zero in both directions'
                tiles[-1, -1] = 1.0
            assert np.all(tiles > 0), f'HW={hw} chosen={c} f={f}: a tile partial is zero'
            if hw > 1:
                share = float((t > 0).mean())
                lo, hi = min(lo, share), max(hi, share)
                assert 0.25 <= share <= 0.75, f'HW={hw} chosen={c} f={f}: share of positive terms {share:.3f}'
            elif d['scores'][c][f] > 0:
                nonzero_scores.append(d['scores'][c][f])
        if hw > 1:
            assert np.unique(d['scores'][c]).size == nf, f'HW={hw} chosen={c}: frames share a score'
    assert np.unique(nonzero_scores).size == len(nonzero_scores), f'HW={hw}: frames share a score'
    return lo, hi


# ---------------------------------------------------------------------------------------------------------
# the exact-regime edge shapes of the score kernel: one partial wave block, both 32-row halves, a wave-block edge, a tile edge, 3 x 3
# tiles with a one-row last tile, and 17 x 17 = 289 tiles (more than the reduce kernel's 256 threads) with a one-row last tile.
# HW -> (frames, seed, alpha): alpha cycles through the exact set; the seed is the first of 1, 2, ... whose draw meets
# assert_not_vacuous (a property of the reference alone; ties and all-zero one-row tiles are common among few-bit operands).
# ---------------------------------------------------------------------------------------------------------
EDGE_HW = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
EDGE_CASES = {1: (3, 1, 0.5), 31: (3, 1, 1.0), 32: (3, 1, 0.0), 33: (3, 1, 0.5), 63: (3, 1, 1.0), 64: (3, 1, 0.0), 65: (3, 1, 0.5),
              127: (3, 1, 1.0), 128: (3, 1, 0.0), 129: (3, 1, 0.5), 257: (3, 5, 1.0), 2049: (2, 1, 0.5)}
_EDGE_CACHE = {}


def edge_case(hw):
    """make_inputs('exact', ...) of one EDGE_CASES entry, computed once per process."""
    if hw not in _EDGE_CACHE:
        nf, seed, alpha = EDGE_CASES[hw]
        _EDGE_CACHE[hw] = make_inputs('exact', nf, hw, seed, alpha=alpha)
    return _EDGE_CACHE[hw]
