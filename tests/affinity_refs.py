"""Plain float64 statement of the affinity top-k (xmem_affinity_topk / xmem_affinity_topk_hinted), the data regimes and adversarial
memory orderings its tests run, the checker they hold the kernels to, and the table of named shapes with the route each must take.

Written from the header comments of include/xmem_hip.h and from the oracle (oracle/cpu_ref.py), not from the kernels.  No GPU.
Row-major operands, as the C ABI takes them: key [n, 64], shrinkage [n], qk / qe [HW, 64]; similarities [HW, n].
tests/test_affinity_refs_host.py ties everything here to the oracle on the CPU; tests/test_gpu_affinity_edges.py runs the kernels.

Regimes
  exact   every operand a dyadic rational with few bits (x, k multiples of 1/2 in [-2, 2]; e multiples of 1/4 in [0, 1] - [-1, 1] for
          the mixed-sign ordering; shrinkage in {1/2, 1, 2, 4}).  Every term x^2 e, 2 x k e, e k^2 is a multiple of 1/16 below 8, so
          any partial sum of the 192 terms is a multiple of 1/16 below 2^11: exact in fp32 in any order and under any FMA contraction;
          the scale shrinkage / 8 is a power of two.  The filter's operand rows ms/8 x^2 and ms/8 x are multiples of 1/64 of at
          most 2: exact in fp16.  The kernels must return the reference's values and indices exactly.  Full of exact ties.
  dense   normal keys (x 0.9), shrinkage in [1, 4], e in [0.05, 0.95]; held to similarity_dense_bound.
"""
import numpy as np
import torch

import memory_kernel_refs as M

U = M.U
CK = 64
SMALL, LARGE_SAMPLED, LARGE_HINTED_FP32, LARGE_HINTED_FILTER16 = 0, 1, 2, 3     # XMEM_AFF_* (include/xmem_hip.h)
ROUTES = ('small', 'large-sampled', 'large-hinted-fp32', 'large-hinted-filter16')
ORDERINGS = ('ascending', 'descending', 'clustered', 'all_tied', 'tie_at_kth', 'unsampled', 'zero_sim', 'mixed_sign')


# ---------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------
def similarity_ref(key, shr, qk, qe):
    """float64 [HW, n] (the oracle's get_similarity on float64 inputs)."""
    return M.similarity_dense_ref(key, shr, qk, qe)


def topk_ref(sim64, k):
    """Per row of sim64 [HW, n]: the k best by (value descending, index ascending); -0.0 == +0.0.  Returns (values, indices)."""
    sim64 = np.asarray(sim64, np.float64)
    hw, n = sim64.shape
    if not 1 <= k <= n:
        raise ValueError('k out of range')
    kth = np.partition(sim64, n - k, axis=1)[:, n - k]
    idx = np.empty((hw, k), np.int64)
    for q in range(hw):
        cand = np.nonzero(sim64[q] >= kth[q])[0]                       # ascending index
        idx[q] = cand[np.argsort(-sim64[q, cand], kind='stable')[:k]]
    return np.take_along_axis(sim64, idx, 1), idx


def weights_ref(vals):
    """exp(v) / sum exp(v) over the last axis, float64, no max shift (model/memory_util.py:48-49)."""
    e = np.exp(np.asarray(vals, np.float64))
    return e / e.sum(-1, keepdims=True)


def weights_rel_bound(k):
    """(16 + k/8) u: expf, the sum tree and the division (the constant of softmax_suffix_rel_bound)."""
    return (16.0 + k / 8.0) * U


# ---------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------
_HALVES = torch.arange(-4, 5, dtype=torch.float32) * 0.5
_HALF_P = torch.tensor([1., 1., 2., 4., 6., 4., 2., 1., 1.])         # concentrated around 0: the best similarities stay above -80


def _draw(values, probs, shape, gen):
    return values[torch.multinomial(probs, int(np.prod(shape)), replacement=True, generator=gen)].reshape(shape)


def make_inputs(regime, n, hw, seed, signed_e=False):
    """dict(key [n,64], shr [n], qk [hw,64], qe [hw,64]) of CPU float32 tensors."""
    gen = torch.Generator().manual_seed(seed)
    if regime == 'exact':
        key = _draw(_HALVES, _HALF_P, (n, CK), gen)
        qk = _draw(_HALVES, _HALF_P, (hw, CK), gen)
        ev = torch.arange(-4 if signed_e else 0, 5, dtype=torch.float32) * 0.25
        qe = _draw(ev, torch.ones(ev.numel()), (hw, CK), gen)
        shr = _draw(torch.tensor([0.5, 1., 2., 4.]), torch.ones(4), (n,), gen)
    elif regime == 'dense':
        key = torch.randn(n, CK, generator=gen) * 0.9
        qk = torch.randn(hw, CK, generator=gen) * 0.9
        qe = torch.rand(hw, CK, generator=gen) * 0.9 + 0.05
        if signed_e:
            qe = qe * (torch.randint(0, 2, (hw, CK), generator=gen).float() * 2 - 1)
        shr = torch.rand(n, generator=gen) * 3 + 1
    else:
        raise ValueError(regime)
    return dict(key=key, shr=shr, qk=qk, qe=qe)


def is_exact_regime(d, signed_e=False):
    """Every operand in the exact regime's set (the premise of its exactness argument)."""
    on = lambda t, step, lo, hi: bool(((t / step) == (t / step).round()).all() and t.min() >= lo and t.max() <= hi)
    return (on(d['key'], 0.5, -2, 2) and on(d['qk'], 0.5, -2, 2) and on(d['qe'], 0.25, -1 if signed_e else 0, 1)
            and bool(torch.isin(d['shr'], torch.tensor([0.5, 1., 2., 4.])).all()))


def order_memory(d, ordering, k, positions=None, seed=0):
    """One memory against one query tile: returns a new dict in which queries 0 .. min(hw, 64) - 1 are copies of query 0 and the memory
    rows are arranged against it.  Rows are permuted or copied, never altered, so a regime's operand set is kept.
      ascending   similarity to query 0 strictly non-decreasing with the index: every row beats (or ties) all earlier ones
      descending  the reverse
      clustered   the k best rows sit at `positions` (k indices, ascending), the rest keep their order
      all_tied    every row is a copy of row 0
      tie_at_kth  100 scattered rows are copies of the k-th best row (k - 1 rows stay above them)
      unsampled   best rows first into the tiles with tile % 4 != 0, the worst quarter into the tiles with tile % 4 == 0
      zero_sim    query 0 has e = 0 (every similarity is a zero) and rows 0 .. 2k-1 alternate -qk[0], +qk[0]; for q >= 1 row
                  2k + 2(q-1) + 1 equals qk[q] (similarity exactly 0, the maximum for e >= 0)
      mixed_sign  no rearrangement: the caller draws qe with both signs (make_inputs(signed_e=True))"""
    key, shr, qk, qe = (d[x].clone() for x in ('key', 'shr', 'qk', 'qe'))
    n, hw = key.shape[0], qk.shape[0]
    tile = min(hw, 64)
    if ordering != 'zero_sim':
        qk[:tile] = qk[0]
        qe[:tile] = qe[0]
    if ordering == 'mixed_sign':
        return dict(key=key, shr=shr, qk=qk, qe=qe)
    if ordering == 'all_tied':
        key[:] = key[0]
        shr[:] = shr[0]
        return dict(key=key, shr=shr, qk=qk, qe=qe)
    if ordering == 'zero_sim':
        assert n >= 2 * k + 2 * hw
        qe[0] = 0.0
        nz = torch.where(qk[0] == 0, torch.full_like(qk[0], 0.5), qk[0])      # no zero entry: every product below has a sign
        qk[0] = nz
        key[0:2 * k:2] = -nz
        key[1:2 * k:2] = nz
        for q in range(1, hw):
            key[2 * k + 2 * (q - 1) + 1] = qk[q]
        return dict(key=key, shr=shr, qk=qk, qe=qe)
    s0 = similarity_ref(key, shr, qk[:1], qe[:1])[0]
    desc = np.argsort(-s0, kind='stable')
    if ordering == 'ascending':
        perm = desc[::-1].copy()
    elif ordering == 'descending':
        perm = desc
    elif ordering == 'clustered':
        positions = np.asarray(positions, np.int64)
        assert positions.shape == (k,) and positions.min() >= 0 and positions.max() < n and np.unique(positions).size == k
        best = desc[:k]
        rest = np.setdiff1d(np.arange(n), best)                              # ascending
        perm = np.empty(n, np.int64)
        free = np.ones(n, bool)
        free[positions] = False
        perm[positions] = best
        perm[free] = rest
    elif ordering == 'unsampled':
        t = np.arange(n) // 32
        slots = np.concatenate([np.nonzero(t % 4 != 0)[0], np.nonzero(t % 4 == 0)[0]])
        perm = np.empty(n, np.int64)
        perm[slots] = desc
    elif ordering == 'tie_at_kth':
        assert n >= k + 100
        rng = np.random.default_rng(seed)
        spots = torch.from_numpy(np.sort(rng.choice(desc[k:], 100, replace=False)))
        key[spots] = key[int(desc[k - 1])].clone()
        shr[spots] = shr[int(desc[k - 1])].clone()
        return dict(key=key, shr=shr, qk=qk, qe=qe)
    else:
        raise ValueError(ordering)
    perm = torch.from_numpy(np.ascontiguousarray(perm))
    return dict(key=key[perm].contiguous(), shr=shr[perm].contiguous(), qk=qk, qe=qe)


# ---------------------------------------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------------------------------------
def check_topk(got_idx, got_sim, got_w, ref64, bound, k, exact=False, tag='', detail=None):
    """Every query, no sampling.  got_* [HW, k]; ref64 [HW, n] float64; bound [HW, n] float64 (ignored under exact: 0).
    (a) indices distinct and in [0, n);  (b) |got_sim[s] - ref64[idx[s]]| <= bound[idx[s]] (exact: equality);
    (c) (got_sim, idx) strictly descending in (value descending, index ascending), -0.0 == +0.0;
    (d) no unpicked j with ref64[j] - bound[j] > min_s (ref64[idx_s] + bound[idx_s]);
    (e) got_w against float64 exp / sum of the kernel's own got_sim, relative error <= (16 + k/8) u (got_w None: skipped);
    under exact, idx == topk_ref.  Returns (largest err/bound of (b) and (e), share of queries whose index set equals topk_ref's);
    a dict passed as `detail` receives the two parts, detail['sim'] and detail['w']."""
    ref64 = np.asarray(ref64, np.float64)
    hw, n = ref64.shape
    idx = np.asarray(got_idx).astype(np.int64)
    sim = np.asarray(got_sim, np.float64)
    assert idx.shape == (hw, k) and sim.shape == (hw, k), f'{tag}: output shape'
    bnd = np.zeros_like(ref64) if exact else np.asarray(bound, np.float64)
    assert np.all((idx >= 0) & (idx < n)), f'{tag}: (a) index outside [0, {n})'
    srt = np.sort(idx, 1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), f'{tag}: (a) duplicate index within a query'
    r = np.take_along_axis(ref64, idx, 1)
    b = np.take_along_axis(bnd, idx, 1)
    assert not np.any(np.isnan(sim)), f'{tag}: NaN similarity'
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.where(sim == r, 0.0, np.abs(sim - r))
        ratio = np.where(err == 0, 0.0, err / b)
    worst = float(ratio.max())
    if detail is not None:
        detail.update(sim=worst, w=0.0)
    q_bad = np.argwhere(~(err <= b))
    assert q_bad.size == 0, (f'{tag}: (b) similarity off its own index: query {q_bad[0][0]} rank {q_bad[0][1]} got '
                             f'{sim[tuple(q_bad[0])]!r} ref {r[tuple(q_bad[0])]!r} bound {b[tuple(q_bad[0])]:.3g}; max err/bound {worst:.3f}')
    ok = (sim[:, :-1] > sim[:, 1:]) | ((sim[:, :-1] == sim[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))
    assert np.all(ok), f'{tag}: (c) not in (value descending, index ascending) order at query {np.argwhere(~ok)[0][0]}'
    thresh = (r + b).min(1)
    out = ref64 - bnd > thresh[:, None]
    np.put_along_axis(out, idx, False, 1)
    assert not out.any(), (f'{tag}: (d) {int(out.sum())} unpicked elements are certainly better than a member '
                           f'(first: query {np.argwhere(out)[0][0]}, element {np.argwhere(out)[0][1]})')
    vals_ref, idx_ref = topk_ref(ref64, k)
    if exact:
        bad = np.argwhere(idx != idx_ref)
        assert bad.size == 0, (f'{tag}: exact regime: indices differ from topk_ref at query {bad[0][0]} rank {bad[0][1]}: '
                               f'got {idx[bad[0][0]].tolist()} want {idx_ref[bad[0][0]].tolist()}') if bad.size else ''
    if got_w is not None:
        w = np.asarray(got_w, np.float64)
        assert np.all(np.abs(vals_ref) < 80) and np.all(np.exp(vals_ref).sum(1) > 1e-30), f'{tag}: inputs outside the weights check'
        w64 = weights_ref(sim)
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = np.where(w == w64, 0.0, np.abs(w - w64) / w64)
        wr = float(rel.max() / weights_rel_bound(k))
        assert wr <= 1.0, f'{tag}: (e) weights off exp / sum of the returned similarities: err/bound {wr:.3f}'
        worst = max(worst, wr)
        if detail is not None:
            detail['w'] = wr
    same = float((srt == np.sort(idx_ref, 1)).all(1).mean())
    return worst, same


# ---------------------------------------------------------------------------------------------------------
# named shapes: (segment sizes, HW, top_k) -> the route and grid the host arithmetic must give (xmem_affinity_plan_info).
# hint: None | 'k' (a hint of top_k entries) | an int (its top_k) | 'nseg' (a hint whose n_seg differs: ignored);
# f16: the value of XMEM_AFFINITY_FILTER16.  want: route, tiles, splits, tiles_per_split, chunk, bound_stride.
# ---------------------------------------------------------------------------------------------------------
def shape(segs, hw, k, route, tiles, hint=None, f16=1, **grid):
    return dict(segs=tuple(segs), hw=hw, k=k, hint=hint, f16=f16, route=route, tiles=tiles, grid=grid)


SHAPES = {
    # small path: tiles < 256
    'n=k': shape((30,), 65, 30, SMALL, 1), 'n=k+1': shape((31,), 65, 30, SMALL, 1), 'n=32': shape((32,), 65, 30, SMALL, 1),
    'n=33': shape((33,), 65, 30, SMALL, 2), 'n=97': shape((97,), 65, 30, SMALL, 4), 'n=225': shape((225,), 65, 30, SMALL, 8),
    'n=512': shape((512,), 65, 30, SMALL, 16), 'n=1000': shape((1000,), 65, 30, SMALL, 32),
    'n=8160': shape((8160,), 65, 30, SMALL, 255),
    'n=1000 HW=1': shape((1000,), 1, 30, SMALL, 32), 'n=1000 HW=63': shape((1000,), 63, 30, SMALL, 32),
    'n=1000 HW=64': shape((1000,), 64, 30, SMALL, 32), 'n=1000 HW=129': shape((1000,), 129, 30, SMALL, 32),
    '(31,33,1,n-65) n=1000': shape((31, 33, 1, 935), 65, 30, SMALL, 1 + 2 + 1 + 30),
    '(8,7,8,7)': shape((8, 7, 8, 7), 65, 30, SMALL, 4),
    # large path, un-hinted
    'n=8161': shape((8161,), 129, 30, LARGE_SAMPLED, 256, splits=4, tiles_per_split=64, chunk=0, bound_stride=4),
    'n=8192': shape((8192,), 129, 30, LARGE_SAMPLED, 256, splits=4, tiles_per_split=64, chunk=0, bound_stride=4),
    '(1,1,1,8100)': shape((1, 1, 1, 8100), 129, 30, LARGE_SAMPLED, 257, splits=4, tiles_per_split=65, chunk=0, bound_stride=4),
    '20000 ragged': shape((6001, 0, 13999), 300, 30, LARGE_SAMPLED, 188 + 438, chunk=0, bound_stride=4),
    'n=131072 HW=100': shape((131072,), 100, 30, LARGE_SAMPLED, 4096, splits=32, tiles_per_split=128, chunk=8, bound_stride=4),
    'n=262144 HW=40': shape((262144,), 40, 30, LARGE_SAMPLED, 8192, splits=32, tiles_per_split=256, chunk=8, bound_stride=8),
    # hinted
    'n=8161 hinted': shape((8161,), 129, 30, LARGE_HINTED_FILTER16, 256, hint='k', list_cap=2048, list_stride=8192),
    'n=8161 hinted fp32': shape((8161,), 129, 30, LARGE_HINTED_FP32, 256, hint='k', f16=0, splits=4, tiles_per_split=64, chunk=0),
    '(1,1,1,8100) hinted': shape((1, 1, 1, 8100), 129, 30, LARGE_HINTED_FILTER16, 257, hint='k', list_cap=2048, list_stride=8192),
    'n=8192 hint k=64': shape((8192,), 129, 30, LARGE_HINTED_FILTER16, 256, hint=64),
    'n=8192 hint k<top_k': shape((8192,), 129, 30, LARGE_SAMPLED, 256, hint=8, bound_stride=4),
    'n=8192 hint n_seg mismatch': shape((8192,), 129, 30, LARGE_SAMPLED, 256, hint='nseg', bound_stride=4),
    'n=8160 hinted': shape((8160,), 129, 30, SMALL, 255, hint='k'),
    '20000 ragged hinted': shape((6001, 0, 13999), 260, 30, LARGE_HINTED_FILTER16, 188 + 438, hint='k', list_cap=2048, list_stride=8192),
}


def plan_info(segs, hw, k, hint_k=None, hint_n_seg=None):
    """xmem_affinity_plan_info for segment sizes `segs` (host only).  hint_k: top_k of a hint (None: no hint) whose idx pointer is a
    non-NULL address that must never be dereferenced; hint_n_seg: its n_seg (default: len(segs)).  Returns (status, dict of fields)."""
    import ctypes as C
    from xmem2_amd import _lib
    lib = _lib.load()
    Plan, Hint = _lib._STRUCTS['xmem_affinity_plan'], _lib.AffinityHint
    arr = (C.c_int * max(len(segs), 1))(*segs)
    hp = None
    if hint_k is not None:
        h = Hint()
        h.idx = 0x10
        h.top_k = hint_k
        h.n_seg = len(segs) if hint_n_seg is None else hint_n_seg
        for i, s in enumerate(segs[:4]):
            h.seg_n[i] = s
        h.grid_w = 0
        hp = C.byref(h)
    out = Plan()
    rc = lib.xmem_affinity_plan_info(C.cast(arr, C.c_void_p), len(segs), hw, k, hp, C.byref(out))
    return rc, {f: getattr(out, f) for f, _ in Plan._fields_}


def shape_plan(sh):
    """plan_info of a SHAPES entry (the caller sets XMEM_AFFINITY_FILTER16 to sh['f16'] first)."""
    hk, hn = None, None
    if sh['hint'] == 'k':
        hk = sh['k']
    elif sh['hint'] == 'nseg':
        hk, hn = sh['k'], len(sh['segs']) + 1
    elif sh['hint'] is not None:
        hk = int(sh['hint'])
    return plan_info(list(sh['segs']), sh['hw'], sh['k'], hk, hn)
