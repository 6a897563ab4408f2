"""tests/affinity_refs.py on the CPU: the float64 reference against the oracle, the exactness premise of the `exact` regime, the
checker against hand-corrupted outputs, the adversarial orderings, and the route table of every named shape (host-only
xmem_affinity_plan_info).  No GPU."""
import numpy as np
import pytest
import torch

import affinity_refs as A
import memory_kernel_refs as M
from oracle import cpu_ref as R


def test_reference_agrees_with_the_oracle_on_gapped_inputs():
    """get_similarity + do_softmax(top_k) in fp32 against similarity_ref + topk_ref + weights_ref, on inputs whose neighbouring
    similarities are further apart than fp32 can confuse (so torch.topk has one answer)."""
    n, hw, k = 120, 7, 30
    d = A.make_inputs('dense', n, hw, 11)
    sim64 = A.similarity_ref(d['key'], d['shr'], d['qk'], d['qe'])
    vals, idx = A.topk_ref(sim64, k)
    srt = -np.sort(-sim64, 1)[:, :k + 1]
    assert np.all(srt[:, :-1] - srt[:, 1:] > 1e-4), 'inputs not gapped: pick another seed'
    sim32 = R.get_similarity(d['key'].t().unsqueeze(0), d['shr'].view(1, 1, -1), d['qk'].t().unsqueeze(0), d['qe'].t().unsqueeze(0))
    assert np.allclose(sim32[0].t().numpy(), sim64, rtol=0, atol=float(M.similarity_dense_bound(d['key'], d['shr'], d['qk'], d['qe']).max()))
    aff = R.do_softmax(sim32.clone(), top_k=k)[0].t().double().numpy()                    # [hw, n]
    mine = np.zeros_like(sim64)
    np.put_along_axis(mine, idx, A.weights_ref(vals), 1)
    assert np.array_equal(mine > 0, aff > 0), 'index sets differ from torch.topk'
    assert np.allclose(mine, aff, rtol=1e-4, atol=1e-9)
    w_sparse, i_sparse = R.topk_softmax_sparse(sim32, k)
    assert np.array_equal(i_sparse[0].t().numpy(), idx), 'order differs from torch.topk on gapped inputs'


def test_topk_ref_tie_rule():
    sim = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0, -np.inf, 2.0]])
    vals, idx = A.topk_ref(sim, 6)
    assert idx.tolist() == [[1, 2, 5, 7, 0, 3]] and vals.tolist() == [[3.0, 3.0, 3.0, 2.0, 1.0, 0.0]]
    assert A.topk_ref(sim, 8)[1].tolist() == [[1, 2, 5, 7, 0, 3, 4, 6]]
    assert A.topk_ref(np.zeros((2, 50)), 30)[1].tolist() == [list(range(30))] * 2


@pytest.mark.parametrize('signed_e', [False, True])
def test_exact_regime_is_exact(signed_e):
    """fp32 evaluation forwards, reversed, pairwise and in the expanded GEMM form all equal the float64 value; the fp16 filter
    operands survive the round trip."""
    n, hw = 300, 9
    d = A.make_inputs('exact', n, hw, 5, signed_e=signed_e)
    assert A.is_exact_regime(d, signed_e)
    ref = A.similarity_ref(d['key'], d['shr'], d['qk'], d['qe'])                          # [hw, n]
    x, ms, k, e = (d[t].numpy() for t in ('key', 'shr', 'qk', 'qe'))
    f = np.float32
    terms = np.concatenate([(x * x)[None, :, :] * (-e)[:, None, :], x[None, :, :] * (f(2) * (k * e))[:, None, :],
                            np.broadcast_to((-(e * (k * k)))[:, None, :], (hw, n, 64))], 2)   # [hw, n, 192] fp32
    assert terms.dtype == np.float32
    scale = (ms * f(0.125))[None, :]
    fwd = np.cumsum(terms, 2, dtype=np.float32)[:, :, -1] * scale
    rev = np.cumsum(terms[:, :, ::-1], 2, dtype=np.float32)[:, :, -1] * scale
    pair = terms.sum(2, dtype=np.float32) * scale
    op_mem = np.concatenate([x * x, x], 1)                                                # [n, 128]
    op_q = np.concatenate([-e, f(2) * (k * e)], 1)                                        # [hw, 128]
    gemm = ((op_q @ op_mem.T) - (e * (k * k)).sum(1, dtype=np.float32)[:, None]) * scale
    for name, got in dict(forwards=fwd, reversed=rev, pairwise=pair, expanded=gemm).items():
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), ref), name
    msr = (ms * f(0.125))[:, None]
    for row in (msr * (x * x), msr * x):
        assert np.array_equal(row.astype(np.float16).astype(np.float32), row)
    b = M.similarity_dense_bound(d['key'], d['shr'], d['qk'], d['qe'])
    assert b.shape == ref.shape and np.all(b >= 0)


def _good(regime, n=300, hw=5, k=8, seed=3, ordering=None):
    d = A.make_inputs(regime, n, hw, seed)
    if ordering:
        d = A.order_memory(d, ordering, k, seed=seed)
    ref = A.similarity_ref(d['key'], d['shr'], d['qk'], d['qe'])
    bound = M.similarity_dense_bound(d['key'], d['shr'], d['qk'], d['qe'])
    vals, idx = A.topk_ref(ref, k)
    sim = vals.astype(np.float32)
    w = A.weights_ref(sim.astype(np.float64)).astype(np.float32)
    return ref, bound, idx.astype(np.int32), sim, w, k


def test_checker_accepts_the_reference():
    for regime in ('exact', 'dense'):
        ref, bound, idx, sim, w, k = _good(regime)
        worst, same = A.check_topk(idx, sim, w, ref, bound, k, exact=regime == 'exact')
        assert worst <= 1.0 and same == 1.0


def _swap(idx, sim, w, ref, bound, k):
    idx[2, [1, 4]] = idx[2, [4, 1]]


def _next_best(idx, sim, w, ref, bound, k):
    order = np.argsort(-ref[1], kind='stable')
    assert ref[1, order[k - 1]] - ref[1, order[k]] > 4 * bound[1].max()               # the (k+1)-th is clearly worse
    idx[1, k - 1] = order[k]
    sim[1, k - 1] = ref[1, order[k]]
    w[1] = A.weights_ref(sim[1].astype(np.float64))


def _rotate_w(idx, sim, w, ref, bound, k):
    w[:] = np.roll(w, 1, 1)


def _duplicate(idx, sim, w, ref, bound, k):
    idx[3, 5] = idx[3, 4]
    sim[3, 5] = sim[3, 4]


def _off_by_two_bounds(idx, sim, w, ref, bound, k):
    sim[0, 3] = np.float32(ref[0, idx[0, 3]] + 2 * bound[0, idx[0, 3]])
    w[0] = A.weights_ref(sim[0].astype(np.float64))


def _out_of_range(idx, sim, w, ref, bound, k):
    idx[4, 0] = ref.shape[1]


@pytest.mark.parametrize('corrupt', [_swap, _next_best, _rotate_w, _duplicate, _off_by_two_bounds, _out_of_range])
def test_checker_rejects_corrupted_outputs(corrupt):
    ref, bound, idx, sim, w, k = _good('dense')
    corrupt(idx, sim, w, ref, bound, k)
    with pytest.raises((AssertionError, IndexError)):
        A.check_topk(idx, sim, w, ref, bound, k)


def test_checker_rejects_a_tie_resolved_to_the_higher_index():
    ref, bound, idx, sim, w, k = _good('exact', ordering='tie_at_kth')
    tied = np.nonzero(ref[0] == ref[0, idx[0, k - 1]])[0]
    assert tied.size >= 100 and idx[0, k - 1] == tied[0]
    idx[0, k - 1] = tied[1]
    with pytest.raises(AssertionError, match='topk_ref'):
        A.check_topk(idx, sim, w, ref, bound, k, exact=True)
    ref, bound, idx, sim, w, k = _good('exact', ordering='tie_at_kth')                # two tied members in the wrong order: rule (c)
    idx[0, k - 1], idx[0, k - 2] = tied[0], tied[5]
    sim[0, k - 2] = sim[0, k - 1]
    with pytest.raises(AssertionError):
        A.check_topk(idx, sim, None, ref, bound, k)


@pytest.mark.parametrize('regime', ['exact', 'dense'])
def test_orderings_do_what_they_say(regime):
    n, hw, k = 1000, 65, 30
    base = A.make_inputs(regime, n, hw, 21)
    sim0 = lambda d: A.similarity_ref(d['key'], d['shr'], d['qk'][:1], d['qe'][:1])[0]
    a = sim0(A.order_memory(base, 'ascending', k))
    assert np.all(np.diff(a) >= 0)
    assert np.all(np.diff(sim0(A.order_memory(base, 'descending', k))) <= 0)
    pos = np.arange(960, 990)
    c = A.order_memory(base, 'clustered', k, positions=pos)
    assert sorted(A.topk_ref(sim0(c)[None], k)[1][0].tolist()) == pos.tolist() or regime == 'exact'      # exact: ties may sit elsewhere
    assert np.all(np.sort(sim0(c))[::-1][:k] == np.sort(sim0(c)[pos])[::-1])
    t = A.order_memory(base, 'all_tied', k)
    assert A.topk_ref(A.similarity_ref(t['key'], t['shr'], t['qk'], t['qe']), k)[1].tolist() == [list(range(k))] * hw
    s = sim0(A.order_memory(base, 'tie_at_kth', k))
    kth = np.sort(s)[::-1][k - 1]
    assert (s == kth).sum() >= 100 and (s > kth).sum() <= k - 1
    u = sim0(A.order_memory(base, 'unsampled', k))
    sampled = (np.arange(n) // 32) % 4 == 0
    assert u[sampled].max() <= u[~sampled].min()
    z = A.order_memory(base, 'zero_sim', k)
    zs = A.similarity_ref(z['key'], z['shr'], z['qk'], z['qe'])
    tol = 0.0 if regime == 'exact' else 1e-12            # dense: the float64 evaluation of the expanded form rounds
    assert np.all(zs[0] == 0) and all(abs(zs[q, 2 * k + 2 * (q - 1) + 1]) <= tol and zs[q].max() <= tol for q in range(1, hw))
    m = A.make_inputs(regime, n, hw, 21, signed_e=True)
    ms = A.similarity_ref(m['key'], m['shr'], m['qk'], m['qe'])
    assert (ms > 0).any() and (ms < 0).any()
    for name, d in dict(ascending=A.order_memory(base, 'ascending', k), zero=z, tie=A.order_memory(base, 'tie_at_kth', k)).items():
        assert regime != 'exact' or A.is_exact_regime(d), name
        assert torch.equal(d['qk'][0], d['qk'][min(hw, 64) - 1]) or name == 'zero'


@pytest.mark.parametrize('name', list(A.SHAPES))
def test_route_table(name, monkeypatch):
    """Every named shape of the GPU tests takes the route (and grid) written beside it.  The hint's idx is a bogus non-NULL address:
    plan_info must not dereference it."""
    sh = A.SHAPES[name]
    monkeypatch.setenv('XMEM_AFFINITY_FILTER16', str(sh['f16']))
    rc, got = A.shape_plan(sh)
    assert rc == 0
    want = dict(route=sh['route'], tiles=sh['tiles'], **sh['grid'])
    assert {f: got[f] for f in want} == want, f'{name}: {got}'
    if sh['route'] != A.LARGE_SAMPLED:
        assert got['bound_stride'] == 0 and got['bound_splits'] == 0
    if sh['route'] != A.LARGE_HINTED_FILTER16:
        assert got['list_cap'] == 0 and got['list_stride'] == 0
    assert got['splits'] >= 1 and got['splits'] * got['tiles_per_split'] >= got['tiles']


def test_plan_info_validates_like_the_call():
    OK, BAD_ARG, UNSUPPORTED, TOPK = 0, -1, -2, -5
    assert A.plan_info([100], 10, 30)[0] == OK
    assert A.plan_info([100], 10, 0)[0] == UNSUPPORTED and A.plan_info([100], 10, 65)[0] == UNSUPPORTED
    assert A.plan_info([100, -1], 10, 30)[0] == BAD_ARG and A.plan_info([20] * 5, 10, 30)[0] == BAD_ARG
    assert A.plan_info([100], 0, 30)[0] == BAD_ARG
    assert A.plan_info([15, 14], 10, 30)[0] == TOPK and A.plan_info([15, 0, 15], 10, 30)[0] == OK
    # the threshold is a tile count: 255 tiles small, 256 large, and padding tiles of short segments count
    assert A.plan_info([8160], 100, 30)[1]['route'] == A.SMALL and A.plan_info([8161], 100, 30)[1]['route'] == A.LARGE_SAMPLED
    assert A.plan_info([1, 1, 1, 8100], 100, 30)[1]['tiles'] == 257
