"""The float64 references of tests/memory_kernel_refs.py against what the project already trusts (oracle/cpu_ref.py,
torch), on the CPU.  The GPU tests (test_gpu_memory_kernels.py) then compare the kernels with these references."""
import numpy as np
import pytest
import torch

import memory_kernel_refs as M
from oracle import cpu_ref as R


def g_(seed):
    return torch.Generator().manual_seed(seed)


def _dense_case(seed, n=150, hw=23, ck=16, top_k=7):
    gen = g_(seed)
    mk = torch.randn(1, ck, n, generator=gen) * 0.9
    ms = torch.rand(1, 1, n, generator=gen) * 3 + 1
    qk = torch.randn(1, ck, hw, generator=gen) * 0.9
    qe = torch.rand(1, ck, hw, generator=gen) * 0.9 + 0.05
    sim = R.get_similarity(mk, ms, qk, qe)                         # [1, n, hw]
    w, idx = R.topk_softmax_sparse(sim, top_k)                     # [1, k, hw]
    return sim, w[0].t().contiguous(), idx[0].t().contiguous()


@pytest.mark.parametrize('largest', [True, False])
def test_topk_ref_equals_torch_topk_without_ties(largest):
    v = torch.randperm(1000, generator=g_(1)).float() * 0.37 - 90.0           # distinct values
    for k in (1, 128, 1000):
        rv, ri = torch.topk(v, k, largest=largest, sorted=True)
        vals, idx = M.topk_1d_ref(v, k, largest)
        assert idx.tolist() == ri.tolist()
        assert np.array_equal(vals, rv.numpy())


def test_topk_ref_tie_rule_and_range():
    v = np.array([1.0, 0.0, 1.0, -0.0, 0.0, 1.0, np.inf, -np.inf], np.float32)
    assert M.topk_1d_ref(v, 5, True)[1].tolist() == [6, 0, 2, 5, 1]
    assert M.topk_1d_ref(v, 5, False)[1].tolist() == [7, 1, 3, 4, 0]
    with pytest.raises(ValueError):
        M.topk_1d_ref(v, 9, True)


def test_usage_ref_equals_dense_usage():
    sim, w, idx = _dense_case(2)
    n = sim.shape[1]
    aff, usage = R.do_softmax(sim, top_k=7, return_usage=True)     # [1, n, hw], [1, n]
    S, hits = M.usage_ref(w, idx, 0, n)
    np.testing.assert_allclose(S, usage[0].double().numpy(), rtol=1e-5, atol=1e-7)
    assert np.array_equal(hits, (aff[0] > 0).sum(1).numpy())
    # a window of the index space is the same slice of the dense usage
    S2, hits2 = M.usage_ref(w, idx, 40, 61)
    assert np.array_equal(S2, S[40:101]) and np.array_equal(hits2, hits[40:101])


def test_eviction_ref_equals_refstore_with_ties_at_the_threshold():
    n, ck, cv, max_size = 300, 4, 3, 200
    gen = g_(3)
    st = R.RefStore(count_usage=True)
    key = torch.zeros(1, ck, n)
    key[0, 0] = torch.arange(n).float()                             # every element carries its index
    st.add(key, torch.randn(1, cv, n, generator=gen), torch.ones(1, 1, n), torch.ones(1, ck, n), [1])
    use = torch.randint(0, 5, (n,), generator=gen).float()          # five usage levels: ties everywhere, zeros included
    st.use_count = use.view(1, 1, n).clone()
    st.life_count = torch.full((1, 1, n), 4.0)
    usage = st.get_usage().flatten()
    k = n - max_size
    vals, _ = M.topk_1d_ref(usage, k, largest=False)
    assert int((usage == float(vals[-1])).sum()) > 1 and int((usage < float(vals[-1])).sum()) < k, 'no tie at the threshold'
    keep = M.select_greater_ref(usage, vals[-1])
    st.remove_obsolete_features(max_size)
    assert st.k[0, 0].long().tolist() == keep.tolist()
    assert np.all(np.diff(keep) > 0)


def _consolidation_inputs(seed, n, n2, ck=16, cv=8, n_obj=(2, 1)):
    gen = g_(seed)
    cand_key = torch.randn(1, ck, n, generator=gen) * 0.9
    cand_shr = torch.rand(1, 1, n, generator=gen) * 3 + 1
    cand_sel = torch.rand(1, ck, n, generator=gen) * 0.9 + 0.05
    usage = (torch.randperm(n, generator=gen).float() / n).view(1, 1, n)       # tie-free
    values = [torch.randn(n_obj[0], cv, n, generator=gen)]
    if n2 is not None:
        values.append(torch.randn(n_obj[1], cv, n2, generator=gen) if n2 > 0 else None)
    return cand_key, cand_shr, cand_sel, usage, values


@pytest.mark.parametrize('n2', [None, 130, 0], ids=['one_group', 'two_groups', 'second_group_absent'])
def test_consolidation_ref_equals_refmemory(n2):
    from conftest import base_config
    P = 16
    args = _consolidation_inputs(4, 200, n2)
    mem = R.RefMemory(base_config(num_prototypes=P))
    pk, pv, ps = mem.consolidation(*args)
    qk, qv, qs = M.consolidation_ref(*args, P)
    assert torch.equal(pk.double(), qk)
    assert len(pv) == len(qv)
    for a, b in zip(pv, qv):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape
            np.testing.assert_allclose(a.double().numpy(), b.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ps.double().numpy(), qs.numpy(), rtol=1e-4, atol=1e-5)
    if n2 == 130:
        assert 0 < qv[1].shape[-1] < P, 'the case must exercise the validity selection'


def test_consolidation_pieces_compose_to_the_whole():
    """softmax_suffix_ref / weighted_rows_ref / similarity_dense_ref are the row-major pieces of consolidation_ref."""
    P = 16
    cand_key, cand_shr, cand_sel, usage, values = _consolidation_inputs(5, 200, 130)
    qk, qv, qs, aux = M.consolidation_ref(cand_key, cand_shr, cand_sel, usage, values, P, return_aux=True)
    rows = lambda t: t[0].t().contiguous()
    sim = M.similarity_dense_ref(rows(cand_key), cand_shr.flatten(), rows(qk), rows(aux['proto_sel']))
    np.testing.assert_allclose(sim, aux['similarity'][0].t().numpy(), rtol=1e-12, atol=1e-12)
    for gi, cnt in enumerate((200, 130)):
        aff = M.softmax_suffix_ref(sim, cnt)
        assert float(np.abs(aff[:, :200 - cnt]).max(initial=0.0)) == 0.0
        valid = aux['validity'][gi].numpy()
        for o in range(values[gi].shape[0]):
            val, mag = M.weighted_rows_ref(aff, cnt, values[gi][o].t())
            np.testing.assert_allclose(val[valid], qv[gi][o].t().numpy(), rtol=1e-12, atol=1e-13)
            assert np.all(mag >= np.abs(val) - 1e-15)
    val, _ = M.weighted_rows_ref(M.softmax_suffix_ref(sim, 200), 200, cand_shr.flatten())
    np.testing.assert_allclose(val[:, 0], qs.flatten().numpy(), rtol=1e-12)


def test_readout_ref_equals_dense_matmul():
    sim, w, idx = _dense_case(6)
    n, hw = sim.shape[1], sim.shape[2]
    aff = R.do_softmax(sim, top_k=7)                                # [1, n, hw]
    mv = torch.randn(3, 12, n, generator=g_(7))                     # [n_obj, Cv, n]
    dense = (mv.double() @ aff[0].double()).permute(0, 2, 1).numpy()           # [n_obj, hw, Cv]
    cuts = [0, 0, 60, 60, n]                                        # [0, n1, 0, n2] segments
    vsegs = [[(mv[o, :, a:b].t().contiguous() if b > a else None) for a, b in zip(cuts[:-1], cuts[1:])] for o in range(3)]
    val, mag = M.readout_ref(vsegs, w, idx)
    np.testing.assert_allclose(val, dense, rtol=1e-6, atol=1e-7)
    assert val.shape == (3, hw, 12) and np.all(mag >= np.abs(val) - 1e-15)
