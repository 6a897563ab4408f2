"""Host tests of the eviction with several object groups: the restated rule (tests/store_group_refs.py) against the oracle's store where
the oracle has one, the pairing it must keep, the preconditions of the GPU comparisons against the patched oracle, and the C entry
point's declaration and argument refusals (no device needed)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import store_group_refs as G
from conftest import ROOT, base_config
from oracle import cpu_ref as R
from test_oracle_goldens import _feed, _query

T = torch.from_numpy


def g_(seed):
    return torch.Generator().manual_seed(seed)


def test_evict_ref_equals_refstore_with_one_group_and_ties_at_the_threshold():
    n, ck, cv, max_size = 300, 4, 3, 200
    gen = g_(3)
    st = R.RefStore(count_usage=True)
    key = torch.zeros(1, ck, n)
    key[0, 0] = torch.arange(n).float()                             # every element carries its index
    st.add(key, torch.randn(2, cv, n, generator=gen), torch.rand(1, 1, n, generator=gen) + 1, torch.rand(1, ck, n, generator=gen), [1, 2])
    st.use_count = torch.randint(0, 5, (n,), generator=gen).float().view(1, 1, n)     # five usage levels: ties everywhere, zeros included
    st.life_count = torch.full((1, 1, n), 4.0)
    usage = st.get_usage().flatten()
    thr = G.threshold_of(usage, max_size)
    assert int((usage == thr).sum()) > 1 and int((usage < thr).sum()) < n - max_size, 'no tie at the threshold'
    want = G.evict_ref(G.refstore_tensors(st), usage, max_size)
    st.remove_obsolete_features(max_size)                           # the oracle's own: one group
    assert st.k[0, 0].long().tolist() == want['keep'].tolist() and bool((usage[want['keep']] > thr).all())
    assert want['keep'].numel() == n - int((usage <= thr).sum()) < max_size             # every tie is dropped
    for name, got in G.refstore_tensors(st).items():
        if name == 'value':
            assert len(got) == 1 and torch.equal(got[0], want['value'][0])
        else:
            assert torch.equal(got, want[name]), name


@pytest.mark.parametrize('sizes', [(40, 25, 7), (40, 40, 1), (40, 0, 13)])
def test_evict_ref_keeps_every_key_value_pairing(sizes):
    """Every value column carries the index of the key it belongs to: after the eviction group g's columns are the kept keys at or
    behind its offset, in order - also when a group keeps all, one or none of its columns."""
    N, max_size = sizes[0], 22
    gen = g_(sum(sizes))
    key = torch.arange(N).float().view(1, 1, N)
    usage = torch.rand(N, generator=gen)
    usage[N - 7:] += 2.0                                             # the last group's elements all survive
    usage[:10] = 0.0                                                 # ... and ties at the bottom
    vals = [torch.arange(N - n, N).float().view(1, 1, n).repeat(i + 1, 1, 1) for i, n in enumerate(sizes)]
    out = G.evict_ref({'key': key, 'use': usage.view(1, 1, N), 'value': vals}, usage, max_size)
    kept = out['key'].flatten()
    assert torch.equal(out['use'].flatten(), usage[out['keep']]) and out['shrinkage'] is None
    for i, n in enumerate(sizes):
        want = kept[kept >= N - n]
        assert out['value'][i].shape[0] == i + 1
        for o in range(i + 1):
            assert torch.equal(out['value'][i][o, 0], want)
    assert out['value'][2].shape[-1] >= min(sizes[2], 7) and (sizes[1] != 0 or out['value'][1].shape[-1] == 0)


def test_the_store_level_cases_contain_what_they_are_named_for():
    """The GPU store tests run these cases: a group that keeps all of its rows and one that keeps none, first survivors exactly at a
    group's offset and one element to either side of it, several ties at the threshold, k = 1, a single-row group kept and dropped."""
    def first_from(name, off):
        groups, zeros, ones = G.STORE_CASES[name]
        kept = G.others(groups[0][1], list(zeros) + list(ones))
        return min(i for i in kept if i >= off) - off, max([i for i in kept if i < off], default=None)
    assert first_from('last_group_keeps_all_survivors_begin_at_its_offset', 96) == (0, 20)
    assert first_from('survivors_begin_one_before_and_one_behind_an_offset', 96) == (1, 95)
    assert first_from('survivors_begin_one_before_and_one_behind_an_offset', 48) == (47, 47)
    assert first_from('survivors_begin_at_and_one_behind_the_middle_offset', 48) == (0, None)
    assert first_from('survivors_begin_one_behind_the_middle_offset', 48) == (1, 47)
    for name, (groups, zeros, ones) in G.STORE_CASES.items():
        N = groups[0][1]
        tens, use, life, max_size, kept = G.store_case(name)
        assert [n for _, n in groups] in ([144, 96, 48], [4099, 2050, 1]) and [o for o, _ in groups] == [1, 3, 2]
        out = G.evict_ref(tens, use / life, max_size)
        assert out['keep'].tolist() == kept and N - max_size == len(zeros) + 1
        sizes = [v.shape[-1] for v in out['value']]
        assert sizes == [sum(1 for i in kept if i >= N - n) for _, n in groups]
        if name == 'last_group_keeps_all_survivors_begin_at_its_offset':
            assert sizes[2] == 48
        if name in ('last_group_keeps_none', 'large_single_row_group_dropped'):
            assert sizes[2] == 0 and sizes[1] > 0
        if name == 'several_ties_at_the_threshold':
            assert len(ones) == 5 and int((use / life == 1.0).sum()) == 5
        if name.endswith('k_is_1') or name == 'k_is_1_first_element':
            assert N - max_size == 1 and len(kept) == N - 1
        if name == 'large_half_kept_with_the_single_row_group':
            assert sizes[2] == 1 and 1500 < len(kept) < 2600


def test_the_patch_lifts_the_oracles_refusal_and_is_taken_back():
    orig = R.RefStore.remove_obsolete_features
    st = R.RefStore(count_usage=True)
    gen = g_(5)
    st.add(torch.randn(1, 4, 30, generator=gen), torch.randn(1, 3, 30, generator=gen), torch.ones(1, 1, 30), torch.ones(1, 4, 30), [1])
    st.add(torch.randn(1, 4, 20, generator=gen), torch.randn(2, 3, 20, generator=gen), torch.ones(1, 1, 20), torch.ones(1, 4, 20), [1, 2])
    st.use_count = torch.rand(1, 1, 50, generator=gen)
    st.life_count = torch.ones(1, 1, 50)
    before = G.refstore_tensors(st)
    usage = st.get_usage().clone()
    with G.GroupedEviction() as ge:
        st.remove_obsolete_features(35)
    assert R.RefStore.remove_obsolete_features is orig
    want = G.evict_ref(before, usage, 35)
    assert st.size == 35 and [st.get_v_size(0), st.get_v_size(1)] == [35, int((want['keep'] >= 30).sum())]
    assert torch.equal(st.v[1], want['value'][1]) and torch.equal(st.k, want['key'])
    assert len(ge.events) == 1 and ge.events[0]['num_groups'] == 2 and ge.events[0]['at_threshold'] == 1
    with pytest.raises(NotImplementedError):
        st.remove_obsolete_features(20)


def _run_memory_script():
    mm = R.RefMemory(base_config(**G.EVICT_OVER))
    for step, op in enumerate(G.MEM_SCRIPT):
        if op[0] in ('perm', 'temp'):
            key, shr, val, sel = _feed(step, len(op[1]), G.MEM_HW)
            mm.add_memory(key, shr, val, list(op[1]), selection=sel, permanent=(op[0] == 'perm'), ti=(op[2] if len(op) > 2 else None))
        else:
            out = mm.match_memory(*_query(step, G.MEM_HW))
            assert bool(torch.isfinite(out).all())
    return mm


@pytest.mark.parametrize('pinned', [False, True], ids=['torch_tie_order', 'lowest_index_tie_order'])
def test_the_memory_script_evicts_two_groups_without_emptying_one_or_a_usage_near_the_threshold(pinned):
    """With the oracle as it is, and with the tie order of its prototype selection pinned as the GPU comparison pins it."""
    orig = R.RefMemory.consolidation
    with G.GroupedEviction() as ge:
        if pinned:
            with G.PinnedPrototypeTies() as pin:
                mm = _run_memory_script()
            assert len(pin.ties) == 8 and pin.ties[:2] == [1, 1] and min(pin.ties[2:]) >= 72        # why the pin is there
        else:
            mm = _run_memory_script()
    assert R.RefMemory.consolidation is orig and R.torch is torch
    print([(e['before'], e['after'], f'{e["gap"]:.1e}', e['at_threshold']) for e in ge.events])
    G.check_events(ge.events)
    assert len(ge.events) == 5 and mm.long_mem.num_groups == 2
    if not pinned:
        assert (ge.events[0]['before'], ge.events[0]['after']) == ([96, 81], [68, 53])
        assert (ge.events[-1]['before'], ge.events[-1]['after']) == ([100, 87], [68, 55])


def test_the_end_to_end_stream_evicts_two_groups_twice_after_the_new_object(ref_net):
    from xmem2_amd.synth import synthetic_frames, synthetic_masks
    t = G.E2E_FRAMES
    frames, masks = T(synthetic_frames(t, *G.E2E_HW)), T(synthetic_masks(t, 3, *G.E2E_HW))
    at = []
    with G.GroupedEviction() as ge, G.PinnedPrototypeTies() as pin:      # (the pin only counts here: this stream has no tie to order)
        ref = R.RefCore(ref_net, G.e2e_config())
        for ti in range(t):
            labels, mk, vl = G.e2e_annotation(ti, masks)
            if labels is not None:
                ref.set_all_labels(labels)
            n0 = len(ge.events)
            ref.step(frames[ti], mk.clone() if mk is not None else None, vl, end=(ti == t - 1))
            at += [ti] * (len(ge.events) - n0)
    print(at, ge.events)
    G.check_events(ge.events)
    assert len(at) >= 2 and min(at) > G.E2E_NEW_OBJECT_AT and all(e['num_groups'] == 2 for e in ge.events)
    assert len(pin.ties) >= 4 and max(pin.ties) == 1, f'prototype selections with tied candidates: {pin.ties}'   # the GPU test runs the oracle as it is


def test_store_compact_is_declared_listed_and_exported_and_the_abi_version_stays_5():
    from xmem2_amd import _lib, build, ops
    assert 5 == _lib.ABI_VERSION and _lib.COMPACT_MAX_ARENAS >= 8 and 'store_compact.hip' in build.SOURCES
    src = open(os.path.join(ROOT, 'xmem2_amd', 'kv_memory_store.py')).read()
    assert 'does not support' not in src and 'ops.store_compact' in src
    lib = _lib.load()
    assert hasattr(lib, 'xmem_store_compact') and lib.xmem_version() == 5
    assert callable(ops.store_compact)

    # argument refusals: all answered on the host, before any launch (the addresses below are never touched)
    BAD_ARG, A = -1, _lib.CompactArena
    keep, m, kept = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    call = lambda arr, n, keep=keep, m=m, cap=100, kept=kept: lib.xmem_store_compact(arr, n, keep, m, cap, kept, None)
    ok = lambda **kw: A(**dict(dict(src=1 << 24, dst=2 << 24, width=64, n=100, off=0), **kw))
    assert call(None, 0) == 0                                                              # nothing to do
    assert call(None, -1) == BAD_ARG and call(None, 1) == BAD_ARG
    one = lambda a: (A * 1)(a)
    assert call(one(ok()), 1, cap=-1) == BAD_ARG
    assert call(one(ok()), 1, keep=None) == BAD_ARG and call(one(ok()), 1, m=None) == BAD_ARG and call(one(ok()), 1, kept=None) == BAD_ARG
    assert call(one(ok(src=None)), 1) == BAD_ARG and call(one(ok(dst=None)), 1) == BAD_ARG
    assert call(one(ok(n=-1, off=101)), 1) == BAD_ARG and call(one(ok(n=101, off=-1)), 1) == BAD_ARG
    assert call(one(ok(width=0)), 1) == BAD_ARG
    assert call(one(ok(n=40, off=50)), 1) == BAD_ARG                                       # off is not N - n
    assert call(one(ok(src=(1 << 24) + 2)), 1) == BAD_ARG                                  # not a float address
    assert call(one(ok(dst=1 << 24)), 1) == BAD_ARG                                        # in place
    assert call(one(ok(dst=(1 << 24) + 100 * 64 * 4 - 4)), 1) == BAD_ARG                   # the last float of the source
    assert call(one(ok(dst=(1 << 24) - 100 * 64 * 4 + 4)), 1) == BAD_ARG
    two = (A * 2)(ok(), ok(src=3 << 24, dst=1 << 24, width=1))                             # a destination on ANOTHER arena's source
    assert call(two, 2) == BAD_ARG
    two = (A * 2)(ok(), ok(src=3 << 24, dst=(2 << 24) + 64, width=1))                      # two destinations overlap
    assert call(two, 2) == BAD_ARG
    with pytest.raises(RuntimeError):
        ops.store_compact([(torch.zeros(4, 64), torch.zeros(4, 64))], torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
