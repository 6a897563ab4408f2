"""Least-used eviction of a store with several object groups, restated by plain indexing (torch on the CPU): what
KeyValueMemoryStore.remove_obsolete_features and csrc/store_compact.hip are tested against, and the same rule patched onto the CPU
oracle's store, which - like the reference - refuses more than one group.

The rule.  N elements, `keep` the ascending indices with usage > the (N - max_size)-th smallest usage (strict: every tie at the
threshold is dropped).  Every key-side tensor keeps its columns `keep`.  Group g with n_g columns holds the LAST n_g elements (offset
N - n_g) and keeps its columns keep[j] - (N - n_g) for the j with keep[j] >= N - n_g, in that order, for each of its objects.
"""
import numpy as np
import torch

from conftest import base_config
from oracle import cpu_ref as R

KEY_SIDE = ('key', 'shrinkage', 'selection', 'use', 'life')

# the scripted memory sequence of the tests (fed by test_oracle_goldens._feed / _query): a second object group from step 4 on, and a
# long-term store so small that it is evicted again and again with both groups in it
EVICT_OVER = dict(max_mid_term_frames=3, min_mid_term_frames=1, num_prototypes=32, max_long_term_elements=100)
MEM_HW = (6, 8)
MEM_SCRIPT = [('perm', [1], 0), ('match',), ('temp', [1]), ('match',), ('perm', [1, 2], 5), ('match',)] + 16 * [('temp', [1, 2]), ('match',)]

# the end-to-end stream: test_gpu_e2e's objects-appearing-later clip (three objects, the third annotated at frame 6) run long enough
# for the long-term store to be evicted twice while it holds both groups
E2E_HW = (128, 192)
E2E_FRAMES = 22          # the long-term store holds 96 and 100 elements at frames 16 and 20: evicted at both, object 3's group in it since 8
E2E_NEW_OBJECT_AT = 6


def e2e_config():
    return base_config(mem_every=2, **EVICT_OVER)


def e2e_annotation(ti, masks):
    """(labels | None, mask | None, valid labels | None) of frame ti: objects 1, 2 at frame 0, object 3 joins at frame 6 and is the only
    valid label there (the others keep their prediction)."""
    if ti == 0:
        return [1, 2], masks[ti, :2], [1, 2]
    if ti == E2E_NEW_OBJECT_AT:
        return [1, 2, 3], masks[ti], [3]
    return None, None, None


def threshold_of(usage, max_size):
    """The (N - max_size)-th smallest usage."""
    usage = usage.flatten()
    k = usage.numel() - max_size
    assert 1 <= k <= usage.numel()
    return torch.sort(usage).values[k - 1]


def evict_ref(store_tensors, usage, max_size):
    """store_tensors: reference-shaped tensors {'key' [1,C,N], 'shrinkage' [1,1,N] | None, 'selection' [1,C,N] | None, 'use' / 'life'
    [1,1,N] | None, 'value': list of [n_obj, Cv, n_g]}; usage [N] (any shape).  Returns the same structure after the eviction, plus
    'keep' (int64 [m])."""
    usage = usage.flatten()
    N = usage.numel()
    keep = torch.nonzero(usage > threshold_of(usage, max_size)).flatten()
    out = {'keep': keep}
    for name in KEY_SIDE:
        t = store_tensors.get(name)
        if t is not None:
            assert t.shape[-1] == N, f'{name}: {tuple(t.shape)} in a store of {N}'
        out[name] = t[..., keep] if t is not None else None
    out['value'] = []
    for v in store_tensors['value']:
        off = N - v.shape[-1]
        assert off >= 0
        out['value'].append(v[..., keep[keep >= off] - off])
    return out


def refstore_tensors(st):
    return {'key': st.k, 'shrinkage': st.s, 'selection': st.e, 'use': st.use_count, 'life': st.life_count, 'value': list(st.v)}


def grouped_remove_obsolete_features(self, max_size):
    """RefStore.remove_obsolete_features without the refusal of several groups: the rule above."""
    out = evict_ref(refstore_tensors(self), self.get_usage(), max_size)
    self.k, self.s, self.e = out['key'], out['shrinkage'], out['selection']
    self.use_count, self.life_count = out['use'], out['life']
    self.v = out['value']


class GroupedEviction:
    """Patches the rule onto oracle.cpu_ref.RefStore for the duration of a `with` block and records, per eviction: the number of groups,
    the group sizes before and after, the relative distance from the threshold of the nearest usage on either side of it and the
    number of elements AT the threshold."""

    def __enter__(self):
        self.events, self._orig = [], R.RefStore.remove_obsolete_features
        events = self.events

        def evict(store, max_size):
            usage = store.get_usage().flatten().double()
            thr = threshold_of(usage, max_size)
            others = (usage[usage != thr] - thr).abs()
            gap = float(others.min() / thr.abs().clamp_min(1e-300)) if others.numel() else float('inf')
            before = [store.get_v_size(g) for g in range(store.num_groups)]
            grouped_remove_obsolete_features(store, max_size)
            events.append(dict(num_groups=store.num_groups, before=before, after=[store.get_v_size(g) for g in range(store.num_groups)],
                               size=(usage.numel(), store.size), gap=gap, at_threshold=int((usage == thr).sum())))
        R.RefStore.remove_obsolete_features = evict
        return self

    def __exit__(self, *exc):
        R.RefStore.remove_obsolete_features = self._orig


class _LowestIndexTopk:
    """`torch` as oracle.cpu_ref sees it during a consolidation: topk with exact ties ranked lowest index first."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def topk(input, k, dim=-1, largest=True, sorted=True):
        assert largest and sorted
        order = torch.sort(input, dim=dim, descending=True, stable=True)
        values, indices = order.values.narrow(dim, 0, k), order.indices.narrow(dim, 0, k)
        assert torch.equal(values, torch.topk(input, k=k, dim=dim).values)     # the same selection up to the order among EQUAL values
        return values, indices


class PinnedPrototypeTies:
    """torch.topk leaves the order among equal values open, and the oracle's prototype selection (RefMemory.consolidation: the
    num_prototypes most used candidates) meets such ties: on the scripted sequence above every consolidation from the third on ranks
    72 to 83 of its 96 candidates at usage exactly 0 and fills 8 to 19 of its 32 prototypes from them.  xmem_topk_1d ranks equal values
    lowest index first; torch's CPU kernel does not, so the two sides would consolidate different - equally valid - elements.  Inside a
    `with` block the oracle's selection ranks equal values lowest index first too.  `ties` records, per consolidation, how many
    candidates tie with the last prototype."""

    def __enter__(self):
        self.ties, self._orig = [], R.RefMemory.consolidation
        ties, orig = self.ties, self._orig

        def consolidation(mem, cand_key, cand_shrinkage, cand_selection, usage, cand_value):
            u = usage.flatten()
            ties.append(int((u == torch.sort(u, descending=True).values[mem.num_prototypes - 1]).sum()))
            R.torch = _LowestIndexTopk()
            try:
                return orig(mem, cand_key, cand_shrinkage, cand_selection, usage, cand_value)
            finally:
                R.torch = torch
        R.RefMemory.consolidation = consolidation
        return self

    def __exit__(self, *exc):
        R.RefMemory.consolidation = self._orig


def check_events(events, min_two_group_evictions=2):
    """The precondition of a comparison against the patched oracle: enough evictions with two groups, no group emptied (the oracle's own
    slice [:, -0:] would read an empty group as the whole store), and a threshold no usage comes nearer to than 1e-3 relative (the
    device's usage differs from the oracle's by rounding: a nearer one could legitimately be evicted on one side only)."""
    two = [e for e in events if e['num_groups'] >= 2]
    assert len(two) >= min_two_group_evictions, f'{len(two)} evictions with two groups: {events}'
    for e in events:
        assert min(e['after']) > 0, f'an eviction emptied a group: {e}'
        assert e['gap'] >= 1e-3, f'a usage within {e["gap"]:.2e} (relative) of the threshold: {e}'


def usage_for(N, zeros, ones, seed):
    """(use, life, max_size) with an exactly representable ratio use / life: 0 on `zeros`, 1 on `ones` - the threshold for
    max_size = N - len(zeros) - 1, where all of `ones` tie and are dropped - and distinct values from 2 up elsewhere."""
    assert not set(zeros) & set(ones) and len(ones) >= 1
    use = (torch.randperm(N, generator=torch.Generator().manual_seed(seed)).float() + 2.0) * 4.0
    use[torch.tensor(sorted(zeros), dtype=torch.long)] = 0.0
    use[torch.tensor(sorted(ones), dtype=torch.long)] = 4.0
    return use, torch.full((N,), 4.0), N - len(zeros) - 1


def others(N, kept):
    return sorted(set(range(N)) - set(kept))


# store-level cases: (groups [(objects, elements), ...], elements dropped with usage 0, elements dropped AT the threshold)
G144 = [(1, 144), (3, 96), (2, 48)]                      # offsets 0, 48, 96
G4099 = [(1, 4099), (3, 2050), (2, 1)]                   # offsets 0, 2049, 4098: the index crosses workgroup chunks, one group is one row
_bit = lambda i, mul, sh: (i * mul >> sh) & 1
STORE_CASES = {
    'last_group_keeps_all_survivors_begin_at_its_offset': (G144, others(144, [5, 20, 95] + list(range(96, 144))), [95]),
    'survivors_begin_one_before_and_one_behind_an_offset': (G144, others(144, [0, 3, 47, 95] + list(range(97, 144))), [0]),
    'survivors_begin_at_and_one_behind_the_middle_offset': (G144, others(144, [0, 1, 2, 48, 49, 96, 143]), [0, 1, 2]),
    'survivors_begin_one_behind_the_middle_offset': (G144, others(144, [0, 1, 2, 3, 47, 49, 50, 97, 120]), [0, 1, 2, 3]),
    'last_group_keeps_none': (G144, list(range(0, 10)) + list(range(60, 143)), [143]),
    'several_ties_at_the_threshold': (G144, [7, 100], [1, 50, 96, 97, 143]),
    'k_is_1': (G144, [], [96]),
    'k_is_1_first_element': (G144, [], [0]),
    'large_half_kept_with_the_single_row_group': (G4099, [i for i in range(4098) if _bit(i, 2654435761, 7) and i not in (2049, 2050)], [2049, 2050]),
    'large_single_row_group_dropped': (G4099, [i for i in range(4098) if _bit(i, 40503, 5)], [4098]),
    'large_k_is_1': (G4099, [], [2048]),
}


def store_case(name, seed=None):
    """(tensors with 'use' / 'life', use, life, max_size, kept elements) of a store-level case."""
    groups, zeros, ones = STORE_CASES[name]
    N = groups[0][1]
    tens = random_store_tensors(len(name) if seed is None else seed, N, groups)
    use, life, max_size = usage_for(N, zeros, ones, N + len(zeros))
    tens.update(use=use.view(1, 1, N), life=life.view(1, 1, N))
    return tens, use, life, max_size, others(N, list(zeros) + list(ones))


def random_store_tensors(seed, N, groups, ck=64, cv=512):
    """Hash-random reference-shaped tensors of a store of N elements; groups: [(n_obj, n_g), ...] with n_0 = N."""
    from xmem2_amd.synth import hash_normal, hash_uniform
    T = torch.from_numpy
    rnd = lambda shape, s: T(hash_normal(int(np.prod(shape)), seed * 100 + s).reshape(shape).astype(np.float32)) if np.prod(shape) else torch.zeros(shape)
    assert groups[0][1] == N
    return {'key': rnd((1, ck, N), 1), 'shrinkage': T(hash_uniform(N, seed * 100 + 2, 1.0, 4.0).reshape(1, 1, N).astype(np.float32)),
            'selection': T(hash_uniform(ck * N, seed * 100 + 3, 0.05, 0.95).reshape(1, ck, N).astype(np.float32)),
            'value': [rnd((n_obj, cv, n_g), 10 + i) for i, (n_obj, n_g) in enumerate(groups)]}
