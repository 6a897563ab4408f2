"""stages.py (capture, replay, the least-recently-used cache) and hipnet.py's state-dict check, on the host: torch's graph objects are
replaced by fakes, so nothing here needs a device."""
import contextlib
import os
import re

import pytest
import torch

from xmem2_amd import hipnet, ops, stages
from xmem2_amd.stages import Stage, StageCache

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'xmem2_amd')


# ---- StageCache ---------------------------------------------------------------------------------------------------------
def _captured(tag):
    return Stage(object(), [], tag)


def test_lookup_refreshes_the_order():
    c = StageCache(3)
    for k in 'abc':
        c.put(k, _captured(k))
    assert c.lookup('a').outputs == 'a' and list(c) == ['b', 'c', 'a']
    assert c.lookup('missing') is None and list(c) == ['b', 'c', 'a']
    c.put('d', _captured('d'))
    assert list(c) == ['c', 'a', 'd']                      # 'b', not the refreshed 'a', was the oldest


def test_insertion_at_capacity_evicts_through_the_hook():
    c = StageCache(2)
    c.put('a', _captured('a'))
    c.put('b', _captured('b'))
    calls = []

    def drop_two():                                          # an owner's hook may take dependants along
        calls.append(list(c))
        c.popitem(last=False)
        c.pop('b', None)

    assert c.put('c', _captured('c'), evict=drop_two).outputs == 'c'
    assert calls == [['a', 'b']] and list(c) == ['c']
    c.put('d', _captured('d'), evict=drop_two)
    assert calls == [['a', 'b']], 'below capacity nothing is evicted'
    c.put('e', _captured('e'))                               # the default hook drops the oldest entry only
    assert list(c) == ['d', 'e']


def test_callable_capacity_is_read_at_each_insertion():
    bound = [3]
    c = StageCache(lambda: bound[0])
    for k in 'abc':
        c.put(k, _captured(k))
    assert len(c) == 3
    bound[0] = 2
    c.put('d', _captured('d'))
    assert list(c) == ['c', 'd']
    bound[0] = 4
    for k in 'ef':
        c.put(k, _captured(k))
    assert list(c) == ['c', 'd', 'e', 'f']


def test_unbounded_cache_never_evicts():
    c = StageCache()
    for k in range(500):
        c.put(k, _captured(k), evict=lambda: pytest.fail('evicted'))
    assert len(c) == 500 and c.captures == 500


def test_captures_counts_captured_stages_only():
    c = StageCache(2)
    c.put('slot', Stage(None, [], 'buffers'))                # XMem.restored_key_slot: buffers without a graph
    assert c.captures == 0 and len(c) == 1
    c.put('a', _captured('a'))
    c.put('b', _captured('b'))
    assert c.captures == 2 and list(c) == ['a', 'b']
    c.clear()
    assert c.captures == 2 and len(c) == 0                   # graphs captured so far, not graphs held
    st = c.put('c', _captured('c'))
    assert c.captures == 3 and st[1] == [] and st[2] == 'c'  # callers index a stage as a tuple


# ---- capture -------------------------------------------------------------------------------------------------------------
class _FakeGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


@pytest.fixture
def fake_cuda(monkeypatch):
    """torch.cuda.CUDAGraph / graph / synchronize replaced: `events` records synchronize and the begin / end of the capture."""
    events = []

    @contextlib.contextmanager
    def graph_ctx(g):
        assert isinstance(g, _FakeGraph)
        events.append('capture begin')
        try:
            yield
        finally:
            events.append('capture end')

    monkeypatch.setattr(torch.cuda, 'CUDAGraph', _FakeGraph)
    monkeypatch.setattr(torch.cuda, 'graph', graph_ctx)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: events.append('synchronize'))
    return events


def test_capture_order_lock_and_mutated_inputs(fake_cuda):
    events = fake_cuda
    a, h = torch.arange(4.0), torch.ones(3)
    seen = []

    def fn(x, y, z):
        events.append('fn')
        seen.append((x, y, z, ops.CAPTURE_LOCK.locked()))
        if y is not None:
            y += 1                                           # the stage advances its state in place
        return x, y

    st = stages.capture(fn, [a, h, None], mutates=(1, 2))
    assert events == ['fn', 'synchronize', 'capture begin', 'fn', 'capture end']
    (wx, wy, wz, w_locked), (cx, cy, cz, c_locked) = seen
    # the warm-up got a clone of the mutated input (and the absent one as None), the capture the originals
    assert wx is a and wy is not h and wz is None and not w_locked
    assert cx is a and cy is h and cz is None and c_locked
    assert torch.equal(h, torch.full((3,), 2.0)), 'the state advanced once: the warm-up ran on a copy'
    assert not ops.CAPTURE_LOCK.locked()
    assert isinstance(st.graph, _FakeGraph) and st.inputs[1] is h and st.outputs[1] is h and st[2] is st.outputs


def test_capture_releases_the_lock_when_fn_raises(fake_cuda):
    calls = []

    def fn(x):
        calls.append(ops.CAPTURE_LOCK.locked())
        if len(calls) == 2:
            raise ValueError('inside the capture')
        return x

    with pytest.raises(ValueError, match='inside the capture'):
        stages.capture(fn, [torch.zeros(1)])
    assert calls == [False, True]
    assert not ops.CAPTURE_LOCK.locked()
    assert fake_cuda[-1] == 'capture end'


# ---- Stage.replay --------------------------------------------------------------------------------------------------------
def test_replay_copies_only_foreign_inputs(monkeypatch):
    own, other, absent = torch.zeros(4), torch.zeros(4), None
    st = Stage(_FakeGraph(), [own, other, absent], ('out',))
    copies = []
    orig = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, 'copy_', lambda self, src, *a, **k: (copies.append(self.data_ptr()), orig(self, src, *a, **k))[1])
    src = torch.arange(4.0)
    assert st.replay([own, src, None]) == ('out',)
    assert copies == [other.data_ptr()], 'the static buffer itself is not copied, another tensor is'
    assert torch.equal(other, src) and st.graph.replays == 1
    assert st.replay([own.view(2, 2), other, None]) == ('out',) and copies == [other.data_ptr()] and st.graph.replays == 2


# ---- the state-dict check ------------------------------------------------------------------------------------------------
SPEC = {'conv.weight': (2, 3), 'bn.running_mean': (2,), 'bn.num_batches_tracked': (), 'gate': ()}


def _toy_sd():
    return {'conv.weight': torch.zeros(2, 3), 'bn.running_mean': torch.zeros(2), 'bn.num_batches_tracked': torch.tensor(0), 'gate': torch.zeros(1)}


def test_state_dict_check_accepts_and_tolerates():
    sd = _toy_sd()
    hipnet.check_state_dict(sd, SPEC, 'Toy')                 # a one-element tensor passes for a scalar
    del sd['bn.num_batches_tracked']
    hipnet.check_state_dict(sd, SPEC, 'Toy')
    sd['aspp_dropout'] = torch.zeros(5)
    hipnet.check_state_dict(sd, SPEC, 'Toy', ignored=('aspp_dropout',))
    with pytest.raises(RuntimeError, match='unexpected'):
        hipnet.check_state_dict(sd, SPEC, 'Toy')


def test_state_dict_check_rejects_with_todays_messages():
    sd = _toy_sd()
    del sd['conv.weight']
    with pytest.raises(RuntimeError) as e:
        hipnet.check_state_dict(sd, SPEC, 'Toy')
    assert str(e.value) == "Error(s) in loading state_dict for Toy: missing ['conv.weight']..., unexpected []..."
    sd = _toy_sd()
    sd['extra.bias'] = torch.zeros(1)
    with pytest.raises(RuntimeError) as e:
        hipnet.check_state_dict(sd, SPEC, 'Toy')
    assert str(e.value) == "Error(s) in loading state_dict for Toy: missing []..., unexpected ['extra.bias']..."
    sd = _toy_sd()
    sd['conv.weight'] = torch.zeros(3, 2)
    with pytest.raises(RuntimeError) as e:
        hipnet.check_state_dict(sd, SPEC, 'Toy')
    assert str(e.value) == 'size mismatch for conv.weight: checkpoint (3, 2) vs model (2, 3)'


# ---- the source ----------------------------------------------------------------------------------------------------------
def test_one_capture_site_and_no_borrowed_methods():
    sources = {}
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith('.py'):
                with open(os.path.join(root, f)) as fh:
                    sources[os.path.relpath(os.path.join(root, f), PKG)] = fh.read()
    assert [p for p, text in sorted(sources.items()) if 'torch.cuda.graph(' in text] == ['stages.py']
    for p in ('s2m.py', 'click.py'):
        assert not re.search(r'XMem', sources[p]), f'{p} still reaches into network.XMem'
