"""Captured HIP-graph stages: capture once, replay, keep the most recently replayed ones.

A *stage* is one forward function of fixed shapes captured into a HIP graph together with the static buffers it reads and writes.
Kernels are launched through ctypes on torch's current stream, which is the capturing stream inside ``torch.cuda.graph``, so they are
captured like any other launch.  Every network of the package (network.py, s2m.py, click.py, click_brs.py) captures through
``capture`` and keeps its stages in a ``StageCache``: nothing else in the package calls ``torch.cuda.graph``.
"""
from collections import OrderedDict, namedtuple

import torch

from . import ops


class Stage(namedtuple('Stage', ['graph', 'inputs', 'outputs'])):
    """(graph, static inputs, static outputs).  `graph` is None for a slot that only stores buffers (XMem.restored_key_slot)."""
    __slots__ = ()

    def replay(self, inputs):
        """Copy each of `inputs` (device or host tensors) into its static buffer unless it already is that buffer, replay the graph and
        return the static outputs.  A static input that is None (an absent optional input) takes nothing."""
        for dst, src in zip(self.inputs, inputs):
            if dst is not None and dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
        self.graph.replay()
        return self.outputs


def capture(fn, static_in, mutates=()):
    """Capture `fn(*static_in)` into a HIP graph -> Stage(graph, static_in, what fn returned).  `fn` first runs once eagerly: that sizes
    every workspace and picks the plans before the capture.  Inputs the stage updates in place (positions `mutates`: a hidden state) are
    cloned for this warm-up, otherwise warm-up + first replay would advance the state twice.
    The capture holds ops.CAPTURE_LOCK: no helper thread pins host memory meanwhile, which would invalidate it."""
    fn(*[t.clone() if (i in mutates and t is not None) else t for i, t in enumerate(static_in)])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.CAPTURE_LOCK, torch.cuda.graph(graph):
        outputs = fn(*static_in)
    return Stage(graph, static_in, outputs)


class StageCache(OrderedDict):
    """key -> stage, least recently used first.  `capacity`: the most entries kept - an int, None (unbounded) or a callable read at
    every insertion (a module constant that tests and tools may change).  `captures` counts the captured stages inserted so far; it
    survives clear().  A stage is anything with a `graph` attribute (Stage; click_brs._Objective)."""

    def __init__(self, capacity=None):
        super().__init__()
        self.capacity = capacity
        self.captures = 0

    def lookup(self, key):
        """The stage of `key`, now the most recently used one, or None."""
        st = self.get(key)
        if st is not None:
            self.move_to_end(key)
        return st

    def evict_lru(self):
        self.popitem(last=False)

    def put(self, key, stage, evict=None):
        """Insert `stage` as the most recently used entry and return it.  While the cache is at capacity, `evict()` is called first
        (default: evict_lru, which drops the least recently used entry); an owner whose entries depend on each other passes its own."""
        cap = self.capacity() if callable(self.capacity) else self.capacity
        while cap is not None and len(self) >= max(cap, 1):
            (evict or self.evict_lru)()
        self[key] = stage
        if stage.graph is not None:
            self.captures += 1
        return stage
