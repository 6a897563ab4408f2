"""The session's feature cache without a GPU: the C-ABI surface of `xmem_copy_segments`, and the policy of `FeatureCache` inside
`VideoSession.propagate` on a stub core - which batches go to the key pass, which are restored, which frames own an entry under a
budget, and what `cache_info()` counts.  The clip is the one of tests/test_gpu_session_cache.py: 9 frames, key_batch 4, so the
batches of a forward pass are [0-3], [4-7] and a tail [8] at batch 1."""

import numpy as np
import pytest
import torch

N, HW, CK, GRID = 9, (16, 32), 4, (1, 2)
# one frame's slices of a (made-up) key pass: key, shrinkage, selection, f16, skip8, skip4 - 2 grid cells, odd byte counts on purpose
LAYOUT = (((2, CK), torch.float32), ((2,), torch.float32), ((2, CK), torch.float32), ((1, 1, 2, 3), torch.float16),
          ((1, 2, 4, 5), torch.float16), ((1, 4, 8, 1), torch.float32))


# ---- 2. symbols -------------------------------------------------------------------------------------------------------------
def test_copy_segments_is_declared_listed_and_exported_and_the_abi_version_stays_5():
    from xmem2_amd import _lib, build, ops
    assert 5 == _lib.ABI_VERSION and _lib.COPY_MAX_SEGMENTS >= 16 and 'copy_segments.hip' in build.SOURCES
    lib = _lib.load()
    assert hasattr(lib, 'xmem_copy_segments') and lib.xmem_version() == 5
    # bad arguments and empty calls are answered on the host, without a launch
    assert lib.xmem_copy_segments(None, None, None, 0, None) == 0
    assert lib.xmem_copy_segments(None, None, None, 2, None) != 0 and lib.xmem_copy_segments(None, None, None, -1, None) != 0
    import ctypes as C
    src, dst = (C.c_void_p * 2)(4096, 0), (C.c_void_p * 2)(4096 + 8, 0)
    assert lib.xmem_copy_segments(src, dst, (C.c_size_t * 2)(0, 0), 2, None) == 0           # nothing but empty segments
    assert lib.xmem_copy_segments(src, dst, (C.c_size_t * 2)(0, 16), 2, None) != 0          # a NULL side of a non-empty segment
    assert lib.xmem_copy_segments(src, dst, (C.c_size_t * 2)(16, 0), 2, None) != 0          # source and destination overlap
    assert callable(ops.copy_segments)
    with pytest.raises(RuntimeError):
        ops.copy_segments([(torch.zeros(4), torch.zeros(4))])                               # host tensors: there is no CPU path


# ---- 3. policy --------------------------------------------------------------------------------------------------------------
class _Core:
    """Records the hints a session gives its core.  `strict`: the core of today - `prefetch_keys(frames, inputs_complete=...)` is the only
    call it knows."""

    def __init__(self, log, strict):
        self.log, self.strict, self.memory = log, strict, None

    def set_all_labels(self, labels):
        pass

    def clear_memory(self, keep_permanent=False):
        pass

    def put_to_permanent_memory(self, image, mask, ti=None):
        return False

    def _frames(self, images):
        return [int(im[0, 0, 0]) for im in images]

    def prefetch_keys(self, images, inputs_complete=False, **more):
        if self.strict:
            assert more == {}, f'unexpected arguments {sorted(more)}'
            self.log.append(('keys', self._frames(images), inputs_complete))
            return list(images)
        entries = more.pop('save_to')(LAYOUT)                 # the key pass reports its layout and is told where to save
        assert more == {} and len(entries) == len(images)
        for t, e in zip(self._frames(images), entries):
            if e is not None:
                assert [(tuple(v.shape), v.dtype) for v in e] == [tuple(x) for x in LAYOUT]
                for v in e:
                    v.fill_(t)                                # "saved": the entry now holds frame t
        self.log.append(('keys', self._frames(images), inputs_complete, [t for t, e in zip(self._frames(images), entries) if e is not None]))
        return list(images)

    def prefetch_cached(self, images, entries, inputs_complete=False):
        assert not self.strict
        for t, e in zip(self._frames(images), entries):
            assert all(bool((v == t).all()) for v in e), f'the entry handed over for frame {t} is not the one saved for it'
        self.log.append(('cached', self._frames(images), inputs_complete))
        return list(images)

    def step(self, image, mask, labels, end=False, manually_curated_masks=False, do_not_add_mask_to_memory=False, return_key_and_stuff=False):
        prob = torch.zeros((2,) + HW); prob[0] = 1.0
        key = torch.zeros(1, CK, *GRID)
        return prob, key, torch.zeros(1, 1, *GRID), key


def _session(monkeypatch, budget_entries=None, strict=False):
    """A session on stubs (tests/test_session_host.py's manner); budget_entries None: the cache option is off."""
    import xmem2_amd.run_on_video as rv
    from xmem2_amd import session as S
    from xmem2_amd.mask_mapper import MaskMapper
    s = object.__new__(S.VideoSession)
    s.device = torch.device('cpu')
    s.log = []
    s.core, s.mapper = _Core(s.log, strict), MaskMapper()
    s.shape, s.frames = HW, []
    for t in range(N):
        f = object.__new__(S._Frame)
        gt = np.zeros(HW, np.uint8); gt[2:5, 1 + t % 3:6] = 1
        f.frame, f.shape, f.need_resize, f.raw_image_pil, f.mask = f'{t:05d}.jpg', HW, False, None, gt
        s.frames.append(f)
    s.n_device_frames = N
    s._dev_frames = torch.zeros((N,) + HW + (3,), dtype=torch.uint8)
    for t in range(N):
        s._dev_frames[t] = t                                  # a frame is recognised by its value
    s._host_frames = None
    s.grid_hw = GRID
    s.key = torch.zeros(N, 2, CK); s.shrinkage = torch.zeros(N, 2); s.selection = torch.zeros(N, 2, CK)
    s.masks = torch.zeros((N,) + HW, dtype=torch.uint8)
    s._present, s._refs, s.key_batch = [False] * N, {}, 4
    if budget_entries is not None:
        entry = _entry_bytes()
        s._fcache = S.FeatureCache(N, budget_entries * entry + entry // 2, s.device)     # half an entry too much: it must not be used
    monkeypatch.setattr(rv, '_post_process_gpu', lambda sample, prob: prob.argmax(0).to(torch.uint8))
    s.save_reference(0)
    return s


def _entry_bytes():
    from xmem2_amd.session import ENTRY_ALIGN
    return sum(-(-int(np.prod(sh)) * torch.empty((), dtype=dt).element_size() // ENTRY_ALIGN) * ENTRY_ALIGN for sh, dt in LAYOUT)


def test_with_the_option_off_the_core_sees_todays_calls_and_nothing_else(monkeypatch):
    s = _session(monkeypatch, None, strict=True)
    assert getattr(s, '_fcache', None) is None
    for _ in range(2):
        s.log.clear()
        s.full_propagation()
        assert s.log == [('keys', [0, 1, 2, 3], True), ('keys', [4, 5, 6, 7], True), ('keys', [8], True)]
    assert s.cache_info() == dict(entry_bytes=0, frames=0, bytes=0, hits=0, misses=0)


def test_the_option_is_read_from_the_config_and_is_not_a_default():
    from xmem2_amd.configuration import VIDEO_INFERENCE_CONFIG
    from xmem2_amd import session as S
    assert 'session_feature_cache_bytes' not in VIDEO_INFERENCE_CONFIG
    import inspect
    assert "config.get('session_feature_cache_bytes', 0)" in inspect.getsource(S.VideoSession.__init__)
    a = S.parse_args(['--images', 'i', '--masks', 'm', '--out', 'o', '--feature-cache-gb', '1.5'])
    assert a.feature_cache_gb == 1.5 and S.parse_args(['--images', 'i', '--masks', 'm', '--out', 'o']).feature_cache_gb == 0.0
    with pytest.raises(SystemExit):
        S.parse_args(['--images', 'i', '--masks', 'm', '--out', 'o', '--feature-cache-gb', '-1'])


def test_round_one_saves_and_round_two_restores_whole_batches(monkeypatch):
    s = _session(monkeypatch, N)
    assert s.cache_info() == dict(entry_bytes=0, frames=0, bytes=0, hits=0, misses=0)      # no key pass yet: no layout, no arena
    s.full_propagation()
    assert s.log == [('keys', [0, 1, 2, 3], True, [0, 1, 2, 3]), ('keys', [4, 5, 6, 7], True, [4, 5, 6, 7]), ('keys', [8], True, [8])]
    entry = _entry_bytes()
    assert s.cache_info() == dict(entry_bytes=entry, frames=N, bytes=N * entry, hits=0, misses=N)
    assert entry % 256 == 0 and s._fcache.arena.numel() == N * entry                       # min(budget, T * entry_bytes)
    for round_ in (2, 3):
        s.log.clear()
        s.full_propagation()
        assert s.log == [('cached', [0, 1, 2, 3], True), ('cached', [4, 5, 6, 7], True), ('cached', [8], True)]
        assert s.cache_info()['hits'] == (round_ - 1) * N and s.cache_info()['misses'] == N
    # entries do not overlap and are aligned
    fc = s._fcache
    spans = sorted((v.data_ptr(), v.data_ptr() + v.numel() * v.element_size()) for t in range(N) for v in fc._entry(fc._slot[t]))
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and all((a - fc.arena.data_ptr()) % 256 == 0 for a, _ in spans)
    with pytest.raises(RuntimeError, match='layout'):
        fc.claim([0], LAYOUT[:-1])


def test_a_batch_with_one_untagged_or_differently_tagged_frame_goes_to_the_key_pass(monkeypatch):
    s = _session(monkeypatch, N)
    s.propagate(1, 'forward', 4)                             # [1, 2, 3, 4] as one batch of four
    assert s.log == [('keys', [1, 2, 3, 4], True, [1, 2, 3, 4])]
    s.log.clear()
    s.full_propagation()                                     # [0-3]: frame 0 has no entry; [4-7]: only frame 4 has one; [8]: none
    assert s.log == [('keys', [0, 1, 2, 3], True, [0, 1, 2, 3]), ('keys', [4, 5, 6, 7], True, [4, 5, 6, 7]), ('keys', [8], True, [8])]
    s.log.clear()
    s.propagate(6, 'forward')                                # [6], [7], [8] frame by frame: 6 and 7 were saved by a pass of four
    assert s.log == [('keys', [6], True, [6]), ('keys', [7], True, [7]), ('cached', [8], True)]
    s.log.clear()
    s.full_propagation()                                     # ... and are now tagged 1: their batch of four runs the key pass again
    assert s.log == [('cached', [0, 1, 2, 3], True), ('keys', [4, 5, 6, 7], True, [4, 5, 6, 7]), ('cached', [8], True)]
    assert s.cache_info()['hits'] == 1 + 4 + 1 and s.cache_info()['misses'] == 4 + 9 + 2 + 4


def test_a_budget_of_five_entries_caches_frames_0_to_4(monkeypatch):
    s = _session(monkeypatch, 5)
    s.full_propagation()
    assert s.log == [('keys', [0, 1, 2, 3], True, [0, 1, 2, 3]), ('keys', [4, 5, 6, 7], True, [4]), ('keys', [8], True, [])]
    entry = _entry_bytes()
    info = s.cache_info()
    assert info == dict(entry_bytes=entry, frames=5, bytes=5 * entry, hits=0, misses=N) and info['bytes'] <= s._fcache.budget
    s.log.clear()
    s.full_propagation()
    assert s.log == [('cached', [0, 1, 2, 3], True), ('keys', [4, 5, 6, 7], True, [4]), ('keys', [8], True, [])]
    assert s.cache_info() == dict(entry_bytes=entry, frames=5, bytes=5 * entry, hits=4, misses=N + 5)


def test_a_backward_pass_after_a_forward_one(monkeypatch):
    s = _session(monkeypatch, N)
    s.full_propagation()
    s.log.clear()
    s.propagate(8, 'backward')
    # frame 8 was saved alone and frame 0 in a batch of four: their batches run the key pass; [4, 3, 2, 1] were all saved by passes of four
    assert s.log == [('keys', [8, 7, 6, 5], True, [8, 7, 6, 5]), ('cached', [4, 3, 2, 1], True), ('keys', [0], True, [0])]
    assert s.cache_info()['hits'] == 4 and s.cache_info()['misses'] == N + 5
    s.log.clear()
    s.propagate(8, 'backward')                               # the re-tagged entries now serve this order
    assert s.log == [('cached', [8, 7, 6, 5], True), ('cached', [4, 3, 2, 1], True), ('cached', [0], True)]
    assert s.cache_info()['hits'] == 4 + N and s.cache_info()['frames'] == N
