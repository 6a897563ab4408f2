"""Edge-shape float64 parity of the affinity top-k (xmem_affinity_topk / xmem_affinity_topk_hinted: csrc/affinity.hip,
csrc/affinity_filter.hip) through the C ABI, for EVERY query of every case, against tests/affinity_refs.py:

    exact regime   out_sim equals the float64 similarity and out_idx equals topk_ref (value descending, index ascending), on every path
    dense regime   (a) indices distinct and in range, (b) each value within similarity_dense_bound of ITS index's reference,
                   (c) strict (value, index) order, (d) no unpicked element certainly better than a member
    both           (e) weights within (16 + k/8) u of float64 exp / sum of the returned similarities

Every launch writes into sentinel-padded outputs and a 0xFF-filled workspace of workspace_bytes + 4096 whose tail must survive; the
path each case is meant for is asserted with xmem_affinity_plan_info (affinity_refs.SHAPES holds the named shapes), so a heuristic
change that moves a shape off its edge fails here instead of leaving the edge untested.  Large-path cases run twice (the list
positions come from atomics) and must repeat their bits.  `pytest -s` prints, per test, the cases, the largest err/bound and the
share of queries whose index set equals topk_ref (never a gate in the dense regime: (d) is); profiles/r14_affinity_edge_tests.txt
holds the table of one run.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import affinity_refs as A
import memory_kernel_refs as M

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED, WORKSPACE, TOPK = 0, -1, -2, -3, -5          # xmem_status (include/xmem_hip.h)
W_SENT, I_SENT = -777.0, -12345
PAD = 64
REGIMES = ('exact', 'dense')
_CACHE = {}


def case(regime, n, hw, seed, ordering=None, k=30, positions=None, signed_e=False):
    """(inputs, ref64 [hw, n], bound [hw, n]) of one memory, computed once per session and never modified."""
    key = (regime, n, hw, seed, ordering, k if ordering else None, None if positions is None else tuple(positions), signed_e)
    if key not in _CACHE:
        d = A.make_inputs(regime, n, hw, seed, signed_e=signed_e or ordering == 'mixed_sign')
        if ordering:
            d = A.order_memory(d, ordering, k, positions=positions, seed=seed)
        if regime == 'exact':
            assert A.is_exact_regime(d, signed_e or ordering == 'mixed_sign')
        ref = A.similarity_ref(d['key'], d['shr'], d['qk'], d['qe'])
        bound = None if regime == 'exact' else M.similarity_dense_bound(d['key'], d['shr'], d['qk'], d['qe'])
        if len(_CACHE) > 6:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = (d, ref, bound)
    return _CACHE[key]


def launch(d, sizes, k, hint=None, want_sim=True, null_shr=(), ck=64, ws_short=0, n_seg=None):
    """One xmem_affinity_topk_hinted call on the memory d split into segments of `sizes` (each its own allocation).  Returns
    (status, w, idx, sim | None) as numpy [HW, k]; asserts that nothing beyond HW * k outputs and workspace_bytes was written."""
    from xmem2_amd import _lib
    lib = _lib.load()
    hw = d['qk'].shape[0]
    cuts = np.concatenate([[0], np.cumsum([max(s, 0) for s in sizes])]).astype(int)
    keep = []
    arr = (_lib.KeySegment * max(len(sizes), 1))()
    for i, s in enumerate(sizes):
        a, b = cuts[i], cuts[i + 1]
        kt = d['key'][a:b].clone().cuda() if s > 0 else None
        st = d['shr'][a:b].clone().cuda() if s > 0 and i not in null_shr else None
        keep += [kt, st]
        arr[i].key = kt.data_ptr() if kt is not None else None
        arr[i].shrinkage = st.data_ptr() if st is not None else None
        arr[i].n = s
        arr[i].rows16 = None
    qk, qe = d['qk'].cuda(), d['qe'].cuda()
    kk = max(k, 1)
    w = torch.full((hw * kk + PAD,), W_SENT, device='cuda')
    sim = torch.full((hw * kk + PAD,), W_SENT, device='cuda')
    idx = torch.full((hw * kk + PAD,), I_SENT, dtype=torch.int32, device='cuda')
    n_total = int(sum(s for s in sizes if s > 0))
    need = lib.xmem_affinity_topk_workspace_bytes(max(n_total, kk), hw, kk)
    assert need > 0
    ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device='cuda')
    hp = None
    if hint is not None:
        h = _lib.AffinityHint()
        hidx = hint['idx']
        assert hidx.is_cuda and hidx.dtype == torch.int32 and hidx.is_contiguous() and hidx.shape[0] == hw
        h.idx = hidx.data_ptr()
        h.top_k = hidx.shape[1]
        h.n_seg = hint.get('n_seg', len(hint['seg_n']))
        for i, s in enumerate(hint['seg_n']):
            h.seg_n[i] = int(s)
        h.grid_w = int(hint.get('grid_w', 0))
        hp = C.byref(h)
    rc = lib.xmem_affinity_topk_hinted(arr, len(sizes) if n_seg is None else n_seg, _lib.ptr(qk), _lib.ptr(qe), ck, hw, k, hp, _lib.ptr(w),
                                       _lib.ptr(idx), _lib.ptr(sim) if want_sim else None, _lib.ptr(ws), need - ws_short, _lib.stream_ptr())
    torch.cuda.synchronize()
    del keep
    used = hw * k if rc == OK else 0
    assert bool((w[used:] == W_SENT).all()) and bool((idx[used:] == I_SENT).all()), 'wrote past out_w / out_idx [HW][top_k]'
    assert bool((sim[used if want_sim else 0:] == W_SENT).all()), 'wrote past out_sim [HW][top_k] (or to a NULL out_sim)'
    assert bool((ws[need:] == 0xFF).all()), 'wrote past the workspace xmem_affinity_topk_workspace_bytes asks for'
    if rc != OK:
        assert bool((ws == 0xFF).all()), 'a refused call wrote to the workspace'
        return rc, None, None, None
    shape = (hw, k)
    return rc, w[:used].cpu().numpy().reshape(shape), idx[:used].cpu().numpy().reshape(shape), \
        (sim[:used].cpu().numpy().reshape(shape) if want_sim else None)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(x, y):
    return all((a is None and b is None) or np.array_equal(bits(a), bits(b)) for a, b in zip(x, y))


def route_of(sizes, hw, k, hint=None):
    rc, p = A.plan_info(list(sizes), hw, k, None if hint is None else hint['idx'].shape[1],
                        None if hint is None else hint.get('n_seg', len(hint['seg_n'])))
    assert rc == OK
    return p


class Table:
    """Collects (err/bound, set share) over the cases of one test and prints one line."""
    def __init__(self, name):
        self.name, self.n, self.sim, self.w, self.share = name, 0, 0.0, 0.0, 1.0

    def add(self, detail, share):
        self.n += 1
        self.sim, self.w = max(self.sim, detail['sim']), max(self.w, detail['w'])
        self.share = min(self.share, share)

    def show(self):
        print(f'\naffedge | {self.name:<80s} | {self.n:3d} cases | err/bound: similarity {self.sim:.3f} weights {self.w:.3f} | set share {self.share:.3f}')


def run_and_check(tab, regime, d, ref, bound, sizes, k, route, hint=None, twice=None, tag=''):
    """Launch, assert the route, hold every query to the reference; large paths run twice.  Returns (w, idx, sim)."""
    hw = d['qk'].shape[0]
    p = route_of(sizes, hw, k, hint)
    assert p['route'] == route, f'{tag}: planned {A.ROUTES[p["route"]]}, the case is meant for {A.ROUTES[route]} ({p})'
    rc, w, idx, sim = launch(d, sizes, k, hint=hint)
    assert rc == OK, f'{tag}: status {rc}'
    detail = {}
    worst, share = A.check_topk(idx, sim, w, ref, bound, k, exact=regime == 'exact', tag=f'{tag} [{regime}]', detail=detail)
    assert worst <= 1.0
    if route != A.SMALL if twice is None else twice:
        again = launch(d, sizes, k, hint=hint)
        assert same_bits((w, idx, sim), again[1:]), f'{tag}: a second launch returned other bits'
    tab.add(detail, share)
    return w, idx, sim


# ---------------------------------------------------------------------------------------------------------
# small path
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', REGIMES)
def test_small_path_memory_sizes(regime):
    """n = k, k + 1, around one tile, ragged last tiles, several splits, and the last size before the large path; HW = 65: two query
    tiles, the second with one query."""
    tab = Table(f'small path, n in k..8160, top_k=30 HW=65 [{regime}]')
    for n in (30, 31, 32, 33, 97, 225, 512, 1000, 8160):
        d, ref, bound = case(regime, n, 65, 100 + n)
        run_and_check(tab, regime, d, ref, bound, [n], 30, A.SMALL, tag=f'n={n}')
    tab.show()


@pytest.mark.parametrize('regime', REGIMES)
def test_small_path_query_counts(regime):
    tab = Table(f'small path, HW in 1, 63, 64, 65, 129 n=1000 [{regime}]')
    for hw in (1, 63, 64, 65, 129):
        d, ref, bound = case(regime, 1000, hw, 200 + hw)
        run_and_check(tab, regime, d, ref, bound, [1000], 30, A.SMALL, tag=f'HW={hw}')
    tab.show()


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('k', [1, 2, 30, 63, 64])
def test_small_path_top_k(k, regime):
    tab = Table(f'small path, top_k={k} x n in k, k+1, 97, 1000 x HW in 1, 65 [{regime}]')
    for n in sorted({k, k + 1, 97, 1000}):
        for hw in (1, 65):
            d, ref, bound = case(regime, n, hw, 300 + n + hw)
            run_and_check(tab, regime, d, ref, bound, [n], k, A.SMALL, tag=f'k={k} n={n} HW={hw}')
    tab.show()


def _cluster_positions(n, k, p):
    """The three places a whole top-k can hide: inside one tile, at the very end of the memory (its last, partial tile and the rows
    before it), across the boundary between the first two splits."""
    out = {'one tile': np.arange(5 * 32 + 1, 5 * 32 + 1 + k), 'memory end': np.arange(n - k, n)}
    if p['splits'] > 1 and not p['chunk']:
        b = p['tiles_per_split'] * 32
        out['split boundary'] = np.arange(b - k // 2, b - k // 2 + k)
    return out


def _ordering_cases(regime, n, hw, k, seed):
    p = route_of([n], hw, k)
    for o in A.ORDERINGS:
        if o == 'clustered':
            for name, pos in _cluster_positions(n, k, p).items():
                yield f'{o} ({name})', o, case(regime, n, hw, seed, o, k, positions=pos)
        else:
            yield o, o, case(regime, n, hw, seed, o, k)


def _check_ordering(o, d, ref, idx, k):
    """What an ordering promises beyond the reference check, in either regime: copies of a row have one fp32 value, so which of them
    are picked is decided by the index alone."""
    tile = min(d['qk'].shape[0], 64)
    if o == 'all_tied':
        assert np.array_equal(idx, np.broadcast_to(np.arange(k), idx.shape)), 'all rows tied: the result must be 0 .. k-1'
    if o == 'tie_at_kth':
        for q in range(tile):
            tied = np.nonzero(ref[q] == ref[q, idx[q, k - 1]])[0]
            got = np.sort(idx[q][np.isin(idx[q], tied)])
            assert tied.size >= 100 and np.array_equal(got, tied[:got.size]), f'query {q}: ties at the k-th place must go to the lowest indices'
    if o == 'zero_sim':
        assert np.array_equal(idx[0], np.arange(k)), f'every similarity of query 0 is a zero of either sign: 0 .. k-1, got {idx[0].tolist()}'


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('n', [1000, 8160])
def test_small_path_orderings(n, regime):
    """Adversarial arrangements of one memory against one query tile (64 copies of query 0, one more query behind them)."""
    tab = Table(f'small path, 10 orderings n={n} HW=65 top_k=30 [{regime}]')
    for name, o, (d, ref, bound) in _ordering_cases(regime, n, 65, 30, 400 + n):
        _, idx, _ = run_and_check(tab, regime, d, ref, bound, [n], 30, A.SMALL, tag=f'{name} n={n}')
        _check_ordering(o, d, ref, idx, 30)
    tab.show()


# ---------------------------------------------------------------------------------------------------------
# segment layouts: one virtual concatenation
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('n', [97, 1000])
def test_segment_layouts_return_the_same_bits(n, regime):
    """Every split of one memory into <= 4 segments (empty ones, one-element ones, ragged ones) gives the bits of the single segment."""
    tab = Table(f'segment layouts of n={n} HW=65 top_k=30 [{regime}]')
    d, ref, bound = case(regime, n, 65, 500 + n)
    layouts = [[n], [1, n - 1], [n - 1, 1], [0, n], [n, 0, 0, 0], [31, 33, 1, n - 65]]
    first = None
    for sizes in layouts:
        out = run_and_check(tab, regime, d, ref, bound, sizes, 30, A.SMALL, tag=f'layout {sizes}')
        first = first or out
        assert same_bits(first, out), f'layout {sizes} differs from the single segment'
    tab.show()


@pytest.mark.parametrize('regime', REGIMES)
def test_segments_that_sum_to_top_k_and_null_shrinkage(regime):
    tab = Table(f'(8,7,8,7) = top_k; shrinkage NULL on some segments [{regime}]')
    d, ref, bound = case(regime, 30, 65, 600)
    a = run_and_check(tab, regime, d, ref, bound, [8, 7, 8, 7], 30, A.SMALL, tag='(8,7,8,7)')
    assert same_bits(a, run_and_check(tab, regime, d, ref, bound, [30], 30, A.SMALL, tag='(30)'))
    # NULL shrinkage = 1: a memory whose segments 1 and 3 have shrinkage 1 gives the same bits with and without their arrays
    d0, _, _ = case(regime, 1000, 65, 601)
    d1 = dict(d0, shr=d0['shr'].clone())
    sizes = [31, 33, 1, 935]
    d1['shr'][31:64] = 1.0
    d1['shr'][65:] = 1.0
    ref1 = A.similarity_ref(d1['key'], d1['shr'], d1['qk'], d1['qe'])
    bound1 = None if regime == 'exact' else M.similarity_dense_bound(d1['key'], d1['shr'], d1['qk'], d1['qe'])
    full = run_and_check(tab, regime, d1, ref1, bound1, sizes, 30, A.SMALL, tag='shrinkage arrays')
    rc, w, idx, sim = launch(d1, sizes, 30, null_shr=(1, 3))
    assert rc == OK and same_bits(full, (w, idx, sim)), 'NULL shrinkage must mean 1'
    tab.show()


# ---------------------------------------------------------------------------------------------------------
# large path, un-hinted
# ---------------------------------------------------------------------------------------------------------
LARGE = {'n=8161': [8161], 'n=8192': [8192], '(1,1,1,8100)': [1, 1, 1, 8100]}


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', list(LARGE))
def test_large_path_thresholds(name, regime):
    """256 tiles with fewer than 8192 elements, 8192 elements, and 257 tiles of which three are padding; HW around the 128-query tile."""
    sizes = LARGE[name]
    n = sum(sizes)
    tab = Table(f'large path {name}, HW in 1, 127, 128, 129, 300 x top_k in 1, 30, 64 [{regime}]')
    for hw in (1, 127, 128, 129, 300):
        d, ref, bound = case(regime, n, hw, 700 + n + hw)
        for k in (1, 30, 64):
            run_and_check(tab, regime, d, ref, bound, sizes, k, A.LARGE_SAMPLED, tag=f'{name} HW={hw} k={k}')
    tab.show()


@pytest.mark.parametrize('regime', REGIMES)
def test_large_path_ragged_segments(regime):
    sh = A.SHAPES['20000 ragged']
    tab = Table(f'large path, 20000 elements in (6001, 0, 13999) HW=300 [{regime}]')
    d, ref, bound = case(regime, 20000, sh['hw'], 800)
    for k in (1, 30, 64):
        run_and_check(tab, regime, d, ref, bound, list(sh['segs']), k, A.LARGE_SAMPLED, tag=f'ragged k={k}')
    tab.show()


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', ['n=131072 HW=100', 'n=262144 HW=40'])
def test_large_path_chunk_dealing_and_bound_stride(name, regime):
    """Chunks dealt round-robin to the splits (on from 16 chunks per split), and the bound pass at every 8th tile (8192 tiles)."""
    sh = A.SHAPES[name]
    n = sum(sh['segs'])
    p = route_of(sh['segs'], sh['hw'], sh['k'])
    assert p['chunk'] == sh['grid']['chunk'] > 0 and p['bound_stride'] == sh['grid']['bound_stride']
    tab = Table(f'large path {name}: chunk {p["chunk"]}, R = {p["bound_stride"]} [{regime}]')
    d, ref, bound = case(regime, n, sh['hw'], 900)
    run_and_check(tab, regime, d, ref, bound, list(sh['segs']), sh['k'], A.LARGE_SAMPLED, tag=name)
    tab.show()


@pytest.mark.parametrize('regime', REGIMES)
def test_large_path_orderings(regime):
    """ascending drives the self-tightening lists, unsampled hides every good match from the sampled bound pass."""
    tab = Table(f'large path, 10 orderings n=8192 HW=129 top_k=30 [{regime}]')
    for name, o, (d, ref, bound) in _ordering_cases(regime, 8192, 129, 30, 1000):
        _, idx, _ = run_and_check(tab, regime, d, ref, bound, [8192], 30, A.LARGE_SAMPLED, tag=f'{name} n=8192')
        _check_ordering(o, d, ref, idx, 30)
    tab.show()


# ---------------------------------------------------------------------------------------------------------
# hinted
# ---------------------------------------------------------------------------------------------------------
def _hints(i0, sizes, hw, k, ref):
    """name -> (hint, is it used).  The stale ones are safe by reading affinity_hint_bound_kernel: the old slot and the row are clamped
    into today's segments before any load (`if (sgi >= p.n_seg)`, `if (o < 0)`, `if (o >= sd.n)`), and the hint array itself is read
    only at [neighbour < HW][position < k'].  Any k distinct elements give a valid bound, so every hint must give the reference."""
    n = int(sum(sizes))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    gw = max(1, int(round(hw ** 0.5)))
    out = {'perfect': (dict(idx=dev(i0), seg_n=sizes, grid_w=gw if hw % gw == 0 else 1), True)}
    if k < 64:
        out["k' = 64"] = (dict(idx=dev(A.topk_ref(ref, 64)[1]), seg_n=sizes), True)
    if k > 1:
        out["k' < k (ignored)"] = (dict(idx=dev(i0[:, :k - 1]), seg_n=sizes), False)
    out['n_seg mismatch (ignored)'] = (dict(idx=dev(i0), seg_n=sizes, n_seg=len(sizes) % 4 + 1), False)
    out['grid_w does not divide HW'] = (dict(idx=dev(i0), seg_n=sizes, grid_w=7), True)
    out['grid_w > HW'] = (dict(idx=dev(i0), seg_n=sizes, grid_w=hw + 3), True)
    grown = [s + 1500 for s in sizes]                         # the hint is from BEFORE an eviction: larger segments, indices beyond today's total
    out['before an eviction'] = (dict(idx=dev(i0 + 1500 * len(sizes)), seg_n=grown, grid_w=gw), True)
    shrunk = [max(s // 2, 1) for s in sizes]                  # from before growth: smaller segments
    out['before growth'] = (dict(idx=dev(i0 % sum(shrunk)), seg_n=shrunk, grid_w=gw), True)
    neg = i0.copy()
    neg[:, ::2] = -1 - neg[:, ::2]
    neg[0] = -2 ** 31
    out['negative entries'] = (dict(idx=dev(neg), seg_n=sizes, grid_w=gw), True)
    return out


HINTED = {'n=8161': [8161], 'n=8192': [8192], '(1,1,1,8100)': [1, 1, 1, 8100], '20000 ragged': [6001, 0, 13999]}


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('f16', ['1', '0'], ids=['filter16', 'fp32'])
@pytest.mark.parametrize('name', list(HINTED))
def test_hinted_paths_hold_the_reference(name, f16, regime, monkeypatch):
    """Every hint, fresh or stale, against the float64 reference AND bit for bit against the un-hinted call; HW in 1, 127, 128, 129,
    260 x top_k in 1, 30, 64.  The stale hints (from before an eviction: larger segments and indices at or beyond today's total; from
    before growth; negative entries) are safe by reading affinity_hint_bound_kernel: the old slot and the row are clamped into today's
    segments before any load, and the hint array is read only inside [HW][k']."""
    monkeypatch.setenv('XMEM_AFFINITY_FILTER16', f16)
    sizes = HINTED[name]
    n = sum(sizes)
    want = A.LARGE_HINTED_FILTER16 if f16 == '1' else A.LARGE_HINTED_FP32
    tab = Table(f'hinted {name} XMEM_AFFINITY_FILTER16={f16} [{regime}]')
    for hw in (1, 127, 128, 129, 260):
        d, ref, bound = case(regime, n, hw, 1100 + n + hw)
        for k in (1, 30, 64):
            rc, w0, i0, s0 = launch(d, sizes, k)
            assert rc == OK
            hints = _hints(i0, sizes, hw, k, ref)
            if (hw, k) not in ((128, 30), (260, 30)):               # every kind of hint at two sizes, the perfect one everywhere
                hints = {h: hints[h] for h in ('perfect',)}
            for hname, (hint, used) in hints.items():
                out = run_and_check(tab, regime, d, ref, bound, sizes, k, want if used else A.LARGE_SAMPLED, hint=hint,
                                    tag=f'{name} HW={hw} k={k} hint: {hname}')
                assert same_bits((w0, i0, s0), out), f'{name} HW={hw} k={k} hint {hname}: differs from the un-hinted call'
    tab.show()


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('f16', ['1', '0'], ids=['filter16', 'fp32'])
def test_hinted_orderings(f16, regime, monkeypatch):
    """Exact ties by the thousand and the signed zeros through the hint bound, the fp16 filter's lists and the refine."""
    monkeypatch.setenv('XMEM_AFFINITY_FILTER16', f16)
    want = A.LARGE_HINTED_FILTER16 if f16 == '1' else A.LARGE_HINTED_FP32
    tab = Table(f'hinted orderings n=8192 HW=129 XMEM_AFFINITY_FILTER16={f16} [{regime}]')
    for o in ('all_tied', 'tie_at_kth', 'zero_sim', 'mixed_sign', 'ascending'):
        d, ref, bound = case(regime, 8192, 129, 1000, o, 30)
        rc, w0, i0, s0 = launch(d, [8192], 30)
        assert rc == OK
        hint = dict(idx=torch.from_numpy(i0).cuda(), seg_n=[8192], grid_w=43)
        out = run_and_check(tab, regime, d, ref, bound, [8192], 30, want, hint=hint, tag=f'hinted {o}')
        assert same_bits((w0, i0, s0), out)
        _check_ordering(o, d, ref, out[1], 30)
    tab.show()


# ---------------------------------------------------------------------------------------------------------
# out_sim = NULL, the Python surface, refusals, non-finite similarities
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f16', ['1', '0'], ids=['filter16', 'fp32'])
def test_null_out_sim_changes_nothing(f16, monkeypatch):
    monkeypatch.setenv('XMEM_AFFINITY_FILTER16', f16)
    for sizes, hw in (([1000], 65), ([8192], 129)):
        d, ref, bound = case('dense', sum(sizes), hw, 1200)
        rc, w, idx, sim = launch(d, sizes, 30)
        hint = dict(idx=torch.from_numpy(idx).cuda(), seg_n=sizes)
        for h in (None, hint):
            rc2, w2, idx2, sim2 = launch(d, sizes, 30, hint=h, want_sim=False)
            assert rc == rc2 == OK and sim2 is None and same_bits((w, idx), (w2, idx2)), f'{sizes}: out_sim = NULL changed w or idx'


@pytest.mark.parametrize('regime', REGIMES)
def test_python_surface(regime):
    """ops.affinity_topk (what the product calls) on a small and a large memory with an empty middle segment."""
    from xmem2_amd import ops
    tab = Table(f'ops.affinity_topk, (400, 0, 600) and (6001, 0, 13999) [{regime}]')
    for sizes, hw in (([400, 0, 600], 65), ([6001, 0, 13999], 129)):
        d, ref, bound = case(regime, sum(sizes), hw, 1300)
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        segs = [(d['key'][a:b].cuda(), d['shr'][a:b].cuda()) for a, b in zip(cuts[:-1], cuts[1:])]
        w, idx, sim = ops.affinity_topk(segs, d['qk'].cuda(), d['qe'].cuda(), 30, want_sim=True)
        torch.cuda.synchronize()
        detail = {}
        _, share = A.check_topk(idx.cpu().numpy(), sim.cpu().numpy(), w.cpu().numpy(), ref, bound, 30, exact=regime == 'exact', tag=str(sizes), detail=detail)
        tab.add(detail, share)
        rc, w2, idx2, sim2 = launch(d, sizes, 30)
        assert same_bits((w.cpu().numpy(), idx.cpu().numpy(), sim.cpu().numpy()), (w2, idx2, sim2))
    tab.show()


def test_refusals_write_nothing():
    """Status codes, and neither the outputs nor the workspace are touched (launch() asserts both for every refused call)."""
    d, _, _ = case('dense', 1000, 65, 1400)
    five = dict(d, key=d['key'][:100], shr=d['shr'][:100])
    cases = {
        'workspace one byte short': (dict(d=d, sizes=[1000], k=30, ws_short=1), WORKSPACE),
        'Ck = 32': (dict(d=d, sizes=[1000], k=30, ck=32), UNSUPPORTED),
        'top_k = 0': (dict(d=d, sizes=[1000], k=0), UNSUPPORTED),
        'top_k = 65': (dict(d=d, sizes=[1000], k=65), UNSUPPORTED),
        'n_seg = 5': (dict(d=five, sizes=[20, 20, 20, 20, 20], k=30), BAD_ARG),
        'a negative n': (dict(d=d, sizes=[500, -1, 500], k=30), BAD_ARG),
        'sum n = k - 1': (dict(d=d, sizes=[15, 0, 14], k=30), TOPK),
    }
    for name, (kw, want) in cases.items():
        rc = launch(**kw)[0]
        assert rc == want, f'{name}: status {rc}, expected {want}'
    assert launch(d, [1000], 30)[0] == OK                                   # the valid twin is served


def _nonfinite_case(n, k, huge_rows, hw=65, seed=1500):
    d, _, _ = case('dense', n, hw, seed)
    d = dict(d, key=d['key'].clone())
    d['key'][huge_rows, 7] = 2e19                                           # its square overflows fp32: the similarity is -inf (e > 0)
    ref = A.similarity_ref(d['key'], d['shr'], d['qk'], d['qe'])
    bound = M.similarity_dense_bound(d['key'], d['shr'], d['qk'], d['qe'])
    ref[:, huge_rows] = -np.inf                                             # what fp32 (torch.topk on the fp32 similarity) sees
    return d, ref, bound


@pytest.mark.parametrize('name,n,huge', [('n = top_k + 2', 32, [1, 5, 29, 31]), ('n = 8192', 8192, [1, 5, 4000, 8191]),
                                         ('n = 8192, top_k - 2 finite', 8192, None)])
def test_non_finite_similarities(name, n, huge):
    """Key entries of 2e19 (the square overflows): those rows have similarity -inf.  With fewer than top_k finite similarities
    the -inf rows fill the result, lower index first, with weight 0 and out_sim = -inf - as torch.topk + exp give.  Only the affinity
    entry runs here and the outputs are inspected on the host."""
    k = 30
    if huge is None:
        huge = np.setdiff1d(np.arange(n), np.arange(40, 40 + 37 * (k - 2), 37))
    d, ref, bound = _nonfinite_case(n, k, np.asarray(huge))
    rc, w, idx, sim = launch(d, [n], k)
    assert rc == OK
    worst, share = A.check_topk(idx, sim, None, ref, bound, k, tag=name)
    vals_ref, idx_ref = A.topk_ref(ref, k)
    n_inf = int(np.isinf(vals_ref[0]).sum())
    assert np.array_equal(np.isinf(sim), np.isinf(vals_ref)) and np.array_equal(idx[np.isinf(sim)], idx_ref[np.isinf(vals_ref)])
    assert np.all(w[np.isinf(sim)] == 0) and np.all(np.isfinite(w))
    w64 = A.weights_ref(sim.astype(np.float64))
    fin = w64 > 0
    assert np.all(np.abs(w[fin] - w64[fin]) <= A.weights_rel_bound(k) * w64[fin])
    wr = float((np.abs(w[fin] - w64[fin]) / w64[fin]).max() / A.weights_rel_bound(k))
    print(f'\naffedge | {"non-finite, " + name + f" ({n_inf} members at -inf)":<80s} |   1 cases | err/bound: similarity {worst:.3f} weights {wr:.3f} | set share {share:.3f}')
