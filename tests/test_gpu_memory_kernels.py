"""Edge-shape float64 parity of the memory readout, usage and consolidation kernels (csrc/affinity.hip: readout_sparse,
usage_update, similarity_dense; csrc/consolidate.hip), and of MemoryManager.consolidation as a whole.

Every comparison is against the float64 references of tests/memory_kernel_refs.py over ALL outputs, within an a-priori
round-off bound per output element computed from the reference's own magnitudes (u = 2^-24):

    readout, fp32 out      (top_k + 1) u sum_s |w v|
    readout, half out      the fp32 bound + 2^-11 |ref| + 2^-25                 (one rounding to half)
    usage_update           2 (hits 2^-40 + u S + u |use_old + S|)               (truncation per term, sum and add rounded once)
    weighted_rows          (count/4 + 4) u sum_i |aff V|
    softmax_rows_suffix    relative (A + count/256 + 16) u, + 1e-37 absolute    (A: largest shift of a non-negligible entry)
    similarity_dense       (2 Ck + 4) u (sum_c (|x^2 e| + 2 |x k e|) + |b_sq|) ms / sqrt(Ck)
    topk_1d, select_greater, gather_rows      bit-exact values, exact index lists
    usage_ratio            1 ulp of torch's fp32 use / life

Each test prints its largest err / bound (`pytest -s`); the table of one run is profiles/r08_memory_kernel_tests.txt.
"""
import numpy as np
import pytest
import torch

import memory_kernel_refs as M
from conftest import base_config

pytestmark = pytest.mark.gpu
U = M.U
SENTINEL = -777.0                 # exactly representable as a half

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2          # xmem_status (include/xmem_hip.h)


def g_(seed):
    return torch.Generator().manual_seed(seed)


def report(name, got, ref, bound):
    """max |got - ref| / bound over all elements (0 where the error is exactly 0; inf where a bound of 0 is missed)."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f'{name}: non-finite output'
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / np.broadcast_to(bound, err.shape))
    return float(ratio.max()) if ratio.size else 0.0


def show(name, worst):
    print(f'\nmemkern | {name:<58s} | max err/bound {worst:.3f}')


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ---------------------------------------------------------------------------------------------------------
# sparse readout
# ---------------------------------------------------------------------------------------------------------
N1, N2, N3, N4 = 19, 33, 1, 64
LAYOUTS = {'n': [53], '0_n1_n2': [0, N1, N2], 'n1_0_n2': [N1, 0, N2], 'n1_n2_0': [N1, N2, 0], 'n1_n2_n3_n4': [N1, N2, N3, N4]}


def _readout_inputs(sizes, n_obj, top_k, cv, hw, seed):
    gen = g_(seed)
    n_total = sum(sizes)
    V = [torch.randn(n_total, cv, generator=gen) + 0.25 * (o + 1) for o in range(n_obj)]     # distinct per object
    idx = torch.randint(0, n_total, (hw, top_k), generator=gen).to(torch.int32)
    edges, a = [], 0
    for s in sizes:                                   # first and last row of every non-empty segment is hit by some query
        if s:
            edges += [a, a + s - 1]
        a += s
    assert len(edges) + 2 <= hw
    for j, r in enumerate(edges):
        idx[j, 0] = r
    if top_k >= 2:                                    # duplicate indices within a query
        idx[hw - 1, 1] = idx[hw - 1, 0]
        idx[hw - 2, :] = idx[hw - 2, 0]
    w = torch.rand(hw, top_k, generator=gen) + 0.01
    w = w / w.sum(1, keepdim=True) * (0.5 + torch.rand(hw, 1, generator=gen))      # rows sum to 0.5 .. 1.5: no weight is exactly 1
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    host = [[(V[o][a:b] if b > a else None) for a, b in zip(cuts[:-1], cuts[1:])] for o in range(n_obj)]
    # every segment is its own allocation (made in reverse order): a kernel that walked on from segment 0's pointer would not land in the next one
    dev = [[(s.clone().cuda() if s is not None else None) for s in reversed(segs)][::-1] for segs in reversed(host)][::-1]
    return host, dev, w, idx


def _run_readout(sizes, n_obj, top_k, cv, hw, seed, half, sliced):
    """Launch into a sentinel-filled buffer; returns err/bound of the slices, after checking that nothing else was written."""
    from xmem2_amd import ops
    host, dev, w, idx = _readout_inputs(sizes, n_obj, top_k, cv, hw, seed)
    ld, off = (cv + 12, 8) if sliced else (cv, 0)
    stride = hw * ld + (16 if sliced else 0)
    buf = torch.full((n_obj * stride,), SENTINEL, dtype=torch.float16 if half else torch.float32, device='cuda')
    ops.readout_sparse(dev, w.cuda(), idx.cuda(), cv, buf, ld, stride, out_off=off)
    torch.cuda.synchronize()
    flat = buf.cpu().double().numpy()
    pos = np.arange(n_obj)[:, None, None] * stride + np.arange(hw)[None, :, None] * ld + off + np.arange(cv)[None, None, :]
    out = flat[pos]
    rest = np.ones(flat.size, bool)
    rest[pos.ravel()] = False
    assert np.all(flat[rest] == SENTINEL), 'the readout wrote outside out[obj][q][out_off : out_off + Cv]'
    ref, mag = M.readout_ref(host, w, idx)
    bound = (top_k + 1) * U * mag
    if half:
        bound = bound + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    return report('readout', out, ref, bound)


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half'])
@pytest.mark.parametrize('top_k', [1, 5, 6, 7, 30, 31, 64])
def test_readout_topk_and_segment_layouts(top_k, half):
    """top_k around the unroll of 6 (tail loop), x every segment layout (empty leading / middle / trailing segments passed
    as None), x 1 and 3 objects; Cv = 36, HW = 37."""
    worst = 0.0
    for li, (name, sizes) in enumerate(LAYOUTS.items()):
        for n_obj in (1, 3):
            r = _run_readout(sizes, n_obj, top_k, 36, 37, 1000 + 10 * top_k + li, half, sliced=False)
            assert r <= 1.0, f'layout {name}, {n_obj} objects: err/bound {r:.3f}'
            worst = max(worst, r)
    show(f'readout {"half" if half else "fp32"} top_k={top_k} (5 layouts x 1,3 objects)', worst)


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half'])
@pytest.mark.parametrize('cv', [4, 36, 512, 1028, 2048])
def test_readout_channel_counts(cv, half):
    """Cv below one wave, the product's 512, and > 1024 (several passes of the 256-thread channel loop, ragged last pass)."""
    r = _run_readout(LAYOUTS['n1_n2_n3_n4'], 3, 7, cv, 37, 2000 + cv, half, sliced=False)
    show(f'readout {"half" if half else "fp32"} Cv={cv} top_k=7', r)
    assert r <= 1.0


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half'])
@pytest.mark.parametrize('n_obj,layout', [(17, 'n1_n2_n3_n4'), (65, 'n')], ids=['17obj_4seg', '65obj_1seg'])
def test_readout_object_chunking(n_obj, layout, half):
    """More objects than one launch carries (64 / n_seg pointer slots): 16 + 1 and 64 + 1."""
    r = _run_readout(LAYOUTS[layout], n_obj, 7, 36, 37, 3000 + n_obj, half, sliced=False)
    show(f'readout {"half" if half else "fp32"} {n_obj} objects x {len(LAYOUTS[layout])} segments', r)
    assert r <= 1.0


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half'])
@pytest.mark.parametrize('n_obj,layout,top_k', [(3, 'n1_0_n2', 7), (3, 'n1_n2_n3_n4', 30), (17, 'n1_n2_n3_n4', 31)])
def test_readout_into_a_slice(n_obj, layout, top_k, half):
    """ldout = Cv + 12, out_off = 8, obj_stride = HW * ldout + 16: everything outside the slices keeps the sentinel."""
    r = _run_readout(LAYOUTS[layout], n_obj, top_k, 36, 37, 4000 + top_k, half, sliced=True)
    show(f'readout {"half" if half else "fp32"} into a slice, {n_obj} objects top_k={top_k}', r)
    assert r <= 1.0


def _raw_readout(segs, n_obj, n_seg, hw, top_k, cv, ldout, obj_stride, half=False, buf_elems=None):
    """xmem_readout_sparse_t through the C ABI with explicit (possibly invalid) arguments; returns (status, output buffer)."""
    from xmem2_amd import _lib
    lib = _lib.load()
    arr = (_lib.ValueSegment * len(segs))()
    for i, v in enumerate(segs):
        arr[i].value = v.data_ptr() if v is not None else None
        arr[i].n = v.shape[0] if v is not None else 0
    k_alloc = max(top_k, 1)
    w = torch.full((hw, k_alloc), 1.0 / k_alloc, device='cuda')
    idx = torch.zeros((hw, k_alloc), dtype=torch.int32, device='cuda')
    buf = torch.full((buf_elems or n_obj * max(obj_stride, hw * max(ldout, cv)),), SENTINEL,
                     dtype=torch.float16 if half else torch.float32, device='cuda')
    rc = lib.xmem_readout_sparse_t(arr, n_obj, n_seg, _lib.ptr(w), _lib.ptr(idx), hw, top_k, cv, _lib.ptr(buf), int(half),
                                   ldout, obj_stride, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, buf


def test_readout_refuses_unsupported_arguments():
    """Status codes only (nothing is launched): Cv % 4, ldout < Cv, five segments, an object whose segment sizes differ."""
    hw = 5
    v8 = [torch.ones(10, 8, device='cuda') for _ in range(5)]
    short = torch.ones(9, 8, device='cuda')
    cases = {
        'Cv % 4': (dict(segs=[torch.ones(10, 6, device='cuda')], n_obj=1, n_seg=1, cv=6, ldout=8, obj_stride=hw * 8), UNSUPPORTED),
        'ldout < Cv': (dict(segs=v8[:1], n_obj=1, n_seg=1, cv=8, ldout=4, obj_stride=hw * 8), UNSUPPORTED),
        'n_seg = 5': (dict(segs=v8, n_obj=1, n_seg=5, cv=8, ldout=8, obj_stride=hw * 8), BAD_ARG),
        'segment sizes differ': (dict(segs=[v8[0], v8[1], v8[2], short], n_obj=2, n_seg=2, cv=8, ldout=8, obj_stride=hw * 8), BAD_ARG),
    }
    for name, (kw, want) in cases.items():
        rc, buf = _raw_readout(hw=hw, top_k=3, **kw)
        assert rc == want, f'{name}: status {rc}, expected {want}'
        assert bool((buf == SENTINEL).all()), f'{name}: a refused call wrote to the output'
    rc, buf = _raw_readout(segs=v8[:2], n_obj=2, n_seg=1, hw=hw, top_k=3, cv=8, ldout=8, obj_stride=hw * 8)     # the valid twin is served
    assert rc == OK and not bool((buf == SENTINEL).any())


@pytest.mark.parametrize('half', [False, True], ids=['fp32', 'half'])
def test_readout_refuses_top_k_above_64(half):
    """The kernel resolves its row pointers into 64-entry tables: top_k = 65 is XMEM_ERR_UNSUPPORTED and nothing is written;
    top_k = 64 (the largest the select emits) is served; top_k = 0 stays a bad argument."""
    v = [torch.ones(70, 8, device='cuda')]
    rc, buf = _raw_readout(segs=v, n_obj=1, n_seg=1, hw=5, top_k=65, cv=8, ldout=8, obj_stride=40, half=half)
    assert rc == UNSUPPORTED, f'top_k = 65: status {rc}'
    assert bool((buf == SENTINEL).all()), 'a refused call wrote to the output'
    rc, buf = _raw_readout(segs=v, n_obj=1, n_seg=1, hw=5, top_k=0, cv=8, ldout=8, obj_stride=40, half=half)
    assert rc == BAD_ARG and bool((buf == SENTINEL).all())
    rc, buf = _raw_readout(segs=v, n_obj=1, n_seg=1, hw=5, top_k=64, cv=8, ldout=8, obj_stride=40, half=half)
    assert rc == OK
    assert bool((buf.float() - 1.0).abs().max() < 1e-3)          # 64 weights of 1/64 on rows of ones


# ---------------------------------------------------------------------------------------------------------
# usage_update
# ---------------------------------------------------------------------------------------------------------
def _usage_inputs(hw, top_k, L, T, Pm, seed):
    """(w, idx) over an index space [long L | tmp T | perm Pm]: one element of each counted store is hit by every query, the
    window edges are hit, and two elements per store are never hit."""
    gen = g_(seed)
    n = L + T + Pm
    never = torch.tensor([10, L - 3, L + 10, L + T - 3])
    idx = torch.randint(0, n, (hw, top_k), generator=gen)
    idx[torch.isin(idx, never)] = n - 1
    if top_k >= 2:
        idx[:, 0] = L + 5                             # the largest sum: hit by every query
        idx[:, 1] = 3
    for j, r in enumerate([0, L - 1, L, L + T - 1, L + T]):
        idx[j, top_k - 1] = r
    w = torch.rand(hw, top_k, generator=gen) + 1e-3
    w = w / w.sum(1, keepdim=True)
    return w, idx.to(torch.int32), never


def _check_usage(tag, w, idx, first, count, never, seed):
    from xmem2_amd import ops
    gen = g_(seed)
    use0 = torch.rand(count, generator=gen) * 5 + 0.5              # non-zero use_count
    life0 = torch.randint(1, 9, (count,), generator=gen).float() + 1e-7
    use, life = use0.cuda(), life0.cuda()
    wd, idxd = w.cuda(), idx.cuda()
    ops.usage_update(wd, idxd, first, count, use, life)
    torch.cuda.synchronize()
    S, hits = M.usage_ref(w, idx, first, count)
    got = use.cpu().numpy()
    r = report(tag, got, use0.double().numpy() + S, M.usage_bound(S, hits, use0))
    cold = hits == 0
    assert cold.sum() >= 2 and set((never[(never >= first) & (never < first + count)] - first).tolist()) <= set(np.nonzero(cold)[0].tolist())
    assert np.array_equal(bits(got[cold]), bits(use0.numpy()[cold])), 'an element without a hit changed its use_count'
    assert np.array_equal(bits(life.cpu().numpy()), bits((life0 + 1).numpy())), 'life_count != life + 1'
    assert int(hits.max()) >= w.shape[0], 'no element is hit by every query'
    # determinism: the same call again, and with the query rows permuted
    for perm in (None, torch.randperm(w.shape[0], generator=gen)):
        use2, life2 = use0.cuda(), life0.cuda()
        w2, i2 = (wd, idxd) if perm is None else (w[perm].contiguous().cuda(), idx[perm].contiguous().cuda())
        ops.usage_update(w2, i2, first, count, use2, life2)
        assert torch.equal(use2, use), 'use_count depends on the accumulation order'
    return r


@pytest.mark.parametrize('hw,top_k', [(37, 7), (8200, 64)], ids=['37x7', '8200x64_grid_stride'])
def test_usage_update_windows(hw, top_k):
    """The two windows match_memory_rows passes ([0, L) for the long-term store, [L, L + T) for the temporary one; the
    permanent range is never passed): indices below and beyond each window are filtered, sums within the fixed-point bound,
    cold elements untouched, life + 1, bit-identical under repetition and permutation of the queries."""
    L, T, Pm = 700, 1300, 500
    w, idx, never = _usage_inputs(hw, top_k, L, T, Pm, 50 + hw)
    assert int((idx < L).sum()) and int((idx >= L + T).sum())
    r_long = _check_usage('usage long', w, idx, 0, L, never, 60)
    r_tmp = _check_usage('usage tmp', w, idx, L, T, never, 61)
    show(f'usage_update HW*top_k={hw}x{top_k} window [0,L)', r_long)
    show(f'usage_update HW*top_k={hw}x{top_k} window [L,L+T)', r_tmp)
    assert r_long <= 1.0 and r_tmp <= 1.0


def test_usage_update_count_zero_is_a_noop():
    from xmem2_amd import _lib
    lib = _lib.load()
    w, idx, _ = _usage_inputs(37, 7, 70, 130, 50, 70)
    use, life = torch.full((8,), 2.5, device='cuda'), torch.full((8,), 3.0, device='cuda')
    fx = torch.full((8,), 99, dtype=torch.int64, device='cuda')
    rc = lib.xmem_usage_update(_lib.ptr(w.cuda()), _lib.ptr(idx.cuda()), 37, 7, 70, 0, _lib.ptr(use), _lib.ptr(life), _lib.ptr(fx),
                               _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == OK
    assert bool((use == 2.5).all()) and bool((life == 3.0).all()) and bool((fx == 99).all())


# ---------------------------------------------------------------------------------------------------------
# eviction / prototype selection: topk_1d, select_greater, gather_rows, usage_ratio
# ---------------------------------------------------------------------------------------------------------
SIZES_1D = [1, 255, 256, 257, 1000]


def _value_sets(n, seed):
    gen = g_(seed)
    zeros = torch.zeros(n)
    hot = torch.randperm(n, generator=gen)[:max(1, n // 40)]
    zeros[hot] = torch.randint(1, 4, (hot.numel(),), generator=gen).float() * 0.125         # positives with ties among them
    return {
        'distinct': torch.randperm(n, generator=gen).float() * 0.37 - 0.25 * n,
        'five_values': torch.randint(0, 5, (n,), generator=gen).float() * 0.5,
        'all_equal': torch.full((n,), 0.75),
        'mostly_zeros': zeros,                         # the long-term usage picture: never-matched elements have usage 0
    }


def _check_topk(v, k, largest, tag):
    from xmem2_amd import ops
    vals, idx = ops.topk_1d(v.cuda(), k, largest=largest)
    torch.cuda.synchronize()
    rv, ri = M.topk_1d_ref(v, k, largest)
    assert idx.cpu().tolist() == ri.tolist(), f'{tag}: index list differs from the stable ranking'
    assert np.array_equal(bits(vals.cpu().numpy()), bits(rv)), f'{tag}: values are not bit-exact'


@pytest.mark.parametrize('n', SIZES_1D)
def test_topk_1d_ties_and_chunk_edges(n):
    from xmem2_amd import ops
    ks = sorted({1, n} | ({128} if n >= 128 else set()))
    for name, v in _value_sets(n, 80 + n).items():
        for k in ks:
            for largest in (True, False):
                _check_topk(v, k, largest, f'{name} n={n} k={k} largest={largest}')
    with pytest.raises(RuntimeError, match='top_k'):
        ops.topk_1d(torch.zeros(n, device='cuda'), n + 1)


def test_topk_1d_infinities_and_signed_zeros():
    v = torch.tensor([0.0, -0.0, 1.0, float('inf'), -0.0, 0.0, float('-inf'), float('inf'), -1.0, float('-inf'), 0.0] * 25)
    for k in (1, 7, 128, v.numel()):
        for largest in (True, False):
            _check_topk(v, k, largest, f'inf/zero k={k} largest={largest}')


@pytest.mark.parametrize('n', SIZES_1D)
def test_select_greater_thresholds(n):
    from xmem2_amd import ops
    for name, v in _value_sets(n, 90 + n).items():
        srt = torch.sort(v)[0]
        for what, thr in (('max', float(v.max())), ('below_min', float(v.min()) - 1.0), ('tied', float(srt[n // 2]))):
            sel, cnt = ops.select_greater(v.cuda(), torch.tensor([thr], device='cuda'))
            torch.cuda.synchronize()
            keep = M.select_greater_ref(v, thr)
            m = int(cnt.item())
            assert m == keep.size, f'{name} n={n} thr={what}: count {m}, expected {keep.size}'
            assert sel[:m].cpu().tolist() == keep.tolist(), f'{name} n={n} thr={what}: kept indices differ'
            if what == 'max':
                assert m == 0
            if what == 'below_min':
                assert m == n


@pytest.mark.parametrize('n', SIZES_1D[1:])
def test_eviction_survivors_on_tied_usage(n):
    """topk_1d(largest=False) + select_greater == usage > topk(usage, k, largest=False).values[-1] (the reference's survivor
    formula, kv_memory_store.py:165) on usage vectors full of exact ties."""
    from xmem2_amd import ops
    for name, v in _value_sets(n, 100 + n).items():
        for k in sorted({1, n // 3, n - 1, n}):
            vals, _ = ops.topk_1d(v.cuda(), k, largest=False)
            sel, cnt = ops.select_greater(v.cuda(), vals[k - 1:k])
            keep = torch.nonzero(v > torch.topk(v, k, largest=False, sorted=True).values[-1]).flatten()
            m = int(cnt.item())
            assert m == keep.numel() and sel[:m].cpu().tolist() == keep.tolist(), f'{name} n={n} k={k}'


@pytest.mark.parametrize('c', [1, 3, 24, 512])
def test_gather_rows_exact(c):
    from xmem2_amd import ops
    gen = g_(110 + c)
    n_src = 700
    src = torch.randn(n_src, generator=gen) if c == 1 else torch.randn(n_src, c, generator=gen)
    picks = {
        'repeated': torch.randint(0, 40, (300,), generator=gen),
        'descending': torch.arange(n_src - 1, -1, -1),
        'edges': torch.tensor([0, n_src - 1, 0, n_src - 1]),
    }
    if c == 512:
        picks['grid_stride_2100x512'] = torch.randint(0, n_src, (2100,), generator=gen)      # n * C > 4096 * 256
    for name, pick in picks.items():
        got = ops.gather_rows(src.cuda(), pick.to(torch.int32).cuda())
        torch.cuda.synchronize()
        want = src[pick]
        assert got.shape == want.shape
        assert np.array_equal(bits(got.cpu().numpy()), bits(want.numpy())), f'C={c} {name}'


def test_usage_ratio_one_ulp():
    from xmem2_amd import ops
    gen = g_(120)
    n = 1000
    use = torch.rand(n, generator=gen) * 40
    use[::7] = 0.0
    life = torch.randint(1, 60, (n,), generator=gen).float() + 1e-7
    got = ops.usage_ratio(use.cuda(), life.cuda()).cpu().numpy()
    ref = (use / life).numpy()
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ulp).max())
    show('usage_ratio n=1000 (err in ulps of torch fp32 use/life)', worst)
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------
# consolidation: softmax_rows_suffix, weighted_rows, similarity_dense
# ---------------------------------------------------------------------------------------------------------
def _check_softmax(sim, count, tag):
    from xmem2_amd import ops
    n = sim.shape[1]
    got = ops.softmax_rows_suffix(sim.clone().cuda(), count).cpu().numpy()
    assert np.all(got[:, :n - count] == 0.0), f'{tag}: the prefix is not exactly 0'
    ref = M.softmax_suffix_ref(sim, count)
    rel = M.softmax_suffix_rel_bound(sim, count)
    r = report(tag, got[:, n - count:], ref[:, n - count:], rel * ref[:, n - count:] + 1e-37)
    assert r <= 1.0, f'{tag}: err/bound {r:.3f}'
    return r


@pytest.mark.parametrize('P', [1, 128])
def test_softmax_rows_suffix_shapes(P):
    worst = 0.0
    for n, count in [(300, 1), (300, 255), (600, 256), (600, 257), (500, 500), (2500, 1700)]:
        sim = torch.randn(P, n, generator=g_(130 + count)) * 3.0
        worst = max(worst, _check_softmax(sim, count, f'softmax P={P} n={n} count={count}'))
    show(f'softmax_rows_suffix P={P} (6 (n, count) shapes)', worst)


def test_softmax_rows_suffix_needs_its_max_shift():
    """Rows around -1e4 with a spread of 60: exp(x) underflows for every entry, exp(x - max) does not."""
    P, n, count = 7, 600, 257
    sim = -1e4 + torch.rand(P, n, generator=g_(140)) * 60.0
    sim[:, :n - count] = 5.0                            # a larger value before the suffix must not become the shift
    show('softmax_rows_suffix rows ~ -1e4, spread 60', _check_softmax(sim, count, 'softmax shifted'))


@pytest.mark.parametrize('count', [1, 3, 4, 5, 1700])
def test_weighted_rows_shapes(count):
    from xmem2_amd import ops
    n = count + 37
    worst = 0.0
    for P in (1, 7, 8, 9, 128):
        gen = g_(150 + count + P)
        aff = torch.rand(P, n, generator=gen)            # the first n - count columns must not be read
        aff[:, n - count:] /= aff[:, n - count:].sum(1, keepdim=True)
        for c in (1, 63, 64, 65, 512):
            V = torch.randn(count, generator=gen) if c == 1 else torch.randn(count, c, generator=gen)
            got = ops.weighted_rows(aff.cuda(), count, V.cuda()).cpu().numpy()
            ref, mag = M.weighted_rows_ref(aff, count, V)
            r = report('weighted_rows', got, ref, (count / 4.0 + 4.0) * U * mag)
            assert r <= 1.0, f'P={P} C={c} count={count}: err/bound {r:.3f}'
            worst = max(worst, r)
    show(f'weighted_rows count={count} (P in 1,7,8,9,128 x C in 1,63,64,65,512)', worst)


@pytest.mark.parametrize('ck', [4, 64, 132])
def test_similarity_dense_shapes(ck):
    from xmem2_amd import ops
    worst = 0.0
    for n in (1, 255, 257, 2500):
        for P in (1, 128):
            gen = g_(160 + n + P + ck)
            key = torch.randn(n, ck, generator=gen) * 0.9
            shr = torch.rand(n, generator=gen) * 3 + 1
            qk = torch.randn(P, ck, generator=gen) * 0.9
            qe = torch.rand(P, ck, generator=gen) * 0.9 + 0.05
            for use_s in (True, False):
                for use_e in (True, False):
                    s, e = (shr if use_s else None), (qe if use_e else None)
                    got = ops.similarity_dense(key.cuda(), s.cuda() if use_s else None, qk.cuda(), e.cuda() if use_e else None)
                    r = report('similarity_dense', got.cpu().numpy(), M.similarity_dense_ref(key, s, qk, e),
                               M.similarity_dense_bound(key, s, qk, e))
                    assert r <= 1.0, f'n={n} P={P} Ck={ck} shrinkage={use_s} selection={use_e}: err/bound {r:.3f}'
                    worst = max(worst, r)
    show(f'similarity_dense Ck={ck} (n in 1,255,257,2500 x P in 1,128 x +-shr x +-sel)', worst)


def test_similarity_dense_refuses_ck_6():
    from xmem2_amd import ops
    with pytest.raises(RuntimeError, match='not supported'):
        ops.similarity_dense(torch.ones(10, 6, device='cuda'), None, torch.ones(2, 6, device='cuda'), None)


# ---------------------------------------------------------------------------------------------------------
# MemoryManager.consolidation as a whole, with the usage ranking pinned
# ---------------------------------------------------------------------------------------------------------
H16, W16, CK, CV, P_PROTO, MIN_FRAMES = 6, 8, 64, 32, 16, 2
HW = H16 * W16


def _manager(frames_objects, seed):
    """A MemoryManager whose temporary store was filled through add_memory, one entry of `frames_objects` per frame."""
    from xmem2_amd.memory_manager import MemoryManager
    gen = g_(seed)
    mm = MemoryManager(base_config(min_mid_term_frames=MIN_FRAMES, max_mid_term_frames=50, num_prototypes=P_PROTO))
    for objects in frames_objects:
        key = (torch.randn(HW, CK, generator=gen) * 0.9).cuda()
        shr = (torch.rand(HW, generator=gen) * 3 + 1).cuda()
        sel = (torch.rand(HW, CK, generator=gen) * 0.9 + 0.05).cuda()
        val = (torch.randn(len(objects), HW, CV, generator=gen) + torch.arange(len(objects)).view(-1, 1, 1) * 0.25).cuda()
        mm.add_memory(key, shr, val, objects, selection=sel, hw_shape=(H16, W16))
    return mm


def _consolidate_and_compare(mm, use, tag):
    """Pin usage = use / 4 (exact in fp32), run mm.consolidation and compare with consolidation_ref on the same rows."""
    tmp = mm.temporary_work_mem
    total = tmp.size
    assert use.numel() == total
    tmp._use.rows().copy_(use.cuda())
    tmp._life.rows().fill_(4.0)
    n_c = total - mm.min_work_elements
    cand_counts = []                                   # as compress_features derives them (memory_manager.py:316-347)
    for gi in range(tmp.num_groups):
        n_g = tmp.get_v_size(gi)
        cand_counts.append(n_g - mm.min_work_elements if (n_g == total or n_g > mm.min_work_elements) else None)
    pk, pv, ps = mm.consolidation(n_c, cand_counts)
    torch.cuda.synchronize()

    cand_key = tmp.key_rows()[:n_c].t().unsqueeze(0).cpu()
    cand_shr = tmp.shrinkage_rows()[:n_c].view(1, 1, -1).cpu()
    cand_sel = tmp.selection_rows()[:n_c].t().unsqueeze(0).cpu()
    usage = (use[:n_c] / 4.0).view(1, 1, -1)
    cand_values = [tmp.value_rows(gi)[:, :cnt].transpose(1, 2).cpu() if cnt is not None else None
                   for gi, cnt in enumerate(cand_counts)]
    qk, qv, qs, aux = M.consolidation_ref(cand_key, cand_shr, cand_sel, usage, cand_values, P_PROTO, return_aux=True)

    assert np.array_equal(bits(pk.cpu().numpy()), bits(qk[0].t().float().numpy())), f'{tag}: prototype keys are not bit-equal'
    # The similarity of the candidates to the (bit-equal) prototypes is the deterministic kernel checked on its own above: it is
    # recomputed here and held to its bound, and the values / shrinkage are then held to the composed softmax and weighted-rows
    # bounds on that fp32 similarity - round-off only, nothing is left for a ranking or a gather to hide in.
    from xmem2_amd import ops
    sim64 = aux['similarity'][0].t().numpy()                                        # [P, n_c]
    rows = lambda t: t[0].t().contiguous()
    proto_sel32 = rows(aux['proto_sel']).float()
    eps = M.similarity_dense_bound(rows(cand_key), cand_shr.flatten(), rows(qk).float(), proto_sel32)
    sim32 = ops.similarity_dense(tmp.key_rows()[:n_c], tmp.shrinkage_rows()[:n_c], pk, proto_sel32.cuda()).cpu().numpy()
    r_sim = report('similarity', sim32, sim64, eps)
    assert r_sim <= 1.0, f'{tag}: similarity err/bound {r_sim:.3f}'
    worst = 0.0
    assert len(pv) == len(qv)
    for gi, cnt in enumerate(cand_counts):
        assert (pv[gi] is None) == (qv[gi] is None), f'{tag}: group {gi} None-ness differs'
        if qv[gi] is None:
            continue
        valid = aux['validity'][gi].numpy()
        d_sm = M.softmax_suffix_rel_bound(sim32, cnt)                                # relative error of the fp32 affinity, per prototype
        d_sim = np.expm1(2.0 * eps[:, n_c - cnt:].max(1, keepdims=True))             # what the similarity's own error does to it
        aff = M.softmax_suffix_ref(sim32, cnt)
        assert tuple(pv[gi].shape) == (qv[gi].shape[0], int(valid.sum()), CV), f'{tag}: group {gi} prototype count'

        def check(name, got, V, full64):
            ref, mag = M.weighted_rows_ref(aff, cnt, V)
            bound = ((cnt / 4.0 + 4.0) * U * (1.0 + d_sm) + d_sm) * mag + 1e-37 * np.abs(M._np64(V)).sum(0)
            assert np.all(np.abs(ref[valid] - full64) <= 1.01 * (d_sim * mag)[valid] + 1e-300), f'{tag}: {name} left the float64 consolidation'
            return report(name, got, ref[valid], bound[valid])
        for o in range(qv[gi].shape[0]):
            worst = max(worst, check('proto value', pv[gi][o].cpu().numpy(), cand_values[gi][o].t(), qv[gi][o].t().numpy()))
        if gi == 0:
            worst = max(worst, check('proto shrinkage', ps.cpu().numpy()[:, None], cand_shr.flatten(), qs.flatten().numpy()[:, None]))
    show(f'consolidation {tag} (similarity {r_sim:.3f})', worst)
    assert worst <= 1.0
    return aux, pv, cand_counts


def test_consolidation_one_group():
    mm = _manager([[1, 2]] * 5, 200)
    use = torch.randperm(5 * HW, generator=g_(201)).float()
    aux, pv, counts = _consolidate_and_compare(mm, use, 'one group')
    assert counts == [3 * HW] and tuple(pv[0].shape) == (2, P_PROTO, CV)


def test_consolidation_two_groups_valid_gather():
    """The third object appears in frame 4 of 6: its group holds 3 frames > min_work_elements, so only the prototypes drawn
    from its candidates (the last HW of 4 HW) are valid for it."""
    mm = _manager([[1, 2]] * 3 + [[1, 2, 3]] * 3, 210)
    n_c = 4 * HW
    gen = g_(211)
    use = torch.randperm(6 * HW, generator=gen).float()
    early = torch.randperm(3 * HW, generator=gen)[:11]
    late = 3 * HW + torch.randperm(HW, generator=gen)[:5]
    order = torch.cat([early, late])[torch.randperm(16, generator=gen)]
    use[order] = 1000.0 + torch.arange(16, 0, -1).float()            # the prototypes, in this order
    aux, pv, counts = _consolidate_and_compare(mm, use, 'two groups, valid gather')
    assert counts == [n_c, HW]
    assert aux['proto_idx'].tolist() == order.tolist()
    assert tuple(pv[0].shape) == (2, P_PROTO, CV) and tuple(pv[1].shape) == (1, 5, CV)


def test_consolidation_second_group_too_young():
    """The third object appears in the last two frames: n_g == min_work_elements -> no candidates -> None."""
    mm = _manager([[1, 2]] * 4 + [[1, 2, 3]] * 2, 220)
    use = torch.randperm(6 * HW, generator=g_(221)).float()
    aux, pv, counts = _consolidate_and_compare(mm, use, 'second group too young')
    assert counts == [4 * HW, None] and pv[1] is None


def test_consolidation_no_valid_prototype_for_second_group():
    mm = _manager([[1, 2]] * 3 + [[1, 2, 3]] * 3, 230)
    use = torch.randperm(6 * HW, generator=g_(231)).float()
    use[:3 * HW] += 1000.0                                            # every prototype comes from before the third object
    aux, pv, counts = _consolidate_and_compare(mm, use, 'no valid prototype for group 2')
    assert counts == [4 * HW, HW] and pv[1] is None and int(aux['proto_idx'].max()) < 3 * HW


def test_consolidation_ties_across_the_last_rank():
    """Five usage levels: the P-th rank falls inside a run of equal usages; the documented rule (lower index first) decides
    which of them become prototypes, and in which order."""
    mm = _manager([[1, 2]] * 3 + [[1, 2, 3]] * 3, 240)
    gen = g_(241)
    n_c = 4 * HW
    use = torch.zeros(6 * HW)
    spots = torch.randperm(n_c, generator=gen)
    use[spots[:6]] = 4.0
    use[spots[6:36]] = 3.0                                            # ranks 7..36 are tied: 10 of the 30 are taken
    use[spots[36:80]] = 2.0
    use[n_c:] = torch.randint(0, 5, (2 * HW,), generator=gen).float()
    aux, pv, counts = _consolidate_and_compare(mm, use, 'ties across the P-th rank')
    want = sorted(spots[:6].tolist()) + sorted(spots[6:36].tolist())[:10]
    assert aux['proto_idx'].tolist() == want
    n_valid = sum(i >= 3 * HW for i in want)
    assert (pv[1] is None) == (n_valid == 0) and (pv[1] is None or pv[1].shape[1] == n_valid)
