"""Edge-shape parity of the annotation-candidate selector kernels (csrc/selector.hip) through xmem2_amd.ops, against
tests/selector_refs.py:

    score    exact regime: the per-tile float64 partials the kernel leaves in the 'selector' workspace and its scores EQUAL score_ref
             at every edge of the 64x64 wave block and the 128x128 tile, with every frame in turn as `chosen`; 289 tiles reach the
             reduce kernel's strided pass.  dense regime: every tile and score within score_tile_bound.
    prepare  Mexp and Qexp bit-equal to prepare_ref, bsq within (Ck + 2) u sum |e ck^2| (equal in the exact regime), the nearest-resize
             source pixel read back as a value, the presence count exact on both grid-stride passes, for the float and the uint8 kernel.

Nothing here is tuned to the kernels' output: tests/test_selector_refs_host.py shows on the CPU that the exact comparison of tiles
catches a mis-masked edge, exchanged operands, a transposed accumulator block and a wave block counted twice.
`pytest -s` prints the largest err/bound of the dense cases."""
import numpy as np
import pytest
import torch

import selector_refs as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (5, 7, 2, 3), (3, 4, 6, 8), (97, 131, 7, 9), (10, 10, 3, 3), (480, 854, 30, 54)]        # H, W, h, w
WIDTHS = (1, 8, 64, 96, 128)          # an idle-lane wave, the product width, a half-full second pass, two passes
ALPHAS = (0.0, 0.3, 0.5, 1.0)
NAN = float('nan')
_DEVICE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------
# score kernel
# ---------------------------------------------------------------------------------------------------------
def run_score(d, chosen, valid=None):
    """ops.cycle_dissimilarity on the operands of d: (tiles [F, t, t], scores [F]) as float64 numpy.  The workspace is NaN-filled
    before the call, so a partial the kernel does not write cannot pass."""
    from xmem2_amd import ops
    from xmem2_amd._lib import load
    dev = torch.device('cuda:0')
    if id(d) not in _DEVICE:
        _DEVICE.clear()                                           # one case resident at a time
        _DEVICE[id(d)] = tuple(d[k].to(dev).contiguous() for k in ('Mexp', 'Qexp', 'bsq', 'shr'))
    nf, hw = d['Mexp'].shape[0], d['Mexp'].shape[1]
    t = S.n_tiles(hw)
    nbytes = load().xmem_cycle_dissimilarity_workspace_bytes(nf, hw)
    assert nbytes == nf * t * t * 8
    ops.workspace(nbytes, dev, 'selector')[:nbytes].view(torch.float64).fill_(NAN)
    v = None if valid is None else torch.tensor(valid, dtype=torch.uint8, device=dev)
    scores = ops.cycle_dissimilarity(*_DEVICE[id(d)], chosen, v)
    assert scores.dtype == torch.float64 and scores.shape == (nf,)
    tiles = ops.workspace(nbytes, dev, 'selector')[:nbytes].view(torch.float64).view(nf, t, t).cpu().numpy()
    return tiles, scores.cpu().numpy()


@pytest.mark.parametrize('hw', S.EDGE_HW)
def test_score_exact_tiles_and_scores_equal_the_reference(hw):
    d = S.edge_case(hw)
    for chosen in range(3):
        tiles, scores = run_score(d, chosen)
        bad = np.argwhere(tiles != d['tiles'][chosen])
        assert bad.size == 0, (f'HW={hw} chosen={chosen}: tile partial (frame, row tile, column tile) = {bad[0].tolist()}: got '
                               f'{tiles[tuple(bad[0])]!r} want {d["tiles"][chosen][tuple(bad[0])]!r}; {len(bad)} of {tiles.size} differ')
        assert np.array_equal(scores, d['scores'][chosen]), f'HW={hw} chosen={chosen}: scores {scores} want {d["scores"][chosen]}'


def test_score_exact_289_tiles_reach_the_strided_reduce():
    d = S.edge_case(2049)
    assert S.n_tiles(2049) ** 2 == 289 > 256
    for chosen in range(2):
        tiles, scores = run_score(d, chosen)
        assert np.array_equal(scores, d['scores'][chosen]), f'chosen={chosen}: scores {scores} want {d["scores"][chosen]}'
        assert np.array_equal(tiles, d['tiles'][chosen]), f'chosen={chosen}: {int((tiles != d["tiles"][chosen]).sum())} tile partials differ'


def test_score_invalid_frame_is_zero_and_leaves_the_others_alone():
    d = S.edge_case(129)
    for chosen in (0, 2):
        t_all, s_all = run_score(d, chosen)
        t_v, s_v = run_score(d, chosen, valid=[1, 0, 1])
        assert not t_v[1].any() and not np.signbit(t_v[1]).any() and s_v[1] == 0.0 and not np.signbit(s_v[1])
        for f in (0, 2):
            assert np.array_equal(t_v[f], t_all[f]) and s_v[f] == s_all[f]
        want_t, want_s = S.score_ref(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], chosen, [1, 0, 1])
        assert np.array_equal(t_v, want_t) and np.array_equal(s_v, want_s)


@pytest.mark.parametrize('hw,alpha', [(33, 0.3), (129, 0.7), (257, 0.5)])
def test_score_dense_within_the_derived_bounds(hw, alpha):
    d = S.make_inputs('dense', 3, hw, 20 + hw, alpha=alpha)
    worst_t = worst_s = 0.0
    for chosen in range(3):
        tiles, scores = run_score(d, chosen)
        again_t, again_s = run_score(d, chosen)
        assert np.array_equal(tiles.view(np.int64), again_t.view(np.int64)) and np.array_equal(scores.view(np.int64), again_s.view(np.int64))
        assert scores[chosen] == 0.0 and not tiles[chosen].any(), 'a frame against itself: both chains see the same operands'
        bt, bs = S.score_tile_bound(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], chosen)
        et, es = np.abs(tiles - d['tiles'][chosen]), np.abs(scores - d['scores'][chosen])
        other = np.arange(3) != chosen
        worst_t = max(worst_t, float((et[other] / bt[other]).max()))
        worst_s = max(worst_s, float((es[other] / bs[other]).max()))
        print(f'dense HW={hw} chosen={chosen}: max err/bound tiles {float((et[other] / bt[other]).max()):.4f} scores {float((es[other] / bs[other]).max()):.4f}')
        assert np.all(et <= bt), f'HW={hw} chosen={chosen}: tile off by {float((et[other] / bt[other]).max()):.3f} of its bound'
        assert np.all(es <= bs), f'HW={hw} chosen={chosen}: score off by {float((es[other] / bs[other]).max()):.3f} of its bound'
    print(f'dense HW={hw}: max err/bound tiles {worst_t:.4f} scores {worst_s:.4f}')


def test_score_serves_only_ck_64():
    from xmem2_amd import ops
    x = torch.zeros(2, 5, 16, device='cuda')
    b = torch.zeros(2, 5, device='cuda')
    with pytest.raises(RuntimeError):
        ops.cycle_dissimilarity(x, x, b, b, 0)


# ---------------------------------------------------------------------------------------------------------
# prepare kernels
# ---------------------------------------------------------------------------------------------------------
def run_prepare(key, sel, mask, h, w, alpha, eps=0.5, lut=None):
    """ops.selector_prepare (lut: ops.selector_prepare_u8) into NaN-filled outputs: (Mexp, Qexp, bsq, presence) as numpy / int."""
    from xmem2_amd import ops
    hw, ck = key.shape
    Mexp = torch.full((hw, 2 * ck), NAN, device='cuda')
    Qexp = torch.full_like(Mexp, NAN)
    bsq = torch.full((hw,), NAN, device='cuda')
    pres = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    if lut is None:
        ops.selector_prepare(key, sel, mask, h, w, alpha, eps, Mexp, Qexp, bsq, pres)
    else:
        ops.selector_prepare_u8(key, sel, mask, lut, h, w, alpha, eps, Mexp, Qexp, bsq, pres)
    return Mexp.cpu().numpy(), Qexp.cpu().numpy(), bsq.cpu().numpy(), int(pres)


def check_prepare(got, ref, tag):
    Mexp, Qexp, bsq, pres = got
    for name, a in (('Mexp', Mexp), ('Qexp', Qexp)):
        bad = np.argwhere(bits(a) != bits(ref[name]))
        assert bad.size == 0, f'{tag}: {name}[{bad[0].tolist()}] = {a[tuple(bad[0])]!r}, want {ref[name][tuple(bad[0])]!r} ({len(bad)} differ)'
    err = np.abs(bsq.astype(np.float64) - ref['bsq'])
    assert np.all(err <= ref['bsq_bound']), f'{tag}: bsq off by {float(err.max()):.3g} at pixel {int(err.argmax())} (bound {ref["bsq_bound"][err.argmax()]:.3g})'
    assert pres == ref['presence'], f'{tag}: presence {pres}, want {ref["presence"]}'
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.where(err > 0, err / ref['bsq_bound'], 0.0).max())


@pytest.mark.parametrize('H,W,h,w', SHAPES)
def test_prepare_matches_the_reference(H, W, h, w):
    g = torch.Generator().manual_seed(H * 1000 + W)
    key_all = torch.randn(h * w, max(WIDTHS), generator=g)
    sel_all = torch.rand(h * w, max(WIDTHS), generator=g)
    mask3 = torch.rand(3, H, W, generator=g)
    mask3.view(-1)[::7] = 0.0
    mask3.view(-1)[3::11] = 1.0
    worst = dict.fromkeys(WIDTHS, 0.0)
    for C in (1, 3):
        mask = mask3[:C].contiguous()
        mask_d = mask.cuda()
        for ck in WIDTHS:
            key, sel = key_all[:, :ck].contiguous(), sel_all[:, :ck].contiguous()
            key_d, sel_d = key.cuda(), sel.cuda()
            for alpha in ALPHAS:
                ref = S.prepare_ref(key, sel, mask, h, w, alpha)
                worst[ck] = max(worst[ck], check_prepare(run_prepare(key_d, sel_d, mask_d, h, w, alpha), ref, f'{(H, W, h, w)} C={C} Ck={ck} alpha={alpha}'))
    print(f'prepare {(H, W, h, w)}: bsq max err/bound by Ck ' + ', '.join(f'{ck}: {v:.3f}' for ck, v in worst.items()))


@pytest.mark.parametrize('H,W,h,w', SHAPES)
def test_prepare_reads_the_pixel_interpolate_nearest_reads(H, W, h, w):
    """key = 1, alpha = 1, mask[y][x] = y W + x (exact in fp32): the composite key IS the index of the source pixel."""
    plane = torch.arange(H * W, dtype=torch.float32).view(1, H, W)
    assert H * W < 2 ** 24
    want = S.nearest(plane, h, w).reshape(h * w).numpy()
    ck = 8
    key = torch.ones(h * w, ck, device='cuda')
    Mexp, _, _, pres = run_prepare(key, key, plane.cuda(), h, w, 1.0)
    got = Mexp[:, ck:]
    bad = np.argwhere(got != want[:, None])
    assert bad.size == 0, f'pixel {bad[0][0]} = ({bad[0][0] // w}, {bad[0][0] % w}) read source index {got[tuple(bad[0])]}, interpolate reads {want[bad[0][0]]}'
    assert pres == H * W - 1                                     # every index but 0 exceeds eps = 0.5


@pytest.mark.parametrize('ck', [1, 64, 96])
def test_prepare_without_a_mask_keeps_the_key_bits(ck):
    g = torch.Generator().manual_seed(ck)
    key, sel = torch.randn(35, ck, generator=g), torch.rand(35, ck, generator=g)
    key[0, 0] = -0.0
    got = run_prepare(key.cuda(), sel.cuda(), None, 5, 7, 0.3)
    assert np.array_equal(bits(got[0][:, ck:]), bits(key.numpy()))
    check_prepare(got, S.prepare_ref(key, sel, None, 5, 7, 0.3), f'no mask Ck={ck}')


@pytest.mark.parametrize('hw', [33, 129])
def test_prepare_exact_regime_bsq_is_equal(hw):
    d = S.edge_case(hw)
    for f in range(3):
        mask = d['m'][f].view(1, hw, 1)
        Mexp, Qexp, bsq, pres = run_prepare(d['key'][f].cuda(), d['sel'][f].cuda(), mask.cuda(), hw, 1, d['alpha'])
        assert np.array_equal(bits(Mexp), bits(d['Mexp'][f].numpy())) and np.array_equal(bits(Qexp), bits(d['Qexp'][f].numpy()))
        assert np.array_equal(bsq.astype(np.float64), d['bsq64'][f]) and pres == int(d['m'][f].sum())


def _presence_mask(C, n, eps, seed):
    """[C, n] float32 of values around eps: just below, equal, just above, 0 and 1."""
    e = np.float32(eps)
    vals = torch.tensor([float(np.nextafter(e, np.float32(0))), float(e), float(np.nextafter(e, np.float32(1))), 0.0, 1.0])
    g = torch.Generator().manual_seed(seed)
    return vals[torch.randint(0, 5, (C, n), generator=g)]


@pytest.mark.parametrize('H,W', [(1, 1), (15, 17), (513, 512)])
@pytest.mark.parametrize('C', [1, 2])
def test_presence_is_an_exact_count_of_strictly_greater(H, W, C):
    """H W = 1, 255 and 513 * 512 = 262656 > 1024 blocks x 256 threads: the grid-stride second pass runs."""
    eps = 0.3
    mask = _presence_mask(C, H * W, eps, H + C).view(C, H, W)
    merged = mask.max(0).values.numpy()
    want = int((merged > np.float32(eps)).sum())
    assert H * W < 10 or 0 < int((merged == np.float32(eps)).sum()) and 0 < want < H * W
    key = torch.ones(1, 1, device='cuda')
    mask_d = mask.cuda()
    assert run_prepare(key, key, mask_d, 1, 1, 0.5, eps=eps)[3] == want
    mask_d[:, -1, -1] = 1.0                                       # the last pixel counts
    mask_d[:, 0, 0] = eps                                         # the first does not
    want = int((mask_d.max(0).values.cpu().numpy() > np.float32(eps)).sum())
    assert run_prepare(key, key, mask_d, 1, 1, 0.5, eps=eps)[3] == want
    assert run_prepare(key, key, torch.full_like(mask_d, eps), 1, 1, 0.5, eps=eps)[3] == 0
    assert run_prepare(key, key, torch.ones_like(mask_d), 1, 1, 0.5, eps=eps)[3] == H * W


def _lut(eps, seed):
    g = torch.Generator().manual_seed(seed)
    lut = torch.rand(256, generator=g)
    lut[::5] = float(np.float32(eps))                            # labels whose value equals eps: not counted
    lut[0], lut[255] = 0.0, 1.0
    return lut


@pytest.mark.parametrize('H,W', [(4, 5), (3, 7), (2, 9), (5, 7)])
def test_prepare_u8_at_every_byte_offset_and_length_residue(H, W):
    """H W mod 4 = 0, 1, 2, 3; planes at byte offsets 0 .. 3 of one allocation (offset 0: the four-labels-per-load path and its tail)."""
    eps, h, w, ck, alpha = 0.3, 2, 3, 8, 0.3
    g = torch.Generator().manual_seed(H * W)
    lut = _lut(eps, 1)
    key, sel = torch.randn(h * w, ck, generator=g), torch.rand(h * w, ck, generator=g)
    buf = torch.randint(0, 256, (H * W + 8,), generator=g, dtype=torch.uint8)
    buf_d, lut_d, key_d, sel_d = buf.cuda(), lut.cuda(), key.cuda(), sel.cuda()
    assert buf_d.data_ptr() % 4 == 0
    for off in range(4):
        plane = buf[off:off + H * W].view(H, W)
        plane_d = buf_d[off:off + H * W].view(H, W)
        assert plane_d.data_ptr() % 4 == off and plane_d.is_contiguous()
        ref = S.prepare_ref(key, sel, lut[plane.long()][None], h, w, alpha, eps)
        assert 0 < ref['presence'] < H * W
        check_prepare(run_prepare(key_d, sel_d, plane_d, h, w, alpha, eps=eps, lut=lut_d), ref, f'u8 {H}x{W} offset {off}')


@pytest.mark.parametrize('off', [0, 1])
def test_prepare_u8_large_plane_runs_the_second_pass(off):
    """1025 x 1024 labels > 1024 blocks x 256 threads x 4 labels: the vector path (offset 0) and the byte path (offset 1) both stride."""
    H, W, eps, h, w, ck, alpha = 1025, 1024, 0.3, 3, 5, 8, 0.5
    g = torch.Generator().manual_seed(5)
    lut = _lut(eps, 2)
    key, sel = torch.randn(h * w, ck, generator=g), torch.rand(h * w, ck, generator=g)
    buf = torch.randint(0, 256, (H * W + 4,), generator=g, dtype=torch.uint8)
    buf_d = buf.cuda()
    plane, plane_d = buf[off:off + H * W].view(H, W), buf_d[off:off + H * W].view(H, W)
    assert plane_d.data_ptr() % 4 == off
    ref = S.prepare_ref(key, sel, lut[plane.long()][None], h, w, alpha, eps)
    check_prepare(run_prepare(key.cuda(), sel.cuda(), plane_d, h, w, alpha, eps=eps, lut=lut.cuda()), ref, f'u8 1025x1024 offset {off}')
    counted = bool(lut[int(plane[-1, -1])].numpy() > np.float32(eps))
    plane_d[-1, -1] = 0 if counted else 255                        # the very last label flips the count by one (lut[0] = 0, lut[255] = 1)
    delta = -1 if counted else 1
    assert run_prepare(key.cuda(), sel.cuda(), plane_d, h, w, alpha, eps=eps, lut=lut.cuda())[3] == ref['presence'] + delta
