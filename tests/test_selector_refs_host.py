"""tests/selector_refs.py on the CPU: prepare_ref and score_ref against the oracle (composite_keys_and_validity, cycle_dissimilarity),
the exactness premise and the non-vacuity conditions of every exact-regime shape the GPU test runs, and the evidence that the GPU
test's exact comparison of per-tile partials bites: faults injected into a copy of the reference computation must fail it at every
edge shape where the fault can exist at all.  No GPU."""
import numpy as np
import pytest
import torch

import selector_refs as S
from oracle import cpu_ref as R


# ---------------------------------------------------------------------------------------------------------
# the reference against the oracle
# ---------------------------------------------------------------------------------------------------------
def _against_oracle(regime, h, w, H, W, C, alpha, seed, eps=0.5):
    """Frames drawn by make_inputs, masks [C, H, W] at full resolution: (prepare_ref o score_ref, the oracle) on the same inputs."""
    nf, hw = 3, h * w
    d = S.make_inputs(regime, nf, hw, seed, alpha=alpha, vacuity=False)
    gen = torch.Generator().manual_seed(seed + 100)
    if regime == 'exact':
        masks = [torch.randint(0, 2, (C, H, W), generator=gen).float() for _ in range(nf)]
    else:
        masks = [torch.rand(C, H, W, generator=gen) for _ in range(nf)]
    prep = [S.prepare_ref(d['key'][f], d['sel'][f], masks[f], h, w, alpha, eps) for f in range(nf)]
    grid = lambda rows: rows.t().reshape(-1, h, w).contiguous()                               # [HW, Ck] -> [Ck, h, w]
    keys = [grid(d['key'][f]) for f in range(nf)]
    composite, valid = R.composite_keys_and_validity(keys, masks, (0,), alpha, 0.0, eps)
    assert valid.all()
    for f in range(nf):
        assert np.array_equal(grid(torch.from_numpy(prep[f]['ck'])).numpy().view(np.int32), composite[f].numpy().view(np.int32)), 'composite key'
        assert prep[f]['presence'] == int((masks[f].max(0).values > eps).sum())
    Mexp, Qexp = np.stack([p['Mexp'] for p in prep]), np.stack([p['Qexp'] for p in prep])
    bsq = np.stack([p['bsq'] for p in prep]).astype(np.float32)
    out = []
    for c in range(nf):
        tiles, scores = S.score_ref(Mexp, Qexp, bsq, d['shr'], c)
        _, bound = S.score_tile_bound(Mexp, Qexp, bsq, d['shr'], c)
        oracle = [float(R.cycle_dissimilarity(composite[c], d['shr'][c].view(1, h, w), grid(d['sel'][c]),
                                              composite[f], d['shr'][f].view(1, h, w), grid(d['sel'][f]))) for f in range(nf)]
        out.append((tiles, scores, bound, np.asarray(oracle, np.float64)))
    return out


@pytest.mark.parametrize('h,w,H,W,C,alpha', [(2, 4, 5, 9, 1, 0.5), (4, 4, 8, 8, 2, 1.0), (4, 8, 12, 20, 3, 0.0), (4, 8, 3, 5, 2, 0.5)])
def test_reference_equals_the_oracle_in_the_exact_regime(h, w, H, W, C, alpha):
    """HW^2 is a power of two and sum terms 2^Q < 2^24, so the oracle's fp32 sum and its division are exact in any order."""
    for tiles, scores, _, oracle in _against_oracle('exact', h, w, H, W, C, alpha, seed=7):
        assert tiles.sum() * 2.0 ** S.Q_BITS < 2.0 ** 24 and scores.max() > 0
        assert np.array_equal(scores, oracle)


@pytest.mark.parametrize('h,w,H,W,C,alpha', [(2, 3, 5, 7, 1, 0.3), (5, 7, 40, 33, 2, 0.5), (6, 8, 96, 128, 3, 0.7), (3, 3, 10, 10, 1, 1.0)])
def test_reference_bounds_the_fp32_oracle_in_the_dense_regime(h, w, H, W, C, alpha):
    worst = 0.0
    for c, (tiles, scores, bound, oracle) in enumerate(_against_oracle('dense', h, w, H, W, C, alpha, seed=9)):
        assert scores[c] == 0.0 and oracle[c] == 0.0 and bound[c] >= 0
        err = np.abs(oracle - scores)
        assert np.all(err <= bound), (err, bound)
        worst = max(worst, float((err[err > 0] / bound[err > 0]).max()))
    print(f'oracle fp32 vs score_ref: max err/bound {worst:.3f}')


def test_prepare_ref_without_a_mask_keeps_the_key_bits():
    d = S.make_inputs('dense', 1, 35, 3)
    p = S.prepare_ref(d['key'][0], d['sel'][0], None, 5, 7, 0.3)
    k, e = d['key'][0].numpy(), d['sel'][0].numpy()
    assert np.array_equal(p['Mexp'][:, 64:].view(np.int32), k.view(np.int32)) and p['presence'] == 0
    assert np.array_equal(p['Mexp'][:, :64], k * k) and np.array_equal(p['Qexp'][:, :64], -e) and np.array_equal(p['Qexp'][:, 64:], 2 * (k * e))
    assert np.all(np.abs(p['bsq'] - (e * k * k).sum(1)) <= p['bsq_bound'])


def test_presence_is_strictly_greater_than_eps():
    eps = np.float32(0.3)
    m = torch.tensor([[[float(np.nextafter(eps, np.float32(0))), float(eps)], [float(np.nextafter(eps, np.float32(1))), 0.0]],
                      [[0.0, float(eps)], [0.0, 1.0]]])
    p = S.prepare_ref(torch.zeros(1, 4), torch.zeros(1, 4), m, 1, 1, 0.5, eps=0.3)
    assert p['presence'] == 2


@pytest.mark.parametrize('hw', [1, 33, 129, 257])
def test_tiles_add_up_and_the_chosen_frame_scores_zero(hw):
    for regime in ('exact', 'dense'):
        d = S.edge_case(hw) if regime == 'exact' else S.make_inputs('dense', 3, hw, 4, alpha=0.3)
        t = S.n_tiles(hw)
        for c in range(3):
            tiles, scores = d['tiles'][c], d['scores'][c]
            assert tiles.shape == (3, t, t) and scores[c] == 0.0 and not tiles[c].any()
            for f in range(3):
                whole = S.pair_terms(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], c, f)
                assert whole.shape == (hw, hw)
                assert np.isclose(tiles[f].sum(), whole.sum(), rtol=1e-12, atol=0) and np.isclose(scores[f], whole.mean(), rtol=1e-12, atol=0)
                if regime == 'exact':
                    assert tiles[f].sum() == whole.sum()
                assert np.isclose(tiles[f][-1, -1], whole[(t - 1) * S.TILE:, (t - 1) * S.TILE:].sum(), rtol=1e-12, atol=0)
                assert np.isclose(tiles[f][0, -1], whole[:S.TILE, (t - 1) * S.TILE:].sum(), rtol=1e-12, atol=0)      # row tile major
        v = np.array([1, 0, 1], np.uint8)
        tiles, scores = S.score_ref(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], 0, v)
        assert not tiles[1].any() and scores[1] == 0.0 and np.array_equal(tiles[2], d['tiles'][0][2])


# ---------------------------------------------------------------------------------------------------------
# the exact regime's premise and the non-vacuity conditions, for every shape the GPU test uses
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', S.EDGE_HW + (2049,))
def test_exact_edge_cases_are_exact_and_not_vacuous(hw):
    d = S.edge_case(hw)
    assert S.is_exact_regime(d)
    unit, bits = S.exact_bits(d)
    assert unit and bits < 24.0
    lo, hi = S.assert_not_vacuous(d)
    print(f'HW={hw}: {bits:.1f} bits, share of positive terms {lo:.2f} .. {hi:.2f}')
    if hw <= 129:
        # the fp32 evaluation in the expanded GEMM form, forwards and reversed over k, equals the float64 reference
        Mx, Qx, b, s = (d[k].numpy() for k in ('Mexp', 'Qexp', 'bsq', 'shr'))
        for c, f in ((0, 1), (2, 0)):
            for order in (slice(None), slice(None, None, -1)):
                vf = ((Mx[c][:, order] @ Qx[f][:, order].T - b[f][None, :]) * s[c][:, None]) / np.float32(8)
                vr = ((Mx[f][:, order] @ Qx[c][:, order].T - b[c][None, :]) * s[f][:, None]) / np.float32(8)
                got = np.maximum(vf - vr, np.float32(0))
                assert got.dtype == np.float32
                assert np.array_equal(got.astype(np.float64), S.pair_terms(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], c, f))


def test_alpha_one_quarter_is_outside_the_exact_regime():
    """ck becomes a multiple of 1/8 and the terms multiples of 2^-12, not of 2^-Q_BITS: the premise check refuses the data."""
    with pytest.raises(AssertionError):
        S.make_inputs('exact', 3, 33, 1, alpha=0.25)
    d = dict(S.edge_case(33))
    d['alpha'] = 0.25
    p = [S.prepare_ref(d['key'][f], d['sel'][f], d['m'][f].view(1, 33, 1), 33, 1, 0.25) for f in range(3)]
    d['Mexp'], d['Qexp'] = (torch.from_numpy(np.stack([q[k] for q in p])) for k in ('Mexp', 'Qexp'))
    d['bsq64'] = np.stack([q['bsq'] for q in p])
    d['bsq'] = torch.from_numpy(d['bsq64'].astype(np.float32))
    assert not S.exact_bits(d)[0] and not S.is_exact_regime(d)


# ---------------------------------------------------------------------------------------------------------
# faults the exact comparison of tiles must catch
# ---------------------------------------------------------------------------------------------------------
def _copy(d, c, f, fault=None):
    """A copy of the reference computation (pair_terms, tile_sums) with one fault of a kernel injected.  Returns (terms, tiles)."""
    Mx, Qx, b, s = (np.asarray(d[k], np.float64) for k in ('Mexp', 'Qexp', 'bsq', 'shr'))
    hw = Mx.shape[1]
    MA, QA, bA, sA, MB, QB, bB, sB = Mx[c], Qx[c], b[c], s[c], Mx[f], Qx[f], b[f], s[f]
    if fault == 'sA and sB exchanged':
        sA, sB = sB, sA
    if fault == 'bsqA and bsqB exchanged':
        bA, bB = bB, bA
    dot_f, dot_r = MA @ QB.T, MB @ QA.T
    if fault == 'a 32x32 sub-block transposed':                   # the accumulator of rows 0..31 x columns 0..31 of the forward chain
        n = min(hw, 32)
        dot_f[:n, :n] = dot_f[:n, :n].T.copy()
    if fault == 'k-halves crossed':                               # float4 pair 0: k 0..3 of one operand against k 4..7 of the other
        dot_f += MA[:, 0:4] @ QB[:, 4:8].T + MA[:, 4:8] @ QB[:, 0:4].T - MA[:, 0:8] @ QB[:, 0:8].T
    terms = np.maximum((dot_f - bB[None, :]) * sA[:, None] / 8.0 - (dot_r - bA[None, :]) * sB[:, None] / 8.0, 0.0)
    if fault == 'last row masked':
        terms[hw - 1, :] = 0.0
    if fault == 'last column masked':
        terms[:, hw - 1] = 0.0
    if fault == 'wave blocks swapped inside a tile':
        terms[0:64, 0:64], terms[0:64, 64:128] = terms[0:64, 64:128].copy(), terms[0:64, 0:64].copy()
    if fault == 'wave blocks swapped across a tile edge':
        terms[0:64, 64:128], terms[0:64, 128:192] = terms[0:64, 128:192].copy(), terms[0:64, 64:128].copy()
    tiles = S.tile_sums(terms)
    if fault == 'one row past HW' and hw % S.TILE:                              # row HW of the last row of tiles, read from the clamped row HW-1
        tiles[-1, :] += S.tile_sums(np.where(np.arange(hw)[:, None] == hw - 1, terms, 0.0))[-1, :]
    if fault == 'one column past HW' and hw % S.TILE:
        tiles[:, -1] += S.tile_sums(np.where(np.arange(hw)[None, :] == hw - 1, terms, 0.0))[:, -1]
    if fault == 'a wave block twice, its neighbour dropped':
        tiles[0, 0] += terms[0:64, 0:64].sum() - terms[0:64, 64:128].sum()
    return terms, tiles


# fault -> the shapes at which a kernel can have it at all (elsewhere the injected fault must leave the tiles unchanged)
FAULTS = {
    'last row masked': lambda hw: True,
    'last column masked': lambda hw: True,
    'one row past HW': lambda hw: hw % S.TILE != 0,               # HW a multiple of the tile: the grid has no row past HW
    'one column past HW': lambda hw: hw % S.TILE != 0,
    'sA and sB exchanged': lambda hw: True,
    'bsqA and bsqB exchanged': lambda hw: True,
    'a 32x32 sub-block transposed': lambda hw: hw > 1,            # 1 x 1: its own transpose
    'k-halves crossed': lambda hw: True,
    'a wave block twice, its neighbour dropped': lambda hw: True,  # HW <= 64: the neighbour is empty, the tile doubles
}


def _all_pairs(d, fault):
    nf = d['Mexp'].shape[0]
    return [(c, f) + _copy(d, c, f, fault) for c in range(nf) for f in range(nf) if f != c]


@pytest.mark.parametrize('hw', S.EDGE_HW)
def test_injected_faults_fail_the_exact_tile_comparison(hw):
    d = S.edge_case(hw)
    for c, f, terms, tiles in _all_pairs(d, None):
        assert np.array_equal(terms, S.pair_terms(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], c, f)) and np.array_equal(tiles, d['tiles'][c][f])
    for fault, applies in FAULTS.items():
        same = all(np.array_equal(tiles, d['tiles'][c][f]) for c, f, _, tiles in _all_pairs(d, fault))
        if applies(hw):
            assert not same, f'HW={hw}: "{fault}" passes the exact comparison of tiles'
        else:
            assert same, f'HW={hw}: "{fault}" cannot exist at this shape, yet the copy changed'


@pytest.mark.parametrize('hw', [128, 129, 257])
def test_swapped_wave_blocks_show_in_the_tiles_only_across_a_tile_edge(hw):
    """Both 64x64 blocks full.  The total, hence the score, never sees a swap; the element-level statement always does; the tiles do
    exactly when the two blocks lie in different tiles."""
    d = S.edge_case(hw)
    faults = ['wave blocks swapped inside a tile'] + (['wave blocks swapped across a tile edge'] if hw >= 192 else [])
    for fault in faults:
        for c, f, terms, tiles in _all_pairs(d, fault):
            ref_terms = S.pair_terms(d['Mexp'], d['Qexp'], d['bsq'], d['shr'], c, f)
            assert tiles.sum() / (hw * hw) == d['scores'][c][f], 'the score-level check sees a swap'
            assert not np.array_equal(terms, ref_terms)
            assert np.array_equal(tiles, d['tiles'][c][f]) == (fault == 'wave blocks swapped inside a tile')
