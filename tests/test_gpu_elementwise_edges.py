"""Edge-shape parity of the frame-loop elementwise kernels (csrc/elementwise.hip) against the float64 references and a-priori bounds
of tests/elementwise_refs.py: 1 x 1 and 1 x n maps, channel counts off the tiles, object broadcast, strided channel slices, every
storage combination, saturated gates and probabilities, more than 8 objects, NULL optional outputs, refusals, and one case per
grid-stride kernel that takes the loop's second trip.

Every case is launched through the C ABI (strides, offsets, NULL outputs and status codes are not expressible through ops.*;
test_ops_surface runs a slice through the wrappers).  Per case:
  - every output buffer is filled with the sentinel -777 (exact as a half) and carries 8 spare elements: nothing outside the documented
    destination may change - padding channels, columns outside the slice, rows past the last pixel;
  - inputs hold the finite junk value 7 outside their slices, CBAM's workspace is followed by 4096 bytes of 0xFF that must survive;
  - exact operations must EQUAL the float64 value (rounded once to half for a half destination), the others stay within the bound
    (err / bound <= 1); a refused call writes nothing.
Run with -s for the table (profiles/r15_elementwise_edge_tests.txt is one run)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import elementwise_refs as R

pytestmark = pytest.mark.gpu
SENTINEL, JUNK = R.SENTINEL, R.JUNK
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3          # xmem_status (include/xmem_hip.h)
TAIL = 8                                                     # spare sentinel elements behind every output


@pytest.fixture(scope='module')
def lib():
    from xmem2_amd import _lib
    return _lib.load()


def show(name, worst, n):
    print(f'\nelemedge | {name:<58s} | {n:4d} cases | max err/bound {worst:.3f}')


def stream():
    from xmem2_amd import _lib
    return _lib.stream_ptr()


def sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a device fault: nothing more may run on this GPU from this process
        pytest.exit(f'GPU fault at {what}: {e}', returncode=3)


def dt(half):
    return torch.float16 if half else torch.float32


class Buf:
    """A device buffer of `rows` pixels with pixel stride ld, the operand at columns off : off + C; `fill` everywhere else."""

    def __init__(self, rows, C_, half=0, ld=None, off=0, fill=SENTINEL, data=None, dtype=None):
        self.rows, self.C, self.ld, self.off = rows, C_, ld or C_, off
        dtype = dtype or dt(half)
        host = torch.full((rows * self.ld + TAIL,), fill, dtype=dtype)
        if data is not None:
            host[:rows * self.ld].view(rows, self.ld)[:, off:off + C_] = data.reshape(rows, C_).to(dtype)
        self.t = host.cuda()
        self.fill = fill

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.off * self.t.element_size())

    def read(self, what, written=True):
        """The operand as float64 [rows, C] after checking that everything around it still holds the fill value."""
        flat = self.t.cpu().double()
        keep = torch.ones_like(flat, dtype=torch.bool)
        if written:
            keep[:self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.C] = False
        assert bool((flat[keep] == self.fill).all()), f'{what}: wrote outside its destination' if written else f'{what}: a refused call wrote to the output'
        return flat[:self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.C]


def src(t, half=0, ld=None, off=0):
    t = torch.as_tensor(t)
    Cc = t.shape[-1]
    return Buf(t.numel() // Cc, Cc, half, ld, off, fill=JUNK, data=t)


def hold(what, got, ref, bound, fails):
    """err / bound of one case (0 for an exact match); appends a description of a miss to `fails` (the grid goes on)."""
    got, ref = got.reshape(ref.shape).double(), ref.double()
    if bound is None:
        if not bool((got == ref).all()):
            fails.append(f'{what}: {int((got != ref).sum())} of {ref.numel()} elements differ from the exact result, max |diff| {float((got - ref).abs().max()):.3e}')
        return 0.0
    err = (got - ref).abs()
    if not bool(torch.isfinite(got).all()):
        fails.append(f'{what}: non-finite output')
        return float('inf')
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    worst = float(ratio.max())
    if worst > 1.0:
        k = int(ratio.argmax())
        fails.append(f'{what}: err/bound {worst:.3f} (err {float(err.flatten()[k]):.3e}, ref {float(ref.flatten()[k]):.6e}, element {k})')
    return worst


def hold_sum(what, got, K, fails):
    """|sum over classes - 1| / ((K + 2) u) of probability planes got [K+1][...]"""
    r = float((got.double().sum(0) - 1.0).abs().max()) / R.sum_to_one_bound(K)
    if r > 1.0:
        fails.append(f'{what}: |sum over classes - 1| = {r:.2f} x (K + 2) u')
    return r


def finish(name, fails, worst, n, extra=''):
    show(name + extra, worst, n)
    assert not fails, f'{len(fails)} failures:\n' + '\n'.join(fails[:40])


# ---------------------------------------------------------------------------------------------------------
# one launcher per operation: case + inputs -> (status, output float64 in the reference's shape)
# ---------------------------------------------------------------------------------------------------------
def run_maxpool(lib, c, i):
    B, H, W, Cc = i['x'].shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, out = src(i['x'], c['in_half']), Buf(B * Ho * Wo, Cc, c['out_half'])
    rc = lib.xmem_maxpool3x3s2_t(x.ptr, c['in_half'], out.ptr, c['out_half'], B, H, W, Cc, stream())
    return rc, out


def run_upsample(lib, c, i):
    B, h, w, Cc = i['g'].shape
    g, skip, out = src(i['g'], c['half']), src(i['skip'], c['half']), Buf(B * 4 * h * w, Cc, c['half'])
    rc = lib.xmem_upsample2x_add_t(g.ptr, skip.ptr, out.ptr, c['half'], B, h, w, Cc, stream())
    return rc, out


def run_area(lib, c, i):
    B, H, W, Cc = i['x'].shape
    r = c['r']
    x = src(i['x'], c['in_half'], c['ldin'], c['in_off'])
    out = Buf(B * (H // r) * (W // r), Cc, c['out_half'], c['ldout'], c['out_off'])
    rc = lib.xmem_area_downsample_t(x.ptr, c['in_half'], c['ldin'], out.ptr, c['out_half'], c['ldout'], B, H, W, Cc, r, stream())
    return rc, out


def run_copy(lib, c, i, C_=None, ldsrc=None, lddst=None, skew=0):
    s = src(i['src'], c['in_half'], c['ldsrc'], c['src_off'])
    out = Buf(c['B'] * c['P'], c['C'], c['out_half'], c['lddst'], c['dst_off'])
    rc = lib.xmem_copy_channels_t(C.c_void_p(s.ptr.value + skew), c['in_half'], ldsrc or c['ldsrc'], c['srcB'], out.ptr, c['out_half'],
                                  lddst or c['lddst'], c['B'], c['P'], C_ or c['C'], stream())
    return rc, out


def run_hidden(lib, c, i):
    K, h, w = c['K'], c['h'], c['w']
    tot = c['c16'] + c['c8'] + c['c4'] + 1
    ins = [src(i[k]) for k in ('g16', 'g8', 'g4')] + [src(i['logits'][..., None])]
    out = Buf(K * h * w, tot, 0, c['ldout'])
    rc = lib.xmem_hidden_update_gather(ins[0].ptr, c['c16'], ins[1].ptr, c['c8'], ins[2].ptr, c['c4'], ins[3].ptr, out.ptr, c['ldout'], K, h, w,
                                       stream())
    # the four-launch composition the header promises the same bits as
    two = Buf(K * h * w, tot, 0, c['ldout'])
    at = lambda off: C.c_void_p(two.t.data_ptr() + 4 * off)
    assert lib.xmem_copy_channels(ins[0].ptr, c['c16'], K, at(0), c['ldout'], K, h * w, c['c16'], stream()) == OK
    assert lib.xmem_area_downsample(ins[1].ptr, c['c8'], at(c['c16']), c['ldout'], K, 2 * h, 2 * w, c['c8'], 2, stream()) == OK
    assert lib.xmem_area_downsample(ins[2].ptr, c['c4'], at(c['c16'] + c['c8']), c['ldout'], K, 4 * h, 4 * w, c['c4'], 4, stream()) == OK
    assert lib.xmem_area_downsample(ins[3].ptr, 1, at(tot - 1), c['ldout'], K, 4 * h, 4 * w, 1, 4, stream()) == OK
    sync(R.tag(c))
    assert torch.equal(out.t, two.t), f'{R.tag(c)}: not the bits of copy_channels + three area_downsample calls'
    return rc, out


_cbam_w = {}


def cbam_dev_weights(i, Cc):
    if Cc not in _cbam_w:
        _cbam_w[Cc] = {k: i[k].contiguous().cuda() for k in ('w1', 'b1', 'w2', 'b2', 'sw', 'sb')}
    return _cbam_w[Cc]


def run_cbam(lib, c, i, short=0, skew=0):
    from xmem2_amd import _lib
    B, H, W, Cc = i['g'].shape
    w = cbam_dev_weights(i, Cc)
    g, out = src(i['g'], c['half']), Buf(B * H * W, Cc, c['half'])
    need = lib.xmem_cbam_workspace_bytes(B, H * W, Cc)
    ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device='cuda')
    rc = lib.xmem_cbam_residual_t(C.c_void_p(g.ptr.value + skew), out.ptr, c['half'], B, H, W, Cc, *(_lib.ptr(w[k]) for k in ('w1', 'b1', 'w2', 'b2', 'sw', 'sb')),
                                  _lib.ptr(ws), need - short, stream())
    sync(R.tag(c))
    assert bool((ws[need - short:] == 0xFF).all()), f'{R.tag(c)}: the kernels wrote past the {need} workspace bytes the library asked for'
    return rc, out


def run_gru(lib, c, i):
    N, Ch = i['h'].shape
    v = src(i['values'], c['half'])
    h = Buf(N, Ch, 0, fill=SENTINEL, data=i['h'])
    out = h if c['inplace'] else Buf(N, Ch, 0)
    rc = lib.xmem_gru_gate_t(v.ptr, c['half'], h.ptr, out.ptr, 1, N, Ch, stream())
    return rc, out


def run_logits(lib, c, i):
    K, h4, w4 = i['logits'].shape
    lg = src(i['logits'].reshape(-1, 1))
    prob = Buf(K + 1, c['H'] * c['W'])
    pad = Buf(K + 1, 16 * h4 * w4) if c['padded'] else None
    rc = lib.xmem_logits_to_prob(lg.ptr, prob.ptr, pad.ptr if pad else None, K, h4, w4, c['H'], c['W'], c['lh'], c['lw'], stream())
    return rc, prob, pad


def run_aggregate(lib, c, i):
    m = src(i['masks'].reshape(-1, 1))
    out = Buf(c['K'] + 1, c['H'] * c['W'])
    return lib.xmem_aggregate_masks(m.ptr, out.ptr, c['K'], c['H'], c['W'], stream()), out


def run_resize(lib, c, i):
    x, out = src(i['x'].reshape(-1, 1)), Buf(c['C'], c['Ho'] * c['Wo'])
    return lib.xmem_resize_bilinear(x.ptr, out.ptr, c['C'], c['Hi'], c['Wi'], c['Ho'], c['Wo'], stream()), out


def run_merge(lib, c, i):
    p, m, out = src(i['pred'].reshape(-1, 1)), src(i['mask'].reshape(-1, 1)), Buf(c['K'], c['H'] * c['W'])
    return lib.xmem_merge_masks(p.ptr, m.ptr, C.c_uint64(c['valid_bits']), out.ptr, c['K'], c['H'], c['W'], stream()), out


def run_argmax(lib, c, i):
    p = src(i['prob'].reshape(-1, 1))
    out = Buf(1, c['P'], dtype=torch.uint8, fill=0xAB)
    return lib.xmem_argmax_u8(p.ptr, out.ptr, c['C'], 1, c['P'], stream()), out


RUN = dict(maxpool=run_maxpool, upsample2x_add=run_upsample, area_downsample=run_area, copy_channels=run_copy, hidden_update_gather=run_hidden,
           cbam_residual=run_cbam, gru_gate=run_gru, aggregate_masks=run_aggregate, resize_bilinear=run_resize, merge_masks=run_merge,
           argmax_u8=run_argmax)


def run_grid(lib, op, cases=None):
    """Every case of the operation's grid against its reference; returns (failures, worst err/bound, cases, note): the note splits
    the worst figure by the destination's storage type where the grid has both (one rounding to half may use all of its 2^-11 |ref|)."""
    fails, n, by = [], 0, {}
    for c in (cases if cases is not None else R.CASES[op]()):
        i = R.make_inputs(c)
        ref, bound = R.reference(c, i)
        rc, out = RUN[op](lib, c, i)
        sync(R.tag(c))
        n += 1
        if rc != OK:
            fails.append(f'{R.tag(c)}: status {rc}')
            continue
        kind = 'half' if c.get('out_half', c.get('half', 0)) and op != 'gru_gate' else 'fp32'
        by[kind] = max(by.get(kind, 0.0), hold(R.tag(c), out.read(R.tag(c)), ref, bound, fails))
    note = f" (fp32 destination {by['fp32']:.3f}, half {by['half']:.3f})" if len(by) == 2 and max(by.values()) > 0 else ''
    return fails, max(by.values(), default=0.0), n, note


# ---------------------------------------------------------------------------------------------------------
# the grids
# ---------------------------------------------------------------------------------------------------------
def test_maxpool_edges(lib):
    """1 x 1, 1 x n, 2 x 2, even / odd maps, C = 4 / 8 / 68, all-negative data (the padding is -inf, not 0), four storage
    combinations: exact (the clamped taps repeat an in-range neighbour of the same window on every one of these maps)."""
    finish('maxpool3x3s2_t', *run_grid(lib, 'maxpool'))


def test_upsample2x_add_edges(lib):
    """From 1 x 1 / 1 x n / n x 1 maps, the skip shared by all B images, fp32 and half."""
    finish('upsample2x_add_t', *run_grid(lib, 'upsample2x_add'))


def test_area_downsample_edges(lib):
    """r = 1 / 2 / 4 on one and on 2 x 3 windows, C = 1 / 3 / 36, ldin > C with an input offset, ldout > C with an output offset,
    four storage combinations; H % r != 0 is refused with the output untouched."""
    fails, w, n, note = run_grid(lib, 'area_downsample')
    for c in (R.case('area_downsample', B=1, H=5, W=4, C=3, r=2, in_half=0, out_half=0, ldin=3, in_off=0, ldout=3, out_off=0),
              R.case('area_downsample', B=1, H=4, W=6, C=3, r=4, in_half=0, out_half=1, ldin=3, in_off=0, ldout=3, out_off=0)):
        i = R.make_inputs(c)
        x = src(i['x'], c['in_half'])
        out = Buf((c['H'] // c['r']) * (c['W'] // c['r']), 3, c['out_half'])
        rc = lib.xmem_area_downsample_t(x.ptr, c['in_half'], 3, out.ptr, c['out_half'], 3, 1, c['H'], c['W'], 3, c['r'], stream())
        sync(R.tag(c))
        assert rc == UNSUPPORTED, (R.tag(c), rc)
        out.read(R.tag(c), written=False)
        n += 1
    finish('area_downsample_t', fails, w, n, note)


def test_copy_channels_edges(lib):
    """(srcB, B) = (1, 1), (1, 3), (3, 3), (2, 4) (b % srcB with 1 < srcB < B), both strides wider than C, four storage combinations:
    exact, fp32 -> half rounds once.  C % 4, ld % 4 and a pointer off its alignment are refused with nothing written."""
    fails, w, n, note = run_grid(lib, 'copy_channels')
    c = next(R.copy_cases())
    i = R.make_inputs(c)
    for kw in (dict(C_=3), dict(ldsrc=c['ldsrc'] + 2), dict(lddst=c['lddst'] + 1), dict(skew=4)):
        rc, out = run_copy(lib, c, i, **kw)
        sync(f'copy_channels refusal {kw}')
        assert rc == UNSUPPORTED, (kw, rc)
        out.read(f'copy_channels refusal {kw}', written=False)
        n += 1
    finish('copy_channels_t', fails, w, n, note)


def test_hidden_update_gather_edges(lib):
    """(K, h, w) = (1, 1, 1) and (3, 2, 3), two channel splits, 3 and 7 spare channels behind c16 + c8 + c4 + 1 (untouched): within the
    float64 bound and still the bits of the four-launch composition."""
    finish('hidden_update_gather', *run_grid(lib, 'hidden_update_gather'))


def test_cbam_edges(lib):
    """P = 1, 6, 16, 17, 17, 35 (empty pooling splits, P % 16 != 0, maps narrower than the 7 x 7 gate), C = 16, 48 (Cr = 3: scalar w2
    path, partial pooling workgroup), 64, 528 (Cr = 33: second pass of the hidden-unit loop), B = 1 / 3, all-negative features,
    fp32 and half.  A workspace one byte short -> WORKSPACE, C % 16 -> UNSUPPORTED, a pointer off the vector alignment ->
    UNSUPPORTED; none of them launches or writes."""
    fails, w, n, note = run_grid(lib, 'cbam_residual')
    c = R.case('cbam_residual', B=1, H=2, W=3, C=48, data='randn', half=0)
    i = R.make_inputs(c)
    for kw, want in ((dict(short=1), WORKSPACE), (dict(skew=4), UNSUPPORTED)):
        rc, out = run_cbam(lib, c, i, **kw)
        assert rc == want, (kw, rc)
        out.read(f'cbam refusal {kw}', written=False)
        n += 1
    g, out = src(torch.zeros(1, 1, 2, 24)), Buf(2, 24)
    ws = torch.full((1 << 16,), 0xFF, dtype=torch.uint8, device='cuda')
    from xmem2_amd import _lib
    wd = cbam_dev_weights(i, 48)
    rc = lib.xmem_cbam_residual_t(g.ptr, out.ptr, 0, 1, 1, 2, 24, *(_lib.ptr(wd[k]) for k in ('w1', 'b1', 'w2', 'b2', 'sw', 'sb')), _lib.ptr(ws), 1 << 16, stream())
    sync('cbam C % 16')
    assert rc == UNSUPPORTED, rc
    out.read('cbam C % 16', written=False)
    assert bool((ws == 0xFF).all())
    finish('cbam_residual_t', fails, w, n + 1, note)


def test_gru_gate_edges(lib):
    """Ch = 1 / 3 / 64, B P = 1 / 35, out of place and new_h == h, ordinary values and gates at +-30 / +-100 (finite, within the
    bound: the 1 - u of a saturated update gate is held to the absolute term of the 1 + exp(-x) form), half values."""
    finish('gru_gate_t', *run_grid(lib, 'gru_gate'))


def test_add3_and_packing(lib):
    """add3 at n = 1 / 255 / 257; pack_image without padding and with all of it on one side; pack_value_input at K = 1 / 12 on 0 / 1
    masks (exact, the zero 4th / 6th-8th channels included)."""
    fails, worst, n = [], 0.0, 0
    g = R.rng_of('add3')
    for m in (1, 255, 257):
        a, b, c3 = (R.randn(g, m, 1) for _ in range(3))
        A, B_, C3, out = src(a), src(b), src(c3), Buf(1, m)
        assert lib.xmem_add3(A.ptr, B_.ptr, C3.ptr, out.ptr, m, stream()) == OK
        sync(f'add3 n={m}')
        worst = max(worst, hold(f'add3 n={m}', out.read(f'add3 n={m}'), *R.add3_ref(a, b, c3), fails))
        n += 1
    img = R.randn(g, 3, 5, 6)
    for Hp, Wp, lh, lw in ((5, 6, 0, 0), (16, 16, 11, 10), (16, 16, 0, 0)):
        what = f'pack_image {Hp}x{Wp} lh={lh} lw={lw}'
        x, out = src(img.reshape(-1, 1)), Buf(Hp * Wp, 4)
        assert lib.xmem_pack_image(x.ptr, out.ptr, 5, 6, Hp, Wp, lh, lw, stream()) == OK
        sync(what)
        hold(what, out.read(what), R.pack_image_ref(img, Hp, Wp, lh, lw)[0], None, fails)
        n += 1
    for K in (1, 12):
        what = f'pack_value_input K={K}'
        masks, im4 = (torch.rand(K, 4, 8, generator=g) < 0.4).float(), R.randn(g, 4, 8, 4)
        m, x, out = src(masks.reshape(-1, 1)), src(im4), Buf(K * 32, 8)
        assert lib.xmem_pack_value_input(x.ptr, m.ptr, out.ptr, K, 4, 8, stream()) == OK
        sync(what)
        hold(what, out.read(what), R.pack_value_input_ref(im4, masks)[0], None, fails)
        n += 1
    finish('add3, pack_image, pack_value_input', fails, worst, n)


def test_key_post_edges(lib):
    """Ck = 1 / 64, P = 1 / 37, ldp = 2 Ck + 1 and wider, shrinkage / selection NULL one at a time and together, e at +-100.  The key
    part is exact."""
    fails, worst, n = [], 0.0, 0
    for Ck, P, spare, want_s, want_e in ((a, b, s, ws, we) for a in (1, 64) for b in (1, 37) for s in (0, 7) for ws in (0, 1) for we in (0, 1)):
        what = f'key_post Ck={Ck} P={P} ldp={2 * Ck + 1 + spare} shrinkage={want_s} selection={want_e}'
        g = R.rng_of('key_post', Ck, P)
        proj = R.randn(g, P, 2 * Ck + 1)
        proj[0, Ck + 1] = 100.0
        proj[P - 1, 2 * Ck] = -100.0 if Ck > 1 or P > 1 else 100.0
        x = src(proj, 0, 2 * Ck + 1 + spare)
        key, shr, sel = Buf(P, Ck), Buf(P, 1), Buf(P, Ck)
        rc = lib.xmem_key_post(x.ptr, x.ld, key.ptr, shr.ptr if want_s else None, sel.ptr if want_e else None, P, Ck, stream())
        sync(what)
        assert rc == OK, (what, rc)
        (rk, _), (rs, bs), (re, be) = R.key_post_ref(proj, Ck)
        hold(what + ' key', key.read(what), rk, None, fails)
        got_s, got_e = shr.read(what, written=bool(want_s)), sel.read(what, written=bool(want_e))
        if want_s:
            worst = max(worst, hold(what + ' shrinkage', got_s, rs, bs, fails))
        if want_e:
            worst = max(worst, hold(what + ' selection', got_e, re, be, fails))
        n += 1
    finish('key_post', fails, worst, n)


def check_probabilities(what, K, out, ref, bound, fails):
    got = out.read(what)
    return hold(what, got, ref.reshape(K + 1, -1), bound.reshape(K + 1, -1), fails), hold_sum(what, got, K, fails)


def test_logits_to_prob_edges(lib):
    """K = 1 / 8 / 9 / 12 on 1 x 1 ... 5 x 7 maps, cropped and uncropped, prob_padded NULL and given, logits randn * 4, saturated at
    +-40, and mixtures where one object and the background both saturate: within the conditioning bound AND |sum - 1| <= (K + 2) u,
    which holds only if every numerator is the value the denominator summed.  Objects 9, 10, ... are recomputed in the kernel's
    passes 2 and 3 (KREG = 8); an object moved from slot 0 to slot 10 must stay inside the bound in both places.
    First run on the MI355X, kernel unchanged: all 194 cases inside the bound (largest err/bound 0.652) and |sum - 1| at most
    0.746 (K + 2) u, K = 9 and 12 included - with this compiler the three evaluations of objects 9, 10, ... come out bit-identical,
    so numerator and denominator agree.  Nothing in the source forces that (the kernel's own comment says why), so the kernel was
    left as it is and this assertion is now the guard: a recomputation that drifts by one ulp of a saturated probability moves a
    numerator by ~1e-4 and fails it (tests/test_elementwise_refs_host.py, mutation `numerator_8_recomputed`)."""
    fails, worst, wsum, n = [], 0.0, 0.0, 0
    for c in R.logits_cases():
        i = R.make_inputs(c)
        (ref, bound), (pref, pbound) = R.logits_to_prob_ref(i['logits'], c['H'], c['W'], c['lh'], c['lw'])
        rc, prob, pad = run_logits(lib, c, i)
        sync(R.tag(c))
        assert rc == OK, (R.tag(c), rc)
        for o, r, b in ((prob, ref, bound), (pad, pref, pbound)):
            if o is not None:
                e, s = check_probabilities(R.tag(c), c['K'], o, r, b, fails)
                worst, wsum = max(worst, e), max(wsum, s)
        n += 1
    g = R.rng_of('slots')
    obj, other = R.randn(g, 5, 7) * 4, R.randn(g, 5, 7) * 4
    for slot in (0, 10):
        lg = other[None].repeat(12, 1, 1)
        lg[slot] = obj
        c = R.case('logits_to_prob', K=12, h4=5, w4=7, H=20, W=28, lh=0, lw=0, padded=0, data=f'object in slot {slot}')
        (ref, bound), _ = R.logits_to_prob_ref(lg, 20, 28, 0, 0)
        rc, prob, _ = run_logits(lib, c, dict(logits=lg))
        sync(R.tag(c))
        assert rc == OK
        e, s = check_probabilities(R.tag(c), 12, prob, ref, bound, fails)
        worst, wsum, n = max(worst, e), max(wsum, s), n + 1
    finish('logits_to_prob', fails, worst, n, f' (|sum - 1| / (K + 2) u: {wsum:.3f})')


def test_aggregate_masks_edges(lib):
    """K = 1 / 8 / 9 / 12 on hard 0 / 1 masks, uniform masks and masks where two objects are both 1: the conditioning bound and
    |sum - 1| <= (K + 2) u."""
    fails, worst, wsum, n = [], 0.0, 0.0, 0
    for c in R.aggregate_cases():
        i = R.make_inputs(c)
        ref, bound = R.reference(c, i)
        rc, out = run_aggregate(lib, c, i)
        sync(R.tag(c))
        assert rc == OK
        e, s = check_probabilities(R.tag(c), c['K'], out, ref, bound, fails)
        worst, wsum, n = max(worst, e), max(wsum, s), n + 1
    finish('aggregate_masks', fails, worst, n, f' (|sum - 1| / (K + 2) u: {wsum:.3f})')


def test_merge_resize_argmax_edges(lib):
    """merge_masks at K = 1 / 3 / 64 (bit 63) with no / all / the first / the last label valid and mask sums of exactly 0.5 and just
    above; resize_bilinear up, down, identity and from / to one pixel; argmax_u8 at C = 1 / 2 / 255 with exact ties (first index) and no
    pixel excluded."""
    for op, name in (('merge_masks', 'merge_masks'), ('resize_bilinear', 'resize_bilinear'), ('argmax_u8', 'argmax_u8')):
        finish(name, *run_grid(lib, op))


def test_transposes_edges(lib):
    """(P, C) over {1, 31, 32, 33}^2 (below, at and above the 32 x 32 tile), B = 1 / 3, ld = C and C + 5: exact, columns past C
    untouched (nchw_to_nhwc) or never read (nhwc_to_nchw)."""
    fails, n = [], 0
    for P, Cc, B, spare in ((p, c, b, s) for p in (1, 31, 32, 33) for c in (1, 31, 32, 33) for b in (1, 3) for s in (0, 5)):
        what = f'P={P} C={Cc} B={B} ld={Cc + spare}'
        x = torch.arange(B * P * Cc, dtype=torch.float32).reshape(B, P, Cc) - 100.0
        a, out = src(x, 0, Cc + spare), Buf(B * Cc, P)
        assert lib.xmem_nhwc_to_nchw(a.ptr, Cc + spare, out.ptr, B, P, Cc, stream()) == OK
        sync('nhwc_to_nchw ' + what)
        hold('nhwc_to_nchw ' + what, out.read(what), x.permute(0, 2, 1).double(), None, fails)
        b_, out2 = src(x.permute(0, 2, 1).reshape(-1, 1)), Buf(B * P, Cc, 0, Cc + spare)
        assert lib.xmem_nchw_to_nhwc(b_.ptr, out2.ptr, Cc + spare, B, P, Cc, stream()) == OK
        sync('nchw_to_nhwc ' + what)
        hold('nchw_to_nhwc ' + what, out2.read(what), x.double(), None, fails)
        n += 2
    finish('nhwc_to_nchw, nchw_to_nhwc', fails, 0.0, n)


def test_misaligned_activations_are_refused(lib):
    """maxpool3x3s2_t, upsample2x_add_t and cbam_residual_t read and write 16-byte vectors (8 bytes for halfs): a pointer off that
    alignment is refused on the host (UNSUPPORTED, no launch, nothing written), as copy_channels_t always did."""
    n = 0
    for half in (0, 1):
        skew = 2 if half else 4                       # one element: aligned for a scalar access, not for the vector
        x, out = src(torch.zeros(1, 3, 3, 8), half), Buf(4, 8, half)
        for a, b in ((skew, 0), (0, skew)):
            rc = lib.xmem_maxpool3x3s2_t(C.c_void_p(x.ptr.value + a), half, C.c_void_p(out.ptr.value + b), half, 1, 2, 2, 8, stream())
            assert rc == UNSUPPORTED, ('maxpool', half, a, b, rc)
            n += 1
        g, skip, up = src(torch.zeros(1, 2, 2, 8), half), src(torch.zeros(4, 4, 8), half), Buf(16, 8, half)
        for a, b, d in ((skew, 0, 0), (0, skew, 0), (0, 0, skew)):
            rc = lib.xmem_upsample2x_add_t(C.c_void_p(g.ptr.value + a), C.c_void_p(skip.ptr.value + b), C.c_void_p(up.ptr.value + d), half, 1, 1, 1, 8,
                                           stream())
            assert rc == UNSUPPORTED, ('upsample2x_add', half, a, b, d, rc)
            n += 1
        sync('misaligned refusals')
        out.read('maxpool misaligned', written=False)
        up.read('upsample2x_add misaligned', written=False)
        c = R.case('cbam_residual', B=1, H=1, W=1, C=16, data='randn', half=half)
        rc, o = run_cbam(lib, c, R.make_inputs(c), skew=skew)
        assert rc == UNSUPPORTED, ('cbam', half, rc)
        o.read('cbam misaligned', written=False)
        n += 1
    show('misaligned pointers refused', 0.0, n)


# ---------------------------------------------------------------------------------------------------------
# the second trip of the grid-stride loops
# ---------------------------------------------------------------------------------------------------------
GRID_DOC = """grid_for() in csrc/elementwise.hip caps the grid at 8192 workgroups of 256 threads (R.GRID_CAP, R.GRID_BLOCK, read from the
source), so a kernel with more than 8192 * 256 = 2,097,152 work items takes `e += gridDim.x * blockDim.x`.  One case per kernel that
launches through grid_for, its work-item count just above that; every element is checked.  Exact operations run on small integers
against torch's fp32 result (tests/test_elementwise_refs_host.py ties that to the float64 statement).  No op-level test took that
second trip before; the first run on the MI355X found every kernel correct on it."""
_nchw, _nhwc = (lambda t: t.permute(0, 3, 1, 2)), (lambda t: t.permute(0, 2, 3, 1))


class Trip:
    def __init__(self, seed):
        self.fails, self.worst, self.n = [], 0.0, 0
        self.g = R.rng_of('grid', seed)

    def ints(self, *shape):
        return torch.randint(-8, 9, shape, generator=self.g).float()

    def done(self, what, items, out, ref, bound):
        assert items > R.GRID_ITEMS, (what, items)
        sync(what)
        r = hold(f'{what} ({items} work items)', out.read(what), ref, bound, self.fails)
        print(f'\nelemedge |   {what:<24s} {items:8d} work items, second trip from {R.GRID_ITEMS} | ' + ('exact' if bound is None else f'err/bound {r:.3f}'), end='')
        self.worst, self.n = max(self.worst, r), self.n + 1

    def finish(self, name):
        finish('second grid-stride trip: ' + name, self.fails, self.worst, self.n)


def test_grid_stride_second_trip_decoder_maps(lib):
    t = Trip(0)
    ints, done, nchw, nhwc = t.ints, t.done, _nchw, _nhwc
    x = ints(1, 2900, 2900, 4)                                       # maxpool: B Ho Wo C/4 = 1450^2
    a, out = src(x), Buf(1450 * 1450, 4)
    assert lib.xmem_maxpool3x3s2_t(a.ptr, 0, out.ptr, 0, 1, 2900, 2900, 4, stream()) == OK
    done('maxpool3x3s2', 1450 * 1450, out, nhwc(F.max_pool2d(nchw(x), 3, 2, 1)), None)

    area4 = nhwc(F.avg_pool2d(nchw(x), 4))                           # hidden_update_gather: K h w ((c16 + c8 + c4) / 4 + 1) = 725^2 * 4
    g16, g8, lg = ints(1, 725, 725, 4), ints(1, 1450, 1450, 4), ints(1, 2900, 2900, 1)
    ins, out = [a, src(g16), src(g8), src(lg)], Buf(725 * 725, 13, 0, 16)
    assert lib.xmem_hidden_update_gather(ins[1].ptr, 4, ins[2].ptr, 4, a.ptr, 4, ins[3].ptr, out.ptr, 16, 1, 725, 725, stream()) == OK
    done('hidden_update_gather', 725 * 725 * 4, out, torch.cat([g16, nhwc(F.avg_pool2d(nchw(g8), 2)), area4, nhwc(F.avg_pool2d(nchw(lg), 4))], -1), None)
    del a, ins, x, area4, lg

    skip = ints(1450, 1450, 4)                                       # upsample2x_add: B 4 h w C/4 = 1450^2
    a, b, out = src(g16), src(skip), Buf(1450 * 1450, 4)
    assert lib.xmem_upsample2x_add_t(a.ptr, b.ptr, out.ptr, 0, 1, 725, 725, 4, stream()) == OK
    done('upsample2x_add', 1450 * 1450, out, *R.upsample2x_add_ref(g16, skip))
    t.finish('maxpool, hidden_update_gather, upsample2x_add')


def test_grid_stride_second_trip_channel_kernels(lib):
    t = Trip(1)
    ints, done, nchw, nhwc, g = t.ints, t.done, _nchw, _nhwc, t.g
    x = ints(1, 1674, 1674, 3)                                       # area_downsample: B Ho Wo C = 837^2 * 3
    a, out = src(x), Buf(837 * 837, 3)
    assert lib.xmem_area_downsample_t(a.ptr, 0, 3, out.ptr, 0, 3, 1, 1674, 1674, 3, 2, stream()) == OK
    done('area_downsample', 837 * 837 * 3, out, nhwc(F.avg_pool2d(nchw(x), 2)), None)

    x = ints(1, 525000, 8)                                           # copy_channels: B P C/4 = 2 * 525,000 * 2, srcB = 1
    a, out = src(x), Buf(2 * 525000, 8)
    assert lib.xmem_copy_channels_t(a.ptr, 0, 8, 1, out.ptr, 0, 8, 2, 525000, 8, stream()) == OK
    done('copy_channels', 2 * 525000 * 2, out, x.expand(2, -1, -1), None)

    v, h = R.randn(g, 32813, 192), R.randn(g, 32813, 64)             # gru_gate: B P Ch = 32,813 * 64 = 2,100,032
    a, b, out = src(v), src(h), Buf(32813, 64)
    assert lib.xmem_gru_gate_t(a.ptr, 0, b.ptr, out.ptr, 1, 32813, 64, stream()) == OK
    done('gru_gate', 32813 * 64, out, *R.gru_gate_ref(v, h))

    m = 2100000                                                      # add3: n
    t3 = [ints(m, 1) for _ in range(3)]
    a, b, c3, out = src(t3[0]), src(t3[1]), src(t3[2]), Buf(1, m)
    assert lib.xmem_add3(a.ptr, b.ptr, c3.ptr, out.ptr, m, stream()) == OK
    done('add3', m, out, t3[0] + t3[1] + t3[2], None)

    img = ints(3, 1448, 1449)                                        # pack_image: Hp Wp = 1450^2
    a, out = src(img.reshape(-1, 1)), Buf(1450 * 1450, 4)
    assert lib.xmem_pack_image(a.ptr, out.ptr, 1448, 1449, 1450, 1450, 1, 1, stream()) == OK
    done('pack_image', 1450 * 1450, out, R.pack_image_ref(img, 1450, 1450, 1, 1)[0], None)

    masks, im4 = (torch.rand(2, 1025, 1025, generator=g) < 0.5).float(), ints(1025, 1025, 4)       # pack_value_input: K Hp Wp = 2 * 1025^2
    a, b, out = src(im4), src(masks.reshape(-1, 1)), Buf(2 * 1025 * 1025, 8)
    assert lib.xmem_pack_value_input(a.ptr, b.ptr, out.ptr, 2, 1025, 1025, stream()) == OK
    done('pack_value_input', 2 * 1025 * 1025, out, R.pack_value_input_ref(im4, masks)[0], None)

    proj = R.randn(g, 16300, 129)                                    # key_post: P (2 Ck + 1) = 16,300 * 129
    a, key, shr, sel = src(proj), Buf(16300, 64), Buf(16300, 1), Buf(16300, 64)
    assert lib.xmem_key_post(a.ptr, 129, key.ptr, shr.ptr, sel.ptr, 16300, 64, stream()) == OK
    (rk, _), (rs, bs), (re, be) = R.key_post_ref(proj, 64)
    done('key_post key', 16300 * 129, key, rk, None)
    done('key_post shrinkage', 16300 * 129, shr, rs, bs)
    done('key_post selection', 16300 * 129, sel, re, be)
    t.finish('area, copy, gru, add3, pack_image, pack_value_input, key_post')


def test_grid_stride_second_trip_probability_planes(lib):
    t = Trip(2)
    done, g, fails = t.done, t.g, t.fails
    lg = R.randn(g, 1, 272, 484) * 4                                 # logits_to_prob: 16 h4 w4 = 1088 * 1936, K = 1 (the size of a 1080p frame, padded)
    (ref, bound), _ = R.logits_to_prob_ref(lg, 1080, 1920, 4, 8)
    a, out = src(lg.reshape(-1, 1)), Buf(2, 1080 * 1920)
    assert lib.xmem_logits_to_prob(a.ptr, out.ptr, None, 1, 272, 484, 1080, 1920, 4, 8, stream()) == OK
    done('logits_to_prob', 1088 * 1936, out, ref.reshape(2, -1), bound.reshape(2, -1))

    masks = torch.rand(1, 1450 * 1450, generator=g)                  # aggregate_masks, merge_masks, argmax_u8: H W = 1450^2
    a, out = src(masks.reshape(-1, 1)), Buf(2, 1450 * 1450)
    assert lib.xmem_aggregate_masks(a.ptr, out.ptr, 1, 1450, 1450, stream()) == OK
    done('aggregate_masks', 1450 * 1450, out, *R.aggregate_ref(masks))
    got = out.read('aggregate_masks')
    hold_sum('aggregate_masks, second trip', got, 1, fails)

    given = (torch.rand(1, 1450 * 1450, generator=g) < 0.3).float()
    b, out = src(given.reshape(-1, 1)), Buf(1, 1450 * 1450)
    assert lib.xmem_merge_masks(a.ptr, b.ptr, C.c_uint64(0), out.ptr, 1, 1450, 1450, stream()) == OK
    done('merge_masks', 1450 * 1450, out, R.merge_masks_ref(masks, given, 0)[0], None)

    p2 = torch.cat([masks, given * 0.5], 0)
    a, out = src(p2.reshape(-1, 1)), Buf(1, 1450 * 1450, dtype=torch.uint8, fill=0xAB)
    assert lib.xmem_argmax_u8(a.ptr, out.ptr, 2, 1450, 1450, stream()) == OK
    done('argmax_u8', 1450 * 1450, out, R.argmax_ref(p2)[0][None], None)

    x = torch.rand(1, 700, 710, generator=g)                         # resize_bilinear: C Ho Wo = 1450^2
    a, out = src(x.reshape(-1, 1)), Buf(1, 1450 * 1450)
    assert lib.xmem_resize_bilinear(a.ptr, out.ptr, 1, 700, 710, 1450, 1450, stream()) == OK
    ref, bound = R.resize_bilinear_ref(x, 1450, 1450)
    done('resize_bilinear', 1450 * 1450, out, ref.reshape(1, -1), bound.reshape(1, -1))
    t.finish('logits_to_prob, aggregate, merge, argmax, resize')


for _f in (test_grid_stride_second_trip_decoder_maps, test_grid_stride_second_trip_channel_kernels, test_grid_stride_second_trip_probability_planes):
    _f.__doc__ = GRID_DOC


# ---------------------------------------------------------------------------------------------------------
# a slice through the ops.* wrappers
# ---------------------------------------------------------------------------------------------------------
def test_ops_surface(lib):
    """The same references through xmem2_amd.ops at one edge shape per wrapper (the wrappers allocate dense outputs)."""
    from xmem2_amd import ops
    fails, worst, n = [], 0.0, 0

    def one(what, got, ref, bound):
        nonlocal worst, n
        sync(what)
        worst = max(worst, hold('ops.' + what, got.cpu().double(), ref, bound, fails))
        n += 1
    c = R.case('maxpool', B=3, H=5, W=7, C=68, data='negative', in_half=0, out_half=1)
    i = R.make_inputs(c)
    one('maxpool3x3s2', ops.maxpool3x3s2(i['x'].cuda(), out_dtype=torch.float16), *R.reference(c, i))
    c = R.case('upsample2x_add', B=3, h=1, w=3, C=12, half=0)
    i = R.make_inputs(c)
    one('upsample2x_add', ops.upsample2x_add(i['g'].cuda(), i['skip'].cuda()), *R.reference(c, i))
    c = R.case('cbam_residual', B=3, H=1, W=17, C=528, data='negative', half=0)
    i = R.make_inputs(c)
    one('cbam_residual', ops.cbam_residual(i['g'].cuda(), cbam_dev_weights(i, 528)), *R.reference(c, i))
    c = R.case('gru_gate', Ch=3, N=35, inplace=1, data='saturated', half=0)
    i = R.make_inputs(c)
    h = i['h'].reshape(1, 5, 7, 3).cuda()
    one('gru_gate', ops.gru_gate(i['values'].reshape(1, 5, 7, 9).cuda(), h, out=h), *R.reference(c, i))
    c = R.case('logits_to_prob', K=12, h4=5, w4=7, H=18, W=25, lh=1, lw=2, padded=1, data='mixed')
    i = R.make_inputs(c)
    (ref, bound), (pref, pbound) = R.logits_to_prob_ref(i['logits'], 18, 25, 1, 2)
    prob, padded = ops.logits_to_prob(i['logits'].cuda(), 18, 25, 1, 2)
    one('logits_to_prob', prob, ref, bound)
    one('logits_to_prob padded', padded, pref, pbound)
    hold_sum('ops.logits_to_prob', prob.cpu().reshape(13, -1), 12, fails)
    c = R.case('aggregate_masks', K=9, H=9, W=13, data='overlap')
    i = R.make_inputs(c)
    got = ops.aggregate_masks(i['masks'].cuda())
    one('aggregate_masks', got.reshape(10, -1), *R.reference(c, i))
    hold_sum('ops.aggregate_masks', got.cpu().reshape(10, -1), 9, fails)
    c = R.case('argmax_u8', C=255, P=300)
    i = R.make_inputs(c)
    one('argmax_u8', ops.argmax_u8(i['prob'].reshape(255, 12, 25).cuda()).reshape(-1), *R.reference(c, i))
    c = R.case('resize_bilinear', C=3, Hi=1, Wi=9, Ho=4, Wo=20)
    i = R.make_inputs(c)
    one('resize_bilinear', ops.resize_bilinear(i['x'].cuda(), (4, 20)), *R.reference(c, i))
    finish('through xmem2_amd.ops', fails, worst, n)
