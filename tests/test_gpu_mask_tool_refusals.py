"""GPU: what the mask-tool wrappers of xmem2_amd/ops.py (J&F counts, robot clicks, run lengths, clean-up, polygons, fill, mattes) refuse
on the host.

A table of calls, each with the exception type and the whole message it must give, written out from the wrappers' source as it
stood before their argument checks were folded into shared helpers.  While a refused call runs, every way to the library raises: a
refusal launches nothing.  The integer arguments take a bool, a float, one below and one above their range, and a numpy integer
where the site refuses it; where the site accepts one, a call of a few pixels shows that it gives what the Python integer gives.
Cases named `order-` have two bad arguments and pin which of them is reported."""
import types

import numpy as np
import pytest
import torch

from xmem2_amd import ops, polygons

pytestmark = pytest.mark.gpu

NO_CPU = ' - xmem2_amd has no CPU path'
NP2 = np.int64(2)
EDGES, PLANE = polygons.pack_edges([[[[1, 1, 5, 1, 5, 5, 1, 5]], [[2, 2, 7, 2, 7, 6]]]], 2, 8)     # one 8 x 8 frame, two rows
CASES = []


def case(name, exc, message, call):
    CASES.append(pytest.param(exc, message, call, id=name))


def integers(site, arg, lo, hi, call, template, numpy_refused=False):
    """`arg` as True, a float, lo - 1 and hi + 1 (and a numpy.int64 where the site takes Python integers only) -> ValueError(template)"""
    for v in (True, 2.0, lo - 1, hi + 1) + ((np.int64(lo),) if numpy_refused else ()):
        case(f'{site}-{arg}-{v!r}', ValueError, template.format(v=v), lambda t, v=v: call(t, v))


@pytest.fixture(scope='module')
def t():
    """the tensors the table's calls take: 8 x 8 pixels, K = 2"""
    dev = torch.device('cuda', torch.cuda.current_device())
    maps = np.zeros((8, 8), np.uint8)
    maps[1:4, 1:5], maps[5:7, 2:8] = 1, 2
    ns = types.SimpleNamespace(
        u8=torch.from_numpy(maps).to(dev), u8_cpu=torch.from_numpy(maps), f32=torch.zeros((8, 8), device=dev),
        u8_1d=torch.zeros(8, dtype=torch.uint8, device=dev), u8_4d=torch.zeros((1, 1, 8, 8), dtype=torch.uint8, device=dev),
        u8_empty=torch.zeros((0, 8), dtype=torch.uint8, device=dev), u8_empty3=torch.zeros((2, 8, 0), dtype=torch.uint8, device=dev),
        u8_44=torch.zeros((4, 4), dtype=torch.uint8, device=dev), f32_44=torch.zeros((4, 4), device=dev),
        u8_strided=torch.zeros((8, 16), dtype=torch.uint8, device=dev)[:, ::2], u8_188=torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev),
        u8_144=torch.zeros((1, 4, 4), dtype=torch.uint8, device=dev), i32_188=torch.zeros((1, 8, 8), dtype=torch.int32, device=dev),
        u8_188_strided=torch.zeros((1, 8, 16), dtype=torch.uint8, device=dev)[:, :, ::2],
        i32=torch.zeros((8, 8), dtype=torch.int32, device=dev), i32_44=torch.zeros((4, 4), dtype=torch.int32, device=dev),
        i32_strided=torch.zeros((8, 16), dtype=torch.int32, device=dev)[:, ::2],
        d2=torch.zeros((2, 8, 8), dtype=torch.int32, device=dev),
        rec28=torch.zeros(28, dtype=torch.int32, device=dev), rec29=torch.zeros(29, dtype=torch.int32, device=dev),
        rec27=torch.zeros(27, dtype=torch.int32, device=dev), rec_cpu=torch.zeros(28, dtype=torch.int32),
        rec_i64=torch.zeros(28, dtype=torch.int64, device=dev), rec_2d=torch.zeros((2, 14), dtype=torch.int32, device=dev),
        rec_strided=torch.zeros(56, dtype=torch.int32, device=dev)[::2], rec_many=torch.zeros(65536 * 13, dtype=torch.int32, device=dev),
        chars=torch.full((4,), 48, dtype=torch.uint8, device=dev), ofs=torch.zeros((1, 3), dtype=torch.int32, device=dev),
        ofs_k3=torch.zeros((1, 4), dtype=torch.int32, device=dev), ofs_cpu=torch.zeros((1, 3), dtype=torch.int32),
        ofs_none=torch.zeros((0, 3), dtype=torch.int32, device=dev), ofs_many=torch.zeros((65536, 3), dtype=torch.int32, device=dev),
        tables=torch.zeros((2, 33), dtype=torch.uint8, device=dev), tables_short=torch.zeros((1, 10), dtype=torch.uint8, device=dev),
        tables_5=torch.zeros((5, 33), dtype=torch.uint8, device=dev), tables_i32=torch.zeros((2, 33), dtype=torch.int32, device=dev),
        tables_1d=torch.zeros(33, dtype=torch.uint8, device=dev), tables_cpu=torch.zeros((2, 33), dtype=torch.uint8),
        nhwc=torch.zeros((1, 2, 2, 4), device=dev), sb8=torch.zeros(8, device=dev), sb6=torch.zeros(6, device=dev))
    return ns


# ---- jf_counts, further up in ops.py, takes its maps through the same check --------------------------------------------------------------

for _name, _m in (('dtype', 'f32'), ('cpu', 'u8_cpu'), ('rank1', 'u8_1d'), ('rank4', 'u8_4d')):
    case(f'jf_counts-gt-{_name}', RuntimeError, 'gt: expected a uint8 CUDA (HIP) tensor [H,W] or [B,H,W]' + NO_CPU,
         lambda t, m=_m: ops.jf_counts(getattr(t, m), t.u8, 1))
    case(f'jf_counts-pred-{_name}', RuntimeError, 'pred: expected a uint8 CUDA (HIP) tensor [H,W] or [B,H,W]' + NO_CPU,
         lambda t, m=_m: ops.jf_counts(t.u8, getattr(t, m), 1))
case('jf_counts-shapes', RuntimeError, 'gt and pred differ in shape: (8, 8) != (4, 4)', lambda t: ops.jf_counts(t.u8, t.u8_44, 1))
case('order-jf_counts-gt-before-pred', RuntimeError, 'gt: expected a uint8 CUDA (HIP) tensor [H,W] or [B,H,W]' + NO_CPU,
     lambda t: ops.jf_counts(t.f32, t.i32, 1))
case('order-jf_counts-pred-before-shapes', RuntimeError, 'pred: expected a uint8 CUDA (HIP) tensor [H,W] or [B,H,W]' + NO_CPU,
     lambda t: ops.jf_counts(t.u8, t.f32_44, 1))
case('jf_counts-out', RuntimeError, 'out: expected a contiguous int32 CUDA (HIP) tensor of shape (1, 256, 7)', lambda t: ops.jf_counts(t.u8, t.u8, 1, out=t.i32))

# ---- robot clicks ---------------------------------------------------------------------------------------------------------------

case('edt_sq-rank', RuntimeError, 'edt_sq: expected [H,W] or [B,H,W], got (8,)', lambda t: ops.edt_sq(t.u8_1d))
case('edt_sq-dtype', RuntimeError, 'mask: expected a uint8 CUDA (HIP) tensor' + NO_CPU, lambda t: ops.edt_sq(t.f32))
case('edt_sq-cpu', RuntimeError, 'mask: expected a uint8 CUDA (HIP) tensor' + NO_CPU, lambda t: ops.edt_sq(t.u8_cpu))
for _name, _out in (('shape', 'i32_44'), ('dtype', 'u8'), ('strided', 'i32_strided')):
    case(f'edt_sq-out-{_name}', RuntimeError, 'edt_sq: out must be a contiguous int32 CUDA (HIP) tensor of shape (8, 8)',
         lambda t, o=_out: ops.edt_sq(t.u8, out=getattr(t, o)))
case('click_errors-rank', RuntimeError, 'click_errors: gt must be [H,W], got (8,)', lambda t: ops.click_errors(t.u8, t.u8_1d))
case('click_errors-dtype', RuntimeError, 'gt: expected a uint8 CUDA (HIP) tensor' + NO_CPU, lambda t: ops.click_errors(t.u8, t.f32))
case('click_errors-threshold', RuntimeError, 'click_errors: a probability map needs its threshold', lambda t: ops.click_errors(t.f32, t.u8))
case('click_errors-prob-shape', RuntimeError, 'click_errors: pred (4, 4) and gt (8, 8) differ in shape',
     lambda t: ops.click_errors(t.f32_44, t.u8, threshold=0.5))
case('click_errors-mask-shape', RuntimeError, 'pred: expected a uint8 CUDA (HIP) tensor of shape (8, 8)' + NO_CPU,
     lambda t: ops.click_errors(t.u8_44, t.u8))
case('click_errors-planes', RuntimeError, 'planes: expected a uint8 CUDA (HIP) tensor of shape (2, 8, 8)' + NO_CPU,
     lambda t: ops.click_errors(t.u8, t.u8, planes=t.u8_188))
case('next_click-d2', RuntimeError, 'next_click: d2 must be a contiguous int32 CUDA (HIP) tensor [2,H,W]', lambda t: ops.next_click(t.i32_188, t.u8))
case('next_click-d2-dtype', RuntimeError, 'next_click: d2 must be a contiguous int32 CUDA (HIP) tensor [2,H,W]',
     lambda t: ops.next_click(t.d2.float(), t.u8))
for _name, _nc in (('shape', 'u8_44'), ('dtype', 'i32'), ('strided', 'u8_strided')):
    case(f'next_click-not_clicked-{_name}', RuntimeError,
         'next_click: not_clicked must be a contiguous uint8 CUDA (HIP) tensor of shape (8, 8) (it is written)',
         lambda t, n=_nc: ops.next_click(t.d2, getattr(t, n)))

# ---- rle_encode and mask_polygons: the same arguments ------------------------------------------------------------------------------

for _fn in ('rle_encode', 'mask_polygons'):
    for _name, _m in (('dtype', 'f32'), ('cpu', 'u8_cpu'), ('rank1', 'u8_1d'), ('rank4', 'u8_4d')):
        case(f'{_fn}-{_name}', RuntimeError, 'masks: expected a uint8 CUDA (HIP) tensor [H,W] or [B,H,W]' + NO_CPU,
             lambda t, f=_fn, m=_m: getattr(ops, f)(getattr(t, m), 2))
    integers(_fn, 'K', 1, 254, lambda t, v, f=_fn: getattr(ops, f)(t.u8, v), _fn + ': K = {v!r} must be an integer in 1..254', numpy_refused=True)
    case(f'{_fn}-empty', RuntimeError, _fn + ': empty input (0, 8)', lambda t, f=_fn: getattr(ops, f)(t.u8_empty, 2))
    case(f'{_fn}-empty3', RuntimeError, _fn + ': empty input (2, 8, 0)', lambda t, f=_fn: getattr(ops, f)(t.u8_empty3, 2))
    case(f'order-{_fn}-masks-before-K', RuntimeError, 'masks: expected a uint8 CUDA (HIP) tensor [H,W] or [B,H,W]' + NO_CPU,
         lambda t, f=_fn: getattr(ops, f)(t.f32, 0))
    case(f'order-{_fn}-K-before-empty', ValueError, _fn + ': K = 0 must be an integer in 1..254', lambda t, f=_fn: getattr(ops, f)(t.u8_empty, 0))
    case(f'order-{_fn}-empty-before-capacity', RuntimeError, _fn + ': empty input (0, 8)', lambda t, f=_fn: getattr(ops, f)(t.u8_empty, 2, capacity=0))
case('rle_encode-capacity-0', ValueError, 'rle_encode: capacity = 0 must be at least 1', lambda t: ops.rle_encode(t.u8, 2, capacity=0))
case('mask_polygons-capacity-0', ValueError, 'mask_polygons: capacity = 0 must be in 1..268435456', lambda t: ops.mask_polygons(t.u8, 2, capacity=0))
case('mask_polygons-capacity-above', ValueError, 'mask_polygons: capacity = 268435457 must be in 1..268435456',
     lambda t: ops.mask_polygons(t.u8, 2, capacity=268435457))

# ---- rle_decode ---------------------------------------------------------------------------------------------------------------------

for _i, (_arg, _top) in enumerate((('H', 16384), ('W', 16384), ('K', 254))):
    integers('rle_decode', _arg, 1, _top, lambda t, v, i=_i: ops.rle_decode(t.rec28, *((8, 8, 2)[:i] + (v,) + (8, 8, 2)[i + 1:]), capacity=16),
             'rle_decode: ' + _arg + ' = {v!r} must be an integer in 1..' + str(_top))
for _v in (True, 1.5, 0, -3):
    case(f'rle_decode-capacity-{_v!r}', ValueError, f'rle_decode: capacity = {_v!r} must be an integer of at least 1',
         lambda t, v=_v: ops.rle_decode(t.rec28, 8, 8, 2, capacity=v))
for _name, _rec in (('cpu', 'rec_cpu'), ('dtype', 'rec_i64'), ('rank', 'rec_2d'), ('strided', 'rec_strided')):
    case(f'rle_decode-record-{_name}', RuntimeError, 'record: expected the contiguous int32 CUDA (HIP) tensor of rle_encode(wait=False)' + NO_CPU,
         lambda t, r=_rec: ops.rle_decode(getattr(t, r), 8, 8, 2, capacity=16))
case('rle_decode-no-capacity', ValueError, 'rle_decode: a device record needs the capacity it was encoded with', lambda t: ops.rle_decode(t.rec28, 8, 8, 2))
case('rle_decode-record-29', ValueError, 'rle_decode: a record of 29 words is not a whole number of frames of K = 2, capacity = 16',
     lambda t: ops.rle_decode(t.rec29, 8, 8, 2, capacity=16))
case('rle_decode-record-27', ValueError, 'rle_decode: a record of 27 words is not a whole number of frames of K = 2, capacity = 16',
     lambda t: ops.rle_decode(t.rec27, 8, 8, 2, capacity=16))
case('rle_decode-frames', ValueError, 'rle_decode: 65536 frames in one launch, at most 65535', lambda t: ops.rle_decode(t.rec_many, 8, 8, 2, capacity=1))
case('rle_decode-host-meta', ValueError, 'rle_decode: expected (meta [B, 2, >= 1], B event arrays), got meta (1, 3, 6) and 1 arrays',
     lambda t: ops.rle_decode((np.zeros((1, 3, 6), np.int32), [np.zeros(0, np.uint32)]), 8, 8, 2))
case('rle_decode-host-arrays', ValueError, 'rle_decode: expected (meta [B, 2, >= 1], B event arrays), got meta (1, 2, 6) and 2 arrays',
     lambda t: ops.rle_decode((np.zeros((1, 2, 6), np.int32), [np.zeros(0, np.uint32)] * 2), 8, 8, 2))
for _name, _values in (('length', [1, 2, 3]), ('range', [1, 256]), ('kind', [1.0, 2.0])):
    case(f'rle_decode-values-{_name}', ValueError, 'rle_decode: values must be 2 integers in 0..255',
         lambda t, v=_values: ops.rle_decode(t.rec28, 8, 8, 2, capacity=16, values=v))
case('rle_decode-values-tensor-dtype', ValueError, 'rle_decode: values must be uint8 [2]',
     lambda t: ops.rle_decode(t.rec28, 8, 8, 2, capacity=16, values=torch.zeros(2, dtype=torch.int32)))
case('rle_decode-values-tensor-shape', ValueError, 'rle_decode: values must be uint8 [2]',
     lambda t: ops.rle_decode(t.rec28, 8, 8, 2, capacity=16, values=torch.zeros(3, dtype=torch.uint8)))
for _name, _out in (('shape', 'u8_144'), ('rank', 'u8'), ('dtype', 'i32_188'), ('strided', 'u8_188_strided'), ('cpu', 'u8_cpu')):
    case(f'rle_decode-out-{_name}', RuntimeError, 'rle_decode: out must be a contiguous uint8 CUDA (HIP) tensor (1, 8, 8)',
         lambda t, o=_out: ops.rle_decode(t.rec28, 8, 8, 2, capacity=16, out=getattr(t, o)))
case('order-rle_decode-H-before-record', ValueError, 'rle_decode: H = 0 must be an integer in 1..16384', lambda t: ops.rle_decode(t.rec_i64, 0, 8, 2))
case('order-rle_decode-record-before-no-capacity', RuntimeError,
     'record: expected the contiguous int32 CUDA (HIP) tensor of rle_encode(wait=False)' + NO_CPU, lambda t: ops.rle_decode(t.rec_i64, 8, 8, 2))
case('order-rle_decode-no-capacity-before-frames', ValueError, 'rle_decode: a device record needs the capacity it was encoded with',
     lambda t: ops.rle_decode(t.rec29, 8, 8, 2))
case('order-rle_decode-frames-before-out', ValueError, 'rle_decode: a record of 29 words is not a whole number of frames of K = 2, capacity = 16',
     lambda t: ops.rle_decode(t.rec29, 8, 8, 2, capacity=16, out=t.u8_144))
case('order-rle_decode-values-before-out', ValueError, 'rle_decode: values must be 2 integers in 0..255',
     lambda t: ops.rle_decode(t.rec28, 8, 8, 2, capacity=16, values=[1], out=t.u8_144))

# ---- rle_compress, rle_string_offsets, rle_decompress ---------------------------------------------------------------------------------

for _i, (_arg, _top) in enumerate((('H', 16384), ('W', 16384), ('K', 254))):
    integers('rle_compress', _arg, 1, _top, lambda t, v, i=_i: ops.rle_compress(t.rec28, *((8, 8, 2)[:i] + (v,) + (8, 8, 2)[i + 1:]), 16),
             'rle_compress: ' + _arg + ' = {v!r} must be an integer in 1..' + str(_top))
    integers('rle_decompress', _arg, 1, _top, lambda t, v, i=_i: ops.rle_decompress([['0', '0']], *((8, 8, 2)[:i] + (v,) + (8, 8, 2)[i + 1:])),
             'rle_decompress: ' + _arg + ' = {v!r} must be an integer in 1..' + str(_top))
integers('rle_compress', 'capacity', 1, 1 << 28, lambda t, v: ops.rle_compress(t.rec28, 8, 8, 2, v),
         'rle_compress: capacity = {v!r} must be an integer in 1..268435456')
integers('rle_compress', 'char_capacity', 1, (1 << 31) - 1, lambda t, v: ops.rle_compress(t.rec28, 8, 8, 2, 16, char_capacity=v),
         'rle_compress: char_capacity = {v!r} must be an integer in 1..2147483647')
integers('rle_decompress', 'capacity', 1, (1 << 31) - 1, lambda t, v: ops.rle_decompress([['0', '0']], 8, 8, 2, capacity=v),
         'rle_decompress: capacity = {v!r} must be an integer in 1..2147483647')
for _name, _rec in (('cpu', 'rec_cpu'), ('dtype', 'rec_i64'), ('rank', 'rec_2d'), ('strided', 'rec_strided')):
    case(f'rle_compress-record-{_name}', RuntimeError, 'record: expected the contiguous int32 CUDA (HIP) tensor of rle_encode(wait=False)' + NO_CPU,
         lambda t, r=_rec: ops.rle_compress(getattr(t, r), 8, 8, 2, 16))
case('rle_compress-record-list', RuntimeError, 'record: expected the contiguous int32 CUDA (HIP) tensor of rle_encode(wait=False)' + NO_CPU,
     lambda t: ops.rle_compress([0] * 28, 8, 8, 2, 16))
case('rle_compress-record-29', ValueError, 'rle_compress: a record of 29 words is not a whole number of frames of K = 2, capacity = 16',
     lambda t: ops.rle_compress(t.rec29, 8, 8, 2, 16))
case('rle_compress-record-27', ValueError, 'rle_compress: a record of 27 words is not a whole number of frames of K = 2, capacity = 16',
     lambda t: ops.rle_compress(t.rec27, 8, 8, 2, 16))
case('rle_compress-frames', ValueError, 'rle_compress: 65536 frames in one launch, at most 65535', lambda t: ops.rle_compress(t.rec_many, 8, 8, 2, 1))
case('order-rle_compress-capacity-before-record', ValueError, 'rle_compress: capacity = 0 must be an integer in 1..268435456',
     lambda t: ops.rle_compress(t.rec_i64, 8, 8, 2, 0))
case('order-rle_compress-frames-before-char_capacity', ValueError,
     'rle_compress: a record of 29 words is not a whole number of frames of K = 2, capacity = 16',
     lambda t: ops.rle_compress(t.rec29, 8, 8, 2, 16, char_capacity=0))
case('rle_string_offsets-dtype', ValueError,
     'rle_string_offsets: expected the uint8 device tensor of rle_compress(wait=False) for 1 frames, K = 2, char_capacity = 20',
     lambda t: ops.rle_string_offsets(t.rec28, 1, 2, 20))
case('rle_string_offsets-length', ValueError,
     'rle_string_offsets: expected the uint8 device tensor of rle_compress(wait=False) for 1 frames, K = 2, char_capacity = 16',
     lambda t: ops.rle_string_offsets(t.u8_1d, 1, 2, 16))
case('rle_decompress-chars-dtype', RuntimeError, 'rle_decompress: chars must be a contiguous uint8 CUDA (HIP) tensor' + NO_CPU,
     lambda t: ops.rle_decompress((t.rec28, t.ofs), 8, 8, 2, capacity=4))
case('rle_decompress-chars-rank', RuntimeError, 'rle_decompress: chars must be a contiguous uint8 CUDA (HIP) tensor' + NO_CPU,
     lambda t: ops.rle_decompress((t.u8, t.ofs), 8, 8, 2, capacity=4))
for _name, _ofs in (('K', 'ofs_k3'), ('cpu', 'ofs_cpu'), ('dtype', 'u8_44')):
    case(f'rle_decompress-ofs-{_name}', ValueError, 'rle_decompress: str_ofs must be a contiguous int32 tensor [B, 3] on the device of chars',
         lambda t, o=_ofs: ops.rle_decompress((t.chars, getattr(t, o)), 8, 8, 2, capacity=4))
case('rle_decompress-no-capacity', ValueError, 'rle_decompress: a device record needs a capacity', lambda t: ops.rle_decompress((t.chars, t.ofs), 8, 8, 2))
case('rle_decompress-frames-0', ValueError, 'rle_decompress: 0 frames in one launch, 1..65535 fit',
     lambda t: ops.rle_decompress((t.chars, t.ofs_none), 8, 8, 2, capacity=4))
case('rle_decompress-frames-65536', ValueError, 'rle_decompress: 65536 frames in one launch, 1..65535 fit',
     lambda t: ops.rle_decompress((t.chars, t.ofs_many), 8, 8, 2, capacity=4))
case('rle_decompress-no-frames', ValueError, 'rle_decompress: no frames', lambda t: ops.rle_decompress([], 8, 8, 2))
case('rle_decompress-rows', ValueError, 'rle_decompress: frame 0 has 1 rows, expected 2', lambda t: ops.rle_decompress([['0']], 8, 8, 2))
case('rle_decompress-ascii', ValueError, 'rle_decompress: frame 0, row 1: a character outside 48..111', lambda t: ops.rle_decompress([['0', 'é']], 8, 8, 2))
case('rle_decompress-type', ValueError, 'rle_decompress: frame 0, row 0: expected str, bytes or None, got int', lambda t: ops.rle_decompress([[7, '0']], 8, 8, 2))
case('rle_decompress-empty-string', ValueError, 'rle_decompress: frame 0, row 0: an empty string holds no counts',
     lambda t: ops.rle_decompress([['', '0']], 8, 8, 2))

# ---- components, clean_masks ------------------------------------------------------------------------------------------------------------

for _v in (6, True, None):
    case(f'components-connectivity-{_v!r}', ValueError, f'components: connectivity = {_v!r} must be 4 or 8',
         lambda t, v=_v: ops.components(t.u8, connectivity=v))
for _fn, _call in (('components', lambda m: ops.components(m)), ('clean_masks', lambda m: ops.clean_masks(m, min_area=2)),
                   ('signed_edt_sq', lambda m: ops.signed_edt_sq(m, 2, 3)), ('mask_mattes', lambda m: ops.mask_mattes(m, 2, None, 3)),
                   ('grow_masks', lambda m: ops.grow_masks(m, 1))):
    for _name, _m in (('dtype', 'f32'), ('cpu', 'u8_cpu'), ('rank1', 'u8_1d'), ('rank4', 'u8_4d')):
        case(f'{_fn}-{_name}', RuntimeError, _fn + ': expected a uint8 CUDA (HIP) tensor [H,W] or [N,H,W]' + NO_CPU,
             lambda t, c=_call, m=_m: c(getattr(t, m)))
    case(f'{_fn}-empty', RuntimeError, _fn + ': empty input (0, 8)', lambda t, c=_call: c(t.u8_empty))
    case(f'{_fn}-empty3', RuntimeError, _fn + ': empty input (2, 8, 0)', lambda t, c=_call: c(t.u8_empty3))
for _fn, _call in (('clean_masks', lambda m, o: ops.clean_masks(m, min_area=2, out=o)), ('grow_masks', lambda m, o: ops.grow_masks(m, 1, out=o))):
    for _name, _out in (('shape', 'u8_44'), ('rank', 'u8_188'), ('dtype', 'i32'), ('strided', 'u8_strided'), ('cpu', 'u8_cpu')):
        case(f'{_fn}-out-{_name}', RuntimeError, _fn + ": out must be a contiguous uint8 CUDA (HIP) tensor of shape (8, 8) on the masks' device",
             lambda t, c=_call, o=_out: c(t.u8, getattr(t, o)))
    case(f'{_fn}-out-shape3', RuntimeError, _fn + ": out must be a contiguous uint8 CUDA (HIP) tensor of shape (1, 8, 8) on the masks' device",
         lambda t, c=_call: c(t.u8_188, t.u8))
case('clean_masks-min_area', ValueError, 'mask_cleanup: min_area = -1 must be in 0..2^31-1', lambda t: ops.clean_masks(t.u8, min_area=-1))
case('clean_masks-max_hole', ValueError, 'mask_cleanup: max_hole = 1.5 must be an integer', lambda t: ops.clean_masks(t.u8, max_hole=1.5))
case('clean_masks-keep_largest', ValueError, 'mask_cleanup: keep_largest = 2 must be a bool', lambda t: ops.clean_masks(t.u8, keep_largest=2))
case('order-clean_masks-spec-before-masks', ValueError, 'mask_cleanup: min_area = -1 must be in 0..2^31-1', lambda t: ops.clean_masks(t.f32, min_area=-1))
case('order-clean_masks-masks-before-out', RuntimeError, 'clean_masks: expected a uint8 CUDA (HIP) tensor [H,W] or [N,H,W]' + NO_CPU,
     lambda t: ops.clean_masks(t.f32, min_area=2, out=t.i32))

# ---- fill_edges, fill_polygons --------------------------------------------------------------------------------------------------------

for _i, (_arg, _lo, _hi) in enumerate((('N', 1, 1 << 30), ('H', 1, 16384), ('W', 1, 16384), ('R', 1, 1 << 20))):
    integers('fill_edges', _arg, _lo, _hi, lambda t, v, i=_i: ops.fill_edges(EDGES, PLANE, *((1, 8, 8, 2)[:i] + (v,) + (1, 8, 8, 2)[i + 1:])),
             'fill_polygons: ' + _arg + ' = {v!r} must be an integer in ' + f'{_lo}..{_hi}')
integers('fill_edges', 'frac_bits', 0, 8, lambda t, v: ops.fill_edges(EDGES, PLANE, 1, 8, 8, 2, frac_bits=v),
         'fill_polygons: frac_bits = {v!r} must be an integer in 0..8')
case('fill_edges-planes', ValueError, 'fill_polygons: 2 edges, 3 plane indices', lambda t: ops.fill_edges(EDGES[:2], [0, 0, 1], 1, 8, 8, 2))
case('fill_edges-rows-256', ValueError, 'fill_polygons: 256 rows need a values table, row + 1 does not fit a byte',
     lambda t: ops.fill_edges(EDGES, PLANE, 1, 8, 8, 256))
for _name, _values in (('length', [1, 2, 3]), ('range', [1, 256]), ('negative', [-1, 2]), ('kind', [1.0, 2.0])):
    case(f'fill_edges-values-{_name}', ValueError, 'fill_polygons: values must be 2 integers in 0..255',
         lambda t, v=_values: ops.fill_edges(EDGES, PLANE, 1, 8, 8, 2, values=v))
case('fill_edges-overlay', ValueError, 'fill_polygons: overlay needs the planes to lay over (out)',
     lambda t: ops.fill_edges(EDGES, PLANE, 1, 8, 8, 2, overlay=True))
for _name, _out in (('shape', 'u8_144'), ('rank', 'u8'), ('dtype', 'i32_188'), ('strided', 'u8_188_strided'), ('cpu', 'u8_cpu')):
    case(f'fill_edges-out-{_name}', RuntimeError, 'fill_polygons: out must be a contiguous uint8 CUDA (HIP) tensor (1, 8, 8)' + NO_CPU,
         lambda t, o=_out: ops.fill_edges(EDGES, PLANE, 1, 8, 8, 2, out=getattr(t, o)))
case('fill_edges-out-array', RuntimeError, 'fill_polygons: out must be a contiguous uint8 CUDA (HIP) tensor (1, 8, 8)' + NO_CPU,
     lambda t: ops.fill_edges(EDGES, PLANE, 1, 8, 8, 2, out=np.zeros((1, 8, 8), np.uint8)))
case('order-fill_edges-N-before-values', ValueError, 'fill_polygons: N = 0 must be an integer in 1..1073741824',
     lambda t: ops.fill_edges(EDGES, PLANE, 0, 8, 8, 2, values=[1]))
case('order-fill_edges-values-before-out', ValueError, 'fill_polygons: values must be 2 integers in 0..255',
     lambda t: ops.fill_edges(EDGES, PLANE, 1, 8, 8, 2, values=[1], out=t.u8_144))
case('fill_polygons-no-frames', ValueError, 'fill_polygons: no frames', lambda t: ops.fill_polygons([], 8, 8))

# ---- signed_edt_sq, mask_mattes, grow_masks -------------------------------------------------------------------------------------------

for _fn, _call in (('signed_edt_sq', lambda t, K, R: ops.signed_edt_sq(t.u8, K, R)), ('mask_mattes', lambda t, K, R: ops.mask_mattes(t.u8, K, t.tables, R))):
    integers(_fn, 'K', 1, 255, lambda t, v, c=_call: c(t, v, 3), _fn + ': K = {v!r} must be an integer in 1..255', numpy_refused=True)
    integers(_fn, 'R', 1, 127, lambda t, v, c=_call: c(t, 2, v), _fn + ': R = {v!r} must be an integer in 1..127', numpy_refused=True)
    case(f'order-{_fn}-K-before-R', ValueError, _fn + ': K = 0 must be an integer in 1..255', lambda t, c=_call: c(t, 0, 0))
case('order-signed_edt_sq-K-before-masks', ValueError, 'signed_edt_sq: K = 0 must be an integer in 1..255', lambda t: ops.signed_edt_sq(t.f32, 0, 3))
for _name, _tables in (('none', None), ('array', np.zeros((2, 33), np.uint8))):
    case(f'mask_mattes-tables-{_name}', RuntimeError, "mask_mattes: tables must be a uint8 tensor [T, 2 (R + 1)^2 + 1] on the masks' device",
         lambda t, v=_tables: ops.mask_mattes(t.u8, 2, v, 3))
for _name, _tables in (('dtype', 'tables_i32'), ('rank', 'tables_1d'), ('cpu', 'tables_cpu')):
    case(f'mask_mattes-tables-{_name}', RuntimeError, "mask_mattes: tables must be a uint8 tensor [T, 2 (R + 1)^2 + 1] on the masks' device",
         lambda t, v=_tables: ops.mask_mattes(t.u8, 2, getattr(t, v), 3))
case('mask_mattes-tables-length', ValueError, 'mask_mattes: tables (1, 10): expected 1..4 rows of 33 for R = 3',
     lambda t: ops.mask_mattes(t.u8, 2, t.tables_short, 3))
case('mask_mattes-tables-5', ValueError, 'mask_mattes: tables (5, 33): expected 1..4 rows of 33 for R = 3', lambda t: ops.mask_mattes(t.u8, 2, t.tables_5, 3))
case('mask_mattes-tables-other-R', ValueError, 'mask_mattes: tables (2, 33): expected 1..4 rows of 51 for R = 4', lambda t: ops.mask_mattes(t.u8, 2, t.tables, 4))
case('order-mask_mattes-masks-before-tables', RuntimeError, 'mask_mattes: expected a uint8 CUDA (HIP) tensor [H,W] or [N,H,W]' + NO_CPU,
     lambda t: ops.mask_mattes(t.f32, 2, None, 3))
for _v in (0, 0.5, -0.9):
    case(f'grow_masks-r-{_v!r}', ValueError, f'grow_masks: r = {_v!r} changes nothing (|r| must be at least 1)', lambda t, v=_v: ops.grow_masks(t.u8, v))
for _v in (True, 'a', float('nan')):
    case(f'grow_masks-r-{_v!r}', ValueError, f'grow: r = {_v!r} must be a finite number', lambda t, v=_v: ops.grow_masks(t.u8, v))
case('grow_masks-r-128', ValueError, 'grow: |r| = 128 must be at most 127', lambda t: ops.grow_masks(t.u8, -128))
case('order-grow_masks-r-before-masks', ValueError, 'grow_masks: r = 0 changes nothing (|r| must be at least 1)', lambda t: ops.grow_masks(t.f32, 0))

# ---- the click refinement's wrappers, which share the section ---------------------------------------------------------------------------

case('brs_affine-dtype', RuntimeError, 'brs_affine input: expected float32', lambda t: ops.brs_affine(t.nhwc.half(), t.sb8))
case('brs_affine-length', RuntimeError, 'brs_affine: expected a contiguous input and 8 scale / bias values', lambda t: ops.brs_affine(t.nhwc, t.sb6))
case('brs_affine-out', RuntimeError, 'brs_affine: out must be contiguous and shaped like the input', lambda t: ops.brs_affine(t.nhwc, t.sb8, out=t.f32))
case('relu_gate-shape', RuntimeError, 'relu_gate: y and g must be contiguous tensors of one shape', lambda t: ops.relu_gate(t.f32, t.f32_44))
case('relu_gate-out', RuntimeError, 'relu_gate: out must be contiguous and shaped like g', lambda t: ops.relu_gate(t.f32, t.f32, out=t.f32_44))
case('relu_gate_outer-shape', RuntimeError, 'relu_gate_outer: expected contiguous y [..., C], g1 with one value per pixel and w [C]',
     lambda t: ops.relu_gate_outer(t.nhwc, t.f32, t.sb8))
case('brs_param_grad-shape', RuntimeError, 'brs_param_grad: g and x must be contiguous tensors of one shape',
     lambda t: ops.brs_param_grad(t.nhwc, t.f32, t.sb8, t.sb8, t.sb8))
case('brs_param_grad-length', RuntimeError, 'brs_param_grad: scale_bias and grad hold 8 contiguous floats',
     lambda t: ops.brs_param_grad(t.nhwc, t.nhwc, t.sb6, t.sb8, t.sb8))
case('brs_loss-batch', RuntimeError, 'brs_loss: expected contiguous logits [1 or 2, h4, w4], got (3, 2, 2)',
     lambda t: ops.brs_loss(torch.zeros((3, 2, 2), device=t.f32.device), 8, 8, None, None, None, None, None))
case('brs_loss-rects', RuntimeError, 'brs_loss: rects must be a contiguous int32 [1, cap, 5] tensor on the device',
     lambda t: ops.brs_loss(torch.zeros((1, 2, 2), device=t.f32.device), 8, 8, t.i32_188, None, None, None, None))


@pytest.mark.parametrize('exc, message, call', CASES)
def test_refused_on_the_host_with_this_message(t, monkeypatch, exc, message, call):
    from xmem2_amd import _lib_masks, _lib_matte, _lib_polygons, _lib_raster

    def library(*args):
        raise AssertionError('a call that is to be refused reached the library')
    monkeypatch.setattr(ops, 'load', library)
    for module in (_lib_masks, _lib_polygons, _lib_raster, _lib_matte):
        monkeypatch.setattr(module, 'load', library)
    with pytest.raises(exc) as e:
        call(t)
    assert type(e.value) is exc and str(e.value) == message


def test_the_table_covers_every_wrapper_of_the_section():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for fn in ('jf_counts', 'edt_sq', 'click_errors', 'next_click', 'rle_encode', 'rle_decode', 'rle_compress', 'rle_string_offsets', 'rle_decompress',
               'components', 'clean_masks', 'mask_polygons', 'fill_edges', 'fill_polygons', 'signed_edt_sq', 'mask_mattes', 'grow_masks',
               'brs_affine', 'relu_gate', 'relu_gate_outer', 'brs_loss', 'brs_param_grad'):
        assert any(i.startswith(fn + '-') for i in ids), fn


# ---- numpy integers where the site takes them: the same result as with Python integers -------------------------------------------------

def test_rle_decode_compress_decompress_take_numpy_integers(t):
    i8, i32, i64 = np.int64(8), np.int64(32), np.int64(64)                # the maps have 20 events
    record = ops.rle_encode(t.u8, 2, capacity=32, wait=False)
    want = ops.rle_decode(record, 8, 8, 2, capacity=32)
    assert torch.equal(want, t.u8[None])
    assert torch.equal(ops.rle_decode(record, i8, i8, NP2, capacity=i32), want)
    strings = ops.rle_compress(record, 8, 8, 2, 32, char_capacity=64)
    assert strings == ops.rle_compress(record, i8, i8, NP2, i32, char_capacity=i64) and all(strings[0])
    again = ops.rle_decompress(strings, i8, i8, NP2, capacity=i32)
    assert torch.equal(again, ops.rle_decompress(strings, 8, 8, 2, capacity=32))
    assert torch.equal(ops.rle_decode(again, 8, 8, 2, capacity=32), want)


def test_fill_edges_takes_numpy_integers(t):
    want = ops.fill_edges(EDGES, PLANE, 1, 8, 8, 2, frac_bits=8)
    assert want.shape == (1, 8, 8) and sorted(want.unique().tolist()) == [0, 1, 2]
    assert torch.equal(ops.fill_edges(EDGES, PLANE, np.int64(1), np.int64(8), np.int64(8), NP2, frac_bits=np.int64(8)), want)
