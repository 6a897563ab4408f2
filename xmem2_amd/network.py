"""XMem network on MI355X: the reference's ``XMem`` surface (model/network.py:17-198) over HIP kernels.

``XMem(config, model_path, map_location, ...)`` keeps the constructor, ``encode_key`` / ``encode_value`` /
``segment`` / ``load_weights`` and the 412-name state_dict of the reference, so an upstream ``XMem.pth``
loads unchanged.  Internally nothing is an nn.Module: at load time every convolution is re-laid-out to
``[Cout][KH][KW][Cin]`` with its eval-mode BatchNorm folded to a per-channel (scale, shift) epilogue
(ATen's own alpha/beta form), and every activation lives in NHWC so that the implicit-GEMM kernel
(csrc/conv_mfma.hip) reads K-contiguous operands.

Public methods take / return NCHW-shaped tensors like the reference (zero-copy permuted views of the
NHWC buffers); the ``*_nhwc`` methods are the hot path used by ``InferenceCore``.
"""
import os
import warnings

import torch

from . import ops, stages
from .arch import infer_dims, state_dict_spec
from .hipnet import HipNet, _pad4
from .ops import ConvWeights


# captured HIP-graph stages kept before the least recently replayed one is dropped
MAX_STAGES = 160
# 1/16-resolution pixels (objects x h x w) from which the decoder's tail runs as ops.mask_head_gather - one wave per such pixel: below,
# too few waves to cover the latency of their loads, the mask head, hidden_update_gather and copy_channels stay three launches
# (NOT MEASURED yet: placed between the 240p map, 405 pixels, and the 480p one, 1 620; profiles/r07_decoder_tail.txt)
FUSED_TAIL_MIN_PIXELS = 512
# pixels (batch x h x w) from which a bottleneck's expand 1x1 and the next block's reduce 1x1 run as one launch (ops.conv2d_pointwise_pair):
# a pair workgroup owns 64 pixels whatever the channel counts, so a small map is a small grid (batch 1 at 1/16 resolution: 26 workgroups
# on 256 CUs).  Set from the isolated timings of profiles/r11_bottleneck_pairs.txt.
FUSED_BOTTLENECK_MIN_PIXELS = 25920


# stages whose static outputs other stages read in place: the key encoder, and the slot a cached key pass is restored into
_KEY_PRODUCERS = ('key', 'keyr')


def _flat_outputs(outs):
    for o in outs:
        if isinstance(o, torch.Tensor):
            yield o
        elif isinstance(o, tuple):
            yield from (t for t in o if isinstance(t, torch.Tensor))


def _span(t):
    """[first, last) address of a static buffer; a placeholder (stride 0, `restored_key_slot`) owns its one element only"""
    n = 1 if (t.dim() and t.stride(-1) == 0) else t.numel()
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


def _padc(n):
    """channel padding of a buffer the network allocates: 4 floats or (fp16 loop) 8 halfs = one 16-byte operand chunk"""
    return (n + 7) // 8 * 8 if ops.act_dtype() == torch.float16 else _pad4(n)


class XMem(HipNet):
    def __init__(self, config, model_path=None, map_location=None, pretrained_key_encoder=True, pretrained_value_encoder=True):
        """Same signature as model/network.py:18.  `pretrained_*` are accepted for compatibility; torchvision
        ImageNet weights cannot be fetched offline, so a checkpoint (or load_weights) is the only weight source."""
        # captured stages are bounded by MAX_STAGES and evicted by _evict_lru (_run_stage)
        super().__init__(torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu'),
                         max_stages=lambda: MAX_STAGES)
        self.single_object = config.get('single_object', False)
        self.model_path = model_path                 # what a caller's config['model'] is compared with when the network is handed over
        self._cbam = {}
        # launch-bound stages (61 convolutions + ~40 small kernels per frame) are replayed as HIP graphs
        self.use_graphs = os.environ.get('XMEM_HIP_GRAPHS', '1') != '0'
        # the decoder's tail: mask head + HiddenUpdater input + hidden copy in one launch (ops.mask_head_gather) and the fused hidden-update
        # convolution's Cin padded to a multiple of 32 (the 1x1 operand loader).  XMEM_FUSED_TAIL=0 (or fused_tail = False BEFORE the
        # weights are uploaded) keeps the separate launches and the unpadded filters: an A/B switch, bit-identical either way
        self.fused_tail = os.environ.get('XMEM_FUSED_TAIL', '1') != '0'
        self.fused_tail_min_pixels = FUSED_TAIL_MIN_PIXELS
        # sibling 3x3 convolutions of a residual block / of the batched key pass behind one Winograd input transform, and the block's
        # branch folded into its last output transform (ops.conv2d_shared / conv2d_folded).  XMEM_SHARED_TRANSFORMS=0 keeps the
        # separate convolutions: an A/B switch, bit-identical either way.  fp32 only; the other precisions always run separately
        self.shared_transforms = os.environ.get('XMEM_SHARED_TRANSFORMS', '1') != '0'
        # a bottleneck's conv3 (+ residual, relu) and the next block's conv1 (relu) in one launch from fused_bottleneck_min_pixels pixels on
        # (ops.conv2d_pointwise_pair).  XMEM_FUSED_BOTTLENECK=0 keeps the separate convolutions: an A/B switch, bit-identical either way
        self.fused_bottleneck = os.environ.get('XMEM_FUSED_BOTTLENECK', '1') != '0'
        self.fused_bottleneck_min_pixels = FUSED_BOTTLENECK_MIN_PIXELS
        # 'fp32' (default: the parity contract) | 'fp16' (opt-in: the fp16 loop - half activations in HBM, half-operand convolutions
        # on the fp16 MFMA with fp32 accumulation: the counterpart of the reference's autocast loop, run_on_video.py:76; the
        # permanent-memory preload stays fp32 as in run_on_video.py:59-66) | 'fp16w' / 'fp32x' (experiments, ops.PRECISIONS)
        self.precision = config.get('precision', os.environ.get('XMEM_PRECISION', 'fp32'))
        if self.precision not in ops.PRECISIONS:
            raise ValueError(f"config['precision'] must be one of {ops.PRECISIONS}, got {self.precision!r}")
        self._zeros = {}                 # zero-filled scratch only (_zero_scratch): nothing of the weights, so it outlives them
        self._owner_free, self._owner_next = [], 0   # owner tokens of the cores driving this network (see acquire_owner)
        self._call_precision = None      # per-call override (InferenceCore preloads permanent memory in fp32)
        weights = self.init_hyperparameters(config, model_path, map_location)
        if weights is not None:
            self.load_weights(weights, init_as_zero_if_needed=True)

    # ---- reference surface --------------------------------------------------------------------
    def init_hyperparameters(self, config, model_path=None, map_location=None):
        """model/network.py:134-182: C_k/C_v/C_h from the checkpoint if given, else config/defaults; writes them back."""
        if model_path is not None:
            weights = torch.load(model_path, map_location=map_location or 'cpu', weights_only=True)
            self.key_dim, self.value_dim, self.hidden_dim = infer_dims(weights)
            self.disable_hidden = self.hidden_dim == 0
        else:
            weights = None
            self.key_dim = config.get('key_dim', 64)
            self.value_dim = config.get('value_dim', 512)
            self.hidden_dim = config.get('hidden_dim', 64)
            self.disable_hidden = self.hidden_dim <= 0
        config['key_dim'], config['value_dim'], config['hidden_dim'] = self.key_dim, self.value_dim, self.hidden_dim
        return weights

    def load_weights(self, src_dict, init_as_zero_if_needed=False):
        """model/network.py:184-198: pads a single-object 4-channel value stem to the 5-channel multi-object one."""
        src_dict = dict(src_dict)
        k = 'value_encoder.conv1.weight'
        if k in src_dict and src_dict[k].shape[1] == 4 and not self.single_object:
            pads = torch.zeros((64, 1, 7, 7), device=src_dict[k].device)
            if not init_as_zero_if_needed:
                torch.nn.init.orthogonal_(pads)
            src_dict[k] = torch.cat([src_dict[k], pads], 1)
        return super().load_weights(src_dict)

    def _spec(self):
        return state_dict_spec(self.key_dim, self.value_dim, self.hidden_dim, self.single_object)

    def _reupload(self):
        if self.device.type == 'cuda':          # an XMem may exist on the CPU without uploading (_need_weights)
            super()._reupload()

    def cuda(self, index=None):
        return self.to(torch.device('cuda', index if index is not None else torch.cuda.current_device()))

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('xmem2_amd.XMem is inference-only (training is out of scope, SURVEY.md section 2 #19)')
        return self

    # ---- weight preparation ---------------------------------------------------------------------
    def _upload(self):
        sd, W = self._sd, {}
        W['key_encoder.conv1'] = self._conv_w('key_encoder.conv1', 'key_encoder.bn1', 2, 3)

        def bottleneck_stage(prefix, blocks, stride):
            for b in range(blocks):
                p, s = f'{prefix}.{b}', (stride if b == 0 else 1)
                W[p + '.conv1'] = self._conv_w(p + '.conv1', p + '.bn1', 1, 0)
                W[p + '.conv2'] = self._conv_w(p + '.conv2', p + '.bn2', s, 1)
                W[p + '.conv3'] = self._conv_w(p + '.conv3', p + '.bn3', 1, 0)
                if (p + '.downsample.0.weight') in sd:
                    W[p + '.downsample'] = self._conv_w(p + '.downsample.0', p + '.downsample.1', s, 0)

        def basic_stage(prefix, blocks, stride):
            for b in range(blocks):
                p, s = f'{prefix}.{b}', (stride if b == 0 else 1)
                W[p + '.conv1'] = self._conv_w(p + '.conv1', p + '.bn1', s, 1)
                W[p + '.conv2'] = self._conv_w(p + '.conv2', p + '.bn2', 1, 1)
                if (p + '.downsample.0.weight') in sd:
                    W[p + '.downsample'] = self._conv_w(p + '.downsample.0', p + '.downsample.1', s, 0)

        bottleneck_stage('key_encoder.res2', 3, 1)
        bottleneck_stage('key_encoder.layer2', 4, 2)
        bottleneck_stage('key_encoder.layer3', 6, 2)
        W['value_encoder.conv1'] = self._conv_w('value_encoder.conv1', 'value_encoder.bn1', 2, 3)
        if W['value_encoder.conv1'].cin != 8:       # 5 (or 4) input channels live in an 8-channel packed tensor
            cw = W['value_encoder.conv1']
            wk = torch.nn.functional.pad(cw.w, (0, 8 - cw.cin))
            W['value_encoder.conv1'] = ConvWeights(wk.contiguous(), cw.scale, cw.shift, 2, 3, cin_true=cw.cin_true)
        basic_stage('value_encoder.layer1', 2, 1)
        basic_stage('value_encoder.layer2', 2, 2)
        basic_stage('value_encoder.layer3', 2, 2)

        def group_res(p):
            if (p + '.downsample.weight') in sd:
                W[p + '.downsample'] = self._conv_w(p + '.downsample', None, 1, 1)
            W[p + '.conv1'] = self._conv_w(p + '.conv1', None, 1, 1)
            W[p + '.conv2'] = self._conv_w(p + '.conv2', None, 1, 1)

        def fusion(p):
            group_res(p + '.block1')
            group_res(p + '.block2')
            a = p + '.attention'
            dev = self.device
            self._cbam[a] = dict(
                w1=sd[a + '.ChannelGate.mlp.1.weight'].float().contiguous().to(dev),
                b1=sd[a + '.ChannelGate.mlp.1.bias'].float().contiguous().to(dev),
                w2=sd[a + '.ChannelGate.mlp.3.weight'].float().contiguous().to(dev),
                b2=sd[a + '.ChannelGate.mlp.3.bias'].float().contiguous().to(dev),
                sw=sd[a + '.SpatialGate.spatial.conv.weight'].float().reshape(2, 7, 7).contiguous().to(dev),
                sb=sd[a + '.SpatialGate.spatial.conv.bias'].float().contiguous().to(dev))

        fusion('value_encoder.fuser')
        fusion('decoder.fuser')

        def split_shared(name, x_dim=1024):
            """FeatureFusionBlock sees cat([x, g]) where x (the f16 feature) is the same for every object: W*cat = W[:, :x]*x +
            W[:, x:]*g, so with several objects the x half is convolved once and enters the per-object half as a
            broadcast residual (its scale is 1, the bias stays with the per-object half)."""
            cw = W[name]
            ones, zeros = torch.ones_like(cw.scale), torch.zeros_like(cw.shift)
            W[name + '@x'] = ConvWeights(cw.w[..., :x_dim].contiguous(), ones, zeros, cw.stride, cw.pad)
            W[name + '@g'] = ConvWeights(cw.w[..., x_dim:].contiguous(), cw.scale, cw.shift, cw.stride, cw.pad)

        for blk in ('value_encoder.fuser.block1', 'decoder.fuser.block1'):
            for c in ('.conv1', '.downsample'):
                if (blk + c) in W and W[blk + c].cin > 1024 and (W[blk + c].cin - 1024) % 32 == 0:
                    split_shared(blk + c)
        if self.hidden_dim > 0:
            W['value_encoder.hidden_reinforce.transform'] = self._conv_w('value_encoder.hidden_reinforce.transform', None, 1, 1)
            W['decoder.hidden_update.g16_conv'] = self._conv_w('decoder.hidden_update.g16_conv', None, 1, 0)
            W['decoder.hidden_update.g8_conv'] = self._conv_w('decoder.hidden_update.g8_conv', None, 1, 0)
            W['decoder.hidden_update.g4_conv'] = self._conv_w('decoder.hidden_update.g4_conv', None, 1, 0)
            W['decoder.hidden_update.transform'] = self._conv_w('decoder.hidden_update.transform', None, 1, 1)
            # HiddenUpdater (model/modules.py:84-110) sums three pointwise convolutions, g16_conv(g16) + g8_conv(area(g8)) + g4_conv(area(g4)):
            # ONE pointwise convolution over the concatenated input [g16 | g8 | g4] with the filters concatenated along Cin and the
            # biases summed - one GEMM (K = 512 + 256 + 260) instead of three short ones chained through residual reads with two
            # split-K reductions (44 -> ~20 us per frame at 480p).  Same products; the sum runs over one chain instead of three.
            parts = [W['decoder.hidden_update.' + n] for n in ('g16_conv', 'g8_conv', 'g4_conv')]
            if all(float((p.scale - 1).abs().max()) == 0.0 for p in parts):
                wk = torch.cat([p.w for p in parts], 3)
                if self.fused_tail and wk.shape[3] % 32:
                    # zero filter columns up to a multiple of the 32-deep k-tile (1028 -> 1056): the convolution takes the 1x1 operand
                    # loader instead of the general one (per-tile index arithmetic, masked loads).  As many k-tiles as before, and the
                    # general loader's masked tail was a run of zero operands too: the same bits under the same plan.  The input buffer
                    # (segment_nhwc: zero-initialised scratch as wide as this Cin) keeps zeros in the padding channels.
                    wk = torch.nn.functional.pad(wk, (0, 32 - wk.shape[3] % 32))
                wk = wk.contiguous()
                W['decoder.hidden_update.g_fused'] = ConvWeights(wk, parts[0].scale, (parts[0].shift + parts[1].shift + parts[2].shift).contiguous(),
                                                                 1, 0, cin_true=sum(p.cin_true for p in parts))
        W['decoder.up_16_8.skip_conv'] = self._conv_w('decoder.up_16_8.skip_conv', None, 1, 1)
        group_res('decoder.up_16_8.out_conv')
        W['decoder.up_8_4.skip_conv'] = self._conv_w('decoder.up_8_4.skip_conv', None, 1, 1)
        group_res('decoder.up_8_4.out_conv')
        W['decoder.pred'] = self._conv_w('decoder.pred', None, 1, 1)
        # KeyProjection: key | shrinkage | selection share one implicit GEMM (Cout = 2*C_k + 1 = 129), padded with zero filters to the
        # row stride of its output (132): a channel count that is a multiple of 4 is what lets the layer take the Winograd plans
        # (K = 9 * 1024: 228 -> 85 us at batch 4); the padding columns of `proj` receive zeros, key_post never reads them
        parts = [self._conv_w('key_proj.' + n, None, 1, 1) for n in ('key_proj', 'd_proj', 'e_proj')]
        wk = torch.cat([p.w for p in parts], 0)
        sc, sh = torch.cat([p.scale for p in parts], 0), torch.cat([p.shift for p in parts], 0)
        extra = _pad4(wk.shape[0]) - wk.shape[0]
        if extra:
            wk = torch.cat([wk, wk.new_zeros((extra,) + tuple(wk.shape[1:]))], 0)
            sc, sh = torch.cat([sc, sc.new_ones(extra)], 0), torch.cat([sh, sh.new_zeros(extra)], 0)
        W['key_proj'] = ConvWeights(wk.contiguous(), sc.contiguous(), sh.contiguous(), 1, 1, cin_true=parts[0].cin_true)
        self._w = W

    def _need_weights(self):
        if not self._w:
            if self._sd is None:
                warnings.warn('XMem: no checkpoint loaded - using the deterministic synthetic weights (xmem2_amd.synth)')
                from .synth import synthetic_state_dict
                self._sd = synthetic_state_dict(0, self.key_dim, self.value_dim, self.hidden_dim)
            if self.device.type != 'cuda':
                raise RuntimeError('xmem2_amd.XMem runs on an MI355X (HIP) device only; call .to("cuda") - there is no CPU path')
            self._upload()

    # ---- HIP-graph staging ------------------------------------------------------------------------
    def _run_stage(self, name, key, inputs, fn, alias=(), mutates=()):
        """Run `fn(*inputs)` eagerly, or capture it once per (name, shapes, flags) into a HIP graph with static
        input / output buffers and replay it (stages.py)."""
        prec = self._call_precision or self.precision
        if not self.use_graphs or ops.eager_only() or name in os.environ.get('XMEM_EAGER_STAGES', '').split(','):
            with ops.precision(prec):
                return fn(*inputs)
        full_key = (name, key, prec) + tuple(tuple(t.shape) if t is not None else None for t in inputs)
        st = self._stages.lookup(full_key)
        if st is None:
            # inputs listed in `alias` are themselves stable buffers (outputs of another stage): use them in place
            static_in = [(t if i in alias else t.clone()) if t is not None else None for i, t in enumerate(inputs)]
            with ops.precision(prec):
                st = stages.capture(fn, static_in, mutates)
            self._stages.put(full_key, st, evict=self._evict_lru)
        return st.replay(inputs)

    def _evict_lru(self):
        """Bound the cache (every resolution / object count / slot / owner adds graphs with private pools): drop the least
        recently replayed stage.  Decoder and value stages read a key-encoder stage's outputs in place; when a key stage goes,
        the stages aliasing its buffers go with it (they would otherwise pay a copy per frame into buffers nobody produces
        into any more) and are re-captured on demand against the new key stage.  A restored-key slot (`restored_key_slot`) is
        such a producer too and is dropped the same way."""
        key, st = self._stages.popitem(last=False)
        if key[0] not in _KEY_PRODUCERS:
            return
        if key[0] == 'keyr':
            torch.cuda.synchronize()          # plain allocations, not a graph's pool: every stream is done with them before they are freed
        spans = [_span(t) for t in _flat_outputs(st[2])]
        inside = lambda t: isinstance(t, torch.Tensor) and any(a <= t.data_ptr() < b for a, b in spans)
        for k in [k for k, v in self._stages.items() if k[0] not in _KEY_PRODUCERS and any(inside(t) for t in v[1])]:
            del self._stages[k]

    def acquire_owner(self):
        """Owner token of an InferenceCore: its decoder stages advance ITS hidden state in place, so stages are keyed by
        owner.  Tokens are small integers recycled when a core dies (`release_owner`): the next core (eval.py builds one per
        video) takes over the dead core's captured stages - its fresh hidden state is copied into the stage's state buffer
        once and the core then continues on that buffer - instead of re-capturing every decoder graph per video."""
        if self._owner_free:
            # the smallest free token: the cores a caller builds in a fixed order (an ensemble's passes) get the same tokens call after
            # call, whatever order the previous call's cores died in, and so find their own captured stages again
            self._owner_free.sort(reverse=True)
            return self._owner_free.pop()
        self._owner_next += 1
        return self._owner_next

    def release_owner(self, token):
        self._owner_free.append(token)

    def _is_stage_output(self, t):
        """True when `t` lives inside a static output buffer of a key-encoder stage or of a restored-key slot (a whole output, or
        the slice of one frame of a batched pass): such tensors keep their address, so later stages may capture them in place."""
        a = t.data_ptr()
        for k, st in self._stages.items():
            if k[0] not in _KEY_PRODUCERS:
                continue
            for o in st[2]:
                if isinstance(o, torch.Tensor):
                    lo, hi = _span(o)
                    if lo <= a < hi:
                        return True
        return False

    def restored_key_slot(self, slot, frame_layout, batch):
        """Static buffers with the shapes, dtypes and batched layout of the outputs of the key stage `encode_key_nhwc(image4 of `batch`
        frames, with_skips=True, inline_skips=True, slot=...)`, for a caller that RESTORES those outputs from a cache instead of running
        the stage (InferenceCore.prefetch_cached).  `frame_layout`: (shape, dtype) of ONE frame's slice of key, shrinkage, selection,
        f16 and of every extra, in that order (what a cache entry holds).  Returns (key, shrinkage, selection, f16, f8, f4, extras) like
        the stage.  f8 and f4 are NOT stored: with the inlined skip convolutions no kernel reads them, so they are placeholders of the
        right shape without memory behind them (one element, stride 0).
        The buffers are stable (`_is_stage_output`): decoder and value stages captured for `slot` read them in place.  One slot per
        (slot, precision, geometry); it counts as a stage for MAX_STAGES and the LRU order, and takes its dependants with it."""
        self._need_weights()
        prec = self._call_precision or self.precision
        frame_layout = tuple((tuple(int(v) for v in shape), dtype) for shape, dtype in frame_layout)
        if len(frame_layout) < 6 or batch < 1:
            raise ValueError('restored_key_slot: the layout of key, shrinkage, selection, f16, skip8 and skip4 is required')
        full_key = ('keyr', slot, prec, int(batch), frame_layout)
        st = self._stages.lookup(full_key)
        if st is not None:
            return st.outputs
        dev = self.device
        bufs = [torch.empty((shape[0] * batch,) + shape[1:], dtype=dtype, device=dev) for shape, dtype in frame_layout]
        f16, skip8, skip4 = bufs[3], bufs[4], bufs[5]
        hole = torch.empty(1, dtype=f16.dtype, device=dev)
        f8 = hole.expand(batch, skip8.shape[1], skip8.shape[2], self._w['decoder.up_16_8.skip_conv'].cin)
        f4 = hole.expand(batch, skip4.shape[1], skip4.shape[2], self._w['decoder.up_8_4.skip_conv'].cin)
        out = (bufs[0], bufs[1], bufs[2], f16, f8, f4, tuple(bufs[4:]))
        self._stages.put(full_key, stages.Stage(None, [], out), evict=self._evict_lru)
        return out

    # ---- building blocks (NHWC) -----------------------------------------------------------------
    def _group_res(self, g, p, out=None, out_ld=None):
        """GroupResBlock, model/group_modules.py:44-52: conv2(relu(conv1(relu(g)))) + (downsample(g) | g)."""
        W = self._w
        if self.shared_transforms and (p + '.downsample') in W:
            # one input transform of g for both convolutions; the branch stays in the Winograd domain until conv2's output transform
            o, res = ops.conv2d_shared(g, [dict(cw=W[p + '.conv1'], relu_in=True, relu_out=True), dict(cw=W[p + '.downsample'])], defer=1)
            return ops.conv2d_folded(o, W[p + '.conv2'], res, out=out, out_ld=out_ld)
        o = ops.conv2d(g, W[p + '.conv1'], relu_in=True, relu_out=True)
        res = ops.conv2d(g, W[p + '.downsample']) if (p + '.downsample') in W else g
        return ops.conv2d(o, W[p + '.conv2'], res=res, out=out, out_ld=out_ld)

    def _shares_x(self, p, n_obj):
        """True when `_fusion(cat, p, x)` convolves the shared x half once (several objects, split weights uploaded)."""
        W = self._w
        return n_obj > 1 and (p + '.block1.conv1@x') in W and (p + '.block1.downsample@x') in W

    def _fusion(self, cat, p, x=None, pre=None):
        """FeatureFusionBlock, model/modules.py:31-41, on the already concatenated [x | g] tensor.  With several objects
        and `x` given ([1,h,w,1024], the shared f16 half of `cat`), block1's two 3x3 convolutions run the x half once
        and only the g half per object (saves 64 % / 80 % of block1's FLOPs for every object but the first)."""
        W = self._w
        b1 = p + '.block1'
        if x is not None and (pre is not None or self._shares_x(p, cat.shape[0])):
            xd = x.shape[3]
            gpart = cat[..., xd:]
            ld, cg = cat.shape[3], cat.shape[3] - xd
            # pre = (conv1@x(relu(x)), downsample@x(x)) already made in the batched key pass (prefetched frames)
            sx = pre[0] if pre is not None else ops.conv2d(x, W[b1 + '.conv1@x'], relu_in=True)
            dx = pre[1] if pre is not None else ops.conv2d(x, W[b1 + '.downsample@x'])
            if self.shared_transforms:
                o, res = ops.conv2d_shared(gpart, [dict(cw=W[b1 + '.conv1@g'], relu_in=True, relu_out=True, res=sx, res_broadcast=True),
                                                   dict(cw=W[b1 + '.downsample@g'], res=dx, res_broadcast=True)], in_ld=ld, cin=cg, defer=1)
                g = ops.conv2d_folded(o, W[b1 + '.conv2'], res)
            else:
                o = ops.conv2d(gpart, W[b1 + '.conv1@g'], relu_in=True, relu_out=True, res=sx, res_broadcast=True, in_ld=ld, cin=cg)
                res = ops.conv2d(gpart, W[b1 + '.downsample@g'], res=dx, res_broadcast=True, in_ld=ld, cin=cg)
                g = ops.conv2d(o, W[b1 + '.conv2'], res=res)
        else:
            g = self._group_res(cat, b1)
        g = ops.cbam_residual(g, self._cbam[p + '.attention'])
        return self._group_res(g, p + '.block2')

    def read_memory(self, query_key, query_selection, memory_key, memory_shrinkage, memory_value):
        """model/network.py:89-105 (training-time read: full softmax over all memory elements, dense readout).
        query_* B x CK x H x W, memory_key B x CK x T x H x W, memory_shrinkage B x 1 x T x H x W,
        memory_value B x num_objects x CV x T x H x W -> B x num_objects x CV x H x W."""
        from .memory_util import get_affinity, readout
        batch_size, num_objects = memory_value.shape[:2]
        mv = memory_value.flatten(start_dim=1, end_dim=2)
        affinity = get_affinity(memory_key, memory_shrinkage, query_key, query_selection)
        memory = readout(affinity, mv)
        return memory.view(batch_size, num_objects, self.value_dim, *memory.shape[-2:])

    # ---- hot path (NHWC) ------------------------------------------------------------------------
    def encode_key_nhwc(self, image4, need_sk=True, need_ek=True, with_skips=False, slot=0, inline_skips=False):
        """image4 [B,Hp,Wp,4] -> key [B*h*w,Ck], shrinkage [B*h*w]|None, selection|None, f16, f8, f4 (NHWC)
        [+ the decoder's skip convolutions of f8 / f4 (and the decoder fuser's f16 half) when inline_skips, else None, when with_skips].
        With graphs on, the returned tensors are the stage's static buffers: valid until the next call
        with the same `slot` (two slots let the key encoder of frame t+1 run while frame t is still being decoded)."""
        self._need_weights()
        inline = bool(with_skips and inline_skips)      # a prefetched pass also runs the decoder's skip convolutions
        # key-encoder graphs may run on a side stream: never share scratch with the decoder, nor with another network instance
        self._key_ws = f'@key{slot}#{self._scope}#'
        with ops.ws_scope(self._key_ws):
            out = self._run_stage('key', (need_sk, need_ek, inline, slot), [image4],
                                  lambda im: self._encode_key_eager(im, need_sk, need_ek, inline))
        if with_skips:
            return out if inline else tuple(out) + (None,)
        return out[:6]

    def _encode_key_eager(self, image4, need_sk, need_ek, inline_skips=False):
        W = self._w
        x = ops.conv2d(image4, W['key_encoder.conv1'], relu_out=True)       # the stem reads the fp32 image in every mode
        x = ops.maxpool3x3s2(x, out_dtype=ops.act_dtype())                # fp16 loop: activations become halfs here
        f4, pre = self._stage(x, 'key_encoder.res2', 3, self._bottleneck, then='key_encoder.layer2.0.conv1')
        f8, pre = self._stage(f4, 'key_encoder.layer2', 4, self._bottleneck, pre=pre, then='key_encoder.layer3.0.conv1')
        f16 = self._stage(f8, 'key_encoder.layer3', 6, self._bottleneck, pre=pre)
        B, h, w, _ = f16.shape
        ld = _pad4(2 * self.key_dim + 1)
        proj = torch.empty((B, h, w, ld), dtype=torch.float32, device=f16.device)
        b1 = 'decoder.fuser.block1'
        split_x = (b1 + '.conv1@x') in W and (b1 + '.downsample@x') in W
        fx = None
        if inline_skips and split_x and self.shared_transforms:
            # the three 3x3 layers that read f16 behind one input transform (two V: raw for key_proj and downsample@x, relu for conv1@x)
            _, *fx = ops.conv2d_shared(f16, [dict(cw=W['key_proj'], out=proj, out_ld=ld, out_dtype=torch.float32),
                                             dict(cw=W[b1 + '.conv1@x'], relu_in=True), dict(cw=W[b1 + '.downsample@x'])])
        else:
            ops.conv2d(f16, W['key_proj'], out=proj, out_ld=ld, out_dtype=torch.float32)     # keys / shrinkage / selection are fp32 in every mode
        key, shr, sel = ops.key_post(proj, self.key_dim, need_sk, need_ek)
        if inline_skips:                      # same stream: f8 / f4 only depend on the image (model/modules.py:186,231-232)
            extras = (ops.conv2d(f8, W['decoder.up_16_8.skip_conv']), ops.conv2d(f4, W['decoder.up_8_4.skip_conv']))
            if split_x:
                # FeatureFusionBlock convolves cat([f16, readout, hidden]) (model/modules.py:31-41): W * cat = W_x * f16 + W_g * [readout |
                # hidden], and the f16 half (1024 of 1600 input channels of block1's two 3x3 convolutions) depends on the frame only -
                # so it is convolved HERE, in the batched pass on the side stream, and enters the decoder as a residual
                extras += tuple(fx) if fx is not None else (ops.conv2d(f16, W[b1 + '.conv1@x'], relu_in=True), ops.conv2d(f16, W[b1 + '.downsample@x']))
            return key, shr, sel, f16, f8, f4, extras
        return key, shr, sel, f16, f8, f4

    def encode_value_nhwc(self, image4, f16, hidden, masks, is_deep_update=True, slot=0):
        """image4 [1,Hp,Wp,4], f16 [1,h,w,1024], hidden [K,h,w,Ch], masks [K,Hp,Wp] -> value [K,h,w,Cv], hidden."""
        self._need_weights()
        value, new_hidden = self._run_stage('value', (bool(is_deep_update), slot), [image4, f16, hidden, masks],
                                            lambda a, b, c, d: self._encode_value_eager(a, b, c, d, is_deep_update),
                                            alias=(1,) if self._is_stage_output(f16) else ())
        if self.use_graphs and new_hidden is not None and new_hidden is not hidden:
            new_hidden = new_hidden.clone()                 # the hidden state outlives the stage's static buffer
        return value, new_hidden

    def _encode_value_eager(self, image4, f16, hidden, masks, is_deep_update):
        W = self._w
        x = ops.pack_value_input(image4, masks)
        act = ops.act_dtype()
        g = ops.conv2d(x, W['value_encoder.conv1'], relu_out=True)     # relu and max-pool commute (modules.py:137-138)
        g = ops.maxpool3x3s2(g, out_dtype=act)
        g = self._stage(g, 'value_encoder.layer1', 2, self._basic)
        g = self._stage(g, 'value_encoder.layer2', 2, self._basic)
        g = self._stage(g, 'value_encoder.layer3', 2, self._basic)
        K, h, w, cg = g.shape
        cat = torch.empty((K, h, w, f16.shape[3] + cg), dtype=act, device=g.device)
        if not self._shares_x('value_encoder.fuser', K):
            ops.copy_channels(f16, cat, 0)
        ops.copy_channels(g, cat, f16.shape[3])
        value = self._fusion(cat, 'value_encoder.fuser', x=f16)
        if is_deep_update and self.hidden_dim > 0:
            cat2 = torch.empty((K, h, w, self.value_dim + self.hidden_dim), dtype=act, device=g.device)
            ops.copy_channels(value, cat2, 0)
            ops.copy_channels(hidden, cat2, self.value_dim)
            values = ops.conv2d(cat2, W['value_encoder.hidden_reinforce.transform'])
            hidden = ops.gru_gate(values, hidden)
        return value, hidden

    def encode_value_frames_nhwc(self, image4, f16, masks):
        """Value encoder over SEVERAL frames at once (the batched permanent-memory preload: an annotated frame and its
        augmentations, inference/run_on_video.py:59-66,231-242): image4 [B,Hp,Wp,4], f16 [B,h,w,1024], masks = list of B tensors
        [K,Hp,Wp] -> value [B*K,h,w,Cv] (frame-major).  No deep update (put_to_permanent_memory never makes one), eager,
        in the network's full-precision arithmetic."""
        self._need_weights()
        W = self._w
        B = image4.shape[0]
        K = masks[0].shape[0]
        with ops.precision('fp32'):
            x = torch.empty((B * K,) + tuple(image4.shape[1:3]) + (8,), dtype=torch.float32, device=image4.device)
            for b in range(B):
                x[b * K:(b + 1) * K].copy_(ops.pack_value_input(image4[b:b + 1], masks[b]))
            g = ops.conv2d(x, W['value_encoder.conv1'], relu_out=True)
            g = ops.maxpool3x3s2(g)
            g = self._stage(g, 'value_encoder.layer1', 2, self._basic)
            g = self._stage(g, 'value_encoder.layer2', 2, self._basic)
            g = self._stage(g, 'value_encoder.layer3', 2, self._basic)
            _, h, w, cg = g.shape
            cat = torch.empty((B * K, h, w, f16.shape[3] + cg), dtype=torch.float32, device=g.device)
            for b in range(B):                        # each frame's own f16 in front of its objects' features
                ops.copy_channels(f16[b:b + 1], cat[b * K:(b + 1) * K], 0)
            ops.copy_channels(g, cat, f16.shape[3])
            return self._fusion(cat, 'value_encoder.fuser', x=None)

    def new_decoder_input(self, K, h, w, device, slot=0, owner=0, h_out=None, has_skips=None, static_only=False, out_hw=None, pad_tl=None):
        """[K,h,w, 1024+Cv+Ch] buffer; the readout kernel writes channels [1024, 1024+Cv) in place.
        Once the matching decoder stage is captured this is its static input buffer (no copy before the replay).
        static_only: None instead of a fresh buffer when no captured stage matches.  out_hw / pad_tl: the remaining components of the
        stage key (two resolutions that pad to one h x w have stages of their own)."""
        shape = (K, h, w, 1024 + self.value_dim + self.hidden_dim)
        prec = self._call_precision or self.precision
        if self.use_graphs and not ops.eager_only():
            for k, st in self._stages.items():
                if k[0] != 'segment' or k[2] != (self._call_precision or self.precision) or k[1][-2] != slot or k[1][-1] != owner \
                        or tuple(st[1][3].shape) != shape:
                    continue
                if (h_out is not None and k[1][2] != bool(h_out)) or (has_skips is not None and k[1][3] != bool(has_skips)):
                    continue
                if (out_hw is not None and k[1][0] != tuple(out_hw)) or (pad_tl is not None and k[1][1] != tuple(pad_tl)):
                    continue
                return st[1][3]
        if static_only:
            return None
        return torch.empty(shape, dtype=torch.float16 if prec == 'fp16' else torch.float32, device=device)

    def _zero_scratch(self, shape, device, dtype=torch.float32):
        """Persistent zero-initialised buffer (allocated outside any capture): kernels overwrite only its data channels, the
        padding channels stay zero - no per-frame fill kernel."""
        key = (tuple(shape), str(device), dtype)
        buf = self._zeros.get(key)
        if buf is None:
            buf = torch.zeros(shape, dtype=dtype, device=device)
            self._zeros[key] = buf
        return buf

    def segment_nhwc(self, f16, f8, f4, cat16, hidden, out_hw, pad_tl, h_out=True, skips=None, slot=0, owner=0):
        """Decoder + soft aggregation.  cat16 holds the memory readout at channels [1024,1024+Cv).
        Returns new_hidden|None, prob [K+1,H,W] (unpadded), prob_padded [K+1,Hp,Wp].
        The hidden state is updated IN PLACE (`new_hidden is hidden` when h_out): the captured stage reads and writes the
        caller's state tensor (`owner` keys the stage so that two cores sharing one network never share a state buffer)."""
        self._need_weights()
        K, h, w, _ = cat16.shape
        g4d = None
        if h_out and self.hidden_dim > 0:
            c4 = self._w['decoder.pred'].cin
            half = (self._call_precision or self.precision) == 'fp16'
            gf = self._w.get('decoder.hidden_update.g_fused')
            if gf is not None and not half:
                # the concatenated input of the fused hidden-update convolution [g16 | area(g8) | area(g4), area(logits), zero padding]
                g4d = self._zero_scratch((K, h, w, gf.cin), cat16.device, torch.float32)
            else:
                g4d = self._zero_scratch((K, h, w, (c4 + 1 + 7) // 8 * 8 if half else _pad4(c4 + 1)), cat16.device,
                                         torch.float16 if half else torch.float32)
        if skips is not None and len(skips) >= 4:
            out = self._run_stage('segment', (tuple(out_hw), tuple(pad_tl), bool(h_out), True, slot, owner),
                                  [f16, f8, f4, cat16, hidden, skips[0], skips[1], skips[2], skips[3]],
                                  lambda a, b, c, d, e, s8, s4, sx, dx: self._segment_eager(a, b, c, d, e, h_out, (s8, s4, sx, dx), g4d),
                                  alias=(0, 1, 2, 4, 5, 6, 7, 8) if self._is_stage_output(f16) else (4,), mutates=(4,))
        elif skips is not None:
            out = self._run_stage('segment', (tuple(out_hw), tuple(pad_tl), bool(h_out), True, slot, owner),
                                  [f16, f8, f4, cat16, hidden, skips[0], skips[1]],
                                  lambda a, b, c, d, e, s8, s4: self._segment_eager(a, b, c, d, e, h_out, (s8, s4), g4d),
                                  alias=(0, 1, 2, 4, 5, 6) if self._is_stage_output(f16) else (4,), mutates=(4,))
        else:
            out = self._run_stage('segment', (tuple(out_hw), tuple(pad_tl), bool(h_out), False, slot, owner),
                                  [f16, f8, f4, cat16, hidden],
                                  lambda a, b, c, d, e: self._segment_eager(a, b, c, d, e, h_out, None, g4d),
                                  alias=(0, 1, 2, 4) if self._is_stage_output(f16) else (4,), mutates=(4,))
        new_hidden, logits = out
        # soft aggregation outside the captured stage: prob / prob_padded are fresh tensors the caller may keep (no clone)
        H, Wd = out_hw
        prob, prob_padded = ops.logits_to_prob(logits.view(K, 4 * h, 4 * w), H, Wd, pad_tl[0], pad_tl[1])
        return new_hidden, prob, prob_padded

    def _segment_eager(self, f16, f8, f4, cat16, hidden, h_out, skips=None, g4d=None):
        W = self._w
        K, h, w, _ = cat16.shape
        hd = self.hidden_dim
        pre = (skips[2], skips[3]) if (skips is not None and len(skips) >= 4) else None
        if pre is None and not self._shares_x('decoder.fuser', K):
            ops.copy_channels(f16, cat16, 0)               # with several objects the f16 half is convolved once (see _fusion)
        if hd > 0:
            ops.copy_channels(hidden, cat16, 1024 + self.value_dim)
        g16 = self._fusion(cat16, 'decoder.fuser', x=f16, pre=pre)
        skip8 = skips[0] if skips is not None else ops.conv2d(f8, W['decoder.up_16_8.skip_conv'])
        g8 = self._group_res(ops.upsample2x_add(g16, skip8), 'decoder.up_16_8.out_conv')
        skip4 = skips[1] if skips is not None else ops.conv2d(f4, W['decoder.up_8_4.skip_conv'])
        g4 = self._group_res(ops.upsample2x_add(g8, skip4), 'decoder.up_8_4.out_conv')
        gf = W.get('decoder.hidden_update.g_fused') if h_out and hd > 0 else None
        if self.fused_tail and gf is not None and g4d is not None and g4d.shape[3] == gf.cin and K * h * w >= self.fused_tail_min_pixels \
                and hidden.shape[3] == hd:
            # mask head, HiddenUpdater input and the hidden half of `cat` in one launch that reads g4 once (the same bits as the calls below)
            mid = gf.cout
            cat = torch.empty((K, h, w, mid + hd), dtype=torch.float32, device=g4.device)
            if ops.mask_head_gather_ok(g16, g8, g4, W['decoder.pred'], hidden, g4d, cat, mid):
                logits = ops.mask_head_gather(g16, g8, g4, W['decoder.pred'], hidden, g4d, cat, mid)
                ops.conv2d(g4d, gf, out=cat, out_ld=cat.shape[3])           # writes the disjoint [:mid]
                values = ops.conv2d(cat, W['decoder.hidden_update.transform'])
                return ops.gru_gate(values, hidden, out=hidden), logits
        logits = ops.conv2d(g4, W['decoder.pred'], relu_in=True, out_dtype=torch.float32)          # [K,4h,4w,1], fp32 in every mode
        new_hidden = None
        if h_out and hd > 0:
            c4 = g4.shape[3]
            if g4d is None:
                g4d = self._zero_scratch((K, h, w, _padc(c4 + 1)), g4.device, ops.act_dtype())
            if gf is not None and g4d.shape[3] == gf.cin and g4d.dtype == torch.float32:
                # one pointwise convolution over [g16 | area(g8) | area(g4), area(logits)] (see _upload)
                c16, c8, ld = g16.shape[3], g8.shape[3], g4d.shape[3]
                if all(t.is_contiguous() for t in (g16, g8, g4, logits)):
                    ops.hidden_update_gather(g16, g8, g4, logits, g4d)        # one launch (round 6; the same bits as the four below)
                else:
                    ops.copy_channels(g16, g4d, 0)
                    ops.area_downsample(g8, 2, out=g4d, out_ld=ld, out_off=c16)
                    ops.area_downsample(g4, 4, out=g4d, out_ld=ld, out_off=c16 + c8)
                    ops.area_downsample(logits, 4, out=g4d, out_ld=ld, out_off=c16 + c8 + c4)
                mid = gf.cout
                cat = torch.empty((K, h, w, mid + hd), dtype=ops.act_dtype(), device=g4.device)
                ops.conv2d(g4d, gf, out=cat, out_ld=cat.shape[3], plan=self._unpadded_g_fused_plan(gf, K, h, w, cat.shape[3]))
            else:
                ops.area_downsample(g4, 4, out=g4d, out_ld=g4d.shape[3])
                ops.area_downsample(logits, 4, out=g4d, out_ld=g4d.shape[3], out_off=c4)
                g8d = ops.area_downsample(g8, 2)
                t = ops.conv2d(g16, W['decoder.hidden_update.g16_conv'])
                t = ops.conv2d(g8d, W['decoder.hidden_update.g8_conv'], res=t)
                mid = t.shape[3]
                cat = torch.empty((K, h, w, mid + hd), dtype=ops.act_dtype(), device=g4.device)
                ops.conv2d(g4d, W['decoder.hidden_update.g4_conv'], res=t, out=cat, out_ld=cat.shape[3])
            ops.copy_channels(hidden, cat, mid)
            values = ops.conv2d(cat, W['decoder.hidden_update.transform'])
            new_hidden = ops.gru_gate(values, hidden, out=hidden)          # in place: the state tensor itself advances
        return new_hidden, logits

    @staticmethod
    def _unpadded_g_fused_plan(gf, K, h, w, out_ld):
        """The plan table lists the fused hidden-update convolution under its padded Cin (fused_tail, the default).  With the padding
        switched off the layer runs under that same entry - the same tile and split-K, so the same summation order: the switch
        changes no bit, and both of its sides are measured under the tuned plan.  None: the usual choice (conv_plan.choose)."""
        from . import conv_plan
        if gf.cin % 32 == 0 or ops._PRECISION != 'fp32' or conv_plan.CONV_FORM or conv_plan.AUTOTUNE:
            return None
        cp = (gf.cin + 31) // 32 * 32
        return conv_plan.FP32.get(f'{K}x{h}x{w}x{cp}/{cp}->{gf.cout}/{out_ld} k1s1p0 r000')

    # ---- reference-shaped wrappers (NCHW in / out) ----------------------------------------------
    @staticmethod
    def _as_nhwc(t):
        p = t.permute(0, 2, 3, 1)
        return p if p.is_contiguous() else ops.nchw_to_nhwc(t)

    def encode_key(self, frame, need_sk=True, need_ek=True):
        """model/network.py:40-70 for 4-D input [B,3,H,W] (H, W multiples of 16)."""
        if frame.dim() != 4:
            raise NotImplementedError
        B, _, H, Wd = frame.shape
        image4 = torch.cat([ops.pack_image(frame[b], H, Wd, 0, 0) for b in range(B)], 0) if B > 1 \
            else ops.pack_image(frame[0], H, Wd, 0, 0)
        key, shr, sel, f16, f8, f4 = self.encode_key_nhwc(image4, need_sk, need_ek)
        h, w = f16.shape[1], f16.shape[2]
        nchw = lambda t: t.permute(0, 3, 1, 2)
        key = nchw(key.view(B, h, w, self.key_dim))
        shr = shr.view(B, 1, h, w) if shr is not None else None
        sel = nchw(sel.view(B, h, w, self.key_dim)) if sel is not None else None
        self._last_image4 = (frame.data_ptr(), image4)
        return key, shr, sel, nchw(f16), nchw(f8), nchw(f4)

    def encode_value(self, frame, image_feat_f16, h16, masks, is_deep_update=True):
        """model/network.py:72-85: frame [1,3,H,W], f16 [1,1024,h,w], h16 [1,K,Ch,h,w], masks [1,K,H,W]."""
        cached = getattr(self, '_last_image4', None)
        if cached is not None and cached[0] == frame.data_ptr():
            image4 = cached[1]
        else:
            image4 = ops.pack_image(frame[0], frame.shape[2], frame.shape[3], 0, 0)
        f16 = self._as_nhwc(image_feat_f16)
        hidden = self._as_nhwc(h16[0]) if h16 is not None else None
        m = masks[0] if masks[0].is_contiguous() else masks[0].contiguous()
        value, hidden = self.encode_value_nhwc(image4, f16, hidden, m, is_deep_update)
        value = value.permute(0, 3, 1, 2).unsqueeze(0)
        hidden = hidden.permute(0, 3, 1, 2).unsqueeze(0) if hidden is not None else None
        return value, hidden

    def segment(self, multi_scale_features, memory_readout, hidden_state, selector=None, h_out=True, strip_bg=True):
        """model/network.py:107-120.  Returns (hidden, None, prob): the aggregated logits are a training-only
        output of the reference and are not produced here."""
        if selector is not None:
            raise NotImplementedError('selector is a training-time argument (model/trainer.py) - out of scope')
        f16, f8, f4 = [self._as_nhwc(t) for t in multi_scale_features]
        ro = self._as_nhwc(memory_readout[0])                      # [K,h,w,Cv]
        K, h, w, _ = ro.shape
        hidden = self._as_nhwc(hidden_state[0]) if hidden_state is not None else None
        cat16 = self.new_decoder_input(K, h, w, ro.device)
        ops.copy_channels(ro, cat16, 1024)
        if hidden is not None and hidden_state is not None and hidden.data_ptr() == hidden_state.data_ptr():
            hidden = hidden.clone()                     # the reference-shaped call must not edit the caller's tensor
        new_hidden, _, prob = self.segment_nhwc(f16, f8, f4, cat16, hidden, (16 * h, 16 * w), (0, 0), h_out)
        if new_hidden is not None:
            new_hidden = new_hidden.clone()             # the stage's state buffer is reused by the next call
        prob = prob.unsqueeze(0)
        if strip_bg:
            prob = prob[:, 1:]
        new_hidden = new_hidden.permute(0, 3, 1, 2).unsqueeze(0) if new_hidden is not None else None
        return new_hidden, None, prob

    def forward(self, mode, *args, **kwargs):
        if mode == 'encode_key':
            return self.encode_key(*args, **kwargs)
        if mode == 'encode_value':
            return self.encode_value(*args, **kwargs)
        if mode == 'segment':
            return self.segment(*args, **kwargs)
        raise NotImplementedError(mode)

    __call__ = forward
