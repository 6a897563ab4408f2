"""Click-to-mask on MI355X: the reference's f-BRS click network and its NoBRS predictor over HIP kernels.

    python -m xmem2_amd.click --images DIR --clicks FILE.json --out DIR [--prev-masks DIR] [--model fbrs.pth | --synthetic-seed N]
                              [--num-objects K] [--brs-mode NoBRS|f-BRS-B|f-BRS-C]

``ClickNet`` mirrors ``get_deeplab_model(backbone='resnet50', deeplab_ch)`` (inference/interact/fbrs/model/is_deeplab_model.py:9-66):
click distance maps and the rgb_conv input MLP, a ResNet-50-v1s at output stride 8 (fbrs/model/modeling/resnetv1b.py), the
DeepLabV3+ of fbrs/model/modeling/deeplab_v3.py with separable convolutions, and the SepConvHead (basic_blocks.py:27-54).  As in
s2m.py nothing is an nn.Module: BatchNorm is folded at load time, activations are NHWC, every operation is a HIP kernel (ops), and
the forward is captured once per working geometry as a HIP graph and replayed.

``NoBRSPredictor`` is BasePredictor (fbrs/inference/predictors/base.py) with its transforms: ZoomIn and LimitLongestSide are ported
as host state machines over device tensors; SigmoidForPred and AddHorizontalFlip live inside the input and output kernels
(ops.click_input builds both samples, ops.click_prob averages the logits and applies the sigmoid).  ``FBRSController`` keeps the
reference's surface (inference/interact/fbrs_controller.py) with the NoBRS predictor: ``brs_mode`` other than 'NoBRS' raises
NotImplementedError there.  The back-propagating refinement of 'f-BRS-B' / 'f-BRS-C' is click_brs.py (FeatureBRSController).

The JSON of the command line maps a frame number to a list of {"object": k, "x": col, "y": row, "positive": bool}.  The objects of a
frame are processed one after the other (a fresh anchor per object), each committed as ClickInteraction.predict does
(interaction.py:247-254), and the argmax is written as a palette PNG named after the frame, so the output directory serves as
the masks directory of run_on_video.
"""
import argparse
import json
import os
import sys
from collections import namedtuple

import numpy as np
import torch

from . import ops, stages
from .arch import BN_EPS, click_state_dict_spec
from .hipnet import HipNet, check_state_dict

NORM_RADIUS = 260.0             # fbrs_controller.py:8
ASPP_RATES = (12, 24, 36)       # deeplab_v3.py:43
HARD_TEMPERATURE = 1000.0       # aggregate_wbg(hard=True), interaction.py:45-47
CLICK_CAPACITY = 64             # clicks per polarity of a captured graph's click buffer (grows, with a recapture, beyond that)
MAX_GEOMETRIES = 8              # captured graphs kept per network (least recently used dropped)
BRS_MODES = ('f-BRS-A', 'f-BRS-B', 'f-BRS-C', 'RGB-BRS', 'DistMap-BRS')

Click = namedtuple('Click', ['is_positive', 'coords'])      # coords = (row, col), fbrs/inference/clicker.py:7


def state_dict_spec(deeplab_ch=128):
    """Names and shapes of the reference's click-network state dict (413 tensors, state_dict order)."""
    return click_state_dict_spec(deeplab_ch)


def _ceil_half(n):
    return (n - 1) // 2 + 1


def run_click_stage(cache, forward, image, points, cap, with_flip):
    """The stage of `cache` (a StageCache) for the geometry of `image` [3,h,w] and `with_flip`, captured from forward(image, clicks,
    counts, with_flip) when the cache does not hold it, replayed on `image` and `points` -> its static output.
    points [2n,2] (row, col) as get_points_nd lays one clicks list out (n positive then n negative entries, (-1, -1) = padding) fill the
    stage's click buffers: clicks [2,cap,2], padded with -1, and counts [2] = (n, n)."""
    pts = np.asarray(points, dtype=np.float32).reshape(2, -1, 2)
    n = pts.shape[1]
    host = np.full((2, cap, 2), -1.0, np.float32)
    host[:, :n] = pts
    clicks, counts = torch.from_numpy(host), torch.from_numpy(np.array([n, n], np.int32))
    key = (int(image.shape[-2]), int(image.shape[-1]), bool(with_flip))
    st = cache.lookup(key)
    if st is None:
        dev = image.device
        st = cache.put(key, stages.capture(lambda *a: forward(*a, with_flip), (image.clone(), clicks.to(dev), counts.to(dev))))
    return st.replay((image, clicks, counts))


def grown_capacity(cap, n):
    """`cap` doubled until it holds n clicks per polarity.  The caller drops its captured graphs when it grows: they hold the old buffers."""
    while cap < n:
        cap *= 2
    return cap


class ClickNet(HipNet):
    """DistMapsModel(DeepLabV3Plus(resnet50), SepConvHead) on HIP kernels (fp32)."""

    _synthetic = 'synthetic_click_state_dict'
    ignored_keys = ('aspp_dropout',)

    def __init__(self, model_path=None, device=None):
        super().__init__(torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device()),
                         max_stages=lambda: MAX_GEOMETRIES)
        self.deeplab_ch = 128
        self._graphs = self._stages    # (h, w, with_flip) -> Stage, least recently used first
        self._brs = {}                 # insertion mode -> the f-BRS engine with its own captured graphs (click_brs.engine_for)
        self._cap = CLICK_CAPACITY
        if model_path is not None:
            self.load_weights(model_path)

    # ---- weights ----------------------------------------------------------------------------------
    def load_state_dict(self, sd, strict=True):
        """As load_deeplab_is_model (fbrs/inference/utils.py:67-100): the backbone is identified by its parameter count, deeplab_ch is
        read from aspp.project.0.weight, `aspp_dropout` and num_batches_tracked are ignored."""
        if any('feature_extractor.stage2.0.branches' in k for k in sd):
            raise NotImplementedError('ClickNet: this is an HRNet click checkpoint; only the DeepLabV3+ / ResNet-50 model is built')
        n_backbone = len([k for k in sd if 'feature_extractor.backbone' in k and 'num_batches_tracked' not in k])
        if not 181 < n_backbone <= 276:
            kind = 'resnet34' if n_backbone <= 181 else ('resnet101' if n_backbone <= 531 else 'unknown')
            raise NotImplementedError(f'ClickNet: the checkpoint has {n_backbone} backbone tensors ({kind}); only resnet50 (182..276) is built')
        proj = [v for k, v in sd.items() if 'aspp.project.0.weight' in k]
        if len(proj) != 1:
            raise RuntimeError('ClickNet: the checkpoint has no aspp.project.0.weight to read deeplab_ch from')
        ch = int(proj[0].shape[0])
        if ch % 8:
            raise NotImplementedError(f'ClickNet: deeplab_ch = {ch} is not a multiple of 8')
        if strict:
            check_state_dict(sd, state_dict_spec(ch), 'ClickNet', self.ignored_keys)
        self.deeplab_ch = ch
        self._adopt(sd)

    def _weights_replaced(self):
        super()._weights_replaced()
        self._brs.clear()

    def _separable(self, W, key, prefix):
        """SeparableConv2d: depthwise weights [C,1,3,3] -> [9][C]; the pointwise convolution carries the BatchNorm (and ReLU)."""
        dw = self._sd[prefix + '.body.0.weight'].float()
        W[key + '.dw'] = dw.reshape(dw.shape[0], 9).t().contiguous().to(self.device)
        W[key + '.pw'] = self._conv_w(prefix + '.body.1', prefix + '.body.2', 1, 0)
        # the adjoints f-BRS back-propagates through (click_brs.py): the taps reversed, the BN-folded pointwise matrix transposed
        W[key + '.dwT'] = W[key + '.dw'].flip(0).contiguous()
        W[key + '.pwT'] = self._transposed(W[key + '.pw'])

    @staticmethod
    def _transposed(cw):
        """The adjoint of a pointwise layer as a pointwise layer: (scale[o] w[o][i])^T with scale 1 and shift 0."""
        wt = (cw.w[:, 0, 0, :cw.cin_true] * cw.scale[:, None]).t().contiguous()
        dev = wt.device
        return ops.ConvWeights(wt.reshape(cw.cin_true, 1, 1, cw.cout), torch.ones(cw.cin_true, device=dev),
                               torch.zeros(cw.cin_true, device=dev), 1, 0)

    def _upload(self):
        sd, W = self._sd, {}
        # rgb_conv (is_deeplab_model.py:36-41): Conv(5, 8) -> LeakyReLU -> BN -> Conv(8, 3); the BN is folded into the second convolution
        d = lambda k: sd[k].double()
        s = d('rgb_conv.2.weight') / torch.sqrt(d('rgb_conv.2.running_var') + BN_EPS)
        t = d('rgb_conv.2.bias') - d('rgb_conv.2.running_mean') * s
        w2 = d('rgb_conv.3.weight').reshape(3, 8)
        W['rgb_conv'] = torch.cat([d('rgb_conv.0.weight').reshape(40), d('rgb_conv.0.bias'), (w2 * s[None]).reshape(24),
                                   d('rgb_conv.3.bias') + w2 @ t]).float().contiguous().to(self.device)
        bb = 'feature_extractor.backbone.'
        W['stem.0'] = self._conv_w(bb + 'conv1.0', bb + 'conv1.1', 2, 1)        # 3 channels, padded to 4 of the packed 8
        W['stem.3'] = self._conv_w(bb + 'conv1.3', bb + 'conv1.4', 1, 1)
        W['stem.6'] = self._conv_w(bb + 'conv1.6', bb + 'bn1', 1, 1)
        # resnetv1b.py:133-141, 153-195: the stride sits on conv2; layer3 / layer4 trade their stride for dilation 2 / 4, and the
        # first block of each runs at half that dilation
        for name, stride, dils in (('layer1', 1, (1, 1, 1)), ('layer2', 2, (1, 1, 1, 1)), ('layer3', 1, (1, 2, 2, 2, 2, 2)),
                                   ('layer4', 1, (2, 4, 4))):
            for b, dil in enumerate(dils):
                p, st = f'{bb}{name}.{b}', (stride if b == 0 else 1)
                W[p + '.conv1'] = self._conv_w(p + '.conv1', p + '.bn1', 1, 0)
                cw = W[p + '.conv2'] = self._conv_w(p + '.conv2', p + '.bn2', st, dil)
                if dil > 1:
                    cw.dilation, cw.wu, cw.wu_f16 = dil, None, None
                W[p + '.conv3'] = self._conv_w(p + '.conv3', p + '.bn3', 1, 0)
                if (p + '.downsample.0.weight') in sd:
                    W[p + '.downsample'] = self._conv_w(p + '.downsample.0', p + '.downsample.1', st, 0)
        fe = 'feature_extractor.'
        W['skip_project'] = self._conv_w(fe + 'skip_project.skip_project.0', fe + 'skip_project.skip_project.1', 1, 0)
        W['aspp.0'] = self._conv_w(fe + 'aspp.concurent.0.0', fe + 'aspp.concurent.0.1', 1, 0)
        for i, rate in enumerate(ASPP_RATES, 1):
            cw = W[f'aspp.{i}'] = self._conv_w(f'{fe}aspp.concurent.{i}.0', f'{fe}aspp.concurent.{i}.1', 1, rate)
            cw.dilation, cw.wu, cw.wu_f16 = rate, None, None
        W['aspp.pool'] = self._conv_w(fe + 'aspp.concurent.4.gap.1', fe + 'aspp.concurent.4.gap.2', 1, 0)
        W['aspp.project'] = self._conv_w(fe + 'aspp.project.0', fe + 'aspp.project.1', 1, 0)
        self._separable(W, 'dl.0', fe + 'head.block.0')
        self._separable(W, 'dl.1', fe + 'head.block.1')
        W['dl.2'] = self._conv_w(fe + 'head.block.2', None, 1, 0)
        W['dl.2T'] = self._transposed(W['dl.2'])
        self._separable(W, 'head.0', 'head.layers.0')
        self._separable(W, 'head.1', 'head.layers.1')
        W['head.2'] = self._conv_w('head.layers.2', None, 1, 0)
        h2 = W['head.2']
        W['head.2T'] = (h2.w[0, 0, 0, :h2.cin_true] * h2.scale[0]).contiguous()       # one output channel: its adjoint is an outer product
        self._w = W

    # ---- forward (NHWC) -------------------------------------------------------------------------
    def features(self, x):
        """x [B,H,W,8] (ops.click_input) -> dict of NHWC tensors: c1 [B,h4,w4,256] (layer1), aspp [B,h8,w8,ch] (the ASPP output) and
        head_input [B,h4,w4,ch+32] = cat(upsample(aspp), skip_project(c1)), the tensor f-BRS-B's `after_aspp` scale and bias act on.
        Odd sizes are legal: h4 = ceil(ceil(H/2)/2), h8 = ceil(h4/2)."""
        self._need_weights()
        W, ch = self._w, self.deeplab_ch
        bb = 'feature_extractor.backbone.'
        x = ops.conv2d(x, W['stem.0'], relu_out=True, in_ld=x.shape[3], cin=W['stem.0'].cin)
        x = ops.conv2d(x, W['stem.3'], relu_out=True)
        x = ops.conv2d(x, W['stem.6'], relu_out=True)
        x = ops.maxpool3x3s2(x)
        c1 = self._stage(x, bb + 'layer1', 3, self._bottleneck)
        x = self._stage(c1, bb + 'layer2', 4, self._bottleneck)
        x = self._stage(x, bb + 'layer3', 6, self._bottleneck)
        x = self._stage(x, bb + 'layer4', 3, self._bottleneck)
        B, h, w, c = x.shape
        cat = torch.empty((B, h, w, 5 * ch), dtype=torch.float32, device=x.device)
        for i in range(4):
            ops.conv2d(x, W[f'aspp.{i}'], relu_out=True, out=cat[..., ch * i:ch * (i + 1)], out_ld=5 * ch)
        pooled = ops.conv2d(ops.channel_mean(x).view(B, 1, 1, c), W['aspp.pool'], relu_out=True)
        ops.broadcast_channels(pooled.view(B, ch), cat[..., 4 * ch:5 * ch])       # align_corners upsample of one pixel = that pixel
        aspp = ops.conv2d(cat, W['aspp.project'], relu_out=True)                  # Dropout is the identity in eval
        h4, w4 = c1.shape[1], c1.shape[2]
        head_input = torch.empty((B, h4, w4, ch + 32), dtype=torch.float32, device=x.device)
        ops.resize_bilinear_ac_nhwc(aspp, (h4, w4), out=head_input[..., 0:ch])
        ops.conv2d(c1, W['skip_project'], relu_out=True, out=head_input[..., ch:ch + 32], out_ld=ch + 32)
        return dict(c1=c1, aspp=aspp, head_input=head_input)

    def head(self, head_input):
        """head_input [B,h4,w4,ch+32] -> logits [B,h4,w4,1]: _DeepLabHead (deeplab_v3.py:99-112), then SepConvHead."""
        return self.sep_conv_head(self.deeplab_head(head_input))

    def deeplab_head(self, head_input, kept=None):
        """_DeepLabHead: head_input [B,h4,w4,ch+32] -> [B,h4,w4,ch], the tensor f-BRS-C's `after_deeplab` scale and bias act on.  `kept`
        (a list) receives the two ReLU outputs the backward pass gates with."""
        self._need_weights()
        W = self._w
        x = head_input
        for key in ('dl.0', 'dl.1'):
            x = ops.conv2d(ops.depthwise3x3(x, W[key + '.dw']), W[key + '.pw'], relu_out=True)
            if kept is not None:
                kept.append(x)
        return ops.conv2d(x, W['dl.2'])

    def sep_conv_head(self, x, kept=None, out=None):
        """SepConvHead: [B,h4,w4,ch] -> logits [B,h4,w4,1] (into `out` when given); `kept` as in deeplab_head."""
        self._need_weights()
        W = self._w
        for key in ('head.0', 'head.1'):
            x = ops.conv2d(ops.depthwise3x3(x, W[key + '.dw']), W[key + '.pw'], relu_out=True)
            if kept is not None:
                kept.append(x)
        return ops.conv2d(x, W['head.2'], out=out, out_ld=None if out is None else 1)

    def _forward(self, image, clicks, counts, with_flip):
        x = ops.click_input(image, clicks, counts, self._w['rgb_conv'], NORM_RADIUS, with_flip)
        lg = self.head(self.features(x)['head_input'])
        return ops.click_prob(lg.view(lg.shape[0], lg.shape[1], lg.shape[2]), image.shape[1], image.shape[2])

    def run(self, image, points, with_flip=True):
        """image [3,h,w] on the device, already at the network's working size; points [2n,2] (row, col) as get_points_nd lays one
        clicks list out: n positive then n negative entries, (-1, -1) = padding -> prob [h,w], sigmoid of the (flip-averaged) logits.
        The returned tensor is the graph's static buffer: valid until the next call at the same geometry."""
        self._need_weights()
        n = np.asarray(points).size // 4
        if n > self._cap:                      # grow the click buffers: every captured graph holds the old ones
            self._cap = grown_capacity(self._cap, n)
            self._graphs.clear()
        with ops.ws_scope(f'@click#{self._scope}#'):
            return run_click_stage(self._graphs, self._forward, image, points, self._cap, with_flip)


# ---- the predictor's host logic (fbrs/utils/misc.py, fbrs/inference/transforms/zoom_in.py) ----------------------------

def expand_bbox(bbox, expand_ratio, min_crop_size=None):
    rmin, rmax, cmin, cmax = bbox
    rcenter, ccenter = 0.5 * (rmin + rmax), 0.5 * (cmin + cmax)
    height, width = expand_ratio * (rmax - rmin + 1), expand_ratio * (cmax - cmin + 1)
    if min_crop_size is not None:
        height, width = max(height, min_crop_size), max(width, min_crop_size)
    return (int(round(rcenter - 0.5 * height)), int(round(rcenter + 0.5 * height)),
            int(round(ccenter - 0.5 * width)), int(round(ccenter + 0.5 * width)))


def clamp_bbox(bbox, rmin, rmax, cmin, cmax):
    return (max(rmin, bbox[0]), min(rmax, bbox[1]), max(cmin, bbox[2]), min(cmax, bbox[3]))


def get_segments_iou(s1, s2):
    a, b = s1
    c, d = s2
    return max(0, min(b, d) - max(a, c) + 1) / max(1e-6, max(b, d) - min(a, c) + 1)


def get_bbox_iou(b1, b2):
    return get_segments_iou(b1[:2], b2[:2]) * get_segments_iou(b1[2:4], b2[2:4])


def positive_click_pixels(clicks_list):
    """The pixels get_object_roi sets in the mask: (int(row), int(col)) of every positive click (zoom_in.py:130-132)."""
    return [(int(c.coords[0]), int(c.coords[1])) for c in clicks_list if c.is_positive]


def mask_bbox_host(prob, threshold, click_pixels=()):
    """numpy statement of ops.mask_bbox: (rmin, rmax, cmin, cmax, count) of prob > threshold, the click pixels joining the box."""
    mask = np.asarray(prob) > threshold
    count = int(mask.sum())
    mask = mask.copy()
    for r, c in click_pixels:
        if 0 <= r < mask.shape[0] and 0 <= c < mask.shape[1]:
            mask[r, c] = True
    if not mask.any():
        return (2 ** 31 - 1, -1, 2 ** 31 - 1, -1, 0)
    rows, cols = np.where(mask.any(1))[0], np.where(mask.any(0))[0]
    return (int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1]), count)


def get_object_roi(bbox, shape, expansion_ratio, min_crop_size):
    """get_object_roi from the mask's bounding box (ops.mask_bbox / mask_bbox_host): expanded, then clamped to the map."""
    bbox = expand_bbox(tuple(int(v) for v in bbox[:4]), expansion_ratio, min_crop_size)
    return clamp_bbox(bbox, 0, shape[0] - 1, 0, shape[1] - 1)


def check_object_roi(object_roi, clicks_list):
    for click in clicks_list:
        if click.is_positive:
            if click.coords[0] < object_roi[0] or click.coords[0] >= object_roi[1]:
                return False
            if click.coords[1] < object_roi[2] or click.coords[1] >= object_roi[3]:
                return False
    return True


def roi_image_size(object_roi, target_size):
    """Size of get_roi_image_nd's output (zoom_in.py:142-153): the ROI scaled so that its longest side is target_size."""
    rmin, rmax, cmin, cmax = object_roi
    height, width = rmax - rmin + 1, cmax - cmin + 1
    if isinstance(target_size, tuple):
        return target_size
    scale = target_size / max(height, width)
    return int(round(height * scale)), int(round(width * scale))


def transform_clicks(clicks_list, object_roi, crop_size):
    """ZoomIn._transform_clicks (zoom_in.py:112-124)."""
    if object_roi is None:
        return clicks_list
    rmin, rmax, cmin, cmax = object_roi
    crop_height, crop_width = crop_size
    return [Click(c.is_positive, (crop_height * (c.coords[0] - rmin) / (rmax - rmin + 1),
                                  crop_width * (c.coords[1] - cmin) / (cmax - cmin + 1))) for c in clicks_list]


def get_points_nd(clicks_lists, net_clicks_limit=None):
    """BasePredictor.get_points_nd (predictors/base.py:76-94) as a float32 array [len(clicks_lists), 2n, 2]: per list its first
    net_clicks_limit clicks, n positive then n negative (row, col) entries padded with (-1, -1)."""
    num_pos = [sum(c.is_positive for c in cl) for cl in clicks_lists]
    num_neg = [len(cl) - p for cl, p in zip(clicks_lists, num_pos)]
    num_max = max(num_pos + num_neg)
    if net_clicks_limit is not None:
        num_max = min(net_clicks_limit, num_max)
    num_max = max(1, num_max)
    total = []
    for cl in clicks_lists:
        cl = cl[:net_clicks_limit]
        pos = [c.coords for c in cl if c.is_positive]
        neg = [c.coords for c in cl if not c.is_positive]
        total.append(pos + (num_max - len(pos)) * [(-1, -1)] + neg + (num_max - len(neg)) * [(-1, -1)])
    return np.array(total, dtype=np.float32)


def _device_bbox(prob, threshold, clicks_list):
    pix = positive_click_pixels(clicks_list)
    dev = torch.from_numpy(np.array(pix, np.int32).reshape(-1, 2)).to(prob.device) if pix else None
    return [int(v) for v in ops.mask_bbox(prob, threshold, dev).cpu().numpy()]        # 20 bytes to the host, not the map


class ZoomIn:
    """fbrs/inference/transforms/zoom_in.py:8-124 over device tensors: images [3,H,W], probability maps [H,W]."""

    def __init__(self, target_size=400, skip_clicks=1, expansion_ratio=1.4, min_crop_size=200, recompute_thresh_iou=0.5, prob_thresh=0.5):
        self.target_size, self.min_crop_size, self.skip_clicks = target_size, min_crop_size, skip_clicks
        self.expansion_ratio, self.recompute_thresh_iou, self.prob_thresh = expansion_ratio, recompute_thresh_iou, prob_thresh
        self.reset()

    def reset(self):
        self._input_image_shape = None
        self._object_roi = None
        self._prev_probs = None
        self._roi_image = None
        self.image_changed = False

    def get_state(self):
        return self._input_image_shape, self._object_roi, self._prev_probs, self._roi_image, self.image_changed

    def set_state(self, state):
        self._input_image_shape, self._object_roi, self._prev_probs, self._roi_image, self.image_changed = state

    def _roi_image_of(self, image):
        return ops.resize_bilinear_ac(image, roi_image_size(self._object_roi, self.target_size), crop=self._object_roi)

    def transform(self, image, clicks_list):
        self.image_changed = False
        if len(clicks_list) <= self.skip_clicks:
            return image, clicks_list
        self._input_image_shape = tuple(image.shape)
        current_object_roi = None
        if self._prev_probs is not None:
            box = _device_bbox(self._prev_probs, self.prob_thresh, clicks_list)
            if box[4] > 0:
                current_object_roi = get_object_roi(box, self._prev_probs.shape, self.expansion_ratio, self.min_crop_size)
        if current_object_roi is None:
            return image, clicks_list
        if self._object_roi is None or not check_object_roi(self._object_roi, clicks_list) \
                or get_bbox_iou(current_object_roi, self._object_roi) < self.recompute_thresh_iou:
            self._object_roi = current_object_roi
            self._roi_image = self._roi_image_of(image)
            self.image_changed = True
        return self._roi_image, self._transform_clicks(clicks_list)

    def inv_transform(self, prob):
        """prob is never written after this call (the predictor hands over a copy of the graph's output), so states kept for undo
        stay valid."""
        if self._object_roi is None:
            self._prev_probs = prob
            return prob
        roi = self._object_roi
        if self._prev_probs is not None:
            out = torch.empty((1,) + tuple(self._prev_probs.shape), dtype=torch.float32, device=prob.device)
            new = ops.resize_bilinear_ac(prob[None], None, out=out, paste=roi, zero_fill=True)[0]
        else:
            new = ops.resize_bilinear_ac(prob[None], (roi[1] - roi[0] + 1, roi[3] - roi[2] + 1))[0]
        self._prev_probs = new
        return new

    def check_possible_recalculation(self):
        if self._prev_probs is None or self._object_roi is not None or self.skip_clicks > 0:
            return False
        box = _device_bbox(self._prev_probs, self.prob_thresh, [])
        if box[4] > 0:
            roi = get_object_roi(box, self._prev_probs.shape, self.expansion_ratio, self.min_crop_size)
            image_roi = (0, self._input_image_shape[-2] - 1, 0, self._input_image_shape[-1] - 1)
            return get_bbox_iou(roi, image_roi) < 0.50
        return False

    def _transform_clicks(self, clicks_list):
        return transform_clicks(clicks_list, self._object_roi, None if self._roi_image is None else self._roi_image.shape[-2:])


class LimitLongestSide(ZoomIn):
    """fbrs/inference/transforms/limit_longest_side.py.  It inherits inv_transform and keeps its _object_roi when a later call returns
    early, as the reference does: a zoomed click on an image larger than max_size is resized to the full image and back."""

    def __init__(self, max_size=800):
        super().__init__(target_size=max_size, skip_clicks=0)

    def transform(self, image, clicks_list):
        self.image_changed = False
        if max(image.shape[-2:]) <= self.target_size:
            return image, clicks_list
        self._object_roi = (0, image.shape[-2] - 1, 0, image.shape[-1] - 1)
        self._roi_image = self._roi_image_of(image)
        self.image_changed = True
        return self._roi_image, self._transform_clicks(clicks_list)


class NoBRSPredictor:
    """BasePredictor (fbrs/inference/predictors/base.py:7-100) for one image and one clicks list."""

    def __init__(self, net, net_clicks_limit=None, with_flip=True, zoom_in=None, max_size=None):
        self.net, self.net_clicks_limit, self.with_flip, self.zoom_in = net, net_clicks_limit, with_flip, zoom_in
        self.original_image = None
        self.transforms = [zoom_in] if zoom_in is not None else []
        if max_size is not None:
            self.transforms.append(LimitLongestSide(max_size=max_size))
        self.last_geometry = None       # (working size, transformed clicks) of the last forward

    def set_input_image(self, image):
        for t in self.transforms:
            t.reset()
        self.original_image = image

    def apply_transforms(self, image, clicks_list):
        changed = False
        for t in self.transforms:
            image, clicks_list = t.transform(image, clicks_list)
            changed |= t.image_changed
        return image, clicks_list, changed

    def get_prediction(self, clicks_list):
        image, clicks, changed = self.apply_transforms(self.original_image, list(clicks_list))
        self.last_geometry = (tuple(image.shape[-2:]), [tuple(c.coords) for c in clicks])
        prob = self._predict(image, clicks, changed)
        for t in reversed(self.transforms):
            prob = t.inv_transform(prob)
        if self.zoom_in is not None and self.zoom_in.check_possible_recalculation():
            return self.get_prediction(clicks_list)
        return prob

    def _predict(self, image, clicks, image_changed):
        """The probability map [h,w] of the working image for its (transformed) clicks: BasePredictor._get_prediction with the
        flip-averaged sigmoid of the output transforms."""
        points = get_points_nd([clicks], self.net_clicks_limit)[0]
        return self.net.run(image, points, self.with_flip).clone()       # a copy: the static buffer is overwritten by the next click

    def get_states(self):
        return {'transform_states': [t.get_state() for t in self.transforms]}

    def set_states(self, states):
        assert len(states['transform_states']) == len(self.transforms)
        for state, t in zip(states['transform_states'], self.transforms):
            t.set_state(state)


class FBRSController:
    """inference/interact/fbrs_controller.py with fbrs/controller.py's InteractiveController folded in: clicks on one anchored image ->
    the object's mask.  Defaults are the reference's (zoom-in skip_clicks=1, target_size=480, expansion_ratio=1.4; with_flip;
    prob_thresh 0.5; max_size 800) except the predictor: brs_mode='NoBRS' with NoBRS's own net_clicks_limit=None (with the reference
    controller's limit of 8, clicks after the eighth would be ignored outright once no optimisation follows them).  This class
    runs no back-propagating refinement: click_brs.FeatureBRSController is the controller with the reference's own defaults
    ('f-BRS-B', net_clicks_limit=8).  The first click of every mode is identical to NoBRS's (no optimisation runs before
    optimize_after_n_clicks=1); later clicks lack the refinement here."""

    def __init__(self, checkpoint_path_or_net, device='cuda:0', max_size=800, brs_mode='NoBRS', zoom_in_params=None, with_flip=True,
                 net_clicks_limit=None, prob_thresh=0.5):
        if brs_mode in BRS_MODES:
            raise NotImplementedError(f"FBRSController: brs_mode={brs_mode!r} needs the back-propagating refinement (backward kernels and "
                                      "L-BFGS), which this controller does not run.  Its first click is identical to brs_mode='NoBRS'; "
                                      "later clicks lack the refinement.  xmem2_amd.click_brs.FeatureBRSController runs 'f-BRS-B' and "
                                      "'f-BRS-C'.")
        if brs_mode != 'NoBRS':
            raise ValueError(f'FBRSController: unknown brs_mode {brs_mode!r}')
        self._setup(checkpoint_path_or_net, device, max_size, zoom_in_params, with_flip, net_clicks_limit, prob_thresh)

    def _setup(self, checkpoint_path_or_net, device, max_size, zoom_in_params, with_flip, net_clicks_limit, prob_thresh):
        self.device = torch.device(device)
        self.net = checkpoint_path_or_net if isinstance(checkpoint_path_or_net, ClickNet) \
            else ClickNet(checkpoint_path_or_net, device=self.device)
        self.zoom_in_params = dict(skip_clicks=1, target_size=480, expansion_ratio=1.4)
        self.zoom_in_params.update(zoom_in_params or {})
        self.max_size, self.with_flip, self.net_clicks_limit, self.prob_thresh = max_size, with_flip, net_clicks_limit, prob_thresh
        self.anchored = False
        self.image = None
        self.predictor = None
        self._reset_object()

    def _reset_object(self):
        self.clicks, self.states, self.probs_history = [], [], []

    def _reset_predictor(self):
        self.predictor = NoBRSPredictor(self.net, self.net_clicks_limit, self.with_flip,
                                        ZoomIn(prob_thresh=self.prob_thresh, **self.zoom_in_params), self.max_size)
        if self.image is not None:
            self.predictor.set_input_image(self.image)

    def unanchor(self):
        self.anchored = False

    @property
    def prob(self):
        """The last probability map [H,W] (None before the first click and after the last undo)."""
        return self.probs_history[-1] if self.probs_history else None

    def _mask(self):
        p = self.prob
        return None if p is None else ops.prob_threshold(p, 0.5).view(1, 1, *p.shape)

    def interact(self, image, x, y, is_positive):
        """image [1,3,H,W] or [3,H,W] (normalised), a click at column x, row y -> [1,1,H,W] float mask (prob > 0.5) on the device."""
        with torch.cuda.device(self.device):
            if not self.anchored:
                image = image.to(self.device, torch.float32, non_blocking=True)
                image = image[0] if image.dim() == 4 else image
                if image.dim() != 3 or image.shape[0] != 3:
                    raise ValueError(f'FBRSController: expected an image [1,3,H,W] or [3,H,W], got {tuple(image.shape)}')
                self.image = image.contiguous()
                self._reset_object()
                self._reset_predictor()
                self.anchored = True
            self.states.append({'clicker': list(self.clicks), 'predictor': self.predictor.get_states()})
            self.clicks.append(Click(bool(is_positive), (y, x)))
            self.probs_history.append(self.predictor.get_prediction(self.clicks))
            return self._mask()

    def undo(self):
        if not self.states:
            return None
        prev = self.states.pop()
        self.clicks = list(prev['clicker'])
        self.predictor.set_states(prev['predictor'])
        self.probs_history.pop()
        with torch.cuda.device(self.device):
            return self._mask()


def click_commit(prev_prob, obj_mask, tar_obj):
    """ClickInteraction.predict (interaction.py:247-254): (aggregate_wbg of the clamped previous maps with row tar_obj replaced by the
    click mask [K+1,H,W], its argmax uint8 [H,W])."""
    return ops.click_commit(prev_prob, obj_mask, tar_obj, HARD_TEMPERATURE)


# ---- command line ----------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m xmem2_amd.click', description='Clicks -> annotation masks (the click step of the '
                                 'interactive demo, without the GUI).')
    ap.add_argument('--images', required=True, help='directory of frames')
    ap.add_argument('--clicks', required=True, help='JSON: {frame number: [{"object": k, "x": col, "y": row, "positive": bool}, ...]}')
    ap.add_argument('--out', required=True, help='output directory for the palette masks')
    ap.add_argument('--prev-masks', default=None, help='directory of indexed previous masks (default: none)')
    src = ap.add_mutually_exclusive_group()
    src.add_argument('--model', default=None, help='click-network checkpoint (saves/fbrs.pth)')
    src.add_argument('--synthetic-seed', type=int, default=None, help='conditioned synthetic weights instead of a checkpoint')
    ap.add_argument('--num-objects', type=int, default=None, help='objects (default: the largest label in clicks / masks)')
    ap.add_argument('--brs-mode', choices=('NoBRS', 'f-BRS-B', 'f-BRS-C'), default='NoBRS',
                    help="click refinement: 'f-BRS-B' is the interactive demo's (default: NoBRS, no refinement)")
    args = ap.parse_args(argv)
    if args.model is None and args.synthetic_seed is None:
        ap.error('one of --model or --synthetic-seed is required')
    if args.model is not None and not os.path.isfile(args.model):
        ap.error(f'--model: no such file: {args.model}')
    if not os.path.isfile(args.clicks):
        ap.error(f'--clicks: no such file: {args.clicks}')
    if args.num_objects is not None and not 1 <= args.num_objects <= 254:
        ap.error('--num-objects must be in [1, 254]')
    return args


def load_clicks(path):
    """{frame number: [(object, x, y, positive), ...]} of a clicks JSON, validated."""
    with open(path) as f:
        data = json.load(f)
    if not isinstance(data, dict):
        raise ValueError(f'{path}: expected an object mapping frame numbers to click lists')
    out = {}
    for frame, clicks in data.items():
        try:
            n = int(frame)
        except (TypeError, ValueError):
            raise ValueError(f'{path}: frame key {frame!r} is not an integer') from None
        if n in out:
            raise ValueError(f'{path}: frame {n} appears twice')
        if not isinstance(clicks, list) or not clicks:
            raise ValueError(f'{path}: frame {n}: expected a non-empty list of clicks')
        rows = []
        for c in clicks:
            if not isinstance(c, dict) or set(c) != {'object', 'x', 'y', 'positive'}:
                raise ValueError(f'{path}: frame {n}: a click is {{"object", "x", "y", "positive"}}, got {c!r}')
            if isinstance(c['object'], bool) or not isinstance(c['object'], int) or not 1 <= c['object'] <= 254:
                raise ValueError(f'{path}: frame {n}: object must be an integer in [1, 254], got {c["object"]!r}')
            if any(isinstance(c[k], bool) or not isinstance(c[k], (int, float)) or c[k] < 0 for k in ('x', 'y')):
                raise ValueError(f'{path}: frame {n}: x and y must be non-negative numbers, got {c["x"]!r}, {c["y"]!r}')
            if not isinstance(c['positive'], bool):
                raise ValueError(f'{path}: frame {n}: positive must be true or false, got {c["positive"]!r}')
            rows.append((c['object'], c['x'], c['y'], c['positive']))
        out[n] = rows
    return out


def main(argv=None):
    args = parse_args(argv)
    from PIL import Image
    from .scribble import IM_MEAN, IM_STD, _load_index, _palette, index_dir
    torch.set_grad_enabled(False)
    clicks = load_clicks(args.clicks)
    imgs, prevs = index_dir(args.images), index_dir(args.prev_masks, ('.png',))
    missing = sorted(set(clicks) - set(imgs))
    if missing:
        raise FileNotFoundError(f'clicks without a frame: numbers {missing[:10]}')
    loaded, k_max = [], 0
    for n in sorted(clicks):
        img = np.array(Image.open(os.path.join(args.images, imgs[n])).convert('RGB'), dtype=np.uint8)
        prev = _load_index(os.path.join(args.prev_masks, prevs[n])) if n in prevs else np.zeros(img.shape[:2], np.uint8)
        if prev.shape != img.shape[:2]:
            raise ValueError(f'frame {n}: image {img.shape[:2]} and previous mask {prev.shape} differ in size')
        for _, x, y, _p in clicks[n]:
            if not (x <= img.shape[1] - 1 and y <= img.shape[0] - 1):
                raise ValueError(f'frame {n}: click ({x}, {y}) lies outside the {img.shape[1]}x{img.shape[0]} frame')
        k_max = max([k_max] + [c[0] for c in clicks[n]] + [int(v) for v in np.unique(prev) if 0 < v < 255])
        loaded.append((imgs[n], img, prev, clicks[n]))
    K = args.num_objects or k_max
    if k_max > K:
        raise ValueError(f'--num-objects {K} is smaller than the largest label {k_max}')
    device = torch.device('cuda', torch.cuda.current_device())
    from . import click as pkg      # under `python -m` this module is __main__: take the classes click_brs subclasses from the package
    net = pkg.ClickNet(device=device)
    if args.model:
        net.load_weights(args.model)
    else:
        from .synth import synthetic_click_state_dict
        net.load_state_dict(synthetic_click_state_dict(args.synthetic_seed))
    if args.brs_mode == 'NoBRS':
        ctl = pkg.FBRSController(net, device=device)
    else:
        from .click_brs import FeatureBRSController
        ctl = FeatureBRSController(net, device=device, brs_mode=args.brs_mode)
    os.makedirs(args.out, exist_ok=True)
    pal = _palette()
    for fi, img, prev, frame_clicks in loaded:
        image = torch.from_numpy(((img.astype(np.float32) / 255.0 - IM_MEAN) / IM_STD).transpose(2, 0, 1).copy()).to(device)
        onehot = np.stack([prev == k for k in range(K + 1)]).astype(np.float32)
        prob, mask = torch.from_numpy(onehot).to(device), torch.from_numpy(prev).to(device)
        for k in sorted({c[0] for c in frame_clicks}):
            ctl.unanchor()                     # a fresh anchor per object
            for _, x, y, positive in (c for c in frame_clicks if c[0] == k):
                obj = ctl.interact(image, x, y, positive)
            prob, mask = click_commit(prob, obj, k)
        out = Image.fromarray(mask.cpu().numpy(), mode='P')
        out.putpalette(pal)
        out.save(os.path.join(args.out, os.path.splitext(fi)[0] + '.png'))
    print(f'wrote {len(loaded)} mask(s) for {K} object(s) to {args.out} ({net.captures} graph capture(s))')
    return 0


if __name__ == '__main__':
    sys.exit(main())
