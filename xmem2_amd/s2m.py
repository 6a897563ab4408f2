"""Scribble-to-mask (S2M) on MI355X: the reference's interactive-annotation network over HIP kernels.

``S2M`` mirrors ``deeplabv3plus_resnet50(num_classes=1, output_stride=16)`` (inference/interact/s2m/s2m_network.py:54-65):
a ResNet-50 with a 6-channel stem and a dilated layer4 (s2m_resnet.py), and the DeepLabV3+ head (s2m/_deeplab.py:30-53,
113-166).  As in network.py, nothing is an nn.Module: BatchNorm is folded into the convolutions' scale / shift at load time,
activations are NHWC, and every operation is a HIP kernel (ops).  All K objects run as one batch of K, where the reference loops
over them, and the forward is captured once per (K, H, W) as a HIP graph and replayed.

``S2MController`` keeps the reference's interface (inference/interact/s2m_controller.py) and ``aggregate_wbg`` that of
interaction.py:36-51, so the GUI's commit sequence (argmax -> one-hot -> [1:] -> InferenceCore.put_to_permanent_memory,
gui.py:851-859) runs unchanged on the result.
"""
import weakref

import numpy as np
import torch

from . import ops
from .arch import s2m_state_dict_spec
from .network import XMem

ASPP_RATES = (6, 12, 18)        # output_stride 16 (s2m_network.py:12-13)
HARD_TEMPERATURE = 1000.0       # aggregate_wbg(hard=True): logits x 1000 (interaction.py:45-47)


def state_dict_spec():
    """Names and shapes of the reference's S2M state dict (368 tensors, state_dict order)."""
    return s2m_state_dict_spec()


def pad_divide_by_16(h, w):
    """(Hp, Wp, lh, lw) of pad_divide_by(., 16) (util/tensor_util.py:47-62): centred zero padding to multiples of 16."""
    Hp, Wp = -(-h // 16) * 16, -(-w // 16) * 16
    return Hp, Wp, (Hp - h) // 2, (Wp - w) // 2


class S2M:
    """deeplabv3plus_resnet50(num_classes=1, output_stride=16) on HIP kernels (fp32, the demo's --no_amp arithmetic)."""

    # the ResNet building blocks of network.py: the same BN folding, bottleneck and stage code
    _conv_w = XMem._conv_w
    _bottleneck = XMem._bottleneck
    _stage = XMem._stage

    def __init__(self, model_path=None, device=None):
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._sd = None
        self._w = {}
        self._graphs = {}
        self.captures = 0              # graphs captured so far (one per (K, H, W))
        self._scope = ops.new_scope()
        weakref.finalize(self, ops.release_scope, self._scope)
        if model_path is not None:
            self.load_weights(model_path)

    # ---- weights ----------------------------------------------------------------------------------
    def load_weights(self, src):
        """A checkpoint path (torch.load('saves/s2m.pth')) or a state dict."""
        if isinstance(src, (str, bytes)) or hasattr(src, '__fspath__'):
            src = torch.load(src, map_location='cpu', weights_only=True)
        self.load_state_dict(src)
        return self

    def load_state_dict(self, sd, strict=True):
        spec = state_dict_spec()
        if strict:
            missing = [k for k in spec if k not in sd and not k.endswith('num_batches_tracked')]
            unexpected = [k for k in sd if k not in spec]
            if missing or unexpected:
                raise RuntimeError(f'Error(s) in loading state_dict for S2M: missing {missing[:5]}..., unexpected {unexpected[:5]}...')
        for k, shape in spec.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape) and not (len(shape) == 0 and sd[k].numel() == 1):
                raise RuntimeError(f'size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shape)}')
        self._sd = {k: v.detach().to('cpu') for k, v in sd.items()}
        self._graphs.clear()
        self._upload()

    def state_dict(self):
        return dict(self._sd) if self._sd is not None else {}

    def to(self, device):
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        if self._sd is not None:
            self._graphs.clear()
            self._upload()
        return self

    def eval(self):
        return self

    def _upload(self):
        if self.device.type != 'cuda':
            raise RuntimeError('xmem2_amd.S2M runs on an MI355X (HIP) device only; there is no CPU path')
        W = {}
        W['backbone.conv1'] = self._conv_w('backbone.conv1', 'backbone.bn1', 2, 3)      # 6 channels, padded to the packed 8
        for prefix, blocks, stride in (('backbone.layer1', 3, 1), ('backbone.layer2', 4, 2), ('backbone.layer3', 6, 2),
                                       ('backbone.layer4', 3, 1)):
            for b in range(blocks):
                p, s = f'{prefix}.{b}', (stride if b == 0 else 1)
                # layer4: stride replaced by dilation 2; block 0 keeps dilation 1 (torchvision _make_layer, s2m_resnet.py:138-150)
                dil = 2 if prefix == 'backbone.layer4' and b > 0 else 1
                W[p + '.conv1'] = self._conv_w(p + '.conv1', p + '.bn1', 1, 0)
                W[p + '.conv2'] = self._conv_w(p + '.conv2', p + '.bn2', s, dil)
                W[p + '.conv2'].dilation = dil
                W[p + '.conv3'] = self._conv_w(p + '.conv3', p + '.bn3', 1, 0)
                if (p + '.downsample.0.weight') in self._sd:
                    W[p + '.downsample'] = self._conv_w(p + '.downsample.0', p + '.downsample.1', s, 0)
        c = 'classifier.'
        W['project'] = self._conv_w(c + 'project.0', c + 'project.1', 1, 0)
        W['aspp.0'] = self._conv_w(c + 'aspp.convs.0.0', c + 'aspp.convs.0.1', 1, 0)
        for i, rate in enumerate(ASPP_RATES, 1):
            W[f'aspp.{i}'] = self._conv_w(f'{c}aspp.convs.{i}.0', f'{c}aspp.convs.{i}.1', 1, rate)
            W[f'aspp.{i}'].dilation = rate
        W['aspp.pool'] = self._conv_w(c + 'aspp.convs.4.1', c + 'aspp.convs.4.2', 1, 0)
        W['aspp.project'] = self._conv_w(c + 'aspp.project.0', c + 'aspp.project.1', 1, 0)
        W['head.0'] = self._conv_w(c + 'classifier.0', c + 'classifier.1', 1, 1)
        W['head.3'] = self._conv_w(c + 'classifier.3', None, 1, 0)
        self._w = W

    def _need_weights(self):
        if not self._w:
            raise RuntimeError('S2M: no weights loaded (load_weights(path) or load_state_dict(sd); '
                               'xmem2_amd.synth.synthetic_s2m_state_dict gives conditioned synthetic ones)')

    # ---- forward (NHWC) -------------------------------------------------------------------------
    def features(self, x):
        """x [K,Hp,Wp,8] (ops.s2m_pack) -> dict of NHWC tensors: low_level [K,Hp/4,Wp/4,256] (layer1), aspp [K,Hp/16,Wp/16,256]
        (the ASPP output), logits [K,Hp/4,Wp/4,1] (the head's 1/4-resolution output, before the final upsample)."""
        self._need_weights()
        W = self._w
        x = ops.conv2d(x, W['backbone.conv1'], relu_out=True)
        x = ops.maxpool3x3s2(x)
        low = self._stage(x, 'backbone.layer1', 3, self._bottleneck)
        x = self._stage(low, 'backbone.layer2', 4, self._bottleneck)
        x = self._stage(x, 'backbone.layer3', 6, self._bottleneck)
        x = self._stage(x, 'backbone.layer4', 3, self._bottleneck)
        K, h, w, c = x.shape
        # ASPP (_deeplab.py:136-166): the five branches write their slices of the 1280-channel concat buffer
        cat = torch.empty((K, h, w, 5 * 256), dtype=torch.float32, device=x.device)
        ops.conv2d(x, W['aspp.0'], relu_out=True, out=cat[..., 0:256], out_ld=1280)
        for i in range(1, 4):
            ops.conv2d(x, W[f'aspp.{i}'], relu_out=True, out=cat[..., 256 * i:256 * (i + 1)], out_ld=1280)
        pooled = ops.channel_mean(x).view(K, 1, 1, c)
        pooled = ops.conv2d(pooled, W['aspp.pool'], relu_out=True)
        ops.broadcast_channels(pooled.view(K, 256), cat[..., 1024:1280])
        aspp = ops.conv2d(cat, W['aspp.project'], relu_out=True)            # Dropout(0.1) is the identity in eval
        # DeepLabV3+ decoder (_deeplab.py:49-53): cat([project(low_level), upsample(aspp)]) -> 3x3 -> 1x1
        h4, w4 = low.shape[1], low.shape[2]
        dec = torch.empty((K, h4, w4, 304), dtype=torch.float32, device=x.device)
        ops.conv2d(low, W['project'], relu_out=True, out=dec[..., 0:48], out_ld=304)
        ops.resize_bilinear_nhwc(aspp, (h4, w4), out=dec[..., 48:304])
        y = ops.conv2d(dec, W['head.0'], relu_out=True)
        logits = ops.conv2d(y, W['head.3'])
        return dict(low_level=low, aspp=aspp, logits=logits)

    def _forward(self, image, prev_mask, scr, K, ignore_class):
        H, W = image.shape[-2:]
        Hp, Wp, lh, lw = pad_divide_by_16(H, W)
        x = ops.s2m_pack(image, prev_mask, scr, K, ignore_class, Hp, Wp, lh, lw)
        lg = self.features(x)['logits']
        return ops.s2m_output(lg.view(K, lg.shape[1], lg.shape[2]), H, W, lh, lw, HARD_TEMPERATURE)

    def run(self, image, prev_mask, scr, num_objects, ignore_class=255):
        """image [3,H,W] float (normalised), prev_mask [H,W] float (index), scr [H,W] uint8, all on the device ->
        (prob [K,H,W], prob_wbg [K+1,H,W] = aggregate_wbg(prob, keep_bg=True, hard=True), mask [H,W] uint8 = its argmax).
        The returned tensors are the graph's static buffers: valid until the next call at the same (K, H, W)."""
        self._need_weights()
        K, H, W = int(num_objects), int(image.shape[-2]), int(image.shape[-1])
        key = (K, H, W, int(ignore_class))
        st = self._graphs.get(key)
        with ops.ws_scope(f'@s2m#{self._scope}#'):
            if st is None:
                static_in = (image.clone(), prev_mask.clone(), scr.clone())
                self._forward(*static_in, K, ignore_class)          # warm-up: sizes every workspace and picks the plans
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static_out = self._forward(*static_in, K, ignore_class)
                st = self._graphs[key] = (graph, static_in, static_out)
                self.captures += 1
            graph, static_in, static_out = st
            for dst, src in zip(static_in, (image, prev_mask, scr)):
                dst.copy_(src)
            graph.replay()
        return static_out


def aggregate_wbg(prob, keep_bg=False, hard=False):
    """interaction.py:36-51: prob [K,H,W] -> softmax of the clamped logits of cat(prod(1 - prob), prob), x1000 with hard;
    [K+1,H,W] with keep_bg, else the K object rows."""
    return ops.aggregate_wbg(prob, keep_bg=keep_bg, temperature=HARD_TEMPERATURE if hard else 1.0)


class S2MController:
    """inference/interact/s2m_controller.py: scribbles -> one probability map per object.  ignore_class is usually 255;
    0 is NOT the ignore class - it is the label for the background."""

    def __init__(self, s2m_net, num_objects, ignore_class=255, device='cuda:0'):
        if int(num_objects) < 1 or int(num_objects) > 254:
            raise ValueError(f'S2MController: num_objects must be in [1, 254], got {num_objects}')
        self.s2m_net = s2m_net
        self.num_objects = int(num_objects)
        self.ignore_class = int(ignore_class)
        self.device = torch.device(device)

    def _inputs(self, image, prev_mask, scr_mask):
        image = image.to(self.device, torch.float32, non_blocking=True)
        if image.dim() == 4:
            if image.shape[0] != 1:
                raise ValueError(f'S2MController: expected one image [1,3,H,W], got {tuple(image.shape)}')
            image = image[0]
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError(f'S2MController: expected an image [1,3,H,W] or [3,H,W], got {tuple(image.shape)}')
        H, W = image.shape[-2:]
        prev = torch.as_tensor(prev_mask).to(self.device, torch.float32)
        scr = torch.from_numpy(np.ascontiguousarray(scr_mask, dtype=np.uint8)) if isinstance(scr_mask, np.ndarray) \
            else torch.as_tensor(scr_mask, dtype=torch.uint8)
        if tuple(prev.shape) != (H, W) or tuple(scr.shape) != (H, W):
            raise ValueError(f'S2MController: image {H}x{W}, prev_mask {tuple(prev.shape)} and scr_mask {tuple(scr.shape)} differ in size')
        return image, prev, scr.to(self.device)

    def interact(self, image, prev_mask, scr_mask):
        """image [1,3,H,W] (normalised), prev_mask [H,W] (float index), scr_mask numpy uint8 [H,W] -> [K,H,W] on the device."""
        with torch.cuda.device(self.device):
            prob, _, _ = self.s2m_net.run(*self._inputs(image, prev_mask, scr_mask), self.num_objects, self.ignore_class)
            return prob.clone()

    def predict(self, image, prev_mask, scr_mask):
        """ScribbleInteraction.predict (interaction.py:193-196) in the same launch: (aggregate_wbg(interact(...), keep_bg=True,
        hard=True) [K+1,H,W], its argmax uint8 [H,W])."""
        with torch.cuda.device(self.device):
            _, wbg, mask = self.s2m_net.run(*self._inputs(image, prev_mask, scr_mask), self.num_objects, self.ignore_class)
            return wbg.clone(), mask.clone()
