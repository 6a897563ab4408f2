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
import numpy as np
import torch

from . import ops, stages
from .arch import s2m_state_dict_spec
from .hipnet import HipNet

ASPP_RATES = (6, 12, 18)        # output_stride 16 (s2m_network.py:12-13)
HARD_TEMPERATURE = 1000.0       # aggregate_wbg(hard=True): logits x 1000 (interaction.py:45-47)


def state_dict_spec():
    """Names and shapes of the reference's S2M state dict (368 tensors, state_dict order)."""
    return s2m_state_dict_spec()


def pad_divide_by_16(h, w):
    """(Hp, Wp, lh, lw) of pad_divide_by(., 16) (util/tensor_util.py:47-62): centred zero padding to multiples of 16."""
    Hp, Wp = -(-h // 16) * 16, -(-w // 16) * 16
    return Hp, Wp, (Hp - h) // 2, (Wp - w) // 2


class S2M(HipNet):
    """deeplabv3plus_resnet50(num_classes=1, output_stride=16) on HIP kernels (fp32, the demo's --no_amp arithmetic)."""

    _synthetic = 'synthetic_s2m_state_dict'

    def __init__(self, model_path=None, device=None):
        super().__init__(torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device()))
        self._graphs = self._stages         # one graph per (K, H, W, ignore_class), unbounded
        if model_path is not None:
            self.load_weights(model_path)

    def _spec(self):
        return state_dict_spec()

    def _upload(self):
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
        with ops.ws_scope(f'@s2m#{self._scope}#'):
            st = self._graphs.lookup(key)
            if st is None:
                st = self._graphs.put(key, stages.capture(lambda *a: self._forward(*a, K, ignore_class),
                                                          (image.clone(), prev_mask.clone(), scr.clone())))
            return st.replay((image, prev_mask, scr))


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
