"""What the networks of the package (network.XMem, s2m.S2M, click.ClickNet) share: the weights surface and the ResNet blocks.

Nothing is an nn.Module.  A network keeps the checkpoint on the host (``_sd``), uploads it re-laid-out (``_w``: every convolution as
``[Cout][KH][KW][Cin]`` with its eval-mode BatchNorm folded to a per-channel scale and shift) and captures its forward passes into
HIP graphs (``_stages``, stages.py).  The captured kernels hold the device pointers of ``_w``, hence the one rule of this module:
weights replaced -> captured stages dropped.  Every path that uploads again (load_state_dict, to) goes through ``_reupload``.
"""
import weakref

import torch

from . import ops
from .arch import BN_EPS
from .ops import ConvWeights
from .stages import StageCache


def _pad4(n):
    return (n + 3) // 4 * 4


def check_state_dict(sd, spec, who, ignored=()):
    """The strict check of load_state_dict: `sd` against `spec` (name -> shape) of the network `who`.  num_batches_tracked and the names
    in `ignored` may be absent or present; a one-element tensor passes for a scalar."""
    free = lambda k: k in ignored or k.endswith('num_batches_tracked')
    missing = [k for k in spec if k not in sd and not free(k)]
    unexpected = [k for k in sd if k not in spec and not free(k)]
    if missing or unexpected:
        raise RuntimeError(f'Error(s) in loading state_dict for {who}: missing {missing[:5]}..., unexpected {unexpected[:5]}...')
    for k, shape in spec.items():
        if k in sd and tuple(sd[k].shape) != tuple(shape) and not (len(shape) == 0 and sd[k].numel() == 1):
            raise RuntimeError(f'size mismatch for {k}: checkpoint {tuple(sd[k].shape)} vs model {tuple(shape)}')


class HipNet:
    """Base of XMem, S2M and ClickNet.  A subclass gives `_spec()` and `_upload()`, and `_synthetic` unless it has a `_need_weights` of its own."""
    # a bottleneck's conv3 and the next block's conv1 in one launch (_stage): XMem switches it on
    fused_bottleneck = False
    fused_bottleneck_min_pixels = 0
    ignored_keys = ()               # checkpoint entries that are neither required nor kept

    def __init__(self, device, max_stages=None):
        self.device = device
        self._sd = None
        self._w = {}
        self._stages = StageCache(max_stages)       # captured forward passes, least recently replayed first
        # scratch of stages that may run on a side stream is scoped to this instance and released with it
        self._scope = ops.new_scope()
        weakref.finalize(self, ops.release_scope, self._scope)

    @property
    def captures(self):
        """graphs captured so far"""
        return self._stages.captures

    # ---- weights ----------------------------------------------------------------------------------
    def _spec(self):
        """name -> shape of the state dict this network loads"""
        raise NotImplementedError

    def _upload(self):
        """self._sd -> self._w on self.device"""
        raise NotImplementedError

    def load_weights(self, src):
        """A checkpoint path or a state dict."""
        if isinstance(src, (str, bytes)) or hasattr(src, '__fspath__'):
            src = torch.load(src, map_location='cpu', weights_only=True)
        self.load_state_dict(src)
        return self

    def load_state_dict(self, sd, strict=True):
        if strict:
            check_state_dict(sd, self._spec(), type(self).__name__, self.ignored_keys)
        self._adopt(sd)

    def _adopt(self, sd):
        """`sd` (checked) becomes the network's weights"""
        self._sd = {k: v.detach().to('cpu') for k, v in sd.items() if k not in self.ignored_keys}
        self._reupload()

    def state_dict(self):
        return dict(self._sd) if self._sd is not None else {}

    def to(self, device):
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = device
        if self._sd is not None:
            self._reupload()
        return self

    def eval(self):
        return self

    def _reupload(self):
        if self.device.type != 'cuda':
            raise RuntimeError(f'xmem2_amd.{type(self).__name__} runs on an MI355X (HIP) device only; there is no CPU path')
        self._weights_replaced()
        self._upload()

    def _weights_replaced(self):
        """The tensors of self._w are about to be freed: drop every captured stage, whose kernels hold their addresses.  The stages are
        captured again, against the new tensors, when they next run."""
        self._stages.clear()

    def _need_weights(self):
        if not self._w:
            raise RuntimeError(f'{type(self).__name__}: no weights loaded (load_weights(path) or load_state_dict(sd); '
                               f'xmem2_amd.synth.{self._synthetic} gives conditioned synthetic ones)')

    def _conv_w(self, name, bn=None, stride=1, pad=0):
        sd = self._sd
        w = sd[name + '.weight'].float()
        cout, cin = w.shape[0], w.shape[1]
        wk = w.permute(0, 2, 3, 1)
        if cin % 4:
            wk = torch.nn.functional.pad(wk, (0, _pad4(cin) - cin))
        if bn is not None:
            invstd = 1.0 / torch.sqrt(sd[bn + '.running_var'].float() + BN_EPS)
            scale = invstd * sd[bn + '.weight'].float()
            shift = sd[bn + '.bias'].float() - sd[bn + '.running_mean'].float() * scale
        else:
            scale = torch.ones(cout)
            shift = sd[name + '.bias'].float() if (name + '.bias') in sd else torch.zeros(cout)
        dev = self.device
        return ConvWeights(wk.contiguous().to(dev), scale.contiguous().to(dev), shift.contiguous().to(dev), stride, pad, cin_true=cin)

    # ---- ResNet building blocks (NHWC) ------------------------------------------------------------
    def _bottleneck(self, x, p):
        W = self._w
        o = ops.conv2d(x, W[p + '.conv1'], relu_out=True)
        o = ops.conv2d(o, W[p + '.conv2'], relu_out=True)
        res = ops.conv2d(x, W[p + '.downsample']) if (p + '.downsample') in W else x
        return ops.conv2d(o, W[p + '.conv3'], res=res, relu_out=True)

    def _basic(self, x, p):
        W = self._w
        o = ops.conv2d(x, W[p + '.conv1'], relu_out=True)
        res = ops.conv2d(x, W[p + '.downsample']) if (p + '.downsample') in W else x
        return ops.conv2d(o, W[p + '.conv2'], res=res, relu_out=True)

    def _stage(self, x, prefix, blocks, fn, pre=None, then=None):
        """The blocks of one ResNet stage.  A bottleneck stage of a network with `fused_bottleneck` walks its blocks so that block b's conv3 and
        block b + 1's conv1 are one launch (ops.conv2d_pointwise_pair); `then` names the convolution that reads the stage's output next (the
        following stage's first conv1), which is paired with the last conv3 and returned with the output: -> (x, then(x)), and `pre` is
        block 0's conv1 output made that way.  A pair the op does not take runs as the two convolutions: the same bits either way."""
        if fn != self._bottleneck or not self.fused_bottleneck:
            for b in range(blocks):
                x = fn(x, f'{prefix}.{b}')
            return x if then is None else (x, None)
        W = self._w
        for b in range(blocks):
            p = f'{prefix}.{b}'
            o = pre if pre is not None else ops.conv2d(x, W[p + '.conv1'], relu_out=True)
            o = ops.conv2d(o, W[p + '.conv2'], relu_out=True)
            res = ops.conv2d(x, W[p + '.downsample']) if (p + '.downsample') in W else x
            follow = f'{prefix}.{b + 1}.conv1' if b + 1 < blocks else then
            if follow is not None and o.shape[0] * o.shape[1] * o.shape[2] >= self.fused_bottleneck_min_pixels:
                x, pre = ops.conv2d_pointwise_pair(o, W[p + '.conv3'], res, W[follow])
            else:
                x, pre = ops.conv2d(o, W[p + '.conv3'], res=res, relu_out=True), None
        return x if then is None else (x, pre)
