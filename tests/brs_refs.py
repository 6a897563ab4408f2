"""Float64 restatement of the f-BRS objective for the tests: torch on the CPU, gradients by autograd.

The head of the click network is rebuilt from the state dict with torch.nn.functional (SeparableConv2d = depthwise 3x3 without bias,
pointwise 1x1 without bias, BatchNorm in eval mode, ReLU; _DeepLabHead = two of them and a biased 1x1; SepConvHead = two of them and
a biased 1x1 to one channel), the objective is

    y = input_data (1 + scale) + bias -> [_DeepLabHead ->] SepConvHead -> align_corners upsample -> sigmoid = p
    f = sum(((1 - p) pos)^2) / (sum(pos) + 1e-5) + sum((p neg)^2) / (sum(neg) + 1e-5) + 1e-3 (sum(scale^2) + 10 sum(bias^2))

over both flip samples jointly, and the click maps are painted with the numpy slices the optimiser's masks are defined by.  x is
rounded to float32 first, as the optimiser hands it over.  Nothing here touches a GPU or the package's kernels.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
EPS = 1e-5
REG_WEIGHT, REG_BIAS_WEIGHT = 1e-3, 10.0


def click_maps(clicks_lists, shape, radius=1):
    """(pos, neg) float64 [n,1,H,W]: per clicks list the 3 x 3 squares around (int(round(row)), int(round(col))), painted by numpy
    slicing - so a square is clipped at the far edges and EMPTY when its first row or column index is negative.  clicks: (is_positive,
    (row, col))."""
    pos = np.zeros((len(clicks_lists), 1) + tuple(shape), np.float64)
    neg = np.zeros_like(pos)
    for i, cl in enumerate(clicks_lists):
        for is_positive, (row, col) in cl:
            y, x = int(round(row)), int(round(col))
            (pos if is_positive else neg)[i, 0, y - radius:y + radius + 1, x - radius:x + radius + 1] = 1.0
    return pos, neg


def maps_from_squares(rects, shape):
    """Paint int [n, k, 5] rectangles (r0, r1, c0, c1, positive) - the form the loss kernel takes - into (pos, neg) maps."""
    pos = np.zeros((rects.shape[0], 1) + tuple(shape), np.float64)
    neg = np.zeros_like(pos)
    for i in range(rects.shape[0]):
        for r0, r1, c0, c1, p in rects[i]:
            (pos if p else neg)[i, 0, r0:r1, c0:c1] = 1.0
    return pos, neg


def _separable(sd, prefix, x):
    d = lambda k: sd[prefix + k].double()
    x = F.conv2d(x, d('.body.0.weight'), padding=1, groups=x.shape[1])
    x = F.conv2d(x, d('.body.1.weight'))
    x = F.batch_norm(x, d('.body.2.running_mean'), d('.body.2.running_var'), d('.body.2.weight'), d('.body.2.bias'), False, 0.0, BN_EPS)
    return F.relu(x)


def deeplab_head(sd, x):
    p = 'feature_extractor.head.block.'
    x = _separable(sd, p + '1', _separable(sd, p + '0', x))
    return F.conv2d(x, sd[p + '2.weight'].double(), sd[p + '2.bias'].double())


def sep_conv_head(sd, x):
    x = _separable(sd, 'head.layers.1', _separable(sd, 'head.layers.0', x))
    return F.conv2d(x, sd['head.layers.2.weight'].double(), sd['head.layers.2.bias'].double())


def loss(logits, pos, neg, size):
    """logits [B,1,h4,w4] -> (data loss, f_max_pos, f_max_neg, upsampled logits [B,1,H,W])."""
    up = F.interpolate(logits, size=tuple(size), mode='bilinear', align_corners=True)
    p = torch.sigmoid(up)
    pos_diff, neg_diff = (1 - p) * pos, p * neg
    value = (pos_diff ** 2).sum() / (pos.sum() + EPS) + (neg_diff ** 2).sum() / (neg.sum() + EPS)
    return value, float(pos_diff.detach().abs().max()), float(neg_diff.detach().abs().max()), up


def loss_and_gradient(logits, pos, neg, size):
    """The loss kernel's float64 counterpart: logits [B,h4,w4] numpy -> dict(loss, f_max_pos, f_max_neg, dlogit [B,h4,w4], up [B,H,W])."""
    with torch.enable_grad():
        lg = torch.from_numpy(np.asarray(logits, np.float64))[:, None].clone().requires_grad_(True)
        value, fmp, fmn, up = loss(lg, torch.from_numpy(pos), torch.from_numpy(neg), size)
        value.backward()
    return dict(loss=float(value), f_max_pos=fmp, f_max_neg=fmn, dlogit=lg.grad[:, 0].numpy(), up=up.detach()[:, 0].numpy())


def objective(sd, input_data, x, pos, neg, size, insertion_mode):
    """input_data [B,C,h4,w4] float64 (NCHW), x [2C] -> dict(f, grad [2C], f_max_pos, f_max_neg, logits [B,h4,w4], up [B,H,W])."""
    assert insertion_mode in ('after_aspp', 'after_deeplab'), insertion_mode
    with torch.enable_grad():
        x = torch.from_numpy(np.asarray(x, np.float64).astype(np.float32)).double().requires_grad_(True)
        feat = torch.as_tensor(input_data, dtype=torch.float64)
        scale, bias = torch.chunk(x, 2)
        y = feat * (1 + scale).view(1, -1, 1, 1) + bias.view(1, -1, 1, 1)
        if insertion_mode == 'after_aspp':
            y = deeplab_head(sd, y)
        logits = sep_conv_head(sd, y)
        value, fmp, fmn, up = loss(logits, torch.from_numpy(pos), torch.from_numpy(neg), size)
        f = value + REG_WEIGHT * ((scale ** 2).sum() + REG_BIAS_WEIGHT * (bias ** 2).sum())
        f.backward()
    return dict(f=float(f), grad=x.grad.numpy(), f_max_pos=fmp, f_max_neg=fmn, logits=logits.detach()[:, 0].numpy(),
                up=up.detach()[:, 0].numpy())
