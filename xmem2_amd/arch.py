"""Architecture table of the XMem network on the hot path.

The reference builds its network from nn.Modules (model/network.py:18-38,
model/modules.py:102-250, model/resnet.py:117-164).  Here the same network is
described as a flat table: every parameter tensor with the name and shape an
upstream ``XMem.pth`` checkpoint carries (412 tensors), generated in the same
order ``nn.Module.state_dict()`` would emit them, so an upstream checkpoint
loads unchanged and a synthetic one can be produced without torch modules.
"""
from collections import OrderedDict

BN_EPS = 1e-5  # nn.BatchNorm2d default used by model/resnet.py


def _conv(spec, name, cout, cin, k, bias):
    spec[name + '.weight'] = (cout, cin, k, k)
    if bias:
        spec[name + '.bias'] = (cout,)


def _bn(spec, name, c):
    spec[name + '.weight'] = (c,)
    spec[name + '.bias'] = (c,)
    spec[name + '.running_mean'] = (c,)
    spec[name + '.running_var'] = (c,)
    spec[name + '.num_batches_tracked'] = ()


def _bottleneck_layer(spec, prefix, inplanes, planes, blocks, stride):
    """ResNet-50 stage (model/resnet.py:78-114, 141-152)."""
    for b in range(blocks):
        p = f'{prefix}.{b}'
        cin = inplanes if b == 0 else planes * 4
        _conv(spec, p + '.conv1', planes, cin, 1, False); _bn(spec, p + '.bn1', planes)
        _conv(spec, p + '.conv2', planes, planes, 3, False); _bn(spec, p + '.bn2', planes)
        _conv(spec, p + '.conv3', planes * 4, planes, 1, False); _bn(spec, p + '.bn3', planes * 4)
        if b == 0 and (stride != 1 or inplanes != planes * 4):
            _conv(spec, p + '.downsample.0', planes * 4, inplanes, 1, False)
            _bn(spec, p + '.downsample.1', planes * 4)
    return planes * 4


def _basic_layer(spec, prefix, inplanes, planes, blocks, stride):
    """ResNet-18 stage (model/resnet.py:46-75, 141-152)."""
    for b in range(blocks):
        p = f'{prefix}.{b}'
        cin = inplanes if b == 0 else planes
        _conv(spec, p + '.conv1', planes, cin, 3, False); _bn(spec, p + '.bn1', planes)
        _conv(spec, p + '.conv2', planes, planes, 3, False); _bn(spec, p + '.bn2', planes)
        if b == 0 and (stride != 1 or inplanes != planes):
            _conv(spec, p + '.downsample.0', planes, inplanes, 1, False)
            _bn(spec, p + '.downsample.1', planes)
    return planes


def _group_res_block(spec, prefix, cin, cout):
    """GroupResBlock (model/group_modules.py:32-52): downsample registered first."""
    if cin != cout:
        _conv(spec, prefix + '.downsample', cout, cin, 3, True)
    _conv(spec, prefix + '.conv1', cout, cin, 3, True)
    _conv(spec, prefix + '.conv2', cout, cout, 3, True)


def _fusion_block(spec, prefix, x_in, g_in, g_mid, g_out):
    """FeatureFusionBlock (model/modules.py:22-41) with CBAM (model/cbam.py:21-77)."""
    _group_res_block(spec, prefix + '.block1', x_in + g_in, g_mid)
    spec[prefix + '.attention.ChannelGate.mlp.1.weight'] = (g_mid // 16, g_mid)
    spec[prefix + '.attention.ChannelGate.mlp.1.bias'] = (g_mid // 16,)
    spec[prefix + '.attention.ChannelGate.mlp.3.weight'] = (g_mid, g_mid // 16)
    spec[prefix + '.attention.ChannelGate.mlp.3.bias'] = (g_mid,)
    _conv(spec, prefix + '.attention.SpatialGate.spatial.conv', 1, 2, 7, True)
    _group_res_block(spec, prefix + '.block2', g_mid, g_out)


def state_dict_spec(key_dim=64, value_dim=512, hidden_dim=64, single_object=False):
    """name -> shape for every tensor of the reference's state_dict, in order."""
    s = OrderedDict()
    # KeyEncoder: ResNet-50 stem..layer3 (model/modules.py:153-175)
    _conv(s, 'key_encoder.conv1', 64, 3, 7, False); _bn(s, 'key_encoder.bn1', 64)
    c = _bottleneck_layer(s, 'key_encoder.res2', 64, 64, 3, 1)
    c = _bottleneck_layer(s, 'key_encoder.layer2', c, 128, 4, 2)
    c = _bottleneck_layer(s, 'key_encoder.layer3', c, 256, 6, 2)
    # ValueEncoder: ResNet-18 stem..layer3 + fuser + GRU (model/modules.py:102-150)
    extra = 1 if single_object else 2
    _conv(s, 'value_encoder.conv1', 64, 3 + extra, 7, False); _bn(s, 'value_encoder.bn1', 64)
    c = _basic_layer(s, 'value_encoder.layer1', 64, 64, 2, 1)
    c = _basic_layer(s, 'value_encoder.layer2', c, 128, 2, 2)
    c = _basic_layer(s, 'value_encoder.layer3', c, 256, 2, 2)
    _fusion_block(s, 'value_encoder.fuser', 1024, 256, value_dim, value_dim)
    if hidden_dim > 0:
        _conv(s, 'value_encoder.hidden_reinforce.transform', hidden_dim * 3, value_dim + hidden_dim, 3, True)
    # KeyProjection (model/modules.py:194-211)
    _conv(s, 'key_proj.key_proj', key_dim, 1024, 3, True)
    _conv(s, 'key_proj.d_proj', 1, 1024, 3, True)
    _conv(s, 'key_proj.e_proj', key_dim, 1024, 3, True)
    # Decoder (model/modules.py:214-250)
    _fusion_block(s, 'decoder.fuser', 1024, value_dim + hidden_dim, 512, 512)
    if hidden_dim > 0:
        _conv(s, 'decoder.hidden_update.g16_conv', 256, 512, 1, True)
        _conv(s, 'decoder.hidden_update.g8_conv', 256, 256, 1, True)
        _conv(s, 'decoder.hidden_update.g4_conv', 256, 257, 1, True)
        _conv(s, 'decoder.hidden_update.transform', hidden_dim * 3, 256 + hidden_dim, 3, True)
    _conv(s, 'decoder.up_16_8.skip_conv', 512, 512, 3, True)
    _group_res_block(s, 'decoder.up_16_8.out_conv', 512, 256)
    _conv(s, 'decoder.up_8_4.skip_conv', 256, 256, 3, True)
    _group_res_block(s, 'decoder.up_8_4.out_conv', 256, 256)
    _conv(s, 'decoder.pred', 1, 256, 3, True)
    return s


def infer_dims(state_dict):
    """C_k / C_v / C_h from checkpoint tensor shapes (model/network.py:142-154)."""
    key_dim = state_dict['key_proj.key_proj.weight'].shape[0]
    value_dim = state_dict['value_encoder.fuser.block2.conv2.weight'].shape[0]
    if 'decoder.hidden_update.transform.weight' in state_dict:
        hidden_dim = state_dict['decoder.hidden_update.transform.weight'].shape[0] // 3
    else:
        hidden_dim = 0
    return key_dim, value_dim, hidden_dim


def s2m_state_dict_spec():
    """The 368 tensors of the S2M network, deeplabv3plus_resnet50(num_classes=1, output_stride=16)
    (inference/interact/s2m/s2m_network.py:19-35): a ResNet-50 backbone with a 6-channel stem (s2m_resnet.py:92), layer1 and
    layer4 as IntermediateLayerGetter keeps them, and the DeepLabV3+ head (s2m/_deeplab.py:30-45, 136-155), in state_dict order."""
    spec = OrderedDict()
    _conv(spec, 'backbone.conv1', 64, 6, 7, False)
    _bn(spec, 'backbone.bn1', 64)
    c = _bottleneck_layer(spec, 'backbone.layer1', 64, 64, 3, 1)
    c = _bottleneck_layer(spec, 'backbone.layer2', c, 128, 4, 2)
    c = _bottleneck_layer(spec, 'backbone.layer3', c, 256, 6, 2)
    _bottleneck_layer(spec, 'backbone.layer4', c, 512, 3, 2)       # stride replaced by dilation: the same tensors
    _conv(spec, 'classifier.project.0', 48, 256, 1, False)
    _bn(spec, 'classifier.project.1', 48)
    _conv(spec, 'classifier.aspp.convs.0.0', 256, 2048, 1, False)
    _bn(spec, 'classifier.aspp.convs.0.1', 256)
    for i in (1, 2, 3):
        _conv(spec, f'classifier.aspp.convs.{i}.0', 256, 2048, 3, False)
        _bn(spec, f'classifier.aspp.convs.{i}.1', 256)
    _conv(spec, 'classifier.aspp.convs.4.1', 256, 2048, 1, False)
    _bn(spec, 'classifier.aspp.convs.4.2', 256)
    _conv(spec, 'classifier.aspp.project.0', 256, 1280, 1, False)
    _bn(spec, 'classifier.aspp.project.1', 256)
    _conv(spec, 'classifier.classifier.0', 256, 304, 3, False)
    _bn(spec, 'classifier.classifier.1', 256)
    _conv(spec, 'classifier.classifier.3', 1, 256, 1, True)
    return spec


def _separable(spec, prefix, cin, cout):
    """SeparableConv2d (fbrs/model/modeling/basic_blocks.py:57-71): depthwise 3x3, pointwise 1x1, BN (ReLU has no tensors)."""
    spec[prefix + '.body.0.weight'] = (cin, 1, 3, 3)
    _conv(spec, prefix + '.body.1', cout, cin, 1, False)
    _bn(spec, prefix + '.body.2', cout)


def click_state_dict_spec(deeplab_ch=128):
    """The 413 tensors of the click network, get_deeplab_model(backbone='resnet50', deeplab_ch) (inference/interact/fbrs/model/
    is_deeplab_model.py:9-48): rgb_conv, then DeepLabV3Plus (fbrs/model/modeling/deeplab_v3.py:36-46: backbone = ResNet-50-v1s with a
    three-convolution stem, resnetv1b.py:121-146, 240-241; head, skip_project, aspp in that registration order), then the
    SepConvHead (basic_blocks.py:27-54), in state_dict order.  The dilations of layer3 / layer4 add no tensors."""
    ch = int(deeplab_ch)
    spec = OrderedDict()
    _conv(spec, 'rgb_conv.0', 8, 5, 1, True)
    _bn(spec, 'rgb_conv.2', 8)
    _conv(spec, 'rgb_conv.3', 3, 8, 1, True)
    bb = 'feature_extractor.backbone.'
    _conv(spec, bb + 'conv1.0', 64, 3, 3, False); _bn(spec, bb + 'conv1.1', 64)
    _conv(spec, bb + 'conv1.3', 64, 64, 3, False); _bn(spec, bb + 'conv1.4', 64)
    _conv(spec, bb + 'conv1.6', 128, 64, 3, False)
    _bn(spec, bb + 'bn1', 128)
    c = _bottleneck_layer(spec, bb + 'layer1', 128, 64, 3, 1)
    c = _bottleneck_layer(spec, bb + 'layer2', c, 128, 4, 2)
    c = _bottleneck_layer(spec, bb + 'layer3', c, 256, 6, 1)
    c = _bottleneck_layer(spec, bb + 'layer4', c, 512, 3, 1)
    fe = 'feature_extractor.'
    _separable(spec, fe + 'head.block.0', ch + 32, ch)
    _separable(spec, fe + 'head.block.1', ch, ch)
    _conv(spec, fe + 'head.block.2', ch, ch, 1, True)
    _conv(spec, fe + 'skip_project.skip_project.0', 32, 256, 1, False)
    _bn(spec, fe + 'skip_project.skip_project.1', 32)
    _conv(spec, fe + 'aspp.concurent.0.0', ch, c, 1, False); _bn(spec, fe + 'aspp.concurent.0.1', ch)
    for i in (1, 2, 3):
        _conv(spec, fe + f'aspp.concurent.{i}.0', ch, c, 3, False); _bn(spec, fe + f'aspp.concurent.{i}.1', ch)
    _conv(spec, fe + 'aspp.concurent.4.gap.1', ch, c, 1, False); _bn(spec, fe + 'aspp.concurent.4.gap.2', ch)
    _conv(spec, fe + 'aspp.project.0', ch, 5 * ch, 1, False); _bn(spec, fe + 'aspp.project.1', ch)
    _separable(spec, 'head.layers.0', ch, ch // 2)
    _separable(spec, 'head.layers.1', ch // 2, ch // 2)
    _conv(spec, 'head.layers.2', 1, ch // 2, 1, True)
    return spec
