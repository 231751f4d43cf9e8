"""CPU reference of SSD-300: an fp32 NHWC restatement of ``ssd_net`` of nets/ssd_vgg_300.py:434-523 (test infrastructure).

Built from the oracle's primitives (oracle/ron_forward.py BACKENDS, oracle/ssd_forward.py conv2d_pad_np / max_pool3x3_s1_np /
l2_normalization, oracle/np_post.py softmax_last) plus the one layer the other networks do not have: the SAME 2x2 stride-2 pool on an
odd map (75 -> 38: ceil, the last window holds one row / column), with a numpy and a torch back-end.

What is pinned and what is not: conv1_1 .. conv7 - the odd pool3 included - are pinned to the reference's own torch ``VGG16``
(convert_pytorch_vgg.py:37-57, whose pool3 is the ceil_mode 'C' pool) by golden G9 (tests/golden/g9_vgg_backbone_300.npz); the anchors
are pinned by g9_anchors_ssd300.npz (the reference's numpy function).  Blocks 8-11 and the multibox heads are TensorFlow graph code with
no executable form in the reference: **parity unpinned**, cross-checked between the numpy and the torch-CPU operators, as for SSD-512.
"""
import numpy as np

from oracle import np_post
from oracle import ssd_forward as osf
from oracle.ron_forward import BACKENDS, F32

SCOPE = 'ssd_300_vgg'
FEAT_LAYERS = ['block4', 'block7', 'block8', 'block9', 'block10', 'block11']
# SSDNet.default_params, nets/ssd_vgg_300.py:94-124
SSD300 = dict(
    img_shape=(300, 300),
    feat_shapes=[(38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1)],
    anchor_sizes=[(21., 45.), (45., 99.), (99., 153.), (153., 207.), (207., 261.), (261., 315.)],
    anchor_ratios=[[2, .5], [2, .5, 3, 1. / 3], [2, .5, 3, 1. / 3], [2, .5, 3, 1. / 3], [2, .5], [2, .5]],
    anchor_steps=[8, 16, 32, 64, 100, 300],
    anchor_offset=0.5,
    normalizations=[20, -1, -1, -1, -1, -1],
    prior_scaling=[0.1, 0.1, 0.2, 0.2],
)
# blocks 8-11 (nets/ssd_vgg_300.py:484-506): 1x1 to `mid`, then 3x3 to `out` with (stride, explicit zero padding)
EXTRA = [(8, 2, 1), (9, 2, 1), (10, 1, 0), (11, 1, 0)]


def anchors_all_layers():
    return osf.anchors_all_layers(SSD300)


def max_pool2x2_same_np(x):
    """slim.max_pool2d [2, 2] stride 2 SAME: ceil(H/2) x ceil(W/2); the padding never wins the max."""
    n, h, w, c = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    xp = np.pad(x, ((0, 0), (0, 2 * ho - h), (0, 2 * wo - w), (0, 0)), constant_values=-np.inf)
    return xp.reshape(n, ho, 2, wo, 2, c).max(axis=(2, 4))


def max_pool2x2_same_torch(x):
    import torch
    import torch.nn.functional as Fn
    xt = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)
    return Fn.max_pool2d(xt, 2, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous().numpy()


def ssd300_forward(images, weights, num_classes=21, round_fn=None, collect=None, backend='numpy', stop_after=None):
    """(predictions, localisations, logits, end_points) like SSDNet.net; backend 'torch' swaps every conv / pool for the torch-CPU
    operator; stop_after='block7' returns after the VGG backbone (the G9 pin needs conv1_1 .. conv7 weights only)."""
    rnd = round_fn if round_fn is not None else (lambda a: a)
    conv_same = BACKENDS[backend][0]
    conv_pad = osf.conv2d_pad_np if backend == 'numpy' else osf.conv2d_pad_torch
    pool2 = max_pool2x2_same_np if backend == 'numpy' else max_pool2x2_same_torch
    pool3 = osf.max_pool3x3_s1_np if backend == 'numpy' else osf.max_pool3x3_s1_torch

    def var(name):
        return np.asarray(weights[SCOPE + '/' + name], dtype=F32)

    def conv(x, scope, stride=1, rate=1, pad=None, relu=True):
        w = var(scope + '/weights')
        y = conv_same(rnd(x), rnd(w), stride, rate) if pad is None else conv_pad(rnd(x), rnd(w), stride, rate, pad)
        y = y + var(scope + '/biases')
        return np.maximum(y, 0) if relu else y

    end_points = {}
    x = np.asarray(images, dtype=F32)
    for bi, reps in enumerate([2, 2, 3, 3, 3]):
        for r in range(reps):
            x = conv(x, 'conv%d/conv%d_%d' % (bi + 1, bi + 1, r + 1))
            if collect is not None:
                collect['conv%d_%d' % (bi + 1, r + 1)] = x
        end_points['block%d' % (bi + 1)] = x
        x = pool2(x) if bi < 4 else pool3(x)
        if collect is not None:
            collect['pool%d' % (bi + 1)] = x
    x = conv(x, 'conv6', rate=6)
    end_points['block6'] = x
    x = conv(x, 'conv7')
    end_points['block7'] = x
    if collect is not None:
        collect['conv6'], collect['conv7'] = end_points['block6'], end_points['block7']
    if stop_after == 'block7':
        return None, None, None, end_points
    for b, stride, pad in EXTRA:
        x = conv(x, 'block%d/conv1x1' % b)
        if collect is not None:
            collect['block%d_mid' % b] = x
        x = conv(x, 'block%d/conv3x3' % b, stride=stride, pad=pad)
        end_points['block%d' % b] = x
    predictions, logits, localisations = [], [], []
    for i, layer in enumerate(FEAT_LAYERS):
        net = end_points[layer]
        if SSD300['normalizations'][i] > 0:
            net = osf.l2_normalization(net, var(layer + '_box/L2Normalization/gamma'))
            if collect is not None:
                collect[layer + '_norm'] = net
        a = len(SSD300['anchor_sizes'][i]) + len(SSD300['anchor_ratios'][i])
        loc = conv(net, layer + '_box/conv_loc', relu=False)
        cls = conv(net, layer + '_box/conv_cls', relu=False)
        n, h, w, _ = net.shape
        loc = loc.reshape(n, h, w, a, 4).astype(F32)
        cls = cls.reshape(n, h, w, a, num_classes).astype(F32)
        predictions.append(np_post.softmax_last(cls))
        logits.append(cls)
        localisations.append(loc)
    return predictions, localisations, logits, end_points


def macs_per_image(variable_shapes):
    """MACs of one image from the variable shapes and the map sizes: every convolution's kh*kw*cin*cout times its output pixels
    (FLOPs = 2 x MACs over convolutions and heads; pools, ReLU, L2 norm and softmax are not counted)."""
    px = {}
    h = 300
    for b in range(1, 6):
        for r in range(1, 4):
            px['conv%d/conv%d_%d' % (b, b, r)] = h * h
        if b < 5:
            h = (h + 1) // 2                   # SAME 2x2 pools; pool5 is 3x3 stride 1
    px['conv6'] = px['conv7'] = h * h          # 19 x 19
    for b, stride, pad in EXTRA:
        px['block%d/conv1x1' % b] = h * h
        h = (h + 2 * pad - 3) // stride + 1
        px['block%d/conv3x3' % b] = h * h
    for layer, (fh, fw) in zip(FEAT_LAYERS, SSD300['feat_shapes']):
        px[layer + '_box/conv_loc'] = px[layer + '_box/conv_cls'] = fh * fw
    total = 0
    for name, shape in variable_shapes:
        if name.endswith('/weights'):
            total += int(np.prod(shape)) * px[name[len(SCOPE) + 1:-len('/weights')]]
    return total
