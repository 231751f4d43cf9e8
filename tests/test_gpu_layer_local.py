"""Layer-local parity of the launched networks: one forward pass of the context the bench and the drivers build (bf16, fused pools;
level, mid and carrier launch plans by max_batch), then a walk over the network in Python - for every operation whose input AND
output are materialised end points, the GPU's OWN input end point (exactly representable in the storage type) goes through the
operation in float64 with the weights rounded as the library rounds them, and the GPU's output end point is graded per element by
the bound of tests/conv_bounds.py.  No accumulated-rounding budget: each layer is judged on its own arithmetic, at full size, in the
plan that ships.  Two limits: the head tensors are float32, so their bound is the accumulation term alone (u = 0), which the matrix
cores use to less than 1 % - it catches a wrong bias, scale, tap or channel there, not an error of a few float32 ulps; and `fold_bn`
below copies the library's own folding arithmetic, so a mistake in the fold itself is left to the whole-network tests against the
unfolded oracle (tests/test_gpu_forward.py).

The topology follows oracle/ron_forward.py / oracle/ssd_forward.py (same end-point names).  Their layer functions are not called
directly because the library folds the inference BatchNorm into the weights BEFORE rounding them to the storage type (graph.cpp
Rows::fold_bn, restated by `fold_bn` below in the same float32 operations), and computes the packed launches (`*_hcat` = objectness
hidden | box hidden | inception-1, `*_inc2`) that the oracle keeps as separate tensors.

Operations that are two layers between materialised tensors carry the first layer's bound into the second (conv_bounds docstring):
stem2 (image -> pool1) and the reverse connection (left conv into the reference map, the transposed conv adds in place).
320 / 160 / 80 scales: the first and the last image of the batch; 40 x 40 and below: every image."""
import time

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_bounds as cb  # noqa: E402
from oracle import ron_forward as orf  # noqa: E402
from oracle import ssd_forward as osf  # noqa: E402

F32 = np.float32
RND = {'bf16': orf.round_bf16, 'fp16': orf.round_f16}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def fold_bn(w, b, weights, scope):
    """graph.cpp Rows::fold_bn in the same float32 operations: w * s, (b - mean) * s + beta, s = gamma / sqrt(var + 1e-5)."""
    ga, be, mu, va = (np.asarray(weights[scope + '/BatchNorm/' + k], F32) for k in ('gamma', 'beta', 'moving_mean', 'moving_variance'))
    s = (ga / np.sqrt(va + F32(1e-5))).astype(F32)
    b = np.zeros_like(s) if b is None else np.asarray(b, F32)
    return (np.asarray(w, F32) * s).astype(F32), ((b - mu) * s + be).astype(F32)


class Walk(object):
    """Grades operations one by one; keeps (name, largest ratio) and the failures."""

    def __init__(self, net, n, dtype, tag):
        self.net, self.n, self.dtype, self.tag = net, n, dtype, tag
        self.rnd = RND[dtype]
        self.rows, self.bad, self.cache = [], [], {}

    def ep(self, name):
        if name not in self.cache:
            self.cache = {k: v for k, v in self.cache.items() if k in self.keep}
            self.cache[name] = self.net.end_point(name, self.n).cpu().numpy()
        return self.cache[name]

    keep = ()

    def images(self, h):
        """Every image at 40 x 40 and below; the first and the last (where a plan sized for max_batch goes wrong) above."""
        return list(range(self.n)) if h <= 40 else sorted({0, self.n - 1})

    def grade(self, name, got, ref, S, K, out_dtype=None, extra=0.0, exact=False):
        if exact:
            top, at = (0.0, ()) if np.array_equal(got, ref) else (np.inf, tuple(np.argwhere(got != ref)[0]))
        else:
            top, at = cb.worst(cb.ratio(got, ref, S, K, self.dtype, out_dtype, extra))
        self.rows.append((name, top))
        if top > 1.0:
            self.bad.append('%s: error / bound %.3f at %s (got %r, float64 %r)' % (name, top, at, float(got[at]), float(ref[at])))

    def conv(self, name, x, w, b, got, idx, out_dtype=None, x_slice=None, **op):
        x = x[idx] if x_slice is None else x[idx][..., x_slice[0]:x_slice[1]]
        assert np.array_equal(self.rnd(x), x), name + ': the input end point is not representable in the storage type'
        ref, S, K = cb.conv_op(x, self.rnd(w), b, **op)
        self.grade(name, got[idx].reshape(ref.shape), ref, S, K, out_dtype)

    def report(self):
        worst = max(self.rows, key=lambda r: r[1])
        print('LAYERS %s: %d operations, largest error / bound %.3f (%s)' % (self.tag, len(self.rows), worst[1], worst[0]))
        print('LAYERS %s: %s' % (self.tag, ' '.join('%s=%.2f' % r for r in self.rows)))
        assert not self.bad, '%s: %d operations outside the per-element bound:\n%s' % (self.tag, len(self.bad), '\n'.join(self.bad))


# the VGG body from pool1 on, as both networks launch it with fused pools: (output end point, input end point, conv scope, fused 2x2 pool)
VGG_BODY = [('conv2_1', 'pool1', 'conv2/conv2_1', False), ('pool2', 'conv2_1', 'conv2/conv2_2', True),
            ('conv3_1', 'pool2', 'conv3/conv3_1', False), ('conv3_2', 'conv3_1', 'conv3/conv3_2', False), ('pool3', 'conv3_2', 'conv3/conv3_3', True),
            ('conv4_1', 'pool3', 'conv4/conv4_1', False), ('conv4_2', 'conv4_1', 'conv4/conv4_2', False), ('conv4_3', 'conv4_2', 'conv4/conv4_3', False),
            ('conv5_1', 'pool4', 'conv5/conv5_1', False), ('conv5_2', 'conv5_1', 'conv5/conv5_2', False), ('conv5_3', 'conv5_2', 'conv5/conv5_3', False)]


def _var(weights, scope):
    return lambda name: np.asarray(weights[scope + '/' + name], F32)


def walk_ron(net, weights, variant, n, img, heads, dtype='bf16'):
    W = Walk(net, n, dtype, 'ron %s max_batch %d n %d' % (variant, net.max_batch, n))
    var = _var(weights, 'ron_320_vgg')
    rnd = W.rnd
    # ---- stem2: image -> conv1_1 -> conv1_2 -> pool1 in one kernel (two layers: the first one's bound propagates)
    idx = W.images(320)
    ref, S, K, extra = cb.stem2_op(rnd(img[idx]), rnd(var('conv1/conv1_1/weights')), var('conv1/conv1_1/biases'),
                                   rnd(var('conv1/conv1_2/weights')), var('conv1/conv1_2/biases'), dtype)
    W.grade('stem2', W.ep('pool1')[idx], ref, S, K, extra=extra)
    # ---- VGG body from pool1 on
    for out, src, scope, pool in VGG_BODY:
        x = W.ep(src)
        W.keep = (src, out)
        W.conv(out, x, var(scope + '/weights'), var(scope + '/biases'), W.ep(out), W.images(x.shape[1]), pool=pool)
        if out in ('conv4_3', 'conv5_3'):          # their pool comes from the same launch (or a pool kernel): exact
            p = 'pool%s' % out[4]
            W.grade(p, W.ep(p), cb.pool64(W.ep(out).astype(np.float64)), None, 0, exact=True)
    W.keep = ('pool5', 'fc6', 'fc7', 'conv4_3', 'conv5_3')
    allimg = list(range(n))
    W.conv('fc6', W.ep('pool5'), var('fc6/weights'), var('fc6/biases'), W.ep('fc6'), allimg, rate=3 if variant == 'reducedfc' else 1)
    W.conv('fc7', W.ep('fc6'), var('fc7/weights'), var('fc7/biases'), W.ep('fc7'), allimg)
    # ---- reverse connections and heads, coarse -> fine
    left_src = {'block7': 'fc7', 'block6': 'fc6', 'block5': 'conv5_3', 'block4': 'conv4_3'}
    cls_l, obj_l, loc_l = heads
    prev = None
    for i, L in enumerate(orf.FEAT_LAYERS):
        vs = 'ron_320_vgg/reverse_module/%s_reverse' % L
        v = lambda name, vs=vs: np.asarray(weights[vs + name], F32)      # noqa: E731  (scopes are '<L>_reverse' + suffix)
        W.keep = tuple(left_src.values()) + (L + '_ref', L + '_hcat', L + '_inc2') + ((prev + '_ref',) if prev else ())
        wl, bl = fold_bn(v('_conv_left/weights'), None, weights, vs + '_conv_left')
        left = W.ep(left_src[L])
        if prev is None:
            W.conv(L + '_ref', left, wl, bl, W.ep(L + '_ref'), allimg, stride=2)
        else:
            # left conv writes its half into the reference map, the transposed conv adds its own in place: two layers, one end point
            lref, lS, lK = cb.conv_op(left, rnd(wl), bl)
            delta = cb.bound(lref, lS, lK, dtype)
            ref, S, K = cb.conv_op(W.ep(prev + '_ref'), rnd(v('_deconv_right/weights')), v('_deconv_right/biases'), residual=lref,
                                   stride=2, transpose=True)
            W.grade(L + '_ref', W.ep(L + '_ref'), ref, S, K, extra=delta)
        # hcat = [objectness hidden | box hidden | inception-1 (3x3 | 1x1 in the centre tap)], each with its BatchNorm folded
        w_o, b_o = fold_bn(v('_objectness/weights'), None, weights, vs + '_objectness')
        w_r, b_r = fold_bn(v('/Conv2d_0_3x3/weights'), None, weights, vs + '/Conv2d_0_3x3')
        w_h, b_h = _inception(v, weights, vs, '_inception1', 512)
        W.conv(L + '_hcat', W.ep(L + '_ref'), np.concatenate([w_o, w_r, w_h], axis=3), np.concatenate([b_o, b_r, b_h]), W.ep(L + '_hcat'), allimg)
        w_i, b_i = _inception(v, weights, vs, '_inception2', 1024)
        W.conv(L + '_inc2', W.ep(L + '_hcat'), w_i, b_i, W.ep(L + '_inc2'), allimg, x_slice=(1024, 2048))
        W.conv(L + ' objectness', W.ep(L + '_hcat'), v('_objectness_score/weights'), v('_objectness_score/biases'), obj_l[i], allimg,
               out_dtype='fp32', x_slice=(0, 512), relu=False)
        W.conv(L + ' loc', W.ep(L + '_hcat'), v('/Conv2d_1_3x3/weights'), v('/Conv2d_1_3x3/biases'), loc_l[i], allimg, out_dtype='fp32',
               x_slice=(512, 1024), relu=False)
        W.conv(L + ' cls', W.ep(L + '_inc2'), v('_inception2/Conv2d_pred_3x3/weights'), v('_inception2/Conv2d_pred_3x3/biases'), cls_l[i], allimg,
               out_dtype='fp32', relu=False)
        prev = L
    return W


def _inception(v, weights, vs, blk, cin):
    """(3x3 || 1x1) -> concat -> BatchNorm as one 3x3 convolution: the 1x1 branch in the centre tap, each half with its BN half."""
    w3, w1 = v(blk + '/Branch_0/Conv2d_3x3/weights'), v(blk + '/Branch_1/Conv2d_1x1/weights')
    wc = np.zeros((3, 3, cin, 512), F32)
    wc[1, 1] = w1[0, 0]
    w = np.concatenate([w3, wc], axis=3)
    b = np.concatenate([v(blk + '/Branch_0/Conv2d_3x3/biases'), v(blk + '/Branch_1/Conv2d_1x1/biases')])
    return fold_bn(w, b, weights, vs + blk)


@pytest.fixture(scope='module')
def synth():
    from ron_tensorflow_amd.weights import synthetic_weights
    cache = {}

    def get(variant):
        if variant not in cache:
            cache.clear()
            cache[variant] = synthetic_weights(variant, seed=1 if variant == 'reducedfc' else 2)
        return cache[variant]
    return get


@pytest.mark.parametrize('max_batch,n', [(1, 1), (12, 12), (16, 16), (16, 13), (32, 32)])
@pytest.mark.parametrize('variant', ['reducedfc', 'full'])
def test_ron_320_layer_by_layer(dev, synth, variant, max_batch, n):
    from ron_tensorflow_amd.nets import nets_factory
    from ron_tensorflow_amd.weights import synthetic_images
    weights = synth(variant)
    img = synthetic_images(n, seed=30 + n)
    cls = nets_factory.get_network('ron_320_vgg')
    net = cls(variant=variant, dtype='bf16', max_batch=max_batch, device=dev, fuse_pools=True)
    net.load_weights(weights)
    t0 = time.time()
    try:
        heads = [[t.cpu().numpy().reshape(t.shape[0], t.shape[1], t.shape[2], -1) for t in grp] for grp in net.forward_heads(torch.from_numpy(img).to(dev))]
        assert not _has(net, 'conv1_1', n)                   # fused into stem2: no end point, so no operation of its own here
        W = walk_ron(net, weights, variant, n, img, heads)
    finally:
        net.close()
    print('LAYERS %s: float64 walk %.1f s' % (W.tag, time.time() - t0))
    assert len(W.rows) == 1 + 11 + 2 + 2 + 4 * 6
    W.report()


# --------------------------------------------------------------------------------------------------------------------- #
# SSD-512
# --------------------------------------------------------------------------------------------------------------------- #
def _pad_conv64(x, w, b, stride, pad, relu=True):
    """oracle.ssd_forward.conv2d_pad_np (explicit symmetric padding, VALID) as conv_op's (ref64, S, K)."""
    def run(x_, w_, b_, act):
        xp = np.pad(np.asarray(x_, np.float64), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
        kh = w_.shape[0]
        n, hp, wp, cin = xp.shape
        ho, wo = (hp - kh) // stride + 1, (wp - kh) // stride + 1
        out = np.zeros((n * ho * wo, w_.shape[3]), np.float64)
        for ky in range(kh):
            for kx in range(kh):
                out += xp[:, ky: ky + (ho - 1) * stride + 1: stride, kx: kx + (wo - 1) * stride + 1: stride, :].reshape(-1, cin) @ np.asarray(w_[ky, kx], np.float64)
        y = out.reshape(n, ho, wo, -1) + np.asarray(b_, np.float64)
        return np.maximum(y, 0) if act and relu else y
    return run(x, w, b, True), run(np.abs(x), np.abs(w), np.abs(b), False), w.shape[0] * w.shape[1] * w.shape[2]


def test_ssd_512_layer_by_layer(dev):
    """SSD-512 bf16 at max_batch 2: the VGG body, conv6 (rate 6) / conv7, the extra blocks (1x1 -> 3x3 stride 2 with explicit padding;
    block12: 4x4), the 3x3 stride-1 pool5 (exact), block4's L2 normalisation (float64 reference, u |ref| + C 2^-23 S for its
    C = 512 channel sum of squares), and the class + box convolutions of every feature layer (one launch, two fp32 tensors)."""
    from ron_tensorflow_amd.nets import nets_factory
    from ron_tensorflow_amd.weights import ssd_synthetic_weights, synthetic_images
    n, dtype = 2, 'bf16'
    weights = ssd_synthetic_weights(seed=3)
    img = synthetic_images(n, seed=5, img_shape=(512, 512))
    cls = nets_factory.get_network('ssd_512_vgg')
    net = cls(dtype=dtype, max_batch=2, device=dev, fuse_pools=True)
    net.load_weights(weights)
    try:
        cls_l, _, loc_l = net.forward_heads(torch.from_numpy(img).to(dev))
        cls_l = [t.cpu().numpy().reshape(t.shape[0], t.shape[1], t.shape[2], -1) for t in cls_l]
        loc_l = [t.cpu().numpy().reshape(t.shape[0], t.shape[1], t.shape[2], -1) for t in loc_l]
        W = Walk(net, n, dtype, 'ssd512 max_batch 2')
        var = _var(weights, osf.SCOPE)
        rnd = W.rnd
        allimg = [0, 1]
        W.keep = ('pool1',)
        assert not _has(net, 'conv1_1', n)                   # fused into stem2: no end point, so no operation of its own here
        ref, S, K, extra = cb.stem2_op(rnd(img), rnd(var('conv1/conv1_1/weights')), var('conv1/conv1_1/biases'),
                                       rnd(var('conv1/conv1_2/weights')), var('conv1/conv1_2/biases'), dtype)
        W.grade('stem2', W.ep('pool1'), ref, S, K, extra=extra)
        for out, src, scope, pool in VGG_BODY:
            W.keep = (src, out, 'conv4_3')
            W.conv(out, W.ep(src), var(scope + '/weights'), var(scope + '/biases'), W.ep(out), allimg, pool=pool)
            if out == 'conv4_3':
                W.grade('pool4', W.ep('pool4'), cb.pool64(W.ep(out).astype(np.float64)), None, 0, exact=True)
        W.keep = ('conv4_3', 'conv5_3', 'pool5', 'conv6', 'conv7')
        W.grade('pool5', W.ep('pool5'), osf.max_pool3x3_s1_np(W.ep('conv5_3')), None, 0, exact=True)
        W.conv('conv6', W.ep('pool5'), var('conv6/weights'), var('conv6/biases'), W.ep('conv6'), allimg, rate=6)
        W.conv('conv7', W.ep('conv6'), var('conv7/weights'), var('conv7/biases'), W.ep('conv7'), allimg)
        src = 'conv7'
        for b in range(8, 13):
            B = 'block%d' % b
            W.keep = (src, B + '_mid', B, 'conv4_3', 'conv7') + tuple('block%d' % k for k in range(8, 13))
            W.conv(B + '_mid', W.ep(src), var(B + '/conv1x1/weights'), var(B + '/conv1x1/biases'), W.ep(B + '_mid'), allimg)
            leaf = 'conv3x3' if b < 12 else 'conv4x4'
            x = W.ep(B + '_mid')
            ref, S, K = _pad_conv64(x, rnd(var(B + '/%s/weights' % leaf)), var(B + '/%s/biases' % leaf), 2 if b < 12 else 1, 1)
            W.grade(B, W.ep(B), ref, S, K)
            src = B
        # block4: L2 normalisation over the 512 channels, x * rsqrt(max(sum x^2, 1e-12)) * gamma
        x = W.ep('conv4_3').astype(np.float64)
        gamma = var('block4_box/L2Normalization/gamma').astype(np.float64)
        ss = np.maximum((x * x).sum(axis=-1, keepdims=True), 1e-12)
        ref = x / np.sqrt(ss) * gamma
        # the C = 512-term float32 sum of squares (bf16 squares are exact in float32: C 2^-23, relative, all terms positive), then
        # 1 / sqrt and two multiplications: every term is relative to |ref|, so S = |ref| and K = C
        W.grade('block4_norm', W.ep('block4_norm'), ref, np.abs(ref), 512)
        feat = ['block4_norm', 'conv7'] + ['block%d' % b for b in range(8, 13)]
        for i, (layer, t) in enumerate(zip(osf.FEAT_LAYERS, feat)):
            x = W.ep(t)
            for kind, got in (('conv_cls', cls_l[i]), ('conv_loc', loc_l[i])):
                W.conv('%s %s' % (layer, kind), x, var(layer + '_box/%s/weights' % kind), var(layer + '_box/%s/biases' % kind), got, allimg,
                       out_dtype='fp32', relu=False)
    finally:
        net.close()
    assert len(W.rows) == 1 + 11 + 2 + 2 + 5 * 2 + 1 + 7 * 2      # stem2, body, pool4 / pool5, conv6 / conv7, blocks 8-12, L2 norm, heads
    W.report()


def _has(net, name, n):
    try:
        net.end_point(name, n)
        return True
    except Exception:      # noqa: BLE001  (ron_end_point_copy refuses tensors that are not materialised, by name)
        return False
