"""SSD-512 (VGG) network object with the interface of the reference's ``nets/ssd_vgg_512.py`` (BASELINE config 5).

``SSDNet`` keeps names / defaults / return arity of the reference class (nets/ssd_vgg_512.py:63-218): ``net`` returns
``(predictions, localisations, logits, end_points)``; ``detected_bboxes`` is select -> top-k sort -> NMS with no clipping
and no min-size filter (:182-201).  Everything runs through libron_hip.so (ron_ctx variant RON_VARIANT_SSD512)."""
import contextlib
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check, current_stream, lib, ptr
from . import ron_vgg_320
from .ron_vgg_320 import RONNet

# same field names as the reference namedtuple (nets/ssd_vgg_512.py:44-60)
SSDParams = namedtuple('SSDParameters', ['img_shape', 'num_classes', 'no_annotation_label', 'feat_layers', 'feat_shapes',
                                         'anchor_size_bounds', 'anchor_sizes', 'anchor_ratios', 'anchor_steps',
                                         'anchor_offset', 'normalizations', 'prior_scaling'])


_LOSS_KEYS = ('cross_entropy_pos', 'cross_entropy_neg', 'localization', 'total')
_NO_BORDER = 1 << 24       # allowed border of ron_bboxes_encode under which the inside test never fails for a finite anchor


class _SSDLossesFunction(torch.autograd.Function):
    """SSDNet.losses for head tensors that require grad.  forward: one ron_ssd_losses_grad call, the unit gradients saved; backward:
    the localisation gradient times (upstream of its term + upstream of the total), and the class gradient, whose rows belong to
    the positive or to the mined set, times the upstream of that row's term + the upstream of the total: torch multiplies on the
    device.  The inputs are (number of layers, (gclasses, glocalisations, gscores), loss keyword arguments, then the logits and
    localisations of every layer); the outputs the four losses as one tensor [4] and the counts."""

    @staticmethod
    def forward(ctx, num_layers, fixed, kwargs, *heads):
        logits, localisations = list(heads[:num_layers]), list(heads[num_layers:])
        gclasses, glocalisations, gscores = fixed
        out, counts, _, d_cls, d_loc = ops.ssd_losses_grad(logits, localisations, gclasses, glocalisations, gscores, **kwargs)
        ctx.save_for_backward(*(d_cls + d_loc + list(gscores)))
        ctx.num_layers, ctx.match_threshold = num_layers, float(kwargs['match_threshold'])
        ctx.mark_non_differentiable(counts)
        return out, counts

    @staticmethod
    def backward(ctx, g, _g_counts):
        n = ctx.num_layers
        saved = ctx.saved_tensors
        d_cls, d_loc, gscores = saved[:n], saved[n:2 * n], saved[2 * n:]
        s_pos, s_neg, s_loc = g[0] + g[3], g[1] + g[3], g[2] + g[3]              # 0-d tensors on the device
        grads = [d * torch.where(sc > ctx.match_threshold, s_pos, s_neg).unsqueeze(-1) if ctx.needs_input_grad[3 + i] else None
                 for i, (d, sc) in enumerate(zip(d_cls, gscores))]
        grads += [d * s_loc if ctx.needs_input_grad[3 + n + i] else None for i, d in enumerate(d_loc)]
        return (None, None, None) + tuple(grads)


class SSDNet(RONNet):
    """SSD VGG-based 512 network: conv4 64x64, conv7 32x32, conv8 16x16, conv9 8x8, conv10 4x4, conv11 2x2, conv12 1x1."""
    default_params = SSDParams(
        img_shape=(512, 512),
        num_classes=21,
        no_annotation_label=21,
        feat_layers=['block4', 'block7', 'block8', 'block9', 'block10', 'block11', 'block12'],
        feat_shapes=[(64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1)],
        anchor_size_bounds=[0.10, 0.90],
        anchor_sizes=[(20.48, 51.2), (51.2, 133.12), (133.12, 215.04), (215.04, 296.96), (296.96, 378.88),
                      (378.88, 460.8), (460.8, 542.72)],
        anchor_ratios=[[2, .5], [2, .5, 3, 1. / 3], [2, .5, 3, 1. / 3], [2, .5, 3, 1. / 3], [2, .5, 3, 1. / 3], [2, .5], [2, .5]],
        anchor_steps=[8, 16, 32, 64, 128, 256, 512],
        anchor_offset=0.5,
        normalizations=[20, -1, -1, -1, -1, -1, -1],
        prior_scaling=[0.1, 0.1, 0.2, 0.2])

    _variant = 'ssd512'        # _lib.VARIANTS key of the context this class builds (ssd_vgg_300.SSDNet: 'ssd300')
    _mining = 'layer'          # ssd_losses selects its hard negatives per feature layer here, over the batch in ssd_vgg_300

    def __init__(self, params=None, dtype='bf16', max_batch=16, device=None, fuse_pools=False):
        self.params = params if isinstance(params, SSDParams) else type(self).default_params
        if dtype not in _lib.DTYPES:
            raise ValueError('Unknown dtype %s' % dtype)
        self.variant, self.dtype, self.max_batch, self.fuse_pools = self._variant, dtype, max_batch, fuse_pools
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._ctx = None
        self._anchors_dev = None

    def _head_buffers(self, n):
        geom, nc = self._head_geometry()             # from the context, not from params.feat_shapes (update_feature_shapes)
        cls, loc = [], []
        for (fh, fw, a) in geom:
            cls.append(torch.empty((n, fh, fw, a, nc), dtype=torch.float32, device=self.device))
            loc.append(torch.empty((n, fh, fw, a, 4), dtype=torch.float32, device=self.device))
        return cls, None, loc

    def forward_heads(self, inputs):
        """Conv stack only: (logits, None, localisations)."""
        inputs = inputs.to(self.device, torch.float32).contiguous()
        n = inputs.shape[0]
        assert tuple(inputs.shape[1:]) == tuple(self.params.img_shape) + (3,)
        cls, _, loc = self._head_buffers(n)
        hd = _lib.Heads()
        for i in range(len(cls)):
            hd.cls[i], hd.loc[i] = cls[i].data_ptr(), loc[i].data_ptr()
        check(lib().ron_forward(self._context(), ptr(inputs), n, C.byref(hd), current_stream()))
        return cls, None, loc

    def net(self, inputs, is_training=True, update_feat_shapes=True, dropout_keep_prob=0.5, prediction_fn=None, reuse=None,
            scope='ssd_512_vgg', end_points=('block4', 'block7', 'block8', 'block9', 'block10', 'block11', 'block12')):
        """nets/ssd_vgg_512.py:108-133 -> (predictions, localisations, logits, end_points)."""
        nchw = getattr(self, '_data_format', 'NHWC') == 'NCHW'
        if nchw:
            inputs = inputs.permute(0, 2, 3, 1)
        logits, _, localisations = self.forward_heads(inputs)
        fn = prediction_fn if prediction_fn is not None else ops.softmax_last
        predictions = [fn(l) for l in logits]
        eps = {name: self.end_point(name, inputs.shape[0]) for name in (end_points or ())}
        if nchw:
            eps = {k: v.permute(0, 3, 1, 2).contiguous() for k, v in eps.items()}
        if update_feat_shapes:                       # nets/ssd_vgg_512.py:134-136: the feature shapes follow the predictions
            self.update_feature_shapes(predictions)
        return predictions, localisations, logits, eps

    def update_feature_shapes(self, predictions):
        """nets/ssd_vgg_512.py:141-146 -> ssd_feat_shapes_from_net (nets/ssd_vgg_300.py:282-303): feat_shapes become the
        [H, W, A] of every prediction tensor ([N, H, W, A, C]); anchors() reads the first two entries like the reference's."""
        self.params = self.params._replace(feat_shapes=[[int(d) for d in p.shape[1:4]] for p in predictions])

    def anchors(self, img_shape, dtype=np.float32):
        """nets/ssd_vgg_512.py:148-157: list of (y, x, h, w) per layer."""
        p = self.params
        out = []
        for i, s in enumerate(p.feat_shapes):
            fh, fw = int(s[0]), int(s[1])
            sizes, ratios = p.anchor_sizes[i], p.anchor_ratios[i]
            na = len(sizes) + len(ratios)
            y = np.empty((fh, fw, 1), np.float32)
            x = np.empty((fh, fw, 1), np.float32)
            h = np.empty((na,), np.float32)
            w = np.empty((na,), np.float32)
            sz = (C.c_double * len(sizes))(*[float(v) for v in sizes])
            rt = (C.c_double * max(len(ratios), 1))(*[float(v) for v in ratios])
            check(lib().ron_ssd_anchor_one_layer(int(img_shape[0]), int(img_shape[1]), fh, fw, sz, len(sizes), rt, len(ratios),
                                                 float(p.anchor_steps[i]), float(p.anchor_offset), ptr(y), ptr(x), ptr(h), ptr(w)))
            out.append((y.astype(dtype, copy=False), x.astype(dtype, copy=False), h.astype(dtype, copy=False), w.astype(dtype, copy=False)))
        return out

    def detected_bboxes(self, predictions, localisations, select_threshold=None, nms_threshold=0.5, clipping_bbox=None,
                        top_k=400, keep_top_k=200, nms_mode='min'):
        """nets/ssd_vgg_512.py:182-201: select -> sort -> NMS; `clipping_bbox` is accepted and ignored like there."""
        from .. import tfe
        return tfe.detected_bboxes(predictions, localisations, num_classes=self.params.num_classes,
                                   select_threshold=select_threshold, nms_threshold=nms_threshold, clipping_bbox=None,
                                   top_k=top_k, keep_top_k=keep_top_k, nms_mode=nms_mode, min_size=None)

    # ------------------------------------------------------------------ label side (gradients stop at the head tensors)
    def bboxes_encode(self, labels, bboxes, anchors, scope=None):
        """Ground truth -> per-anchor targets (nets/ssd_vgg_512.py:161-171, nets/ssd_vgg_300.py:191-201) on the GPU.  The reference's
        own call hands five arguments to the eight-argument ssd_common.tf_ssd_bboxes_encode and cannot run; its evident intent is
        the contract: a match at an overlap of 0.5 or more, no ignore band, no border restriction.  One image, labels [G] and bboxes
        [G, 4] (outputs without a batch axis), or a padded batch [N, G] / [N, G, 4] with label 0 as padding behind the present rows,
        as in RONNet.bboxes_encode; returns its four per-layer lists."""
        glabels, gbboxes, single = self._ground_truth(labels, bboxes)
        adev = ops.anchors_to_device(anchors, self.device)
        shapes = [(int(np.shape(y)[0]), int(np.shape(y)[1]), int(np.size(h))) for (y, x, h, w) in anchors]
        out = ops.bboxes_encode(glabels, gbboxes, adev, shapes, self.params.img_shape, [_NO_BORDER] * len(shapes), 0.5, 0.5,
                                tuple(self.params.prior_scaling))
        return tuple([t[0] for t in lst] for lst in out) if single else out

    def losses(self, logits, localisations, gclasses, glocalisations, gscores, match_threshold=0.5, negative_ratio=3., alpha=1.,
               label_smoothing=0., scope='ssd_losses'):
        """The SSD losses (nets/ssd_vgg_512.py:203-218 -> ssd_losses, :516-607: hard negatives per feature layer; ssd_vgg_300.SSDNet
        -> nets/ssd_vgg_300.py:580-659: over the whole batch) of a batch, one ron_ssd_losses call.  `label_smoothing` is accepted
        and unused, as in the reference.  Returns 0-d GPU tensors {'cross_entropy_pos', 'cross_entropy_neg', 'localization',
        'total'} and 'counts' (int32 [S, 4], ops.SSD_LOSS_COUNTS per segment: S = 1 over the batch, the number of layers else).
        When autograd is enabled and a tensor of `logits` or `localisations` requires grad, the four scalars are differentiable with
        respect to those tensors (ron_ssd_losses_grad, one call; the same values bit for bit); the mining threshold is a constant."""
        kwargs = dict(mining=self._mining, match_threshold=match_threshold, negative_ratio=negative_ratio, alpha=alpha)
        heads = list(logits) + list(localisations)
        if torch.is_grad_enabled() and any(t.requires_grad for t in heads):
            out, counts = _SSDLossesFunction.apply(len(logits), (gclasses, glocalisations, gscores), kwargs, *heads)
        else:
            out, counts, _ = ops.ssd_losses(logits, localisations, gclasses, glocalisations, gscores, **kwargs)
        res = {k: out[i] for i, k in enumerate(_LOSS_KEYS)}
        res['counts'] = counts
        return res

    def losses_and_gradients(self, logits, localisations, gclasses, glocalisations, gscores, match_threshold=0.5, negative_ratio=3.,
                             alpha=1., label_smoothing=0., scope='ssd_losses'):
        """`losses` and, from the same call (ron_ssd_losses_grad), 'gradients': {'logits', 'localisations'}: per-layer lists of
        float32 GPU tensors shaped like the inputs, d (cross_entropy_pos + cross_entropy_neg) / d logits and d localization /
        d localisations; each term reads one head tensor, so these are also the gradients of 'total'.  The loss values are those of
        `losses` bit for bit."""
        with torch.no_grad():
            out, counts, _, d_cls, d_loc = ops.ssd_losses_grad(logits, localisations, gclasses, glocalisations, gscores,
                                                               mining=self._mining, match_threshold=match_threshold,
                                                               negative_ratio=negative_ratio, alpha=alpha)
        res = {k: out[i] for i, k in enumerate(_LOSS_KEYS)}
        res.update(counts=counts, gradients={'logits': d_cls, 'localisations': d_loc})
        return res

    def validation_losses(self, images, glabels, gbboxes, **loss_kwargs):
        """Held-out loss of a labelled batch: net() -> bboxes_encode (on the network's own anchors) -> losses, all on the device;
        no host copy in between.  glabels [N, G] (0 = padding), gbboxes [N, G, 4]; loss_kwargs go to `losses`."""
        _, localisations, logits, _ = self.net(images, is_training=False, update_feat_shapes=False, end_points=())
        glabels, gbboxes, _ = self._ground_truth(glabels, gbboxes)
        hd = _lib.Heads()
        check(lib().ron_heads_describe(self._context(), C.byref(hd)))
        gclasses, glocalisations, gscores, _ = ops.bboxes_encode(
            glabels, gbboxes, None, None, self.params.img_shape, [_NO_BORDER] * int(hd.num_layers), 0.5, 0.5,
            tuple(self.params.prior_scaling), heads=hd)
        return self.losses(logits, localisations, gclasses, glocalisations, gscores, **loss_kwargs)

    def detect(self, inputs, select_threshold=0.01, nms_threshold=0.45, top_k=400, bbox_img=(0., 0., 1., 1.), out=None):
        """forward + np_methods post-processing (no objectness gate for SSD)."""
        return RONNet.detect(self, inputs, objectness_thres=0.0, select_threshold=select_threshold,
                             nms_threshold=nms_threshold, top_k=top_k, bbox_img=bbox_img, out=out)

    def detect_tfe(self, inputs, select_threshold=None, nms_threshold=0.5, clipping_bbox=None, top_k=400, keep_top_k=200,
                   nms_mode='min', out=None):
        """forward + detected_bboxes in one enqueue (ron_detect_tfe), as SSDNet.detected_bboxes: no objectness gate, no size
        filter, `clipping_bbox` accepted and ignored."""
        return self._detect_tfe(inputs, 0.0, select_threshold, nms_threshold, None, top_k, keep_top_k, nms_mode, None,
                                out).as_dicts()


# ---------------------------------------------------------------------- the reference's function entries (nets_factory.networks_map)
def _ssd_net_fn(cls, inputs, num_classes, feat_layers, anchor_sizes, anchor_ratios, normalizations, is_training, dropout_keep_prob,
                prediction_fn, reuse, scope, weights, dtype, max_batch):
    """ssd_net of either SSD module: a scope name owns one network object of class `cls`, like ron_vgg_320.ron_net."""
    params = cls.default_params._replace(num_classes=num_classes, feat_layers=list(feat_layers), anchor_sizes=list(anchor_sizes),
                                         anchor_ratios=list(anchor_ratios), normalizations=list(normalizations))
    dev = inputs.device if inputs.is_cuda else torch.device('cuda', torch.cuda.current_device())
    key = (scope, cls._variant, num_classes, dtype, str(dev))
    net = ron_vgg_320._scoped_net(key, lambda: cls(params, dtype=dtype, max_batch=max(max_batch, inputs.shape[0]), device=dev), weights, reuse)
    fmt = ron_vgg_320._ARG_SCOPE_FORMAT[-1] if ron_vgg_320._ARG_SCOPE_FORMAT else 'NHWC'
    with ron_vgg_320._DataFormatScope([net], fmt):
        return net.net(inputs, is_training=is_training, update_feat_shapes=False, dropout_keep_prob=dropout_keep_prob,
                       prediction_fn=prediction_fn, reuse=reuse, scope=scope)


def ssd_net(inputs, num_classes=SSDNet.default_params.num_classes, feat_layers=SSDNet.default_params.feat_layers,
            anchor_sizes=SSDNet.default_params.anchor_sizes, anchor_ratios=SSDNet.default_params.anchor_ratios,
            normalizations=SSDNet.default_params.normalizations, is_training=True, dropout_keep_prob=0.5, prediction_fn=None,
            reuse=None, scope='ssd_512_vgg', weights=None, dtype='bf16', max_batch=16):
    """SSD net definition (nets/ssd_vgg_512.py:364-460): (predictions, localisations, logits, end_points).  A scope name owns one
    network object, like ron_vgg_320.ron_net: the first call needs `weights=`."""
    return _ssd_net_fn(SSDNet, inputs, num_classes, feat_layers, anchor_sizes, anchor_ratios, normalizations, is_training,
                       dropout_keep_prob, prediction_fn, reuse, scope, weights, dtype, max_batch)


ssd_net.default_image_size = 512


def _ssd_losses_fn(mining, logits, localisations, gclasses, glocalisations, gscores, match_threshold, negative_ratio, alpha):
    net = SSDNet.__new__(SSDNet)                       # losses() reads nothing of the object but the mining mode
    net._mining = mining
    return net.losses(logits, localisations, gclasses, glocalisations, gscores, match_threshold=match_threshold,
                      negative_ratio=negative_ratio, alpha=alpha)


def ssd_losses(logits, localisations, gclasses, glocalisations, gscores, match_threshold=0.5, negative_ratio=3., alpha=1.,
               label_smoothing=0., scope=None):
    """Loss functions of the SSD-512 network (nets/ssd_vgg_512.py:516-607): hard negatives per feature layer.  The reference adds
    its terms to TF collections; here they are returned, as SSDNet.losses returns them."""
    return _ssd_losses_fn('layer', logits, localisations, gclasses, glocalisations, gscores, match_threshold, negative_ratio, alpha)


def ssd_arg_scope(weight_decay=0.0005, data_format='NHWC'):
    """Defines the VGG arg scope (nets/ssd_vgg_512.py:463-487)."""
    return ron_vgg_320._ArgScope(weight_decay, True, data_format)


def ssd_arg_scope_caffe(caffe_scope):
    """nets/ssd_vgg_512.py:490-513 takes the Caffe weight initialisers from `caffe_scope`; initialisers have no meaning for an
    inference graph whose weights are loaded: the scope is the plain one."""
    return ron_vgg_320._ArgScope()
