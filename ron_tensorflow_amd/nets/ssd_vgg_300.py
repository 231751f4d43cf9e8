"""SSD-300 (VGG) network object with the interface of the reference's ``nets/ssd_vgg_300.py``.

``SSDNet`` keeps names / defaults / return arity of the reference class (nets/ssd_vgg_300.py:82-245): ``net`` returns
``(predictions, localisations, logits, end_points)``.  It is ``ssd_vgg_512.SSDNet`` with other parameters and the context
variant RON_VARIANT_SSD300: ``update_feature_shapes``, ``anchors``, ``bboxes_decode``, ``detected_bboxes``, ``detect``,
``detect_tfe``, ``bboxes_encode``, ``losses``, ``losses_and_gradients``, ``validation_losses``, ``load_weights``,
``load_checkpoint`` and ``clone`` are inherited.  The maps are 300 -> 150 -> 75 -> 38 -> 19 (SAME 2x2 pools: ceil) -> 10 -> 5
(pad 1 + 3x3 stride 2) -> 3 -> 1 (3x3 VALID): 8732 anchors."""
from . import ron_vgg_320, ssd_vgg_512
from .ssd_vgg_512 import SSDParams

_FEAT_LAYERS = ('block4', 'block7', 'block8', 'block9', 'block10', 'block11')


class SSDNet(ssd_vgg_512.SSDNet):
    """SSD VGG-based 300 network: conv4 38x38, conv7 19x19, conv8 10x10, conv9 5x5, conv10 3x3, conv11 1x1."""
    default_params = SSDParams(
        img_shape=(300, 300),
        num_classes=21,
        no_annotation_label=21,
        feat_layers=['block4', 'block7', 'block8', 'block9', 'block10', 'block11'],
        feat_shapes=[(38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1)],
        anchor_size_bounds=[0.15, 0.90],
        anchor_sizes=[(21., 45.), (45., 99.), (99., 153.), (153., 207.), (207., 261.), (261., 315.)],
        anchor_ratios=[[2, .5], [2, .5, 3, 1. / 3], [2, .5, 3, 1. / 3], [2, .5, 3, 1. / 3], [2, .5], [2, .5]],
        anchor_steps=[8, 16, 32, 64, 100, 300],
        anchor_offset=0.5,
        normalizations=[20, -1, -1, -1, -1, -1],
        prior_scaling=[0.1, 0.1, 0.2, 0.2])
    _variant = 'ssd300'
    _mining = 'batch'          # nets/ssd_vgg_300.py:580-659: one hard-negative selection over the whole batch

    def __init__(self, params=None, dtype='bf16', max_batch=32, device=None, fuse_pools=False):
        ssd_vgg_512.SSDNet.__init__(self, params, dtype=dtype, max_batch=max_batch, device=device, fuse_pools=fuse_pools)

    def net(self, inputs, is_training=True, update_feat_shapes=True, dropout_keep_prob=0.5, prediction_fn=None, reuse=None,
            scope='ssd_300_vgg', end_points=_FEAT_LAYERS):
        """nets/ssd_vgg_300.py:136-160 -> (predictions, localisations, logits, end_points)."""
        return ssd_vgg_512.SSDNet.net(self, inputs, is_training=is_training, update_feat_shapes=update_feat_shapes,
                                      dropout_keep_prob=dropout_keep_prob, prediction_fn=prediction_fn, reuse=reuse, scope=scope,
                                      end_points=end_points)


# ---------------------------------------------------------------------- the reference's function entries (nets_factory.networks_map)
def ssd_net(inputs, num_classes=SSDNet.default_params.num_classes, feat_layers=SSDNet.default_params.feat_layers,
            anchor_sizes=SSDNet.default_params.anchor_sizes, anchor_ratios=SSDNet.default_params.anchor_ratios,
            normalizations=SSDNet.default_params.normalizations, is_training=True, dropout_keep_prob=0.5, prediction_fn=None,
            reuse=None, scope='ssd_300_vgg', weights=None, dtype='bf16', max_batch=32):
    """SSD net definition (nets/ssd_vgg_300.py:434-523): (predictions, localisations, logits, end_points).  A scope name owns one
    network object, like ron_vgg_320.ron_net: the first call needs `weights=`."""
    return ssd_vgg_512._ssd_net_fn(SSDNet, inputs, num_classes, feat_layers, anchor_sizes, anchor_ratios, normalizations, is_training,
                                   dropout_keep_prob, prediction_fn, reuse, scope, weights, dtype, max_batch)


ssd_net.default_image_size = 300


def ssd_losses(logits, localisations, gclasses, glocalisations, gscores, match_threshold=0.5, negative_ratio=3., alpha=1.,
               label_smoothing=0., device='/cpu:0', scope=None):
    """Loss functions of the SSD-300 network (nets/ssd_vgg_300.py:580-659): one hard-negative selection over the whole batch.
    `device` is accepted and unused; the terms are returned, as SSDNet.losses returns them."""
    return ssd_vgg_512._ssd_losses_fn('batch', logits, localisations, gclasses, glocalisations, gscores, match_threshold,
                                      negative_ratio, alpha)


def ssd_arg_scope(weight_decay=0.0005, data_format='NHWC'):
    """Defines the VGG arg scope (nets/ssd_vgg_300.py:527-550)."""
    return ron_vgg_320._ArgScope(weight_decay, True, data_format)


def ssd_arg_scope_caffe(caffe_scope):
    """nets/ssd_vgg_300.py:556-580 takes the Caffe weight initialisers from `caffe_scope`; the weights of an inference graph are
    loaded, so the scope is the plain one (as for SSD-512)."""
    return ron_vgg_320._ArgScope()
