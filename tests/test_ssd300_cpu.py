"""CPU: SSD-300 (ssd_300_vgg) - golden G9 against the host functions, the CPU reference (tests/ssd300_ref.py) and the numpy oracle;
the library's dry run of the variant-3 graph (variables, heads, FLOPs, launch plan).  The GPU side is tests/test_gpu_ssd300.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_post, synth

import ssd300_cases
import ssd300_ref
from g9_util import G9, check_tensor

HERE = os.path.dirname(os.path.abspath(__file__))
FEAT = [[38, 38, 4], [19, 19, 6], [10, 10, 6], [5, 5, 6], [3, 3, 4], [1, 1, 4]]


def _g(name):
    return np.load(os.path.join(HERE, 'golden', name))


def test_factory_knows_the_network():
    from ron_tensorflow_amd import _lib
    from ron_tensorflow_amd.nets import nets_factory, ssd_vgg_300, ssd_vgg_512
    assert _lib.VARIANTS['ssd300'] == 3
    for name in ('ssd_300_vgg', 'ssd_300_vgg_caffe'):
        assert nets_factory.networks_map[name] is ssd_vgg_300.ssd_net and name in nets_factory.arg_scopes_map
    assert nets_factory.networks_map['ssd_300_vgg'].default_image_size == 300
    cls = nets_factory.get_network('ssd_300_vgg')
    assert cls is ssd_vgg_300.SSDNet and issubclass(cls, ssd_vgg_512.SSDNet)
    p = cls.default_params                                        # nets/ssd_vgg_300.py:94-124, field by field
    assert p.img_shape == (300, 300) and p.num_classes == 21 and p.no_annotation_label == 21
    assert p.feat_layers == ssd300_ref.FEAT_LAYERS and p.feat_shapes == ssd300_ref.SSD300['feat_shapes']
    assert p.anchor_size_bounds == [0.15, 0.90] and p.anchor_sizes == ssd300_ref.SSD300['anchor_sizes']
    assert p.anchor_ratios == ssd300_ref.SSD300['anchor_ratios'] and p.anchor_steps == [8, 16, 32, 64, 100, 300]
    assert p.anchor_offset == 0.5 and p.normalizations == [20, -1, -1, -1, -1, -1] and p.prior_scaling == [0.1, 0.1, 0.2, 0.2]
    # the existing entries are what they were
    assert nets_factory.networks_map['ssd_512_vgg'] is ssd_vgg_512.ssd_net and nets_factory.get_network('ssd_512_vgg') is ssd_vgg_512.SSDNet
    assert ssd_vgg_512.SSDNet.default_params.img_shape == (512, 512) and ssd_vgg_512.ssd_net.default_image_size == 512


def test_anchors_equal_the_reference():
    """SSDNet.anchors((300, 300)) through the host C function, and the CPU reference's, == the reference's own (G9)."""
    from ron_tensorflow_amd.nets import nets_factory
    g = _g('g9_anchors_ssd300.npz')
    net = nets_factory.get_network('ssd_300_vgg')(device='cpu')
    for layers in (net.anchors((300, 300)), ssd300_ref.anchors_all_layers()):
        assert [tuple(l[0].shape) for l in layers] == [(h, w, 1) for h, w, _ in FEAT]
        assert sum(l[0].shape[0] * l[0].shape[1] * len(l[2]) for l in layers) == 8732
        for i, (y, x, h, w) in enumerate(layers):
            for nm, arr in (('y', y), ('x', x), ('h', h), ('w', w)):
                assert arr.dtype == np.float32 and np.array_equal(arr, g['%s%d' % (nm, i)]), (nm, i)
    assert abs(float(g['y0'][0, 0, 0]) - 0.0133333) < 1e-7
    np.testing.assert_allclose(g['h0'][:3], [0.07, 0.10246951, 0.04949747], rtol=0, atol=1e-8)


@pytest.mark.parametrize('backend', ['numpy', 'torch'])
def test_reference_backbone_reproduces_the_reference_vgg(backend):
    """tests/ssd300_ref.py conv1_1 .. conv7 on a 300^2 image - the odd pool3 (75 -> 38) included - == the reference's torch VGG16
    (G9), with the tolerances tests/test_oracle_g8.py applies to G8."""
    weights = synth.vgg_backbone_weights_tf(int(G9['seed_weights']), ssd300_ref.SCOPE)
    img = synth.vgg_backbone_image(int(G9['seed_image_300']), 300)
    collect = {}
    ssd300_ref.ssd300_forward(img, weights, collect=collect, backend=backend, stop_after='block7')
    assert sorted(collect) == sorted(synth.VGG_TAPS)
    assert collect['pool3'].shape == (1, 38, 38, 256) and collect['conv7'].shape == (1, 19, 19, 1024)
    worst = max(check_tensor(name, collect[name])[0] for name in synth.VGG_TAPS)
    print('ssd300 reference (%s) vs G9: worst %.2e' % (backend, worst))


def test_g9_check_catches_a_wrong_edge_row():
    """The last row of pool3 comes from one-row windows: computed as a VALID pool padded with zeros it differs only there."""
    weights = synth.vgg_backbone_weights_tf(int(G9['seed_weights']), ssd300_ref.SCOPE)
    img = synth.vgg_backbone_image(int(G9['seed_image_300']), 300)
    collect = {}
    ssd300_ref.ssd300_forward(img, weights, collect=collect, backend='torch', stop_after='block7')
    bad = collect['pool3'].copy()
    bad[0, 37, 5, :] = bad[0, 36, 5, :]            # (column 5 is not sampled)
    with pytest.raises(AssertionError):
        check_tensor('pool3', bad)


@pytest.mark.parametrize('shape', [(2, 75, 75, 8), (2, 3, 5, 4), (1, 7, 2, 4), (3, 1, 1, 2), (2, 8, 6, 4)])
def test_ceil_pool_backends_agree(shape):
    x = np.random.RandomState(sum(shape)).randn(*shape).astype(np.float32)         # negative values too: padding must never win
    a, b = ssd300_ref.max_pool2x2_same_np(x), ssd300_ref.max_pool2x2_same_torch(x)
    assert a.shape == (shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2, shape[3]) and a.dtype == np.float32
    assert np.array_equal(a, b)
    assert np.array_equal(a[:, -1, -1], x[:, 2 * (a.shape[1] - 1):, 2 * (a.shape[2] - 1):].max(axis=(1, 2)))


def test_numpy_oracle_reproduces_the_reference_pipeline():
    """oracle/np_post.py on the 8732 SSD-300 anchors == the reference's np_methods (G9), graded as G5 is."""
    g = _g('g9_pipeline_ssd300.npz')
    layers = ssd300_ref.anchors_all_layers()
    assert [str(n) for n in g['names']] == [c[0] for c in ssd300_cases.G9_CASES]
    for name, seed, bg, scale, thr, nms in ssd300_cases.G9_CASES:
        assert list(g[name + '/params']) == [seed, bg, scale, thr, nms]
        cls, loc = ssd300_cases.head_tensors(seed, bg, scale)
        pred = [np_post.softmax_last(c) for c in cls]
        res = np_post.detect_from_predictions(pred, loc, layers, objness_pred=None, select_threshold=thr, top_k=400,
                                              nms_threshold=nms)[0]
        assert res['n_candidates'] == int(g[name + '/n_cand']), name
        assert res['n_sorted'] == int(g[name + '/n_sorted']), name
        assert np.array_equal(res['classes'], g[name + '/classes']), name
        assert np.array_equal(res['scores'], g[name + '/scores']), name
        assert np.array_equal(res['bboxes'].reshape(-1, 4), g[name + '/bboxes']), name
        if res['anchor_index'].size:
            assert res['anchor_index'].min() >= 0 and res['anchor_index'].max() < 8732
    assert [int(g[c[0] + '/n_cand']) for c in ssd300_cases.G9_CASES] == [1264, 22934, 90791, 2915, 0]


CRC_512 = {'conv1_1': 1547877605, 'block12_cls_b': 2069885908}


def test_existing_weight_functions_are_unchanged_and_the_new_ones_fit():
    import zlib
    import ron_tensorflow_amd.weights as W
    shp = W.ssd_variable_shapes()
    assert len(shp) == 79 and shp[34] == ('ssd_512_vgg/block9/conv1x1/weights', (1, 1, 512, 128))
    assert shp[50] == ('ssd_512_vgg/block4_box/L2Normalization/gamma', (512,))
    assert ('ssd_512_vgg/block12/conv4x4/weights', (4, 4, 128, 256)) in shp
    w = W.ssd_synthetic_weights(seed=5)
    # recorded from the functions as they were before they shared code with the SSD-300 ones
    assert zlib.crc32(w['ssd_512_vgg/conv1/conv1_1/weights'].tobytes()) == CRC_512['conv1_1']
    assert zlib.crc32(w['ssd_512_vgg/block12_box/conv_cls/biases'].tobytes()) == CRC_512['block12_cls_b']
    s3 = W.ssd300_variable_shapes()
    assert len(s3) == 2 * (13 + 2 + 8 + 12) + 1 == 71 and all(n.startswith('ssd_300_vgg/') for n, _ in s3)
    assert ('ssd_300_vgg/block10/conv3x3/weights', (3, 3, 128, 256)) in s3 and ('ssd_300_vgg/block11_box/conv_cls/biases', (84,)) in s3
    assert 2 * ssd300_ref.macs_per_image(s3) == 62747075584          # 31.37 GMAC: "about 31 GMAC", the commonly quoted size



def test_synthetic_network_yields_more_than_400_candidates():
    """ssd300_synthetic_weights' background bias: the CPU reference's predictions pass select 0.01 more than 400 times (what the GPU
    post-processing test relies on), and not for nearly every score either."""
    import ron_tensorflow_amd.weights as W
    weights = W.ssd300_synthetic_weights(seed=6)
    images = W.synthetic_images(1, seed=4, img_shape=(300, 300))
    pred, loc, logits, _ = ssd300_ref.ssd300_forward(images, weights, backend='torch')
    n = sum(int((p[..., 1:] > 0.01).sum()) for p in pred)
    print('candidates at select 0.01: %d of %d scores; logit std per layer %s' % (n, 8732 * 20, ['%.2f' % l[..., 1:].std() for l in logits]))
    assert 400 < n < 8732 * 20 // 2


def test_dry_run_plans_the_variant():
    """RON_PLAN_ONLY=1: variant 3 for fp32 / bf16 / fp16 / f16x3, with and without fused pools, max_batch 1 / 16 / 32."""
    import ron_tensorflow_amd.weights as W
    env = dict(os.environ, RON_PLAN_ONLY='1')
    r = subprocess.run([sys.executable, os.path.join(HERE, 'ssd300_plan_child.py')], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    runs = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert len(runs) == 24
    want_vars = [[n, list(s)] for n, s in W.ssd300_variable_shapes()]
    want_flops = 2.0 * ssd300_ref.macs_per_image(W.ssd300_variable_shapes())
    for run in runs:
        key = (run['dtype'], run['flags'], run['max_batch'])
        assert run['variables'] == want_vars, key
        assert run['heads'] == FEAT, key
        assert run['flops'] == want_flops, (key, run['flops'], want_flops)
        assert run['grouped'] == 4, key
        plan = run['plan']
        # block4 / block7 heads: two-output launches; the small blocks' heads grouped with the next block's 1x1
        assert 'block4_box_conv_cls_loc' in plan and 'block7_box_conv_cls_loc' in plan, key
        for b in (8, 9, 10):
            i = plan.index('group[block%d_box_conv_loc+2]' % b)
            assert plan[i + 1:i + 3] == ['(block%d_box_conv_cls)' % b, '(block%d_conv1x1)' % (b + 1)], key
        i = plan.index('group[block11_box_conv_loc+1]')
        assert plan[i + 1] == '(block11_box_conv_cls)', key
        assert ('conv3_3+pool3' in plan) == bool(run['flags']), key
        # no fused stem on 300 x 300 (its 8 x 32 tile does not divide the map): the stem kernel + conv1_2 (+pool1)
        assert 'conv1_1+conv1_2+pool1' not in plan and 'conv1_1' in plan, key
