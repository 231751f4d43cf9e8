"""GPU parity: SSD-300 (ssd_300_vgg, ron_ctx variant 3) through the C ABI - the backbone against the reference's own torch VGG16 on a
300^2 image (golden G9: the odd pool3 75 -> 38 included, stand-alone and fused), the whole conv stack against tests/ssd300_ref.py,
the detections against the numpy oracles, the reference's np_methods pipeline on the 8732 anchors (G9)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import ssd300_cases  # noqa: E402
import ssd300_ref  # noqa: E402
from g9_util import G9, check_tensor  # noqa: E402
from oracle import np_post, synth, tfe_post  # noqa: E402
from oracle import ron_forward as orf  # noqa: E402

FEAT = [[38, 38, 4], [19, 19, 6], [10, 10, 6], [5, 5, 6], [3, 3, 4], [1, 1, 4]]
LAYERS = ['block4', 'block7', 'block8', 'block9', 'block10', 'block11']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def setup():
    import ron_tensorflow_amd.weights as W
    from ron_tensorflow_amd.nets import nets_factory
    weights = W.ssd300_synthetic_weights(seed=6)
    images = W.synthetic_images(1, seed=4, img_shape=(300, 300))
    col = {}
    ref = ssd300_ref.ssd300_forward(images, weights, collect=col)
    return dict(W=W, factory=nets_factory, weights=weights, images=images, ref=ref, col=col)


def _rel(got, ref):
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-12))


def _net(setup, dtype, max_batch=1, fuse_pools=False, weights=None):
    cls = setup['factory'].get_network('ssd_300_vgg')
    net = cls(cls.default_params._replace(num_classes=21), dtype=dtype, max_batch=max_batch, fuse_pools=fuse_pools)
    return net.load_weights(setup['weights'] if weights is None else weights)


@pytest.mark.parametrize('fuse_pools', [False, True], ids=['pools', 'fused'])
@pytest.mark.parametrize('dtype', ['fp32', 'f16x3'])
def test_backbone_reproduces_the_reference_vgg(setup, dev, dtype, fuse_pools):
    """conv1_1 .. conv7 on G9's weights and 300^2 image; fuse_pools runs conv3_3 + pool3 (75 -> 38) as one launch.  Every stored tap
    within 1e-4 of the tensor's largest value, whole-tensor sums within 1e-5 (tests/test_gpu_g8.py's tolerances)."""
    weights = dict(setup['weights'])
    for k, v in synth.vgg_backbone_weights_tf(int(G9['seed_weights']), ssd300_ref.SCOPE).items():
        assert weights[k].shape == v.shape, k
        weights[k] = v
    net = _net(setup, dtype, fuse_pools=fuse_pools, weights=weights)
    plan = net.launch_plan()
    assert ('conv3_3+pool3' in plan) == fuse_pools and 'conv1_1+conv1_2+pool1' not in plan, plan[:10]
    x = torch.from_numpy(synth.vgg_backbone_image(int(G9['seed_image_300']), 300)).to(dev)
    net.forward_heads(x)
    names = [n for n in synth.VGG_TAPS if not (fuse_pools and n in ('conv1_2', 'conv2_2', 'conv3_3'))]
    errs = {n: check_tensor(n, net.end_point(n, 1).cpu().numpy(), tol=1e-4, sum_tol=1e-5) for n in names}
    assert torch.equal(net.end_point('block7', 1), net.end_point('conv7', 1)) and torch.equal(net.end_point('block6', 1), net.end_point('conv6', 1))
    net.close()
    worst = max(errs, key=lambda n: errs[n][0])
    print('SSD-300 %s %s device path vs G9: worst sample %.2e (%s), worst sums %.2e / %.2e; pool3 %.2e %.2e %.2e' % (
        dtype, 'fused' if fuse_pools else 'pools', errs[worst][0], worst, max(e[1] for e in errs.values()),
        max(e[2] for e in errs.values()), errs['pool3'][0], errs['pool3'][1], errs['pool3'][2]))


def test_fp32_forward_and_detect(setup, dev):
    net = _net(setup, 'fp32')
    assert net.variables() == [(n, tuple(s)) for n, s in setup['W'].ssd300_variable_shapes()]
    assert net.flops_per_image() == 2.0 * ssd300_ref.macs_per_image(setup['W'].ssd300_variable_shapes())
    x = torch.from_numpy(setup['images']).to(dev)
    net.params = net.params._replace(feat_shapes=[(1, 1)] * 6)
    pred, loc, logits, eps = net.net(x, is_training=False, update_feat_shapes=False)
    assert net.params.feat_shapes == [(1, 1)] * 6
    pred, loc, logits, eps = net.net(x, is_training=False)
    assert net.params.feat_shapes == FEAT
    r_pred, r_loc, r_logits, r_eps = setup['ref']
    assert len(pred) == 6 and sorted(eps) == sorted(LAYERS)
    for i in range(6):
        assert tuple(logits[i].shape) == r_logits[i].shape == (1,) + tuple(FEAT[i]) + (21,)
        el, eo = _rel(logits[i].cpu().numpy(), r_logits[i]), _rel(loc[i].cpu().numpy(), r_loc[i])
        print('fp32 layer %d: logits %.2e loc %.2e' % (i, el, eo))
        assert el < 1e-4 and eo < 1e-4, i
        np.testing.assert_allclose(pred[i].cpu().numpy(), r_pred[i], rtol=0, atol=1e-4)
    for name in ('block4', 'block7', 'block8', 'block11'):
        assert _rel(eps[name].cpu().numpy(), r_eps[name]) < 1e-4, name
    assert _rel(net.end_point('block4_norm', 1).cpu().numpy(), setup['col']['block4_norm']) < 1e-4
    anchors = ssd300_ref.anchors_all_layers()
    for a, b in zip(net.anchors((300, 300)), anchors):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    # fused detect == the numpy oracle on the heads this context produced
    det = net.detect(x).to_lists()[0]
    want = np_post.detect_from_predictions([p.cpu().numpy() for p in pred], [l.cpu().numpy() for l in loc], anchors,
                                           objness_pred=None, prior_scaling=net.params.prior_scaling)[0]
    assert want['n_candidates'] > 400
    assert np.array_equal(det['classes'], want['classes'])
    assert np.array_equal(det['anchor_index'], want['anchor_index'])
    assert np.array_equal(det['scores'], want['scores'])
    np.testing.assert_allclose(det['bboxes'], want['bboxes'], rtol=0, atol=1e-5)
    # decode, then detected_bboxes (no clip, no size filter), and the same in one enqueue: == oracle/tfe_post.py bit for bit
    dec = net.bboxes_decode(loc, net.anchors((300, 300)))
    args = dict(select_threshold=0.01, nms_threshold=0.45, clipping_bbox=None, top_k=400, keep_top_k=200)
    ds, db = net.detected_bboxes(pred, dec, **args)
    ts, tb = net.detect_tfe(x, **args)
    rs, rb = tfe_post.detected_bboxes([p.cpu().numpy() for p in pred], [d.cpu().numpy() for d in dec], num_classes=21,
                                      nms_mode='min', min_size=None, **args)
    for c in range(1, 21):
        assert np.array_equal(ds[c].cpu().numpy(), rs[c]) and np.array_equal(db[c].cpu().numpy(), rb[c]), c
        assert np.array_equal(ts[c].cpu().numpy(), rs[c]) and np.array_equal(tb[c].cpu().numpy(), rb[c]), c
    assert sum(int((rs[c] > 0).sum()) for c in range(1, 21)) > 0
    assert net.grouped_launches() == 4 and sum(n.startswith('group[') for n in net.launch_plan()) == 4
    assert 'block4_box_conv_cls_loc' in net.launch_plan() and 'block7_box_conv_cls_loc' in net.launch_plan()
    net.close()


def test_bf16_forward(setup, dev):
    """bf16 against the reference with bf16-rounded operands: SSD-512's bounds (tests/test_gpu_ssd.py:88-89: 0.05 logits, 0.08 loc; the
    same layer types and K lengths)."""
    ref = ssd300_ref.ssd300_forward(setup['images'], setup['weights'], round_fn=orf.round_bf16)
    for fuse in (True, False):
        net = _net(setup, 'bf16', fuse_pools=fuse)
        logits, _, loc = net.forward_heads(torch.from_numpy(setup['images']).to(dev))
        errs = [(_rel(logits[i].cpu().numpy(), ref[2][i]), _rel(loc[i].cpu().numpy(), ref[1][i])) for i in range(6)]
        print('bf16 fuse_pools=%s: logits %s loc %s' % (fuse, ['%.4f' % e[0] for e in errs], ['%.4f' % e[1] for e in errs]))
        for i, (el, eo) in enumerate(errs):
            assert el < 0.05 and eo < 0.08, (i, el, eo)
        net.close()


def test_split_precision_forward_and_detect(setup, dev):
    from ron_tensorflow_amd.metrics import detection_agreement
    net = _net(setup, 'f16x3', fuse_pools=True)
    x = torch.from_numpy(setup['images']).to(dev)
    logits, _, loc = net.forward_heads(x)
    r_pred, r_loc, r_logits, _ = setup['ref']
    for i in range(6):
        el, eo = _rel(logits[i].cpu().numpy(), r_logits[i]), _rel(loc[i].cpu().numpy(), r_loc[i])
        print('f16x3 layer %d: logits %.2e loc %.2e' % (i, el, eo))
        assert el < 2e-5 and eo < 2e-5, i
    assert _rel(net.end_point('block4_norm', 1).cpu().numpy(), setup['col']['block4_norm']) < 2e-5
    det = net.detect(x).to_lists()[0]
    want = np_post.detect_from_predictions(r_pred, r_loc, ssd300_ref.anchors_all_layers(), objness_pred=None,
                                           prior_scaling=net.params.prior_scaling)[0]
    a = detection_agreement(det, want, tol=1e-4)
    print('f16x3 detect vs oracle pipeline on the oracle heads:', a)
    assert a['reproduced'] >= 0.98 and a['within_tol'] == 1.0, a
    net.close()


def test_post_np_golden_pipeline_ssd300(dev):
    """ron_post_np on the 8732 SSD-300 anchors against what the reference's np_methods produced (G9), graded as G5 is."""
    from ron_tensorflow_amd import ops
    adev = ops.anchors_to_device(ssd300_ref.anchors_all_layers(), dev)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g9_pipeline_ssd300.npz'))
    to_dev = lambda ts: [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in ts]       # noqa: E731
    for name, seed, bg, scale, thr, nms in ssd300_cases.G9_CASES:
        cls, loc = ssd300_cases.head_tensors(seed, bg, scale)
        pred = [np_post.softmax_last(c) for c in cls]          # the probabilities the reference was fed (tests/test_gpu_post.py)
        out, srt, ncand = ops.post_np(to_dev(pred), None, to_dev(loc), adev, select_threshold=float(thr), nms_threshold=float(nms),
                                      cls_is_prob=True, want_sorted=True)
        assert int(ncand.cpu().numpy()[0]) == int(g[name + '/n_cand']), name
        assert int(srt.count.cpu().numpy()[0]) == int(g[name + '/n_sorted']), name
        got = out.to_lists()[0]
        assert np.array_equal(got['classes'], g[name + '/classes']), name
        assert np.array_equal(got['scores'], g[name + '/scores']), name
        np.testing.assert_allclose(got['bboxes'], g[name + '/bboxes'], rtol=0, atol=1e-5, err_msg=name)          # BOX_TOL of tests/test_gpu_post.py
        s = srt.to_lists()[0]
        assert np.array_equal(s['classes'], g[name + '/sorted_classes']) and np.array_equal(s['scores'], g[name + '/sorted_scores']), name


def test_two_slot_pipeline_equals_the_single_context(setup, dev):
    from ron_tensorflow_amd.pipeline import DetectPipeline
    net = _net(setup, 'bf16', max_batch=2, fuse_pools=True)
    fields = ('count', 'classes', 'scores', 'bboxes', 'anchor_index')
    batches = [torch.from_numpy(setup['W'].synthetic_images(2, seed=30 + i, img_shape=(300, 300))).to(dev) for i in range(4)]
    refs = []
    for b in batches:
        d = net.detect(b)
        refs.append({k: getattr(d, k).clone() for k in fields})
    torch.cuda.synchronize()
    assert int(refs[0]['count'].min()) > 0 and any(not torch.equal(refs[0]['scores'], r['scores']) for r in refs[1:])
    pipe = DetectPipeline(net, slots=2)
    tickets = [pipe.submit(b) for b in batches[:2]]
    for j in range(4):
        d = tickets.pop(0).wait()
        for k in fields:
            assert torch.equal(getattr(d, k), refs[j][k]), (j, k)
        if j + 2 < 4:
            tickets.append(pipe.submit(batches[j + 2]))
    pipe.close()
    net.close()


def test_network_fn(setup, dev):
    fn = setup['factory'].get_network_fn('ssd_300_vgg', 21, is_training=False, weights=setup['weights'], dtype='bf16', max_batch=1)
    assert fn.default_image_size == 300
    out = fn(torch.from_numpy(setup['images']).to(dev), end_points=())
    assert len(out) == 4 and len(out[0]) == 6
    assert tuple(out[0][0].shape) == (1, 38, 38, 4, 21) and tuple(out[1][5].shape) == (1, 1, 1, 4, 4)
    fn.network.close()
