"""GPU: ron_detect_tfe (RONNet / SSDNet.detect_tfe) - forward + TF-evaluation post-processing in one enqueue.

Bit for bit (torch.equal on scores and boxes) against
  - ron_forward on the same context followed by ron_post_tfe on the raw heads,
  - the driver's unfused sequence (net -> bboxes_decode -> objectness gate -> detected_bboxes, eval_ron_network.py:209-236),
  - oracle/tfe_post.py on the heads of that sequence,
in the dense synthetic regime and in a background-biased one (most anchors take the select kernel's early exit), and the
context's workspace keeps working when ron_detect and ron_detect_tfe alternate with any batch size."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import tfe_post  # noqa: E402

BG_DENSE, BG_BIASED = 8.0, 10.0
_NETS = {}


@pytest.fixture(scope='module', autouse=True)
def _close_nets():
    yield
    for net in _NETS.values():
        net.close()
    _NETS.clear()


def _make(variant='reducedfc', dtype='bf16', num_classes=21, bg=BG_DENSE, max_batch=4):
    from ron_tensorflow_amd import weights as W
    from ron_tensorflow_amd.nets import nets_factory
    cls = nets_factory.get_network('ron_320_vgg')
    net = cls(cls.default_params._replace(num_classes=num_classes), variant=variant, dtype=dtype, max_batch=max_batch,
              fuse_pools=True)
    return net.load_weights(W.synthetic_weights(variant, num_classes=num_classes, seed=1, bg=bg))


def _net(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _NETS:
        _NETS[key] = _make(**kw)
    return _NETS[key]


def _images(n, seed=0):
    from ron_tensorflow_amd import weights as W
    return torch.from_numpy(W.synthetic_images(n, seed=seed)).cuda()


def _dense(d):
    """(dict_scores, dict_bboxes) -> dense [N, C-1, K] / [N, C-1, K, 4]."""
    s, b = d
    keys = sorted(s)
    return torch.stack([s[c] for c in keys], 1), torch.stack([b[c] for c in keys], 1)


def _same(a, b):
    """a, b: (dict_scores, dict_bboxes) or dense (scores, bboxes) tensors."""
    sa, ba = _dense(a) if isinstance(a[0], dict) else a
    sb, bb = _dense(b) if isinstance(b[0], dict) else b
    assert torch.equal(sa, sb), 'scores differ'
    assert torch.equal(ba, bb), 'boxes differ'


def _n_kept(d):
    return int((_dense(d)[0] > 0).sum())


def _forward_then_post(net, x, ssd=False, **kw):
    """ron_forward on the same context, then ron_post_tfe on the raw heads (logits, objectness logits, raw offsets)."""
    from ron_tensorflow_amd import ops, tfe
    cls, obj, loc = net.forward_heads(x)
    adev = ops.anchors_to_device(net.anchors(net.params.img_shape), net.device)
    if ssd:
        kw = dict(kw, clipping_bbox=None)                   # SSDNet.detected_bboxes ignores it
    s, b = tfe.post_tfe(cls, obj, loc, adev, num_classes=net.params.num_classes, min_size=None if ssd else 0.03,
                        cls_is_prob=False, obj_is_prob=False, loc_decoded=False, **kw)
    return s, b                                             # dense [N, C-1, K] / [N, C-1, K, 4]


def _driver(net, x, objectness_thres=0.03, **kw):
    """eval_ron_network.py:209-236 as the driver runs it."""
    predictions, logits, objness_pred, objness_logits, localisations, _ = net.net(x, is_training=False, end_points=())
    localisations = net.bboxes_decode(localisations, net.anchors(net.params.img_shape))
    gated = [(o > objectness_thres).to(torch.float32) * predictions[k] for k, o in enumerate(objness_pred)]
    return net.detected_bboxes(gated, localisations, **kw), gated, localisations


ARGS = dict(select_threshold=0.01, nms_threshold=0.4, clipping_bbox=[0., 0., 1., 1.], top_k=200, keep_top_k=100)


@pytest.mark.parametrize('variant,dtype', [('reducedfc', 'bf16'), ('full', 'bf16'), ('reducedfc', 'f16x3'), ('full', 'f16x3')])
@pytest.mark.parametrize('bg', [BG_DENSE, BG_BIASED], ids=['dense', 'biased'])
def test_equals_forward_then_post_tfe(variant, dtype, bg):
    net = _net(variant=variant, dtype=dtype, bg=bg)
    x = _images(2, seed=3)
    got = net.detect_tfe(x, **ARGS)
    ref = _forward_then_post(net, x, **ARGS)
    _same(got, ref)
    assert _n_kept(got) > 0


@pytest.mark.parametrize('nms_mode', ['min', 'union'])
@pytest.mark.parametrize('bg', [BG_DENSE, BG_BIASED], ids=['dense', 'biased'])
def test_equals_driver_sequence_and_oracle(bg, nms_mode):
    net = _net(bg=bg)
    x = _images(2, seed=5)
    args = dict(ARGS, nms_mode=nms_mode)
    (ds, db), gated, dec = _driver(net, x, **args)
    got = net.detect_tfe(x, **args)
    _same(got, (ds, db))
    rs, rb = tfe_post.detected_bboxes([g.cpu().numpy() for g in gated], [d.cpu().numpy() for d in dec], num_classes=21,
                                      min_size=0.03, **args)
    for c in range(1, 21):
        assert np.array_equal(got[0][c].cpu().numpy(), rs[c]), c
        assert np.array_equal(got[1][c].cpu().numpy(), rb[c]), c
    assert _n_kept(got) > 0
    if bg == BG_BIASED:
        # the regime the early exit is for: most anchors' best class logit trails the background's by more than -log(0.01)
        logits = net.forward_heads(x)[0]
        z = torch.cat([l.reshape(2, -1, 21) for l in logits], 1)
        gap = z[..., 1:].max(-1).values - z.max(-1).values
        assert float((gap < np.log(0.01) - 1e-2).float().mean()) > 0.5


def test_scores_at_the_threshold():
    """select_threshold set to a score that occurs (strictly greater fails) and to the float just below it (passes)."""
    net = _net(bg=BG_BIASED)
    x = _images(1, seed=7)
    (_, _), gated, _ = _driver(net, x, **ARGS)
    p = torch.cat([g.reshape(1, -1, 21)[..., 1:].reshape(-1) for g in gated]).cpu().numpy()
    p = p[p > 0]
    s = np.float32(p[np.argmin(np.abs(p - np.float32(0.01)))])      # the occurring score nearest the driver's threshold
    for thr in (s, np.nextafter(s, np.float32(0))):
        assert abs(float(thr) - float(s)) < 1e-6
        args = dict(ARGS, select_threshold=float(thr), top_k=512, keep_top_k=512)
        _same(net.detect_tfe(x, **args), _driver(net, x, **args)[0])


# select_threshold 0: every (anchor, class) pair with a non-zero gated score is listed (~21 k keys per list), the early exit is off
@pytest.mark.parametrize('top_k,keep_top_k,nms_mode,thr', [(400, 400, 'min', 0.005), (512, 512, 'union', 0.005), (512, 200, 'min', 0.0)])
def test_top_k_edges(top_k, keep_top_k, nms_mode, thr):
    net = _net()
    x = _images(3, seed=11)
    args = dict(ARGS, top_k=top_k, keep_top_k=keep_top_k, nms_mode=nms_mode, select_threshold=thr)
    got = net.detect_tfe(x, **args)
    _same(got, _driver(net, x, **args)[0])
    _same(got, _forward_then_post(net, x, **args))


@pytest.mark.parametrize('num_classes,bg', [(2, 3.0), (81, 6.0), (128, 6.0)])
def test_other_class_counts(num_classes, bg):
    net = _net(num_classes=num_classes, bg=bg, max_batch=2)
    x = _images(2, seed=13)
    args = dict(ARGS, top_k=400, keep_top_k=200)
    got = net.detect_tfe(x, **args)
    assert len(got[0]) == num_classes - 1
    _same(got, _driver(net, x, **args)[0])
    _same(got, _forward_then_post(net, x, **args))
    assert _n_kept(got) > 0


def test_ssd512_no_gate_no_size_filter():
    from ron_tensorflow_amd import weights as W
    from ron_tensorflow_amd.nets import nets_factory
    cls = nets_factory.get_network('ssd_512_vgg')
    net = cls(cls.default_params._replace(num_classes=21), dtype='bf16', max_batch=2).load_weights(W.ssd_synthetic_weights(seed=5))
    try:
        x = torch.from_numpy(W.synthetic_images(1, seed=4, img_shape=(512, 512))).cuda()
        args = dict(ARGS, top_k=400, keep_top_k=200)
        got = net.detect_tfe(x, **args)
        _same(got, _forward_then_post(net, x, ssd=True, **args))
        predictions, localisations, _, _ = net.net(x, is_training=False, end_points=())
        dec = net.bboxes_decode(localisations, net.anchors(net.params.img_shape))
        _same(got, net.detected_bboxes(predictions, dec, **args))
        assert _n_kept(got) > 0
    finally:
        net.close()


def _np_same(a, b):
    for k in ('count', 'classes', 'scores', 'bboxes', 'anchor_index'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_alternating_with_detect_on_one_context():
    """n = 3, max_batch, 1 with ron_detect calls in between (and both orders of the switch): every result equals a fresh
    context's.  ron_detect's keys land on the TF counters and the TF keys run past the np counters: a workspace that did not
    keep them apart shows up here as lists or counts of the wrong length."""
    mb = 4
    net = _make(max_batch=mb)
    xs = {n: _images(n, seed=20 + n) for n in (1, 3, mb)}
    seq = [('tfe', 3), ('np', mb), ('tfe', mb), ('tfe', 1), ('np', 1), ('np', 3), ('tfe', 3), ('np', mb), ('tfe', 1)]
    got = [net.detect_tfe(xs[n], **ARGS) if kind == 'tfe' else net.detect(xs[n]) for kind, n in seq]
    torch.cuda.synchronize()
    net.close()
    refs = {}
    for kind, n in set(seq):
        fresh = _make(max_batch=mb)
        refs[kind, n] = fresh.detect_tfe(xs[n], **ARGS) if kind == 'tfe' else fresh.detect(xs[n])
        torch.cuda.synchronize()
        fresh.close()
    for (kind, n), g in zip(seq, got):
        ref = refs[kind, n]
        if kind == 'tfe':
            _same(g, ref)
            assert _n_kept(g) > 0
        else:
            _np_same(g, ref)


def test_rejected_cfg_leaves_context_usable():
    from ron_tensorflow_amd._lib import RonError
    net = _net()
    x = _images(2, seed=31)
    ref = net.detect_tfe(x, **ARGS)
    for bad in (dict(ARGS, keep_top_k=300, top_k=200), dict(ARGS, top_k=1000), dict(ARGS, select_threshold=-0.5),
                dict(ARGS, keep_top_k=0)):
        with pytest.raises(RonError):
            net.detect_tfe(x, **bad)
    with pytest.raises(RonError):
        net.detect_tfe(_images(5, seed=1), **ARGS)               # n > max_batch
    _same(net.detect_tfe(x, **ARGS), ref)


def test_clone_gives_source_results():
    net = _net()
    x = _images(3, seed=41)
    ref = net.detect_tfe(x, **ARGS)
    slot = net.clone()
    _same(slot.detect_tfe(x, **ARGS), ref)
    torch.cuda.synchronize()
    slot.close()
    net._slots = []


def test_profile_counts_post_stage():
    import ctypes as C
    from ron_tensorflow_amd import _lib
    net = _net()
    x = _images(1, seed=43)
    net.detect_tfe(x, **ARGS)
    L, ctx = _lib.lib(), net._context()
    _lib.check(L.ron_profile_reset(ctx))
    _lib.check(L.ron_profile_enable(ctx, 2))
    net.detect_tfe(x, **ARGS)
    net.detect_tfe(x, **ARGS)
    _lib.check(L.ron_profile_enable(ctx, 0))
    last = L.ron_profile_num_ops(ctx) - 1
    ms, launches = C.c_double(), C.c_int()
    _lib.check(L.ron_profile_get(ctx, last, None, None, None, C.byref(ms), C.byref(launches), None, None))
    assert launches.value == 2 and ms.value > 0
    _lib.check(L.ron_profile_reset(ctx))


def test_pipeline_tfe_equals_sequential():
    from ron_tensorflow_amd import pipeline, tfe
    net = _make(max_batch=4)
    sizes = [1, 3, 4, 2, 4, 1]
    xs = [_images(n, seed=50 + i) for i, n in enumerate(sizes)]
    ref = [net.detect_tfe(x, **ARGS) for x in xs]
    torch.cuda.synchronize()
    p = pipeline.DetectPipeline(net, slots=2, buffers_per_slot=3, post='tfe', top_k=ARGS['top_k'], keep_top_k=ARGS['keep_top_k'])
    args = {k: v for k, v in ARGS.items() if k not in ('top_k', 'keep_top_k')}
    tickets = [p.submit(x, **args) for x in xs]
    for t, r, n in zip(tickets, ref, sizes):
        d = t.wait()
        assert isinstance(d, tfe.TfeBuffers) and d.n == n
        _same(d.as_dicts(), r)
    p.close()
    net.close()


def test_eval_driver_fused_detect_matches_default():
    from ron_tensorflow_amd import eval_ron_network
    argv = ['--batch_size', '2', '--max_num_batches', '2']
    a = eval_ron_network.main(argv)
    b = eval_ron_network.main(argv + ['--fused_detect', '1'])
    assert a['AP_VOC07/mAP'] == b['AP_VOC07/mAP'] and a['AP_VOC12/mAP'] == b['AP_VOC12/mAP']
    assert len(a['detections']) == len(b['detections']) == 2
    kept = 0
    for da, db in zip(a['detections'], b['detections']):
        assert sorted(da) == sorted(db)
        for c in da:
            assert np.array_equal(da[c][0], db[c][0]) and np.array_equal(da[c][1], db[c][1])
            kept += int((da[c][0] > 0).sum())
    assert kept > 0
