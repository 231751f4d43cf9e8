"""GPU: RONNet.losses / RONNet.validation_losses against the float64 reference (tests/encode_ref.py).

The six counts are equal to the reference's; the three terms and their sum lie within the bound derived in DESIGN.md section 4
(encode_ref.losses_bound: per-row error of the float32 cross-entropy and smooth-L1, accumulation, the mean's three roundings); NaN
where the reference is NaN; two calls on the same inputs give the same bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_cases as ec  # noqa: E402
import encode_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_CASES = ec.loss_cases()
KEYS = ('cross_entropy_pos', 'cross_entropy_objectness', 'localization', 'total')


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _net(dev, **params):
    from ron_tensorflow_amd.nets.ron_vgg_320 import RONNet
    return RONNet(RONNet.default_params._replace(**params), dtype='fp32', max_batch=2, device=dev)


def _dev_lists(dev, *lists):
    import torch
    return [[torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in lst] for lst in lists]


def _run(net, dev, logits, loc, objl, objp, gcl, glo, rand_obj, rand_cls, **kwargs):
    import torch
    d = _dev_lists(dev, logits, loc, objl, objp, gcl, glo)
    gsc = [torch.zeros(t.shape, dtype=torch.float32, device=dev) for t in d[4]]
    r = net.losses(d[0], d[1], d[2], d[3], d[4], d[5], gsc, rand_objness=torch.from_numpy(rand_obj).to(dev),
                   rand_cls=torch.from_numpy(rand_cls).to(dev), **kwargs)
    assert all(r[k].dim() == 0 and r[k].is_cuda for k in KEYS)
    return np.array([r[k].item() for k in KEYS], np.float32), r['counts'].cpu().numpy()


def _compare(got, counts, logits, loc, objl, objp, gcl, glo, rand_obj, rand_cls, **kwargs):
    f = er.flatten_rows
    C = logits[0].shape[-1]
    fi = dict(logits=f(logits, C), localisations=f(loc, 4), objness_logits=f(objl, 2), objness_pred=f(objp), gclasses=f(gcl),
              glocalisations=f(glo, 4), rand_obj=rand_obj, rand_cls=rand_cls)
    ref, ref_counts, terms = er.losses_ref(**fi, **kwargs)
    bound = er.losses_bound(fi['logits'], fi['localisations'], fi['objness_logits'], fi['glocalisations'], terms)
    print('losses', got, 'reference', ref, 'bound', bound, 'counts', counts)
    assert np.array_equal(counts, ref_counts), (counts, ref_counts)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    ok = ~np.isnan(ref)
    assert (np.abs(got.astype(np.float64) - ref)[ok] <= bound[ok]).all(), (got, ref, bound)
    return ref


@pytest.mark.parametrize('case', LOSS_CASES, ids=[c.name for c in LOSS_CASES])
def test_hand_cases(dev, case):
    net = _net(dev)
    args = (case.logits, case.localisations, case.objness_logits, case.objness_pred, case.gclasses, case.glocalisations,
            case.rand_objness, case.rand_cls)
    got, counts = _run(net, dev, *args, **case.kwargs)
    ref = _compare(got, counts, *args, **case.kwargs)
    again, counts2 = _run(net, dev, *args, **case.kwargs)
    assert got.tobytes() == again.tobytes() and np.array_equal(counts, counts2)          # bit-identical, NaN included
    if case.name == 'no_positive':
        assert not got.any()
    if case.name == 'empty_class_set_is_nan':
        assert np.isnan(got[0]) and np.isnan(got[3]) and np.isnan(ref[0])


def test_ron320_shapes_with_encodes_own_targets(dev):
    """The RON-320 layer shapes at N = 2: 42 500 rows, 167 workgroups of partial sums, the last one ragged."""
    import torch
    from oracle import synth
    from ron_tensorflow_amd import ops
    net = _net(dev)
    gl, gb = ec.random_ground_truth(21, 2, 7, counts=[7, 4])
    gcl, glo, gsc, _ = net.bboxes_encode(torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev), net.anchors((320, 320)))
    cls, obj, loc = synth.head_tensors(9, batch=2, bg=2.0, ob=0.0)
    objp = [ops.softmax_last(torch.from_numpy(o).to(dev), pick=1).cpu().numpy() for o in obj]
    rs = np.random.RandomState(3)
    rows = sum(t.numel() for t in gcl)
    assert rows == 2 * 21250
    rand_obj, rand_cls = rs.uniform(0, 1, rows).astype(np.float32), rs.uniform(0, 1, rows).astype(np.float32)
    args = (cls, loc, obj, objp, [t.cpu().numpy() for t in gcl], [t.cpu().numpy() for t in glo], rand_obj, rand_cls)
    got, counts = _run(net, dev, *args)
    assert counts[0] > 0 and counts[2] > 0 and counts[4] > counts[0] and counts[5] > counts[2]
    _compare(got, counts, *args)
    again, _ = _run(net, dev, *args)
    assert got.tobytes() == again.tobytes()


def test_random_draws_come_from_the_generator(dev):
    import torch
    case = [c for c in LOSS_CASES if c.name == 'every_negative_selected'][0]
    net = _net(dev)
    d = _dev_lists(dev, case.logits, case.localisations, case.objness_logits, case.objness_pred, case.gclasses, case.glocalisations)
    out = []
    for _ in range(2):
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        r = net.losses(d[0], d[1], d[2], d[3], d[4], d[5], None, generator=gen)
        out.append(np.array([r[k].item() for k in KEYS], np.float32).tobytes() + r['counts'].cpu().numpy().tobytes())
    assert out[0] == out[1]


def test_validation_losses_equals_the_three_calls(dev):
    """64 x 64, the smallest RON input, fp32: net() -> bboxes_encode -> losses in one call, bit for bit the separate calls."""
    import torch
    from ron_tensorflow_amd.weights import synthetic_images, synthetic_weights
    net = _net(dev, img_shape=(64, 64), feat_shapes=[(1, 1), (2, 2), (4, 4), (8, 8)])
    net.load_weights(synthetic_weights('reducedfc', seed=1, bg=2.0, ob=0.0))
    images = torch.from_numpy(synthetic_images(2, seed=2, img_shape=(64, 64))).to(dev)
    gl, gb = ec.random_ground_truth(31, 2, 4, counts=[3, 1], lo=0.3, hi=0.8)
    d_gl, d_gb = torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev)
    rows = 2 * 10 * (1 + 4 + 16 + 64)
    rs = np.random.RandomState(8)
    r_obj = torch.from_numpy(rs.uniform(0, 1, rows).astype(np.float32)).to(dev)
    r_cls = torch.from_numpy(rs.uniform(0, 1, rows).astype(np.float32)).to(dev)
    fused = net.validation_losses(images, d_gl, d_gb, rand_objness=r_obj, rand_cls=r_cls)
    _, logits, objp, objl, loc, _ = net.net(images, is_training=False, end_points=())
    gcl, glo, gsc, _ = net.bboxes_encode(d_gl, d_gb, net.anchors((64, 64)))
    sep = net.losses(logits, loc, objl, objp, gcl, glo, gsc, rand_objness=r_obj, rand_cls=r_cls)
    for k in KEYS:
        assert fused[k].cpu().numpy().tobytes() == sep[k].cpu().numpy().tobytes(), k
    assert np.array_equal(fused['counts'].cpu().numpy(), sep['counts'].cpu().numpy())
    counts = sep['counts'].cpu().numpy()
    assert counts[0] > 0 and counts[0] + counts[1] <= rows
    # and the value itself, against the float64 reference on the same head tensors and targets
    got = np.array([sep[k].item() for k in KEYS], np.float32)
    tonp = lambda lst: [t.cpu().numpy() for t in lst]
    _compare(got, counts, tonp(logits), tonp(loc), tonp(objl), tonp(objp), tonp(gcl), tonp(glo), r_obj.cpu().numpy(), r_cls.cpu().numpy())
    net.close()
