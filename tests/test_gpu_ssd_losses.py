"""GPU: ron_ssd_losses / ron_ssd_losses_grad (ops.ssd_losses, ops.ssd_losses_grad, SSDNet.losses, losses_and_gradients,
validation_losses) against the references of tests/ssd_loss_ref.py.

The select is exact on the device's own values: with `nvalues` copied back numpy recomputes k, t and the mined mask from those bits,
and `counts` and the mask (read off the d_cls rows) must be equal, for every case; `nvalues` lies within the expf bound of the
float64 background probability.  On the hand cases that mask is also the float64 reference's own.  Losses and gradients lie within
the derived bounds of the float64 reference evaluated under the mask, NaN where it is NaN; rows outside the
sets are +0; every element is written; two calls give the same bytes; the gradient entry gives the forward entry's bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_cases as ec  # noqa: E402
import ssd_loss_cases as sc  # noqa: E402
import ssd_loss_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

HAND = sc.hand_cases()
LAYOUT = sc.layout_cases()
VALUES = sc.value_cases()
KEYS = ('cross_entropy_pos', 'cross_entropy_neg', 'localization', 'total')
SENTINEL = -12345.5


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _to_dev(dev, case):
    import torch
    up = lambda lst: [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in lst]
    return dict(logits=up(case.logits), localisations=up(case.localisations), gclasses=up(case.gclasses),
                glocalisations=up(case.glocalisations), gscores=up(case.gscores))


def _flat(per_layer, width):
    return np.concatenate([t.cpu().numpy().reshape(-1, width) for t in per_layer])


def _call(dev, case, sentinel=False):
    """ops.ssd_losses and ops.ssd_losses_grad on the case: (losses, counts, nvalues, d_cls, d_loc) as flat numpy arrays."""
    import torch
    from ron_tensorflow_amd import ops
    d = _to_dev(dev, case)
    out = None
    if sentinel:
        out = tuple([torch.full(t.shape, SENTINEL, dtype=torch.float32, device=dev) for t in d[k]] for k in ('logits', 'localisations'))
    fwd, fwd_counts, fwd_nv = ops.ssd_losses(**d, mining=case.mining, nvalues=True, **case.kwargs)
    quiet = ops.ssd_losses(**d, mining=case.mining, **case.kwargs)
    got, counts, nv, d_cls, d_loc = ops.ssd_losses_grad(**d, mining=case.mining, nvalues=True, out=out, **case.kwargs)
    assert quiet[2] is None and quiet[0].cpu().numpy().tobytes() == fwd.cpu().numpy().tobytes()
    assert got.cpu().numpy().tobytes() == fwd.cpu().numpy().tobytes()                  # NaN included
    assert np.array_equal(counts.cpu().numpy(), fwd_counts.cpu().numpy()) and counts.dtype == torch.int32
    assert nv.cpu().numpy().tobytes() == fwd_nv.cpu().numpy().tobytes()
    segs = 1 if case.mining == 'batch' else len(case.logits)
    assert tuple(counts.shape) == (segs, 4) and tuple(got.shape) == (4,)
    for lst, like in ((d_cls, d['logits']), (d_loc, d['localisations'])):
        assert all(g.shape == t.shape and g.dtype == torch.float32 and g.is_cuda for g, t in zip(lst, like))
    C = case.logits[0].shape[-1]
    return got.cpu().numpy(), counts.cpu().numpy(), nv.cpu().numpy(), _flat(d_cls, C), _flat(d_loc, 4)


def _check(case, losses, counts, nv, d_cls, d_loc, hand=False):
    fi = sc.flat_inputs(case)
    ratio = fi.get('negative_ratio', 3.)
    pos, cand = sr.row_sets(fi['s'], fi.get('match_threshold', 0.5))
    # the select, exactly, on the device's own values
    assert nv.dtype == np.float32 and (nv[~cand] == np.float32(1)).all()
    want_counts, mined, _ = sr.mine(nv, pos, cand, fi['layer_rows'], fi['N'], fi['mining'], ratio)
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    with np.errstate(invalid='ignore'):
        mined_dev = ~pos & (d_cls[:, 0] != 0)
    assert np.array_equal(mined_dev, mined)
    ref = sr.losses_ref(**fi, mined=mined)
    p0_err = np.abs(nv.astype(np.float64) - ref['v'])
    assert (p0_err <= np.where(cand, sr.p0_bound(fi['x']), 0.0)).all()
    if hand:
        own = sr.losses_ref(**fi)
        assert np.array_equal(counts, own['counts']) and np.array_equal(mined, own['mined'])
    b = sr.losses_bound(fi['x'], fi['loc'], fi['gloc'], ref, fi.get('alpha', 1.))
    b_cls, b_loc = sr.grad_bound(fi['x'], fi['loc'], fi['gloc'], ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        print(case.name, 'losses', losses, 'error / bound', np.abs(losses - ref['losses']) / b)
        for name, got, want, bound in (('d_cls', d_cls, ref['d_cls'], b_cls), ('d_loc', d_loc, ref['d_loc'], b_loc)):
            err = np.abs(got.astype(np.float64) - want)
            print(case.name, name, 'largest error', np.nanmax(err, initial=0.0), 'largest error / bound',
                  np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0))
    assert sr.within(losses, ref['losses'], b), (losses, ref['losses'], b)
    assert sr.within(d_cls, ref['d_cls'], b_cls)
    assert sr.within(d_loc, ref['d_loc'], b_loc)
    outside = d_cls[~(pos | mined)]
    assert (outside == 0).all() and not np.signbit(outside).any()
    outside = d_loc[~pos]
    assert (outside == 0).all() and not np.signbit(outside).any()
    return ref


@pytest.mark.parametrize('case', HAND, ids=[c.name for c in HAND])
def test_hand_cases(dev, case):
    losses, counts, nv, d_cls, d_loc = _call(dev, case)
    assert np.array_equal(counts, np.array(case.expect['counts'], np.int32))
    ref = _check(case, losses, counts, nv, d_cls, d_loc, hand=True)
    if case.name == 'no_candidates':
        assert losses[1] == 0 and not d_cls[~ref['pos']].any()
    if case.name == 'positive_label_equal_to_num_classes':
        assert np.isnan(d_cls[0]).all() and not np.isnan(d_cls[1:]).any() and np.isnan(losses[[0, 3]]).all()
    if case.name == 'candidate_p0_exactly_one':
        assert nv[1] == np.float32(1) and not d_cls[1].any()
    if case.name == 'layer_without_positives':
        assert np.isfinite(losses).all() and not d_loc[8:].any()


@pytest.mark.parametrize('case', LAYOUT + VALUES, ids=[c.name for c in LAYOUT + VALUES])
def test_layout_and_value_cases(dev, case):
    losses, counts, nv, d_cls, d_loc = _call(dev, case, sentinel=True)
    for g in (d_cls, d_loc):
        assert not (g == np.float32(SENTINEL)).any()                                    # every element was written
    _check(case, losses, counts, nv, d_cls, d_loc)
    if nv.size >= 64:
        assert counts[:, 3].sum() > 0 and d_cls.any() and d_loc.any()


def test_two_calls_give_equal_bytes(dev):
    for case in (LAYOUT[0], LAYOUT[1], VALUES[0]):
        a, b = _call(dev, case), _call(dev, case)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def _nets(dev):
    from ron_tensorflow_amd.nets import ssd_vgg_300, ssd_vgg_512
    return {'batch': ssd_vgg_300.SSDNet(dtype='fp32', max_batch=2, device=dev), 'layer': ssd_vgg_512.SSDNet(dtype='fp32', max_batch=2, device=dev)}


@pytest.mark.parametrize('mining', ['batch', 'layer'])
def test_autograd_equals_losses_and_gradients_times_the_upstream_scalars(dev, mining):
    import torch
    net = _nets(dev)[mining]
    case = [c for c in LAYOUT if c.name == 'three_layers_c3_n3_' + mining][0]
    d = _to_dev(dev, case)
    args = lambda: (d['logits'], d['localisations'], d['gclasses'], d['glocalisations'], d['gscores'])
    plain = net.losses(*args())
    assert all(plain[k].grad_fn is None and plain[k].dim() == 0 and plain[k].is_cuda for k in KEYS)
    both = net.losses_and_gradients(*args())
    assert sorted(both['gradients']) == ['localisations', 'logits']
    direct = _call(dev, case)
    assert np.array_equal(plain['counts'].cpu().numpy(), direct[1])                      # the class's own mining mode
    for k in ('logits', 'localisations'):
        for t in d[k]:
            t.requires_grad_(True)
    out = net.losses(*args())
    for k in KEYS:
        assert out[k].grad_fn is not None and out[k].dim() == 0
        assert out[k].detach().cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes() == both[k].cpu().numpy().tobytes()
    assert np.array_equal(out['counts'].cpu().numpy(), plain['counts'].cpu().numpy())
    up = 2 * out['cross_entropy_pos'] + 3 * out['cross_entropy_neg'] + 5 * out['localization'] + 7 * out['total']
    grads = torch.autograd.grad(up, d['logits'] + d['localisations'])
    n = len(d['logits'])
    for g, unit, sc_ in zip(grads[:n], both['gradients']['logits'], d['gscores']):
        w = torch.where(sc_ > 0.5, torch.tensor(9.0, device=dev), torch.tensor(10.0, device=dev)).unsqueeze(-1)
        assert unit.any() and torch.equal(g, unit * w)
    for g, unit in zip(grads[n:], both['gradients']['localisations']):
        assert unit.any() and torch.equal(g, unit * 12.0)
    # only the localisations require grad: the logits get none; under no_grad nothing is recorded
    d = _to_dev(dev, case)
    for t in d['localisations']:
        t.requires_grad_(True)
    net.losses(*args())['total'].backward()
    assert all(t.grad is not None for t in d['localisations']) and all(t.grad is None for t in d['logits'])
    with torch.no_grad():
        quiet = net.losses(*args())
    assert all(quiet[k].grad_fn is None and quiet[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes() for k in KEYS)


def test_module_level_ssd_losses(dev):
    from ron_tensorflow_amd.nets import ssd_vgg_300, ssd_vgg_512
    for mod, mining in ((ssd_vgg_300, 'batch'), (ssd_vgg_512, 'layer')):
        case = [c for c in LAYOUT if c.name == 'three_layers_c2_n2_' + mining][0]
        d = _to_dev(dev, case)
        out = mod.ssd_losses(d['logits'], d['localisations'], d['gclasses'], d['glocalisations'], d['gscores'], 0.5, 3., 1.)
        direct = _call(dev, case)
        assert np.array_equal(np.array([out[k].item() for k in KEYS], np.float32), direct[0])
        assert np.array_equal(out['counts'].cpu().numpy(), direct[1])


def test_ssd300_end_to_end(dev):
    """SSD-300, fp32, batch 2 (17 464 rows), synthetic weights: validation_losses is net -> bboxes_encode -> losses bit for bit."""
    import torch
    from ron_tensorflow_amd.nets import ssd_vgg_300
    from ron_tensorflow_amd.weights import ssd300_synthetic_weights, synthetic_images
    net = ssd_vgg_300.SSDNet(dtype='fp32', max_batch=2, device=dev)
    net.load_weights(ssd300_synthetic_weights(seed=6))
    images = torch.from_numpy(synthetic_images(2, seed=0, img_shape=(300, 300))).to(dev)
    gl, gb = ec.random_ground_truth(21, 2, 7, counts=[7, 4])
    gl_d, gb_d = torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev)
    val = net.validation_losses(images, gl_d, gb_d)
    _, localisations, logits, _ = net.net(images, is_training=False, end_points=())
    assert sum(t.numel() for t in logits) // 21 == 17464
    gcl, glo, gsc, _ = net.bboxes_encode(gl_d, gb_d, net.anchors((300, 300)))
    manual = net.losses(logits, localisations, gcl, glo, gsc)
    for k in KEYS:
        assert val[k].cpu().numpy().tobytes() == manual[k].cpu().numpy().tobytes() and np.isfinite(val[k].item())
    counts = val['counts'].cpu().numpy()
    assert np.array_equal(counts, manual['counts'].cpu().numpy()) and counts.shape == (1, 4)
    assert (counts[:, 0] > 0).all() and counts[0, 3] > 0
    net.close()
