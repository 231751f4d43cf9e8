"""GPU: ron_losses_grad (ops.losses_grad, RONNet.losses_and_gradients, the differentiable RONNet.losses) against the references of
tests/loss_grad_ref.py.

`losses` and `counts` are those of ops.losses bit for bit; the localisation gradient equals the float32 emulation bit for bit; the
class and objectness gradients lie within grad_bound ("Loss gradients") of the float64 reference; rows
outside the sets are exactly zero; every element is written; two calls give the same bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_cases as ec  # noqa: E402
import loss_grad_cases as gc  # noqa: E402
import loss_grad_ref as gr  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = gc.grad_cases()
LAYOUT = gc.layout_cases()
KEYS = ('cross_entropy_pos', 'cross_entropy_objectness', 'localization', 'total')
SENTINEL = -12345.5


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def net(dev):
    from ron_tensorflow_amd.nets.ron_vgg_320 import RONNet
    return RONNet(RONNet.default_params, dtype='fp32', max_batch=2, device=dev)


def _to_dev(dev, case):
    import torch
    up = lambda lst: [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in lst]
    return dict(logits=up(case.logits), localisations=up(case.localisations), objness_logits=up(case.objness_logits),
                objness_pred=up(case.objness_pred), gclasses=up(case.gclasses), glocalisations=up(case.glocalisations),
                rand_objness=torch.from_numpy(case.rand_objness).to(dev), rand_cls=torch.from_numpy(case.rand_cls).to(dev))


def _flat(per_layer, width):
    return np.concatenate([t.cpu().numpy().reshape(-1, width) for t in per_layer])


def _call(dev, case, sentinel=False):
    """ops.losses and ops.losses_grad on the case: (losses, counts, d_cls, d_obj, d_loc) as flat numpy arrays."""
    import torch
    from ron_tensorflow_amd import ops
    d = _to_dev(dev, case)
    out = None
    if sentinel:
        out = tuple([torch.full(t.shape, SENTINEL, dtype=torch.float32, device=dev) for t in d[k]]
                    for k in ('logits', 'objness_logits', 'localisations'))
    fwd, fwd_counts = ops.losses(**d, **case.kwargs)
    got, counts, d_cls, d_obj, d_loc = ops.losses_grad(**d, **case.kwargs, out=out)
    assert got.cpu().numpy().tobytes() == fwd.cpu().numpy().tobytes()                  # NaN included
    assert np.array_equal(counts.cpu().numpy(), fwd_counts.cpu().numpy())
    for lst, like in ((d_cls, d['logits']), (d_obj, d['objness_logits']), (d_loc, d['localisations'])):
        assert all(g.shape == t.shape and g.dtype == torch.float32 and g.is_cuda for g, t in zip(lst, like))
    C = case.logits[0].shape[-1]
    return got.cpu().numpy(), counts.cpu().numpy(), _flat(d_cls, C), _flat(d_obj, 2), _flat(d_loc, 4)


def _check(case, counts, d_cls, d_obj, d_loc):
    fi = gc.flat_inputs(case)
    ref = gr.grads_ref(**fi, **case.kwargs)
    emu = gr.grads_emulated(**fi, **case.kwargs)
    b_cls, b_obj = gr.grad_bound(fi['logits'], fi['objness_logits'], ref)
    mk = ref['masks']
    assert np.array_equal(counts, ref['counts'])
    assert np.array_equal(d_loc, emu['d_loc']), np.abs(d_loc - emu['d_loc']).max()
    for name, got, want, bound, inside in (('d_cls', d_cls, ref['d_cls'], b_cls, mk['cls_set']),
                                           ('d_obj', d_obj, ref['d_obj'], b_obj, mk['obj_set'])):
        ok = ~np.isnan(want)
        err = np.abs(got.astype(np.float64) - want)
        with np.errstate(invalid='ignore', divide='ignore'):
            print(case.name, name, 'largest error', err[ok].max(initial=0.0), 'largest error / bound',
                  np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0))
        assert gr.within(got, want, bound), name
        outside = got[~inside]
        assert (outside == 0).all() and not np.signbit(outside).any(), name
        rows = inside & ok.all(axis=1)
        assert (np.abs(got[rows].astype(np.float64).sum(axis=1)) <= bound[rows].sum(axis=1)).all(), name
    outside = d_loc[~mk['cls_pos']]
    assert (outside == 0).all() and not np.signbit(outside).any()
    return ref, emu


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_hand_cases(dev, case):
    assert case.condition(case, gc.loss_case_masks(case))
    losses, counts, d_cls, d_obj, d_loc = _call(dev, case)
    ref, emu = _check(case, counts, d_cls, d_obj, d_loc)
    if case.name in ('no_positive', 'empty_class_set_is_nan'):
        assert not d_cls.any()
    if case.name == 'no_positive':
        assert not d_obj.any() and not d_loc.any()
    if case.name == 'no_positive_above_the_objectness_threshold':
        assert not d_loc.any() and d_obj.any()
    if case.name == 'label_equal_to_num_classes':
        nan_rows = ref['masks']['cls_set'] & (ref['masks']['g'] == gc.C)
        assert nan_rows.any() and np.isnan(d_cls[nan_rows]).all() and not np.isnan(d_cls[~nan_rows]).any() and np.isnan(losses[0])
    if case.name == 'class_weight_zero':
        assert not d_cls.any() and d_obj.any() and d_loc.any()


@pytest.mark.parametrize('case', LAYOUT, ids=[c.name for c in LAYOUT])
def test_layout_cases(dev, case):
    losses, counts, d_cls, d_obj, d_loc = _call(dev, case, sentinel=True)
    for g in (d_cls, d_obj, d_loc):
        assert not (g == np.float32(SENTINEL)).any()                                    # every element was written
    _check(case, counts, d_cls, d_obj, d_loc)
    assert d_cls.any() and d_obj.any() and d_loc.any()


def _ron320_inputs(dev, net):
    import torch
    from oracle import synth
    from ron_tensorflow_amd import ops
    gl, gb = ec.random_ground_truth(21, 2, 7, counts=[7, 4])
    gcl, glo, gsc, _ = net.bboxes_encode(torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev), net.anchors((320, 320)))
    cls, obj, loc = synth.head_tensors(9, batch=2, bg=2.0, ob=0.0)
    objp = [ops.softmax_last(torch.from_numpy(o).to(dev), pick=1).cpu().numpy() for o in obj]
    rs = np.random.RandomState(3)
    rows = sum(t.numel() for t in gcl)
    assert rows == 2 * 21250
    d = dict(logits=cls, localisations=loc, objness_logits=obj, objness_pred=objp, gclasses=[t.cpu().numpy() for t in gcl],
             glocalisations=[t.cpu().numpy() for t in glo], rand_objness=rs.uniform(0, 1, rows).astype(np.float32),
             rand_cls=rs.uniform(0, 1, rows).astype(np.float32))
    return ec._lcase('ron320_batch2', d, None)


def test_ron320_shapes_with_encodes_own_targets(dev, net):
    """The RON-320 layer shapes at N = 2: 42 500 rows, 167 workgroups, the last one ragged, three layer boundaries inside workgroups."""
    case = _ron320_inputs(dev, net)
    losses, counts, d_cls, d_obj, d_loc = _call(dev, case, sentinel=True)
    assert counts[0] > 0 and counts[2] > 0 and counts[4] > counts[0] and counts[5] > counts[2]
    for g in (d_cls, d_obj, d_loc):
        assert not (g == np.float32(SENTINEL)).any()
    _check(case, counts, d_cls, d_obj, d_loc)


def test_two_calls_give_equal_bytes(dev, net):
    case = _ron320_inputs(dev, net)
    a, b = _call(dev, case), _call(dev, case)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def _leaf_case(dev):
    case = [c for c in CASES if c.name == 'every_negative_selected'][0]
    d = _to_dev(dev, case)
    return case, d


def _net_losses(net, d, **kw):
    return net.losses(d['logits'], d['localisations'], d['objness_logits'], d['objness_pred'], d['gclasses'], d['glocalisations'], None,
                      rand_objness=d['rand_objness'], rand_cls=d['rand_cls'], **kw)


def test_autograd_total_equals_losses_and_gradients(dev, net):
    import torch
    case, d = _leaf_case(dev)
    plain = _net_losses(net, d)
    assert all(plain[k].grad_fn is None and not plain[k].requires_grad for k in KEYS)
    both = net.losses_and_gradients(d['logits'], d['localisations'], d['objness_logits'], d['objness_pred'], d['gclasses'],
                                    d['glocalisations'], None, rand_objness=d['rand_objness'], rand_cls=d['rand_cls'])
    assert sorted(both['gradients']) == ['localisations', 'logits', 'objness_logits']
    heads = ('logits', 'objness_logits', 'localisations')
    for k in heads:
        for t in d[k]:
            t.requires_grad_(True)
    out = _net_losses(net, d)
    for k in KEYS:
        assert out[k].grad_fn is not None and out[k].dim() == 0 and out[k].is_cuda
        assert out[k].detach().cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes() == both[k].cpu().numpy().tobytes()
    assert np.array_equal(out['counts'].cpu().numpy(), plain['counts'].cpu().numpy())
    out['total'].backward()
    for k in heads:
        for t, g in zip(d[k], both['gradients'][k]):
            assert t.grad is not None and g.any() and torch.equal(t.grad, g)
    # under no_grad: today's path, today's values
    with torch.no_grad():
        quiet = _net_losses(net, d)
    for k in KEYS:
        assert quiet[k].grad_fn is None and quiet[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes()


def test_autograd_weighs_each_term_by_its_upstream(dev, net):
    import torch
    case, d = _leaf_case(dev)
    both = net.losses_and_gradients(d['logits'], d['localisations'], d['objness_logits'], d['objness_pred'], d['gclasses'],
                                    d['glocalisations'], None, rand_objness=d['rand_objness'], rand_cls=d['rand_cls'])
    for k in ('logits', 'objness_logits', 'localisations'):
        for t in d[k]:
            t.requires_grad_(True)
    out = _net_losses(net, d)
    (3 * out['localization'] + out['cross_entropy_pos']).backward()
    for t, g in zip(d['localisations'], both['gradients']['localisations']):
        assert torch.equal(t.grad, g * 3)
    for t, g in zip(d['logits'], both['gradients']['logits']):
        assert torch.equal(t.grad, g)
    for t in d['objness_logits']:
        assert t.grad is None or not t.grad.any()
    # only some head tensors require grad: the others get none
    case, d = _leaf_case(dev)
    for t in d['localisations']:
        t.requires_grad_(True)
    out = _net_losses(net, d)
    out['total'].backward()
    assert all(t.grad is not None for t in d['localisations']) and all(t.grad is None for t in d['logits'] + d['objness_logits'])


def test_argument_errors(dev):
    import ctypes as C
    from ron_tensorflow_amd import _lib, ops
    case = [c for c in CASES if c.name == 'single_row_batch'][0]
    d = _to_dev(dev, case)
    heads, keep = ops._fill_heads(d['logits'], d['objness_logits'], d['localisations'], None, 21)
    lib = _lib.lib()
    assert lib.ron_losses_grad_workspace_bytes(C.byref(heads), 0) == -1
    assert lib.ron_losses_grad_workspace_bytes(C.byref(heads), 1) == lib.ron_losses_workspace_bytes(C.byref(heads), 1)
    rc = lib.ron_losses_grad(C.byref(heads), None, None, 1, None, None, None, None, 0, None, None, None, None)
    assert rc == -1 and b'ron_losses_grad: null argument' in lib.ron_last_error()
    # every pointer given, the workspace too small; then a layer count out of range: both refused before anything is launched
    import torch
    buf = torch.zeros((64,), dtype=torch.float32, device=dev)
    tg, hg, objp = _lib.Targets(), _lib.HeadGrads(), (C.c_void_p * _lib.RON_MAX_LAYERS)()
    objp[0], tg.gclasses[0], tg.glocalisations[0] = d['objness_pred'][0].data_ptr(), d['gclasses'][0].data_ptr(), d['glocalisations'][0].data_ptr()
    hg.d_cls[0] = hg.d_obj[0] = hg.d_loc[0] = buf.data_ptr()
    cfg = _lib.LossCfg(0.03, 3.0, 1. / 3, 1. / 3)
    args = lambda h, nbytes: (C.byref(h), objp, C.byref(tg), 1, _lib.ptr(buf), _lib.ptr(buf), C.byref(cfg), _lib.ptr(buf), nbytes,
                              _lib.ptr(buf), _lib.ptr(buf), C.byref(hg), None)
    assert lib.ron_losses_grad(*args(heads, 8)) == -1 and b'workspace of 8 bytes' in lib.ron_last_error()
    heads.num_layers = 0
    assert lib.ron_losses_grad(*args(heads, 256)) == -1 and b'0 layers not in' in lib.ron_last_error()
    with pytest.raises(AssertionError):
        ops.losses_grad(**d, out=(d['logits'], d['objness_logits'], d['objness_logits']))      # a gradient tensor of the wrong shape
    del keep
