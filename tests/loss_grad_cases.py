"""Hand-built cases of the loss gradient (ron_losses_grad): the loss cases of tests/encode_cases.py, reused unedited, and the
decision points of the gradient itself.  Every case carries `condition`, asserted on the reference's own masks, as there.
`KILLS` names, for every mutant of tests/loss_grad_ref.py, the case that tells it from the unmutated emulation.
"""
import numpy as np

import encode_cases as ec
import encode_ref as er
from encode_cases import _assert, _lcase, loss_case_masks, loss_inputs
from loss_grad_ref import ONE_NINTH

F = np.float32
C = ec.NUM_CLASSES

KILLS = {
    'keep_one_hot': 'every_negative_selected',
    'mean_all_rows': 'random_value_equal_to_p_and_ignored_rows',
    'le_kink': 'difference_exactly_one_ninth',
    'ignored_as_negative': 'random_value_equal_to_p_and_ignored_rows',
    'loc_all_positives': 'no_positive_above_the_objectness_threshold',
    'no_zero_scale': 'no_positive',
    'no_max': 'large_logits',
}


def flat_inputs(c):
    f = er.flatten_rows
    nc = c.logits[0].shape[-1]
    return dict(logits=f(c.logits, nc), localisations=f(c.localisations, 4), objness_logits=f(c.objness_logits, 2),
                objness_pred=f(c.objness_pred), gclasses=f(c.gclasses), glocalisations=f(c.glocalisations, 4),
                rand_obj=c.rand_objness, rand_cls=c.rand_cls)


def _diffs(c, mk):
    """float32 differences pred - target of the rows the localisation term reads: [rows, 4]."""
    d = er.flatten_rows(c.localisations, 4) - er.flatten_rows(c.glocalisations, 4)
    return d[mk['cls_pos']]


def _gate_open(d):
    d['objness_pred'] = [np.full_like(p, 0.5) for p in d['objness_pred']]
    return d


def grad_cases():
    cases = list(ec.loss_cases())

    d = _gate_open(loss_inputs(11))
    d['localisations'] = [np.where(np.arange(4) % 2 == 0, g, p).astype(F) for p, g in zip(d['localisations'], d['glocalisations'])]
    cases.append(_lcase('difference_zero', d, lambda c, mk: _assert(
        mk['counts'][2] > 0 and (_diffs(c, mk)[:, 0::2] == 0).all() and (_diffs(c, mk)[:, 1::2] != 0).all())))

    below, above = np.nextafter(ONE_NINTH, F(0)), np.nextafter(ONE_NINTH, F(1))
    d = _gate_open(loss_inputs(12))
    d['glocalisations'] = [np.zeros_like(t) for t in d['glocalisations']]
    d['localisations'] = [np.broadcast_to(np.array([below, above, -below, -above], F), t.shape).copy() for t in d['localisations']]
    cases.append(_lcase('one_ulp_on_either_side_of_one_ninth', d, lambda c, mk: _assert(
        mk['counts'][2] > 0 and below < ONE_NINTH < above and np.spacing(below) == ONE_NINTH - below
        and above - ONE_NINTH == np.spacing(ONE_NINTH)
        and (np.abs(_diffs(c, mk)) < ONE_NINTH).tolist() == [[True, False, True, False]] * int(mk['counts'][2]))))

    d = _gate_open(loss_inputs(13))
    d['gclasses'] = [np.where((g > 0) & (np.arange(g.size).reshape(g.shape) % 2 == 0), C, g) for g in d['gclasses']]
    cases.append(_lcase('label_equal_to_num_classes', d, lambda c, mk: _assert(
        (mk['g'][mk['cls_set']] == C).any() and ((mk['g'][mk['cls_set']] > 0) & (mk['g'][mk['cls_set']] < C)).any()
        and mk['g'].max() == C)))

    d = loss_inputs(14)
    cases.append(_lcase('class_weight_zero', d, lambda c, mk: _assert(
        er._loss_weights(c.kwargs['alpha'], c.kwargs['beta'])[0] == 0 and mk['counts'][5] > 0), alpha=0.5, beta=0.5))

    d = _gate_open(loss_inputs(15, n=1, shapes=[(1, 1, 1)]))
    d['gclasses'] = [np.full((1, 1, 1, 1), 7, np.int64)]
    cases.append(_lcase('single_row_batch', d, lambda c, mk: _assert(
        mk['g'].size == 1 and mk['counts'].tolist() == [1, 0, 1, 0, 1, 1])))
    return cases


# ------------------------------------------------------------------------------------------------------------ layout cases
LAYOUT_CLASSES = (2, 3, 21, 128)
# (batch, layers [(H, W, A)]): one row; a layer boundary inside a wave; then the total row counts 63, 64, 65 (around the wave), 255,
# 256, 257 (around the 256-thread workgroup) and 513 (a third workgroup with one row)
LAYOUT_LAYERS = (
    (2, [(1, 1, 1)]),
    (2, [(1, 1, 1), (3, 5, 7)]),
    (1, [(3, 3, 7)]),
    (2, [(4, 4, 2)]),
    (1, [(1, 1, 1), (8, 8, 1)]),
    (3, [(5, 17, 1)]),
    (2, [(8, 8, 2)]),
    (1, [(16, 16, 1), (1, 1, 1)]),
    (1, [(16, 16, 2), (1, 1, 1)]),
)
LAYOUT_ROWS = (2, 212, 63, 64, 65, 255, 256, 257, 513)


def layout_case(num_classes, batch, layers, seed=0):
    """Seeded inputs of the given shape: ~ 25 % positive, 10 % ignored rows, objectness predictions on both sides of the gate."""
    rs = np.random.RandomState(1000 * num_classes + 10 * batch + len(layers) + seed)
    d = dict(logits=[], localisations=[], objness_logits=[], objness_pred=[], gclasses=[], glocalisations=[])
    rows = 0
    for (h, w, a) in layers:
        shp = (batch, h, w, a)
        d['logits'].append((rs.randn(*shp + (num_classes,)) * 2).astype(F))
        d['localisations'].append((rs.randn(*shp + (4,)) * 0.2).astype(F))
        d['objness_logits'].append(rs.randn(*shp + (2,)).astype(F))
        d['objness_pred'].append(rs.uniform(0, 0.2, shp + (1,)).astype(F))
        u = rs.uniform(0, 1, shp)
        d['gclasses'].append(np.where(u < 0.25, rs.randint(1, num_classes, shp), np.where(u < 0.35, -1, 0)).astype(np.int64))
        d['glocalisations'].append((rs.randn(*shp + (4,)) * 0.2).astype(F))
        rows += int(np.prod(shp))
    d['gclasses'][0].reshape(-1)[0] = 1                     # at least one positive, above the gate
    d['objness_pred'][0].reshape(-1)[0] = 0.5
    d['rand_objness'] = rs.uniform(0, 1, rows).astype(F)
    d['rand_cls'] = rs.uniform(0, 1, rows).astype(F)
    return _lcase('C%d_N%d_%s' % (num_classes, batch, '_'.join('%dx%dx%d' % s for s in layers)), d,
                  lambda c, mk: _assert(mk['counts'][2] > 0 and mk['g'].size == rows))


def layout_cases():
    return [layout_case(c, n, layers) for c in LAYOUT_CLASSES for (n, layers) in LAYOUT_LAYERS]
