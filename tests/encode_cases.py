"""Hand-built decision-point cases of RONNet.bboxes_encode and RONNet.losses (CPU data only; the GPU tests run the same cases).

Encode cases use anchor lists of one or two tiny layers on a 64 x 64 image with allowed border 16, so that every coordinate, the
inside bounds (-0.25, 1.25) and the overlaps that matter are exact binary fractions.  Every case carries `condition`, a function
that asserts on the reference's own intermediate values that the case really sits where its name says, and `catches`, the
mutants of tests/encode_ref.py it must tell from the reference.
"""
import collections
import os

import numpy as np

from encode_ref import F, RON_MAX_GT, AnchorTable, encode_np, loss_masks, overlap_matrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

EncodeCase = collections.namedtuple('EncodeCase', 'name anchors borders img_shape glabels gbboxes low high condition catches')

IMG = (64, 64)
BORDER = 16                                       # bounds -16 / 64 = -0.25 and 80 / 64 = 1.25


def grid_layer(ys, xs, hs, ws):
    """One feature layer: cell (r, c) is centred at (ys[r], xs[c]); anchor k has size (hs[k], ws[k])."""
    y = np.repeat(np.asarray(ys, F)[:, None], len(xs), axis=1)[..., None]
    x = np.repeat(np.asarray(xs, F)[None, :], len(ys), axis=0)[..., None]
    return (y, x, np.asarray(hs, F), np.asarray(ws, F))


def cell(y, x, h, w):
    return grid_layer([y], [x], [h], [w])


QUADS = [grid_layer([0.25, 0.75], [0.25, 0.75], [0.5], [0.5])]        # four anchors: the quadrants of the image


def _case(name, anchors, labels, boxes, condition, catches=(), low=0.3, high=0.5, g=None):
    g = g or len(labels)
    gl = np.zeros((1, g), np.int32)
    gb = np.zeros((1, g, 4), F)
    gl[0, :len(labels)] = labels
    gb[0, :len(boxes)] = np.asarray(boxes, F).reshape(-1, 4)
    return EncodeCase(name, anchors, [BORDER] * len(anchors), IMG, gl, gb, low, high, condition, tuple(catches))


def table(case):
    return AnchorTable(case.anchors, case.borders, case.img_shape)


def reference(case, mut=(), image=0):
    return encode_np(case.glabels[image], case.gbboxes[image], table(case), case.high, case.low, mut=mut)


def _ov(case):
    return overlap_matrix(case.gbboxes[0], table(case))


# ------------------------------------------------------------------------------------------------------------ the cases
def _cond_a(case):
    ov, (cls, loc, sc, bb, m) = _ov(case), reference(case)
    assert ov[0, 1] == F(0.5) == F(case.high)                 # exactly on the threshold
    assert m[0] == 0 and m[1] == 0 and cls[1] == 3            # ... and still matched (the claim went to anchor 0)


def _cond_b(case):
    ov, (cls, loc, sc, bb, m) = _ov(case), reference(case)
    assert ov[0, 1] == F(0.25) == F(case.low)
    assert m[1] == -2 and cls[1] == -1 and sc[1] == F(0.25)


def _cond_c(case):
    ov, (cls, loc, sc, bb, m) = _ov(case), reference(case)
    assert ov[0, 2] == ov[1, 2] == F(0.5)                     # both boxes tie on the large anchor
    assert m[2] == 0 and cls[2] == 3


def _cond_d(case):
    ov, (cls, loc, sc, bb, m) = _ov(case), reference(case)
    assert ov[0, 0] == ov[0, 1] and F(case.low) <= ov[0, 0] < F(case.high)
    assert m[0] == 0 and m[1] == -2                           # the lower anchor is claimed, the other one ignored


def _cond_e(case):
    ov, (cls, loc, sc, bb, m) = _ov(case), reference(case)
    assert np.argmax(ov[0]) == 0 and np.argmax(ov[1]) == 0    # both boxes claim anchor 0
    assert ov[1, 0] > ov[0, 0]
    assert m[0] == 0 and cls[0] == 3 and sc[0] == ov[0, 0] == F(0.25)


def _cond_f(case):
    ov, (cls, loc, sc, bb, m) = _ov(case), reference(case)
    assert np.argmax(ov[:, 0]) == 1                           # anchor 0's own best box is box 1 ...
    assert np.argmax(ov[0]) == 0 and np.argmax(ov[1]) == 1    # ... which claims anchor 1, while box 0 claims anchor 0
    assert m[0] == 0 and cls[0] == 3 and m[1] == 1 and cls[1] == 5


def _cond_g(case):
    ov, (cls, loc, sc, bb, m) = _ov(case), reference(case)
    assert ov.max() == F(1.0 / 64) < F(case.low)              # smaller than every anchor
    assert m[0] == 0 and cls[0] == 7 and sc[0] == F(1.0 / 64) and (m[1:] == -1).all()


def _cond_h(case):
    ov, (cls, loc, sc, bb, m) = _ov(case), reference(case)
    assert (ov[1] == 0).all() and ov[0, 0] == 0
    assert m[0] == 1 and cls[0] == 5 and sc[0] == 0 and m[3] == 0


def _cond_i(case):
    tab = table(case)
    assert tab.ymin[0] == tab.lo_y[0] == F(-0.25) and tab.ymax[1] == tab.hi_y[1] == F(1.25)
    ins = tab.inside()
    assert ins[0] and not ins[1]                              # >= on the minimum side, < on the maximum side
    cls, loc, sc, bb, m = reference(case)
    assert cls[0] == 3 and cls[1] == 0 and sc[1] == 0
    free = overlap_matrix(case.gbboxes[0], tab, mut=('no_inside',))
    assert free[0, 1] > F(case.high)                          # only the mask keeps anchor 1 out


def _cond_j(case):
    assert case.glabels[0].tolist() == [3, 5, 0, 0] and case.gbboxes[0, 2:].any()     # garbage behind the present rows
    cls, loc, sc, bb, m = reference(case)
    assert m[0] == -1 and sc[0] == 0 and m[1] == 0 and m[2] == 1


def _cond_k(case):
    assert case.glabels.shape[1] == RON_MAX_GT and (case.glabels != 0).all()
    cls, loc, sc, bb, m = reference(case)
    assert (cls > 0).any()


def _cond_l(case):
    assert case.gbboxes[0, 0, 0] == case.gbboxes[0, 0, 2]      # zero height in row 0
    cls, loc, sc, bb, m = reference(case)
    assert np.isnan(loc[m < 0, 3]).all() and (m < 0).any() and np.isneginf(loc[m == 0, 3]).all()
    assert not np.isnan(loc[:, :3]).any()


def _cond_m(case):
    assert not case.glabels.any()
    cls, loc, sc, bb, m = reference(case)
    assert not cls.any() and not loc.any() and not sc.any()


def _cond_n(case):
    for i in range(case.glabels.shape[0]):
        cls = reference(case, image=i)[0]
        assert (cls > 0).any() and (cls == 0).any() and (cls == -1).any()


def ron320_anchors():
    g = np.load(os.path.join(GOLDEN, 'g1_anchors_ron320.npz'))
    return [(g['y%d' % i], g['x%d' % i], g['h%d' % i], g['w%d' % i]) for i in range(4)]


RON_BORDERS = [32, 16, 8, 4]


def random_ground_truth(seed, n, g, counts=None, lo=0.08, hi=0.6):
    """Padded ground truth: image i holds counts[i] boxes of side lo .. hi inside the unit square (labels 1 .. 20)."""
    rs = np.random.RandomState(seed)
    counts = counts if counts is not None else [g] * n
    gl = np.zeros((n, g), np.int32)
    gb = np.zeros((n, g, 4), F)
    for i, k in enumerate(counts):
        h, w = rs.uniform(lo, hi, k), rs.uniform(lo, hi, k)
        y0, x0 = rs.uniform(0, 1 - h), rs.uniform(0, 1 - w)
        gl[i, :k] = rs.randint(1, 21, k)
        gb[i, :k] = np.stack([y0, x0, y0 + h, x0 + w], axis=-1).astype(F)
    return gl, gb


def encode_cases():
    two = lambda a, b: [a, b]
    cases = [
        _case('a_equal_high_stays_matched', two(cell(0.25, 0.125, 0.5, 0.25), cell(0.25, 0.25, 0.5, 0.5)),
              [3], [[0, 0, 0.5, 0.25]], _cond_a, catches=('high_strict',)),
        _case('b_equal_low_is_ignored', two(cell(0.125, 0.125, 0.25, 0.25), cell(0.25, 0.25, 0.5, 0.5)),
              [3], [[0, 0, 0.25, 0.25]], _cond_b, low=0.25),
        _case('c_two_boxes_tie_on_an_anchor', two(grid_layer([0.25], [0.125, 0.375], [0.5], [0.25]), cell(0.25, 0.25, 0.5, 0.5)),
              [3, 5], [[0, 0, 0.5, 0.25], [0, 0.25, 0.5, 0.5]], _cond_c, catches=('last_gt',)),
        _case('d_two_anchors_tie_for_a_box', [grid_layer([0.5], [0.25, 0.75], [1.0], [0.5])],
              [3], [[0, 0.25, 1, 0.75]], _cond_d, catches=('last_anchor', 'no_claims')),
        _case('e_two_boxes_claim_one_anchor', [grid_layer([0.25, 0.75], [0.25, 0.75], [0.5], [0.5])],
              [3, 5], [[0, 0, 0.25, 0.25], [0, 0, 0.5, 0.25]], _cond_e, catches=('no_claims',)),
        _case('f_claim_against_the_anchors_best_box', two(cell(0.25, 0.25, 0.5, 0.5), cell(0.25, 0.5, 0.5, 1.0)),
              [3, 5], [[0, 0, 0.25, 0.25], [0, 0, 0.5, 1.0]], _cond_f, catches=('no_claims',)),
        _case('g_box_smaller_than_every_anchor', QUADS, [7], [[0.0625, 0.0625, 0.125, 0.125]], _cond_g, catches=('no_claims',)),
        _case('h_box_overlapping_nothing_claims_anchor_0', QUADS, [3, 5], [[0.5, 0.5, 1, 1], [2, 2, 3, 3]], _cond_h,
              catches=('no_claims',)),
        _case('i_anchor_on_the_inside_bounds', [grid_layer([0.25, 0.75], [0.5], [1.0], [0.5])],
              [3], [[0, 0.25, 1, 0.75]], _cond_i, catches=('no_inside', 'le_max')),
        _case('j_padding_rows_behind_the_present_ones', QUADS, [3, 5], [[0, 0.5, 0.5, 1], [0.5, 0, 1, 0.5], [0, 0, 0.5, 0.5], [0, 0, 0.5, 0.5]],
              _cond_j, catches=('keep_padding',), g=4),
        _case('l_zero_height_box_in_row_0', QUADS, [2, 5], [[0.25, 0, 0.25, 0.5], [0.5, 0.5, 1, 1]], _cond_l),
        _case('m_image_without_a_box', QUADS, [0, 0], [[0, 0, 0, 0], [0, 0, 0, 0]], _cond_m),
    ]
    gl, gb = random_ground_truth(11, 1, RON_MAX_GT, lo=0.05, hi=0.5)
    cases.append(EncodeCase('k_max_gt', [grid_layer(np.arange(8) / 8. + 0.0625, np.arange(8) / 8. + 0.0625, [0.125, 0.25], [0.125, 0.25])],
                            [BORDER], IMG, gl, gb, 0.3, 0.5, _cond_k, ()))
    gl, gb = random_ground_truth(5, 4, 7, counts=[1, 7, 3, 5])
    cases.append(EncodeCase('n_ron320_anchors_random_boxes', ron320_anchors(), RON_BORDERS, (320, 320), gl, gb, 0.3, 0.5, _cond_n, ()))
    return cases


# ------------------------------------------------------------------------------------------------------------ loss cases
LossCase = collections.namedtuple('LossCase', 'name logits localisations objness_logits objness_pred gclasses glocalisations '
                                              'rand_objness rand_cls kwargs condition')
LOSS_SHAPES = [(2, 2, 2), (3, 3, 2)]            # 26 anchors per image
NUM_CLASSES = 21


def loss_inputs(seed, n=2, shapes=LOSS_SHAPES, scale=1.0):
    """Seeded per-layer tensors [N, H, W, A, *] and flat random draws; classes ~ 20 % positive, 10 % ignored."""
    rs = np.random.RandomState(seed)
    d = dict(logits=[], localisations=[], objness_logits=[], objness_pred=[], gclasses=[], glocalisations=[])
    rows = 0
    for (h, w, a) in shapes:
        shp = (n, h, w, a)
        d['logits'].append((rs.randn(*shp + (NUM_CLASSES,)) * scale).astype(F))
        d['localisations'].append(rs.randn(*shp + (4,)).astype(F))
        d['objness_logits'].append((rs.randn(*shp + (2,)) * scale).astype(F))
        d['objness_pred'].append(rs.uniform(0, 1, shp + (1,)).astype(F))
        u = rs.uniform(0, 1, shp)
        d['gclasses'].append(np.where(u < 0.2, rs.randint(1, NUM_CLASSES, shp), np.where(u < 0.3, -1, 0)).astype(np.int64))
        d['glocalisations'].append((rs.randn(*shp + (4,)) * 0.5).astype(F))
        rows += int(np.prod(shp))
    d['rand_objness'] = rs.uniform(0, 1, rows).astype(F)
    d['rand_cls'] = rs.uniform(0, 1, rows).astype(F)
    return d


def _flat(per_layer):
    return np.concatenate([t.reshape(-1) for t in per_layer])


def loss_case_masks(c):
    return loss_masks(_flat(c.gclasses), _flat(c.objness_pred), c.rand_objness, c.rand_cls,
                      c.kwargs.get('objness_threshold', 0.03), c.kwargs.get('negative_ratio', 3.))


def _lcase(name, d, condition, **kwargs):
    return LossCase(name, d['logits'], d['localisations'], d['objness_logits'], d['objness_pred'], d['gclasses'],
                    d['glocalisations'], d['rand_objness'], d['rand_cls'], kwargs, condition)


def loss_cases():
    cases = []

    d = loss_inputs(1)
    d['gclasses'] = [np.minimum(g, 0) for g in d['gclasses']]
    cases.append(_lcase('no_positive', d, lambda c, mk: _assert(mk['counts'][0] == 0 and mk['counts'][1] > 0)))

    d = loss_inputs(2)
    d['objness_pred'] = [np.where((g > 0)[..., None], F(0.01), p) for g, p in zip(d['gclasses'], d['objness_pred'])]
    cases.append(_lcase('no_positive_above_the_objectness_threshold', d, lambda c, mk: _assert(
        mk['counts'][0] > 0 and mk['counts'][2] == 0 and mk['counts'][3] > 0 and not mk['cls_set'][mk['pos']].any())))

    d = loss_inputs(3)
    d['objness_pred'] = [np.full_like(p, 0.01) for p in d['objness_pred']]
    cases.append(_lcase('empty_class_set_is_nan', d, lambda c, mk: _assert(mk['counts'][0] > 0 and mk['counts'][5] == 0)))

    d = loss_inputs(4)
    d['gclasses'] = [np.where(g == 0, np.where(np.arange(g.size).reshape(g.shape) % 3 == 0, 0, 4), g) for g in d['gclasses']]
    cases.append(_lcase('every_negative_selected', d, lambda c, mk: _assert(
        3 * mk['counts'][0] > mk['counts'][1] > 0 and mk['p_obj'] == 1 and mk['obj_set'][mk['neg']].all())))

    d = loss_inputs(5, n=1, shapes=[(1, 1, 2), (1, 3, 2)])          # 8 rows: one positive, four negatives, three ignored
    flat = np.array([5, 0, 0, 0, 0, -1, -1, -1], np.int64)
    d['gclasses'] = [flat[:2].reshape(1, 1, 1, 2), flat[2:].reshape(1, 1, 3, 2)]
    d['rand_objness'] = np.array([0.9, 0.75, 0.7499, 0.1, 0.8, 0.0, 0.0, 0.0], F)
    d['objness_pred'] = [np.full((1, 1, 1, 2, 1), 0.5, F), np.full((1, 1, 3, 2, 1), 0.5, F)]
    d['rand_cls'] = np.array([0.9, 0.75, 0.5, 0.74, 0.99, 0.0, 0.0, 0.0], F)
    cases.append(_lcase('random_value_equal_to_p_and_ignored_rows', d, lambda c, mk: _assert(
        mk['p_obj'] == F(0.75) and c.rand_objness[1] == mk['p_obj'] and not mk['obj_set'][1] and mk['obj_set'][2]
        and mk['p_cls'] == F(0.75) and not mk['cls_set'][1] and mk['cls_set'][2]
        and not mk['obj_set'][5:].any() and not mk['cls_set'][5:].any() and (c.rand_objness[5:] == 0).all())))

    d = loss_inputs(6, scale=45.0)
    cases.append(_lcase('large_logits', d, lambda c, mk: _assert(mk['counts'][5] > 0 and _expf_overflows(max(t.max() for t in c.logits)))))

    d = loss_inputs(7)
    d['glocalisations'] = [np.zeros_like(t) for t in d['glocalisations']]
    d['localisations'] = [np.where(np.arange(t.size).reshape(t.shape) % 2 == 0, F(1) / F(9), -(F(1) / F(9))).astype(F)
                          for t in d['localisations']]
    d['objness_pred'] = [np.full_like(p, 0.5) for p in d['objness_pred']]
    cases.append(_lcase('difference_exactly_one_ninth', d, lambda c, mk: _assert(
        mk['counts'][2] > 0 and all((np.abs(a - b) == F(1) / F(9)).all() for a, b in zip(c.localisations, c.glocalisations)))))
    return cases


def _expf_overflows(v):
    with np.errstate(over='ignore'):
        return bool(np.isinf(np.exp(F(v))))


def _assert(cond):
    assert cond
    return True
