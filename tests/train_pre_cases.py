"""Hand-built decision-point cases of ron_preprocess_for_train (CPU data only; the GPU tests run the same cases).

Geometry cases fix the draws of the slots they need (everything else is seeded noise) on small images whose sizes make the
coordinates that matter exact.  Every case carries `condition`, a function that asserts on the vectorised reference's own trace that
the case really sits where its name says, and `catches`, the mutants of tests/train_pre_ref.py it must tell from the reference.
Pixel cases give the geometry row directly.
"""
import collections

import numpy as np

from train_pre_ref import (F, MEANS, RON_TRAIN_DRAWS, RON_TRAIN_GEOM, canvas_fill, geometry_np, int_draw, pixels_ref,
                           size_draw)

GeomCase = collections.namedtuple('GeomCase', 'name h w glabels gbboxes draws condition catches')
PixelCase = collections.namedtuple('PixelCase', 'name images geom out_shape condition catches')

BELOW_ONE = np.nextafter(F(1), F(0))


# ------------------------------------------------------------------------------------------------------------ draw helpers
def noise(seed):
    d = np.random.RandomState(seed).uniform(0, 1, RON_TRAIN_DRAWS).astype(F)
    return np.minimum(d, BELOW_ONE)


def u_size(target, size):
    """A draw whose size_draw(u, size) truncates to `target` (aimed at target + 0.5)."""
    u = F(((target + 0.5) / size - 0.1) / 0.899)
    assert 0 <= u < 1 and int(size_draw(u, size)) == target, (target, size)
    return u


def u_int(v, m):
    """A draw whose int_draw(u, m) is v."""
    u = F((v + 0.5) / m)
    assert 0 <= u < 1 and int_draw(u, m) == v, (v, m)
    return u


def set_roi(d, o, c, H, W, y, x, sh, sw):
    """Attempt (o, c): the first size try gives (sw, sh) - which must pass the aspect test - and the roi lands at (y, x)."""
    base = 5 + (o * 10 + c) * 12
    d[base], d[base + 1] = u_size(sw, W), u_size(sh, H)
    fw, fh = size_draw(d[base], W), size_draw(d[base + 1], H)
    assert not (fw > fh * F(2) or fh > fw * F(2))
    d[base + 10], d[base + 11] = u_int(x, W - sw), u_int(y, H - sh)


def set_every_round(d, H, W, y, x, sh, sw):
    """The same roi at attempt (o, 0) of every overlap round: whichever round is the last, the roi is this one."""
    for o in range(10):
        set_roi(d, o, 0, H, W, y, x, sh, sw)


def _gt(labels, boxes, g=None):
    g = g or len(labels)
    gl, gb = np.zeros(g, np.int32), np.zeros((g, 4), F)
    gl[:len(labels)] = labels
    gb[:len(boxes)] = np.asarray(boxes, F).reshape(-1, 4)
    return gl, gb


def reference(case, mut=()):
    return geometry_np(case.h, case.w, case.glabels, case.gbboxes, case.draws, mut=mut)


def same_result(a, b):
    return (np.array_equal(a['geom'][:10], b['geom'][:10]) and np.array_equal(a['labels'], b['labels'])
            and np.array_equal(a['bboxes'], b['bboxes']) and a['count'] == b['count'])


# ------------------------------------------------------------------------------------------------------------ conditions
def _cond_a(case, r):
    assert case.draws[0] == F(0.5) and case.draws[4] == F(0.5)
    assert r['geom'][0] == 1 and r['geom'][9] == 0                       # 0.5 is not < 0.5: expand, no flip
    assert tuple(r['geom'][1:3]) == (2 * case.h, 2 * case.w)


def _cond_b(case, r):
    a0, a1 = r['trace']['attempts'][:2]
    assert a0['cen_y'][0] == a0['roi'][0] and a0['roi'][1] < a0['cen_x'][0] < a0['roi'][3]      # on the top edge, inside sideways
    assert not a0['mask'].any() and a1['mask'].all() and (a1['o'], a1['c']) == (0, 1)
    assert r['trace']['outer'] == 1 and r['count'] == 1


def _cond_c(case, r):
    t = r['trace']
    assert t['final_jaccard'][0] == t['min_iou'] == F(0.5)               # equal: not below, the loop ends
    assert t['outer'] == 1 and len(t['attempts']) == 1 and r['count'] == 1
    assert t['window'] == [0, 0, 8, 8]


def _cond_d(case, r):
    a0 = r['trace']['attempts'][0]
    assert a0['sw'] == a0['sh'] * F(2) and a0['tries'] == 1              # exactly 2: not greater, accepted at the first try
    assert a0['mask'].all()


def _cond_e(case, r):
    a0 = r['trace']['attempts'][0]
    base = 5
    fifth = size_draw(case.draws[base + 8], 2 * case.w if r['geom'][0] else case.w)
    assert a0['tries'] == 5 and a0['sw'] > a0['sh'] * F(2)               # still too wide, taken anyway
    assert a0['sw'] == fifth and a0['isw'] == int(fifth)
    assert len({int(size_draw(case.draws[base + 2 * t], case.w)) for t in (0, 1, 2, 4)}) == 4      # the tries are told apart
    assert a0['mask'].all()


def _cond_f(case, r):
    t = r['trace']
    assert len(t['attempts']) == 10 and [a['c'] for a in t['attempts']] == list(range(10))
    assert not any(a['mask'].any() for a in t['attempts'])
    assert t['outer'] == 1                                               # an empty kept set ends the overlap loop
    assert t['window'] == [0, 0, case.h, case.w] and r['count'] == 1


def _cond_g(case, r):
    t = r['trace']
    assert t['outer'] == 10 and len(t['attempts']) == 10 and all(a['c'] == 0 and a['mask'].all() for a in t['attempts'])
    assert t['final_jaccard'][0] < t['min_iou'] == F(0.9)                # the overlap condition still fails ...
    assert t['window'] == [4, 4, 24, 24] and r['count'] == 1             # ... and the roi is used all the same


def _cond_h1(case, r):
    t = r['trace']
    assert t['raw'][0] == 7 and t['window'][0] == 6                      # fl(fl(7 / 23) * 23) < 7
    assert r['count'] == 1 and not t['unchanged']


def _cond_h2(case, r):
    t = r['trace']
    assert t['raw'][2] == 2 and t['window'][2] == 1                      # fl((fl(3 / 13) - fl(1 / 13)) * 13) < 2
    assert r['count'] == 1 and not t['unchanged']


def _cond_i(case, r):
    t = r['trace']
    u = t['unclipped'][0]
    assert u[0] < 0 and u[1] < 0 and u[2] > t['window'][2] and u[3] > t['window'][3]
    assert r['geom'][9] == 0 and np.array_equal(r['bboxes'][0], np.array([0, 0, 1, 1], F))


def _cond_j(case, r):
    a = r['trace']['attempts'][-1]
    assert case.glabels.tolist() == [3, 0, 0] and not case.gbboxes[1:].any()
    pad_y, pad_x = F(r['geom'][3]) / F(r['geom'][1]), F(r['geom'][4]) / F(r['geom'][2])       # where a zero box lands on the canvas
    assert r['geom'][0] == 1 and a['roi'][0] < pad_y < a['roi'][2] and a['roi'][1] < pad_x < a['roi'][3]
    assert r['count'] == 1 and r['labels'].tolist() == [3, 0, 0] and not r['bboxes'][1:].any()
    assert reference(case, mut=('keep_padding',))['count'] == 3


def _cond_k(case, r):
    assert case.glabels.size == 1 and case.glabels[0] != 0 and r['count'] == 1


def _cond_l(case, r):
    t = r['trace']
    assert case.w < 10 and len(t['attempts']) == 10 and all(a['isw'] == 0 and a['tries'] == 5 for a in t['attempts'])
    assert all(a['roi'][1] == a['roi'][3] and not a['mask'].any() for a in t['attempts'])
    assert t['window'] == [0, 0, case.h, case.w] and r['count'] == 2


def _cond_l2(case, r):
    t = r['trace']
    assert t['attempts'][-1]['mask'].all() and t['raw'][3] == 1 and t['window'][3] == 0        # a kept box, a window of width 0
    assert t['unchanged'] and tuple(r['geom'][5:9]) == (0, 0, case.h, case.w)
    assert r['geom'][9] == 0 and np.array_equal(r['bboxes'], case.gbboxes) and r['count'] == 2


def _cond_m(case, r):
    d, g, a0 = case.draws, r['geom'], r['trace']['attempts'][0]
    assert d[0] == d[2] == d[3] == BELOW_ONE and d[1] == 0 and d[4] == 0
    assert g[0] == 1 and g[4] == 0 and g[3] == case.h - 1 and g[10] == 5 and g[9] == 1
    assert d[5 + 10] == 0 and d[5 + 11] == BELOW_ONE
    assert a0['x'] == 0 and a0['y'] == 2 * case.h - a0['ish'] - 1


def geometry_cases():
    cases = []

    def add(name, h, w, labels, boxes, d, cond, catches=(), g=None):
        gl, gb = _gt(labels, boxes, g)
        cases.append(GeomCase(name, h, w, gl, gb, d, cond, tuple(catches)))

    d = noise(1)
    d[0], d[4] = 0.5, 0.5
    add('a_expand_and_flip_draws_equal_to_one_half', 16, 16, [3], [[0.25, 0.25, 0.75, 0.75]], d, _cond_a, ('le_expand', 'le_flip'))

    d = noise(2)
    d[0], d[3], d[4] = 0.0, 0.0, 0.9
    set_roi(d, 0, 0, 16, 16, 4, 4, 8, 8)
    set_roi(d, 0, 1, 16, 16, 0, 4, 8, 8)
    add('b_centre_on_the_roi_edge_is_outside', 16, 16, [3], [[0.0625, 0.3125, 0.4375, 0.6875]], d, _cond_b, ('le_center',))

    d = noise(3)
    d[0], d[3], d[4] = 0.0, 0.25, 0.9
    set_roi(d, 0, 0, 16, 16, 0, 0, 8, 8)
    for o in range(1, 10):
        set_roi(d, o, 0, 16, 16, 0, 0, 12, 12)
    add('c_jaccard_equal_to_min_iou_is_accepted', 16, 16, [3], [[0, 0, 0.25, 0.5]], d, _cond_c, ('le_iou',))

    d = noise(4)
    d[0], d[3], d[4] = 0.0, 0.0, 0.9
    for o in range(10):
        base = 5 + o * 120
        d[base:base + 4] = [0.5, 0.5, 0.3, 0.6]
        d[base + 10], d[base + 11] = 0.0, 0.0
    add('d_aspect_exactly_two_is_accepted', 16, 32, [3], [[0.1, 0.1, 0.4, 0.4]], d, _cond_d, ('ge_aspect',))

    d = noise(5)
    d[0], d[3], d[4] = 0.0, 0.0, 0.9
    for o in range(10):
        base = 5 + o * 120
        for t in range(5):
            d[base + 2 * t], d[base + 2 * t + 1] = 0.95 - 0.05 * t, 0.0
        d[base + 10], d[base + 11] = 0.0, u_int(8, 15)
    add('e_aspect_failing_five_times_takes_the_fifth', 16, 16, [3], [[0.43, 0.2, 0.63, 0.8]], d, _cond_e)

    d = noise(6)
    d[0], d[4] = 0.0, 0.9
    for c in range(10):
        set_roi(d, 0, c, 16, 16, 0, 0, 8, 8)
    add('f_ten_attempts_without_a_centre_keep_the_whole_image', 16, 16, [3], [[0.9, 0.9, 1.0, 1.0]], d, _cond_f)

    d = noise(7)
    d[0], d[3], d[4] = 0.0, 0.95, 0.9
    set_every_round(d, 32, 32, 4, 4, 24, 24)
    add('g_ten_rounds_under_min_iou_still_use_the_roi', 32, 32, [3], [[0.4, 0.4, 0.6, 0.6]], d, _cond_g)

    d = noise(8)
    d[0], d[4] = 0.0, 0.9
    set_every_round(d, 23, 23, 7, 0, 8, 12)
    add('h1_crop_y_truncates_below_y', 23, 23, [3], [[0.4, 0.1, 0.6, 0.4]], d, _cond_h1, ('raw_window',))

    d = noise(9)
    d[0], d[4] = 0.0, 0.9
    set_every_round(d, 13, 13, 1, 2, 2, 3)
    add('h2_crop_h_truncates_below_sh', 13, 13, [3], [[0.1, 0.2, 0.2, 0.34]], d, _cond_h2, ('raw_window',))

    d = noise(10)
    d[0], d[4] = 0.0, 0.9
    set_every_round(d, 32, 32, 8, 8, 16, 16)
    add('i_box_clipped_on_every_side', 32, 32, [3], [[0.1, 0.1, 0.9, 0.9]], d, _cond_i)

    d = noise(11)
    d[0], d[1], d[2], d[4] = 0.9, u_int(4, 16), u_int(4, 16), 0.9
    set_every_round(d, 32, 32, 2, 2, 16, 16)
    add('j_padding_rows_whose_zero_boxes_would_match', 16, 16, [3], [[0.25, 0.25, 0.75, 0.75]], d, _cond_j, ('keep_padding',), g=3)

    d = noise(12)
    d[0] = 0.0
    set_every_round(d, 20, 20, 2, 2, 14, 14)
    add('k_single_present_box', 20, 20, [7], [[0.3, 0.3, 0.7, 0.7]], d, _cond_k, ('sequential_draws', 'zero_trip'))

    d = noise(13)
    d[0], d[4] = 0.0, 0.2
    for c in range(10):
        base = 5 + c * 12
        for t in range(5):
            d[base + 2 * t], d[base + 2 * t + 1] = 0.0, 0.5
    add('l_narrow_image_sampled_width_zero', 20, 7, [3, 5], [[0.1, 0.1, 0.5, 0.6], [0.4, 0.3, 0.9, 0.9]], d, _cond_l)

    d = noise(14)
    d[0], d[4] = 0.0, 0.9
    set_every_round(d, 7, 7, 2, 2, 2, 1)
    add('l2_window_of_width_zero_passes_unchanged', 7, 7, [3, 5], [[0.33, 0.3, 0.53, 0.41], [0.31, 0.29, 0.55, 0.42]], d, _cond_l2,
        ('raw_window',))

    d = noise(15)
    d[0], d[1], d[2], d[3], d[4] = BELOW_ONE, 0.0, BELOW_ONE, BELOW_ONE, 0.0
    d[5 + 10], d[5 + 11] = 0.0, BELOW_ONE
    add('m_draws_at_zero_and_just_below_one', 5, 7, [3], [[0.2, 0.2, 0.8, 0.8]], d, _cond_m)
    return cases


def random_images(seed, n, g_choices=(1, 3, 64), lo=(7, 9), hi=(64, 48)):
    """Seeded geometry inputs: n images of lo .. hi pixels with 0 .. G present rows: (hw, G, labels [G], boxes [G, 4], draws) each."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = int(rs.randint(lo[0], hi[0] + 1)), int(rs.randint(lo[1], hi[1] + 1))
        g = int(g_choices[i % len(g_choices)])
        k = int(rs.randint(0, g + 1))
        bh, bw = rs.uniform(0.05, 0.9, k), rs.uniform(0.05, 0.9, k)
        y0, x0 = rs.uniform(0, 1 - bh), rs.uniform(0, 1 - bw)
        gl, gb = np.zeros(g, np.int32), np.zeros((g, 4), F)
        gl[:k] = rs.randint(1, 21, k)
        gb[:k] = np.stack([y0, x0, y0 + bh, x0 + bw], axis=-1).astype(F)
        d = np.minimum(rs.uniform(0, 1, RON_TRAIN_DRAWS).astype(F), BELOW_ONE)
        out.append((h, w, g, gl, gb, d))
    return out


# ------------------------------------------------------------------------------------------------------------ pixel cases
def geom_row(h, w, expanded=False, img=(0, 0), crop=None, flip=False):
    H, W = (2 * h, 2 * w) if expanded else (h, w)
    cy, cx, ch, cw = crop if crop is not None else (0, 0, H, W)
    assert 0 <= cy and 0 <= cx and ch >= 1 and cw >= 1 and cy + ch <= H and cx + cw <= W
    assert (0 <= img[0] < h and 0 <= img[1] < w) if expanded else img == (0, 0)
    row = np.zeros(RON_TRAIN_GEOM, np.int32)
    row[:10] = [int(expanded), H, W, img[0], img[1], cy, cx, ch, cw, int(flip)]
    return row


def random_image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _pcond_flip_order(case):
    ref = pixels_ref(case.images[0], case.geom[0], case.out_shape) + np.asarray(MEANS, F)
    other = pixels_ref(case.images[0], case.geom[0], case.out_shape, mut=('resize_before_flip',)) + np.asarray(MEANS, F)
    assert np.abs(ref[0, :, 0] - np.array([90, 30.000002, 6.6666675])).max() < 1e-4          # flipped, then resized
    assert np.abs(other[0, :, 0] - np.array([63.333332, 16.666668, 0])).max() < 1e-4         # the other way round


def _pcond_window_over_fill(case):
    img, g = case.images[0], case.geom[0]
    h, w = img.shape[:2]
    assert g[0] == 1 and g[5] < g[3] and g[6] < g[4] and g[5] + g[7] > g[3] and g[6] + g[8] > g[4]   # starts in the fill, ends in the image
    assert g[5] + g[7] < g[3] + h or g[6] + g[8] < g[4] + w
    fill = canvas_fill(img)
    assert len(set(fill.tolist())) == 3                                  # three different channel means


def _pcond_rounding(case):
    a = pixels_ref(case.images[0], case.geom[0], case.out_shape)
    b = pixels_ref(case.images[0], case.geom[0], case.out_shape, mut=('whiten_first',))
    assert not np.array_equal(a, b) and np.abs(a - b).max() < 1e-3       # the same picture, rounded differently


def pixel_cases():
    row = np.zeros((1, 5, 3), np.uint8)
    row[0, :, :] = np.array([0, 10, 20, 50, 90], np.uint8)[:, None]
    return [
        PixelCase('p_flip_comes_before_the_resize', [row], np.stack([geom_row(1, 5, flip=True)]), (1, 3), _pcond_flip_order,
                  ('resize_before_flip',)),
        PixelCase('q_window_across_fill_and_image', [random_image(21, 6, 8)],
                  np.stack([geom_row(6, 8, expanded=True, img=(3, 5), crop=(1, 2, 7, 9))]), (16, 16), _pcond_window_over_fill, ()),
        PixelCase('r_scaled_to_one_before_interpolating', [random_image(22, 9, 11)], np.stack([geom_row(9, 11, flip=True)]), (16, 16),
                  _pcond_rounding, ('whiten_first',)),
    ]


def pixel_batches():
    """Ragged batches of three images between 5 x 7 and 33 x 21 for the two output shapes: plain, flip, expand with a window across
    the fill, crop, and all of them combined."""
    sizes = [(5, 7), (33, 21), (12, 19)]
    imgs = [random_image(30 + i, h, w) for i, (h, w) in enumerate(sizes)]
    kinds = {
        'plain': [geom_row(h, w) for h, w in sizes],
        'flip': [geom_row(h, w, flip=True) for h, w in sizes],
        'expand_window_across_fill': [geom_row(5, 7, True, (2, 3), (0, 1, 6, 8)), geom_row(33, 21, True, (20, 11), (10, 5, 40, 30)),
                                      geom_row(12, 19, True, (0, 18), (3, 9, 20, 29))],
        'crop': [geom_row(5, 7, crop=(1, 2, 3, 4)), geom_row(33, 21, crop=(6, 0, 27, 20)), geom_row(12, 19, crop=(11, 18, 1, 1))],
        'combined': [geom_row(5, 7, True, (4, 6), (2, 1, 8, 13), True), geom_row(33, 21, True, (1, 0), (0, 0, 66, 42), True),
                     geom_row(12, 19, crop=(2, 3, 9, 15), flip=True)],
    }
    return [(name, imgs, np.stack(rows), out) for name, rows in kinds.items() for out in ((16, 16), (20, 12))]
