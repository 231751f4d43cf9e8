"""Cases of the SSD losses (ron_ssd_losses / ron_ssd_losses_grad): hand cases at the decision points, layout cases, value-range
cases.  No GPU.

A case holds per-layer tensors as SSDNet.losses takes them ([N, H, 1, 1, *]: the flattening (layer, image, row, column, anchor) of
such a layer is a plain reshape) and the mode.  Hand cases are implementation-independent: any two candidate rows of a segment have
bit-identical logits or float64 background probabilities more than 1e-5 apart relative (`assert_separated`, checked when the case
is built), far above the float32 softmax's error, so the float64 reference's selection is the only right one."""
import collections

import numpy as np

import ssd_loss_ref as sr

F = np.float32
Case = collections.namedtuple('Case', ['name', 'mining', 'N', 'logits', 'localisations', 'gclasses', 'glocalisations', 'gscores',
                                       'kwargs', 'expect'])
UP = lambda v: np.nextafter(F(v), F(np.inf))
DOWN = lambda v: np.nextafter(F(v), F(-np.inf))
IGN = -1.0                       # a score of an ignored row


def flat_inputs(case):
    """The arguments of ssd_loss_ref's functions."""
    C = case.logits[0].shape[-1]
    cat = lambda lst, w: np.concatenate([np.asarray(t).reshape((-1, w) if w else (-1,)) for t in lst])
    d = dict(x=cat(case.logits, C), loc=cat(case.localisations, 4), g=cat(case.gclasses, 0), gloc=cat(case.glocalisations, 4),
             s=cat(case.gscores, 0), layer_rows=[int(np.asarray(t).size) for t in case.gclasses], N=case.N, mining=case.mining)
    d.update(case.kwargs)
    return d


def assert_separated(case):
    fi = flat_inputs(case)
    pos, cand = sr.row_sets(fi['s'], fi.get('match_threshold', 0.5))
    p0 = sr.softmax64(fi['x'])[:, 0]
    for lo, hi in sr.segments(fi['layer_rows'], case.mining):
        idx = np.nonzero(cand[lo:hi])[0] + lo
        order = idx[np.argsort(p0[idx], kind='stable')]
        for a, b in zip(order[:-1], order[1:]):
            same = fi['x'][a].tobytes() == fi['x'][b].tobytes()
            assert same or abs(p0[b] - p0[a]) > 1e-5 * max(p0[a], p0[b]), (case.name, a, b, p0[a], p0[b])
        # ... and from the non-candidates' 1.0, unless the candidate's value is 1.0 itself
        assert all(p0[i] == 1.0 or 1.0 - p0[i] > 1e-5 for i in idx), case.name


def build(name, mining, N, layer_rows, scores, gcls, bg, C=4, loc_d=None, kwargs=None, expect=None, seed=0, check=True):
    """Rows in flattened order.  bg[r] is the row's background logit; the other logits are 0 except a per-row pattern on the last
    class (so that the class terms differ between rows); equal bg -> bit-identical rows.  loc_d [rows, 4]: localisation minus
    target (the targets are 0, so the difference is exact)."""
    rows = int(np.sum(layer_rows))
    scores, gcls, bg = np.asarray(scores, F), np.asarray(gcls, np.int64), np.asarray(bg, F)
    assert scores.shape == gcls.shape == bg.shape == (rows,), (name, rows, scores.shape, gcls.shape, bg.shape)
    x = np.zeros((rows, C), F)
    x[:, 0] = bg
    x[:, C - 1] = (bg * F(0.25)).astype(F)
    rs = np.random.RandomState(seed)
    loc = rs.uniform(-2, 2, (rows, 4)).astype(F) if loc_d is None else np.asarray(loc_d, F)
    gloc = np.zeros((rows, 4), F)
    out = dict(logits=[], localisations=[], gclasses=[], glocalisations=[], gscores=[])
    lo = 0
    for R in layer_rows:
        assert R % N == 0, (name, R, N)
        shp = (N, R // N, 1, 1)
        out['logits'].append(x[lo:lo + R].reshape(shp + (C,)))
        out['localisations'].append(loc[lo:lo + R].reshape(shp + (4,)))
        out['gclasses'].append(gcls[lo:lo + R].reshape(shp))
        out['glocalisations'].append(gloc[lo:lo + R].reshape(shp + (4,)))
        out['gscores'].append(scores[lo:lo + R].reshape(shp))
        lo += R
    case = Case(name, mining, N, kwargs=dict(kwargs or {}), expect=expect, **out)
    if check:
        assert_separated(case)
    return case


def _grid(n, lo=-3.0, step=0.37):
    """n distinct background logits, far apart."""
    return [lo + step * i for i in range(n)]


def hand_cases():
    cases = []
    # scores at the two thresholds and one ulp above: 0.5 is a candidate, 0.5+ a positive; -0.5 is ignored, -0.5+ a candidate
    sc = [0.5, UP(0.5), -0.5, UP(-0.5), 0.9, 0.0, 0.1, 0.2, 0.3, 0.4, IGN, 0.45]
    cases.append(build('scores_at_the_thresholds', 'batch', 1, [12], sc, [1, 2, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0], _grid(12),
                       expect=dict(counts=[[2, 8, 7, 6]])))
    # negative_ratio 2.5 with three positives: (int)7.5 = 7, plus N = 2; two layers under one selection
    sc = [0.9, 0.8, 0.7] + [0.1] * 13 + [0.2] * 8
    cases.append(build('ratio_2p5_three_positives', 'batch', 2, [16, 8], sc, [1, 2, 3] + [0] * 21, _grid(24),
                       kwargs=dict(negative_ratio=2.5), expect=dict(counts=[[3, 21, 9, 8]])))
    # k capped by the number of candidates
    sc = [0.9, 0.8, 0.1, 0.2, 0.3, 0.4, IGN, IGN]
    cases.append(build('k_capped_by_candidates', 'batch', 1, [8], sc, [1, 1, 0, 0, 0, 0, 0, 0], _grid(8),
                       expect=dict(counts=[[2, 4, 4, 3]])))
    # no candidate at all: k = 0, nothing mined, the negative term is 0
    cases.append(build('no_candidates', 'batch', 2, [8], [0.9, 0.8, IGN, IGN, 0.7, IGN, -0.5, IGN], [1, 2, 0, 0, 3, 0, 0, 0], _grid(8),
                       expect=dict(counts=[[3, 0, 0, 0]], neg_zero=True)))
    # LAYER, k = 1 + n_cand < R: t is a non-candidate's 1.0 and every candidate below 1 is mined
    sc = [0.9, 0.8, 0.7, 0.6] + [0.1] * 6 + [IGN] * 6
    cases.append(build('layer_k_one_plus_candidates', 'layer', 1, [16], sc, [1, 2, 3, 1] + [0] * 12, _grid(16),
                       expect=dict(counts=[[4, 6, 7, 6]])))
    # LAYER, every row a candidate: 1 + n_cand > R, k clamped to R; the largest value is t and is not mined
    cases.append(build('layer_all_candidates_k_clamped', 'layer', 4, [8], [0.1] * 8, [0] * 8, _grid(8),
                       expect=dict(counts=[[0, 8, 8, 7]])))
    # LAYER, R / 8 decides (64 / 8 = 8 > 4 N = 4 > 3 n_pos = 3); a second layer where 4 N decides (24 / 8 = 3 < 12)
    sc = [0.9] + [0.1] * 63
    cases.append(build('layer_r8_floor_decides', 'layer', 1, [64], sc, [1] + [0] * 63, _grid(64, -4.0, 0.11),
                       expect=dict(counts=[[1, 63, 8, 7]])))
    sc = [0.9] + [0.1] * 20 + [IGN] * 3
    cases.append(build('layer_4n_floor_decides', 'layer', 3, [24], sc, [1] + [0] * 23, _grid(24),
                       expect=dict(counts=[[1, 20, 12, 11]])))
    # the k-th value shared by three bit-identical rows (ranks 4, 5, 6 of k = 5): none of them is mined, n_mined = 3 < k - 1
    bg = [0.0, 0.0] + [-3.0, -2.5, -2.0] + [-1.0, -1.0, -1.0] + [0.5, 1.0, 1.5, 2.0]
    sc = [0.9, IGN] + [0.1] * 10
    cases.append(build('kth_value_tied', 'batch', 2, [12], sc, [1] + [0] * 11, bg, expect=dict(counts=[[1, 10, 5, 3]])))
    # a candidate whose background probability is exactly 1.0f: it ties with the non-candidates and is never mined
    bg = [0.0, 200.0, -1.0, -2.0, 0.5, 0.0]
    cases.append(build('candidate_p0_exactly_one', 'batch', 1, [6], [0.9, 0.1, 0.1, 0.1, 0.1, IGN], [1, 0, 0, 0, 0, 0], bg,
                       expect=dict(counts=[[1, 4, 4, 3]])))
    # a positive row labelled num_classes: NaN class term, NaN total, a NaN gradient row; the other terms stay finite
    cases.append(build('positive_label_equal_to_num_classes', 'batch', 1, [8], [0.9, 0.8] + [0.1] * 6, [4, 1] + [0] * 6, _grid(8),
                       expect=dict(counts=[[2, 6, 6, 5]], nan=(0, 3))))
    # LAYER, a layer without positives: its positive and localisation terms are 0, not NaN; its negatives are still mined
    sc = [0.9, 0.8] + [0.1] * 6 + [0.2] * 8
    cases.append(build('layer_without_positives', 'layer', 1, [8, 8], sc, [1, 2] + [0] * 14, _grid(16),
                       expect=dict(counts=[[2, 6, 6, 5], [0, 8, 4, 3]])))
    # a box's best anchor below the threshold (class > 0, score <= 0.5): a candidate, mined as background
    sc = [0.9, 0.3, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]
    cases.append(build('best_anchor_below_threshold_mined_as_background', 'batch', 1, [8], sc, [1, 3, 0, 0, 0, 0, 0, 0],
                       [0.0, -5.0] + _grid(6, -1.0), expect=dict(counts=[[1, 7, 4, 3]], mined_rows=[1])))
    # |d| = 0, 1, 1 -+ one ulp (both signs) in the localisation term; LAYER so that the term is divided by 4 n_pos
    one = F(1.0)
    d = [[0.0, one, -one, UP(one)], [DOWN(one), -UP(one), -DOWN(one), 0.5], [-0.0, 2.0, -3.0, 1e-20]]
    loc_d = np.zeros((8, 4), F)
    loc_d[:3] = np.array(d, F)
    cases.append(build('localisation_kinks', 'layer', 1, [8], [0.9, 0.8, 0.7] + [0.1] * 5, [1, 2, 3] + [0] * 5, _grid(8), loc_d=loc_d,
                       expect=dict(counts=[[3, 5, 6, 5]])))
    return cases


# the hand case that kills each mutant of ssd_loss_ref.MUTANTS
KILLS = {
    'le_threshold': 'kth_value_tied',
    'mine_k_by_index': 'ratio_2p5_three_positives',
    'kth_among_candidates': 'layer_k_one_plus_candidates',
    'no_plus_n': 'ratio_2p5_three_positives',
    'round_k': 'ratio_2p5_three_positives',
    'batch_per_layer': 'ratio_2p5_three_positives',
    'layer_over_batch': 'layer_without_positives',
    'loc_div_n_pos': 'localisation_kinks',
    'ge_match': 'scores_at_the_thresholds',
    'ignored_as_candidates': 'scores_at_the_thresholds',
    'mined_label_g': 'best_anchor_below_threshold_mined_as_background',
}


def random_case(name, mining, N, layer_rows, C, seed, pos_rate=0.02, ign_rate=0.05, kwargs=None, scale=2.0):
    """Random logits and targets; the selection is checked on the device's own values, so near-ties need no care."""
    rs = np.random.RandomState(seed)
    out = dict(logits=[], localisations=[], gclasses=[], glocalisations=[], gscores=[])
    for R in layer_rows:
        assert R % N == 0, (name, R, N)
        shp = (N, R // N, 1, 1)
        u = rs.uniform(0, 1, R)
        sc = np.where(u < pos_rate, rs.uniform(0.51, 1.0, R), np.where(u < pos_rate + ign_rate, -1.0, rs.uniform(0.0, 0.49, R))).astype(F)
        g = np.where(sc > 0.5, rs.randint(1, C, R), np.where(rs.uniform(0, 1, R) < 0.01, rs.randint(1, C, R), 0)).astype(np.int64)
        x = (rs.randn(R, C) * scale).astype(F)
        x[:, 0] += F(1.0)
        out['logits'].append(x.reshape(shp + (C,)))
        out['localisations'].append(rs.randn(R, 4).astype(F).reshape(shp + (4,)))
        out['gclasses'].append(g.reshape(shp))
        out['glocalisations'].append((rs.randn(R, 4) * 0.5).astype(F).reshape(shp + (4,)))
        out['gscores'].append(sc.reshape(shp))
    return Case(name, mining, N, kwargs=dict(kwargs or {}), expect=None, **out)


def layout_cases():
    """C in {2, 3, 21, 128}; segment row counts 2, 63, 64, 65, 255, 256, 257, 513, 4097; 1 to 7 layers; N in {1, 2, 3}; both modes."""
    shapes = [('seven_layers_c21_n1', 1, [2, 63, 64, 65, 255, 256, 257], 21),
              ('two_layers_c128_n1', 1, [513, 4097], 128),
              ('three_layers_c3_n3', 3, [63, 255, 513], 3),
              ('three_layers_c2_n2', 2, [2, 64, 256], 2),
              ('one_layer_c2_n1', 1, [2], 2)]
    cases = []
    for i, (name, N, rows, C) in enumerate(shapes):
        for mining in ('batch', 'layer'):
            cases.append(random_case('%s_%s' % (name, mining), mining, N, rows, C, seed=10 + i, pos_rate=0.05))
    return cases


def low_digit_case(mining='batch'):
    """C = 2, rows [a, 0] with a on a grid of 4096 steps inside +-2e-4: every p0 is 0.5 +- 5e-5, so the upper 16 bits are
    0x3eff below 0.5 and 0x3f00 from it on, nothing else, and the decision falls into the low radix digits; the grid is finer than
    float32 resolves there, so exact ties occur."""
    rs = np.random.RandomState(5)
    R = 4096
    a = ((rs.randint(0, 4096, R) - 2048) * (2e-4 / 2048)).astype(F)
    sc = np.where(np.arange(R) % 64 == 0, 0.9, 0.1).astype(F)
    g = (sc > 0.5).astype(np.int64)
    x = np.zeros((R, 2), F)
    x[:, 0] = a
    shp = (1, R, 1, 1)
    loc = rs.randn(R, 4).astype(F)
    return Case('low_digits_%s' % mining, mining, 1, [x.reshape(shp + (2,))], [loc.reshape(shp + (4,))], [g.reshape(shp)],
                [np.zeros(shp + (4,), F)], [sc.reshape(shp)], {}, None)


def wide_range_case(mining='batch'):
    """Background probabilities from 1e-30 to 1: the decision lies in the high digits."""
    rs = np.random.RandomState(6)
    R = 2048
    a = rs.uniform(-69.0, 12.0, R).astype(F)                   # p0 = 1 / (1 + 2 exp(-a)) with C = 3: 5e-31 .. 1 - 1e-5
    sc = np.where(np.arange(R) % 128 == 0, 0.9, 0.1).astype(F)
    g = (sc > 0.5).astype(np.int64) * 2
    x = np.zeros((R, 3), F)
    x[:, 0] = a
    shp = (2, R // 2, 1, 1)
    loc = rs.randn(R, 4).astype(F)
    return Case('wide_range_%s' % mining, mining, 2, [x.reshape(shp + (3,))], [loc.reshape(shp + (4,))], [g.reshape(shp)],
                [np.zeros(shp + (4,), F)], [sc.reshape(shp)], dict(negative_ratio=40.0), None)


def value_cases():
    return [low_digit_case('batch'), low_digit_case('layer'), wide_range_case('batch'), wide_range_case('layer')]
