"""Ground-truth matching (``ron_bboxes_matching`` = tfe.bboxes_matching_batch) at its decision points (numpy only; test infrastructure).

Ground truth plus Gaussian-jittered copies of it never put a jaccard ON the threshold, never tie two ground-truth boxes, never leave
a detection without any same-class overlap at a chosen row 0, and never present a degenerate box.  The families here do:

  A  threshold   jaccard equal to float32(threshold), one ulp above, one ulp below (0.5 is exact, 0.3 is not representable); pairs on
                 which another summation order of the union, or a fused multiply-add, decides differently (seeded search)
  B  ties        identical same-class boxes at (3,17), (63,64), (0,255), (64,128), (G-2,G-1), three chunks: the first maximum wins
  C  nothing     no same-class box / no overlap / only an other-class box overlaps: every product is 0, the argmax is row 0, and row 0
                 (other class, difficult, padding) decides fp; zero-padded detection rows go the same way
  D  state       the read-modify-write of the matched flags, one list walked through all its transitions
  E  degenerate  inverted, zero-area, NaN and infinite boxes: safe_divide's "not > 0" covers union < 0, 0 / 0 and NaN
  F  extent      the deciding box at G - 1 and at the first lane of the last 64-box chunk, G in {1, 63, 64, 65, 128, 129, 255, 256};
                 K = 1; 81 lists; difficult flags in every chunk; three images with different padding

A case is a ``MatchCase``: the dense inputs of ``metrics.bboxes_matching`` (list l holds label l + 1), the threshold, ``condition(case)``
which asserts ON THE ORACLE'S float32 arithmetic that the case sits where it claims, ``catches`` = the mutants that must change its
result, and ``expect`` = (n_gbboxes, tp, fp) written down by hand where the case was built for a stated outcome (else None).

``match_ref`` is a second reference, written from the TensorFlow text (tf_extended/bboxes.py:316-404, :527-555, math.py:25-38) and not
from ``oracle/eval_metrics.py``: the whole [K, G] jaccard matrix first, vectorised, every intermediate float32 in the reference's
order, then a scalar walk over the detections with a hand-written first-maximum search.  Every mutant is a switch of it.
"""
import collections
import functools

import numpy as np

from oracle import eval_metrics as em

F32 = np.float32
_ERR = dict(divide='ignore', invalid='ignore', over='ignore', under='ignore')
CHUNK = 64                      # ground-truth boxes per wave pass in evalmatch.hip

MatchCase = collections.namedtuple('MatchCase', 'name scores bboxes glabels gbboxes gdifficults threshold condition catches expect')

# 'mark_difficult' (a hit on a difficult box marks it) is listed because the kernel has the corresponding guard, but it is an
# EQUIVALENT mutant: the flag of a difficult box is only ever read in a step whose argmax is that box, and there `not_difficult` is
# false and gates tp and fp both.  No input can show it; tests/test_match_cases_cpu.py asserts exactly that instead of a catch.
EQUIVALENT_MUTANTS = ('mark_difficult',)
MUTANTS = ('ge_threshold', 'last_maximum', 'later_chunk_wins_tie', 'mark_below_threshold', 'mark_difficult', 'fp_ignores_difficulty',
           'tp_ignores_existing', 'existing_needs_match', 'no_label_mask', 'argmax_same_class_only', 'count_difficult', 'union_order',
           'fused_area', 'fused_inter', 'nan_propagates', 'union_ge_zero_divides')


# --------------------------------------------------------------------------- #
# second reference
# --------------------------------------------------------------------------- #
def jaccard_pairs(det, gt, mut=()):
    """float32 jaccard of det [..., 4] with gt [..., 4] (broadcast), in the order of tf_extended/bboxes.py:542-553:
    union = (-inter + gt area) + det area, safe_divide = 0 wherever the union is not > 0 (negative, zero, NaN)."""
    det, gt = np.asarray(det, F32), np.asarray(gt, F32)
    zero = F32(0)
    with np.errstate(**_ERR):
        ymin, xmin = np.maximum(gt[..., 0], det[..., 0]), np.maximum(gt[..., 1], det[..., 1])
        ymax, xmax = np.minimum(gt[..., 2], det[..., 2]), np.minimum(gt[..., 3], det[..., 3])
        h, w = np.maximum(ymax - ymin, zero), np.maximum(xmax - xmin, zero)
        inter = h * w
        gh, gw = gt[..., 2] - gt[..., 0], gt[..., 3] - gt[..., 1]
        dh, dw = det[..., 2] - det[..., 0], det[..., 3] - det[..., 1]
        garea, darea = gh * gw, dh * dw
        if 'union_order' in mut:
            union = (garea + darea) - inter
        elif 'fused_area' in mut:             # fma(dh, dw, -inter + garea): the product unrounded, ONE rounding of the sum
            union = ((-inter + garea).astype(np.float64) + dh.astype(np.float64) * dw.astype(np.float64)).astype(F32)
        elif 'fused_inter' in mut:            # fma(-h, w, garea) + darea
            union = (garea.astype(np.float64) - h.astype(np.float64) * w.astype(np.float64)).astype(F32) + darea
        else:
            union = (-inter + garea) + darea
        assert union.dtype == F32 and inter.dtype == F32
        ok = union >= zero if 'union_ge_zero_divides' in mut else union > zero
        jac = np.where(ok, inter / np.where(ok, union, F32(1)), zero)
        if 'union_ge_zero_divides' in mut:
            jac = np.where(union == zero, inter / union, jac)
        if 'nan_propagates' in mut:
            jac = np.where(np.isnan(union), F32(np.nan), jac)
    return jac.astype(F32)


def jaccard_matrix(dets, gts, mut=()):
    """[K, G]."""
    return jaccard_pairs(np.asarray(dets, F32).reshape(-1, 1, 4), np.asarray(gts, F32).reshape(1, -1, 4), mut)


def _above(a, b):
    """a > b, a NaN counting as larger than every number (numpy's argmax convention; only the mutants ever see one)."""
    return bool(a > b) or bool(a != a and b == b)


def _first_max(row):
    best = 0
    for j in range(1, len(row)):
        if _above(row[j], row[best]):
            best = j
    return best


def _pick(row, same_idx, mut):
    g = len(row)
    if 'argmax_same_class_only' in mut:
        return g - 1 if len(same_idx) == 0 else int(same_idx[_first_max(row[same_idx])])
    if 'last_maximum' in mut:
        return g - 1 - _first_max(row[::-1])
    if 'later_chunk_wins_tie' in mut:
        best = _first_max(row[:CHUNK])
        for c0 in range(CHUNK, g, CHUNK):
            j = c0 + _first_max(row[c0:c0 + CHUNK])
            if not _above(row[best], row[j]):
                best = j
        return best
    return _first_max(row)


def match_list(label, bboxes, glabels, gbboxes, gdifficults, thr, mut=()):
    """One image, one label: (n_gbboxes, tp [K], fp [K])."""
    glabels = np.asarray(glabels).reshape(-1)
    diff = np.asarray(gdifficults).reshape(-1) != 0
    same = glabels == label
    n_gb = int(np.sum(same if 'count_difficult' in mut else same & ~diff))
    jac = jaccard_matrix(bboxes, gbboxes, mut)
    if 'no_label_mask' not in mut:
        with np.errstate(**_ERR):
            jac = jac * same.astype(F32)[None]
    same_idx = np.flatnonzero(same)
    thr = F32(thr)
    k = jac.shape[0]
    marked = [False] * len(glabels)
    tp, fp = np.zeros(k, bool), np.zeros(k, bool)
    for i in range(k):
        idx = _pick(jac[i], same_idx, mut)
        best = jac[i, idx]
        match = bool(best >= thr) if 'ge_threshold' in mut else bool(best > thr)
        existing = marked[idx]
        not_diff = not diff[idx]
        tp[i] = not_diff and match and (True if 'tp_ignores_existing' in mut else not existing)
        wrong = (not match) if 'existing_needs_match' in mut else (existing or not match)
        fp[i] = wrong if 'fp_ignores_difficulty' in mut else (not_diff and wrong)
        if (not_diff or 'mark_difficult' in mut) and (match or 'mark_below_threshold' in mut):
            marked[idx] = True
    return n_gb, tp, fp


def match_ref(scores, bboxes, glabels, gbboxes, gdifficults, thr=0.5, mut=(), labels=None):
    """Dense form like metrics.bboxes_matching: (n_gbboxes [N, L] int64, tp [N, L, K] bool, fp [N, L, K] bool)."""
    n, nl, k = np.asarray(scores).shape
    labels = list(range(1, nl + 1)) if labels is None else list(labels)
    n_gb = np.zeros((n, nl), np.int64)
    tp, fp = np.zeros((n, nl, k), bool), np.zeros((n, nl, k), bool)
    for i in range(n):
        for l, c in enumerate(labels):
            n_gb[i, l], tp[i, l], fp[i, l] = match_list(c, bboxes[i, l], glabels[i], gbboxes[i], gdifficults[i], thr, mut)
    return n_gb, tp, fp


def reference(case, mut=()):
    return match_ref(case.scores, case.bboxes, case.glabels, case.gbboxes, case.gdifficults, case.threshold, mut)


def oracle_dense(scores, bboxes, glabels, gbboxes, gdifficults, thr=0.5, labels=None):
    """oracle.eval_metrics.bboxes_matching_batch, its dicts stacked to the dense form."""
    nl = scores.shape[1]
    labels = list(range(1, nl + 1)) if labels is None else list(labels)
    with np.errstate(**_ERR):
        d_n, d_tp, d_fp = em.bboxes_matching_batch(labels, {c: scores[:, l] for l, c in enumerate(labels)},
                                                   {c: bboxes[:, l] for l, c in enumerate(labels)}, glabels, gbboxes, gdifficults, thr)
    return (np.stack([d_n[c] for c in labels], 1), np.stack([d_tp[c] for c in labels], 1), np.stack([d_fp[c] for c in labels], 1))


def oracle(case):
    return oracle_dense(case.scores, case.bboxes, case.glabels, case.gbboxes, case.gdifficults, case.threshold)


def oracle_jaccard(case, img, lst):
    """[K, G]: the oracle's own jaccard rows of one list, label mask applied."""
    same = (case.glabels[img] == lst + 1).astype(F32)
    with np.errstate(**_ERR):
        return np.stack([em.jaccard(b, case.gbboxes[img]) * same for b in case.bboxes[img, lst]])


def same_result(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def ulps(a, b):
    """Signed distance a - b in float32 ulps (positive finite floats)."""
    return np.asarray(a, F32).view(np.int32).astype(np.int64) - np.asarray(b, F32).view(np.int32).astype(np.int64)


def nudge(v, k):
    """float32 v moved by k ulps (positive finite v)."""
    return (np.asarray(v, F32).view(np.int32) + np.asarray(k, np.int32)).view(F32)


# --------------------------------------------------------------------------- #
# case builder
# --------------------------------------------------------------------------- #
def det_scores(m, k):
    """m detections with scores 0.9, 0.85, ... (sorted, all above the streaming cut of 1e-4), then zero padding."""
    s = np.zeros(k, F32)
    s[:m] = F32(0.9) - np.arange(m, dtype=F32) * F32(0.05)
    return s


def build(name, images, condition, catches=(), thr=0.5, nl=2, k=8, g=None, expect=None):
    """images: one dict per image, gt = [(label, box, difficult), ...] and dets = {list index: [box, ...]}.  Padding: ground truth
    (label 0, zero box, not difficult) up to g, detections (zero box, score 0) up to k."""
    n = len(images)
    g = g or max(1, max(len(im['gt']) for im in images))
    glabels, gbboxes, gdiff = np.zeros((n, g), np.int64), np.zeros((n, g, 4), F32), np.zeros((n, g), np.int64)
    scores, bboxes = np.zeros((n, nl, k), F32), np.zeros((n, nl, k, 4), F32)
    for i, im in enumerate(images):
        assert len(im['gt']) <= g
        for j, (lab, box, d) in enumerate(im['gt']):
            glabels[i, j], gbboxes[i, j], gdiff[i, j] = lab, np.asarray(box, F32), d
        for l, boxes in im.get('dets', {}).items():
            assert l < nl and len(boxes) <= k
            scores[i, l] = det_scores(len(boxes), k)
            for j, b in enumerate(boxes):
                bboxes[i, l, j] = np.asarray(b, F32)
    assert k <= 16 and n <= 3 and (nl <= 4 or nl == 81)
    if expect is not None:
        expect = (np.asarray(expect[0], np.int64).reshape(n, nl), np.asarray(expect[1], bool).reshape(n, nl, k),
                  np.asarray(expect[2], bool).reshape(n, nl, k))
    return MatchCase(name, scores, bboxes, glabels, gbboxes, gdiff, thr, condition, tuple(catches), expect)


def _row(vals, k=8):
    """A tp / fp row of k entries: `vals`, then zeros."""
    return list(vals) + [0] * (k - len(vals))


def _check_expect(case):
    if case.expect is not None:
        got = oracle(case)
        for name, a, b in zip(('n_gbboxes', 'tp', 'fp'), got, case.expect):
            assert np.array_equal(a, b), '%s: oracle %s is %s, the case states %s' % (case.name, name, a.tolist(), b.tolist())


BOX = [0.0, 0.0, 0.5, 0.5]            # area 0.25
FAR = [0.75, 0.75, 1.0, 1.0]          # disjoint from BOX and from everything inside it


# --------------------------------------------------------------------------- #
# A. threshold
# --------------------------------------------------------------------------- #
def _cond_threshold(want):
    """The oracle's jaccard of detection 0 with ground-truth box 0 lies `want` ulps from float32(threshold)."""
    def cond(case):
        j = oracle_jaccard(case, 0, 0)[0, 0]
        assert ulps(j, F32(case.threshold)) == want, (case.name, float(j))
        _check_expect(case)
    return cond


def _threshold_case(name, gt, det, thr, want, catches=()):
    hit = want > 0
    return build(name, [dict(gt=[(1, gt, 0)], dets={0: [det]})], _cond_threshold(want), catches, thr=thr, nl=1, k=1,
                 expect=([1], [hit], [not hit]))


@functools.lru_cache(maxsize=None)
def find_at_threshold(thr, seed=0):
    """{-1, 0, +1} -> (gt, det): a detection inside its ground-truth box (jaccard ~ the ratio of the widths) whose float32 jaccard is
    that many ulps from float32(thr).  Seeded search over boxes and ulp moves of the detection's xmax."""
    rs = np.random.RandomState(300 + seed + int(thr * 1000))
    found = {}
    offs = np.arange(-40, 41)
    for _ in range(400):
        y0, x0 = F32(rs.uniform(0.05, 0.3)), F32(rs.uniform(0.05, 0.3))
        gt = np.array([y0, x0, y0 + F32(rs.uniform(0.2, 0.5)), x0 + F32(rs.uniform(0.2, 0.5))], F32)
        det = np.tile(gt[None], (offs.size, 1))
        det[:, 3] = nudge(gt[1] + F32(thr) * (gt[3] - gt[1]), offs)
        d = ulps(jaccard_pairs(det, gt[None]), F32(thr))
        for want in (-1, 0, 1):
            hit = np.flatnonzero(d == want)
            if want not in found and hit.size:
                found[want] = (gt, det[hit[0]].copy())
        if len(found) == 3:
            return found
    raise RuntimeError('find_at_threshold(%g): found only %s' % (thr, sorted(found)))


def _flip_cells(mutant, seed, n_cells=8, thr=0.5):
    """Pairs on which `mutant` decides jaccard > thr differently: gt random inside cell c of a 4 x 4 grid (pairs of different cells are
    disjoint: every other overlap is exactly 0), det = gt shifted by a third of its width (jaccard ~ 0.5), one of its coordinates
    moved by -3 .. +3 ulps.  Returns n_cells (gt, det, baseline decision) in n_cells different cells, both directions of the flip
    where the search finds them.  About 3 % of the candidates flip, so 16 x 500 x 28 of them give hundreds."""
    rs = np.random.RandomState(500 + seed)
    per_cell, m = {}, 500
    for cell in range(16):
        cy, cx = F32(cell // 4) * F32(0.25), F32(cell % 4) * F32(0.25)
        y0, x0 = (cy + rs.uniform(0.01, 0.05, m)).astype(F32), (cx + rs.uniform(0.01, 0.05, m)).astype(F32)
        h, w = rs.uniform(0.08, 0.15, m).astype(F32), rs.uniform(0.08, 0.12, m).astype(F32)
        gt = np.stack([y0, x0, y0 + h, x0 + w], 1).astype(F32)
        sh = (w / F32(3)).astype(F32)
        det = gt.copy()
        det[:, 1] += sh
        det[:, 3] += sh
        assert (det[:, 3] < cx + F32(0.25)).all() and (gt[:, 2] < cy + F32(0.25)).all()
        coord, off = rs.randint(0, 4, m), np.arange(-3, 4)
        cand_gt = np.repeat(gt, off.size, 0)
        cand_det = np.repeat(det, off.size, 0)
        rows = np.arange(cand_det.shape[0])
        cc = np.repeat(coord, off.size)
        cand_det[rows, cc] = nudge(cand_det[rows, cc], np.tile(off, m))
        base = jaccard_pairs(cand_det, cand_gt) > F32(thr)
        mutd = jaccard_pairs(cand_det, cand_gt, (mutant,)) > F32(thr)
        per_cell[cell] = [(cand_gt[i], cand_det[i], bool(base[i])) for i in np.flatnonzero(base != mutd)]
    out, want_hit = [], True
    for cell in range(16):
        if len(out) == n_cells:
            break
        flips = per_cell[cell]
        pick = [f for f in flips if f[2] == want_hit] or flips          # alternate the direction of the flip where possible
        if pick:
            out.append(pick[0])
            want_hit = not want_hit
    if len(out) < n_cells:
        raise RuntimeError('_flip_cells(%s): %d of %d cells hold a flip' % (mutant, len(out), n_cells))
    return out


def _flip_case(mutant, seed):
    """One list of 8 detections, each with its own ground-truth box in its own grid cell, each a flip under `mutant`."""
    flips = _flip_cells(mutant, seed)

    def cond(case):
        jac = oracle_jaccard(case, 0, 0)
        assert np.count_nonzero(jac) == len(flips) and (np.diag(jac) > 0).all()         # every detection sees its own box only
        base = np.diag(jac) > F32(case.threshold)
        mutd = np.diag(jaccard_matrix(case.bboxes[0, 0], case.gbboxes[0], (mutant,))) > F32(case.threshold)
        assert (base != mutd).all(), (mutant, base, mutd)
        assert np.array_equal(base, [f[2] for f in flips])
        _check_expect(case)
    hit = [f[2] for f in flips]
    return build('A/flip_%s_seed%d' % (mutant, seed), [dict(gt=[(1, f[0], 0) for f in flips], dets={0: [f[1] for f in flips]})], cond,
                 (mutant,), nl=1, k=8, expect=([8], hit, [not h for h in hit]))


def family_A():
    q = F32(0.25)
    out = [_threshold_case('A/half_exact', BOX, [0, 0, .5, q], 0.5, 0, ('ge_threshold',)),
           _threshold_case('A/half_plus_ulp', BOX, [0, 0, .5, np.nextafter(q, F32(1))], 0.5, 1),
           _threshold_case('A/half_minus_ulp', BOX, [0, 0, .5, np.nextafter(q, F32(0))], 0.5, -1)]
    for thr in (0.5, 0.3):
        found = find_at_threshold(thr)
        for want, tag in ((0, 'on'), (1, 'plus_ulp'), (-1, 'minus_ulp')):
            gt, det = found[want]
            out.append(_threshold_case('A/thr%g_%s' % (thr, tag), gt, det, thr, want, ('ge_threshold',) if want == 0 else ()))
    for mutant in ('union_order', 'fused_area', 'fused_inter'):
        for seed in (0, 1):
            out.append(_flip_case(mutant, seed))
    return out


# --------------------------------------------------------------------------- #
# B. ties
# --------------------------------------------------------------------------- #
def _tie_case(name, g, members, difficult, n_dets, expect_tp, expect_fp, catches):
    """g ground-truth boxes: `members` hold BOX with label 1 (difficult where listed), every other row holds BOX with label 2 and the
    difficult flag set (so the label mask is what keeps them out: without it row 0 wins and nothing is written).  n_dets detections
    equal to BOX: jaccard exactly 1 with every member."""
    gt = [(2, BOX, 1)] * g
    for m in members:
        gt[m] = (1, BOX, int(m in difficult))

    def cond(case):
        jac = oracle_jaccard(case, 0, 0)
        for i in range(n_dets):
            assert np.array_equal(np.flatnonzero(jac[i] == jac[i].max()), sorted(members)) and jac[i].max() == 1
        _check_expect(case)
    n_gb = len([m for m in members if m not in difficult])
    return build(name, [dict(gt=gt, dets={0: [BOX] * n_dets})], cond, catches, nl=1, k=2,
                 expect=([n_gb], _row(expect_tp, 2), _row(expect_fp, 2)))


def family_B():
    out = []
    for lo, hi, g in ((3, 17, 32), (63, 64, 65), (0, 255, 256), (64, 128, 129), (128, 129, 130), (254, 255, 256)):
        cross = ('later_chunk_wins_tie',) if lo // CHUNK != hi // CHUNK else ()
        masked = ('no_label_mask',) if lo != 0 else ()          # without the mask row 0 (label 2, difficult, jaccard 1) wins
        # the first maximum is difficult: neither tp nor fp, twice (it is never marked either)
        out.append(_tie_case('B/%d_%d_first_difficult' % (lo, hi), g, (lo, hi), (lo,), 2, [0, 0], [0, 0], ('last_maximum',) + cross))
        # the converse: tp, then the duplicate is fp (the second maximum is never looked at)
        out.append(_tie_case('B/%d_%d_second_difficult' % (lo, hi), g, (lo, hi), (hi,), 2, [1, 0], [0, 1], ('last_maximum',) + cross + masked))
    tri = (10, 70, 200)
    out.append(_tie_case('B/three_chunks_first_difficult', 256, tri, (10,), 2, [0, 0], [0, 0], ('last_maximum', 'later_chunk_wins_tie')))
    out.append(_tie_case('B/three_chunks_middle_difficult', 256, tri, (70,), 2, [1, 0], [0, 1], ('no_label_mask',)))
    out.append(_tie_case('B/three_chunks_first_only', 256, tri, (70, 200), 2, [1, 0], [0, 1], ('last_maximum', 'later_chunk_wins_tie', 'no_label_mask')))
    return out


# --------------------------------------------------------------------------- #
# C. nothing to match
# --------------------------------------------------------------------------- #
DET80 = [0.0, 0.0, 0.5, 0.4]           # inside BOX: jaccard 0.8
DET20 = [0.0, 0.0, 0.5, 0.1]           # inside BOX: jaccard 0.2


def _cond_all_zero(lists=(0,)):
    def cond(case):
        for i in range(case.scores.shape[0]):
            for l in lists:
                assert not oracle_jaccard(case, i, l).any(), (case.name, i, l)
        _check_expect(case)
    return cond


def family_C():
    out = []
    # no same-class box: ground truth of label 2 only, one of them under the detection of list 0 (label 1)
    gt = [(2, BOX, 0), (2, FAR, 0), (2, FAR, 1)]
    out.append(build('C/no_same_class', [dict(gt=gt, dets={0: [DET80]})], _cond_all_zero(), ('no_label_mask', 'argmax_same_class_only'),
                     expect=([0, 2], [_row([]), _row([])], [_row([1] * 8), _row([1] * 8)])))
    # same-class boxes, none overlaps: row 0 (same class, not difficult) takes the fp
    gt = [(1, FAR, 0), (1, [0.6, 0.0, 0.9, 0.2], 1), (2, BOX, 1)]
    out.append(build('C/same_class_no_overlap', [dict(gt=gt, dets={0: [DET80]})], _cond_all_zero(), ('no_label_mask',),
                     expect=([1, 0], [_row([]), _row([])], [_row([1] * 8), _row([1] * 8)])))

    # an other-class box overlaps more, at a lower index, than the same-class one: the mask comes BEFORE the argmax
    def cond_other(case):
        jac = oracle_jaccard(case, 0, 0)[0]
        with np.errstate(**_ERR):
            raw = em.jaccard(case.bboxes[0, 0, 0], case.gbboxes[0])
        assert raw[1] > F32(0.5) > raw[2] > 0 and jac[1] == 0 and np.argmax(jac) == 2 and case.gdifficults[0, 0] == 1
        _check_expect(case)
    gt = [(2, FAR, 1), (2, BOX, 0), (1, [0.0, 0.0, 0.5, 0.1], 0)]
    out.append(build('C/other_class_overlaps_more', [dict(gt=gt, dets={0: [DET80]})], cond_other, ('no_label_mask',),
                     expect=([1, 1], [_row([]), _row([])], [_row([1]), _row([])])))
    # row 0 in turn; the detection of list 0 overlaps only an other-class box, the LAST row is of the opposite difficulty to row 0
    for tag, row0, written in (('other_class_difficult', (2, FAR, 1), 0), ('other_class', (2, FAR, 0), 1),
                               ('padding', (0, [0, 0, 0, 0], 0), 1), ('padding_difficult', (0, [0, 0, 0, 0], 3), 0)):
        gt = [row0, (2, BOX, 0), (3, FAR, 0), (2, FAR, written)]
        catches = ('argmax_same_class_only', 'no_label_mask') + (() if written else ('fp_ignores_difficulty',))
        n_gb = [0, 2 - written + (1 if row0[0] == 2 and not row0[2] else 0)]
        out.append(build('C/row0_%s' % tag, [dict(gt=gt, dets={0: [DET80]})], _cond_all_zero((0, 1)), catches,
                         expect=(n_gb, [_row([]), _row([])], [_row([written] * 8), _row([written] * 8)])))
    # a same-class box exists but does not overlap, row 0 is an other-class difficult box: the argmax is still row 0
    gt = [(2, BOX, 1), (1, FAR, 0)]
    out.append(build('C/row0_difficult_same_class_elsewhere', [dict(gt=gt, dets={0: [DET80]})], _cond_all_zero(),
                     ('argmax_same_class_only', 'fp_ignores_difficulty'),
                     expect=([1, 0], [_row([]), _row([])], [_row([]), _row([])])))
    # zero-padded detection rows behind one real detection: image 0 with a markable row 0 (every padded row is fp), image 1 with a
    # difficult row 0 (no padded row writes anything)
    im0 = dict(gt=[(1, BOX, 0), (1, FAR, 0)], dets={0: [DET80]})
    im1 = dict(gt=[(1, FAR, 1), (1, BOX, 0)], dets={0: [DET80]})

    def cond_pad(case):
        assert not case.bboxes[:, :, 1:].any() and not case.scores[:, :, 1:].any()
        for i in range(2):
            assert not oracle_jaccard(case, i, 0)[1:].any()
        _check_expect(case)
    out.append(build('C/padded_detections', [im0, im1], cond_pad, ('fp_ignores_difficulty',),
                     expect=([[2, 0], [1, 0]], [[_row([1]), _row([])], [_row([1]), _row([])]],
                             [[_row([0] + [1] * 7), _row([1] * 8)], [_row([]), _row([])]])))
    return out


# --------------------------------------------------------------------------- #
# D. state
# --------------------------------------------------------------------------- #
D_A, D_B, D_C = [0.0, 0.0, 0.25, 0.25], [0.5, 0.0, 0.75, 0.25], [0.0, 0.5, 0.25, 0.75]          # pairwise disjoint
D_TP = [1, 0, 0, 1, 0, 0, 0, 0]          # the eight steps of state_case, by hand (tests/test_match_cases_cpu.py has the table)
D_FP = [0, 1, 1, 0, 0, 0, 1, 0]
D_NGB = 2


def inside(box, frac):
    """The part of `box` that keeps `frac` of its width: jaccard ~ frac."""
    return [box[0], box[1], box[2], box[1] + (box[3] - box[1]) * frac]


def state_case():
    """Seven detections of one list, in order: tp on A; a duplicate on A (fp); sub-threshold on the fresh B (fp, B stays unmarked);
    above threshold on B (tp: step 3 did not mark it); a hit on the difficult C (nothing); C again (nothing: it was not marked, and
    would not be counted if it were); sub-threshold on the marked A (fp).  An eighth, sub-threshold on the difficult C, writes
    nothing either (a false positive on a difficult box is not recorded)."""
    dets = [D_A, inside(D_A, 0.9), inside(D_B, 0.4), inside(D_B, 0.8), D_C, inside(D_C, 0.9), inside(D_A, 0.4), inside(D_C, 0.4)]
    gt = [(1, D_A, 0), (1, D_B, 0), (1, D_C, 1)]

    def cond(case):
        jac = oracle_jaccard(case, 0, 0)
        t = F32(case.threshold)
        assert [int(np.argmax(r)) for r in jac] == [0, 0, 1, 1, 2, 2, 0, 2]
        assert [bool(r.max() > t) for r in jac] == [True, True, False, True, True, True, False, False]
        assert (np.count_nonzero(jac, axis=1) == 1).all()
        _check_expect(case)
    return build('D/state_walk', [dict(gt=gt, dets={0: dets})], cond,
                 ('mark_below_threshold', 'tp_ignores_existing', 'existing_needs_match', 'fp_ignores_difficulty', 'count_difficult'),
                 nl=1, k=8, expect=([D_NGB], D_TP, D_FP))


def family_D():
    # the same boxes under two labels, in two images: four lists, each with its own flags (a tp in every one of them)
    gt = [(1, D_A, 0), (2, D_A, 0), (1, D_B, 1), (2, D_B, 1)]
    im = dict(gt=gt, dets={0: [D_A, D_A, D_B], 1: [D_A, D_A, D_B]})

    def cond(case):
        for i in range(2):
            for l in range(2):
                jac = oracle_jaccard(case, i, l)
                assert [int(np.argmax(r)) for r in jac[:3]] == [l, l, 2 + l] and (jac[:3].max(1) == 1).all()
        _check_expect(case)
    lists = [_row([1, 0, 0]), _row([1, 0, 0])]
    fps = [_row([0, 1, 0, 1, 1, 1, 1, 1]), _row([0, 1, 0, 1, 1, 1, 1, 1])]
    two = build('D/two_labels_two_images', [im, im], cond, ('tp_ignores_existing', 'existing_needs_match', 'count_difficult'),
                expect=([[1, 1], [1, 1]], [lists, lists], [fps, fps]))
    return [state_case(), two]


# --------------------------------------------------------------------------- #
# E. degenerate boxes
# --------------------------------------------------------------------------- #
def family_E():
    nan, inf = float('nan'), float('inf')
    pt = [0.3, 0.3, 0.3, 0.3]
    gt = [(1, BOX, 0),                            # 0 a plain box, not difficult: takes every fp below
          (1, pt, 1),                             # 1 zero area, difficult
          (1, [0.1, nan, 0.4, 0.4], 1),           # 2 one NaN coordinate, difficult
          (1, [-inf, -inf, inf, inf], 0),         # 3 the whole plane
          (1, [0.2, 0.45, 0.21, 0.46], 0),       # 4 tiny: area 1e-4
          (1, [nan] * 4, 1)]                      # 5 all NaN, difficult
    dets = [[0.1, 0.4, 0.3, 0.1],                 # inverted in x: area -0.06, union with box 4 negative
            [0.4, 0.4, 0.1, 0.1],                 # inverted in both: area +0.09, no intersection
            pt,                                   # zero area on the zero-area box: 0 / 0
            [0.1, 0.1, nan, 0.4],                 # one NaN coordinate
            [nan] * 4,
            [-inf, -inf, inf, inf],               # inter = the box's area, union inf (inf - inf = NaN against box 3)
            [inf, inf, inf, inf],                 # inf - inf
            [0.0, 0.0, inf, inf],
            [-inf, 0.0, 0.0, 0.5],
            DET80]                                # and the list still works afterwards: tp on box 0

    def cond(case):
        jac = oracle_jaccard(case, 0, 0)
        assert not jac[:9].any() and not np.isnan(jac).any(), jac
        assert np.array_equal(np.flatnonzero(jac[9]), [0]) and jac[9, 0] > F32(0.5)
        g, d = case.gbboxes[0], case.bboxes[0, 0]
        with np.errstate(**_ERR):
            area = lambda b: (b[2] - b[0]) * (b[3] - b[1])
            assert area(d[0]) < 0 and area(g[4]) + area(d[0]) < 0 and area(d[1]) > 0           # union < 0; inverted twice: area > 0
            assert area(g[1]) == 0 and area(d[2]) == 0
        _check_expect(case)
    main = build('E/degenerate_walk', [dict(gt=gt, dets={0: dets})], cond, ('nan_propagates', 'union_ge_zero_divides'), nl=1, k=10,
                 expect=([3], [0] * 9 + [1], [1] * 9 + [0]))
    # a NaN ground-truth box in ROW 0 and a proper match elsewhere: a NaN product must not shadow it
    gt = [(1, [0.1, 0.1, nan, 0.4], 0), (2, FAR, 0), (1, BOX, 0)]

    def cond_nan0(case):
        jac = oracle_jaccard(case, 0, 0)
        assert jac[0, 0] == 0 and jac[0, 2] > F32(0.5)
        _check_expect(case)
    nan0 = build('E/nan_row0_then_match', [dict(gt=gt, dets={0: [DET80]})], cond_nan0, ('nan_propagates',), nl=1, k=2,
                 expect=([2], [1, 0], [0, 1]))
    return [main, nan0]


# --------------------------------------------------------------------------- #
# F. extent
# --------------------------------------------------------------------------- #
GS = (1, 63, 64, 65, 128, 129, 255, 256)


def _extent_case(g, where, at):
    """The only same-class box at `at`; every other row the same box under label 2, difficult."""
    gt = [(2, BOX, 1)] * g
    gt[at] = (1, BOX, 0)

    def cond(case):
        jac = oracle_jaccard(case, 0, 0)
        assert np.array_equal(np.flatnonzero(jac[0]), [at]) and jac[0, at] > F32(0.5)
        _check_expect(case)
    return build('F/g%d_%s' % (g, where), [dict(gt=gt, dets={0: [DET80, DET80]})], cond, ('no_label_mask',) if at else (), nl=1, k=2,
                 expect=([1], [1, 0], [0, 1]))


def grid256(i):
    """Box i of 256 pairwise disjoint boxes on a 16 x 16 grid."""
    y, x = F32(i // 16) / F32(16), F32(i % 16) / F32(16)
    return [y, x, y + F32(0.05), x + F32(0.05)]


def family_F():
    out = []
    for g in GS:
        out.append(_extent_case(g, 'last', g - 1))
        first = CHUNK * ((g - 1) // CHUNK)
        if first != g - 1:
            out.append(_extent_case(g, 'chunk_start', first))
    out.append(build('F/k1', [dict(gt=[(1, BOX, 0)], dets={0: [DET80]})], _cond_threshold_above, (), nl=1, k=1, expect=([1], [1], [0])))
    # 81 lists: label = list + 1; ground-truth labels 81 and 82 (82 belongs to no list)
    gt = [(81, D_A, 0), (82, D_B, 0), (1, D_C, 0), (40, D_B, 0), (81, D_B, 1), (0, [0] * 4, 0), (82, D_A, 0)]
    dets = {80: [D_A, D_B], 0: [D_C], 39: [D_B], 40: [D_B]}
    n_gb = np.zeros(81, np.int64)
    n_gb[[80, 0, 39]] = 1
    tp, fp = np.zeros((81, 2), bool), np.ones((81, 2), bool)          # row 0 (label 81, not difficult) takes every empty row's fp
    tp[80, 0] = tp[0, 0] = tp[39, 0] = True
    fp[80] = fp[0, 0] = fp[39, 0] = False                             # list 80: tp, then a hit on the difficult box (nothing)

    def cond81(case):
        assert case.scores.shape[1] == 81 and {81, 82} <= set(case.glabels[0].tolist())
        assert oracle_jaccard(case, 0, 80)[1, 4] == 1 and not oracle_jaccard(case, 0, 40).any()
        _check_expect(case)
    out.append(build('F/l81', [dict(gt=gt, dets=dets)], cond81, ('count_difficult', 'no_label_mask'), nl=81, k=2,
                     expect=(n_gb, tp, fp)))
    # difficult flags in every 64-box chunk, all 256 boxes of label 1
    hard = (0, 5, 63, 64, 100, 127, 128, 129, 191, 192, 254, 255)
    gt = [(1, grid256(i), int(i in hard)) for i in range(256)]

    def cond_chunks(case):
        d = np.flatnonzero(case.gdifficults[0])
        assert sorted(set((d // CHUNK).tolist())) == [0, 1, 2, 3]
        jac = oracle_jaccard(case, 0, 0)
        assert [int(np.argmax(r)) for r in jac[:3]] == [200, 191, 200] and (jac[:3].max(1) == 1).all()
        _check_expect(case)
    out.append(build('F/difficult_in_every_chunk', [dict(gt=gt, dets={0: [grid256(200), grid256(191), grid256(200)]})], cond_chunks,
                     ('count_difficult', 'fp_ignores_difficulty'), nl=1, k=4, expect=([256 - len(hard)], [1, 0, 0, 0], [0, 0, 1, 0])))
    # three images, 6 / 2 / 0 ground-truth boxes in 6 rows
    im0 = dict(gt=[(2, D_A, 0), (1, D_A, 0), (1, D_B, 0), (2, D_B, 1), (1, D_C, 1), (2, D_C, 0)], dets={0: [D_B, D_C, D_A], 1: [D_C, D_B]})
    im1 = dict(gt=[(1, D_B, 1), (2, D_A, 0)], dets={0: [D_A, D_B], 1: [D_A]})
    im2 = dict(gt=[], dets={0: [D_A], 1: [D_B, D_A]})
    n_gb = [[2, 2], [0, 1], [0, 0]]
    tp = [[_row([1, 0, 1]), _row([1, 0])], [_row([]), _row([1])], [_row([]), _row([])]]
    fp = [[_row([0, 0, 0, 1, 1, 1, 1, 1]), _row([0, 0, 1, 1, 1, 1, 1, 1])],          # image 0: row 0 is not difficult
          [_row([]), _row([])],                                                      # image 1: row 0 is difficult
          [_row([1] * 8), _row([1] * 8)]]                                            # image 2: all padding, row 0 not difficult

    def cond_n3(case):
        assert [int((case.glabels[i] > 0).sum()) for i in range(3)] == [6, 2, 0]
        _check_expect(case)
    out.append(build('F/n3_padding', [im0, im1, im2], cond_n3, ('fp_ignores_difficulty', 'count_difficult', 'no_label_mask'), g=6,
                     expect=(n_gb, tp, fp)))
    return out


def _cond_threshold_above(case):
    assert oracle_jaccard(case, 0, 0)[0, 0] > F32(case.threshold)
    _check_expect(case)


# --------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def match_cases():
    out = family_A() + family_B() + family_C() + family_D() + family_E() + family_F()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def random_inputs(seed, n, nl, k, g, jitter=0.05):
    """Ground truth and jittered copies of it as detections, zero padding at the end of every list: the kind of input
    tests/test_gpu_eval.py draws."""
    rs = np.random.RandomState(seed)
    gl = rs.randint(0, nl + 1, (n, g)).astype(np.int64)
    yx = rs.rand(n, g, 2).astype(F32) * F32(0.6)
    hw = rs.rand(n, g, 2).astype(F32) * F32(0.3) + F32(0.05)
    gb = np.concatenate([yx, yx + hw], -1).astype(F32)
    gb[gl == 0] = 0
    gd = (rs.rand(n, g) < 0.2).astype(np.int64)
    sc = np.sort(rs.rand(n, nl, k).astype(F32), -1)[..., ::-1].copy()
    src = gb[np.arange(n)[:, None, None], rs.randint(0, g, (n, nl, k))]
    bb = (src + rs.randn(n, nl, k, 4).astype(F32) * F32(jitter) * rs.rand(n, nl, k, 1).astype(F32)).astype(F32)
    pad = max(1, k // 5)
    sc[..., -pad:] = 0
    bb[..., -pad:, :] = 0
    return sc, bb, gl, gb, gd


def stack_groups(cases):
    """Cases of equal (L, K, G, threshold) stacked along N: [(names, image offsets, stacked inputs...)]."""
    groups = collections.OrderedDict()
    for c in cases:
        groups.setdefault((c.scores.shape[1], c.scores.shape[2], c.glabels.shape[1], c.threshold), []).append(c)
    out = []
    for key, cs in groups.items():
        if len(cs) < 2:
            continue
        cat = lambda f: np.concatenate([getattr(c, f) for c in cs], 0)
        offs = np.cumsum([0] + [c.scores.shape[0] for c in cs])
        out.append((cs, offs, cat('scores'), cat('bboxes'), cat('glabels'), cat('gbboxes'), cat('gdifficults'), key[3]))
    return out
