"""CPU: the ground-truth matching cases of tests/match_cases.py sit where they claim, the second reference agrees with the oracle on
them and on random inputs, every mutant of the table is caught by the cases that name it, and the family-D list gives the tp / fp
vectors and the two AP values worked out by hand below."""
import numpy as np
import pytest

import match_cases as mc
from oracle import eval_metrics as em
from ron_tensorflow_amd import metrics

CASES = mc.match_cases()
IDS = [c.name for c in CASES]

# --------------------------------------------------------------------------- #
# The family-D list by hand (match_cases.state_case: ground truth A, B of label 1 and the difficult C; threshold 0.5).
#
#   step  detection           argmax  jaccard  flags before   written        flags after
#   1     A                   A       1.0      -              tp             A
#   2     0.9 of A            A       0.9      A              fp (existing)  A
#   3     0.4 of B            B       0.4      A              fp (no match)  A            <- B stays unmarked
#   4     0.8 of B            B       0.8      A              tp             A B
#   5     C (difficult)       C       1.0      A B            nothing        A B
#   6     0.9 of C            C       0.9      A B            nothing        A B
#   7     0.4 of A            A       0.4      A B            fp             A B
#   8     0.4 of C            C       0.4      A B            nothing        A B
#
# n_gbboxes = 2 (A, B; C is difficult).  Scores 0.9, 0.85, ..., 0.55.  The streaming filter keeps the rows with tp | fp: steps
# 1, 2, 3, 4, 7, already in score order:
#   tp = 1 0 0 1 0      cumulated 1 1 1 2 2      recall    = 1/2 1/2 1/2 1   1
#   fp = 0 1 1 0 1      cumulated 0 1 2 2 3      precision = 1   1/2 1/3 1/2 2/5
# VOC07 (11 points t = 0, 0.1, .., 1; best precision at recall >= t): t <= 0.5 (six points) sees 1, t >= 0.6 (five points) sees
# the rows of recall 1, whose best precision is 1/2:  AP07 = (6 * 1 + 5 * 1/2) / 11 = 8.5 / 11.
# VOC12 (area under the monotone envelope): precision envelope 1 up to recall 1/2, then 1/2 up to recall 1:
# AP12 = 1/2 * 1 + 1/2 * 1/2 = 0.75.
# --------------------------------------------------------------------------- #
D_NGB = 2
D_TP = [1, 0, 0, 1, 0, 0, 0, 0]
D_FP = [0, 1, 1, 0, 0, 0, 1, 0]
D_KEPT_TP = [1, 0, 0, 1, 0]
D_KEPT_FP = [0, 1, 1, 0, 1]
D_KEPT_SCORES = np.array([0.9, 0.85, 0.8, 0.75, 0.6], np.float32)          # det_scores: float32(0.9) - j * float32(0.05)
D_PRECISION = [1.0, 1 / 2, 1 / 3, 1 / 2, 2 / 5]
D_RECALL = [0.5, 0.5, 0.5, 1.0, 1.0]
D_AP07 = 8.5 / 11
D_AP12 = 0.75


def chain(n_gb, tp, fp, scores):
    """StreamingTpFp -> precision_recall -> both AP functions, checked against the literals above at every stage."""
    st = metrics.StreamingTpFp([1])
    st.update(n_gb, tp, fp, scores)
    ngb, ndet, t, f, s = st.arrays(1)
    assert (ngb, ndet) == (D_NGB, 5)
    assert t.tolist() == D_KEPT_TP and f.tolist() == D_KEPT_FP
    assert np.allclose(s, D_KEPT_SCORES, rtol=0, atol=1e-6)
    prec, rec = metrics.precision_recall(ngb, ndet, t, f, s)
    assert np.allclose(prec, D_PRECISION, rtol=0, atol=1e-15) and rec.tolist() == D_RECALL
    ap07, ap12 = metrics.average_precision_voc07(prec, rec), metrics.average_precision_voc12(prec, rec)
    assert abs(ap07 - D_AP07) < 1e-12 and ap12 == D_AP12
    res = metrics.evaluate(st)
    assert res['AP_VOC07/mAP'] == ap07 and res['AP_VOC12/mAP'] == ap12
    return ap07, ap12


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_case_condition_holds(case):
    case.condition(case)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_references_agree_on_case(case):
    ref, orc = mc.reference(case), mc.oracle(case)
    for name, a, b in zip(('n_gbboxes', 'tp', 'fp'), ref, orc):
        assert a.shape == b.shape and np.array_equal(a, b), name
    if case.expect is not None:
        assert mc.same_result(ref, case.expect)


@pytest.mark.parametrize('n,nl,k,g', [(2, 20, 60, 12), (3, 5, 64, 1), (1, 3, 33, 64), (2, 4, 50, 100), (1, 2, 40, 256)])
def test_references_agree_on_random_inputs(n, nl, k, g):
    inp = mc.random_inputs(n * 1000 + g, n, nl, k, g)
    ref, orc = mc.match_ref(*inp), mc.oracle_dense(*inp)
    assert ref[1].any() and ref[2].any()
    assert mc.same_result(ref, orc)


def test_case_shapes_stay_tiny():
    for c in CASES:
        n, nl, k = c.scores.shape
        assert k <= 16 and n <= 3 and (nl <= 4 or c.name == 'F/l81'), c.name
        assert 1 <= c.glabels.shape[1] <= 256
    assert sorted({c.glabels.shape[1] for c in CASES if c.name.startswith('F/g')}) == list(mc.GS)


@pytest.mark.parametrize('mutant', [m for m in mc.MUTANTS if m not in mc.EQUIVALENT_MUTANTS])
def test_mutant_is_caught(mutant):
    named = [c for c in CASES if mutant in c.catches]
    assert named, 'no case claims to catch %s' % mutant
    for case in named:
        assert not mc.same_result(mc.reference(case), mc.reference(case, (mutant,))), case.name


@pytest.mark.parametrize('mutant', mc.EQUIVALENT_MUTANTS)
def test_equivalent_mutant_changes_nothing(mutant):
    """Marking a difficult box cannot be seen: its flag is read only when it is the argmax again, and then not_difficult gates both
    outputs.  The table keeps the name so that nobody looks for a case; this asserts the equivalence on everything at hand."""
    assert not any(mutant in c.catches for c in CASES)
    for case in CASES:
        assert mc.same_result(mc.reference(case), mc.reference(case, (mutant,))), case.name
    for seed in range(4):
        inp = mc.random_inputs(seed, 2, 3, 40, 9)
        assert mc.same_result(mc.match_ref(*inp), mc.match_ref(*inp, mut=(mutant,)))


def test_every_catches_entry_is_a_mutant():
    for c in CASES:
        assert set(c.catches) <= set(mc.MUTANTS), c.name


def test_stacked_groups_equal_their_cases():
    """The stacking the GPU file relies on: images are independent in both references."""
    groups = mc.stack_groups(CASES)
    assert len(groups) >= 4
    for cs, offs, sc, bb, gl, gb, gd, thr in groups:
        got = mc.oracle_dense(sc, bb, gl, gb, gd, thr)
        for c, a, b in zip(cs, offs[:-1], offs[1:]):
            assert mc.same_result([x[a:b] for x in got], mc.oracle(c)), c.name


def test_state_walk_chain_by_hand():
    case = [c for c in CASES if c.name == 'D/state_walk'][0]
    for n_gb, tp, fp in (mc.oracle(case), mc.reference(case)):
        assert n_gb.tolist() == [[D_NGB]] and tp[0, 0].astype(int).tolist() == D_TP and fp[0, 0].astype(int).tolist() == D_FP
        chain(n_gb, tp, fp, case.scores)
        # the oracle's own P / R / AP on the same vectors
        t, f, s = em.streaming_filter(tp, fp, case.scores)
        prec, rec = em.precision_recall(D_NGB, t, f, s)
        assert abs(em.average_precision_voc07(prec, rec) - D_AP07) < 1e-12 and em.average_precision_voc12(prec, rec) == D_AP12


def test_precision_recall_ties_across_batches():
    """Equal scores in two batches: the sort is stable, the earlier batch's detection comes first.  Batch 1 holds a tp at 0.5, batch 2
    a fp at 0.9 and a fp at 0.5; one ground-truth box.  Order 0.9 (fp), 0.5 (tp, batch 1), 0.5 (fp, batch 2):
    precision 0, 1/2, 1/3 and recall 0, 1, 1.  (The other order of the tie gives precision 0, 0, 1/3.)"""
    st = metrics.StreamingTpFp([1])
    st.update(np.array([[1]]), np.array([[[True]]]), np.array([[[False]]]), np.array([[[0.5]]], np.float32))
    st.update(np.array([[0]]), np.array([[[False, False]]]), np.array([[[True, True]]]), np.array([[[0.9, 0.5]]], np.float32))
    ngb, ndet, t, f, s = st.arrays(1)
    assert (ngb, ndet) == (1, 3) and t.tolist() == [True, False, False] and s.tolist() == [0.5, np.float32(0.9), 0.5]
    for prec, rec in (metrics.precision_recall(ngb, ndet, t, f, s), em.precision_recall(ngb, t, f, s)):
        assert np.allclose(prec, [0.0, 1 / 2, 1 / 3], rtol=0, atol=1e-15) and rec.tolist() == [0.0, 1.0, 1.0]
    prec, rec = metrics.precision_recall(ngb, ndet, t, f, s)
    # VOC12 by hand: envelope 1/2 over recall 0 .. 1; VOC07: every one of the 11 points sees 1/2
    assert metrics.average_precision_voc12(prec, rec) == 0.5 and abs(metrics.average_precision_voc07(prec, rec) - 0.5) < 1e-12
