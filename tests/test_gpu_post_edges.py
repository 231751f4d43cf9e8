"""GPU parity of the post-processing kernels at their decision points: the families of tests/post_cases.py (A plateaus of equal scores,
B candidate counts on the path boundaries, C values on the thresholds, D overlaps within 2 ulp of the NMS threshold, E degenerate
boxes) through ron_post_np, ron_np_sort_nms, ron_post_tfe / detected_bboxes, ron_post_eval and ron_bboxes_filter_min, against the
oracle on the same arrays.  Probabilities and decoded boxes go in, so everything is compared with np.array_equal: classes, anchor
indices, counts, order, scores and boxes; n_candidates / n_sorted / count equal, rows behind `count` zero.

A test walks every case of its family and reports all the cases that differ, by name."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import post_cases as pc  # noqa: E402
from oracle import anchors as oanchors  # noqa: E402
from oracle import np_post  # noqa: E402

K = pc.constants()
F32 = np.float32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


def _to_dev(lst, dev, order=None):
    if lst is None:
        return None
    return [torch.from_numpy(np.ascontiguousarray(a if order is None else a[order])).to(dev) for a in lst]


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')


def _diff_dets(got, ref, keys=('classes', 'anchor_index', 'scores', 'bboxes')):
    return [k for k in keys if not _eq(got[k], ref[k])]


def _padding_is_zero(buf):
    cnt = buf.count.cpu().numpy()
    arrs = [t.cpu().numpy() for t in (buf.classes, buf.scores, buf.anchor_index, buf.bboxes)]
    return all(not a[i, cnt[i]:].any() for a in arrs for i in range(buf.n))


# --------------------------------------------------------------------------- #
# runners: the list of what differs (empty = parity)
# --------------------------------------------------------------------------- #
def run_np(ops, dev, case, ref, order=None, **flags):
    """ron_post_np on the case's heads (images in `order`), against ref (the oracle's list in the case's own order)."""
    n = case['pred'][0].shape[0]
    order = list(range(n)) if order is None else order
    flags = dict(flags or dict(cls_is_prob=True, obj_is_prob=True, loc_decoded=True))
    anchors_dev = flags.pop('anchors_dev', None)
    out, srt, ncand = ops.post_np(_to_dev(case['pred'], dev, order), _to_dev(case['obj'], dev, order), _to_dev(case['boxes'], dev, order),
                                  anchors_dev, num_classes=case['num_classes'], want_sorted=True, **flags, **case['kw'])
    got, ncand, nsort, cnt = out.to_lists(), ncand.cpu().numpy(), srt.count.cpu().numpy(), out.count.cpu().numpy()
    bad = []
    for slot, img in enumerate(order):
        r = ref[img]
        d = _diff_dets(got[slot], r)
        if ncand[slot] != r['n_candidates'] or nsort[slot] != r['n_sorted'] or cnt[slot] != len(r['classes']):
            d.append('counts %d/%d/%d vs %d/%d/%d' % (ncand[slot], nsort[slot], cnt[slot], r['n_candidates'], r['n_sorted'], len(r['classes'])))
        if d:
            bad.append('image %d: %s' % (img, d))
    if not (_padding_is_zero(out) and _padding_is_zero(srt)):
        bad.append('rows behind count are not zero')
    return bad, got


def run_list(ops, dev, case, ref):
    out, srt = ops.np_sort_nms(torch.from_numpy(case['classes'].astype(np.int32))[None].to(dev), torch.from_numpy(case['scores'])[None].to(dev),
                               torch.from_numpy(case['boxes'])[None].to(dev), want_sorted=True, **case['kw'])
    got, s = out.to_lists()[0], srt.to_lists()[0]
    bad = _diff_dets(got, ref)
    if not _eq(s['anchor_index'], ref['sorted_index']):
        bad.append('sorted order')
    if not (_padding_is_zero(out) and _padding_is_zero(srt)):
        bad.append('rows behind count are not zero')
    return bad


def run_tfe(dev, case, ref, order=None):
    from ron_tensorflow_amd import tfe
    n = case['pred'][0].shape[0]
    order = list(range(n)) if order is None else order
    s, b = tfe.post_tfe(_to_dev(case['pred'], dev, order), _to_dev(case['obj'], dev, order), _to_dev(case['boxes'], dev, order), None,
                        num_classes=case['num_classes'], **case['kw'])
    s, b = s.cpu().numpy(), b.cpu().numpy()
    bad = []
    for slot, img in enumerate(order):
        for c in range(case['num_classes'] - 1):
            if not (_eq(s[slot, c], ref[0][img, c]) and _eq(b[slot, c], ref[1][img, c])):
                bad.append('image %d class %d' % (img, c + 1))
    return bad


def run_eval(dev, case, by_class, ref, order=None):
    from ron_tensorflow_amd import ron_eval
    n = case['pred'][0].shape[0]
    order = list(range(n)) if order is None else order
    det = ron_eval.post_eval(_to_dev(case['pred'], dev, order), _to_dev(case['obj'], dev, order), _to_dev(case['boxes'], dev, order), None,
                             [case['shapes'][i] for i in order], num_classes=case['num_classes'], nms_by_class=by_class, **case['kw'])
    got, cnt = det.to_lists(), det.count.cpu().numpy()
    bad = []
    for slot, img in enumerate(order):
        d = _diff_dets(got[slot], ref[img])
        if cnt[slot] != len(ref[img]['classes']):
            d.append('count %d vs %d' % (cnt[slot], len(ref[img]['classes'])))
        if d:
            bad.append('image %d: %s' % (img, d))
    if not _padding_is_zero(det):
        bad.append('rows behind count are not zero')
    return bad


def _report(failures):
    assert not failures, '\n'.join('%s: %s' % f for f in failures)


# --------------------------------------------------------------------------- #
# ron_post_np
# --------------------------------------------------------------------------- #
def test_np_plateaus(ops, dev):
    """Family A through ron_post_np: RON-320 and SSD-512 layouts, 2 / 21 / 81 classes, top_k 1 / 64 / 400 / RON_MAX_TOPK; all-equal
    heads also as all-equal LOGITS through the fused path (zeros softmax to exactly 1 / C), which must give the identical lists."""
    failures = []
    seen = set()
    for case in pc.family_A_np():
        ref = pc.oracle(case)
        e = case['expect']
        assert ref[0]['n_candidates'] == e['n_candidates'] > case['kw']['top_k'] > e['n_above'] or case['kw']['top_k'] == 1
        seen |= {k for k in ('kSelectCap', 'kSortCap', 'kPartMin') if e['n_candidates'] > K[k]}
        bad, got = run_np(ops, dev, case, ref)
        if case['all_equal']:
            logits = dict(case, pred=[np.zeros_like(p) for p in case['pred']],
                          obj=None if case['obj'] is None else [np.zeros(o.shape[:-1] + (2,), F32) for o in case['obj']])
            bad2, got2 = run_np(ops, dev, logits, ref, cls_is_prob=False, obj_is_prob=False, loc_decoded=True)
            bad += ['fused logit path: ' + b for b in bad2] + ([] if not _diff_dets(got2[0], got[0]) else ['fused path differs from the probability path'])
        if bad:
            failures.append((case['name'], bad))
    assert seen == {'kSelectCap', 'kSortCap', 'kPartMin'}
    _report(failures)


def test_np_candidate_counts_and_reversed_batch(ops, dev):
    """Family B: one batch of 18 images with 0 .. 425 000 candidates on the path boundaries, then the same images in reversed order
    through the same workspace: the reversed result (nothing of the first call may survive in the counters or key lists)."""
    failures = []
    for case in pc.family_B_np():
        ref = pc.oracle(case)
        assert [r['n_candidates'] for r in ref] == case['expect']['counts'] and max(case['expect']['counts']) > K['kPartMin']
        n = len(ref)
        for order in (None, list(range(n))[::-1], None):
            bad, _ = run_np(ops, dev, case, ref, order)
            if bad:
                failures.append((case['name'] + (' reversed' if order else ''), bad))
    _report(failures)


def test_np_thresholds_pairs_and_degenerate_boxes(ops, dev):
    """Families C (strict >), D (pairs with overlaps within 2 ulp of the NMS threshold, and one-class chains of such overlaps that the
    class-wise scan decides link by link; 2, 21 and 81 classes) and E through ron_post_np."""
    failures = []
    for case in pc.family_C_np() + pc.family_D_np(21) + pc.family_D_np(2) + pc.family_D_np(81) + pc.family_E_np():
        ref = pc.oracle(case)
        e = case['expect']
        if 'n_candidates' in e:
            assert ref[0]['n_candidates'] == e['n_candidates']
        if 'n_kept' in e:
            assert len(ref[0]['classes']) == e['n_kept'] and e['n_on'] >= 20
        if 'chain' in e:
            assert len(ref[0]['classes']) == pc.chain_kept(e['chain']) and len(set(ref[0]['classes'])) == 1
        bad, _ = run_np(ops, dev, case, ref)
        if bad:
            failures.append((case['name'], bad))
    _report(failures)


def test_np_infinite_sides_from_raw_offsets(ops, dev):
    """Offsets of +-500 in the size channels through the raw-offset entry: exp overflows to +inf / underflows; every other offset is 0, so
    the remaining boxes are the anchors bit for bit.  Which rows are kept, their scores, and the (finite, clipped) boxes."""
    case = pc.inf_offsets_case()
    ref = pc.oracle(case)
    assert ref[0]['n_candidates'] == 24 and np.isfinite(ref[0]['bboxes']).all()
    adev = ops.anchors_to_device(oanchors.anchors_all_layers(), dev)
    bad, _ = run_np(ops, dev, case, ref, cls_is_prob=True, obj_is_prob=True, loc_decoded=False, anchors_dev=adev)
    _report([(case['name'], bad)] if bad else [])


# --------------------------------------------------------------------------- #
# ron_np_sort_nms
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('fam', ['A_list', 'D_list', 'E_list'])
def test_list_sort_nms(ops, dev, fam):
    failures = []
    for case in pc.FAMILIES[fam]():
        ref = pc.oracle(case)
        e, sc, srt = case['expect'], case['scores'], ref['sorted_index']
        if 'n_kept' in e:
            assert len(ref['classes']) == e['n_kept']
        if 'chain' in e:
            assert len(ref['classes']) == pc.chain_kept(e['chain'])
        if 'three_scores' in case['name']:          # the cut falls inside a plateau: more rows hold the last score than made the list
            assert (sc == sc[srt[-1]]).sum() > (sc[srt] == sc[srt[-1]]).sum() >= 1
        if 'special' in case['name']:               # +inf first, in position order; NaN never
            assert np.isposinf(sc[srt[:100]]).all() and (np.diff(srt[:100]) > 0).all() and not np.isnan(sc[srt]).any()
        if fam == 'E_list':                         # the three 0 / 0 boxes of one class: NaN overlap suppresses, one survives
            assert len(set(ref['anchor_index'].tolist()) & {7, 8, 9}) == 1 and np.isnan(np_post.bboxes_jaccard(case['boxes'][7], case['boxes'][8:9])).all()
        bad = run_list(ops, dev, case, ref)
        if bad:
            failures.append((case['name'], bad))
    _report(failures)


# --------------------------------------------------------------------------- #
# ron_post_tfe / detected_bboxes
# --------------------------------------------------------------------------- #
def test_tfe_plateau_in_one_class_list(dev):
    from ron_tensorflow_amd import tfe
    failures = []
    # 21 classes (three top_k / keep_top_k / mode settings), 2 and 81 classes (the (C - 1)-strided list index), SSD-512 heads (no objectness)
    for case in pc.family_A_tfe(21) + pc.family_A_tfe(2) + pc.family_A_tfe(81) + pc.family_A_tfe(21, pc.SSD512)[1:]:
        ref = pc.oracle(case)
        row = ref[0][0, case['expect']['list_class'] - 1]
        assert case['expect']['n_list'] > K['kPartMin'] and row[-1] == F32(0.5) and row[0] == F32(0.75)      # keep_top_k cuts inside the plateau
        bad = run_tfe(dev, case, ref)
        # the reference's own signature (objectness is all ones here: the gated predictions are the predictions)
        kw = {k: v for k, v in case['kw'].items() if k != 'objectness_thres'}
        ds, db = tfe.detected_bboxes(_to_dev(case['pred'], dev), _to_dev(case['boxes'], dev), num_classes=case['num_classes'], **kw)
        for c in range(1, case['num_classes']):
            if not (_eq(ds[c].cpu().numpy(), ref[0][:, c - 1]) and _eq(db[c].cpu().numpy(), ref[1][:, c - 1])):
                bad.append('detected_bboxes class %d' % c)
        if bad:
            failures.append((case['name'], bad))
    _report(failures)


def test_tfe_class_list_counts_and_reversed_batch(dev):
    failures = []
    for case in pc.family_B_tfe():
        ref = pc.oracle(case)
        counts = case['expect']['counts']
        assert max(counts) > K['kPartMin']
        for img in range(2):        # from the oracle's lists: a list holds rows iff its class has candidates, and top_k / keep_top_k bound it
            kept = [(ref[0][img, c] > 0).sum() for c in range(20)]
            assert [k > 0 for k in kept] == [m > 0 for m in counts] + [False, False] and kept[1] == 1 and max(kept) <= case['kw']['keep_top_k']
        for order in (None, [1, 0], None):
            bad = run_tfe(dev, case, ref, order)
            if bad:
                failures.append((case['name'] + (' reversed' if order else ''), bad))
    _report(failures)


def test_tfe_thresholds_pairs_and_degenerate_boxes(dev):
    """Families C (score, objectness, min_size), D ('min' and 'union', all pairs in one class list, chains; 2, 21 and 81 classes) and E
    (clip with repair and no clip, no size filter: safe_divide meets zero, negative and subnormal denominators)."""
    failures = []
    cases = pc.family_C_tfe() + pc.family_D_tfe(21) + pc.family_D_tfe(2)[:8:3] + pc.family_D_tfe(2)[8:] + pc.family_D_tfe(81)[1::3] + pc.family_E_tfe()
    for case in cases:
        ref = pc.oracle(case)
        e = case['expect']
        if 'n_kept' in e:
            assert int((ref[0] > 0).sum()) == e['n_kept'] and e['n_on'] >= 20
        if 'chain' in e:
            assert int((ref[0] > 0).sum()) == pc.chain_kept(e['chain'])
        if 'n_pass' in e:
            assert int((ref[0] > 0).sum()) == e['n_pass']
        bad = run_tfe(dev, case, ref)
        if bad:
            failures.append((case['name'], bad))
    _report(failures)


def test_bboxes_filter_min_on_the_threshold(ops, dev):
    for case in pc.family_C_filter_min():
        rs, rb = pc.oracle(case)
        assert int((rs > 0).sum()) == case['expect']['n_pass']
        s, b = ops.bboxes_filter_min(torch.from_numpy(case['scores']).to(dev), torch.from_numpy(case['boxes']).to(dev), case['top_k'], case['minsize'])
        assert _eq(s.cpu().numpy(), rs) and _eq(b.cpu().numpy(), rb), case['name']


# --------------------------------------------------------------------------- #
# ron_post_eval
# --------------------------------------------------------------------------- #
BY_CLASS = [False, True, 'scores']


@pytest.mark.parametrize('by_class', BY_CLASS, ids=['agnostic', 'by_class', 'by_class_scores'])
def test_eval_plateau_over_three_passes(dev, by_class):
    failures = []
    for case in pc.family_A_eval(21) + pc.family_A_eval(2) + pc.family_A_eval(81):
        ref = pc.oracle_eval(case, by_class)
        rank = np.searchsorted(case['expect']['rows'], ref[0]['anchor_index'])
        assert (rank >= K['kEvalCand']).any() and (ref[0]['classes'] == case['expect']['label']).all()     # kept rows beyond the first pass; lowest class wins
        bad = run_eval(dev, case, by_class, ref)
        if bad:
            failures.append((case['name'], bad))
    _report(failures)


@pytest.mark.parametrize('by_class', BY_CLASS, ids=['agnostic', 'by_class', 'by_class_scores'])
def test_eval_candidate_counts_and_reversed_batch(dev, by_class):
    failures = []
    for case in pc.family_B_eval():
        ref = pc.oracle_eval(case, by_class)
        n = len(ref)
        if by_class is False:
            assert all(len(r['classes']) < case['kw']['keep_top_k'] for r in ref)        # every pass is taken
        for order in (None, list(range(n))[::-1], None):
            bad = run_eval(dev, case, by_class, ref, order)
            if bad:
                failures.append((case['name'] + (' reversed' if order else ''), bad))
    _report(failures)


@pytest.mark.parametrize('by_class', BY_CLASS, ids=['agnostic', 'by_class', 'by_class_scores'])
def test_eval_thresholds_pairs_and_degenerate_boxes(dev, by_class):
    """Families C (objectness, objectness x probability, per-image min_sizes), D ('union' and 'min'; 2, 21 and 81 classes) and E."""
    failures = []
    cases = pc.family_C_eval() + pc.family_D_eval(21) + pc.family_D_eval(2)[::3] + pc.family_D_eval(81)[1::3] + pc.family_E_eval()       # D: pairs and chains
    for case in cases:
        ref = pc.oracle_eval(case, by_class)
        e = case['expect']
        if 'n_kept' in e:
            assert len(ref[0]['classes']) == e['n_kept'] and e['n_on'] >= 20
        if 'chain' in e:
            assert len(ref[0]['classes']) == pc.chain_kept(e['chain'])
        if 'n_pass' in e:
            assert [len(r['classes']) for r in ref] == [e['n_pass']] * len(ref)
        bad = run_eval(dev, case, by_class, ref)
        if bad:
            failures.append((case['name'], bad))
    _report(failures)
