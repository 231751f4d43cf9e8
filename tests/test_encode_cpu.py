"""CPU: the two references of RONNet.bboxes_encode agree, the decision-point cases sit where they claim and catch every mutant,
and the loss reference agrees with torch's own float64 cross_entropy / smooth_l1_loss on the same masks."""
import numpy as np
import pytest

import encode_cases as ec
import encode_ref as er

CASES = ec.encode_cases()
LOSS_CASES = ec.loss_cases()


def _ulps(a, b):
    """Distance of two float32 arrays in units in the last place (equal NaN / inf positions count as 0)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid='ignore'):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return np.where(same, 0.0, d)


def _agree(vec, sca):
    for k in (0, 2, 3, 4):              # classes, scores, corners, match index
        assert np.array_equal(vec[k], sca[k]), k
    assert np.array_equal(vec[1][:, :2], sca[1][:, :2], equal_nan=True)
    assert np.nanmax(_ulps(vec[1][:, 2:], sca[1][:, 2:]), initial=0.0) <= 1
    assert np.array_equal(np.isnan(vec[1]), np.isnan(sca[1]))


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_case_condition_holds(case):
    case.condition(case)


@pytest.mark.parametrize('case', [c for c in CASES if not c.name.startswith('n_')], ids=lambda c: c.name)
def test_references_agree_on_case(case):
    tab = ec.table(case)
    for i in range(case.glabels.shape[0]):
        vec = er.encode_np(case.glabels[i], case.gbboxes[i], tab, case.high, case.low)
        sca = er.encode_scalar(case.glabels[i], case.gbboxes[i], tab, case.high, case.low)
        _agree(vec, sca)


def test_references_agree_on_ron320_anchors():
    case = [c for c in CASES if c.name.startswith('n_')][0]
    tab = ec.table(case)
    assert tab.total == 21250 and int(tab.inside().sum()) == 13743
    i = 2                                # three boxes: the scalar loops stay around a second
    _agree(er.encode_np(case.glabels[i], case.gbboxes[i], tab), er.encode_scalar(case.glabels[i], case.gbboxes[i], tab))


@pytest.mark.parametrize('seed', range(6))
def test_references_agree_on_random_inputs(seed):
    rs = np.random.RandomState(100 + seed)
    anchors = [ec.grid_layer(np.arange(3) / 3. + 1 / 6., np.arange(3) / 3. + 1 / 6., [0.5, 0.3, 0.7], [0.5, 0.6, 0.25]),
               ec.grid_layer(np.arange(6) / 6. + 1 / 12., np.arange(5) / 5. + 0.1, [0.2, 0.15], [0.2, 0.3])]
    tab = er.AnchorTable(anchors, [8, 2], (64, 64))
    gl, gb = ec.random_ground_truth(seed, 3, 9, counts=[9, int(rs.randint(1, 9)), 0], lo=0.05, hi=0.7)
    for i in range(3):
        _agree(er.encode_np(gl[i], gb[i], tab), er.encode_scalar(gl[i], gb[i], tab))


def _differs(a, b):
    return any(not np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:4], b[:4]))


@pytest.mark.parametrize('mutant', er.MUTANTS)
def test_mutant_is_caught(mutant):
    named = [c for c in CASES if mutant in c.catches]
    assert named, 'no case claims to catch %s' % mutant
    for case in named:
        assert _differs(ec.reference(case), ec.reference(case, mut=(mutant,))), case.name


def test_ron320_case_group_sizes():
    case = [c for c in CASES if c.name.startswith('n_')][0]
    for i in range(case.glabels.shape[0]):
        cls = ec.reference(case, image=i)[0]
        assert 20 <= (cls > 0).sum() <= 400 and 100 <= (cls == -1).sum() <= 2000


def test_wh_bound_holds_for_the_float32_reference():
    for case in CASES:
        tab = ec.table(case)
        for i in range(case.glabels.shape[0]):
            cls, loc, sc, bb, m = ec.reference(case, image=i)
            if er.present_rows(case.glabels[i]) == 0:
                continue
            w64, h64, bw, bh = er.loc_reference64(case.gbboxes[i], tab, m, )
            for got, ref, bound in ((loc[:, 2], w64, bw), (loc[:, 3], h64, bh)):
                ok = np.isfinite(ref)
                assert ok.any() or case.name.startswith('l_')
                assert (np.abs(got[ok] - ref[ok]) <= bound[ok]).all(), case.name


# ------------------------------------------------------------------------------------------------------------ losses
def _flat_inputs(c):
    f = er.flatten_rows
    return dict(logits=f(c.logits, ec.NUM_CLASSES), localisations=f(c.localisations, 4), objness_logits=f(c.objness_logits, 2),
                objness_pred=f(c.objness_pred), gclasses=f(c.gclasses), glocalisations=f(c.glocalisations, 4),
                rand_obj=c.rand_objness, rand_cls=c.rand_cls)


@pytest.mark.parametrize('case', LOSS_CASES, ids=[c.name for c in LOSS_CASES])
def test_loss_case_condition_holds(case):
    assert case.condition(case, ec.loss_case_masks(case))


@pytest.mark.parametrize('case', LOSS_CASES, ids=[c.name for c in LOSS_CASES])
def test_loss_reference_matches_torch_float64(case):
    import torch
    import torch.nn.functional as TF
    fi = _flat_inputs(case)
    ref, counts, terms = er.losses_ref(**fi, **case.kwargs)
    mk = terms['masks']
    w_cls, w_obj, w_loc = terms['weights']
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    cls_set, obj_set, cls_pos = (torch.from_numpy(mk[k]) for k in ('cls_set', 'obj_set', 'cls_pos'))
    labels = torch.from_numpy(np.clip(fi['gclasses'], 0, ec.NUM_CLASSES))
    n_pos, n_cls_pos = int(counts[0]), int(counts[2])
    l_cls = w_cls * TF.cross_entropy(t64(fi['logits'])[cls_set], labels[cls_set]) if n_pos > 0 else torch.tensor(0.0, dtype=torch.float64)
    l_obj = w_obj * TF.cross_entropy(t64(fi['objness_logits'])[obj_set], torch.from_numpy(mk['pos'].astype(np.int64))[obj_set]) \
        if n_pos > 0 else torch.tensor(0.0, dtype=torch.float64)
    # torch's smooth_l1_loss(beta) is 0.5 d^2 / beta below beta and |d| - 0.5 beta above: beta = 1 / 9 is modified_smooth_l1(sigma = 3);
    # its branch is taken on the float64 difference, the reference's on the float32 one: they part only where |d| is within a rounding
    # of 1 / 9, where both branches give 1 / 18 to a relative 1e-7
    sl = TF.smooth_l1_loss(t64(fi['localisations'])[cls_pos], t64(fi['glocalisations'])[cls_pos], beta=1. / 9, reduction='none').sum(dim=1)
    l_loc = w_loc * sl.mean() if n_cls_pos > 0 else torch.tensor(0.0, dtype=torch.float64)
    want = np.array([float(l_cls), float(l_obj), float(l_loc)])
    assert np.array_equal(np.isnan(want), np.isnan(ref[:3]))
    ok = ~np.isnan(want)
    assert np.allclose(ref[:3][ok], want[ok], rtol=1e-9, atol=1e-12)
    assert np.isnan(ref[3]) == np.isnan(want).any()
    if case.name == 'no_positive':
        assert not ref.any()
    if case.name == 'empty_class_set_is_nan':
        assert np.isnan(ref[0]) and not np.isnan(ref[1])
    if case.name == 'no_positive_above_the_objectness_threshold':
        assert ref[2] == 0


@pytest.mark.parametrize('case', LOSS_CASES, ids=[c.name for c in LOSS_CASES])
def test_loss_bound_admits_the_float32_arithmetic(case):
    """The CPU emulation of the kernels' arithmetic lies inside the derived bound ..."""
    fi = _flat_inputs(case)
    ref, counts, terms = er.losses_ref(**fi, **case.kwargs)
    bound = er.losses_bound(fi['logits'], fi['localisations'], fi['objness_logits'], fi['glocalisations'], terms)
    got, c2 = er.losses_emulated(**fi, **case.kwargs)
    assert np.array_equal(counts, c2)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert (np.abs(got.astype(np.float64) - ref)[ok] <= bound[ok]).all(), (got, ref, bound)


def test_loss_bound_rejects_the_mutants():
    """... and the two mutants do not: half-precision accumulation, and the maximum subtraction left out (large logits)."""
    for name, mutant in (('every_negative_selected', 'half_accumulate'), ('large_logits', 'no_max')):
        case = [c for c in LOSS_CASES if c.name == name][0]
        fi = _flat_inputs(case)
        ref, counts, terms = er.losses_ref(**fi, **case.kwargs)
        bound = er.losses_bound(fi['logits'], fi['localisations'], fi['objness_logits'], fi['glocalisations'], terms)
        got, _ = er.losses_emulated(mutant=mutant, **fi, **case.kwargs)
        err = np.abs(got.astype(np.float64) - ref)
        assert not (err[:3] <= bound[:3]).all(), (mutant, got, ref, bound)      # NaN / inf count as outside
