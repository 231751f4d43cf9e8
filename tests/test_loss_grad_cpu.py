"""CPU: the references of the loss gradient (tests/loss_grad_ref.py) on the cases of tests/loss_grad_cases.py.

The float64 analytic reference agrees with torch-CPU float64 autograd; the float32 emulation of the kernel's arithmetic lies inside
grad_bound for every case, its localisation gradient and scales are the float64 ones correctly rounded; every class row's gradient
sums to 0 within the bound; every mutant of the emulation is told from it by the case loss_grad_cases.KILLS names.

`le_kink` (`<=` for `<` at |d| = 1/9) cannot be seen in the gradient: fl(9 * fl(1/9)) is exactly 1.0f, so at the one difference
where the two tests part both branches give copysign(1, d) * s_loc bit for bit.  It is told apart on the branch mask `square`
that the emulation returns, and test_le_kink_is_invisible_in_the_gradient holds the equality itself.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_grad_cases as gc  # noqa: E402
import loss_grad_ref as gr  # noqa: E402

F = np.float32
CASES = gc.grad_cases()
LAYOUT = [gc.layout_case(c, n, layers) for c in (2, 128) for (n, layers) in gc.LAYOUT_LAYERS[1:3]]
BY_NAME = {c.name: c for c in CASES}
# |analytic - autograd| in float64: the largest difference over the cases below is 6.94e-18 (= 2^-57: half an ulp of a float64 gradient
# of magnitude 1/16 .. 1/8; the gradients here stay below 0.5).  The tolerance is 16 times that, absolute: 2^-53.
REF_ATOL = 16 * 6.94e-18


def _refs(case):
    fi = gc.flat_inputs(case)
    ref = gr.grads_ref(**fi, **case.kwargs)
    return fi, ref


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_case_condition_holds(case):
    assert case.condition(case, gc.loss_case_masks(case))


def test_layout_rows():
    for (n, layers), rows in zip(gc.LAYOUT_LAYERS, gc.LAYOUT_ROWS):
        assert n * sum(h * w * a for (h, w, a) in layers) == rows
    assert gc.LAYOUT_ROWS[2:] == (63, 64, 65, 255, 256, 257, 513)
    for c in gc.layout_cases():
        assert c.condition(c, gc.loss_case_masks(c))


@pytest.mark.parametrize('case', CASES + LAYOUT, ids=lambda c: c.name)
def test_analytic_reference_matches_torch_autograd(case):
    fi, ref = _refs(case)
    tor = gr.grads_torch(**fi, **case.kwargs)
    worst = 0.0
    for k in ('d_cls', 'd_obj', 'd_loc'):
        a, b = ref[k], tor[k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = ~np.isnan(a)
        diff = np.abs(a - b)[ok]
        worst = max(worst, float(diff.max(initial=0.0)))
        assert (diff <= REF_ATOL).all(), (k, diff.max())
        assert np.array_equal(a[ok] == 0, b[ok] == 0), k            # the same elements are exactly zero
    print(case.name, 'largest |analytic - autograd|', worst)


@pytest.mark.parametrize('case', CASES + LAYOUT, ids=lambda c: c.name)
def test_emulation_lies_inside_the_bound(case):
    fi, ref = _refs(case)
    emu = gr.grads_emulated(**fi, **case.kwargs)
    b_cls, b_obj = gr.grad_bound(fi['logits'], fi['objness_logits'], ref)
    assert np.array_equal(emu['counts'], ref['counts'])
    assert gr.within(emu['d_cls'], ref['d_cls'], b_cls)
    assert gr.within(emu['d_obj'], ref['d_obj'], b_obj)
    # one rounding away from float64: the scales, and the localisation gradient outside the square branch
    with np.errstate(over='ignore', invalid='ignore'):
        assert np.array_equal(emu['scales'], ref['scales'].astype(F), equal_nan=True)
    assert np.array_equal(emu['square'], ref['square'])
    lin = ~ref['square']
    assert np.array_equal(emu['d_loc'][lin], ref['d_loc'][lin].astype(F))
    sq = ref['square']
    assert (np.abs(emu['d_loc'][sq].astype(np.float64) - ref['d_loc'][sq]) <= 3 * gr.U * np.abs(ref['d_loc'][sq]) + 2.0 ** -149).all()
    # rows outside the sets are exactly +0
    mk = ref['masks']
    for k, inside in (('d_cls', mk['cls_set']), ('d_obj', mk['obj_set']), ('d_loc', mk['cls_pos'])):
        out = emu[k][~inside]
        assert not out.any() and not np.signbit(out).any(), k


@pytest.mark.parametrize('case', CASES + LAYOUT, ids=lambda c: c.name)
def test_class_rows_sum_to_zero_within_the_bound(case):
    fi, ref = _refs(case)
    emu = gr.grads_emulated(**fi, **case.kwargs)
    b_cls, b_obj = gr.grad_bound(fi['logits'], fi['objness_logits'], ref)
    for got, bound, inside in ((emu['d_cls'], b_cls, ref['masks']['cls_set']), (emu['d_obj'], b_obj, ref['masks']['obj_set'])):
        rows = inside & ~np.isnan(got).any(axis=1)
        total = np.abs(got[rows].astype(np.float64).sum(axis=1))
        assert (total <= bound[rows].sum(axis=1)).all()
    if case.name == 'label_equal_to_num_classes':
        nan_rows = np.isnan(emu['d_cls']).any(axis=1)
        assert nan_rows.any() and np.isnan(emu['d_cls'][nan_rows]).all() and (ref['masks']['g'][nan_rows] == gc.C).all()
    if case.name == 'class_weight_zero':
        assert not emu['d_cls'].any() and emu['d_obj'].any()
    if case.name == 'difference_zero':
        assert not emu['d_loc'][:, 0::2].any() and emu['d_loc'][ref['masks']['cls_pos']][:, 1::2].all()


def _killed(case, mutant):
    """The mutated emulation differs from the unmutated one in a returned field, or leaves the bound / turns non-finite."""
    fi, ref = _refs(case)
    base = gr.grads_emulated(**fi, **case.kwargs)
    mutd = gr.grads_emulated(mut=(mutant,), **fi, **case.kwargs)
    differs = [k for k in ('d_cls', 'd_obj', 'd_loc', 'scales', 'square', 'counts') if not np.array_equal(base[k], mutd[k], equal_nan=True)]
    b_cls, b_obj = gr.grad_bound(fi['logits'], fi['objness_logits'], ref)
    outside = not (gr.within(mutd['d_cls'], ref['d_cls'], b_cls) and gr.within(mutd['d_obj'], ref['d_obj'], b_obj))
    return differs, outside


@pytest.mark.parametrize('mutant', gr.MUTANTS)
def test_mutant_is_killed_by_its_named_case(mutant):
    assert sorted(gc.KILLS) == sorted(gr.MUTANTS)
    differs, outside = _killed(BY_NAME[gc.KILLS[mutant]], mutant)
    assert differs or outside, mutant
    if mutant == 'no_max':
        assert outside                     # the large-logits case: a non-finite or out-of-bound gradient, not merely another one
    if mutant == 'le_kink':
        assert differs == ['square']


def test_le_kink_is_invisible_in_the_gradient():
    """9 * fl(1 / 9) rounds to 1: at |d| = 1/9 the square branch's 9 d s and the linear branch's sign(d) s are the same float."""
    assert F(9.0) * gr.ONE_NINTH == F(1.0)
    for name in ('difference_exactly_one_ninth', 'one_ulp_on_either_side_of_one_ninth'):
        fi = gc.flat_inputs(BY_NAME[name])
        base = gr.grads_emulated(**fi, **BY_NAME[name].kwargs)
        mutd = gr.grads_emulated(mut=('le_kink',), **fi, **BY_NAME[name].kwargs)
        assert base['d_loc'].tobytes() == mutd['d_loc'].tobytes() and base['d_loc'].any()


def test_one_ulp_case_takes_both_branches():
    case = BY_NAME['one_ulp_on_either_side_of_one_ninth']
    fi, ref = _refs(case)
    emu = gr.grads_emulated(**fi, **case.kwargs)
    rows = emu['d_loc'][ref['masks']['cls_pos']]
    s = emu['scales'][2]
    below = np.nextafter(gr.ONE_NINTH, F(0))
    want = np.array([(F(9.0) * below) * s, s, (F(9.0) * -below) * s, -s], F)
    assert (rows == want[None, :]).all() and want[0] != want[1]
