"""CPU: the references of the SSD losses agree with each other, the float32 emulation lies within the derived bounds, every mutant of
the emulation is killed by its named hand case, and the C entry points refuse bad arguments before any HIP call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ssd_loss_cases as sc  # noqa: E402
import ssd_loss_ref as sr  # noqa: E402

F = np.float32
HAND = sc.hand_cases()
OTHERS = sc.layout_cases() + sc.value_cases()
BY_NAME = {c.name: c for c in HAND}


def _agrees(got, ref, fi):
    """A result of losses_emulated against one of losses_ref: counts, mask, losses and gradients within the bounds."""
    if not np.array_equal(got['counts'], ref['counts']) or not np.array_equal(got['mined'], ref['mined']):
        return False
    b = sr.losses_bound(fi['x'], fi['loc'], fi['gloc'], ref, fi.get('alpha', 1.))
    b_cls, b_loc = sr.grad_bound(fi['x'], fi['loc'], fi['gloc'], ref)
    return (sr.within(got['losses'], ref['losses'], b) and sr.within(got['d_cls'], ref['d_cls'], b_cls)
            and sr.within(got['d_loc'], ref['d_loc'], b_loc))


@pytest.mark.parametrize('case', HAND, ids=[c.name for c in HAND])
def test_hand_case_is_what_its_name_says(case):
    fi = sc.flat_inputs(case)
    ref = sr.losses_ref(**fi)
    assert np.array_equal(ref['counts'], np.array(case.expect['counts'], np.int32)), ref['counts']
    nan = case.expect.get('nan', ())
    assert all(np.isnan(ref['losses'][i]) == (i in nan) for i in range(4))
    if case.expect.get('neg_zero'):
        assert ref['losses'][1] == 0 and not ref['mined'].any()
    for r in case.expect.get('mined_rows', ()):
        assert ref['mined'][r] and fi['g'][r] > 0 and not ref['pos'][r]
    assert not (ref['pos'] & ref['mined']).any() and not (ref['mined'] & ~ref['cand']).any()
    for (n_pos, n_cand, k, n_mined) in ref['counts']:
        assert n_mined <= max(k - 1, 0)


def test_decision_points():
    ref = lambda name: sr.losses_ref(**sc.flat_inputs(BY_NAME[name]))
    r = ref('scores_at_the_thresholds')
    assert list(r['pos'][:4]) == [False, True, False, False] and list(r['cand'][:4]) == [True, False, False, True]
    r = ref('layer_k_one_plus_candidates')
    assert r['t'][0] == 1.0 and np.array_equal(r['mined'], r['cand'])
    r = ref('layer_all_candidates_k_clamped')
    assert r['counts'][0][2] == 8 and r['t'][0] == r['v'].max() and int(r['mined'].sum()) == 7
    r = ref('kth_value_tied')
    assert int((r['v'] == r['t'][0]).sum()) == 3 and r['counts'][0][3] == r['counts'][0][2] - 2
    r = ref('candidate_p0_exactly_one')
    x = sc.flat_inputs(BY_NAME['candidate_p0_exactly_one'])['x']
    assert sr._softmax32(x)[0][1, 0] == F(1) and r['v'][1] == 1.0 and r['cand'][1] and not r['mined'][1] and r['t'][0] == 1.0
    r = ref('positive_label_equal_to_num_classes')
    assert np.isnan(r['d_cls'][0]).all() and not np.isnan(r['d_cls'][1:]).any() and np.isfinite(r['losses'][[1, 2]]).all()
    r = ref('layer_without_positives')
    assert r['terms'][1][0] == 0 and r['terms'][1][2] == 0 and r['terms'][1][1] > 0
    fi = sc.flat_inputs(BY_NAME['localisation_kinks'])
    d = np.abs(fi['loc'][:3] - fi['gloc'][:3])
    one = F(1)
    for v in (F(0), one, np.nextafter(one, F(2)), np.nextafter(one, F(0))):
        assert (d == v).any()
    # abs_smooth at and around its kink, float32 against float64, within the row bound
    got = sr.abs_smooth32(fi['loc'][:3] - fi['gloc'][:3]).astype(np.float64).sum(axis=1)
    want = sr.abs_smooth(fi['loc'][:3].astype(np.float64) - fi['gloc'][:3].astype(np.float64)).sum(axis=1)
    assert (np.abs(got - want) <= sr._abs_smooth_rows_bound(fi['loc'][:3], fi['gloc'][:3])).all()
    assert sr.abs_smooth(np.array([0.0, 1.0, 2.0, 0.5])).tolist() == [0.0, 0.5, 1.5, 0.125]


@pytest.mark.parametrize('case', HAND + OTHERS, ids=[c.name for c in HAND + OTHERS])
def test_the_two_references_agree(case):
    fi = sc.flat_inputs(case)
    ref, tor = sr.losses_ref(**fi), sr.losses_torch(**fi)
    assert np.array_equal(ref['counts'], tor['counts']) and np.array_equal(ref['mined'], tor['mined'])
    assert np.array_equal(np.isnan(ref['losses']), np.isnan(tor['losses']))
    assert np.allclose(ref['losses'], tor['losses'], rtol=1e-11, atol=1e-13, equal_nan=True)
    assert np.allclose(ref['d_cls'], tor['d_cls'], rtol=1e-10, atol=1e-14, equal_nan=True)
    assert np.allclose(ref['d_loc'], tor['d_loc'], rtol=1e-12, atol=1e-16)      # autograd adds 0.5 - 0.5 + |d| / 2 ... at a tiny |d|


@pytest.mark.parametrize('case', HAND, ids=[c.name for c in HAND])
def test_emulation_within_the_bound_on_hand_cases(case):
    fi = sc.flat_inputs(case)
    ref, emu = sr.losses_ref(**fi), sr.losses_emulated(**fi)
    assert _agrees(emu, ref, fi)
    assert (np.abs(emu['v'].astype(np.float64) - ref['v']) <= sr.p0_bound(fi['x'])).all()


@pytest.mark.parametrize('case', OTHERS, ids=[c.name for c in OTHERS])
def test_emulation_within_the_bound_under_its_own_mask(case):
    """Dense near-ties: the selection is recomputed from the emulation's own float32 values, the reference evaluated under it."""
    fi = sc.flat_inputs(case)
    emu = sr.losses_emulated(**fi)
    counts, mined, _ = sr.mine(emu['v'], emu['pos'], emu['cand'], fi['layer_rows'], fi['N'], fi['mining'], fi.get('negative_ratio', 3.))
    assert np.array_equal(counts, emu['counts']) and np.array_equal(mined, emu['mined'])
    ref = sr.losses_ref(**fi, mined=mined)
    assert _agrees(emu, ref, fi)
    assert (np.abs(emu['v'].astype(np.float64) - ref['v']) <= sr.p0_bound(fi['x'])).all()


def test_value_cases_are_what_they_claim():
    low = sr.losses_emulated(**sc.flat_inputs(sc.low_digit_case()))
    bits = low['v'][low['cand']].view(np.uint32)
    # 0.5 itself lies inside the grid: 0x3eff.... below it, 0x3f00.... from it on, nothing else in the upper sixteen bits
    assert set(bits >> 16) <= {0x3eff, 0x3f00} and len(set(bits)) < bits.size and len(set(bits & 0xffff)) > 256
    wide = sr.losses_ref(**sc.flat_inputs(sc.wide_range_case()))
    v = wide['v'][wide['cand']]
    assert v.min() < 1e-29 and v.max() > 0.999 and wide['counts'][0][2] > 256


@pytest.mark.parametrize('mut', sr.MUTANTS)
def test_every_mutant_is_killed_by_its_hand_case(mut):
    case = BY_NAME[sc.KILLS[mut]]
    fi = sc.flat_inputs(case)
    ref = sr.losses_ref(**fi)
    assert _agrees(sr.losses_emulated(**fi), ref, fi)
    assert not _agrees(sr.losses_emulated(**fi, mut=(mut,)), ref, fi)


def test_mutant_table_is_complete():
    assert sorted(sc.KILLS) == sorted(sr.MUTANTS) and all(v in BY_NAME for v in sc.KILLS.values())


def _fake_call(lib, heads, cfg, nbytes, grad=False, targets=True):
    """The entry point on pointers that are never dereferenced on the host (argument errors come before any HIP call)."""
    from ron_tensorflow_amd import _lib
    tg, hg = _lib.Targets(), _lib.HeadGrads()
    for i in range(min(heads.num_layers, _lib.RON_MAX_LAYERS)):
        tg.gclasses[i] = tg.glocalisations[i] = tg.gscores[i] = 4096
        hg.d_cls[i] = hg.d_loc[i] = 4096
    args = [C.byref(heads), C.byref(tg) if targets else None, 1, None if cfg is None else C.byref(cfg), C.c_void_p(4096), nbytes,
            C.c_void_p(4096), C.c_void_p(4096), None]
    if grad:
        return lib.ron_ssd_losses_grad(*(args + [C.byref(hg), None]))
    return lib.ron_ssd_losses(*(args + [None]))


@pytest.mark.parametrize('grad', [False, True])
def test_argument_errors_without_a_hip_call(grad):
    from ron_tensorflow_amd import _lib
    lib = _lib.lib()
    name = b'ron_ssd_losses_grad' if grad else b'ron_ssd_losses'
    heads = _lib.Heads()
    heads.num_layers, heads.num_classes = 2, 21
    for i in range(2):
        heads.feat_h[i], heads.feat_w[i], heads.num_anchors[i] = 3, 3, 4
        heads.cls[i] = heads.loc[i] = 4096
    size = (lib.ron_ssd_losses_grad_workspace_bytes if grad else lib.ron_ssd_losses_workspace_bytes)
    need = size(C.byref(heads), 1)
    assert need > 0 and size(C.byref(heads), 0) == -1 and size(None, 1) == -1
    good = _lib.SsdLossCfg(_lib.RON_SSD_MINING_BATCH, 0.5, 3.0, 1.0)
    assert _fake_call(lib, heads, None, need, grad) == -1 and name + b': null argument' in lib.ron_last_error()
    assert _fake_call(lib, heads, good, need, grad, targets=False) == -1 and b'null argument' in lib.ron_last_error()
    assert _fake_call(lib, heads, _lib.SsdLossCfg(2, 0.5, 3.0, 1.0), need, grad) == -1 and b'unknown mining mode 2' in lib.ron_last_error()
    assert _fake_call(lib, heads, _lib.SsdLossCfg(-1, 0.5, 3.0, 1.0), need, grad) == -1 and b'unknown mining mode' in lib.ron_last_error()
    assert _fake_call(lib, heads, good, need - 1, grad) == -1 and b'workspace of %d bytes, %d needed' % (need - 1, need) in lib.ron_last_error()
    for nc in (1, 129, 0, -3):
        heads.num_classes = nc
        assert _fake_call(lib, heads, good, need, grad) == -1 and b'classes not in [2, 128]' in lib.ron_last_error()
    heads.num_classes = 21
    heads.num_layers = 9
    assert _fake_call(lib, heads, good, need, grad) == -1 and b'9 layers not in' in lib.ron_last_error()


def test_python_surface():
    from ron_tensorflow_amd import ops
    from ron_tensorflow_amd.nets import ssd_vgg_300, ssd_vgg_512
    assert ops.SSD_LOSS_COUNTS == sr.COUNTS
    assert ssd_vgg_300.SSDNet._mining == 'batch' and ssd_vgg_512.SSDNet._mining == 'layer'
    for mod in (ssd_vgg_300, ssd_vgg_512):
        assert callable(mod.ssd_losses)
        for name in ('bboxes_encode', 'losses', 'losses_and_gradients', 'validation_losses'):
            assert getattr(mod.SSDNet, name).__qualname__.startswith('SSDNet.')
    with pytest.raises(ValueError):
        ops.ssd_losses([np.zeros((1, 1, 1, 1, 2))], None, None, None, None, mining='image')
