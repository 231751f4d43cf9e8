"""The training update without a GPU (references: tests/optim_ref.py, cases: tests/optim_cases.py).

  * the float64 definitions against torch-CPU float64 over four steps: torch.optim.SGD (plain and with momentum, dampening 0, the rate
    changed between the steps), Adam(eps=0) and RMSprop(eps=0, constant rate, mean square started at 0).  With epsilon != 0 torch places
    it differently from TensorFlow and the reference holds no executable TensorFlow: the placement follows TF's kernels as written in
    include/ron_hip.h ("parity unpinned") and the mutant table guards it;
  * the float32 emulation inside the derived bounds on gauss inputs, EQUAL to the definition on the lattice inputs;
  * the mutant table: the definitions pass optim_cases.grade on every named case, each mutant fails on the one it names;
  * optim.learning_rate at its decision points, the name rules of optim.Optimizer;
  * through the C ABI in the library's dry-run mode: ron_optimizer_plan and the workspace size are the emulation's geometry for every
    list the GPU tests and tools/optimizer_time.py use, and every refusal is RON_ERR_INVALID with a message of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import optim_cases as oc
import optim_ref as orf

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda x: float(np.float32(x))


# ---------------------------------------------------------------------------------------------------- the definitions against torch
def _torch_case(rule, hyper, lrs):
    case = oc.gauss_case(rule, [7, 5], [0.25, 0.0], steps=4, lrs=lrs, hyper=hyper)
    for t in case['tensors']:          # torch starts every state at zero
        t['s0'], t['s1'] = np.zeros_like(t['s0']), np.zeros_like(t['s1'])
    return case


def _torch_run(case, make):
    params = [torch.from_numpy(t['w'].astype(np.float64)).requires_grad_(True) for t in case['tensors']]
    opt = make([dict(params=[p], weight_decay=f32(t['wd'])) for p, t in zip(params, case['tensors'])])
    for k, lr in enumerate(case['lrs']):
        for group in opt.param_groups:
            group['lr'] = float(lr)
        for p, t in zip(params, case['tensors']):
            p.grad = torch.from_numpy(t['g'][k].astype(np.float64))
        opt.step()
    return [p.detach().numpy() for p in params]


@pytest.mark.parametrize('rule, tol', [('sgd', 1e-14), ('momentum', 1e-14), ('adam', 1e-12), ('rmsprop', 1e-12)])
def test_definition_is_torch_float64(rule, tol):
    hyper = dict(orf.HYPER, epsilon=0.0)
    lrs = (0.125, 0.125, 0.0625, 0.03125) if rule != 'rmsprop' else (0.125,) * 4          # mom = lr buf only at a constant rate
    case = _torch_case(rule, hyper, lrs)
    make = {'sgd': lambda g: torch.optim.SGD(g, lr=1.0),
            'momentum': lambda g: torch.optim.SGD(g, lr=1.0, momentum=f32(hyper['momentum']), dampening=0),
            'adam': lambda g: torch.optim.Adam(g, lr=1.0, betas=(f32(hyper['beta1']), f32(hyper['beta2'])), eps=0),
            'rmsprop': lambda g: torch.optim.RMSprop(g, lr=1.0, alpha=f32(hyper['decay']), momentum=f32(hyper['momentum']), eps=0)}[rule]
    want = _torch_run(case, make)
    got = orf.run(case, 'f64')[-1]['w']
    worst = max(float(np.abs(a - b).max()) for a, b in zip(got, want))
    print('%s: largest difference from torch over four steps %.3g' % (rule, worst))
    assert worst <= tol


def test_reg_loss_definition_is_slim_s_l2_regularizer():
    case = oc.case('sgd')
    want = sum(f32(t['wd']) * float(np.sum(t['w'].astype(np.float64) ** 2)) / 2 for t in case['tensors'])
    assert abs(orf.run(case, 'f64')[0]['reg'] - want) <= 1e-15 * want and want > 0


# ------------------------------------------------------------------------------------------------------------ the float32 emulation
SHAPED = {
    'singles': lambda rule: oc.gauss_case(rule, list(oc.SINGLE_COUNTS), oc.mixed_decay(len(oc.SINGLE_COUNTS)), steps=3),
    'list': lambda rule: oc.gauss_case(rule, oc.list_counts(2 * oc.E + 1), oc.mixed_decay(2 * oc.E + 1), steps=3),
    'late': lambda rule: oc.gauss_case(rule, [9, 4], oc.mixed_decay(2), steps=2, first_step=100000),
    'reference_hyper': lambda rule: oc.gauss_case(rule, [33, 8], [0.0005, 0.0], steps=3, lrs=(0.001, 0.001, 0.0001),
                                                  hyper=dict(orf.HYPER, epsilon=1.0)),
}


@pytest.mark.parametrize('rule', orf.RULES)
@pytest.mark.parametrize('shape', sorted(SHAPED))
def test_emulation_sits_inside_the_bounds(shape, rule):
    case = SHAPED[shape](rule)
    oc.grade('%s %s' % (shape, rule), orf.emulate32(case), case, verbose=True)


@pytest.mark.parametrize('rule', orf.RULES)
def test_lattice_is_exact(rule):
    case = oc.case('lattice_' + rule)
    assert case['exact']
    oc.grade('lattice ' + rule, orf.emulate32(case), case)
    oc.grade('lattice ' + rule, orf.run(case, 'f64'), case)


def test_lattice_by_hand():
    """w 8, g 2, m 4, decay 1/4, momentum 1/2, rate 1/2: g' = 2 + 8 / 4 = 4, m = 4 / 2 + 4 = 6, w = 8 - 6 / 2 = 5; undecayed: m = 4, w = 6.
    reg_loss = (1 / 8) 64 = 8."""
    one = lambda v: np.array([v], np.float32)
    case = dict(rule='momentum', hyper=dict(orf.HYPER, momentum=0.5), lrs=[np.float32(0.5)], first_step=1, exact=True,
                tensors=[dict(w=one(8), g=[one(2)], s0=one(4), s1=one(0), wd=0.25), dict(w=one(8), g=[one(2)], s0=one(4), s1=one(0), wd=0.0)])
    got = orf.emulate32(case)[0]
    assert [float(x[0]) for x in got['w']] == [5.0, 6.0] and [float(x[0]) for x in got['s0']] == [6.0, 4.0] and float(got['reg']) == 8.0


def test_reg_tree_equals_a_plain_sum_where_both_are_exact():
    w = [np.arange(-40, 2 * oc.U + 7 - 40, dtype=np.float32) % 7 - 3, np.ones(5, np.float32), np.full(300 * oc.U // 64, 2.0, np.float32)]
    wds = [0.5, 0.0, 0.25]
    want = sum(0.5 * wd * float(np.sum(a.astype(np.float64) ** 2)) for a, wd in zip(w, wds))
    assert float(orf.reg_emulate32(w, wds)) == want


# ---------------------------------------------------------------------------------------------------------------- the mutant table
def test_the_table_names_every_mutant():
    assert sorted(oc.MUTANTS) == sorted([
        'decoupled', 'decay_on_undecayed', 'zero_times_w', 'dampening', 'lr_in_accumulator', 'nesterov', 'rms_eps_outside', 'adam_eps_inside',
        'adam_no_bias_correction', 'adam_step_off_by_one', 'reg_no_half', 'reg_from_updated', 'reg_over_undecayed', 'tail_dropped',
        'last_unit_dropped', 'launch_boundary_skipped'])
    assert set(oc.MUTANTS.values()) <= set(oc.CASES)
    poison = oc.case('poison')['tensors'][1]
    assert np.isinf(poison['w']).any() and poison['wd'] == 0.0


@pytest.mark.parametrize('name', sorted(oc.CASES))
def test_definitions_and_emulation_pass_every_named_case(name):
    case = oc.case(name)
    oc.grade(name + ' f64', orf.run(case, 'f64'), case)
    oc.grade(name + ' f32', orf.emulate32(case), case, verbose=True)


@pytest.mark.parametrize('mutant', sorted(oc.MUTANTS))
def test_each_mutant_is_rejected_by_its_case(mutant):
    case = oc.case(oc.MUTANTS[mutant])
    with pytest.raises(AssertionError):
        oc.grade('%s on %s' % (mutant, oc.MUTANTS[mutant]), orf.run(case, 'f64', mutant), case)


# ---------------------------------------------------------------------------------------------------------------- optim.py, host
def test_learning_rate_at_its_decision_points():
    from ron_tensorflow_amd import optim
    v = [f32(0.001 * f) for f in (1., 0.1, 0.001)]
    end = f32(0.00001)
    assert v[2] < end < v[1]
    got = [optim.learning_rate(s) for s in (0, 90000, 90001, 115000, 115001)]
    assert got == [v[0], v[0], v[1], v[1], end]          # the first value holds while step <= 90000; the last one is below `end`
    assert optim.learning_rate(115001, end=0.0) == v[2] and optim.learning_rate(200000, end=1e-7) == v[2]
    assert optim.learning_rate(0, end=0.01) == f32(0.01) and optim.learning_rate(100000, end=0.01) == f32(0.01)          # an end above every value
    assert optim.learning_rate(5, base=0.5, boundaries=(4, 8), factors=(1., 0.5, 0.25), end=0.0) == 0.25
    assert all(f32(x) == x for x in got)


NAMES = ['ron_320_vgg/conv1/conv1_1/weights', 'ron_320_vgg/conv1/conv1_1/biases', 'ron_320_vgg/block4/L2Normalization/gamma',
         'ron_320_vgg/block7_reverse/conv_left/weights', 'ron_320_vgg/block7_reverse/conv_left/BatchNorm/beta',
         'ron_320_vgg/block7_reverse/conv_left/BatchNorm/gamma', 'ron_320_vgg/block7_reverse/conv_left/BatchNorm/moving_mean',
         'ron_320_vgg/block7_reverse/conv_left/BatchNorm/moving_variance', 'ron_320_vgg/block6_reverse/deconv/weights',
         'ron_320_vgg/block6_reverse/deconv/biases', 'ron_320_vgg/block7_box/reg_bbox/Conv2d_1_3x3/weights']


def test_name_rules_of_the_optimizer():
    from ron_tensorflow_amd import optim
    trained = optim.trainable_names(NAMES)
    assert trained == [n for n in NAMES if 'moving_' not in n] and len(trained) == len(NAMES) - 2
    decayed = [n for n in trained if optim.decay_of(n, 0.0005) != 0]
    assert decayed == [n for n in NAMES if n.endswith('/weights')] and len(decayed) == 4
    assert {optim.decay_of(n, 0.0005) for n in decayed} == {0.0005}
    scoped = optim.trainable_names(NAMES, 'ron_320_vgg/block7_reverse, ron_320_vgg/conv1')
    assert scoped == NAMES[3:6] + NAMES[0:2]          # by scope, in the order of the scopes; the moving statistics never
    assert optim.trainable_names(NAMES, 'nothing/') == []


def test_configure_optimizer_mirrors_the_reference():
    from ron_tensorflow_amd import optim
    for name in ('adadelta', 'adagrad', 'ftrl'):
        with pytest.raises(NotImplementedError, match=name):
            optim.configure_optimizer(name)
    with pytest.raises(ValueError, match='was not recognized'):
        optim.configure_optimizer('lion')
    for name in ('rmsprop', 'adam'):
        with pytest.raises(ValueError, match='opt_epsilon'):
            optim.configure_optimizer(name)
    assert optim.configure_optimizer('momentum').keywords == dict(rule='momentum', momentum=0.9)
    assert optim.configure_optimizer('sgd').keywords == dict(rule='sgd')
    assert optim.configure_optimizer('rmsprop', opt_epsilon=1.0).keywords == dict(rule='rmsprop', momentum=0.9, decay=0.9, epsilon=1.0)
    assert optim.configure_optimizer('adam', opt_epsilon=1e-8).keywords == dict(rule='adam', beta1=0.9, beta2=0.999, epsilon=1e-8)


# ------------------------------------------------------------------------------------------------------------ the C ABI, dry run
_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + '/tools')
from ron_tensorflow_amd import _lib
L = _lib.lib()
job = json.loads(sys.argv[1])
fake = lambda i: None if i is None else C.c_void_p(((abs(i) + 1) << 24) + (4 if i < 0 else 0))          # i < 0: 4-byte aligned only
def table(rows):
    t = (_lib.OptTensor * max(len(rows), 1))()
    for i, (var, grad, s0, s1, count, wd) in enumerate(rows):
        t[i] = _lib.OptTensor(fake(var), fake(grad), fake(s0), fake(s1), count, wd)
    return t
def rows_of(counts):
    return [[4 * i + 1, 4 * i + 2, 4 * i + 3, 4 * i + 4, c, 0.5 if i %% 2 == 0 else 0.0] for i, c in enumerate(counts)]
def last():
    msg = L.ron_last_error().decode()
    L.ron_conv_plan(None, None)                      # a stale message cannot pass for the next call's
    return msg
def step(cfg, rows, n, lr, k, reg, ws, nbytes):
    c = _lib.OptCfg(*cfg) if cfg is not None else None
    rc = L.ron_optimizer_step(C.byref(c) if c is not None else None, table(rows) if rows is not None else None, n, lr, k, fake(reg), fake(ws), nbytes, None)
    return [int(rc), last() if rc else '']
import optimizer_time
timed = {v: [c for _, c in optimizer_time.trainable_list(v)] for v in ('reducedfc', 'full')}
out = {'plans': [], 'timed': timed, 'refused_plan': {}, 'refused_step': {}}
for counts in job['lists'] + [timed['reducedfc'], timed['full']]:
    rows = rows_of(counts)
    plan = (C.c_int64 * 4)()
    rc = L.ron_optimizer_plan(table(rows), len(rows), plan)
    nbytes = L.ron_optimizer_workspace_bytes(table(rows), len(rows))
    rcs = [step([rule, 0.5, 0.5, 0.5, 0.5, 0.0], rows, len(rows), 0.125, 1, reg, 9000, nbytes)[0] for rule in range(4) for reg in (None, 9001)]
    out['plans'].append([int(rc), list(plan), int(nbytes), rcs])
last()
stale = L.ron_last_error().decode()                  # what last() leaves behind
for name, counts in job['refused_plan'].items():
    plan = (C.c_int64 * 4)()
    t = table(rows_of(counts)) if counts is not None else None
    n = len(counts) if counts is not None else 1
    rc = L.ron_optimizer_plan(t, n, plan)
    m1 = last()
    nbytes = L.ron_optimizer_workspace_bytes(t, n)
    m2 = last()
    out['refused_plan'][name] = [int(rc), m1, int(nbytes), m2, step([1, 0.5, 0.5, 0.5, 0.5, 0.0], rows_of(counts) if counts is not None else None, n, 0.125, 1, None, None, 0)]
good = rows_of(job['good'])
need = L.ron_optimizer_workspace_bytes(table(good), len(good))
for name, r in job['refused_step'].items():
    rows = [list(x) for x in good]
    for i, col, v in r.get('edit', []):
        rows[i][col] = v
    out['refused_step'][name] = step(r.get('cfg', [3, 0.5, 0.5, 0.5, 0.5, 0.0]), rows, len(rows), r.get('lr', 0.125), r.get('step', 1), r.get('reg', 9001),
                                     r.get('ws', 9000), need - r.get('short', 0))
out['stale'] = stale
print('RESULT ' + json.dumps(out))
'''

LISTS = [[c] for c in oc.SINGLE_COUNTS] + [oc.list_counts(n) for n in oc.LIST_LENGTHS] + [list(oc.SINGLE_COUNTS), [6, 5, 9], [oc.U + 5, 3],
                                                                                            oc.list_counts(oc.E + 2), [1] * 4096, [1 << 34]]
# ... and the other lists of tests/test_gpu_optim.py: the schedule, Adam's steps, the workspace, the stream contract, the reg_bbox chain
LISTS += [[9, 4, oc.U + 3], [33, 6], [6, 5], [5, 2 * oc.U + 7, 3, oc.U], [oc.U + 1] * 7, [oc.U + 9, 7, 64], [5, 8, 3], [3, 1],
          [3 * 3 * 64 * 64, 64, 64, 3 * 3 * 64 * 24, 24]]
GOOD = [6, 5, 9]
NAN, INF = float('nan'), float('inf')
REFUSED_PLAN = {'n 0': [], 'n 4097': [1] * 4097, 'NULL table': None, 'count 0': [4, 0, 4], 'count -1': [-1], 'count 2^40 + 1': [(1 << 40) + 1],
                'units beyond 2^22': [1 << 34, 1]}


def _cfg(rule=3, momentum=0.5, decay=0.5, beta1=0.5, beta2=0.5, epsilon=0.0):
    return [rule, momentum, decay, beta1, beta2, epsilon]


REFUSED_STEP = dict(
    [('rule %d' % r, dict(cfg=_cfg(rule=r))) for r in (-1, 4, 7)] +
    [('%s %s' % (k, v), dict(cfg=_cfg(**{k: v}))) for k in ('momentum', 'decay', 'beta1', 'beta2') for v in (-0.5, 1.5, NAN)] +
    [('adam beta1 1', dict(cfg=_cfg(beta1=1.0))), ('adam beta2 1', dict(cfg=_cfg(beta2=1.0))), ('adam step 0', dict(step=0)),
     ('adam step -3', dict(step=-3)), ('epsilon -1', dict(cfg=_cfg(epsilon=-1.0))), ('epsilon nan', dict(cfg=_cfg(epsilon=NAN))),
     ('epsilon inf', dict(cfg=_cfg(epsilon=INF))), ('rate nan', dict(lr=NAN)), ('rate inf', dict(lr=INF)), ('rate -inf', dict(lr=-INF)),
     ('NULL cfg', dict(cfg=None))] +
    [('NULL %s' % nm, dict(edit=[(1, col, None)])) for col, nm in enumerate(['var', 'grad', 'slot0', 'slot1'])] +
    [('momentum NULL slot0', dict(cfg=_cfg(rule=1), edit=[(2, 2, None)])), ('rmsprop NULL slot1', dict(cfg=_cfg(rule=2), edit=[(0, 3, None)]))] +
    [('misaligned %s' % nm, dict(edit=[(1, col, -(5 + col))])) for col, nm in enumerate(['var', 'grad', 'slot0', 'slot1'])] +
    [('weight_decay %s' % v, dict(edit=[(2, 5, v)])) for v in (-0.5, NAN, INF)] +
    [('var twice', dict(edit=[(2, 0, 1)])), ('var is its grad', dict(edit=[(1, 1, 5)])), ('var is its slot0', dict(edit=[(1, 2, 5)])),
     ('var is its slot1', dict(edit=[(1, 3, 5)])),
     ('NULL workspace', dict(ws=None)), ('misaligned workspace', dict(ws=-9000)), ('short workspace', dict(short=1))])
# what the rule does not use is ignored: a NULL or misaligned slot of sgd / momentum, Adam's step elsewhere, no workspace without reg_loss
ACCEPTED_STEP = {
    'sgd NULL slots': dict(cfg=_cfg(rule=0), edit=[(0, 2, None), (0, 3, None)]), 'sgd misaligned slot0': dict(cfg=_cfg(rule=0), edit=[(0, 2, -7)]),
    'momentum misaligned slot1': dict(cfg=_cfg(rule=1), edit=[(0, 3, -7)]), 'momentum step 0': dict(cfg=_cfg(rule=1), step=0),
    'sgd var is its unused slot': dict(cfg=_cfg(rule=0), edit=[(1, 2, 5)]),
    'momentum beta1 1': dict(cfg=_cfg(rule=1, beta1=1.0)), 'no reg_loss, no workspace': dict(reg=None, ws=None, short=1 << 20),
    'no reg_loss, misaligned workspace': dict(reg=None, ws=-9000), 'decay 0 and 1': dict(cfg=_cfg(rule=2, decay=1.0, momentum=0.0)),
}


@pytest.fixture(scope='module')
def dry_run():
    """One child process in the library's dry-run mode (RON_PLAN_ONLY=1: every host decision, no HIP call)."""
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    job = dict(lists=LISTS, refused_plan=REFUSED_PLAN, good=GOOD, refused_step=dict(REFUSED_STEP, **ACCEPTED_STEP))
    p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(job)], env=dict(os.environ, RON_PLAN_ONLY='1'),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, 'the child ended with status %d (negative: a signal)\n%s%s' % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_plan_and_workspace_are_the_emulation_s_geometry(dry_run):
    timed = dry_run['timed']
    lists = LISTS + [timed['reducedfc'], timed['full']]
    assert len(dry_run['plans']) == len(lists) and len(timed['reducedfc']) > 100 and len(timed['full']) >= len(timed['reducedfc'])
    for counts, (rc, plan, nbytes, rcs) in zip(lists, dry_run['plans']):
        g = orf.geometry(counts)
        assert rc == 0 and plan == [g['launches'], g['units'], orf.ENTRIES, orf.UNIT], (len(counts), plan)
        assert nbytes == g['workspace_bytes'] and nbytes % 256 == 0 and nbytes >= 4 * g['units']
        assert rcs == [0] * 8, (len(counts), rcs)
    assert (orf.ENTRIES * 48 + 64) <= 4096 and orf.UNIT % (4 * orf.THREADS) == 0


def test_lists_outside_the_contract_are_refused(dry_run):
    got = dry_run['refused_plan']
    assert dry_run['stale'] != '' and len(got) == len(REFUSED_PLAN)
    bad = []
    for name in REFUSED_PLAN:
        rc, m1, nbytes, m2, (rc3, m3) = got[name]
        if rc != -1 or nbytes != -1 or rc3 != -1 or not m1 or not m2 or not m3 or dry_run['stale'] in (m1, m2, m3):
            bad.append((name, got[name]))
    assert not bad, 'accepted, or refused without a message of its own: %s' % bad


def test_steps_outside_the_contract_are_refused_by_name(dry_run):
    got = dry_run['refused_step']
    bad = [(name, got[name]) for name in REFUSED_STEP if got[name][0] != -1 or not got[name][1] or got[name][1] == dry_run['stale']]
    assert len(REFUSED_STEP) == 46 and not bad, 'accepted, or refused without a message of its own: %s' % bad
    # the message names what is wrong
    for name, word in (('rule 7', 'rule'), ('momentum 1.5', 'momentum'), ('decay nan', 'decay'), ('beta1 -0.5', 'beta1'), ('beta2 1.5', 'beta2'),
                       ('adam beta1 1', 'below 1'), ('adam step 0', 'step'), ('epsilon -1', 'epsilon'), ('rate nan', 'rate'),
                       ('NULL slot1', 'slot1'), ('momentum NULL slot0', 'slot0'), ('misaligned grad', 'aligned'), ('weight_decay nan', 'weight_decay'),
                       ('var twice', 'twice'), ('var is its grad', 'own grad'), ('var is its slot1', 'own slot'), ('short workspace', 'workspace'),
                       ('misaligned workspace', '256'), ('NULL cfg', 'configuration')):
        assert word in got[name][1], (name, got[name][1])
    assert len({got[name][1] for name in ('var twice', 'var is its grad', 'var is its slot0', 'NULL var', 'misaligned var', 'weight_decay inf',
                                          'short workspace', 'misaligned workspace', 'rule 4', 'adam step 0', 'adam beta1 1')}) == 11


def test_what_a_rule_does_not_use_is_ignored(dry_run):
    bad = [(name, dry_run['refused_step'][name]) for name in ACCEPTED_STEP if dry_run['refused_step'][name][0] != 0]
    assert not bad, 'refused: %s' % bad
