"""Training-mode batch normalisation without a GPU (references: tests/bn_ref.py, cases: tests/bn_cases.py).

  * the float64 reference of both directions against torch-CPU float64 relu(F.batch_norm(training=True)) and its autograd, and the
    moving statistics against torch's running_mean / running_var (momentum = 1 - decay, the same unbiased update);
  * the float32 emulation of the kernel's statistics (its lanes, shifts and merge trees, and one lane adding every row) inside the
    derived bounds, exact on the lattice inputs, within 1e-4 of the variance on the offset inputs where E[x^2] - mean^2 loses it;
  * the mutant table: the definitions pass every check of bn_cases.grade on each named case, each mutant fails there;
  * through the C ABI in the library's dry-run mode: the workspace size is the geometry's for every shape the tests and the timing
    tool use, both entries plan, and every refusal is RON_ERR_INVALID with a message of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bn_cases as bc
import bn_ref as br

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional
TIMED = [(32, s, s, c) for s in (40, 20, 10, 5) for c in (512, 1024)]          # tools/batchnorm_time.py


def _shape(name):
    return name if isinstance(name, tuple) else bc.SHAPES[name]


# ------------------------------------------------------------------------------------------------------------------ the case tables
def test_shapes_sit_on_the_geometry_s_marks():
    for c in (8, 72, 1024):
        g = br.geometry(1, 1, 1, c)
        have = {s[2] for s in bc.SHAPES.values() if s[3] == c and s[0] == s[1] == 1}
        for unit in (g['rows_per_wave'], g['rpb'], g['slice_rows']):
            assert {unit, unit + 1} <= have and (unit == 1 or unit - 1 in have), (c, unit)
        ragged = 2 * g['slice_rows'] + 3
        assert ragged in have and br.geometry(1, 1, ragged, c)['slices'] == 3 and ragged % g['rpb'] != 0
    assert br.geometry(*bc.SHAPES['c72_m1'])['lpr'] == 32 and br.geometry(*bc.SHAPES['c1024_m1'])['tiles'] == 4
    assert br.geometry(*bc.SHAPES['scale40'])['slices'] == 200
    for shape in bc.LATTICE.values():          # every count in the merge tree is a power of two
        g = br.geometry(*shape)
        assert g['rows'] & (g['rows'] - 1) == 0 and {cnt & (cnt - 1) for _, _, _, cnt in br.lanes(g)} == {0}
    assert max(br.geometry(*s)['slices'] for s in TIMED) <= br.MAX_SLICES and br.geometry(1, 4096, 4096, 8)['slices'] == br.MAX_SLICES
    assert sorted(bc.MUTANTS) == sorted(['moving_var_biased', 'normalise_unbiased', 'decay_as_momentum', 'eps_outside_sqrt', 'mask_dy',
                                         'mask_dropped', 'dz_unrounded', 'dbeta_term_dropped', 'dgamma_term_dropped', 'y_unrounded',
                                         'last_slice_dropped', 'naive_variance'])


# ------------------------------------------------------------------------------------------------------- the reference against torch
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('name', ['m2', 'c72_m9', 'c8_m129', 'coarse'])          # (torch refuses M = 1 in training mode: by hand below)
def test_reference_is_torch_float64(name, relu):
    shape = bc.SHAPES[name]
    given = bc.inputs('gauss', shape)
    xs, dy = br.ROUND['bf16'](given['x']), br.ROUND['bf16'](given['dy'])          # dy a storage-type value: round(dy) is dy
    fwd = br.forward64(xs, given['gamma'], given['beta'], relu, given['eps'])
    t = lambda a, grad=False: torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)
    tx, tg, tb = t(xs, True), t(given['gamma'], True), t(given['beta'], True)
    rm, rv = t(given['moving_mean']), t(given['moving_var'])
    momentum = 1.0 - float(np.float32(bc.DECAY))
    ty = F.batch_norm(tx.permute(0, 3, 1, 2), rm, rv, tg, tb, training=True, momentum=momentum, eps=float(np.float32(given['eps'])))
    ty = (torch.relu(ty) if relu else ty).permute(0, 2, 3, 1)
    scale = max(1.0, float(ty.abs().max()))
    assert np.abs(fwd['y'] - ty.detach().numpy()).max() <= 1e-13 * scale
    want_mm, want_mv = br.moving64(given['moving_mean'], given['moving_var'], fwd['mean'], fwd['var'], fwd['rows'], bc.DECAY)
    assert np.abs(want_mm - rm.numpy()).max() <= 1e-14 and np.abs(want_mv - rv.numpy()).max() <= 1e-14
    (ty * t(dy)).sum().backward()
    dz = br.dz_of(fwd['y'], dy, 'bf16', relu)
    bwd = br.backward64(xs, dz, given['gamma'], fwd['mean'], fwd['var'], given['eps'])
    for got, want in ((bwd['dx'], tx.grad), (bwd['dgamma'], tg.grad), (bwd['dbeta'], tb.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))


def test_reference_at_one_row_is_the_definition():
    """M = 1 (torch refuses it): mean = x, var = 0, y = act(beta), the Bessel factor is max(M - 1, 1) = 1, dx = 0."""
    given = bc.inputs('gauss', bc.SHAPES['m1'])
    out = bc.run64(given, 'bf16', 1)
    xs = br.ROUND['bf16'](given['x'])
    assert np.array_equal(out['mean'], xs.reshape(-1).astype(np.float64)) and not out['var'].any()
    assert np.array_equal(out['y'].reshape(-1), br.ROUND['bf16'](np.maximum(given['beta'], 0)))
    d = np.float64(np.float32(bc.DECAY))
    assert np.array_equal(out['moving_var'], d * given['moving_var']) and not out['dx'].any()


# -------------------------------------------------------------------------------------------------------- the float32 accumulation
@pytest.mark.parametrize('order', ['kernel', 'sequential'])
@pytest.mark.parametrize('name', ['m1', 'm2', 'c8_m129', 'c8_m1027', 'c72_m33', 'c72_m67', 'c1024_m35', 'coarse'])
def test_emulated_statistics_sit_inside_their_bounds(name, order):
    for kind in ('gauss', 'tiny'):
        given = bc.inputs(kind, bc.SHAPES[name])
        for dtype in bc.DTYPES:
            xs = br.ROUND[dtype](given['x'])
            fwd = br.forward64(xs, given['gamma'], given['beta'], 0, given['eps'])
            e_mean, e_var, _ = br.stat_bounds(xs, fwd)
            mean, var = br.stats_emulate32(xs, order)
            assert br.ratio(mean, fwd['mean'], e_mean).max() <= 1.0 and br.ratio(var, fwd['var'], e_var).max() <= 1.0, (kind, dtype)


@pytest.mark.parametrize('name', sorted(bc.LATTICE))
def test_lattice_inputs_are_exact_in_the_kernel_s_order(name):
    given = bc.inputs('lattice', bc.LATTICE[name])
    for relu in (0, 1):
        out = bc.run64(given, 'bf16', relu)
        fwd = br.forward64(given['x'], given['gamma'], given['beta'], relu, 0.0)
        bwd = br.backward64(given['x'], br.dz_of(out['y'], given['dy'], 'bf16', relu), given['gamma'], fwd['mean'], fwd['var'], 0.0)
        bc.assert_lattice(given, fwd, bwd)
    mean, var = br.stats_emulate32(given['x'])
    assert np.array_equal(mean, fwd['mean']) and np.array_equal(var, fwd['var'])


@pytest.mark.parametrize('dtype', bc.DTYPES)
def test_offset_inputs_break_the_naive_variance_only(dtype):
    given = bc.inputs('offset', bc.OFFSET_SHAPE, dtype)
    fwd = br.forward64(given['x'], given['gamma'], given['beta'], 0, given['eps'])
    e_mean, e_var, _ = br.stat_bounds(given['x'], fwd)
    _, naive = br.stats_emulate32(given['x'], 'naive')
    assert (np.abs(naive - fwd['var']) >= 0.5 * fwd['var']).all(), 'E[x^2] - mean^2 in float32 should lose the variance here'
    assert br.ratio(naive, fwd['var'], e_var).min() > 1.0
    for order in ('kernel', 'sequential'):
        mean, var = br.stats_emulate32(given['x'], order)
        assert (np.abs(var - fwd['var']) <= 1e-4 * fwd['var']).all() and br.ratio(var, fwd['var'], e_var).max() <= 1.0
        assert br.ratio(mean, fwd['mean'], e_mean).max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the mutant table
@pytest.mark.parametrize('mutant', sorted(bc.MUTANTS))
def test_each_mutant_is_rejected_by_its_case(mutant):
    kind, name, relu = bc.MUTANTS[mutant]
    for dtype in bc.DTYPES:
        given = bc.inputs(kind, _shape(name), dtype)
        bc.grade('%s %s' % (name, dtype), bc.run64(given, dtype, relu), given, dtype, relu)          # the definitions pass
        with pytest.raises(AssertionError):
            bc.grade('%s %s %s' % (mutant, name, dtype), bc.run64(given, dtype, relu, mutant), given, dtype, relu)


# ------------------------------------------------------------------------------------------------------------ the C ABI, dry run
_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
job = json.loads(sys.argv[1])
fake = lambda i: None if i is None else C.c_void_p(((abs(i) + 1) << 24) + (4 if i < 0 else 0))          # i < 0: 4-byte aligned only
def desc(d):
    return _lib.BnDesc(d['n'], d['h'], d['w'], d['c'], d['dtype'], d['relu'], float(d['eps']), float(d['decay']))
def call(d, ptrs, ws, nbytes):
    p = [fake(i) for i in ptrs]
    fn = L.ron_batchnorm_train_nhwc if len(p) == 8 else L.ron_batchnorm_backward_nhwc
    rc = fn(C.byref(desc(d)), *p, fake(ws), nbytes, None)
    msg = L.ron_last_error().decode()
    L.ron_conv_plan(None, None)                      # a stale message cannot pass for the next call's
    return [int(rc), msg if rc else '']
out = {'plans': [], 'refused_desc': {}, 'refused_call': {}}
for d in job['plans']:
    nbytes = L.ron_batchnorm_workspace_bytes(C.byref(desc(d)))
    out['plans'].append([int(nbytes), call(d, [1, 2, 3, 4, 5, 6, 7, 8], 9, nbytes)[0], call(d, [1, 2, 3, 4, 5, 6, None, None], 9, nbytes)[0],
                         call(d, [1, 2 if d['relu'] else None, 3, 4, 5, 6, 7, 8, 9], 10, nbytes)[0],
                         call(d, [1, 2 if d['relu'] else None, 3, 4, 5, 6, None, None, None], 10, nbytes)[0]])
for name, d in job['refused_desc'].items():
    nbytes = L.ron_batchnorm_workspace_bytes(C.byref(desc(d)))
    msg = L.ron_last_error().decode()
    out['refused_desc'][name] = [int(nbytes), msg, call(d, [1, 2, 3, 4, 5, 6, 7, 8], 9, 1 << 40), call(d, [1, 2, 3, 4, 5, 6, 7, 8, 9], 10, 1 << 40)]
good = job['good']
need = L.ron_batchnorm_workspace_bytes(C.byref(desc(good)))
for name, (ptrs, ws, short) in job['refused_call'].items():
    out['refused_call'][name] = call(good, ptrs, ws, need - short)
print('RESULT ' + json.dumps(out))
'''


def _desc(shape, dtype=1, relu=1, eps=bc.EPS, decay=bc.DECAY):
    return dict(n=shape[0], h=shape[1], w=shape[2], c=shape[3], dtype=dtype, relu=relu, eps=eps, decay=decay)


PLANNED = [s for s in list(bc.SHAPES.values()) + list(bc.LATTICE.values()) + [bc.OFFSET_SHAPE] + TIMED + [(1, 4096, 4096, 8)]]
GOOD = (2, 5, 5, 512)
REFUSED_DESC = {
    'dtype fp32': _desc(GOOD, dtype=0), 'dtype f16x3': _desc(GOOD, dtype=3), 'dtype 7': _desc(GOOD, dtype=7),
    'c 12': _desc((2, 5, 5, 12)), 'c 4': _desc((2, 5, 5, 4)), 'c 0': _desc((2, 5, 5, 0)), 'c -8': _desc((2, 5, 5, -8)),
    'n 0': _desc((0, 5, 5, 512)), 'h 0': _desc((2, 0, 5, 512)), 'w -1': _desc((2, 5, -1, 512)),
    'rows 2^24 + 4096': _desc((4097, 64, 64, 8)), 'rows wrap int32': _desc((65536, 65536, 1, 8)),
    'eps -1e-5': _desc(GOOD, eps=-1e-5), 'eps nan': _desc(GOOD, eps=float('nan')), 'eps inf': _desc(GOOD, eps=float('inf')),
    'decay -0.1': _desc(GOOD, decay=-0.1), 'decay 1.5': _desc(GOOD, decay=1.5), 'decay nan': _desc(GOOD, decay=float('nan')),
    'relu 2': _desc(GOOD, relu=2), 'relu -1': _desc(GOOD, relu=-1),
}
_F, _B = [1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 8, 9]


def _swap(ptrs, i, v):
    return ptrs[:i] + [v] + ptrs[i + 1:]


REFUSED_CALL = dict(
    [('forward NULL %s' % nm, (_swap(_F, i, None), 9, 0)) for i, nm in enumerate(['x', 'gamma', 'beta', 'y', 'mean', 'var'])] +
    [('forward misaligned %s' % nm, (_swap(_F, i, -(i + 1)), 9, 0))
     for i, nm in enumerate(['x', 'gamma', 'beta', 'y', 'mean', 'var', 'moving_mean', 'moving_var'])] +
    [('forward moving_mean alone', (_swap(_F, 7, None), 9, 0)), ('forward moving_var alone', (_swap(_F, 6, None), 9, 0)),
     ('forward NULL workspace', (_F, None, 0)), ('forward misaligned workspace', (_F, -9, 0)), ('forward short workspace', (_F, 9, 1))] +
    [('backward NULL %s' % nm, (_swap(_B, i, None), 10, 0)) for i, nm in [(0, 'x'), (1, 'y with relu'), (2, 'dy'), (3, 'gamma'), (4, 'mean'), (5, 'var')]] +
    [('backward misaligned %s' % nm, (_swap(_B, i, -(i + 1)), 10, 0))
     for i, nm in enumerate(['x', 'y', 'dy', 'gamma', 'mean', 'var', 'dx', 'dgamma', 'dbeta'])] +
    [('backward NULL workspace', (_B, None, 0)), ('backward misaligned workspace', (_B, -10, 0)), ('backward short workspace', (_B, 10, 1))])


@pytest.fixture(scope='module')
def dry_run():
    """One child process in the library's dry-run mode (RON_PLAN_ONLY=1: every host decision, no HIP call)."""
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    plans = [_desc(s, dtype, relu) for s in PLANNED for dtype in (1, 2) for relu in (0, 1)]
    job = dict(plans=plans, refused_desc=REFUSED_DESC, good=_desc(GOOD), refused_call=REFUSED_CALL)
    p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(job)], env=dict(os.environ, RON_PLAN_ONLY='1'),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, 'the child ended with status %d (negative: a signal)\n%s%s' % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return plans, json.loads(line[len('RESULT '):])


def test_workspace_is_the_geometry_s_and_every_shape_plans(dry_run):
    plans, out = dry_run
    assert len(out['plans']) == len(plans) == 4 * len(PLANNED)
    for d, (nbytes, *rcs) in zip(plans, out['plans']):
        assert nbytes == br.geometry(d['n'], d['h'], d['w'], d['c'])['workspace_bytes'] and nbytes % 256 == 0, d
        assert rcs == [0, 0, 0, 0], (d, rcs)


def test_descriptors_outside_the_contract_are_refused(dry_run):
    got = dry_run[1]['refused_desc']
    bad = []
    for name in REFUSED_DESC:
        nbytes, msg, fwd, bwd = got[name]
        if nbytes != -1 or not msg or fwd[0] != -1 or not fwd[1] or bwd[0] != -1 or not bwd[1]:
            bad.append((name, got[name]))
    assert not bad, 'accepted, or refused without a message: %s' % bad


def test_calls_outside_the_contract_are_refused(dry_run):
    got = dry_run[1]['refused_call']
    bad = [(name, got[name]) for name in REFUSED_CALL if got[name][0] != -1 or not got[name][1]]
    assert len(got) == len(REFUSED_CALL) == 37 and not bad, 'accepted, or refused without a message: %s' % bad
