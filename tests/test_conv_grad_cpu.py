"""The convolution-backward reference, its mutants and the argument checks of ron_conv2d_backward_nhwc, without a GPU.

  * the float64 formulas of tests/conv_grad_ref.py against torch-CPU float64 autograd;
  * the rounded reference and a float32 emulation (any accumulation order, pixel slices) are inside the bounds the GPU test uses;
  * every mutant of conv_grad_ref.MUTANTS is caught by at least one case under that same grading;
  * the lattice inputs meet the conditions that make them exact;
  * ron_conv2d_backward_workspace_bytes and every refusal of the entry point, through the C ABI in the library's dry-run mode."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_grad_cases as cg
import conv_grad_ref as ref

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('case', cg.SMALL)
def test_reference_is_torch_float64_autograd(case):
    n, h, w, cin, cout, k, rate = cg.CASES[case]
    x, wt, y, dy = cg.inputs('gauss', case)
    xs, ws, dz = ref.seen(x, wt, y, dy, 'bf16', True)
    g = ref.grads64(xs, ws, dz, rate)
    tx = torch.from_numpy(xs.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
    tw = torch.from_numpy(ws.astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True)
    tb = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.conv2d(tx, tw, tb, padding=(k - 1) * rate // 2, dilation=rate)
    (out * torch.from_numpy(dz.astype(np.float64)).permute(0, 3, 1, 2)).sum().backward()
    # the same float64 products summed in another order: 2^-40 of each output's own largest magnitude (K <= 1728 additions of 2^-53)
    for name, got in (('dx', tx.grad.permute(0, 2, 3, 1).numpy()), ('dw', tw.grad.permute(2, 3, 1, 0).numpy()), ('db', tb.grad.numpy())):
        assert np.abs(got - g[name][0]).max() <= 2.0 ** -40 * np.abs(g[name][0]).max(), name
    if case == 'A':          # only the centre tap sees a 1 x 1 map
        off_centre = np.ones((3, 3), bool)
        off_centre[1, 1] = False
        assert not g['dw'][0][off_centre].any() and g['dw'][0][1, 1].any()


@pytest.mark.parametrize('dtype', cg.DTYPES)
@pytest.mark.parametrize('case', sorted(cg.CASES))
def test_lattice_conditions_and_reference_inside_its_bounds(case, dtype):
    rate = cg.CASES[case][6]
    for kind in cg.KINDS:
        x, wt, y, dy = cg.inputs(kind, case)
        for relu in (0, 1):
            xs, ws, dz = ref.seen(x, wt, y, dy, dtype, relu)
            g = ref.grads64(xs, ws, dz, rate)
            if kind == 'lattice':
                assert np.array_equal(xs, x) and np.array_equal(ws, wt)
                cg.assert_lattice(wt, g['dx'][0], g['dw'][0], g['db'][0])
                if relu:
                    assert 0.3 < (y == 0).mean() < 0.5
            ref.check('%s %s relu=%d reference' % (case, kind, relu), ref.deliver(g, dtype), g, dtype, kind)


@pytest.mark.parametrize('order,slices', [('pixel', 1), ('reverse', 1), ('step', 1), ('pixel', 2), ('step', 7)])
def test_float32_emulation_inside_the_bound(order, slices):
    for case in ('B', 'D'):
        n, h, w, cin, cout, k, rate = cg.CASES[case]
        x, wt, y, dy = cg.inputs('gauss', case)
        xs, ws, dz = ref.seen(x, wt, y, dy, 'bf16', True)
        g = ref.grads64(xs, ws, dz, rate)
        dw = ref.dw_emulate32(xs, dz, k, rate, order, slices)
        top = ref.grade('%s %s x%d' % (case, order, slices), {'dw': dw}, g, 'bf16', 'gauss')['dw']
        assert top <= 1.0
        xl, wl, yl, dyl = cg.inputs('lattice', case)
        xs, ws, dz = ref.seen(xl, wl, yl, dyl, 'bf16', True)
        assert np.array_equal(ref.dw_emulate32(xs, dz, k, rate, order, slices), ref.grads64(xs, ws, dz, rate)['dw'][0])


@pytest.mark.parametrize('name', ref.MUTANTS)
def test_every_mutant_is_killed(name):
    """Under the GPU test's grading (lattice: equality, gauss: ratio <= 1) at least one (case, kind) rejects the mutant; the structural
    mutants must fall to the lattice, the rounding ones to the gauss inputs."""
    rounding = name in ('dz_unrounded', 'db_unrounded')
    killed = []
    for case in sorted(cg.CASES):
        rate = cg.CASES[case][6]
        for kind in cg.KINDS:
            x, wt, y, dy = cg.inputs(kind, case)
            out = ref.mutant(name, x, wt, y, dy, 'bf16', 1, rate)
            if out is None:
                continue
            xs, ws, dz = ref.seen(x, wt, y, dy, 'bf16', 1)
            g = ref.grads64(xs, ws, dz, rate)
            tops = ref.grade(case, dict(zip(('dx', 'dw', 'db'), out)), g, 'bf16', kind, verbose=False)
            if max(tops.values()) > 1.0:
                killed.append((case, kind))
        if killed and (rounding or any(kd == 'lattice' for _, kd in killed)):
            break
    assert killed, 'mutant %s survives every case' % name
    if rounding:
        assert all(kd == 'gauss' for _, kd in killed), killed         # integers cannot show a missing rounding
    else:
        assert any(kd == 'lattice' for _, kd in killed), 'mutant %s: no lattice case catches it (%s)' % (name, killed)


def test_unmutated_operator_passes_the_grading():
    for case in cg.SMALL:
        rate = cg.CASES[case][6]
        for kind in cg.KINDS:
            x, wt, y, dy = cg.inputs(kind, case)
            out = ref.mutant(None, x, wt, y, dy, 'bf16', 1, rate)
            g = ref.grads64(*ref.seen(x, wt, y, dy, 'bf16', 1), rate)
            ref.check(case, dict(zip(('dx', 'dw', 'db'), out)), g, 'bf16', kind)


# ------------------------------------------------------------------------------------------------------------- the C ABI, dry run
_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
cases = json.loads(sys.argv[1])
fake = lambda i: C.c_void_p((i + 1) << 24)          # device "addresses" nobody dereferences in the dry run
def desc(n, h, w, cin, cout, k, rate, stride=1, relu=1, transpose=0, dtype='bf16', pool=0, splitk=-1, tile_cfg=-1):
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, rate, relu, transpose, _lib.DTYPES[dtype], tile_cfg, 0, 0, pool, splitk, 0)
def call(d, ws_bytes, y=True):
    return L.ron_conv2d_backward_nhwc(C.byref(d), fake(1), fake(2), fake(3) if y else None, fake(4), fake(5), fake(6), fake(7), fake(8), ws_bytes, None)
out = {'bytes': {}, 'bytes2n': {}, 'ok': {}, 'refused': {}}
for name, c in cases.items():
    d = desc(*c)
    out['bytes'][name] = L.ron_conv2d_backward_workspace_bytes(C.byref(d))
    d2 = desc(2 * c[0], *c[1:])
    out['bytes2n'][name] = L.ron_conv2d_backward_workspace_bytes(C.byref(d2))
    for dt in ('bf16', 'fp16'):
        for sk in (-1, 1, 2, 7):
            d = desc(*c, dtype=dt, splitk=sk)
            out['ok']['%%s %%s %%d' %% (name, dt, sk)] = call(d, L.ron_conv2d_backward_workspace_bytes(C.byref(d)))
b = cases['B']
bad = {
    'stride 2': desc(2, 6, 8, 64, 24, 3, 1, stride=2),
    'transpose': desc(2, 5, 7, 64, 128, 2, 1, stride=2, transpose=1),
    'pool': desc(*b, pool=1),
    'k = 5': desc(2, 5, 7, 64, 24, 5, 1),
    'cin = 96': desc(2, 5, 7, 96, 24, 3, 1),
    'cin = 3': desc(2, 5, 7, 3, 64, 3, 1),
    'fp32': desc(*b, dtype='fp32'),
    'f16x3': desc(*b, dtype='f16x3'),
    'tile_cfg': desc(*b, tile_cfg=1),
    'splitk 0': desc(*b, splitk=0),
    'dilation 32': desc(2, 40, 40, 64, 24, 3, 32),          # the data gradient is a forward launch: its dilation field ends at 31
    'dilation 0': desc(2, 5, 7, 64, 24, 3, 0),
    '1x1 dilation 32': desc(2, 5, 7, 64, 24, 1, 32),
}
for name, d in bad.items():
    nbytes = L.ron_conv2d_backward_workspace_bytes(C.byref(d))
    msg_b = L.ron_last_error().decode()
    rc = call(d, 1 << 40)
    out['refused'][name] = [nbytes, msg_b, rc, L.ron_last_error().decode()]
d = desc(*b)
need = L.ron_conv2d_backward_workspace_bytes(C.byref(d))
rc = call(d, need, y=False)
out['refused']['relu with NULL y'] = [-1, 'x', rc, L.ron_last_error().decode()]
rc = call(d, need - 1)
out['refused']['short workspace'] = [-1, 'x', rc, L.ron_last_error().decode()]
rc = L.ron_conv2d_backward_nhwc(C.byref(d), fake(1), fake(2), fake(3), C.c_void_p((5 << 24) + 4), fake(5), fake(6), fake(7), fake(8), need, None)
out['refused']['misaligned dy'] = [-1, 'x', rc, L.ron_last_error().decode()]
big = desc(32, 320, 320, 64, 64, 3, 1, splitk=1000000)
out['capped'] = L.ron_conv2d_backward_workspace_bytes(C.byref(big))
d = desc(*b, relu=0)
out['ok']['no relu, NULL y'] = call(d, need, y=False)
print('RESULT ' + json.dumps(out))
'''


@pytest.fixture(scope='module')
def dry_run():
    """One child process in the library's dry-run mode (RON_PLAN_ONLY=1: every host decision, no HIP call), so that neither this
    process's library state nor a GPU is involved."""
    import json
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    env = dict(os.environ, RON_PLAN_ONLY='1')
    p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(cg.CASES)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_workspace_bytes(dry_run):
    for name in cg.CASES:
        b, b2 = dry_run['bytes'][name], dry_run['bytes2n'][name]
        assert b > 0 and b % 256 == 0, (name, b)
        assert b2 > b, 'case %s: the workspace does not grow with n (%d -> %d)' % (name, b, b2)


def test_forced_split_is_capped(dry_run):
    """conv1_2 at batch 32 with an absurd forced split: the slabs of the slices stay below 2 GiB, so the whole workspace below 4 GiB."""
    assert 0 < dry_run['capped'] < 4 * 2 ** 30, dry_run['capped']


def test_accepted_descriptors_plan_in_the_dry_run(dry_run):
    assert dry_run['ok'] and all(rc == 0 for rc in dry_run['ok'].values()), {k: v for k, v in dry_run['ok'].items() if v}


def test_refusals(dry_run):
    want = ['stride 2', 'transpose', 'pool', 'k = 5', 'cin = 96', 'cin = 3', 'fp32', 'f16x3', 'relu with NULL y', 'short workspace']
    for name in want + ['tile_cfg', 'splitk 0', 'misaligned dy', 'dilation 32', 'dilation 0', '1x1 dilation 32']:
        nbytes, msg_b, rc, msg = dry_run['refused'][name]
        assert nbytes == -1 and msg_b, (name, nbytes, msg_b)
        assert rc == -1 and msg, '%s: status %d (%s), RON_ERR_INVALID (-1) expected' % (name, rc, msg)
