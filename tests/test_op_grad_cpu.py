"""The references of the pool backward and of the 2x2 stride-2 convolution backwards, their mutants and the argument checks of
ron_maxpool2x2_backward_nhwc / ron_conv2d_k2s2_backward_nhwc, without a GPU.

  * the two pool references (vectorised, loops) agree on every case and with torch-CPU float64 max_pool2d(ceil_mode=True) autograd;
  * the k2s2 float64 formulas against torch-CPU float64 autograd (2^-40 of each output's largest magnitude);
  * the lattice inputs meet the conditions that make them exact; the rounded reference is inside the bounds the GPU test uses;
  * every mutant is caught by at least one named case under the GPU test's own grading, the unmutated operator by none;
  * workspace bytes and every refusal of the two entry points, through the C ABI in the library's dry-run mode."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_grad_ref as cgr
import op_grad_cases as oc
import op_grad_ref as ogr

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_POOL = [c for c in oc.POOL_CASES if c != 'wide']


# ------------------------------------------------------------------------------------------------------------------------ the pool
@pytest.mark.parametrize('dtype', oc.DTYPES)
@pytest.mark.parametrize('kind', oc.POOL_KINDS)
@pytest.mark.parametrize('case', sorted(oc.POOL_CASES))
def test_pool_references_agree(case, kind, dtype):
    x, dy = oc.pool_inputs(kind, case)
    if case == 'wide':          # the loops are too slow for the whole map: its first rows, odd in both axes
        x, dy = x[:, :5, :7, :16], dy[:, :3, :4, :16]
    assert np.array_equal(ogr.pool_backward(x, dy, dtype), ogr.pool_backward_loops(x, dy, dtype))


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('kind', oc.POOL_KINDS)
@pytest.mark.parametrize('case', sorted(oc.POOL_CASES))
def test_pool_reference_is_torch_float64_autograd(case, kind, channels_last):
    x, dy = oc.pool_inputs(kind, case)
    xs, g = cgr.ROUND['bf16'](x), cgr.ROUND['bf16'](dy)
    tx = torch.from_numpy(xs.astype(np.float64)).permute(0, 3, 1, 2)
    tx = (tx.contiguous(memory_format=torch.channels_last) if channels_last else tx.contiguous()).requires_grad_(True)
    out = torch.nn.functional.max_pool2d(tx, 2, 2, ceil_mode=True)
    out.backward(torch.from_numpy(g.astype(np.float64)).permute(0, 3, 1, 2))
    assert np.array_equal(tx.grad.permute(0, 2, 3, 1).numpy(), ogr.pool_backward(x, dy, 'bf16').astype(np.float64))


@pytest.mark.parametrize('dtype', oc.DTYPES)
def test_pool_relu_inputs_hold_the_ties(dtype):
    four, two = oc.assert_pool_ties(dtype)
    print('%s: %d four-way ties, %d two-way ties of the maximum that start behind position (0,0)' % (dtype, four, two))


@pytest.mark.parametrize('dtype', oc.DTYPES)
def test_pool_hand_cases(dtype):
    x, dy, want = oc.pool_hand_inputs()
    dx = ogr.pool_backward(x, dy, dtype)
    assert np.array_equal(dx, ogr.pool_backward_loops(x, dy, dtype))
    for i, (label, _, pos) in enumerate(oc.POOL_HAND):
        flat = dx[i].reshape(4, 8)
        assert np.array_equal(flat[pos], dy[i, 0, 0]), label          # (these dy are exact in both storage types)
        assert not np.delete(flat, pos, axis=0).any(), label


@pytest.mark.parametrize('name', ogr.POOL_MUTANTS)
def test_every_pool_mutant_is_killed(name):
    killed = []
    for case in SMALL_POOL:
        for kind in oc.POOL_KINDS:
            x, dy = oc.pool_inputs(kind, case)
            if not np.array_equal(ogr.pool_backward(x, dy, 'bf16', mutant=name), ogr.pool_backward(x, dy, 'bf16')):
                killed.append((case, kind))
    x, dy, _ = oc.pool_hand_inputs()
    if not np.array_equal(ogr.pool_backward(x, dy, 'bf16', mutant=name), ogr.pool_backward(x, dy, 'bf16')):
        killed.append(('hand', 'hand'))
    assert killed, 'pool mutant %s survives every case' % name
    print(name, killed)


# ---------------------------------------------------------------------------------------------------------------------------- k2s2
@pytest.mark.parametrize('case', sorted(oc.K2S2_CASES))
def test_k2s2_reference_is_torch_float64_autograd(case):
    n, h, w, cin, cout, tr = oc.K2S2_CASES[case]
    x, wt, y, dy = oc.k2s2_inputs('gauss', case)
    xs, ws, dz = cgr.seen(x, wt, y, dy, 'bf16', True)
    g = ogr.grads64_k2s2(xs, ws, dz, tr)
    tx = torch.from_numpy(xs.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
    tb = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    if tr:          # torch: [cin, cout, kh, kw]
        tw = torch.from_numpy(ws.astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True)
        out = torch.nn.functional.conv_transpose2d(tx, tw, tb, stride=2)
        back = (2, 3, 1, 0)
    else:           # torch: [cout, cin, kh, kw]
        tw = torch.from_numpy(ws.astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True)
        out = torch.nn.functional.conv2d(tx, tw, tb, stride=2)
        back = (2, 3, 1, 0)
    (out * torch.from_numpy(dz.astype(np.float64)).permute(0, 3, 1, 2)).sum().backward()
    for name, got in (('dx', tx.grad.permute(0, 2, 3, 1).numpy()), ('dw', tw.grad.permute(*back).numpy()), ('db', tb.grad.numpy())):
        assert got.shape == g[name][0].shape, name
        assert np.abs(got - g[name][0]).max() <= 2.0 ** -40 * np.abs(g[name][0]).max(), name


@pytest.mark.parametrize('dtype', oc.DTYPES)
@pytest.mark.parametrize('case', sorted(oc.K2S2_CASES))
def test_k2s2_lattice_conditions_and_reference_inside_its_bounds(case, dtype):
    tr = oc.K2S2_CASES[case][5]
    for kind in oc.KINDS:
        x, wt, y, dy = oc.k2s2_inputs(kind, case)
        for relu in (0, 1):
            xs, ws, dz = cgr.seen(x, wt, y, dy, dtype, relu)
            g = ogr.grads64_k2s2(xs, ws, dz, tr)
            if kind == 'lattice':
                assert np.array_equal(xs, x) and np.array_equal(ws, wt)
                oc.k2s2_assert_lattice(case, wt, g)
                if relu:
                    assert 0.3 < (y == 0).mean() < 0.5
            cgr.check('%s %s relu=%d reference' % (case, kind, relu), cgr.deliver(g, dtype), g, dtype, kind)


def test_k2s2_bound_terms():
    """K as the issue states it: the products behind one element of each output."""
    for case, (n, h, w, cin, cout, tr) in oc.K2S2_CASES.items():
        x, wt, y, dy = oc.k2s2_inputs('lattice', case)
        g = ogr.grads64_k2s2(x, wt, dy, tr)
        want = (4 * cout, n * h * w, 4 * n * h * w) if tr else (cout, n * (h // 2) * (w // 2), n * (h // 2) * (w // 2))
        assert (g['dx'][2], g['dw'][2], g['db'][2]) == want
        assert g['dx'][0].shape == x.shape and g['dw'][0].shape == wt.shape and g['db'][0].shape == (cout,)


@pytest.mark.parametrize('name', ogr.K2S2_MUTANTS)
def test_every_k2s2_mutant_is_killed(name):
    """Under the GPU test's grading (lattice: equality, gauss: ratio <= 1) at least one (case, kind) rejects the mutant; the structural
    mutants must fall to the lattice, the rounding one to the gauss inputs."""
    rounding = name == 'dz_unrounded'
    killed = []
    for case in sorted(oc.K2S2_CASES):
        tr = oc.K2S2_CASES[case][5]
        for kind in oc.KINDS:
            x, wt, y, dy = oc.k2s2_inputs(kind, case)
            out = ogr.k2s2_mutant(name, x, wt, y, dy, 'bf16', 1, tr)
            if out is None:
                continue
            g = ogr.grads64_k2s2(*cgr.seen(x, wt, y, dy, 'bf16', 1), tr)
            tops = cgr.grade(case, dict(zip(('dx', 'dw', 'db'), out)), g, 'bf16', kind, verbose=False)
            if max(tops.values()) > 1.0:
                killed.append((case, kind))
        if killed and (rounding or any(kd == 'lattice' for _, kd in killed)):
            break
    assert killed, 'mutant %s survives every case' % name
    if rounding:
        assert all(kd == 'gauss' for _, kd in killed), killed
    else:
        assert any(kd == 'lattice' for _, kd in killed), 'mutant %s: no lattice case catches it (%s)' % (name, killed)


def test_unmutated_k2s2_passes_the_grading():
    for case in sorted(oc.K2S2_CASES):
        tr = oc.K2S2_CASES[case][5]
        for kind in oc.KINDS:
            x, wt, y, dy = oc.k2s2_inputs(kind, case)
            out = ogr.k2s2_mutant(None, x, wt, y, dy, 'bf16', 1, tr)
            g = ogr.grads64_k2s2(*cgr.seen(x, wt, y, dy, 'bf16', 1), tr)
            cgr.check(case, dict(zip(('dx', 'dw', 'db'), out)), g, 'bf16', kind)


# ------------------------------------------------------------------------------------------------------------- the C ABI, dry run
_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
pool_cases, cases = json.loads(sys.argv[1]), json.loads(sys.argv[2])
fake = lambda i: C.c_void_p((i + 1) << 24)          # device "addresses" nobody dereferences in the dry run
out = {'pool_ok': {}, 'pool_refused': {}, 'bytes': {}, 'bytes2n': {}, 'ok': {}, 'refused': {}}
def pool(n, h, w, c, dtype='bf16', x=fake(1)):
    rc = L.ron_maxpool2x2_backward_nhwc(x, fake(2), n, h, w, c, _lib.DTYPES[dtype], fake(3), None)
    return [rc, L.ron_last_error().decode()]
for name, c in pool_cases.items():
    for dt in ('bf16', 'fp16'):
        out['pool_ok'][name + ' ' + dt] = pool(*c, dtype=dt)[0]
out['pool_refused'] = {'c = 12': pool(1, 4, 4, 12), 'fp32': pool(1, 4, 4, 8, dtype='fp32'), 'h = 0': pool(1, 0, 4, 8),
                       'misaligned pointer': pool(1, 4, 4, 8, x=C.c_void_p((1 << 24) + 4))}
def desc(n, h, w, cin, cout, transpose, k=2, stride=2, rate=1, relu=1, dtype='bf16', pool=0, splitk=-1, tile_cfg=-1):
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, rate, relu, transpose, _lib.DTYPES[dtype], tile_cfg, 0, 0, pool, splitk, 0)
def call(d, ws_bytes, y=True, dy=fake(4)):
    return L.ron_conv2d_k2s2_backward_nhwc(C.byref(d), fake(1), fake(2), fake(3) if y else None, dy, fake(5), fake(6), fake(7), fake(8), ws_bytes, None)
for name, c in cases.items():
    d = desc(*c)
    out['bytes'][name] = L.ron_conv2d_k2s2_backward_workspace_bytes(C.byref(d))
    d2 = desc(2 * c[0], *c[1:])
    out['bytes2n'][name] = L.ron_conv2d_k2s2_backward_workspace_bytes(C.byref(d2))
    for dt in ('bf16', 'fp16'):
        for sk in (-1, 1, 2, 7):
            for relu in (0, 1):
                d = desc(*c, dtype=dt, splitk=sk, relu=relu)
                out['ok']['%%s %%s %%d %%d' %% (name, dt, sk, relu)] = call(d, L.ron_conv2d_k2s2_backward_workspace_bytes(C.byref(d)), y=bool(relu))
b = cases['c_k30']
bad = {
    'odd h': desc(2, 5, 10, 64, 24, 0),
    'k = 3': desc(*b, k=3),
    'stride = 1': desc(*b, stride=1),
    'dilation = 2': desc(*b, rate=2),
    'cin = 96': desc(2, 6, 10, 96, 24, 0),
    'transposed cout = 24': desc(2, 3, 5, 64, 24, 1),
    'fp32': desc(*b, dtype='fp32'),
    'f16x3': desc(*b, dtype='f16x3'),
    'pool': desc(*b, pool=1),
    'tile_cfg': desc(*b, tile_cfg=1),
    'splitk 0': desc(*b, splitk=0),
}
for name, d in bad.items():
    nbytes = L.ron_conv2d_k2s2_backward_workspace_bytes(C.byref(d))
    msg_b = L.ron_last_error().decode()
    rc = call(d, 1 << 40)
    out['refused'][name] = [nbytes, msg_b, rc, L.ron_last_error().decode()]
for name in ('c_k30', 't_k30'):
    d = desc(*cases[name])
    need = L.ron_conv2d_k2s2_backward_workspace_bytes(C.byref(d))
    rc = call(d, need, y=False)
    out['refused']['relu with NULL y ' + name] = [-1, 'x', rc, L.ron_last_error().decode()]
    rc = call(d, need - 1)
    out['refused']['short workspace ' + name] = [-1, 'x', rc, L.ron_last_error().decode()]
    rc = call(d, need, dy=C.c_void_p((5 << 24) + 4))
    out['refused']['misaligned dy ' + name] = [-1, 'x', rc, L.ron_last_error().decode()]
print('RESULT ' + json.dumps(out))
'''


@pytest.fixture(scope='module')
def dry_run():
    """One child process in the library's dry-run mode (RON_PLAN_ONLY=1: every host decision, no HIP call)."""
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    env = dict(os.environ, RON_PLAN_ONLY='1')
    p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(oc.POOL_CASES), json.dumps(oc.K2S2_CASES)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_pool_dry_run(dry_run):
    assert dry_run['pool_ok'] and all(rc == 0 for rc in dry_run['pool_ok'].values()), dry_run['pool_ok']
    for name in ('c = 12', 'fp32', 'misaligned pointer', 'h = 0'):
        rc, msg = dry_run['pool_refused'][name]
        assert rc == -1 and msg, '%s: status %d (%s), RON_ERR_INVALID (-1) expected' % (name, rc, msg)


def test_k2s2_workspace_bytes(dry_run):
    for name in oc.K2S2_CASES:
        b, b2 = dry_run['bytes'][name], dry_run['bytes2n'][name]
        assert b > 0 and b % 256 == 0, (name, b)
        assert b2 > b, 'case %s: the workspace does not grow with n (%d -> %d)' % (name, b, b2)


def test_k2s2_accepted_descriptors_plan_in_the_dry_run(dry_run):
    assert len(dry_run['ok']) == len(oc.K2S2_CASES) * 2 * 4 * 2
    assert all(rc == 0 for rc in dry_run['ok'].values()), {k: v for k, v in dry_run['ok'].items() if v}


def test_k2s2_refusals(dry_run):
    want = ['odd h', 'k = 3', 'stride = 1', 'dilation = 2', 'cin = 96', 'transposed cout = 24', 'fp32', 'f16x3', 'pool', 'tile_cfg', 'splitk 0']
    want += ['%s %s' % (what, case) for what in ('relu with NULL y', 'short workspace', 'misaligned dy') for case in ('c_k30', 't_k30')]
    assert sorted(want) == sorted(dry_run['refused'])
    for name in want:
        nbytes, msg_b, rc, msg = dry_run['refused'][name]
        assert nbytes == -1 and msg_b, (name, nbytes, msg_b)
        assert rc == -1 and msg, '%s: status %d (%s), RON_ERR_INVALID (-1) expected' % (name, rc, msg)
