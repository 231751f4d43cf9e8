"""The references of the SSD-only backward operators, their bounds and mutants, and the argument checks of
ron_maxpool3x3s1_backward_nhwc / ron_l2norm_backward_nhwc / ron_conv2d_padded_backward_nhwc, without a GPU.

  * pool: the scatter and the loop reference agree and equal torch-CPU max_pool2d(3, 1, 1) autograd in both memory formats; the
    relu inputs hold ties whose first maximum is not the window's first position; every mutant falls to a named case;
  * L2 norm: the float64 formulas against the torch-CPU float64 autograd composition x rsqrt(clamp_min(sum x^2, 1e-12)) gamma; the
    lattice is exact; the delivered reference is inside its own bound; every mutant is rejected under the GPU test's grading;
  * padded conv: the scatter identity against torch-CPU float64 autograd of conv2d(pad(x), w, stride); lattice conditions; mutants;
  * the C ABI in the library's dry-run mode: accepted cases plan, workspace bytes are monotone in n, every refusal is -1 + message."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_grad_ref as cgr
import ssd_grad_cases as sc
import ssd_grad_ref as sr

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_POOL = [c for c in sorted(sc.POOL_CASES) if c != 'pool5']


# ------------------------------------------------------------------------------------------------------------------------ the pool
def _pool_small(kind, case):
    x, dy = sc.pool_inputs(kind, case)
    if case == 'pool5':          # the loops are too slow for 512 channels; the rule is per channel
        x, dy = x[..., :8], dy[..., :8]
    return x, dy


@pytest.mark.parametrize('dtype', sc.DTYPES)
@pytest.mark.parametrize('kind', sc.POOL_KINDS)
@pytest.mark.parametrize('case', sorted(sc.POOL_CASES))
def test_pool_references_agree(case, kind, dtype):
    x, dy = _pool_small(kind, case)
    assert np.array_equal(sr.pool3_backward(x, dy, dtype), sr.pool3_backward_loops(x, dy, dtype))


@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('kind', sc.POOL_KINDS)
@pytest.mark.parametrize('case', sorted(sc.POOL_CASES))
def test_pool_reference_is_torch_autograd(case, kind, channels_last):
    """On storage-representable inputs; torch in float32 adds the windows in its own order, so dy is made of small integers, whose
    sums are exact in any order."""
    x, dy = sc.pool_inputs(kind, case)
    xs = cgr.ROUND['bf16'](x)
    g = np.round(dy * 4).astype(np.float32)
    tx = torch.from_numpy(xs).permute(0, 3, 1, 2)
    tx = (tx.contiguous(memory_format=torch.channels_last) if channels_last else tx.contiguous()).requires_grad_(True)
    out = torch.nn.functional.max_pool2d(tx, 3, 1, 1)
    out.backward(torch.from_numpy(g).permute(0, 3, 1, 2))
    assert np.array_equal(tx.grad.permute(0, 2, 3, 1).numpy(), sr.pool3_backward(x, g, 'bf16'))
    assert np.array_equal(out.detach().permute(0, 2, 3, 1).numpy(), sr.pool3_forward(x, 'bf16'))


@pytest.mark.parametrize('dtype', sc.DTYPES)
def test_pool_relu_inputs_hold_late_ties(dtype):
    total = 0
    for case in sc.POOL_CASES:
        if case == 'one':          # a window of one position cannot hold a tie
            continue
        late = sr.pool3_late_ties(sc.pool_inputs('relu', case)[0], dtype)
        coarse = sr.pool3_late_ties(sc.pool_inputs('coarse', case)[0], dtype)
        print('%s %s: tied windows whose first maximum is not their first position: relu %d, coarse %d' % (case, dtype, late, coarse))
        total += late
        assert coarse > 0 or case == 'two', case          # (four positions per channel: the hand windows cover the small map)
    assert total > 0


@pytest.mark.parametrize('dtype', sc.DTYPES)
def test_pool_hand_cases(dtype):
    x, dy = sc.pool_hand_inputs()
    want = sc.pool_hand_expected()
    assert np.array_equal(sr.pool3_backward(x, dy, dtype), want)
    assert np.array_equal(sr.pool3_backward_loops(x, dy, dtype), want)


@pytest.mark.parametrize('name', sr.POOL_MUTANTS)
def test_every_pool_mutant_is_killed(name):
    killed = []
    for case in SMALL_POOL:
        for kind in sc.POOL_KINDS:
            x, dy = sc.pool_inputs(kind, case)
            if not np.array_equal(sr.pool3_backward(x, dy, 'bf16', mutant=name), sr.pool3_backward(x, dy, 'bf16')):
                killed.append((case, kind))
    x, dy = sc.pool_hand_inputs()
    got = sr.pool3_backward(x, dy, 'bf16', mutant=name)
    for i, (label, _, _, _) in enumerate(sc.POOL_HAND):
        if not np.array_equal(got[i], sc.pool_hand_expected()[i]):
            killed.append(('hand', label))
    assert killed, 'pool mutant %s survives every case' % name
    print(name, killed)
    if name == 'padding_is_zero':
        assert ('hand', 'all negative at a corner') in killed
    if name == 'unrounded_compare':
        assert ('hand', 'tie after rounding') in killed


# ------------------------------------------------------------------------------------------------------------- the L2 normalisation
L2_SMALL = [c for c in sorted(sc.L2_CASES) if sc.L2_CASES[c][3] != 512 or int(np.prod(sc.L2_CASES[c][:3])) <= 257]


@pytest.mark.parametrize('case', ['m5_c72', 'm257_c8', 'm4_c512'])
def test_l2_reference_is_the_torch_float64_composition(case):
    x, gamma, dy = sc.l2_inputs('gauss', case)
    xs, dz = sr.l2_seen(x, dy, 'bf16')
    xs[0, 0, 0] = 0          # a clamped pixel too
    ref = sr.l2_backward64(xs, gamma, dz)
    tx = torch.from_numpy(xs.astype(np.float64)).requires_grad_(True)
    tg = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    y = tx * torch.rsqrt(torch.clamp_min((tx * tx).sum(dim=-1, keepdim=True), sr.CLAMP)) * tg
    y.backward(torch.from_numpy(dz.astype(np.float64)))
    assert np.abs(y.detach().numpy() - sr.l2_forward64(xs, gamma)).max() <= 1e-12 * np.abs(y.detach().numpy()).max()
    for name, got in (('dx', tx.grad.numpy()), ('dgamma', tg.grad.numpy())):
        assert np.abs(got - ref[name]).max() <= 1e-12 * np.abs(ref[name]).max(), name
    assert not ref['live'][0, 0, 0] and np.abs(ref['dx'][0, 0, 0] - dz[0, 0, 0] * gamma.astype(np.float64) / np.sqrt(sr.CLAMP)).max() < 1e-3


@pytest.mark.parametrize('case', L2_SMALL)
def test_l2_lattice_is_exact_and_reference_inside_its_bound(case):
    x, gamma, dy = sc.l2_inputs('lattice', case)
    ref = sc.l2_assert_lattice(x, gamma, dy)
    # any summation order: float32, channels reversed and pixels reversed
    u = (x[..., ::-1] * ref['inv'].astype(np.float32))
    t32 = np.zeros(x.shape[:-1] + (1,), np.float32)
    for k in range(x.shape[-1]):
        t32 = t32 + (dy[..., ::-1] * gamma[::-1])[..., k:k + 1] * u[..., k:k + 1]
    assert np.array_equal(t32, ref['t'])
    for dtype in sc.DTYPES:
        xg, gg, dyg = sc.l2_inputs('gauss', case)
        sr.l2_check(case + ' reference', sr.l2_mutant(None, xg, gg, dyg, dtype), xg, gg, dyg, dtype, 'gauss')


def test_l2_bound_lengths():
    assert sr.l2_lengths(1, 8) == (10, 1 + 1 + 8)
    assert sr.l2_lengths(38 * 38, 512) == (14, 1 + 181 + 8)
    assert sr.l2_lengths(4100, 2048) == (38, 3 + 256 + 8)


@pytest.mark.parametrize('name', sr.L2_MUTANTS)
def test_every_l2_mutant_is_killed(name):
    killed = []
    cases = [(k, c) for c in ('m5_c72', 'm257_c8', 'm257_c72') for k in sc.KINDS] + [('dead', 'dead')]
    for kind, case in cases:
        x, gamma, dy = sc.l2_dead_pixel_inputs() if case == 'dead' else sc.l2_inputs(kind, case)
        grade_kind = 'gauss' if case == 'dead' else kind
        tops = sr.l2_grade(case, sr.l2_mutant(name, x, gamma, dy, 'bf16'), x, gamma, dy, 'bf16', grade_kind, verbose=False)
        if max(tops.values()) > 1.0:
            killed.append((case, kind))
    assert killed, 'L2 mutant %s survives every case' % name
    print(name, killed)
    if name in ('clamp_ignored', 'clamped_pixel_projected'):
        assert killed == [('dead', 'dead')]
    elif name == 'dy_unrounded':
        assert all(k != 'lattice' for _, k in killed)
    else:
        assert any(k == 'lattice' for _, k in killed), killed


def test_unmutated_l2_passes_the_grading():
    for kind in sc.KINDS:
        for case in ('m5_c72', 'm257_c8', 'm257_c72'):
            x, gamma, dy = sc.l2_inputs(kind, case)
            sr.l2_check(case, sr.l2_mutant(None, x, gamma, dy, 'bf16'), x, gamma, dy, 'bf16', kind)
    x, gamma, dy = sc.l2_dead_pixel_inputs()
    sr.l2_check('dead', sr.l2_mutant(None, x, gamma, dy, 'bf16'), x, gamma, dy, 'bf16', 'gauss')


# ------------------------------------------------------------------------------------------------------------ the padded convolutions
PADDED_SMALL = [c for c in sorted(sc.PADDED_CASES) if c != 's2_19']


@pytest.mark.parametrize('case', sorted(sc.PADDED_CASES))
def test_padded_reference_is_torch_float64_autograd(case):
    n, h, w, cin, cout, stride, cpad = sc.PADDED_CASES[case]
    x, wt, y, dy = sc.padded_inputs('gauss', case)
    xs, ws, dz = cgr.seen(x, wt, y, dy, 'bf16', True)
    g = sr.grads64_padded(xs, ws, dz, stride, cpad)
    tx = torch.from_numpy(xs.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
    tw = torch.from_numpy(ws.astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True)
    tb = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.conv2d(torch.nn.functional.pad(tx, (cpad,) * 4), tw, tb, stride=stride)
    assert tuple(out.shape[2:]) == sr.out_hw(h, w, stride, cpad) == tuple(dz.shape[1:3])
    (out * torch.from_numpy(dz.astype(np.float64)).permute(0, 3, 1, 2)).sum().backward()
    for name, got in (('dx', tx.grad.permute(0, 2, 3, 1).numpy()), ('dw', tw.grad.permute(2, 3, 1, 0).numpy()), ('db', tb.grad.numpy())):
        assert got.shape == g[name][0].shape, name
        assert np.abs(got - g[name][0]).max() <= 2.0 ** -40 * max(np.abs(g[name][0]).max(), 1e-30), name
    assert (g['dx'][2], g['dw'][2], g['db'][2]) == (9 * cout, n * h * w, n * h * w)          # K of the full-resolution problem


@pytest.mark.parametrize('dtype', sc.DTYPES)
@pytest.mark.parametrize('case', PADDED_SMALL)
def test_padded_lattice_conditions_and_reference_inside_its_bounds(case, dtype):
    for kind in sc.KINDS:
        for relu in (0, 1):
            (x, wt, y, dy), g = sc.padded_reference(kind, case, dtype, relu)
            if kind == 'lattice':
                assert np.array_equal(cgr.ROUND[dtype](x), x)
            cgr.check('%s %s relu=%d reference' % (case, kind, relu), cgr.deliver(g, dtype), g, dtype, kind)


def test_block12_identity():
    """pad2d(1) + 4x4 VALID on a 2x2 map against torch float64 autograd: only the inner 2x2 taps carry a gradient."""
    x, wt, y, dy = sc.block12_inputs('gauss')
    xs, ws, dz = cgr.seen(x, wt, y, dy, 'bf16', True)
    g = sc.block12_grads64(xs, ws, dz)
    tx = torch.from_numpy(xs.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
    tw = torch.from_numpy(ws.astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True)
    out = torch.nn.functional.conv2d(torch.nn.functional.pad(tx, (1, 1, 1, 1)), tw)
    assert tuple(out.shape) == (1, 128, 1, 1)
    (out * torch.from_numpy(dz.astype(np.float64)).permute(0, 3, 1, 2)).sum().backward()
    assert np.abs(tx.grad.permute(0, 2, 3, 1).numpy() - g['dx'][0]).max() <= 1e-12
    dw = tw.grad.permute(2, 3, 1, 0).numpy()
    assert np.abs(dw - g['dw'][0]).max() <= 1e-12
    outer = np.ones((4, 4), bool)
    outer[1:3, 1:3] = False
    assert not dw[outer].any() and dw[1:3, 1:3].any()


@pytest.mark.parametrize('name', sr.PADDED_MUTANTS)
def test_every_padded_mutant_is_killed(name):
    killed = []
    for case in PADDED_SMALL:
        n, h, w, cin, cout, stride, cpad = sc.PADDED_CASES[case]
        for kind in sc.KINDS:
            (x, wt, y, dy), g = sc.padded_reference(kind, case, 'bf16', 1)
            out = sr.padded_mutant(name, x, wt, y, dy, 'bf16', 1, stride, cpad)
            if out is None:
                continue
            tops = cgr.grade(case, out, g, 'bf16', kind, verbose=False)
            if max(tops.values()) > 1.0:
                killed.append((case, kind))
    assert killed, 'padded-conv mutant %s survives every case' % name
    assert any(k == 'lattice' for _, k in killed), killed
    print(name, killed)


# ------------------------------------------------------------------------------------------------------------- the C ABI, dry run
_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
pool_cases, l2_cases, conv_cases = (json.loads(a) for a in sys.argv[1:4])
fake = lambda i: C.c_void_p((i + 1) << 24)          # device "addresses" nobody dereferences in the dry run
odd = lambda i: C.c_void_p(((i + 1) << 24) + 4)
err = lambda: L.ron_last_error().decode()
out = {'pool_ok': {}, 'pool_refused': {}, 'l2_ok': {}, 'l2_bytes': {}, 'l2_refused': {}, 'conv_ok': {}, 'conv_bytes': {}, 'conv_refused': {}}
def pool(n, h, w, c, dtype='bf16', x=fake(1), dx=fake(3)):
    return [L.ron_maxpool3x3s1_backward_nhwc(x, fake(2), n, h, w, c, _lib.DTYPES[dtype], dx, None), err()]
for name, c in pool_cases.items():
    for dt in ('bf16', 'fp16'):
        out['pool_ok'][name + ' ' + dt] = pool(*c, dtype=dt)[0]
out['pool_refused'] = {'c = 12': pool(1, 4, 4, 12), 'c = 0': pool(1, 4, 4, 0), 'fp32': pool(1, 4, 4, 8, dtype='fp32'), 'h = 0': pool(1, 0, 4, 8),
                       'n = 0': pool(0, 4, 4, 8), 'misaligned x': pool(1, 4, 4, 8, x=odd(1)), 'NULL dx': pool(1, 4, 4, 8, dx=None),
                       'beyond 64-bit indexing': pool(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 8)}
def l2b(n, h, w, c, dtype='bf16'):
    return L.ron_l2norm_backward_workspace_bytes(n, h, w, c, _lib.DTYPES[dtype])
def l2(n, h, w, c, dtype='bf16', ws_bytes=None, x=fake(1), dx=fake(4), dgamma=fake(5), ws=fake(6), gamma=fake(2)):
    need = l2b(n, h, w, c, dtype)
    rc = L.ron_l2norm_backward_nhwc(x, gamma, fake(3), n, h, w, c, _lib.DTYPES[dtype], dx, dgamma, ws, need if ws_bytes is None else ws_bytes, None)
    return [rc, err()]
for name, c in l2_cases.items():
    out['l2_bytes'][name] = [l2b(*c), l2b(2 * c[0], *c[1:]), l2b(64 * c[0], *c[1:])]
    for dt in ('bf16', 'fp16'):
        out['l2_ok'][name + ' ' + dt] = [l2(*c, dtype=dt)[0], l2(*c, dtype=dt, dx=None)[0], l2(*c, dtype=dt, dgamma=None)[0]]
def refused_l2(shape, **kw):
    nbytes = l2b(*shape, dtype=kw.get('dtype', 'bf16'))
    msg = err()
    return [nbytes, msg] + l2(*shape, ws_bytes=1 << 40, **kw)
out['l2_refused'] = {'c = 12': refused_l2((1, 4, 4, 12)), 'c = 4096': refused_l2((1, 4, 4, 4096)), 'fp32': refused_l2((1, 4, 4, 8), dtype='fp32'),
                     'w = 0': refused_l2((1, 4, 0, 8)), 'beyond 64-bit indexing': refused_l2((2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 8))}
out['l2_call_refused'] = {'short workspace': l2(1, 4, 4, 8, ws_bytes=l2b(1, 4, 4, 8) - 1), 'NULL workspace': l2(1, 4, 4, 8, ws=None),
                          'misaligned workspace': l2(1, 4, 4, 8, ws=C.c_void_p((7 << 24) + 16)), 'misaligned x': l2(1, 4, 4, 8, x=odd(1)),
                          'misaligned dgamma': l2(1, 4, 4, 8, dgamma=odd(5)), 'NULL gamma': l2(1, 4, 4, 8, gamma=None)}
def desc(n, h, w, cin, cout, stride, cpad=None, k=3, rate=1, relu=1, dtype='bf16', pool=0, splitk=-1, tile_cfg=-1, transpose=0):
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, rate, relu, transpose, _lib.DTYPES[dtype], tile_cfg, 0, 0, pool, splitk, 0)
def cbytes(d, cpad):
    return L.ron_conv2d_padded_backward_workspace_bytes(C.byref(d), cpad)
def call(d, cpad, ws_bytes, y=True, dy=fake(4), ws=fake(8)):
    return L.ron_conv2d_padded_backward_nhwc(C.byref(d), cpad, fake(1), fake(2), fake(3) if y else None, dy, fake(5), fake(6), fake(7), ws, ws_bytes, None)
for name, c in conv_cases.items():
    cpad = c[6]
    out['conv_bytes'][name] = [cbytes(desc(*c), cpad), cbytes(desc(2 * c[0], *c[1:]), cpad)]
    for dt in ('bf16', 'fp16'):
        for sk in (-1, 1, 2, 7):
            for relu in (0, 1):
                d = desc(*c, dtype=dt, splitk=sk, relu=relu)
                out['conv_ok']['%%s %%s %%d %%d' %% (name, dt, sk, relu)] = call(d, cpad, cbytes(d, cpad), y=bool(relu))
b = conv_cases['s2_5x4']
bad = {
    'stride 2 with cpad 0': (desc(*b), 0),
    'stride 1 with cpad 1': (desc(*b[:5], 1), 1),
    'stride 3': (desc(*b[:5], 3), 1),
    'cpad 2': (desc(*b), 2),
    'k = 1': (desc(*b, k=1), 1),
    'k = 4': (desc(*b, k=4), 1),
    'dilation = 2': (desc(*b, rate=2), 1),
    'VALID on a 2x2 map': (desc(1, 2, 2, 64, 64, 1), 0),
    'cin = 96': (desc(2, 5, 4, 96, 128, 2), 1),
    'fp32': (desc(*b, dtype='fp32'), 1),
    'f16x3': (desc(*b, dtype='f16x3'), 1),
    'pool': (desc(*b, pool=1), 1),
    'transpose': (desc(*b, transpose=1), 1),
    'tile_cfg': (desc(*b, tile_cfg=1), 1),
    'splitk 0': (desc(*b, splitk=0), 1),
}
for name, (d, cpad) in bad.items():
    nbytes = cbytes(d, cpad)
    msg_b = err()
    rc = call(d, cpad, 1 << 40)
    out['conv_refused'][name] = [nbytes, msg_b, rc, err()]
for name in ('s2_5x4', 'v_5x5'):
    c = conv_cases[name]
    d = desc(*c)
    need = cbytes(d, c[6])
    out['conv_refused']['relu with NULL y ' + name] = [-1, 'x', call(d, c[6], need, y=False), err()]
    out['conv_refused']['short workspace ' + name] = [-1, 'x', call(d, c[6], need - 1), err()]
    out['conv_refused']['misaligned dy ' + name] = [-1, 'x', call(d, c[6], need, dy=odd(4)), err()]
    out['conv_refused']['misaligned workspace ' + name] = [-1, 'x', call(d, c[6], need, ws=C.c_void_p((9 << 24) + 16)), err()]
# the existing entry point keeps refusing the strided form
d = desc(*b)
out['plain_refuses_stride_2'] = [L.ron_conv2d_backward_workspace_bytes(C.byref(d)), err()]
print('RESULT ' + json.dumps(out))
'''


@pytest.fixture(scope='module')
def dry_run():
    """One child process in the library's dry-run mode (RON_PLAN_ONLY=1: every host decision, no HIP call)."""
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    env = dict(os.environ, RON_PLAN_ONLY='1')
    p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(sc.POOL_CASES), json.dumps(sc.L2_CASES),
                        json.dumps(sc.PADDED_CASES)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_pool_dry_run(dry_run):
    assert len(dry_run['pool_ok']) == 2 * len(sc.POOL_CASES) and all(rc == 0 for rc in dry_run['pool_ok'].values()), dry_run['pool_ok']
    assert len(dry_run['pool_refused']) == 8
    for name, (rc, msg) in dry_run['pool_refused'].items():
        assert rc == -1 and msg.startswith('maxpool3x3 backward'), '%s: status %d (%s), RON_ERR_INVALID (-1) expected' % (name, rc, msg)


def test_l2_dry_run(dry_run):
    assert len(dry_run['l2_ok']) == 2 * len(sc.L2_CASES)
    assert all(rcs == [0, 0, 0] for rcs in dry_run['l2_ok'].values()), dry_run['l2_ok']
    for name, (n, h, w, c) in sc.L2_CASES.items():
        b1, b2, b64 = dry_run['l2_bytes'][name]
        m = n * h * w
        assert b1 == -(-min(m, sr.L2_MAX_WAVES) * c * 4 // 256) * 256 and b1 % 256 == 0, (name, b1)
        assert b1 <= b2 <= b64 and (b64 > b1 or m >= sr.L2_MAX_WAVES), 'case %s: workspace bytes %d -> %d -> %d with n' % (name, b1, b2, b64)
        assert b64 <= -(-sr.L2_MAX_WAVES * c * 4 // 256) * 256          # the table's height is capped
    assert len(dry_run['l2_refused']) == 5 and len(dry_run['l2_call_refused']) == 6
    for name, (nbytes, msg_b, rc, msg) in dry_run['l2_refused'].items():
        assert nbytes == -1 and msg_b.startswith('l2norm backward'), (name, nbytes, msg_b)
        assert rc == -1 and msg.startswith('l2norm backward'), (name, rc, msg)
    for name, (rc, msg) in dry_run['l2_call_refused'].items():
        assert rc == -1 and msg.startswith('l2norm backward'), (name, rc, msg)


def test_padded_workspace_bytes(dry_run):
    for name in sc.PADDED_CASES:
        b, b2 = dry_run['conv_bytes'][name]
        assert b > 0 and b % 256 == 0, (name, b)
        assert b2 > b, 'case %s: the workspace does not grow with n (%d -> %d)' % (name, b, b2)


def test_padded_accepted_descriptors_plan_in_the_dry_run(dry_run):
    assert len(dry_run['conv_ok']) == len(sc.PADDED_CASES) * 2 * 4 * 2
    assert all(rc == 0 for rc in dry_run['conv_ok'].values()), {k: v for k, v in dry_run['conv_ok'].items() if v}


def test_padded_refusals(dry_run):
    want = ['stride 2 with cpad 0', 'stride 1 with cpad 1', 'stride 3', 'cpad 2', 'k = 1', 'k = 4', 'dilation = 2', 'VALID on a 2x2 map',
            'cin = 96', 'fp32', 'f16x3', 'pool', 'transpose', 'tile_cfg', 'splitk 0']
    want += ['%s %s' % (what, case) for what in ('relu with NULL y', 'short workspace', 'misaligned dy', 'misaligned workspace')
             for case in ('s2_5x4', 'v_5x5')]
    assert sorted(want) == sorted(dry_run['conv_refused'])
    for name in want:
        nbytes, msg_b, rc, msg = dry_run['conv_refused'][name]
        assert nbytes == -1 and msg_b, (name, nbytes, msg_b)
        assert rc == -1 and msg, '%s: status %d (%s), RON_ERR_INVALID (-1) expected' % (name, rc, msg)
    nbytes, msg = dry_run['plain_refuses_stride_2']
    assert nbytes == -1 and 'stride' in msg
