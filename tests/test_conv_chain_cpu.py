"""The host side of ron_conv_chain_forward / ron_conv_chain_backward without a GPU: one child process in the library's dry-run mode
(RON_PLAN_ONLY=1: every host decision is made, no HIP call) sizes and plans every case of tests/conv_chain_cases.py in both
directions, walks a table of refusals, and - with RON_PLAN_TRACE - records the launches of each chain beside the launches of the
per-operator entry points for the same layers: the convolution, weight-gradient, weight-pack and column-sum launches must be the
same kernels on the same grids, which is the pin behind "the same bytes as the operators chained"."""
import json
import os
import subprocess
import sys
import tempfile

import pytest

import conv_chain_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import ctypes as C, json, os, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
cases = json.loads(sys.argv[1])
trace = open(os.environ['RON_PLAN_TRACE'], 'a+')
def new_lines():
    out = [ln.split(' args')[0] for ln in trace.read().splitlines()]
    return out
fake = lambda i, off=0: ((i + 1) << 28) + off          # device "addresses" nobody dereferences in the dry run
def desc(shape, layers, dtype='bf16', num_layers=None):
    d = _lib.ChainDesc()
    d.n, d.h, d.w, d.cin = shape
    d.dtype = _lib.DTYPES[dtype]
    d.num_layers = len(layers) if num_layers is None else num_layers
    for i, l in enumerate(layers[:32]):
        d.layers[i] = _lib.ChainLayer(1, 0, 0, 0, 0, 0, 0) if l[0] == 'p' else _lib.ChainLayer(l[7] if len(l) > 7 else 0, l[1], l[2], l[3], l[4], l[5], l[6])
    return d
size = lambda d: L.ron_conv_chain_workspace_bytes(C.byref(d))
def arr(n, base, null=()):
    return (C.c_void_p * 32)(*[None if i in null else fake(base + i) for i in range(n)])
def fwd(d, ws_bytes, x=fake(1), y=fake(2), ws=fake(3), w_null=(), tap_null=(), w=True):
    n = max(d.num_layers, 0)
    return L.ron_conv_chain_forward(C.byref(d), x, arr(32, 100, w_null) if w else None, arr(32, 200), arr(32, 300, tap_null), y, ws, ws_bytes, None)
def bwd(d, ws_bytes, dy=fake(4), dx=fake(5), ws=fake(3), w_null=(), dtaps=True, dw=True, db=True):
    return L.ron_conv_chain_backward(C.byref(d), dy, arr(32, 400) if dtaps else None, arr(32, 100, w_null), dx, arr(32, 500) if dw else None,
                                     arr(32, 600) if db else None, ws, ws_bytes, None)
out = {'bytes': {}, 'bytes2n': {}, 'shapes': {}, 'ok': {}, 'refused': {}, 'trace': {}}
new_lines()
for name, (shape, layers) in cases.items():
    d = desc(shape, layers)
    out['bytes'][name] = size(d)
    out['bytes2n'][name] = size(desc([2 * shape[0]] + shape[1:], layers))
    sh = []
    for i in range(len(layers)):
        s = (C.c_int64 * 4)()
        assert L.ron_conv_chain_shape(C.byref(d), i, s) == 0
        sh.append(list(s))
    out['shapes'][name] = sh
    for dt in ('bf16', 'fp16'):
        d = desc(shape, layers, dt)
        new_lines()
        out['ok']['%%s %%s forward' %% (name, dt)] = fwd(d, size(d))
        tf = new_lines()
        out['ok']['%%s %%s backward' %% (name, dt)] = bwd(d, size(d))
        tb = new_lines()
        out['ok']['%%s %%s backward without dx, dtaps' %% (name, dt)] = bwd(d, size(d), dx=None, dtaps=False)
        out['ok']['%%s %%s backward dx only' %% (name, dt)] = bwd(d, size(d), dw=False, db=False)
        # the per-operator entry points for every convolution layer, at the shape the chain gives it
        n, h, w, c = shape
        of, ob = [], []
        for l in layers:
            if l[0] == 'p':
                h, w = (h + 1) // 2, (w + 1) // 2
                continue
            _, k, rate, cout, relu, bias, tap = l[:7]
            cd = _lib.ConvDesc(n, h, w, c, cout, k, k, 1, rate, relu, 0, _lib.DTYPES[dt], -1, 0, 0, 0, -1, 0)
            new_lines()
            assert L.ron_conv2d_forward_nhwc(C.byref(cd), fake(1), fake(2), fake(3), fake(4), fake(5), L.ron_conv2d_forward_workspace_bytes(C.byref(cd)), None) == 0
            of.append(new_lines())
            assert L.ron_conv2d_backward_nhwc(C.byref(cd), fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), fake(8),
                                              L.ron_conv2d_backward_workspace_bytes(C.byref(cd)), None) == 0
            ob.append(new_lines())
            c = cout
        out['trace']['%%s %%s' %% (name, dt)] = [tf, tb, of, ob]
shape, layers = cases['mini']
c3 = lambda cout, k=3, rate=1, kind=0: ['c', k, rate, cout, 1, 1, 0, kind]
bad = {
    'num_layers 0': desc(shape, layers, num_layers=0),
    'num_layers 33': desc(shape, layers, num_layers=33),
    'unknown kind': desc(shape, [c3(64), c3(64, kind=2)]),
    'cin 96': desc([2, 12, 20, 96], layers),
    'inner cout 24': desc(shape, [c3(24), c3(64)]),
    'k = 5': desc(shape, [c3(64, k=5)]),
    '7x7 at dilation 2': desc(shape, [c3(64, k=7, rate=2)]),
    'dilation 32': desc(shape, [c3(64, rate=32)]),
    'fp32': desc(shape, layers, 'fp32'),
    'f16x3': desc(shape, layers, 'f16x3'),
    'a tapped pool': desc(shape, [c3(64), ['c', 0, 0, 0, 0, 0, 1, 1]]),
    'a tensor reaching 2 GiB': desc([256, 320, 320, 64], [c3(64)]),
}
for name, d in bad.items():
    nbytes = size(d)
    msg_b = L.ron_last_error().decode()
    rc = fwd(d, 1 << 40)
    msg = L.ron_last_error().decode()
    rcb = bwd(d, 1 << 40)
    out['refused'][name] = [nbytes, msg_b, rc, msg, rcb]
d = desc(shape, layers)
need = size(d)
conv0, tap0 = 0, [i for i, l in enumerate(layers) if l[0] == 'c' and l[6]][0]
per_call = {
    'NULL x': lambda: fwd(d, need, x=None),
    'NULL y': lambda: fwd(d, need, y=None),
    'NULL dy': lambda: bwd(d, need, dy=None),
    'NULL w array': lambda: fwd(d, need, w=False),
    'NULL w[i], forward': lambda: fwd(d, need, w_null=(conv0,)),
    'NULL w[i], backward': lambda: bwd(d, need, w_null=(conv0,)),
    'NULL tap of a tapped layer': lambda: fwd(d, need, tap_null=(tap0,)),
    'misaligned x': lambda: fwd(d, need, x=fake(1, 4)),
    'misaligned dy': lambda: bwd(d, need, dy=fake(4, 8)),
    'short workspace, forward': lambda: fwd(d, need - 1),
    'short workspace, backward': lambda: bwd(d, need - 1),
    'misaligned workspace': lambda: fwd(d, need + 128, ws=fake(3, 128)),
    'NULL workspace': lambda: bwd(d, need, ws=None),
}
new_lines()
for name, f in per_call.items():
    rc = f()
    out['refused'][name] = [-1, 'the call only', rc, L.ron_last_error().decode(), -1]
out['launched_by_refusals'] = new_lines()
print('RESULT ' + json.dumps(out))
'''


@pytest.fixture(scope='module')
def dry_run():
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    with tempfile.TemporaryDirectory() as tmp:
        env = {k: v for k, v in os.environ.items() if not k.startswith('RON_')}
        env.update(RON_PLAN_ONLY='1', RON_PLAN_TRACE=os.path.join(tmp, 'trace.txt'))
        p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(cc.CASES)], env=env, capture_output=True, text=True,
                           timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_workspace_bytes(dry_run):
    for name in cc.CASES:
        b, b2 = dry_run['bytes'][name], dry_run['bytes2n'][name]
        assert b > 0 and b % 256 == 0, (name, b)
        assert b2 > b, 'case %s: the workspace does not grow with n (%d -> %d)' % (name, b, b2)


def test_shapes_agree_with_the_cases(dry_run):
    for name in cc.CASES:
        assert [tuple(s) for s in dry_run['shapes'][name]] == cc.shapes(name), name


def test_every_case_plans_in_both_directions(dry_run):
    assert len(dry_run['ok']) == 8 * len(cc.CASES)
    assert all(rc == 0 for rc in dry_run['ok'].values()), {k: v for k, v in dry_run['ok'].items() if v}


# what replaces the fp32 boundary, and what the boundary itself launches: everything else is pinned
_BOUNDARY = ('memset ', 'conv_bwd_pack_halo_kernel', 'unpack_kernel<', 'maxpool2x2_kernel<', 'chain_join_kernel<', 'chain_zero_kernel',
             'chain_pool_bwd_kernel<')


def _pinned(lines):
    return [ln for ln in lines if not ln.startswith(_BOUNDARY)]


@pytest.mark.parametrize('dtype', cc.DTYPES)
@pytest.mark.parametrize('case', sorted(cc.CASES))
def test_layer_launches_are_the_per_operator_launches(dry_run, case, dtype):
    """kernel, grid, block and LDS bytes of every convolution, weight-pack, weight-gradient and column-sum launch of the chain, in
    order, against the per-operator calls layer by layer (the backward in reverse layer order)."""
    tf, tb, of, ob = dry_run['trace']['%s %s' % (case, dtype)]
    convs = sum(1 for l in cc.CASES[case][1] if l != cc.P)
    assert len(of) == len(ob) == convs
    want_f = [ln for layer in of for ln in _pinned(layer)]
    want_b = [ln for layer in reversed(ob) for ln in _pinned(layer)]
    assert len(want_f) >= 3 * convs and len(want_b) >= 5 * convs, 'the per-operator traces are too short to pin anything'
    assert _pinned(tf) == want_f
    assert _pinned(tb) == want_b
    # and the boundary is really gone: one pack (x) and one unpack per delivered tensor in the forward, one unpack (dx) in the backward
    taps = sum(1 for l in cc.CASES[case][1] if l != cc.P and l[6])
    assert sum(ln.startswith('conv_bwd_pack_halo_kernel') for ln in tf) == 1
    assert sum(ln.startswith('unpack_kernel<') for ln in tf) == 1 + taps
    assert sum(ln.startswith('unpack_kernel<') for ln in tb) == 1
    assert sum(ln.startswith('conv_bwd_pack_halo_kernel') for ln in tb) == (1 if cc.CASES[case][1][-1] == cc.P else 0)


REFUSED_DESCRIPTORS = ['num_layers 0', 'num_layers 33', 'unknown kind', 'cin 96', 'inner cout 24', 'k = 5', '7x7 at dilation 2', 'dilation 32',
                       'fp32', 'f16x3', 'a tapped pool', 'a tensor reaching 2 GiB']
REFUSED_CALLS = ['NULL x', 'NULL y', 'NULL dy', 'NULL w array', 'NULL w[i], forward', 'NULL w[i], backward', 'NULL tap of a tapped layer',
                 'misaligned x', 'misaligned dy', 'short workspace, forward', 'short workspace, backward', 'misaligned workspace',
                 'NULL workspace']


@pytest.mark.parametrize('name', REFUSED_DESCRIPTORS + REFUSED_CALLS)
def test_refusals(dry_run, name):
    nbytes, msg_b, rc, msg, rc_bwd = dry_run['refused'][name]
    assert nbytes == -1 and msg_b, (name, nbytes, msg_b)
    assert rc == -1 and msg, '%s: status %d (%s), RON_ERR_INVALID (-1) expected' % (name, rc, msg)
    assert rc_bwd == -1, '%s: the backward returned %d' % (name, rc_bwd)


def test_a_refused_call_launches_nothing(dry_run):
    assert dry_run['launched_by_refusals'] == []
