"""The host side of ron_conv2d_forward_nhwc without a GPU: one child process in the library's dry-run mode (RON_PLAN_ONLY=1: every
host decision is made, no HIP call) sizes and plans every case of tests/conv_fwd_cases.py and walks a table of refusals; and the
widened backward: ron_conv2d_backward_nhwc accepts the 7 x 7 filter at dilation 1 and nothing else new."""
import os
import subprocess
import sys

import pytest

import conv_fwd_cases as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
cases = json.loads(sys.argv[1])
fake = lambda i, off=0: C.c_void_p(((i + 1) << 24) + off)          # device "addresses" nobody dereferences in the dry run
def desc(n, h, w, cin, cout, k, rate, stride=1, transpose=0, relu=1, dtype='bf16', pool=0, splitk=-1, tile_cfg=-1):
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, rate, relu, transpose, _lib.DTYPES[dtype], tile_cfg, 0, 0, pool, splitk, 0)
size = lambda d: L.ron_conv2d_forward_workspace_bytes(C.byref(d))
def call(d, ws_bytes, x=fake(1), w=fake(2), b=fake(3), y=fake(4), ws=fake(5)):
    return L.ron_conv2d_forward_nhwc(C.byref(d), x, w, b, y, ws, ws_bytes, None)
out = {'bytes': {}, 'bytes2n': {}, 'ok': {}, 'refused': {}, 'bwd': {}}
for name, c in cases.items():
    out['bytes'][name] = size(desc(*c))
    out['bytes2n'][name] = size(desc(2 * c[0], *c[1:]))
    for dt in ('bf16', 'fp16'):
        for relu in (0, 1):
            d = desc(*c, relu=relu, dtype=dt)
            out['ok']['%%s %%s relu=%%d' %% (name, dt, relu)] = call(d, size(d))
            out['ok']['%%s %%s relu=%%d no bias' %% (name, dt, relu)] = call(d, size(d), b=None)
b = cases['B'][:7]
bad = {
    'stride 2 with a 3x3': desc(2, 6, 8, 64, 24, 3, 1, stride=2),
    'k = 5': desc(2, 5, 7, 64, 24, 5, 1),
    '7x7 at dilation 2': desc(2, 5, 7, 64, 24, 7, 2),
    'cin 96': desc(2, 5, 7, 96, 24, 3, 1),
    'cin 3 with cout 32': desc(2, 8, 32, 3, 32, 3, 1),
    'pool': desc(*b, pool=1),
    'tile_cfg': desc(*b, tile_cfg=1),
    'splitk = 2': desc(*b, splitk=2),
    'fp32': desc(*b, dtype='fp32'),
    'f16x3': desc(*b, dtype='f16x3'),
    'transpose with cout 64': desc(2, 3, 5, 64, 64, 2, 1, stride=2, transpose=1),
    'odd h at stride 2': desc(2, 5, 8, 64, 24, 2, 1, stride=2),
}
for name, d in bad.items():
    nbytes = size(d)
    msg_b = L.ron_last_error().decode()
    rc = call(d, 1 << 40)
    out['refused'][name] = [nbytes, msg_b, rc, L.ron_last_error().decode()]
# refusals of the call alone: the descriptor is fine (the sizer's column is filled in so that one assertion serves both tables)
d = desc(*b)
need = size(d)
per_call = {
    'short workspace': lambda: call(d, need - 1),
    'misaligned workspace': lambda: call(d, need + 128, ws=fake(5, 128)),
    'misaligned x': lambda: call(d, need, x=fake(1, 4)),
    'NULL x': lambda: call(d, need, x=None),
    'NULL w': lambda: call(d, need, w=None),
    'NULL y': lambda: call(d, need, y=None),
    'NULL workspace': lambda: call(d, need, ws=None),
}
for name, f in per_call.items():
    rc = f()
    out['refused'][name] = [-1, 'the call only', rc, L.ron_last_error().decode()]
stem = desc(*cases['stemrag'][:7])
out['ok']['the stem takes a 4-byte aligned x'] = call(stem, size(stem), x=fake(1, 4))
# the backward: 7 x 7 at dilation 1 is in, 5 x 5 and a dilated 7 x 7 stay out
def bwd(d):
    n = L.ron_conv2d_backward_workspace_bytes(C.byref(d))
    msg = L.ron_last_error().decode()
    rc = L.ron_conv2d_backward_nhwc(C.byref(d), fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), fake(8), max(n, 0), None)
    return [n, msg, rc]
for name, c in json.loads(sys.argv[2]).items():
    for sk in (-1, 1, 3):
        out['bwd']['%%s splitk=%%d' %% (name, sk)] = bwd(desc(*c, splitk=sk))
out['bwd_fc6'] = [bwd(desc(32, 10, 10, 512, 4096, 7, 1, splitk=sk))[0] for sk in (-1, 1, 1000)]
out['bwd_refused'] = {'k = 5': bwd(desc(2, 5, 7, 64, 24, 5, 1)), '7x7 at dilation 2': bwd(desc(2, 5, 7, 64, 24, 7, 2))}
print('RESULT ' + json.dumps(out))
'''


@pytest.fixture(scope='module')
def dry_run():
    import json
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    env = dict(os.environ, RON_PLAN_ONLY='1')
    p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(cf.CASES), json.dumps(cf.K7_GRAD)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_workspace_bytes(dry_run):
    for name in cf.CASES:
        b, b2 = dry_run['bytes'][name], dry_run['bytes2n'][name]
        assert b > 0 and b % 256 == 0, (name, b)
        assert b2 > b, 'case %s: the workspace does not grow with n (%d -> %d)' % (name, b, b2)


def test_accepted_descriptors_plan_in_the_dry_run(dry_run):
    assert len(dry_run['ok']) == 8 * len(cf.CASES) + 1
    assert all(rc == 0 for rc in dry_run['ok'].values()), {k: v for k, v in dry_run['ok'].items() if v}


REFUSED = ['stride 2 with a 3x3', 'k = 5', '7x7 at dilation 2', 'cin 96', 'cin 3 with cout 32', 'pool', 'tile_cfg', 'splitk = 2', 'fp32',
           'f16x3', 'transpose with cout 64', 'odd h at stride 2', 'short workspace', 'misaligned workspace', 'misaligned x', 'NULL x',
           'NULL w', 'NULL y', 'NULL workspace']


@pytest.mark.parametrize('name', REFUSED)
def test_refusals(dry_run, name):
    nbytes, msg_b, rc, msg = dry_run['refused'][name]
    assert nbytes == -1 and msg_b, (name, nbytes, msg_b)
    assert rc == -1 and msg, '%s: status %d (%s), RON_ERR_INVALID (-1) expected' % (name, rc, msg)


def test_backward_accepts_7x7_at_dilation_1(dry_run):
    assert len(dry_run['bwd']) == 3 * len(cf.K7_GRAD)
    for name, (nbytes, msg, rc) in dry_run['bwd'].items():
        assert nbytes > 0 and nbytes % 256 == 0 and rc == 0, (name, nbytes, msg, rc)
    # fc6 of `full` at batch 32: a slab of the weight gradient is 7 * 7 * 512 * 4096 * 4 bytes, so even an absurd forced split keeps
    # the slabs below 2 GiB; by shape it does not split at all (49 taps x 4 x 32 tiles fill the chip)
    by_shape, off, forced = dry_run['bwd_fc6']
    slab = 7 * 7 * 512 * 4096 * 4
    assert 0 < by_shape == off < forced < off + 2 ** 31, dry_run['bwd_fc6']
    assert (forced - off) % slab == 0 and (forced - off) // slab == (2 ** 31 - 1) // slab


def test_backward_still_refuses_5x5_and_a_dilated_7x7(dry_run):
    for name, (nbytes, msg, rc) in dry_run['bwd_refused'].items():
        assert nbytes == -1 and msg and rc == -1, (name, nbytes, msg, rc)
