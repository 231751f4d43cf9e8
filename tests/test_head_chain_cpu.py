"""The host side of ron_head_chain_forward / ron_head_chain_backward without a GPU: one child process in the library's dry-run mode
(RON_PLAN_ONLY=1: every host decision is made, no HIP call) sizes and plans every case of tests/head_chain_cases.py in both
directions, walks a table of refusals and - with RON_PLAN_TRACE - records the launches of each chain beside those of the per-operator
entry points for the same layers: every convolution, weight-pack, weight-gradient, column-sum and batch-normalisation launch must be
the same kernel on the same grid, which is the pin behind "the same bytes as the operators chained".  The convolution chain's entry
points are the same planner and runner: for tests/conv_chain_cases.py both families must write the same trace, arguments included.
nets.ron_vgg_320.head_chains is checked against the variable table of weights.variable_shapes."""
import json
import os
import subprocess
import sys
import tempfile

import pytest

import conv_chain_cases as cc
import head_chain_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import ctypes as C, json, os, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
cases, old_cases = json.loads(sys.argv[1]), json.loads(sys.argv[2])
trace = open(os.environ['RON_PLAN_TRACE'], 'a+')
def new_lines(args=False):
    return [ln if args else ln.split(' args')[0] for ln in trace.read().splitlines()]
fake = lambda i, off=0: ((i + 1) << 28) + off          # device "addresses" nobody dereferences in the dry run
EPS, DECAY = 1e-5, 0.997
def layer(l, **kw):
    if l[0] == 'p':
        f = dict(kind=1)
    elif l[0] == 'c':
        f = dict(kind=0, k=l[1], dilation=l[2], cout=l[3], relu=l[4], has_bias=l[5], tap=l[6])
    elif l[0] == 'b':
        f = dict(kind=2, relu=l[1], eps=EPS, decay=DECAY)
    else:
        f = dict(kind=3, cout=l[1], cout2=l[2], relu=l[3], has_bias=l[4])
    f.update(kw)
    return _lib.HeadChainLayer(**f)
def desc(shape, layers, dtype='bf16', num_layers=None):
    d = _lib.HeadChainDesc()
    d.n, d.h, d.w, d.cin = shape
    d.dtype = _lib.DTYPES[dtype]
    d.num_layers = len(layers) if num_layers is None else num_layers
    for i, l in enumerate(layers[:32]):
        d.layers[i] = l if isinstance(l, _lib.HeadChainLayer) else layer(l)
    return d
size = lambda d: L.ron_head_chain_workspace_bytes(C.byref(d))
def table(null=(), off={}):
    """32 entries with every pointer set (16-byte aligned fakes); null: (layer, name) left NULL; off: (layer, name) -> byte offset"""
    t = (_lib.HeadChainPtrs * 32)()
    for i in range(32):
        for j, name in enumerate(_lib.HEAD_CHAIN_PTRS):
            if (i, name) not in null and name not in null:
                setattr(t[i], name, fake(100 + 20 * i + j, off.get((i, name), 0)))
    return t
def fwd(d, ws_bytes, x=fake(1), y=fake(2), ws=fake(3), p=None):
    return L.ron_head_chain_forward(C.byref(d), x, table() if p is None else p, y, ws, ws_bytes, None)
def bwd(d, ws_bytes, dy=fake(4), dx=fake(5), ws=fake(3), p=None):
    return L.ron_head_chain_backward(C.byref(d), dy, table() if p is None else p, dx, ws, ws_bytes, None)
out = {'bytes': {}, 'bytes2n': {}, 'shapes': {}, 'ok': {}, 'refused': {}, 'trace': {}, 'old': {}}
new_lines()
GRADS = ('dw', 'dbias', 'dw2', 'dbias2', 'dgamma', 'dbeta')
for name, (shape, layers) in cases.items():
    d = desc(shape, layers)
    out['bytes'][name] = size(d)
    out['bytes2n'][name] = size(desc([2 * shape[0]] + shape[1:], layers))
    sh = []
    for i in range(len(layers)):
        s = (C.c_int64 * 4)()
        assert L.ron_head_chain_shape(C.byref(d), i, s) == 0
        sh.append(list(s))
    out['shapes'][name] = sh
    for dt in ('bf16', 'fp16'):
        d = desc(shape, layers, dt)
        new_lines()
        out['ok']['%%s %%s forward' %% (name, dt)] = fwd(d, size(d))
        tf = new_lines()
        out['ok']['%%s %%s backward' %% (name, dt)] = bwd(d, size(d))
        tb = new_lines()
        out['ok']['%%s %%s backward without dx, dtaps' %% (name, dt)] = bwd(d, size(d), dx=None, p=table(null=('dtap',)))
        out['ok']['%%s %%s backward dx only' %% (name, dt)] = bwd(d, size(d), p=table(null=GRADS))
        out['ok']['%%s %%s forward without mean, var, moving' %% (name, dt)] = fwd(d, size(d), p=table(null=('mean', 'var', 'moving_mean', 'moving_var')))
        new_lines()
        # the per-operator entry points for every layer, at the shape the chain gives it: [[forward lines], [backward lines]] per operator
        n, h, w, c = shape
        of, ob = [], []
        def conv_op(k, rate, cout, relu):
            cd = _lib.ConvDesc(n, h, w, c, cout, k, k, 1, rate, relu, 0, _lib.DTYPES[dt], -1, 0, 0, 0, -1, 0)
            assert L.ron_conv2d_forward_nhwc(C.byref(cd), fake(1), fake(2), fake(3), fake(4), fake(5), L.ron_conv2d_forward_workspace_bytes(C.byref(cd)), None) == 0
            f_ = new_lines()
            assert L.ron_conv2d_backward_nhwc(C.byref(cd), fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), fake(8),
                                              L.ron_conv2d_backward_workspace_bytes(C.byref(cd)), None) == 0
            return [f_, new_lines()]
        for l in layers:
            ops = []
            if l[0] == 'p':
                h, w = (h + 1) // 2, (w + 1) // 2
            elif l[0] == 'c':
                ops.append(conv_op(l[1], l[2], l[3], l[4]))
                c = l[3]
            elif l[0] == '2':
                ops.append(conv_op(3, 1, l[1], l[3]))
                ops.append(conv_op(1, 1, l[2], l[3]))
                c = l[1] + l[2]
            else:
                bd = _lib.BnDesc(n, h, w, c, _lib.DTYPES[dt], l[1], EPS, DECAY)
                nb = L.ron_batchnorm_workspace_bytes(C.byref(bd))
                assert L.ron_batchnorm_train_nhwc(C.byref(bd), *([fake(i) for i in range(1, 10)] + [nb, None])) == 0
                f_ = new_lines()
                assert L.ron_batchnorm_backward_nhwc(C.byref(bd), *([fake(i) for i in range(1, 11)] + [nb, None])) == 0
                ops.append([f_, new_lines()])
            of.append([o[0] for o in ops]); ob.append([o[1] for o in ops])
        out['trace']['%%s %%s' %% (name, dt)] = [tf, tb, of, ob]

# the convolution chain through its own entry points and through the head chain's: one planner, one runner, one trace
for name, (shape, layers) in old_cases.items():
    od = _lib.ChainDesc()
    od.n, od.h, od.w, od.cin = shape
    od.dtype, od.num_layers = _lib.DTYPES['bf16'], len(layers)
    for i, l in enumerate(layers):
        od.layers[i] = _lib.ChainLayer(1, 0, 0, 0, 0, 0, 0) if l[0] == 'p' else _lib.ChainLayer(0, l[1], l[2], l[3], l[4], l[5], l[6])
    hd = desc(shape, layers)
    t = table(null=('w2', 'bias2', 'gamma', 'beta', 'moving_mean', 'moving_var', 'mean', 'var', 'dw2', 'dbias2', 'dgamma', 'dbeta'))
    col = lambda name: (C.c_void_p * 32)(*[getattr(t[i], name) for i in range(32)])
    nb = L.ron_conv_chain_workspace_bytes(C.byref(od))
    same_size = nb == size(hd)
    new_lines()
    assert L.ron_conv_chain_forward(C.byref(od), fake(1), col('w'), col('bias'), col('tap'), fake(2), fake(3), nb, None) == 0
    assert L.ron_conv_chain_backward(C.byref(od), fake(4), col('dtap'), col('w'), fake(5), col('dw'), col('dbias'), fake(3), nb, None) == 0
    a = new_lines(args=True)
    assert fwd(hd, nb, p=t) == 0 and bwd(hd, nb, p=t) == 0
    b = new_lines(args=True)
    out['old'][name] = [same_size, len(a), a == b]

shape, layers = cases['cls']
c3 = lambda cout, **kw: layer(['c', 3, 1, cout, 1, 1, 0], **kw)
bn = lambda **kw: layer(['b', 1], **kw)
pr = lambda cout=64, cout2=64, **kw: layer(['2', cout, cout2, 0, 1], **kw)
bad = {
    'a tap on a batch normalisation': desc(shape, [c3(64), bn(tap=1)]),
    'a tap on a pair': desc(shape, [pr(tap=1)]),
    'a pair behind a tap': desc(shape, [c3(64, tap=1), pr()]),
    'cout2 96': desc(shape, [pr(64, 96), bn()]),
    'cout 32 of a pair': desc(shape, [pr(32, 64), bn()]),
    'BN channels 12': desc([2, 6, 10, 12], [bn()]),
    'BN rows above 2^24': desc([1, 4097, 4096, 8], [bn()]),
    'eps negative': desc(shape, [c3(64), bn(eps=-1e-5)]),
    'eps infinite': desc(shape, [c3(64), bn(eps=float('inf'))]),
    'decay 1.5': desc(shape, [c3(64), bn(decay=1.5)]),
    'decay negative': desc(shape, [c3(64), bn(decay=-0.1)]),
    'BN relu 2': desc(shape, [c3(64), bn(relu=2)]),
    'unknown kind 4': desc(shape, [c3(64), layer(['b', 1], kind=4)]),
    'a convolution behind 8 channels': desc([2, 6, 10, 8], [bn(), c3(64)]),
    'num_layers 0': desc(shape, layers, num_layers=0),
    'fp32': desc(shape, layers, 'fp32'),
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
per_call = {
    'NULL x': lambda: fwd(d, need, x=None),
    'NULL y': lambda: fwd(d, need, y=None),
    'NULL dy': lambda: bwd(d, need, dy=None),
    'NULL pointer table, forward': lambda: L.ron_head_chain_forward(C.byref(d), fake(1), None, fake(2), fake(3), need, None),
    'NULL pointer table, backward': lambda: L.ron_head_chain_backward(C.byref(d), fake(4), None, fake(5), fake(3), need, None),
    'NULL w, forward': lambda: fwd(d, need, p=table(null=((0, 'w'),))),
    'NULL w2, forward': lambda: fwd(d, need, p=table(null=((2, 'w2'),))),
    'NULL w2, backward': lambda: bwd(d, need, p=table(null=((2, 'w2'),))),
    'NULL bias2 of a pair with biases': lambda: fwd(d, need, p=table(null=((0, 'bias2'),))),
    'NULL gamma, forward': lambda: fwd(d, need, p=table(null=((1, 'gamma'),))),
    'NULL gamma, backward': lambda: bwd(d, need, p=table(null=((3, 'gamma'),))),
    'NULL beta': lambda: fwd(d, need, p=table(null=((1, 'beta'),))),
    'moving_mean without moving_var': lambda: fwd(d, need, p=table(null=((1, 'moving_var'),))),
    'moving_var without moving_mean': lambda: fwd(d, need, p=table(null=((3, 'moving_mean'),))),
    'misaligned x': lambda: fwd(d, need, x=fake(1, 4)),
    'misaligned dy': lambda: bwd(d, need, dy=fake(4, 8)),
    'misaligned dx': lambda: bwd(d, need, dx=fake(5, 8)),
    'misaligned gamma': lambda: fwd(d, need, p=table(off={(1, 'gamma'): 4})),
    'misaligned moving_var': lambda: fwd(d, need, p=table(off={(1, 'moving_var'): 8})),
    'misaligned mean': lambda: fwd(d, need, p=table(off={(3, 'mean'): 4})),
    'misaligned dgamma': lambda: bwd(d, need, p=table(off={(1, 'dgamma'): 4})),
    'misaligned dbeta': lambda: bwd(d, need, p=table(off={(3, 'dbeta'): 8})),
    'misaligned w2': lambda: fwd(d, need, p=table(off={(0, 'w2'): 2})),
    'misaligned dw2': lambda: bwd(d, need, p=table(off={(2, 'dw2'): 2})),
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

# one-BN chains for a few shapes of the batch-normalisation tests: one lane group, a ragged channel tile, four channel tiles, 200 slices
BN1_DRY = ['bn1_m1', 'bn1_c8_m1027', 'bn1_c72_m67', 'bn1_c1024_m35', 'bn1_scale40']
DRY_CASES = dict(hc.CASES, **{name: hc.BN1[name] for name in BN1_DRY})


@pytest.fixture(scope='module')
def dry_run():
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    with tempfile.TemporaryDirectory() as tmp:
        env = {k: v for k, v in os.environ.items() if not k.startswith('RON_')}
        env.update(RON_PLAN_ONLY='1', RON_PLAN_TRACE=os.path.join(tmp, 'trace.txt'))
        old = {k: v for k, v in cc.CASES.items() if k not in cc.ONE}
        p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(DRY_CASES), json.dumps(old)], env=env, capture_output=True,
                           text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_workspace_bytes(dry_run):
    for name in DRY_CASES:
        b, b2 = dry_run['bytes'][name], dry_run['bytes2n'][name]
        assert b > 0 and b % 256 == 0, (name, b)
        # (every piece is rounded up to 256 bytes: the one-pixel map of bn1_m1 stays inside the rounding)
        assert b2 > b or (name == 'bn1_m1' and b2 == b), 'case %s: the workspace does not grow with n (%d -> %d)' % (name, b, b2)


def test_shapes_agree_with_the_cases(dry_run):
    for name in DRY_CASES:
        assert [tuple(s) for s in dry_run['shapes'][name]] == hc.shapes(name), name


def test_every_case_plans_in_both_directions(dry_run):
    assert len(dry_run['ok']) == 10 * len(DRY_CASES)
    assert all(rc == 0 for rc in dry_run['ok'].values()), {k: v for k, v in dry_run['ok'].items() if v}


# what replaces the fp32 boundary, and what the boundary itself launches: everything else is pinned
_BOUNDARY = ('memset ', 'conv_bwd_pack_halo_kernel', 'unpack_kernel<', 'maxpool2x2_kernel<', 'chain_join_kernel<', 'chain_zero_kernel',
             'chain_pool_bwd_kernel<', 'chain_add_unpack_kernel<', 'bn_copy_stats_kernel')


def _pinned(lines):
    return [ln for ln in lines if not ln.startswith(_BOUNDARY)]


@pytest.mark.parametrize('dtype', hc.DTYPES)
@pytest.mark.parametrize('case', sorted(DRY_CASES))
def test_layer_launches_are_the_per_operator_launches(dry_run, case, dtype):
    """kernel, grid, block and LDS bytes of every convolution, weight-pack, weight-gradient, column-sum and batch-normalisation launch
    of the chain, in order, against the per-operator calls layer by layer (the backward in reverse layer order; a pair's 3x3 branch
    before its 1x1 in both directions)."""
    tf, tb, of, ob = dry_run['trace']['%s %s' % (case, dtype)]
    layers = DRY_CASES[case][1]
    n_ops = sum({'p': 0, 'c': 1, 'b': 1, '2': 2}[l[0]] for l in layers)
    assert sum(len(l) for l in of) == sum(len(l) for l in ob) == n_ops
    want_f = [ln for layer in of for op in layer for ln in _pinned(op)]
    want_b = [ln for layer in reversed(ob) for op in layer for ln in _pinned(op)]
    assert len(want_f) >= 3 * n_ops and len(want_b) >= 3 * n_ops, 'the per-operator traces are too short to pin anything'
    assert _pinned(tf) == want_f
    assert _pinned(tb) == want_b
    bns = sum(1 for l in layers if l[0] == 'b')
    assert sum(ln.startswith('bn_stats_kernel<') for ln in tf) == bns and sum(ln.startswith('(bn_bwd_dx_kernel<') for ln in tb) == bns
    # and the boundary is really gone: one pack per geometry x is read in, one unpack (y), one copy of the statistics per BN
    first_pair = layers[0][0] == '2'
    assert sum(ln.startswith('conv_bwd_pack_halo_kernel') for ln in tf) == (2 if first_pair else 1)
    assert sum(ln.startswith('unpack_kernel<') for ln in tf) == 1
    assert sum(ln.startswith('bn_copy_stats_kernel') for ln in tf) == bns
    assert sum(ln.startswith('unpack_kernel<') for ln in tb) + sum(ln.startswith('chain_add_unpack_kernel<') for ln in tb) == 1
    assert sum(ln.startswith('chain_add_unpack_kernel<') for ln in tb) == (1 if first_pair else 0)
    assert sum(ln.startswith('conv_bwd_pack_halo_kernel') for ln in tb) == (1 if layers[-1][0] in 'pb' else 0)


@pytest.mark.parametrize('case', sorted(k for k in cc.CASES if k not in cc.ONE))
def test_conv_chain_entry_points_are_the_head_chain_without_new_layers(dry_run, case):
    """ron_conv_chain_forward / _backward and ron_head_chain_forward / _backward on the same layers and pointers: the same workspace
    size and the same trace, line for line with every argument digest."""
    same_size, lines, same = dry_run['old'][case]
    assert same_size and lines > 10 and same


REFUSED_DESCRIPTORS = ['a tap on a batch normalisation', 'a tap on a pair', 'a pair behind a tap', 'cout2 96', 'cout 32 of a pair', 'BN channels 12',
                       'BN rows above 2^24', 'eps negative', 'eps infinite', 'decay 1.5', 'decay negative', 'BN relu 2', 'unknown kind 4',
                       'a convolution behind 8 channels', 'num_layers 0', 'fp32']
REFUSED_CALLS = ['NULL x', 'NULL y', 'NULL dy', 'NULL pointer table, forward', 'NULL pointer table, backward', 'NULL w, forward', 'NULL w2, forward',
                 'NULL w2, backward', 'NULL bias2 of a pair with biases', 'NULL gamma, forward', 'NULL gamma, backward', 'NULL beta',
                 'moving_mean without moving_var', 'moving_var without moving_mean', 'misaligned x', 'misaligned dy', 'misaligned dx',
                 'misaligned gamma', 'misaligned moving_var', 'misaligned mean', 'misaligned dgamma', 'misaligned dbeta', 'misaligned w2',
                 'misaligned dw2', 'short workspace, forward', 'short workspace, backward', 'misaligned workspace', 'NULL workspace']
# a word every message of a refusal must hold: it names what was refused
MESSAGE = {'a tap on a batch normalisation': 'tap', 'a tap on a pair': 'tap', 'a pair behind a tap': 'tapped', 'cout2 96': 'cout2',
           'cout 32 of a pair': 'cout 32', 'BN channels 12': 'multiple of 8', 'BN rows above 2^24': '2^24', 'eps negative': 'eps',
           'eps infinite': 'eps', 'decay 1.5': 'decay', 'decay negative': 'decay', 'BN relu 2': 'relu', 'unknown kind 4': 'kind 4',
           'a convolution behind 8 channels': 'cin 8', 'num_layers 0': 'num_layers', 'fp32': 'dtype',
           'moving_mean without moving_var': 'moving_mean and moving_var', 'moving_var without moving_mean': 'moving_mean and moving_var',
           'short workspace, forward': 'workspace', 'short workspace, backward': 'workspace', 'misaligned workspace': '256-byte',
           'misaligned gamma': '16-byte', 'misaligned moving_var': '16-byte', 'misaligned mean': '16-byte', 'misaligned dgamma': '16-byte',
           'misaligned dbeta': '16-byte', 'misaligned w2': '4-byte', 'misaligned dw2': '4-byte', 'NULL gamma, forward': 'gamma',
           'NULL gamma, backward': 'gamma', 'NULL beta': 'beta', 'NULL w2, forward': 'w2', 'NULL w2, backward': 'w2'}


@pytest.mark.parametrize('name', REFUSED_DESCRIPTORS + REFUSED_CALLS)
def test_refusals(dry_run, name):
    nbytes, msg_b, rc, msg, rc_bwd = dry_run['refused'][name]
    assert nbytes == -1 and msg_b, (name, nbytes, msg_b)
    assert rc == -1 and msg, '%s: status %d (%s), RON_ERR_INVALID (-1) expected' % (name, rc, msg)
    assert rc_bwd == -1, '%s: the backward returned %d' % (name, rc_bwd)
    if name in MESSAGE:
        assert MESSAGE[name] in msg, '%s: the message does not say so: %s' % (name, msg)
        assert name in REFUSED_CALLS or MESSAGE[name] in msg_b, '%s: the sizer\'s message does not say so: %s' % (name, msg_b)


def test_a_refused_call_launches_nothing(dry_run):
    assert dry_run['launched_by_refusals'] == []


@pytest.mark.parametrize('variant', ['reducedfc', 'full'])
def test_head_chains_name_every_head_variable_exactly_once(variant):
    """nets.ron_vgg_320.head_chains over the four scales against weights.variable_shapes: every variable of the reverse modules is
    named exactly once, with the shape its layer gives it, and the layer lists are chains the library plans."""
    pytest.importorskip('torch')
    from ron_tensorflow_amd import weights
    from ron_tensorflow_amd.nets import ron_vgg_320 as net
    A, NC = 10, 21
    table = dict(weights.variable_shapes(variant, num_classes=NC, num_anchors=A))
    heads = {k: v for k, v in table.items() if '/reverse_module/' in k}
    assert len(heads) == 37 + 3 * 39          # the top module has no transposed convolution
    c6 = {'full': 4096, 'reducedfc': 1024}[variant]
    seen = []
    for i, layer in enumerate(weights.FEAT_LAYERS):
        chains = net.head_chains(A, NC, layer, top=i == 0)
        assert (chains['left_conv'] is not None) == (i == 0) and (chains['deconv'] is None) == (i == 0)
        for key in ('left_conv', 'deconv'):
            seen += list((chains[key] or {}).values())
        if i == 0:
            assert table[chains['left_conv']['w']] == (2, 2, c6, 512)
        else:
            assert table[chains['deconv']['w']] == (2, 2, 512, 512) and table[chains['deconv']['bias']] == (512,)
        for key in ('left', 'objness', 'cls', 'reg'):
            layers, names = chains[key]
            assert len(layers) == len(names)
            ch = 512 if key != 'left' or i == 0 else (c6 if i < 2 else 512)
            for l, n in zip(layers, names):
                seen += list(n.values())
                if l['kind'] == 'bn':
                    assert sorted(n) == ['beta', 'gamma', 'moving_mean', 'moving_var'] and all(table[v] == (ch,) for v in n.values()), n
                    assert n['moving_var'].endswith('/BatchNorm/moving_variance')
                    continue
                assert table[n['w']] == (3, 3, ch, l['cout']) and ('bias' in n) == l['bias'], n
                assert 'bias' not in n or table[n['bias']] == (l['cout'],)
                if l['kind'] == 'pair':
                    assert table[n['w2']] == (1, 1, ch, l['cout2']) and table[n['bias2']] == (l['cout2'],)
                ch = l['cout'] + l.get('cout2', 0)
            assert ch == {'left': 512, 'objness': 2 * A, 'cls': A * NC, 'reg': 4 * A}[key]
    assert sorted(seen) == sorted(heads), sorted(set(seen) ^ set(heads))
