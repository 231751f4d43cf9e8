"""The argument envelope of the convolution entry points, without a GPU (cases: tests/conv_envelope_cases.py).

  * the float64 reference (conv_bounds.conv_op) at the last value of every field against torch-CPU float64 conv2d / conv_transpose2d;
  * every edge case can fail: the result a kernel with a one-bit-narrower field would give differs from the reference on the lattice
    inputs and leaves the per-element bound on the gauss inputs - a condition on the INPUTS (far taps that only saw the halo would let
    a wrapped kernel pass);
  * through the C ABI in the library's dry-run mode: every edge descriptor plans, every descriptor beyond a limit is RON_ERR_INVALID
    with a message through every entry point, and the child process exits normally (a stride of 0 used to end it with SIGFPE)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_bounds as cb
import conv_envelope_cases as ce
import conv_grad_cases as cg
import conv_grad_ref as gref
from oracle import ron_forward as orf

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = torch.nn.functional


def test_limits_are_the_documented_ones():
    """LIMITS is written once more in include/ron_hip.h (ron_conv_desc), INTEGRATION.md and csrc/conv_mfma.h: the numbers agree."""
    lim = ce.LIMITS
    assert lim['kh'] == lim['kw'] and lim['stride'] == lim['transposed_kernel']
    header = open(os.path.join(ROOT, 'ron_tensorflow_amd', 'csrc', 'conv_mfma.h')).read()
    for name, value in (('kConvMaxFilter', lim['kh'][1]), ('kConvMaxStride', lim['stride'][1]), ('kConvMaxDilation', lim['dilation'][1]),
                        ('kConvMaxPad', lim['cpad'][1])):
        assert 'constexpr int %s = %d;' % (name, value) in header, name
    sentence = 'kh, kw 1 .. %d; stride 1 .. %d; transposed kernel == stride 1 .. %d; dilation 1 .. %d; SAME padding (kh - 1) * dilation / 2 <= %d' % (
        lim['kh'][1], lim['stride'][1], lim['transposed_kernel'][1], lim['dilation'][1], lim['cpad'][1])
    for doc in (os.path.join('include', 'ron_hip.h'), 'INTEGRATION.md', 'DESIGN.md'):
        text = ' '.join(open(os.path.join(ROOT, doc)).read().replace(' * ', ' ').split())
        assert ' '.join(sentence.replace(' * ', ' ').split()) in text, '%s does not state the envelope: %s' % (doc, sentence)
    # every EDGE case sits inside the limits, on the last value of at least one of them
    for name, (n, h, w, cin, cout, k, stride, dilation, transpose) in ce.EDGE.items():
        pad = (k - 1) * dilation // 2 if stride == 1 and not transpose else 0
        assert 1 <= k <= lim['kh'][1] and 1 <= stride <= lim['stride'][1] and 1 <= dilation <= lim['dilation'][1] and pad <= lim['cpad'][1], name
    on_edge = lambda pick: any(pick(*s) for s in ce.EDGE.values())
    assert on_edge(lambda n, h, w, ci, co, k, s, d, t: k == 15 and s == 1) and on_edge(lambda n, h, w, ci, co, k, s, d, t: s == 7 and not t)
    assert on_edge(lambda n, h, w, ci, co, k, s, d, t: s == 7 and t) and on_edge(lambda n, h, w, ci, co, k, s, d, t: d == 31)
    assert on_edge(lambda n, h, w, ci, co, k, s, d, t: (k - 1) * d // 2 == lim['cpad'][1])


# ----------------------------------------------------------------------------------------------------- the reference at the edges
def _torch_op(name, x, wt, b, res):
    n, h, w, cin, cout, k, stride, dilation, transpose = ce.EDGE[name]
    tx = torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 1, 2)
    tb = torch.from_numpy(np.asarray(b, np.float64))
    if transpose:          # [k, k, Cout, Cin] -> torch's [Cin, Cout, k, k]
        y = F.conv_transpose2d(tx, torch.from_numpy(np.asarray(wt, np.float64)).permute(3, 2, 0, 1), tb, stride=stride)
    else:                  # HWIO -> [Cout, Cin, k, k]; odd filters at stride 1: SAME is symmetric
        tw = torch.from_numpy(np.asarray(wt, np.float64)).permute(3, 2, 0, 1)
        y = F.conv2d(tx, tw, tb, stride=stride, padding=(k - 1) * dilation // 2 if stride == 1 else 0, dilation=dilation)
    y = torch.relu(y).permute(0, 2, 3, 1).numpy()
    if res is not None:
        y = np.maximum(y + np.asarray(res, np.float64), 0)
    return y


@pytest.mark.parametrize('kind', ['lattice', 'gauss'])
@pytest.mark.parametrize('name', sorted(ce.EDGE))
def test_reference_is_torch_float64_at_the_edges(name, kind):
    x, wt, b, res = ce.inputs(kind, name)
    ref, S, K = ce.reference(name, x, wt, b, res)
    want = _torch_op(name, x, wt, b, res)
    assert ref.shape == want.shape
    if kind == 'lattice':
        assert np.array_equal(ref, want)
        assert 0 < np.abs(ref).max() < 256 and S.max() <= 2 * 64 + 8 + 8          # the conditions that make every partial sum exact
        if not ce.EDGE[name][8]:
            k, cin, cout = ce.EDGE[name][5], ce.EDGE[name][3], ce.EDGE[name][4]
            cb.assert_lattice([cb.lattice_weights(k, k, cin, cout, draw=d, seed=sum(ce.EDGE[name])) for d in range(ce.draws(name))])
    else:
        assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()
    # ... and the indexing the mutants are built from is the same operation
    assert np.abs(ce.mutant64(None, name, x, wt, b, res) - ref).max() <= 1e-12 * np.abs(ref).max()


def test_one_hot_filter_shifts_the_input():
    """The reference of the GPU test's corner taps: a 15 x 15 filter with one tap returns the input moved by that tap."""
    n, h, w, cin, cout, k, stride, dilation, transpose = ce.EDGE['k15']
    x = ce.inputs('lattice', 'k15')[0]
    for ky, kx in ((0, 0), (0, 14), (14, 0), (14, 14), (7, 7)):
        ref = cb.conv64(x, ce.one_hot_weights(k, cin, cout, ky, kx))
        assert np.array_equal(ref, ce.shifted(x, k, dilation, ky, kx))
        assert (ky, kx) == (7, 7) or (ref.any() and not np.array_equal(ref, x))       # the corner taps do land inside the 8 x 9 map
    assert np.array_equal(ce.shifted(x, k, dilation, 7, 7), x)


# --------------------------------------------------------------------------------------------------------------- every case can fail
@pytest.mark.parametrize('mutant', [m for m in ce.MUTANTS if m is not None])
def test_a_narrower_field_is_caught(mutant):
    name = ce.MUTANTS[mutant]
    for kind in ('lattice', 'gauss'):
        x, wt, b, res = ce.inputs(kind, name)
        if kind == 'lattice':
            ref, S, K = ce.reference(name, x, wt, b, res)
            assert not np.array_equal(ce.mutant64(mutant, name, x, wt, b, res), ref), '%s: the lattice inputs of %s do not see it' % (mutant, name)
            continue
        for dtype in ('fp32', 'bf16', 'fp16', 'f16x3'):
            rnd = {'fp32': lambda a: np.asarray(a, np.float32), 'bf16': orf.round_bf16, 'fp16': orf.round_f16, 'f16x3': orf.round_f16x3}[dtype]
            xs, ws, rs_ = rnd(x), rnd(wt), None if res is None else rnd(res)
            ref, S, K = ce.reference(name, xs, ws, b, rs_)
            top = cb.ratio(ce.mutant64(mutant, name, xs, ws, b, rs_), ref, S, K, dtype).max()
            assert top > 1.0, '%s: the gauss inputs of %s keep it inside the %s bound (%.3f)' % (mutant, name, dtype, top)


@pytest.mark.parametrize('name', sorted(ce.BACKWARD))
def test_backward_cases(name):
    """The backward's reference at dilation 31 is torch autograd's; on the 1 x 1 filter the dilation does not matter; on the 3 x 3 one a
    dilation wrapped to 15 changes dx and dw on both kinds of inputs."""
    shape = ce.BACKWARD[name]
    n, h, w, cin, cout, k, rate = shape
    for kind in cg.KINDS:
        x, wt, y, dy = cg.inputs(kind, shape)
        xs, ws, dz = gref.seen(x, wt, y, dy, 'bf16', True)
        g = gref.grads64(xs, ws, dz, rate)
        if kind == 'lattice':
            cg.assert_lattice(wt, g['dx'][0], g['dw'][0], g['db'][0])
        else:
            tx = torch.from_numpy(xs.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
            tw = torch.from_numpy(ws.astype(np.float64)).permute(3, 2, 0, 1).requires_grad_(True)
            out = F.conv2d(tx, tw, None, padding=(k - 1) * rate // 2, dilation=rate)
            (out * torch.from_numpy(dz.astype(np.float64)).permute(0, 3, 1, 2)).sum().backward()
            for key, got in (('dx', tx.grad.permute(0, 2, 3, 1).numpy()), ('dw', tw.grad.permute(2, 3, 1, 0).numpy())):
                assert np.abs(got - g[key][0]).max() <= 2.0 ** -40 * np.abs(g[key][0]).max(), key
        wrapped = gref.grads64(xs, ws, dz, rate & 15)
        tops = gref.grade(name, {key: wrapped[key][0] for key in ('dx', 'dw')}, g, 'bf16', kind, verbose=False)
        if k == 1:
            assert max(tops.values()) == 0.0
        else:
            assert min(tops.values()) > 1.0, tops


# ------------------------------------------------------------------------------------------------------------- the C ABI, dry run
_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
job = json.loads(sys.argv[1])
fake = lambda i: C.c_void_p((i + 1) << 24)          # device "addresses" nobody dereferences in the dry run
host = (C.c_float * (1 << 22))()                     # host weights / bias (ron_conv2d_nhwc packs them on the host): zeros, 16 MB
hp = C.cast(host, C.c_void_p)
def desc(d, dtype='bf16', tile_cfg=-1, splitk=-1, **over):
    d = dict(d, **over)
    return _lib.ConvDesc(d['n'], d['h'], d['w'], d['cin'], d['cout'], d['kh'], d['kw'], d['stride'], d['dilation'], d['relu'], d['transpose'],
                         _lib.DTYPES[dtype], tile_cfg, 0, 0, d['pool'], splitk, 0)
def said(rc):
    msg = L.ron_last_error().decode()
    L.ron_conv_plan(None, None)                      # leaves "NULL argument" behind: a stale message cannot pass for the next call's
    return [int(rc), '' if msg == stale else msg]
L.ron_conv_plan(None, None)
stale = L.ron_last_error().decode()
out = {'edge': {}, 'taps_inner': {}, 'edge_backward': {}, 'refused': {}}
o4 = (C.c_int32 * 4)()
for name, d in job['edge'].items():
    for dt in ('fp32', 'bf16', 'fp16', 'f16x3'):
        rc = L.ron_conv_plan(C.byref(desc(d, dt)), o4)
        out['edge']['%%s %%s' %% (name, dt)] = [int(rc), list(o4), L.ron_last_error().decode() if rc else '']
for name in job['taps_inner']:
    ok = []
    for cfg in (7, 9):
        if all(L.ron_conv_plan(C.byref(desc(job['edge'][name], dt, tile_cfg=cfg, splitk=1)), o4) == 0 for dt in ('fp32', 'bf16', 'fp16', 'f16x3')):
            ok.append(cfg)
    out['taps_inner'][name] = ok
for name, d in job['backward'].items():
    for dt in ('bf16', 'fp16'):
        for sk in (-1, 2):
            dd = desc(d, dt, splitk=sk)
            nbytes = L.ron_conv2d_backward_workspace_bytes(C.byref(dd))
            rc = L.ron_conv2d_backward_nhwc(C.byref(dd), fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), fake(8), max(nbytes, 0), None)
            out['edge_backward']['%%s %%s %%d' %% (name, dt, sk)] = [int(nbytes), int(rc)]
for name, d in job['refused'].items():
    r = {}
    assert abs(d['kh'] * d['kw'] * d['cin'] * d['cout']) <= len(host)      # what a library that does NOT refuse it would read
    r['ron_conv_plan'] = said(L.ron_conv_plan(C.byref(desc(d)), o4))
    r['ron_conv2d_nhwc'] = said(L.ron_conv2d_nhwc(C.byref(desc(d)), fake(1), hp, hp, None, fake(2), None))
    if not d['transpose'] and d['stride'] == 1:          # the entries for plain stride-1 convolutions; pool2 wants `pool` set
        dp = desc(d, pool=d['pool'] if d['pool'] != 0 else 1)
        r['ron_conv2d_pool2_nhwc'] = said(L.ron_conv2d_pool2_nhwc(C.byref(dp), fake(1), hp, hp, fake(2), fake(3), None))
        r['ron_conv2d_heads_nhwc'] = said(L.ron_conv2d_heads_nhwc(C.byref(desc(d)), 6, fake(1), hp, hp, fake(2), fake(3), None))
    ms = C.c_float(0)
    r['ron_conv2d_bench'] = said(L.ron_conv2d_bench(C.byref(desc(d)), 0, 1, C.byref(ms)))
    for fam in ('ron_conv2d_backward', 'ron_conv2d_k2s2_backward'):
        r[fam + '_workspace_bytes'] = said(getattr(L, fam + '_workspace_bytes')(C.byref(desc(d))))
        r[fam + '_nhwc'] = said(getattr(L, fam + '_nhwc')(C.byref(desc(d)), fake(1), fake(2), fake(3), fake(4), fake(5), fake(6), fake(7), fake(8), 1 << 40, None))
    out['refused'][name] = r
print('RESULT ' + json.dumps(out))
'''


def run_child(job, timeout=300):
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    env = dict(os.environ, RON_PLAN_ONLY='1')
    return subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(job)], env=env, capture_output=True, text=True, timeout=timeout)


def the_job():
    refused = {name: ce.descriptor(over) for name, over in list(ce.REFUSED.items()) + list(ce.REFUSED_K2S2.items())}
    backward = {name: dict(n=s[0], h=s[1], w=s[2], cin=s[3], cout=s[4], kh=s[5], kw=s[5], stride=1, dilation=s[6], relu=1, transpose=0, pool=0)
                for name, s in ce.BACKWARD.items()}
    return {'edge': {name: ce.edge_descriptor(name) for name in ce.EDGE}, 'taps_inner': sorted(ce.TAPS_INNER), 'backward': backward, 'refused': refused}


@pytest.fixture(scope='module')
def dry_run():
    """One child process in the library's dry-run mode (RON_PLAN_ONLY=1: every host decision, no HIP call)."""
    p = run_child(the_job())
    assert p.returncode == 0, 'the child ended with status %d (negative: a signal)\n%s%s' % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_edge_descriptors_plan(dry_run):
    bad = {k: v for k, v in dry_run['edge'].items() if v[0] != 0}
    assert len(dry_run['edge']) == 4 * len(ce.EDGE) and not bad, bad
    bad = {k: v for k, v in dry_run['edge_backward'].items() if v[0] <= 0 or v[1] != 0}
    assert len(dry_run['edge_backward']) == 4 * len(ce.BACKWARD) and not bad, bad


def test_taps_innermost_table(dry_run):
    """The tile configurations the GPU test forces are the ones the planner accepts for those shapes."""
    assert dry_run['taps_inner'] == {k: list(v) for k, v in ce.TAPS_INNER.items()}


def test_descriptors_beyond_the_envelope_are_refused(dry_run):
    """RON_ERR_INVALID (-1) and a message of its own from every entry point the descriptor was handed to."""
    accepted = []
    for name in list(ce.REFUSED) + list(ce.REFUSED_K2S2):
        calls = dry_run['refused'][name]
        for entry in ('ron_conv_plan', 'ron_conv2d_nhwc', 'ron_conv2d_bench', 'ron_conv2d_backward_workspace_bytes', 'ron_conv2d_backward_nhwc',
                      'ron_conv2d_k2s2_backward_workspace_bytes', 'ron_conv2d_k2s2_backward_nhwc'):
            assert entry in calls, (name, entry)
        d = ce.descriptor(dict(ce.REFUSED, **ce.REFUSED_K2S2)[name])
        assert ('ron_conv2d_pool2_nhwc' in calls and 'ron_conv2d_heads_nhwc' in calls) == (not d['transpose'] and d['stride'] == 1), name
        for entry, (rc, msg) in sorted(calls.items()):
            if rc != -1 or not msg:
                accepted.append('%-28s %-40s -> %d %s' % (name, entry, rc, msg or '(no message)'))
    assert not accepted, 'accepted, or refused without a message:\n' + '\n'.join(accepted)
