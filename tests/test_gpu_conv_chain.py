"""GPU tests of the convolution chain (ron_conv_chain_forward / ron_conv_chain_backward, ops.conv_chain_*).

  * the same bytes - y, every tap, dx, every dw, every db - as the same layers chained through ops.conv2d_nhwc_fn and
    ops.maxpool2x2_nhwc_fn and torch.autograd, for every case of tests/conv_chain_cases.py, bf16 and fp16, on Gaussian inputs.  The
    per-operator functions are the reference: each is pinned per element against float64 by its own tests, so no tolerance appears here;
  * the one-layer chains on the integer lattices of tests/conv_grad_cases.py EQUAL the exact float64 result of tests/conv_grad_ref.py,
    so that the chain is not graded against this library alone;
  * the contract: outputs fully overwritten, nothing assumed about the workspace, nothing written outside it, NULL outputs leave the
    others unchanged, the backward repeatable, NULL dtaps == zero dtaps, nothing cached between calls, the autograd function equal to
    the explicit calls, and all work on the caller's stream without a host synchronisation."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_bounds as cb  # noqa: E402
import conv_chain_cases as cc  # noqa: E402
import conv_grad_cases as cg  # noqa: E402
import conv_grad_ref as ref  # noqa: E402
import stream_util as su  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def side(dev):
    return su.independent_stream(dev, 0)


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ups(arrays, dev):
    return [_up(a, dev) for a in arrays]


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(case, seed=0):
    return cc.inputs(case, seed)


_REFERENCE = {}


def _reference(ops, dev, case, dtype):
    """The layers chained through the per-operator autograd functions: {'y', 'taps', 'dx', 'dw', 'db'} as numpy arrays (lists with one
    entry per layer), computed once per (case, dtype) and shared by the tests that use it (never modified)."""
    if (case, dtype) in _REFERENCE:
        return _REFERENCE[(case, dtype)]
    x, ws, bs, dy, dtaps = _inputs(case)
    layers = cc.layer_dicts(case)
    xt = _up(x, dev).requires_grad_(True)
    wt = [None if w is None else _up(w, dev).requires_grad_(True) for w in ws]
    bt = [None if b is None else _up(b, dev).requires_grad_(True) for b in bs]
    a, taps = xt, [None] * len(layers)
    for i, l in enumerate(layers):
        if l['kind'] == 'pool':
            a = ops.maxpool2x2_nhwc_fn(a, dtype=dtype)
        else:
            a = ops.conv2d_nhwc_fn(a, wt[i], bt[i], relu=l['relu'], dilation=l['dilation'], dtype=dtype)
            if l['tap']:
                taps[i] = a
    roots, grads = [a], [_up(dy, dev)]
    for i, g in enumerate(dtaps):
        if g is not None:
            roots.append(taps[i])
            grads.append(_up(g, dev))
    torch.autograd.backward(roots, grads)
    out = {'y': _np(a), 'taps': [_np(t) for t in taps], 'dx': _np(xt.grad), 'dw': [None if w is None else _np(w.grad) for w in wt],
           'db': [None if b is None else _np(b.grad) for b in bt]}
    _REFERENCE[(case, dtype)] = out
    return out


def _chain(ops, dev, case, dtype, dtaps='given', **kw):
    """The explicit calls on fresh tensors: the same dictionary as _reference, and the tensors for a second call."""
    x, ws, bs, dy, dt = _inputs(case)
    layers = cc.layer_dicts(case)
    xt, wt, bt = _up(x, dev), _ups(ws, dev), _ups(bs, dev)
    y, taps, wsp = ops.conv_chain_forward(xt, layers, wt, bt, dtype=dtype)
    dtl = _ups(dt, dev) if dtaps == 'given' else dtaps
    dx, dws, dbs = ops.conv_chain_backward(xt.shape, layers, wt, _up(dy, dev), dtl, wsp, dtype=dtype, **kw)
    out = {'y': _np(y), 'taps': [_np(t) for t in taps], 'dx': _np(dx), 'dw': [_np(t) for t in dws], 'db': [_np(t) for t in dbs]}
    return out, (xt, wt, bt, layers, wsp)


def _flat(out):
    return [('y', out['y']), ('dx', out['dx'])] + [('%s[%d]' % (k, i), a) for k in ('taps', 'dw', 'db') for i, a in enumerate(out[k])]


def _assert_same(tag, got, want, skip=()):
    for (name, a), (_, b) in zip(_flat(got), _flat(want)):
        if name in skip:
            continue
        assert (a is None) == (b is None), '%s: %s is %s' % (tag, name, 'missing' if a is None else 'unexpected')
        if a is not None:
            assert a.shape == b.shape, '%s: %s has shape %s, %s expected' % (tag, name, a.shape, b.shape)
            assert a.tobytes() == b.tobytes(), '%s: %s differs in %d of %d elements (largest difference %g)' % (
                tag, name, int((a != b).sum()), a.size, float(np.abs(a - b).max()))


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('dtype', cc.DTYPES)
@pytest.mark.parametrize('case', sorted(cc.CASES))
def test_chain_equals_the_operators_chained(ops, dev, case, dtype):
    want = _reference(ops, dev, case, dtype)
    got, (xt, wt, bt, layers, wsp) = _chain(ops, dev, case, dtype)
    assert got['y'].shape == cc.shapes(case)[-1] and np.isfinite(got['y']).all() and got['y'].any() and got['dx'].any()
    _assert_same('%s %s' % (case, dtype), got, want)


@pytest.mark.parametrize('dtype', cc.DTYPES)
@pytest.mark.parametrize('name', sorted(cg.CASES))
def test_one_layer_on_the_lattice_equals_the_exact_result(ops, dev, name, dtype):
    """x, w, dy of conv_grad_cases' lattice through a one-layer chain (ReLU, no bias): y is the rounded exact convolution, and dx, dw,
    db EQUAL conv_grad_ref's float64 gradients under the mask of the EXACT forward (numpy), not of this library's."""
    n, h, w, cin, cout, k, rate = cg.CASES[name]
    x, wt, _, dy = cg.inputs('lattice', name)
    y64 = cb.conv_op(x, wt, None, rate=rate, relu=True)[0]
    assert np.array_equal(y64, np.round(y64)) and np.abs(y64).max() < 2 ** 24 and (y64 == 0).any() and (y64 > 0).any()
    g = ref.grads64(*ref.seen(x, wt, y64.astype(np.float32), dy, dtype, 1), rate)
    cg.assert_lattice(wt, g['dx'][0], g['dw'][0], g['db'][0])
    layers = [ops.chain_conv(cout, k=k, dilation=rate, relu=True, bias=False)]
    xt, wd = _up(x, dev), _up(wt, dev)
    y, _, wsp = ops.conv_chain_forward(xt, layers, [wd], [None], dtype=dtype)
    assert np.array_equal(_np(y), ref.ROUND[dtype](y64.astype(np.float32)))
    dx, dws, dbs = ops.conv_chain_backward(xt.shape, layers, [wd], _up(dy, dev), None, wsp, dtype=dtype, need_db=[True])
    ref.check('one-layer chain %s %s' % (name, dtype), {'dx': _np(dx), 'dw': _np(dws[0]), 'db': _np(dbs[0])}, g, dtype, 'lattice')


# ------------------------------------------------------------------------------------------------------------------ contract
def _raw(case, dtype, T, ws, fill=float('nan'), dx=True, skip_dw=(), skip_db=(), dtaps=True, forward=True, backward=True):
    """The C entries with caller-made, pre-filled outputs and a caller-made workspace; T = (x, weights, biases, dy, dtaps) on the GPU."""
    from ron_tensorflow_amd import _lib
    from ron_tensorflow_amd import ops
    x, wt, bt, dy, dt = T
    layers = cc.layer_dicts(case)
    L = len(layers)
    shapes = cc.shapes(case)
    d = ops._chain_desc(x.shape[0], x.shape[1], x.shape[2], x.shape[3], layers, dtype)
    assert 0 < _lib.lib().ron_conv_chain_workspace_bytes(C.byref(d)) <= ws.numel()
    new = lambda shape: torch.full(tuple(shape), fill, dtype=torch.float32, device=x.device)
    out = {'y': None, 'taps': [None] * L, 'dx': None, 'dw': [None] * L, 'db': [None] * L}
    P = ops._chain_ptrs
    if forward:
        out['y'] = new(shapes[-1])
        out['taps'] = [new(shapes[i]) if l['tap'] else None for i, l in enumerate(layers)]
        _lib.check(_lib.lib().ron_conv_chain_forward(C.byref(d), _lib.ptr(x), P(wt, L), P(bt, L), P(out['taps'], L), _lib.ptr(out['y']),
                                                     _lib.ptr(ws), int(ws.numel()), _lib.current_stream()))
    if backward:
        out['dx'] = new(x.shape) if dx else None
        out['dw'] = [new(w.shape) if w is not None and i not in skip_dw else None for i, w in enumerate(wt)]
        out['db'] = [new((l['cout'],)) if l['kind'] == 'conv' and i not in skip_db else None for i, l in enumerate(layers)]
        _lib.check(_lib.lib().ron_conv_chain_backward(C.byref(d), _lib.ptr(dy), P(dt, L) if dtaps else None, P(wt, L), _lib.ptr(out['dx']),
                                                      P(out['dw'], L), P(out['db'], L), _lib.ptr(ws), int(ws.numel()), _lib.current_stream()))
    return {k: [_np(t) for t in v] if isinstance(v, list) else _np(v) for k, v in out.items()}


def _tensors(case, dev, seed=0):
    x, ws, bs, dy, dt = _inputs(case, seed)
    return _up(x, dev), _ups(ws, dev), _ups(bs, dev), _up(dy, dev), _ups(dt, dev)


def _need(ops, case, dtype):
    (n, h, w, c), _ = cc.CASES[case]
    return ops.conv_chain_workspace_bytes(n, h, w, c, cc.layer_dicts(case), dtype=dtype)


@pytest.mark.parametrize('case', ['mini', 'odd', 'pools'])
def test_workspace_and_output_contract(ops, dev, case):
    """Outputs pre-filled with NaN come back without one; a workspace of 0xFF bytes, of float32 NaNs and of 16-bit NaNs gives the bytes
    a zeroed one gives; carved at exactly the sizer's length out of a larger buffer, the bytes in front of and behind it are
    untouched."""
    T = _tensors(case, dev)
    need = _need(ops, case, 'bf16')
    guard = 4096
    big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    ws = big[guard:guard + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    want = _reference(ops, dev, case, 'bf16')
    fills = {'zero': lambda: ws.zero_(), '0xFF': lambda: ws.fill_(0xFF),
             'fp32 NaN': lambda: ws[:need // 4 * 4].view(torch.int32).fill_(0x7FC00000),
             '16-bit NaN': lambda: ws[:need // 2 * 2].view(torch.int16).fill_(0x7FC0),
             'fp16 NaN': lambda: ws[:need // 2 * 2].view(torch.int16).fill_(0x7E00)}
    for name, fill in fills.items():
        fill()
        got = _raw(case, 'bf16', T, ws)
        for n_, a in _flat(got):
            assert a is None or not np.isnan(a).any(), 'workspace of %s: %d NaN survive in %s' % (name, int(np.isnan(a).sum()), n_)
        _assert_same('workspace of %s' % name, got, want)
    edges = torch.cat([big[:guard], big[guard + need:]]).cpu().numpy()
    assert (edges == 0xA5).all(), 'bytes outside the workspace were written'


def test_null_outputs_leave_the_others_unchanged(ops, dev):
    case = 'mini'
    T = _tensors(case, dev)
    ws = torch.empty((_need(ops, case, 'bf16'),), dtype=torch.uint8, device=dev)
    want = _reference(ops, dev, case, 'bf16')
    _raw(case, 'bf16', T, ws, backward=False)
    got = _raw(case, 'bf16', T, ws, forward=False, dx=False)
    assert got['dx'] is None
    _assert_same('dx NULL', got, want, skip=('y', 'dx') + tuple('taps[%d]' % i for i in range(7)))
    convs = [i for i, l in enumerate(cc.layer_dicts(case)) if l['kind'] == 'conv']
    for i in convs:
        for key, kw in (('dw', {'skip_dw': (i,)}), ('db', {'skip_db': (i,)})):
            got = _raw(case, 'bf16', T, ws, forward=False, **kw)
            assert got[key][i] is None
            _assert_same('%s[%d] NULL' % (key, i), got, want, skip=('y', '%s[%d]' % (key, i)) + tuple('taps[%d]' % j for j in range(7)))
    # nothing but the last layer's gradients: everything in front of it is skipped, dw and db of the last layer are unchanged
    last = convs[-1]
    got = _raw(case, 'bf16', T, ws, forward=False, dx=False, skip_dw=convs[:-1], skip_db=convs[:-1])
    assert got['dw'][last].tobytes() == want['dw'][last].tobytes() and got['db'][last].tobytes() == want['db'][last].tobytes()


@pytest.mark.parametrize('case', ['mini', 'alltaps', 'pools'])
def test_backward_twice_and_null_dtaps_equal_zero_dtaps(ops, dev, case):
    T = _tensors(case, dev)
    ws = torch.empty((_need(ops, case, 'bf16'),), dtype=torch.uint8, device=dev)
    _raw(case, 'bf16', T, ws, backward=False)
    a = _raw(case, 'bf16', T, ws, forward=False)
    b = _raw(case, 'bf16', T, ws, forward=False)
    _assert_same('second backward', b, a)
    _assert_same('backward', a, _reference(ops, dev, case, 'bf16'), skip=('y',) + tuple('taps[%d]' % j for j in range(7)))
    # no dtaps at all (the array NULL), NULL entries, and zero tensors: the same bytes
    shapes, layers = cc.shapes(case), cc.layer_dicts(case)
    zeros = [torch.zeros(shapes[i], dtype=torch.float32, device=dev) if l['tap'] else None for i, l in enumerate(layers)]
    none = _raw(case, 'bf16', T, ws, forward=False, dtaps=False)
    nulls = _raw(case, 'bf16', T[:4] + ([None] * len(layers),), ws, forward=False)
    zero = _raw(case, 'bf16', T[:4] + (zeros,), ws, forward=False)
    _assert_same('NULL entries', nulls, none)
    _assert_same('zero dtaps', zero, none)
    if any(l['tap'] for l in layers):
        assert none['dx'].tobytes() != a['dx'].tobytes(), 'the tap gradients change nothing: the test cannot fail'


def test_nothing_is_cached_between_calls(ops, dev):
    """After the weights changed IN PLACE (the same pointers, as the optimizer leaves them) the forward and backward in the same
    workspace follow the new weights: the bytes of a first call on fresh tensors holding the new values."""
    case = 'odd'
    T = _tensors(case, dev)
    ws = torch.empty((_need(ops, case, 'bf16'),), dtype=torch.uint8, device=dev)
    first = _raw(case, 'bf16', T, ws)
    for w in T[1]:
        if w is not None:
            w.mul_(-1.5)
    second = _raw(case, 'bf16', T, ws)
    assert second['y'].tobytes() != first['y'].tobytes()
    fresh_T = (T[0].clone(), [None if w is None else w.clone() for w in T[1]], T[2], T[3], T[4])
    fresh = _raw(case, 'bf16', fresh_T, torch.zeros_like(ws))
    _assert_same('after the in-place change', second, fresh)


@pytest.mark.parametrize('case', ['mini', 'pools'])
def test_autograd_function_equals_the_explicit_calls(ops, dev, case):
    want = _reference(ops, dev, case, 'bf16')
    x, ws, bs, dy, dt = _inputs(case)
    layers = cc.layer_dicts(case)
    xt = _up(x, dev).requires_grad_(True)
    wt = [None if w is None else _up(w, dev).requires_grad_(True) for w in ws]
    bt = [None if b is None else _up(b, dev).requires_grad_(True) for b in bs]
    outs = ops.conv_chain_fn(xt, layers, wt, bt, dtype='bf16')
    tapped = [i for i, l in enumerate(layers) if l['tap']]
    assert len(outs) == 1 + len(tapped)
    torch.autograd.backward(list(outs), [_up(dy, dev)] + [_up(dt[i], dev) for i in tapped])
    taps = [None] * len(layers)
    for i, t in zip(tapped, outs[1:]):
        taps[i] = _np(t)
    got = {'y': _np(outs[0]), 'taps': taps, 'dx': _np(xt.grad), 'dw': [None if w is None else _np(w.grad) for w in wt],
           'db': [None if b is None else _np(b.grad) for b in bt]}
    _assert_same('conv_chain_fn %s' % case, got, want)
    # needs_input_grad: no gradient for x and for the first convolution's weight -> none computed, the others unchanged
    conv0 = [i for i, l in enumerate(layers) if l['kind'] == 'conv'][0]
    x2 = _up(x, dev)
    w2 = [None if w is None else _up(w, dev).requires_grad_(i != conv0) for i, w in enumerate(ws)]
    b2 = [None if b is None else _up(b, dev).requires_grad_(True) for b in bs]
    outs = ops.conv_chain_fn(x2, layers, w2, b2, dtype='bf16')
    torch.autograd.backward(list(outs), [_up(dy, dev)] + [_up(dt[i], dev) for i in tapped])
    assert x2.grad is None and w2[conv0].grad is None
    for i, w in enumerate(w2):
        if w is not None and i != conv0:
            assert _np(w.grad).tobytes() == want['dw'][i].tobytes(), 'dw[%d]' % i
    for i, b in enumerate(b2):
        if b is not None:
            assert _np(b.grad).tobytes() == want['db'][i].tobytes(), 'db[%d]' % i


# ------------------------------------------------------------------------------------------------------------------ stream contract
def _late_setup(ops, dev, case='mini'):
    layers = cc.layer_dicts(case)

    def flat(T):
        x, wt, bt, dy, dt = T
        return [x] + [t for t in wt if t is not None] + [t for t in bt if t is not None] + [dy] + [t for t in dt if t is not None]

    def unflat(ts, like):
        it = iter(ts)
        x = next(it)
        wt = [None if t is None else next(it) for t in like[1]]
        bt = [None if t is None else next(it) for t in like[2]]
        dy = next(it)
        dt = [None if t is None else next(it) for t in like[4]]
        return x, wt, bt, dy, dt

    given, poison = _tensors(case, dev, 0), _tensors(case, dev, 1)          # two valid sets of values of the same shapes

    def entry(ts):
        x, wt, bt, dy, dt = unflat(ts, given)
        y, taps, wsp = ops.conv_chain_forward(x, layers, wt, bt, dtype='bf16')
        dx, dws, dbs = ops.conv_chain_backward(x.shape, layers, wt, dy, dt, wsp, dtype='bf16')
        return [y, dx] + [t for t in taps + dws + dbs if t is not None]
    real = flat(given)
    expected = [t.clone() for t in entry(real)]
    bufs = [t.clone() for t in flat(poison)]
    poisoned = [t.clone() for t in entry(bufs)]
    torch.cuda.synchronize()
    assert not su.same_bytes(expected, poisoned)

    def fill():
        for b, t in zip(bufs, real):
            b.copy_(t, non_blocking=True)
    return entry, real, bufs, expected, fill


def _clones(tensors):
    return [t.clone() for t in tensors]


def test_stream_contract_late_inputs(ops, dev, side):
    """On a stalled side stream, with x, every w and bias, dy and every dtap copied into their buffers behind the stall: neither call
    waits for the host and neither reads anything early - not the weights either, which both pack on the stream."""
    entry, real, bufs, expected, fill = _late_setup(ops, dev)
    got = su.run_late(side, fill, lambda: entry(bufs), _clones, label='conv_chain mini')
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


def test_stream_contract_control_misdirected(ops, dev, side):
    """Positive control: the same late inputs with the calls on the default stream must NOT give the expected result."""
    entry, real, bufs, expected, fill = _late_setup(ops, dev)
    got = su.run_misdirected(side, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), 'calls on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(_clones(bufs), _clones(real))
