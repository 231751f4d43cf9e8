"""GPU tests of the head chain (ron_head_chain_forward / ron_head_chain_backward, ops.head_chain_*) and of the module built from it
(nets.ron_vgg_320.reverse_module_fn).

  * the same bytes - y, every BN's mean / var and updated moving statistics, dx, every dw, db, dw2, db2, dgamma, dbeta - as the same
    layers chained through ops.conv2d_nhwc_fn, ops.batchnorm_nhwc_fn (over torch.cat of the two branches for a pair),
    ops.maxpool2x2_nhwc_fn and torch.autograd, for every case of tests/head_chain_cases.py, bf16 and fp16, on Gaussian inputs.  The
    per-operator functions are the reference: each is pinned per element against float64 by its own tests, so no tolerance appears here;
  * bn1_*: a chain of one BN equals ops.batchnorm_train_nhwc / ops.batchnorm_backward_nhwc in bytes on every shape of
    tests/bn_cases.py; on the integer lattices it EQUALS bn_ref's exact float64 result, so that the chain is not graded against
    this library alone; the constant-channel / dead-ReLU and offset-variance hand cases of tests/test_gpu_batchnorm.py;
  * the contract: outputs fully overwritten, nothing assumed about the workspace, nothing written outside it, NULL outputs leave the
    others unchanged, the backward repeatable, the forward twice updates the moving statistics twice, decay 0 and 1, nothing cached
    between calls, the autograd function equal to the explicit calls, all work on the caller's stream without a host synchronisation;
  * the module: reverse_module_fn against the per-operator composition with ref_map detached into a leaf, forward and backward."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import bn_cases as bc  # noqa: E402
import bn_ref as br  # noqa: E402
import head_chain_cases as hc  # noqa: E402
import stream_util as su  # noqa: E402

PARAMS = ('w', 'bias', 'w2', 'bias2', 'gamma', 'beta')
GRAD = {'w': 'dw', 'bias': 'dbias', 'w2': 'dw2', 'bias2': 'dbias2', 'gamma': 'dgamma', 'beta': 'dbeta'}


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


def _up_params(params, dev):
    return [None if p is None else {k: _up(v, dev) for k, v in p.items()} for p in params]


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(case, seed=0):
    return hc.inputs(case, seed)


_REFERENCE = {}


def _reference(ops, dev, case, dtype):
    """The layers chained through the per-operator autograd functions: a flat {name: numpy array}, computed once per (case, dtype)
    and shared by the tests that use it (never modified)."""
    if (case, dtype) in _REFERENCE:
        return _REFERENCE[(case, dtype)]
    x, params, dy = _inputs(case)
    layers = hc.layer_dicts(case)
    xt = _up(x, dev).requires_grad_(True)
    pt = _up_params(params, dev)
    out = {}
    a = xt
    for i, (l, p) in enumerate(zip(layers, pt)):
        for k in PARAMS:
            if p is not None and k in p:
                p[k].requires_grad_(True)
        if l['kind'] == 'pool':
            a = ops.maxpool2x2_nhwc_fn(a, dtype=dtype)
        elif l['kind'] == 'conv':
            a = ops.conv2d_nhwc_fn(a, p['w'], p.get('bias'), relu=l['relu'], dilation=l['dilation'], dtype=dtype)
        elif l['kind'] == 'pair':
            a = torch.cat([ops.conv2d_nhwc_fn(a, p['w'], p.get('bias'), relu=l['relu'], dilation=1, dtype=dtype),
                           ops.conv2d_nhwc_fn(a, p['w2'], p.get('bias2'), relu=l['relu'], dilation=1, dtype=dtype)], -1)
        else:
            # the statistics through the explicit operator (on copies of the moving statistics), the layer through the autograd function
            _, mean, var = ops.batchnorm_train_nhwc(a.detach(), p['gamma'].detach(), p['beta'].detach(), p['moving_mean'].clone(),
                                                    p['moving_var'].clone(), relu=l['relu'], eps=l['eps'], decay=l['decay'], dtype=dtype)
            a = ops.batchnorm_nhwc_fn(a, p['gamma'], p['beta'], p['moving_mean'], p['moving_var'], relu=l['relu'], eps=l['eps'], decay=l['decay'],
                                      dtype=dtype)
            out.update({'mean[%d]' % i: _np(mean), 'var[%d]' % i: _np(var), 'moving_mean[%d]' % i: _np(p['moving_mean']),
                        'moving_var[%d]' % i: _np(p['moving_var'])})
    a.backward(_up(dy, dev))
    out.update(y=_np(a), dx=_np(xt.grad))
    for i, p in enumerate(pt):
        for k in PARAMS:
            if p is not None and k in p:
                out['%s[%d]' % (GRAD[k], i)] = _np(p[k].grad)
    _REFERENCE[(case, dtype)] = out
    return out


def _collect(layers, pt, y, stats, dx, grads):
    out = {'y': _np(y), 'dx': _np(dx)}
    for i, l in enumerate(layers):
        if l['kind'] == 'bn':
            if stats is not None:
                out.update({'mean[%d]' % i: _np(stats[i][0]), 'var[%d]' % i: _np(stats[i][1])})
            out.update({'moving_mean[%d]' % i: _np(pt[i]['moving_mean']), 'moving_var[%d]' % i: _np(pt[i]['moving_var'])})
        for k, v in ((grads[i] if grads is not None and grads[i] else {}) or {}).items():
            out['%s[%d]' % (k, i)] = _np(v)
    return out


def _chain(ops, dev, case, dtype, **kw):
    """The explicit calls on fresh tensors: the same dictionary as _reference."""
    x, params, dy = _inputs(case)
    layers = hc.layer_dicts(case)
    xt, pt = _up(x, dev), _up_params(params, dev)
    y, taps, stats, wsp = ops.head_chain_forward(xt, layers, pt, dtype=dtype)
    dx, grads = ops.head_chain_backward(xt.shape, layers, pt, _up(dy, dev), None, wsp, dtype=dtype, **kw)
    return _collect(layers, pt, y, stats, dx, grads)


def _assert_same(tag, got, want, skip=(), only=None):
    names = [n for n in want if n not in skip and (only is None or n in only)]
    assert names
    for name in names:
        a, b = got.get(name), want[name]
        assert a is not None, '%s: %s is missing' % (tag, name)
        assert a.shape == b.shape, '%s: %s has shape %s, %s expected' % (tag, name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), '%s: %s differs in %d of %d elements (largest difference %g)' % (
            tag, name, int((a != b).sum()), a.size, float(np.abs(a - b).max()))


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('dtype', hc.DTYPES)
@pytest.mark.parametrize('case', sorted(hc.CASES))
def test_chain_equals_the_operators_chained(ops, dev, case, dtype):
    want = _reference(ops, dev, case, dtype)
    got = _chain(ops, dev, case, dtype)
    assert got['y'].shape == hc.shapes(case)[-1] and np.isfinite(got['y']).all() and got['y'].any() and got['dx'].any()
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    _assert_same('%s %s' % (case, dtype), got, want)


def _bn1(ops, dev, given, dtype, relu, decay=bc.DECAY, moving=True):
    """A chain of one BN on the inputs of bn_cases: the dict tests/test_gpu_batchnorm.py's _run returns."""
    t = {k: _up(v, dev) for k, v in given.items() if k != 'eps'}
    layers = [ops.chain_bn(relu=bool(relu), eps=given['eps'], decay=decay)]
    p = {'gamma': t['gamma'], 'beta': t['beta']}
    if moving:
        p.update(moving_mean=t['moving_mean'].clone(), moving_var=t['moving_var'].clone())
    y, _, stats, wsp = ops.head_chain_forward(t['x'], layers, [p], dtype=dtype)
    dx, grads = ops.head_chain_backward(t['x'].shape, layers, [p], t['dy'], None, wsp, dtype=dtype)
    got = dict(y=y, mean=stats[0][0], var=stats[0][1], moving_mean=p.get('moving_mean'), moving_var=p.get('moving_var'), dx=dx,
               dgamma=grads[0]['dgamma'], dbeta=grads[0]['dbeta'])
    return {k: _np(v) for k, v in got.items()}


def _bn_op(ops, dev, given, dtype, relu, decay=bc.DECAY):
    t = {k: _up(v, dev) for k, v in given.items() if k != 'eps'}
    mm, mv = t['moving_mean'].clone(), t['moving_var'].clone()
    y, mean, var = ops.batchnorm_train_nhwc(t['x'], t['gamma'], t['beta'], mm, mv, relu=bool(relu), eps=given['eps'], decay=decay, dtype=dtype)
    dx, dgamma, dbeta = ops.batchnorm_backward_nhwc(t['x'], y if relu else None, t['dy'], t['gamma'], mean, var, relu=bool(relu), eps=given['eps'],
                                                    dtype=dtype)
    return {k: _np(v) for k, v in dict(y=y, mean=mean, var=var, moving_mean=mm, moving_var=mv, dx=dx, dgamma=dgamma, dbeta=dbeta).items()}


@pytest.mark.parametrize('dtype', hc.DTYPES)
@pytest.mark.parametrize('name', sorted(bc.SHAPES))
def test_one_bn_equals_the_operator(ops, dev, name, dtype):
    given = bc.inputs('gauss', bc.SHAPES[name])
    for relu in (0, 1):
        got, want = _bn1(ops, dev, given, dtype, relu), _bn_op(ops, dev, given, dtype, relu)
        _assert_same('bn1_%s %s relu=%d' % (name, dtype, relu), got, want)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('dtype', hc.DTYPES)
@pytest.mark.parametrize('name', sorted(bc.LATTICE))
def test_one_bn_on_the_lattice_is_exact(ops, dev, name, dtype, relu):
    given = bc.inputs('lattice', bc.LATTICE[name])
    got = _bn1(ops, dev, given, dtype, relu)
    fwd = br.forward64(given['x'], given['gamma'], given['beta'], relu, 0.0)
    rnd = br.ROUND[dtype]
    assert np.array_equal(got['mean'], fwd['mean']) and np.array_equal(got['var'], fwd['var'])
    assert np.array_equal(got['y'], rnd(fwd['y'].astype(np.float32))) and np.array_equal(got['y'], fwd['y'])
    bwd = br.backward64(given['x'], br.dz_of(got['y'], given['dy'], dtype, relu), given['gamma'], fwd['mean'], fwd['var'], 0.0)
    bc.assert_lattice(given, fwd, bwd)
    assert np.array_equal(got['dbeta'], bwd['dbeta']) and np.array_equal(got['dgamma'], bwd['dgamma'])
    assert np.array_equal(got['dx'], rnd(bwd['dx'].astype(np.float32)))
    got.update(mean32=got['mean'], var32=got['var'])
    bc.grade('bn1 %s %s relu=%d' % (name, dtype, relu), got, given, dtype, relu)


@pytest.mark.parametrize('dtype', hc.DTYPES)
def test_one_bn_offset_variance(ops, dev, dtype):
    given = bc.inputs('offset', bc.OFFSET_SHAPE, dtype)
    got = _bn1(ops, dev, given, dtype, 0)
    fwd = br.forward64(given['x'], given['gamma'], given['beta'], 0, given['eps'])
    rel = np.abs(got['var'] - fwd['var']) / fwd['var']
    assert rel.max() <= 1e-4
    got.update(mean32=got['mean'], var32=got['var'])
    bc.grade('bn1 offset %s' % dtype, got, given, dtype, 0)


@pytest.mark.parametrize('dtype', hc.DTYPES)
def test_one_bn_constant_channel_and_dead_relu(ops, dev, dtype):
    shape = (1, 8, 8, 72)
    given = dict(bc.inputs('gauss', shape))
    x, dy = given['x'].copy(), given['dy'].copy()
    x[..., 0] = 3.0
    dy[..., 0] = 0.5
    given.update(x=x, dy=dy, beta=np.abs(given['beta']) + np.float32(0.25))
    got = _bn1(ops, dev, given, dtype, 1)
    assert got['mean'][0] == 3.0 and got['var'][0] == 0.0
    assert np.array_equal(got['y'][..., 0], np.full(shape[:3], br.ROUND[dtype](given['beta'][:1])[0]))
    assert got['dbeta'][0] == 32.0 and got['dgamma'][0] == 0.0 and not got['dx'][..., 0].any()
    given.update(beta=np.full(72, -100.0, np.float32))
    got = _bn1(ops, dev, given, dtype, 1)
    assert not got['y'].any() and not got['dx'].any() and not got['dgamma'].any() and not got['dbeta'].any()


def test_decay_zero_and_one_and_null_moving_pointers(ops, dev):
    given = bc.inputs('gauss', bc.SHAPES['c72_m67'])
    base = _bn1(ops, dev, given, 'bf16', 1)
    for decay in (0.0, 1.0):
        _assert_same('decay %g' % decay, _bn1(ops, dev, given, 'bf16', 1, decay=decay), _bn_op(ops, dev, given, 'bf16', 1, decay=decay))
    zero, one = _bn1(ops, dev, given, 'bf16', 1, decay=0.0), _bn1(ops, dev, given, 'bf16', 1, decay=1.0)
    assert zero['moving_mean'].tobytes() == zero['mean'].tobytes()
    assert one['moving_mean'].tobytes() == given['moving_mean'].tobytes() and one['moving_var'].tobytes() == given['moving_var'].tobytes()
    none = _bn1(ops, dev, given, 'bf16', 1, moving=False)
    assert none['moving_mean'] is None
    for k in ('y', 'mean', 'var', 'dx', 'dgamma', 'dbeta'):
        assert none[k].tobytes() == base[k].tobytes(), k


# ------------------------------------------------------------------------------------------------------------------ contract
def _tensors(case, dev, seed=0):
    x, params, dy = _inputs(case, seed)
    return _up(x, dev), _up_params(params, dev), _up(dy, dev)


def _raw(case, dtype, T, ws, fill=float('nan'), forward=True, backward=True, null=(), stats=True):
    """The C entries with caller-made, pre-filled outputs and a caller-made workspace; T = (x, params, dy) on the GPU (the moving
    statistics in params are updated in place).  null: output names ('dx', 'dw[0]', 'mean[1]', ...) passed as NULL."""
    from ron_tensorflow_amd import _lib
    from ron_tensorflow_amd import ops
    x, pt, dy = T
    layers = hc.layer_dicts(case)
    L = len(layers)
    shapes = hc.shapes(case)
    d = ops._head_chain_desc(x.shape[0], x.shape[1], x.shape[2], x.shape[3], layers, dtype)
    assert 0 < _lib.lib().ron_head_chain_workspace_bytes(C.byref(d)) <= ws.numel()
    new = lambda shape: torch.full(tuple(shape), fill, dtype=torch.float32, device=x.device)
    cols = {name: [None if p is None else p.get(name) for p in pt] for name in PARAMS + ('moving_mean', 'moving_var')}
    out = {}
    if forward:
        out['y'] = new(shapes[-1])
        for i, l in enumerate(layers):
            if l['kind'] == 'bn' and stats:
                for k in ('mean', 'var'):
                    if '%s[%d]' % (k, i) not in null:
                        out['%s[%d]' % (k, i)] = new((shapes[i][3],))
        table = ops._head_ptrs(L, mean=[out.get('mean[%d]' % i) for i in range(L)], var=[out.get('var[%d]' % i) for i in range(L)], **cols)
        _lib.check(_lib.lib().ron_head_chain_forward(C.byref(d), _lib.ptr(x), table, _lib.ptr(out['y']), _lib.ptr(ws), int(ws.numel()),
                                                     _lib.current_stream()))
        for i, l in enumerate(layers):
            if l['kind'] == 'bn':
                out.update({'moving_mean[%d]' % i: pt[i]['moving_mean'].clone(), 'moving_var[%d]' % i: pt[i]['moving_var'].clone()})
    if backward:
        if 'dx' not in null:
            out['dx'] = new(x.shape)
        for i, p in enumerate(pt):
            for k in PARAMS:
                name = '%s[%d]' % (GRAD[k], i)
                if p is not None and k in p and name not in null:
                    out[name] = new(p[k].shape)
        gcols = {g: [out.get('%s[%d]' % (g, i)) for i in range(L)] for g in GRAD.values()}
        table = ops._head_ptrs(L, w=cols['w'], w2=cols['w2'], gamma=cols['gamma'], **gcols)
        _lib.check(_lib.lib().ron_head_chain_backward(C.byref(d), _lib.ptr(dy), table, _lib.ptr(out.get('dx')), _lib.ptr(ws), int(ws.numel()),
                                                      _lib.current_stream()))
    return {k: _np(v) for k, v in out.items()}


def _need(ops, case, dtype):
    (n, h, w, c), _ = hc.CASES[case]
    return ops.head_chain_workspace_bytes(n, h, w, c, hc.layer_dicts(case), dtype=dtype)


@pytest.mark.parametrize('case', ['cls', 'bnpool', 'objness'])
def test_workspace_and_output_contract(ops, dev, case):
    """Outputs pre-filled with NaN come back without one; a workspace of 0xFF bytes, of float32 NaNs and of 16-bit NaNs gives the bytes
    a zeroed one gives; carved at exactly the sizer's length out of a larger buffer, the bytes in front of and behind it are
    untouched."""
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
        got = _raw(case, 'bf16', _tensors(case, dev), ws)
        for n_, a in got.items():
            assert not np.isnan(a).any(), 'workspace of %s: %d NaN survive in %s' % (name, int(np.isnan(a).sum()), n_)
        assert set(got) == set(want)
        _assert_same('workspace of %s' % name, got, want)
    edges = torch.cat([big[:guard], big[guard + need:]]).cpu().numpy()
    assert (edges == 0xA5).all(), 'bytes outside the workspace were written'


def test_null_outputs_leave_the_others_unchanged(ops, dev):
    case = 'cls'
    ws = torch.empty((_need(ops, case, 'bf16'),), dtype=torch.uint8, device=dev)
    want = _reference(ops, dev, case, 'bf16')
    T = _tensors(case, dev)
    # the forward without mean / var outputs (the statistics stay in the workspace): the backward is unchanged
    got = _raw(case, 'bf16', T, ws, stats=False)
    assert 'mean[1]' not in got
    _assert_same('mean, var NULL', got, want, skip=tuple(n for n in want if n.startswith(('mean', 'var'))))
    one = _raw(case, 'bf16', _tensors(case, dev), ws, null=('mean[1]', 'var[3]'))
    assert 'mean[1]' not in one and 'var[3]' not in one
    _assert_same('mean[1], var[3] NULL', one, want, skip=('mean[1]', 'var[3]'))
    outputs = [n for n in want if n == 'dx' or n.startswith('d')]
    assert len(outputs) == 1 + 4 + 4 + 2 + 4
    for name in outputs:
        got = _raw(case, 'bf16', T, ws, forward=False, null=(name,))
        assert name not in got
        _assert_same('%s NULL' % name, got, want, only=[n for n in outputs if n != name])
    # nothing but the last layer's gradients: everything in front of it is skipped
    last = [n for n in outputs if n.endswith('[4]')]
    got = _raw(case, 'bf16', T, ws, forward=False, null=tuple(n for n in outputs if n not in last))
    assert sorted(got) == sorted(last)
    _assert_same('the last layer only', got, want, only=last)


@pytest.mark.parametrize('case', ['cls', 'bnpool'])
def test_backward_twice_and_forward_twice(ops, dev, case):
    ws = torch.empty((_need(ops, case, 'bf16'),), dtype=torch.uint8, device=dev)
    T = _tensors(case, dev)
    want = _reference(ops, dev, case, 'bf16')
    _raw(case, 'bf16', T, ws, backward=False)
    a = _raw(case, 'bf16', T, ws, forward=False)
    b = _raw(case, 'bf16', T, ws, forward=False)
    _assert_same('second backward', b, a)
    _assert_same('backward', a, want, only=list(a))
    # a second forward updates the moving statistics a second time: two operator calls on the same buffers
    second = _raw(case, 'bf16', T, ws, backward=False)
    for i, l in enumerate(hc.layer_dicts(case)):
        if l['kind'] != 'bn':
            continue
        for k in ('moving_mean', 'moving_var'):
            assert second['%s[%d]' % (k, i)].tobytes() != want['%s[%d]' % (k, i)].tobytes(), 'the second forward left %s alone' % k
        ref_mm, ref_mv = _twice(ops, dev, case, i)
        assert second['moving_mean[%d]' % i].tobytes() == ref_mm.tobytes() and second['moving_var[%d]' % i].tobytes() == ref_mv.tobytes()


def _twice(ops, dev, case, bn_layer, dtype='bf16'):
    """The moving statistics of layer `bn_layer` after the per-operator sequence has run twice on the same buffers."""
    x, params, dy = _inputs(case)
    layers = hc.layer_dicts(case)
    pt = _up_params(params, dev)
    for _ in range(2):
        a = _up(x, dev)
        for l, p in zip(layers, pt):
            if l['kind'] == 'pool':
                a = ops.maxpool2x2_nhwc(a, dtype=dtype)
            elif l['kind'] == 'conv':
                a = ops.conv2d_forward_nhwc(a, p['w'], p.get('bias'), relu=l['relu'], dilation=l['dilation'], dtype=dtype)
            elif l['kind'] == 'pair':
                a = torch.cat([ops.conv2d_forward_nhwc(a, p['w'], p.get('bias'), relu=l['relu'], dtype=dtype),
                               ops.conv2d_forward_nhwc(a, p['w2'], p.get('bias2'), relu=l['relu'], dtype=dtype)], -1)
            else:
                a = ops.batchnorm_train_nhwc(a, p['gamma'], p['beta'], p['moving_mean'], p['moving_var'], relu=l['relu'], eps=l['eps'],
                                             decay=l['decay'], dtype=dtype)[0]
    return _np(pt[bn_layer]['moving_mean']), _np(pt[bn_layer]['moving_var'])


def test_nothing_is_cached_between_calls(ops, dev):
    """After the weights and gamma changed IN PLACE (the same pointers, as the optimizer leaves them) the forward and backward in the
    same workspace follow the new values: the bytes of a first call on fresh tensors holding them."""
    case = 'cls'
    T = _tensors(case, dev)
    ws = torch.empty((_need(ops, case, 'bf16'),), dtype=torch.uint8, device=dev)
    first = _raw(case, 'bf16', T, ws)
    fresh_T = _tensors(case, dev)
    for p, q in zip(T[1], fresh_T[1]):
        for k in ('w', 'w2', 'gamma'):
            if p is not None and k in p:
                p[k].mul_(-1.5)
                q[k].mul_(-1.5)
        if p is not None and 'moving_mean' in p:        # the first call updated them: the fresh set starts where this one stands
            q['moving_mean'].copy_(p['moving_mean'])
            q['moving_var'].copy_(p['moving_var'])
    second = _raw(case, 'bf16', T, ws)
    assert second['y'].tobytes() != first['y'].tobytes()
    fresh = _raw(case, 'bf16', fresh_T, torch.zeros_like(ws))
    _assert_same('after the in-place change', second, fresh)


@pytest.mark.parametrize('case', ['cls', 'objness'])
def test_autograd_function_equals_the_explicit_calls(ops, dev, case):
    want = _reference(ops, dev, case, 'bf16')
    x, params, dy = _inputs(case)
    layers = hc.layer_dicts(case)

    def run(skip=()):
        xt = _up(x, dev).requires_grad_('x' not in skip)
        pt = _up_params(params, dev)
        for i, p in enumerate(pt):
            for k in PARAMS:
                if p is not None and k in p:
                    p[k].requires_grad_((i, k) not in skip)
        outs = ops.head_chain_fn(xt, layers, pt, dtype='bf16')
        assert len(outs) == 1
        outs[0].backward(_up(dy, dev))
        got = {'y': _np(outs[0]), 'dx': _np(xt.grad)}
        for i, p in enumerate(pt):
            for k in PARAMS:
                if p is not None and k in p:
                    got['%s[%d]' % (GRAD[k], i)] = _np(p[k].grad)
            if p is not None and 'moving_mean' in p:
                assert p['moving_mean'].grad is None and not p['moving_mean'].requires_grad
                got.update({'moving_mean[%d]' % i: _np(p['moving_mean']), 'moving_var[%d]' % i: _np(p['moving_var'])})
        return got
    got = run()
    _assert_same('head_chain_fn %s' % case, got, want, skip=tuple(n for n in want if n.startswith(('mean', 'var'))))
    # needs_input_grad: no gradient for x, the first layer's weight and the first BN's gamma -> none computed, the others unchanged
    bn0 = [i for i, l in enumerate(layers) if l['kind'] == 'bn'][0]
    got = run(skip=('x', (0, 'w'), (bn0, 'gamma')))
    assert got['dx'] is None and got['dw[0]'] is None and got['dgamma[%d]' % bn0] is None
    rest = [n for n in want if n.startswith('d') and n not in ('dx', 'dw[0]', 'dgamma[%d]' % bn0)]
    _assert_same('head_chain_fn %s, three gradients not needed' % case, got, want, only=rest)


# ------------------------------------------------------------------------------------------------------------------ stream contract
def _late_setup(ops, dev, case='cls'):
    layers = hc.layer_dicts(case)
    keys = PARAMS + ('moving_mean', 'moving_var')

    def flat(T):
        x, pt, dy = T
        return [x] + [p[k] for p in pt if p is not None for k in keys if k in p] + [dy]

    def unflat(ts, like):
        it = iter(ts)
        x = next(it)
        pt = [None if p is None else {k: next(it) for k in keys if k in p} for p in like[1]]
        return x, pt, next(it)

    given, poison = _tensors(case, dev, 0), _tensors(case, dev, 1)          # two valid sets of values of the same shapes

    def entry(ts):
        x, pt, dy = unflat(ts, given)
        # the moving statistics are updated in place: every call works on copies made on the current stream, and returns them
        pt = [None if p is None else {k: (v.clone() if k.startswith('moving') else v) for k, v in p.items()} for p in pt]
        y, taps, stats, wsp = ops.head_chain_forward(x, layers, pt, dtype='bf16')
        dx, grads = ops.head_chain_backward(x.shape, layers, pt, dy, None, wsp, dtype='bf16')
        out = [y, dx] + [t for s in stats if s is not None for t in s]
        out += [p[k] for p in pt if p is not None for k in ('moving_mean', 'moving_var') if k in p]
        return out + [g[k] for g in grads if g for k in sorted(g)]
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
    """On a stalled side stream, with x, every w, bias, gamma, beta and moving statistic and dy copied into their buffers behind the
    stall: neither call waits for the host and neither reads anything early."""
    entry, real, bufs, expected, fill = _late_setup(ops, dev)
    got = su.run_late(side, fill, lambda: entry(bufs), _clones, label='head_chain cls')
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


def test_stream_contract_control_misdirected(ops, dev, side):
    """Positive control: the same late inputs with the calls on the default stream must NOT give the expected result."""
    entry, real, bufs, expected, fill = _late_setup(ops, dev)
    got = su.run_misdirected(side, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), 'calls on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(_clones(bufs), _clones(real))


# ------------------------------------------------------------------------------------------------------------------ the module
A, NC, WIDTH = 2, 3, 128          # (the transposed convolution wants its channels a multiple of 128)


def _module_inputs(top, dev):
    """left / right maps of 64 channels, the module's variables by name, and the four output gradients"""
    from ron_tensorflow_amd.nets import ron_vgg_320 as net
    rs = np.random.RandomState(900 + int(top))
    f = np.float32
    n, h, w = 2, 6, 10
    chains = net.head_chains(A, NC, 'block5', top=top, width=WIDTH)
    left = rs.randn(n, 2 * h if top else h, 2 * w if top else w, 64).astype(f)
    right = None if top else rs.randn(n, h // 2, w // 2, 64).astype(f)
    variables = {}
    for key, cin0 in (('left', 64), ('objness', WIDTH), ('cls', WIDTH), ('reg', WIDTH)):
        ch = WIDTH if (key == 'left' and top) else cin0
        for l, names in zip(*chains[key]):
            if l['kind'] == 'bn':
                variables[names['gamma']] = (1.0 + 0.2 * rs.uniform(-1, 1, ch)).astype(f)
                variables[names['beta']] = (0.1 * rs.uniform(-1, 1, ch)).astype(f)
                variables[names['moving_mean']] = rs.randn(ch).astype(f)
                variables[names['moving_var']] = (np.abs(rs.randn(ch)) + 0.5).astype(f)
                continue
            variables[names['w']] = (rs.randn(3, 3, ch, l['cout']) * np.sqrt(2.0 / (9 * ch))).astype(f)
            if 'bias' in names:
                variables[names['bias']] = (rs.randn(l['cout']) * 0.1).astype(f)
            if l['kind'] == 'pair':
                variables[names['w2']] = (rs.randn(1, 1, ch, l['cout2']) * np.sqrt(2.0 / ch)).astype(f)
                variables[names['bias2']] = (rs.randn(l['cout2']) * 0.1).astype(f)
            ch = l['cout'] + l.get('cout2', 0)
    if top:
        variables[chains['left_conv']['w']] = (rs.randn(2, 2, 64, WIDTH) * np.sqrt(2.0 / (4 * 64))).astype(f)
    else:
        variables[chains['deconv']['w']] = (rs.randn(2, 2, WIDTH, 64) * np.sqrt(2.0 / 64)).astype(f)
        variables[chains['deconv']['bias']] = (rs.randn(WIDTH) * 0.1).astype(f)
    grads = [rs.randn(n, h, w, WIDTH).astype(f), rs.randn(n, h, w, A, 2).astype(f), rs.randn(n, h, w, A, NC).astype(f), rs.randn(n, h, w, A, 4).astype(f)]
    return chains, left, right, variables, grads


def _module_reference(ops, dev, chains, left, right, variables, grads, dtype):
    """The per-operator functions with ref_map detached into a leaf: the three branch gradients of the leaf by torch.autograd.grad,
    added in the stated order in fp32, the sum sent back through the left part."""
    V = {k: v.requires_grad_(not k.rsplit('/', 1)[-1].startswith('moving')) for k, v in variables.items()}

    def run(a, key):
        for l, names in zip(*chains[key]):
            if l['kind'] == 'conv':
                a = ops.conv2d_nhwc_fn(a, V[names['w']], V.get(names.get('bias')), relu=l['relu'], dilation=1, dtype=dtype)
            elif l['kind'] == 'pair':
                a = torch.cat([ops.conv2d_nhwc_fn(a, V[names['w']], V[names['bias']], relu=l['relu'], dilation=1, dtype=dtype),
                               ops.conv2d_nhwc_fn(a, V[names['w2']], V[names['bias2']], relu=l['relu'], dilation=1, dtype=dtype)], -1)
            else:
                a = ops.batchnorm_nhwc_fn(a, V[names['gamma']], V[names['beta']], V[names['moving_mean']], V[names['moving_var']], relu=l['relu'],
                                          eps=l['eps'], decay=l['decay'], dtype=dtype)
        return a
    if right is None:
        ref = run(ops.conv2d_k2s2_nhwc_fn(left, V[chains['left_conv']['w']], None, relu=False, transpose=False, dtype=dtype), 'left')
    else:
        up = ops.conv2d_k2s2_nhwc_fn(right, V[chains['deconv']['w']], V[chains['deconv']['bias']], relu=True, transpose=True, dtype=dtype)
        ref = torch.relu(run(left, 'left') + up)
    leaf = ref.detach().requires_grad_(True)
    heads = [run(leaf, key) for key in ('objness', 'cls', 'reg')]
    total = grads[0]
    for head, g in zip(heads, grads[1:]):
        head.backward(g.reshape(head.shape), inputs=[leaf] + [v for v in V.values() if v.requires_grad])
        total = total + leaf.grad
        leaf.grad = None
    ref.backward(total)
    return [ref] + heads


@pytest.mark.parametrize('top', [False, True])
def test_reverse_module_equals_the_per_operator_composition(ops, dev, top):
    from ron_tensorflow_amd.nets import ron_vgg_320 as net
    chains, left, right, variables, grads = _module_inputs(top, dev)
    up = lambda a: None if a is None else _up(a, dev)
    gt = [up(g) for g in grads]
    # the reference, on tensors of its own
    l0, r0 = up(left).requires_grad_(True), None if right is None else up(right).requires_grad_(True)
    v0 = {k: up(v) for k, v in variables.items()}
    want = _module_reference(ops, dev, chains, l0, r0, v0, gt, 'bf16')
    # the module
    l1, r1 = up(left).requires_grad_(True), None if right is None else up(right).requires_grad_(True)
    v1 = {k: up(v).requires_grad_(not k.rsplit('/', 1)[-1].startswith('moving')) for k, v in variables.items()}
    outs = net.reverse_module_fn(l1, r1, v1, A, NC, 'block5', dtype='bf16', width=WIDTH)
    n, h, w = 2, 6, 10
    assert [tuple(o.shape) for o in outs] == [(n, h, w, WIDTH), (n, h, w, A, 2), (n, h, w, A, NC), (n, h, w, A, 4)]
    for name, a, b in zip(('ref_map', 'objness_logits', 'cls_pred', 'loc_pred'), outs, want):
        assert _np(a).tobytes() == _np(b).tobytes(), name
        assert _np(a).any()
    torch.autograd.backward(list(outs), gt)
    assert _np(l1.grad).any() and _np(l1.grad).tobytes() == _np(l0.grad).tobytes(), 'd_left'
    if right is not None:
        assert _np(r1.grad).any() and _np(r1.grad).tobytes() == _np(r0.grad).tobytes(), 'd_right'
    assert set(v1) == set(v0) and len(v1) == (37 if top else 39)
    for k in v1:
        if k.rsplit('/', 1)[-1].startswith('moving'):
            assert v1[k].grad is None and _np(v1[k]).tobytes() == _np(v0[k]).tobytes() and _np(v1[k]).tobytes() != variables[k].tobytes(), k
        else:
            assert v1[k].grad is not None and _np(v1[k].grad).tobytes() == _np(v0[k].grad).tobytes(), 'the gradient of %s' % k
