"""GPU parity of training-mode batch normalisation (ron_batchnorm_train_nhwc, ron_batchnorm_backward_nhwc) against the float64
references of tests/bn_ref.py on the cases of tests/bn_cases.py.

  gauss    every shape x bf16 / fp16 x relu 0 / 1: y, mean, var, the moving statistics, dx, dgamma, dbeta graded per element by the
           derived bounds (bn_cases.grade: ratio <= 1, no exclusions), y and dx storage-type values;
  lattice  the outputs must EQUAL the reference (every one of them is exact there: bn_cases);
  offset   the variance an E[x^2] - mean^2 loses: inside the bound and within 1e-4 of the variance;
  hand     decay 0 / 1, NULL moving pointers, a constant channel, an all-zero y;

and the contract of the entry points: outputs fully overwritten, nothing assumed about the workspace, NULL outputs, the same bytes on
every call, the caller's stream without a host synchronisation, and the autograd function against the explicit sequence of calls.

Each gauss case prints its largest ratios (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import bn_cases as bc  # noqa: E402
import bn_ref as br  # noqa: E402
import conv_bounds as cb  # noqa: E402
import conv_grad_ref as cgr  # noqa: E402
import stream_util as su  # noqa: E402

NAMES = ('dx', 'dgamma', 'dbeta')


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
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bytes(outs):
    return [None if t is None else t.cpu().numpy().tobytes() for t in outs]


def _clones(tensors):
    return [t.clone() for t in tensors]


@functools.lru_cache(maxsize=None)
def _given(kind, shape, dtype='bf16'):
    """The inputs of one case, made once and shared (never modified)."""
    return bc.inputs(kind, shape, dtype)


def _run(ops, dev, given, dtype, relu, decay=bc.DECAY, moving=True):
    """Forward, then the backward on the forward's own y, mean and var: the dict bn_cases.grade takes, plus the device tensors."""
    t = {k: _up(v, dev) for k, v in given.items() if k != 'eps'}
    mm, mv = (t['moving_mean'].clone(), t['moving_var'].clone()) if moving else (None, None)
    y, mean, var = ops.batchnorm_train_nhwc(t['x'], t['gamma'], t['beta'], mm, mv, relu=bool(relu), eps=given['eps'], decay=decay, dtype=dtype)
    dx, dgamma, dbeta = ops.batchnorm_backward_nhwc(t['x'], y if relu else None, t['dy'], t['gamma'], mean, var, relu=bool(relu),
                                                    eps=given['eps'], dtype=dtype)
    dev_out = dict(y=y, mean=mean, var=var, moving_mean=mm, moving_var=mv, dx=dx, dgamma=dgamma, dbeta=dbeta)
    host = {k: None if v is None else v.cpu().numpy() for k, v in dev_out.items()}
    host.update(mean32=host['mean'], var32=host['var'])
    return host, dev_out, t


# --------------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize('dtype', bc.DTYPES)
@pytest.mark.parametrize('name', sorted(bc.SHAPES))
def test_gauss_parity(ops, dev, name, dtype):
    given = _given('gauss', bc.SHAPES[name])
    for relu in (0, 1):
        got, _, _ = _run(ops, dev, given, dtype, relu)
        bc.grade('%s %s relu=%d' % (name, dtype, relu), got, given, dtype, relu, verbose=True)


@pytest.mark.parametrize('dtype', bc.DTYPES)
def test_tiny_variance_parity(ops, dev, dtype):
    """var of the size of eps: 1 / sqrt(var + eps), not 1 / (sqrt(var) + eps)."""
    given = _given('tiny', bc.SHAPES['c72_m33'])
    for relu in (0, 1):
        got, _, _ = _run(ops, dev, given, dtype, relu)
        bc.grade('tiny %s relu=%d' % (dtype, relu), got, given, dtype, relu, verbose=True)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('dtype', bc.DTYPES)
@pytest.mark.parametrize('name', sorted(bc.LATTICE))
def test_lattice_is_exact(ops, dev, name, dtype, relu):
    given = _given('lattice', bc.LATTICE[name])
    got, _, _ = _run(ops, dev, given, dtype, relu)
    fwd = br.forward64(given['x'], given['gamma'], given['beta'], relu, 0.0)
    rnd = br.ROUND[dtype]
    assert np.array_equal(got['mean'], fwd['mean']) and np.array_equal(got['var'], fwd['var'])
    assert np.array_equal(got['y'], rnd(fwd['y'].astype(np.float32))) and np.array_equal(got['y'], fwd['y'])
    bwd = br.backward64(given['x'], br.dz_of(got['y'], given['dy'], dtype, relu), given['gamma'], fwd['mean'], fwd['var'], 0.0)
    bc.assert_lattice(given, fwd, bwd)
    assert np.array_equal(got['dbeta'], bwd['dbeta']) and np.array_equal(got['dgamma'], bwd['dgamma'])
    # dx: its float32 value is exact (assert_lattice), so the delivered value is that value rounded once
    assert np.array_equal(got['dx'], rnd(bwd['dx'].astype(np.float32)))
    # the moving statistics: decay * m + (1 - decay) * s rounds (0.997 is no dyadic number): inside the bound instead, graded like gauss
    bc.grade('%s %s relu=%d' % (name, dtype, relu), got, given, dtype, relu)


@pytest.mark.parametrize('dtype', bc.DTYPES)
def test_offset_variance(ops, dev, dtype):
    given = _given('offset', bc.OFFSET_SHAPE, dtype)
    got, _, _ = _run(ops, dev, given, dtype, 0)
    fwd = br.forward64(given['x'], given['gamma'], given['beta'], 0, given['eps'])
    rel = np.abs(got['var'] - fwd['var']) / fwd['var']
    print('offset %s: var %s, largest relative error %.3g' % (dtype, fwd['var'][:2], rel.max()))
    assert rel.max() <= 1e-4
    bc.grade('offset %s' % dtype, got, given, dtype, 0, verbose=True)


# ------------------------------------------------------------------------------------------------------------------------ hand cases
def test_decay_zero_and_one_and_null_moving_pointers(ops, dev):
    given = _given('gauss', bc.SHAPES['c72_m67'])
    base, _, _ = _run(ops, dev, given, 'bf16', 1)
    zero, _, _ = _run(ops, dev, given, 'bf16', 1, decay=0.0)
    one, _, _ = _run(ops, dev, given, 'bf16', 1, decay=1.0)
    none, _, _ = _run(ops, dev, given, 'bf16', 1, moving=False)
    assert zero['moving_mean'].tobytes() == zero['mean'].tobytes(), 'decay 0: moving_mean is not the batch mean bit for bit'
    rows = 67
    assert np.allclose(zero['moving_var'], zero['var'] * rows / (rows - 1), rtol=2 ** -22, atol=0)
    assert one['moving_mean'].tobytes() == given['moving_mean'].tobytes() and one['moving_var'].tobytes() == given['moving_var'].tobytes()
    assert none['moving_mean'] is None
    for other in (zero, one, none):
        for k in ('y', 'mean', 'var', 'dx', 'dgamma', 'dbeta'):
            assert other[k].tobytes() == base[k].tobytes(), k


@pytest.mark.parametrize('dtype', bc.DTYPES)
def test_constant_channel_and_dead_relu(ops, dev, dtype):
    """Channel 0 constant: var = 0, y = act(beta), and dx = 0 where dy is constant over the channel too (in general it is
    gamma / sqrt(eps) (dz - mean(dz)): the operator's true derivative at var = 0).  beta = -100: y = 0 everywhere under ReLU, so all
    three gradients are zero."""
    shape = (1, 8, 8, 72)
    given = dict(_given('gauss', shape))
    x, dy = given['x'].copy(), given['dy'].copy()
    x[..., 0] = 3.0
    dy[..., 0] = 0.5
    given.update(x=x, dy=dy, beta=np.abs(given['beta']) + np.float32(0.25))
    got, _, _ = _run(ops, dev, given, dtype, 1)
    assert got['mean'][0] == 3.0 and got['var'][0] == 0.0
    assert np.array_equal(got['y'][..., 0], np.full(shape[:3], br.ROUND[dtype](given['beta'][:1])[0]))
    assert got['dbeta'][0] == 32.0 and got['dgamma'][0] == 0.0 and not got['dx'][..., 0].any()
    bc.grade('constant channel %s' % dtype, got, given, dtype, 1)
    given.update(beta=np.full(72, -100.0, np.float32))
    got, _, _ = _run(ops, dev, given, dtype, 1)
    assert not got['y'].any() and not got['dx'].any() and not got['dgamma'].any() and not got['dbeta'].any()


# -------------------------------------------------------------------------------------------------------------------- the contract
def _raw(dev, t, given, dtype, relu, fill, workspace, null=()):
    """Both C entries with caller-made outputs (prefilled with `fill`) and workspace; `null`: outputs passed as NULL."""
    from ron_tensorflow_amd import _lib
    n, h, w, c = t['x'].shape
    d = _lib.BnDesc(n, h, w, c, _lib.DTYPES[dtype], int(relu), given['eps'], bc.DECAY)
    assert workspace.numel() >= _lib.lib().ron_batchnorm_workspace_bytes(C.byref(d))
    vec = lambda: torch.full((c,), fill, dtype=torch.float32, device=dev)
    y, mean, var = torch.full_like(t['x'], fill), vec(), vec()
    mm, mv = t['moving_mean'].clone(), t['moving_var'].clone()
    p, L = _lib.ptr, _lib.lib()
    _lib.check(L.ron_batchnorm_train_nhwc(C.byref(d), p(t['x']), p(t['gamma']), p(t['beta']), p(y), p(mean), p(var), p(mm), p(mv), p(workspace),
                                          int(workspace.numel()), _lib.current_stream()))
    outs = {'dx': torch.full_like(t['x'], fill), 'dgamma': vec(), 'dbeta': vec()}
    for name in null:
        outs[name] = None
    _lib.check(L.ron_batchnorm_backward_nhwc(C.byref(d), p(t['x']), p(y if relu else None), p(t['dy']), p(t['gamma']), p(mean), p(var),
                                             p(outs['dx']), p(outs['dgamma']), p(outs['dbeta']), p(workspace), int(workspace.numel()),
                                             _lib.current_stream()))
    return [y, mean, var, mm, mv, outs['dx'], outs['dgamma'], outs['dbeta']]


@pytest.mark.parametrize('name', ['c8_m1027', 'c72_m67', 'c1024_m35', 'coarse'])
def test_outputs_are_overwritten_workspace_is_not_read_null_outputs_and_repeats(ops, dev, name):
    """Outputs prefilled with NaN, a workspace of 0xFF bytes (NaN in every 2- and 4-byte format), then the same buffer straight after a
    call of another shape; each NULL output leaves the others' bytes unchanged; two calls give the same bytes."""
    given = _given('gauss', bc.SHAPES[name])
    for relu in (0, 1):
        got, dev_out, t = _run(ops, dev, given, 'bf16', relu)
        want = _bytes([dev_out[k] for k in ('y', 'mean', 'var', 'moving_mean', 'moving_var', 'dx', 'dgamma', 'dbeta')])
        ws = torch.full((ops.batchnorm_workspace_bytes(*bc.SHAPES['scale40']),), 0xFF, dtype=torch.uint8, device=dev)
        assert _bytes(_raw(dev, t, given, 'bf16', relu, float('nan'), ws)) == want
        assert _bytes(_raw(dev, t, given, 'bf16', relu, float('nan'), ws)) == want, 'two calls differ (the workspace holds the last call)'
        for null in (('dx',), ('dgamma',), ('dbeta',), ('dgamma', 'dbeta'), ('dx', 'dgamma', 'dbeta')):
            part = _bytes(_raw(dev, t, given, 'bf16', relu, float('nan'), ws, null))
            for k, a, b in zip(('y', 'mean', 'var', 'moving_mean', 'moving_var') + NAMES, part, want):
                assert (a is None) if k in null else (a == b), '%s differs when %s is NULL' % (k, null)


def _late_setup(ops, dev, which):
    shape = bc.SHAPES['coarse']
    given, poison = _given('gauss', shape), _given('tiny', shape)          # another valid case of the same shapes
    _, out, t = _run(ops, dev, given, 'bf16', 1)
    _, outp, tp = _run(ops, dev, poison, 'bf16', 1)
    if which == 'forward':
        keys = ('x', 'gamma', 'beta', 'moving_mean', 'moving_var')
        x, xp = [t[k] for k in keys], [tp[k] for k in keys]

        def entry(b):
            mm, mv = b[3].clone(), b[4].clone()
            return list(ops.batchnorm_train_nhwc(b[0], b[1], b[2], mm, mv, relu=True, eps=given['eps'], decay=bc.DECAY)) + [mm, mv]
    else:
        x = [t['x'], out['y'], t['dy'], t['gamma'], out['mean'], out['var']]
        xp = [tp['x'], outp['y'], tp['dy'], tp['gamma'], outp['mean'], outp['var']]

        def entry(b):
            return list(ops.batchnorm_backward_nhwc(b[0], b[1], b[2], b[3], b[4], b[5], relu=True, eps=given['eps']))
    expected = _clones(entry(x))
    bufs = _clones(xp)
    poisoned = _clones(entry(bufs))
    torch.cuda.synchronize()
    assert not su.same_bytes(expected, poisoned)

    def fill():
        for b, src in zip(bufs, x):
            b.copy_(src, non_blocking=True)
    return entry, x, bufs, expected, fill


@pytest.mark.parametrize('which', ['forward', 'backward'])
def test_stream_contract_late_inputs(ops, dev, side, which):
    """On a stalled side stream, with the real inputs copied into the buffers behind the stall: the call does not wait for the host
    and reads nothing early - the result has the default-stream result's bytes."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev, which)
    got = su.run_late(side, fill, lambda: entry(bufs), _clones, label='batchnorm_%s_nhwc' % which)
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


@pytest.mark.parametrize('which', ['forward', 'backward'])
def test_stream_contract_control_misdirected(ops, dev, side, which):
    """Positive control: the same late inputs with the call on the default stream must NOT give the expected result."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev, which)
    got = su.run_misdirected(side, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), 'a call on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(_clones(bufs), _clones(x))


# ------------------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize('x_needs_grad', [False, True])
def test_autograd_reg_bbox_module_is_the_explicit_calls(ops, dev, x_needs_grad):
    """reg_bbox: conv3x3 (no activation) -> batch norm + ReLU -> conv3x3, 2 x 8 x 8, 64 -> 64 -> 24 channels.  .backward() gives, bit for
    bit, what the explicit sequence of backward calls gives on the same saved tensors.  Against float64 the composition is graded stage
    by stage: every stage's reference reads the tensors the stage before DELIVERED (the forward's h, y and the backward's dy chain), so
    each stage's own per-element bound is the composed bound of the chain up to it."""
    rs = np.random.RandomState(11)

    def t(a, grad):
        return torch.from_numpy(a.astype(np.float32)).to(dev).requires_grad_(grad)
    x = t(rs.randn(2, 8, 8, 64), x_needs_grad)
    w1, b1 = t(rs.randn(3, 3, 64, 64) * np.sqrt(2.0 / 576), True), t(rs.randn(64) * 0.1, True)
    gamma, beta = t(1.0 + 0.3 * rs.randn(64), True), t(0.2 * rs.randn(64), True)
    w2, b2 = t(rs.randn(3, 3, 64, 24) * np.sqrt(2.0 / 576), True), t(rs.randn(24) * 0.1, True)
    mm, mv = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    g = torch.from_numpy(rs.randn(2, 8, 8, 24).astype(np.float32)).to(dev)
    h = ops.conv2d_nhwc_fn(x, w1, b1, relu=False)
    y = ops.batchnorm_nhwc_fn(h, gamma, beta, mm, mv, relu=True)
    out = ops.conv2d_nhwc_fn(y, w2, b2, relu=False)
    (out * g).sum().backward()
    assert float(mm.abs().max()) > 0 and float((mv - 1).abs().max()) > 0, 'the forward did not update the moving statistics'
    with torch.no_grad():
        y2, mean, var = ops.batchnorm_train_nhwc(h.detach(), gamma.detach(), beta.detach(), relu=True)
        assert _bytes([y2]) == _bytes([y.detach()])
        dy, dw2, db2 = ops.conv2d_backward_nhwc(y.detach(), w2.detach(), g, None, relu=False)
        dh, dgamma, dbeta = ops.batchnorm_backward_nhwc(h.detach(), y.detach(), dy, gamma.detach(), mean, var, relu=True)
        dxe, dw1, db1 = ops.conv2d_backward_nhwc(x.detach(), w1.detach(), dh, None, relu=False, need=('dx', 'dw', 'db') if x_needs_grad else ('dw', 'db'))
    assert _bytes([w2.grad, b2.grad, gamma.grad, beta.grad, w1.grad, b1.grad]) == _bytes([dw2, db2, dgamma, dbeta, dw1, db1])
    if x_needs_grad:
        assert _bytes([x.grad]) == _bytes([dxe]) and float(x.grad.abs().max()) > 0
    else:
        assert x.grad is None and dxe is None
    # float64, stage by stage on the delivered tensors
    hn, yn, dyn = h.detach().cpu().numpy(), y.detach().cpu().numpy(), dy.cpu().numpy()
    rnd = br.ROUND['bf16']
    for tag, xin, w, b, got in (('conv1', x, w1, b1, hn), ('conv2', y, w2, b2, out.detach().cpu().numpy())):
        ref, S, K = cb.conv_op(rnd(xin.detach().cpu().numpy()), rnd(w.detach().cpu().numpy()), b.detach().cpu().numpy(), relu=False)
        assert cb.ratio(got, ref, S, K, 'bf16').max() <= 1.0, 'reg_bbox %s forward' % tag
    given = dict(gamma=gamma.detach().cpu().numpy(), beta=beta.detach().cpu().numpy())
    br.grade_forward('reg_bbox bn', dict(y=yn, mean=mean.cpu().numpy(), var=var.cpu().numpy()), br.ROUND['bf16'](hn), given['gamma'], given['beta'],
                     1, bc.EPS, 'bf16')
    br.grade_backward('reg_bbox bn', dict(dx=dh.cpu().numpy(), dgamma=dgamma.cpu().numpy(), dbeta=dbeta.cpu().numpy()), br.ROUND['bf16'](hn),
                      br.dz_of(yn, dyn, 'bf16', 1), given['gamma'], mean.cpu().numpy(), var.cpu().numpy(), bc.EPS, 'bf16')
    for tag, xin, w, dz_in, got in (('conv2', yn, w2, g.cpu().numpy(), (dy, dw2, db2)), ('conv1', x.detach().cpu().numpy(), w1, dh.cpu().numpy(), (dxe, dw1, db1))):
        seen = cgr.seen(xin, w.detach().cpu().numpy(), None, dz_in, 'bf16', 0)
        ref = cgr.grads64(*seen)
        cgr.check('reg_bbox %s' % tag, {n_: None if t_ is None else t_.cpu().numpy() for n_, t_ in zip(('dx', 'dw', 'db'), got)}, ref, 'bf16', 'gauss')
