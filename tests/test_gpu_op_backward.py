"""GPU parity of the pool backward (ron_maxpool2x2_backward_nhwc) and of the 2x2 stride-2 convolution backwards
(ron_conv2d_k2s2_backward_nhwc) against the references of tests/op_grad_ref.py on the cases of tests/op_grad_cases.py.

  pool   the result is exact: np.array_equal with the reference on Gaussian and relu(Gaussian) inputs (the latter hold four-way ties
         and two-way ties of the maximum that start behind position (0,0)), and on the hand windows;
  k2s2   kind 'lattice': integer inputs, the three outputs must EQUAL the reference; kind 'gauss': graded per element by the derived
         bound (conv_bounds.ratio <= 1, no exclusions): conv_grad_ref.check unchanged;

and the contract of the entry points: pixel splits, the same bytes on every call, outputs fully overwritten, nothing assumed about
the workspace, NULL outputs, the caller's stream without a host synchronisation, and the autograd functions against the explicit
sequence of backward calls.

Each gauss case prints its largest ratios (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_grad_ref as cgr  # noqa: E402
import op_grad_cases as oc  # noqa: E402
import op_grad_ref as ogr  # noqa: E402
import stream_util as su  # noqa: E402

NAMES = ('dx', 'dw', 'db')


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


def _up(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _bytes(outs):
    return [None if t is None else t.cpu().numpy().tobytes() for t in outs]


def _clones(tensors):
    return [t.clone() for t in tensors]


# ------------------------------------------------------------------------------------------------------------------------ the pool
@functools.lru_cache(maxsize=None)
def _pool_case(kind, case, dtype):
    """Inputs and the reference of one pool case, computed once and shared (never modified)."""
    x, dy = oc.pool_inputs(kind, case)
    if kind == 'relu':
        oc.assert_pool_ties(dtype)
    return (x, dy), ogr.pool_backward(x, dy, dtype)


@pytest.mark.parametrize('kind', oc.POOL_KINDS)
@pytest.mark.parametrize('dtype', oc.DTYPES)
@pytest.mark.parametrize('case', sorted(oc.POOL_CASES))
def test_pool_backward_parity(ops, dev, case, dtype, kind):
    given, want = _pool_case(kind, case, dtype)
    x, dy = _up(given, dev)
    got = ops.maxpool2x2_backward_nhwc(x, dy, dtype).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), '%s %s %s: %d elements differ' % (case, dtype, kind, int((got != want).sum()))
    # the window's gradient lands on one position: the forward's maximum sits there
    y = ops.maxpool2x2_nhwc(x, dtype).cpu().numpy()
    assert np.array_equal(y, ogr._positions(cgr.ROUND[dtype](given[0]), np.float32(-np.inf))[0].max(axis=0))


@pytest.mark.parametrize('dtype', oc.DTYPES)
def test_pool_hand_cases(ops, dev, dtype):
    x, dy, want = oc.pool_hand_inputs()
    got = ops.maxpool2x2_backward_nhwc(*_up((x, dy), dev), dtype).cpu().numpy()
    for i, (label, _, pos) in enumerate(oc.POOL_HAND):
        flat = got[i].reshape(4, 8)
        assert np.array_equal(flat[pos], dy[i, 0, 0]), '%s: the gradient is not at position %d' % (label, pos)
        assert not np.delete(flat, pos, axis=0).any(), '%s: gradient outside position %d' % (label, pos)
    assert np.array_equal(got, ogr.pool_backward(x, dy, dtype))


def _pool_raw(x, dy, dx, dtype='bf16'):
    from ron_tensorflow_amd import _lib
    n, h, w, c = x.shape
    _lib.check(_lib.lib().ron_maxpool2x2_backward_nhwc(_lib.ptr(x), _lib.ptr(dy), n, h, w, c, _lib.DTYPES[dtype], _lib.ptr(dx), _lib.current_stream()))
    return dx


@pytest.mark.parametrize('case', ['odd', 'oddrows', 'wide'])
def test_pool_output_prefilled_with_nan_is_overwritten_and_calls_repeat(ops, dev, case):
    given, want = _pool_case('relu', case, 'bf16')
    x, dy = _up(given, dev)
    a = _pool_raw(x, dy, torch.full_like(x, float('nan')))
    b = _pool_raw(x, dy, torch.full_like(x, float('nan')))
    assert np.array_equal(a.cpu().numpy(), want)
    assert _bytes([a]) == _bytes([b]), 'two calls differ'


def _pool_late_setup(ops, dev):
    given, _ = _pool_case('relu', 'oddrows', 'bf16')
    poison, _ = _pool_case('gauss', 'oddrows', 'bf16')
    x, xp = _up(given, dev), _up(poison, dev)

    def entry(t):
        return [ops.maxpool2x2_backward_nhwc(t[0], t[1], 'bf16')]
    expected = _clones(entry(x))
    bufs = _clones(xp)
    poisoned = _clones(entry(bufs))
    torch.cuda.synchronize()
    assert not su.same_bytes(expected, poisoned)

    def fill():
        for b, t in zip(bufs, x):
            b.copy_(t, non_blocking=True)
    return entry, x, bufs, expected, fill


def test_pool_stream_contract_late_inputs(ops, dev, side):
    entry, x, bufs, expected, fill = _pool_late_setup(ops, dev)
    got = su.run_late(side, fill, lambda: entry(bufs), _clones, label='maxpool2x2_backward_nhwc')
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


def test_pool_stream_contract_control_misdirected(ops, dev, side):
    entry, x, bufs, expected, fill = _pool_late_setup(ops, dev)
    got = su.run_misdirected(side, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), 'a call on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(_clones(bufs), _clones(x))


# ---------------------------------------------------------------------------------------------------------------------------- k2s2
@functools.lru_cache(maxsize=8)
def _case(kind, case, dtype, relu):
    """Inputs and the float64 reference of one case, computed once and shared by the tests that use it (never modified)."""
    x, w, y, dy = oc.k2s2_inputs(kind, case)
    g = ogr.grads64_k2s2(*cgr.seen(x, w, y, dy, dtype, relu), oc.K2S2_CASES[case][5])
    if kind == 'lattice':
        oc.k2s2_assert_lattice(case, w, g)
    return (x, w, y, dy), g


def _host(outs):
    return {n: None if t is None else t.cpu().numpy() for n, t in zip(NAMES, outs)}


def _call(ops, tensors, case, dtype, relu, **kw):
    x, w, y, dy = tensors
    return ops.conv2d_k2s2_backward_nhwc(x, w, dy, y if relu else None, relu=bool(relu), transpose=bool(oc.K2S2_CASES[case][5]), dtype=dtype, **kw)


def _ws_bytes(ops, case, **kw):
    n, h, w, cin, cout, tr = oc.K2S2_CASES[case]
    return ops.conv2d_k2s2_backward_workspace_bytes(n, h, w, cin, cout, transpose=bool(tr), **kw)


def _raw(ops, tensors, case, dtype, relu, outs, workspace, splitk=-1):
    """The C entry with caller-made outputs and workspace (the wrapper allocates its own)."""
    from ron_tensorflow_amd import _lib
    n, h, w, cin, cout, tr = oc.K2S2_CASES[case]
    x, wt, y, dy = tensors
    d = _lib.ConvDesc(n, h, w, cin, cout, 2, 2, 2, 1, int(relu), tr, _lib.DTYPES[dtype], -1, 0, 0, 0, splitk, 0)
    assert workspace.numel() >= _lib.lib().ron_conv2d_k2s2_backward_workspace_bytes(C.byref(d))
    _lib.check(_lib.lib().ron_conv2d_k2s2_backward_nhwc(C.byref(d), _lib.ptr(x), _lib.ptr(wt), _lib.ptr(y if relu else None), _lib.ptr(dy),
                                                        _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(workspace),
                                                        int(workspace.numel()), _lib.current_stream()))
    return outs


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('kind', oc.KINDS)
@pytest.mark.parametrize('dtype', oc.DTYPES)
@pytest.mark.parametrize('case', sorted(oc.K2S2_CASES))
def test_k2s2_backward_parity(ops, dev, case, dtype, kind, relu):
    given, g = _case(kind, case, dtype, relu)
    got = _host(_call(ops, _up(given, dev), case, dtype, relu))
    cgr.check('%s %s relu=%d' % (case, kind, relu), got, g, dtype, kind)


@pytest.mark.parametrize('kind', oc.KINDS)
@pytest.mark.parametrize('case', ['c_k30', 'c_split', 't_k30', 't_split'])
def test_k2s2_pixel_splits(ops, dev, case, kind):
    """splitk -1 (by shape), 1 (off), 2 and 7 (forced): the exact result on the lattice, inside the bound on gauss inputs, and the
    same bytes from two calls of each setting."""
    given, g = _case(kind, case, 'bf16', 1)
    tensors = _up(given, dev)
    for sk in (-1, 1, 2, 7):
        a = _call(ops, tensors, case, 'bf16', 1, splitk=sk)
        b = _call(ops, tensors, case, 'bf16', 1, splitk=sk)
        cgr.check('%s %s splitk=%d' % (case, kind, sk), _host(a), g, 'bf16', kind)
        assert _bytes(a) == _bytes(b), 'splitk %d: two calls differ' % sk


def _fresh_outputs(tensors, fill):
    x, w, _, dy = tensors
    return [torch.full_like(x, fill), torch.full_like(w, fill), torch.full((dy.shape[3],), fill, dtype=torch.float32, device=x.device)]


@pytest.mark.parametrize('case', ['c_k30', 'c_126', 't_k30', 't_192'])
def test_k2s2_outputs_prefilled_with_nan_are_overwritten(ops, dev, case):
    given, g = _case('lattice', case, 'bf16', 1)
    tensors = _up(given, dev)
    ws = torch.empty((_ws_bytes(ops, case),), dtype=torch.uint8, device=dev)
    outs = _raw(ops, tensors, case, 'bf16', 1, _fresh_outputs(tensors, float('nan')), ws)
    cgr.check(case, _host(outs), g, 'bf16', 'lattice')


@pytest.mark.parametrize('case', ['c_k30', 't_k30'])
def test_k2s2_outputs_need_no_16_byte_alignment(ops, dev, case):
    """Only x, y and dy are read 16 bytes at a time: outputs that are merely 4-byte aligned get the same bytes."""
    given, g = _case('gauss', case, 'bf16', 1)
    tensors = _up(given, dev)
    ws = torch.empty((_ws_bytes(ops, case),), dtype=torch.uint8, device=dev)
    want = _raw(ops, tensors, case, 'bf16', 1, _fresh_outputs(tensors, float('nan')), ws)
    outs = []
    for t in want:
        buf = torch.full((t.numel() + 1,), float('nan'), dtype=torch.float32, device=dev)
        outs.append(buf[1:].view(t.shape))
        assert outs[-1].data_ptr() % 16 == 4
    got = _raw(ops, tensors, case, 'bf16', 1, outs, ws)
    assert _bytes(got) == _bytes(want)
    cgr.check(case, _host(got), g, 'bf16', 'gauss')


def test_k2s2_nothing_is_assumed_about_the_workspace(ops, dev):
    """A workspace of 0xFF bytes (NaN in every 2- and 4-byte format), then the same buffer straight after a call of another shape:
    results as with the wrapper's own buffer."""
    order = ('c_tiles', 'c_k30', 't_192', 't_k30')
    nbytes = max(_ws_bytes(ops, c) for c in order)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    for case in order:
        for kind in oc.KINDS:
            given, g = _case(kind, case, 'bf16', 1)
            tensors = _up(given, dev)
            want = _bytes(_call(ops, tensors, case, 'bf16', 1))
            if case in ('c_tiles', 't_192'):
                ws.fill_(0xFF)
            outs = _raw(ops, tensors, case, 'bf16', 1, _fresh_outputs(tensors, float('nan')), ws)
            cgr.check('%s %s' % (case, kind), _host(outs), g, 'bf16', kind)
            assert _bytes(outs) == want


@pytest.mark.parametrize('need', [('dx',), ('dw',), ('db',), ('dx', 'db'), ('dw', 'db')])
def test_k2s2_null_outputs_leave_the_others_unchanged(ops, dev, need):
    for case in ('c_k30', 'c_tiles', 't_k30', 't_split'):
        given, _ = _case('gauss', case, 'bf16', 1)
        tensors = _up(given, dev)
        full = dict(zip(NAMES, _bytes(_call(ops, tensors, case, 'bf16', 1))))
        part = _call(ops, tensors, case, 'bf16', 1, need=need)
        for name, t in zip(NAMES, part):
            if name in need:
                assert t.cpu().numpy().tobytes() == full[name], '%s: %s differs when only %s is computed' % (case, name, need)
            else:
                assert t is None


def _late_setup(ops, dev, case):
    given, _ = _case('gauss', case, 'bf16', 1)
    poison, _ = _case('lattice', case, 'bf16', 1)          # another valid case of the same shapes
    x, xp = _up(given, dev), _up(poison, dev)

    def entry(t):
        return list(_call(ops, t, case, 'bf16', 1))
    expected = _clones(entry(x))
    bufs = _clones(xp)
    poisoned = _clones(entry(bufs))
    torch.cuda.synchronize()
    assert not su.same_bytes(expected, poisoned)

    def fill():
        for b, t in zip(bufs, x):
            b.copy_(t, non_blocking=True)
    return entry, x, bufs, expected, fill


@pytest.mark.parametrize('case', ['c_k30', 't_k30'])
def test_k2s2_stream_contract_late_inputs(ops, dev, side, case):
    """On a stalled side stream, with the real inputs copied into the buffers behind the stall: the call does not wait for the host
    and reads nothing early - the result has the default-stream result's bytes."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev, case)
    got = su.run_late(side, fill, lambda: entry(bufs), _clones, label='conv2d_k2s2_backward_nhwc')
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


@pytest.mark.parametrize('case', ['c_k30', 't_k30'])
def test_k2s2_stream_contract_control_misdirected(ops, dev, side, case):
    """Positive control: the same late inputs with the call on the default stream must NOT give the expected result."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev, case)
    got = su.run_misdirected(side, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), 'a call on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(_clones(bufs), _clones(x))


# ------------------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize('f_needs_grad', [False, True])
def test_autograd_reverse_connection_is_the_explicit_calls(ops, dev, f_needs_grad):
    """The reverse-connection module, ref = relu(relu(conv3x3(pool(f)) + b1) + relu(deconv2x2(r) + b2)): .backward() gives, bit for
    bit, what the explicit sequence of backward calls gives on the same saved tensors, each branch masked by its OWN output (the
    outer ReLU is the identity on a sum of two non-negative maps); tensors that do not require grad get None.

    Shapes: the pooled feature map and the up-sampled coarse map must agree, and the test forward of the transposed convolution
    wants 128 output channels: f is (1,16,16,64) -> pool (1,8,8,64) -> conv (1,8,8,128); r is (1,4,4,64) -> (1,8,8,128)."""
    rs = np.random.RandomState(7)

    def t(a, grad):
        return torch.from_numpy(a.astype(np.float32)).to(dev).requires_grad_(grad)
    f = t(rs.randn(1, 16, 16, 64), f_needs_grad)
    r = t(rs.randn(1, 4, 4, 64), True)
    w1, b1 = t(rs.randn(3, 3, 64, 128) * np.sqrt(2.0 / 576), True), t(rs.randn(128) * 0.1, True)
    w2, b2 = t(rs.randn(2, 2, 128, 64) * np.sqrt(2.0 / 64), True), t(rs.randn(128) * 0.1, False)          # b2 does not require grad
    g = torch.from_numpy(rs.randn(1, 8, 8, 128).astype(np.float32)).to(dev)
    p = ops.maxpool2x2_nhwc_fn(f)
    a = ops.conv2d_nhwc_fn(p, w1, b1, relu=True)
    b = ops.conv2d_k2s2_nhwc_fn(r, w2, b2, relu=True, transpose=True)
    ref = torch.relu(a + b)
    (ref * g).sum().backward()
    with torch.no_grad():
        dref = torch.where(ref > 0, g, torch.zeros_like(g))
        dp, dw1, db1 = ops.conv2d_backward_nhwc(p.detach(), w1.detach(), dref, a.detach(), relu=True,
                                                need=('dx', 'dw', 'db') if f_needs_grad else ('dw', 'db'))
        df = ops.maxpool2x2_backward_nhwc(f.detach(), dp) if f_needs_grad else None
        dr, dw2, db2 = ops.conv2d_k2s2_backward_nhwc(r.detach(), w2.detach(), dref, b.detach(), relu=True, transpose=True, need=('dx', 'dw'))
        assert db2 is None
    assert b2.grad is None
    assert _bytes([w1.grad, b1.grad, r.grad, w2.grad]) == _bytes([dw1, db1, dr, dw2])
    if f_needs_grad:
        assert _bytes([f.grad]) == _bytes([df])
        assert float(f.grad.abs().max()) > 0
    else:
        assert f.grad is None and dp is None
    assert float(w1.grad.abs().max()) > 0 and float(w2.grad.abs().max()) > 0 and float(r.grad.abs().max()) > 0
