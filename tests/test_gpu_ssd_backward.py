"""GPU parity of the backward of the SSD-only operators against the references of tests/ssd_grad_ref.py on the cases of
tests/ssd_grad_cases.py.

  pool     ron_maxpool3x3s1_backward_nhwc: exact - np.array_equal with the float32 reference on Gaussian, relu(Gaussian) and coarse
           inputs (the latter hold tied maxima that do not start their window) and on the hand windows;
  L2 norm  ron_l2norm_backward_nhwc: Gaussian inputs graded per element by the derived bound of ssd_grad_ref (no exclusions), the
           exact lattice with np.array_equal; an all-zero pixel between live ones;
  conv     ron_conv2d_padded_backward_nhwc: lattice inputs must EQUAL the float64 reference, gauss inputs stay inside conv_bounds'
           bound with the K of the full-resolution problem; the block12 route through the k2s2 entry point;

and the contract of the entry points: outputs fully overwritten, nothing assumed about the workspace, NULL outputs, the same bytes
on every call, the caller's stream without a host synchronisation, and the autograd functions against the explicit sequence of
backward calls.  Each gauss case prints its largest ratios (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_grad_ref as cgr  # noqa: E402
import ssd_grad_cases as sc  # noqa: E402
import ssd_grad_ref as sr  # noqa: E402
import stream_util as su  # noqa: E402

NAMES = ('dx', 'dw', 'db')
NAN = float('nan')


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


def _late(side, ops_entry, x, xp, label):
    """(result on the stalled side stream, result of the misdirected control, expected, bufs, x): stream_util's two patterns."""
    expected = _clones(ops_entry(x))
    bufs = _clones(xp)
    poisoned = _clones(ops_entry(bufs))
    torch.cuda.synchronize()
    assert not su.same_bytes(expected, poisoned)

    def fill():
        for b, t in zip(bufs, x):
            b.copy_(t, non_blocking=True)
    got = su.run_late(side, fill, lambda: ops_entry(bufs), _clones, label=label)
    assert su.same_bytes(got, expected), '%s: the result on the stalled stream differs from the default-stream result' % label
    for b, t in zip(bufs, xp):          # the poison again, for the control
        b.copy_(t)
    got = su.run_misdirected(side, fill, lambda: ops_entry(bufs), _clones)
    assert not su.same_bytes(got, expected), '%s: a call on the wrong stream went unnoticed: the harness cannot fail' % label
    assert su.same_bytes(_clones(bufs), _clones(x))


# ------------------------------------------------------------------------------------------------------------------------ the pool
@functools.lru_cache(maxsize=None)
def _pool_case(kind, case, dtype):
    x, dy = sc.pool_inputs(kind, case)
    return (x, dy), sr.pool3_backward(x, dy, dtype)


@pytest.mark.parametrize('kind', sc.POOL_KINDS)
@pytest.mark.parametrize('dtype', sc.DTYPES)
@pytest.mark.parametrize('case', sorted(sc.POOL_CASES))
def test_pool_backward_parity(ops, dev, case, dtype, kind):
    given, want = _pool_case(kind, case, dtype)
    if kind == 'coarse' and case not in ('one', 'two'):
        assert sr.pool3_late_ties(given[0], dtype) > 0
    x, dy = _up(given, dev)
    got = ops.maxpool3x3s1_backward_nhwc(x, dy, dtype).cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), '%s %s %s: %d elements differ' % (case, dtype, kind, int((got != want).sum()))
    if kind != 'gauss':          # the forward test operator: TensorFlow's pool for non-negative inputs
        assert np.array_equal(ops.maxpool3x3s1_nhwc(x, dtype).cpu().numpy(), sr.pool3_forward(given[0], dtype))


@pytest.mark.parametrize('dtype', sc.DTYPES)
def test_pool_hand_cases(ops, dev, dtype):
    x, dy = sc.pool_hand_inputs()
    got = ops.maxpool3x3s1_backward_nhwc(*_up((x, dy), dev), dtype).cpu().numpy()
    want = sc.pool_hand_expected()
    for i, (label, _, _, pos) in enumerate(sc.POOL_HAND):
        assert np.array_equal(got[i], want[i]), '%s: the gradient is not at position %s alone' % (label, pos)
    assert np.array_equal(got, sr.pool3_backward(x, dy, dtype))


def _pool_raw(x, dy, dx, dtype='bf16'):
    from ron_tensorflow_amd import _lib
    n, h, w, c = x.shape
    _lib.check(_lib.lib().ron_maxpool3x3s1_backward_nhwc(_lib.ptr(x), _lib.ptr(dy), n, h, w, c, _lib.DTYPES[dtype], _lib.ptr(dx), _lib.current_stream()))
    return dx


@pytest.mark.parametrize('case', ['rows', 'odd', 'pool5'])
def test_pool_output_prefilled_with_nan_is_overwritten_and_calls_repeat(ops, dev, case):
    given, want = _pool_case('coarse', case, 'bf16')
    x, dy = _up(given, dev)
    a = _pool_raw(x, dy, torch.full_like(x, NAN))
    b = _pool_raw(x, dy, torch.full_like(x, NAN))
    assert np.array_equal(a.cpu().numpy(), want)
    assert su.same_bytes([a], [b]), 'two calls differ'


def test_pool_stream_contract(ops, dev, side):
    given, _ = _pool_case('coarse', 'odd', 'bf16')
    poison, _ = _pool_case('gauss', 'odd', 'bf16')
    _late(side, lambda t: [ops.maxpool3x3s1_backward_nhwc(t[0], t[1], 'bf16')], _up(given, dev), _up(poison, dev), 'maxpool3x3s1_backward_nhwc')


# ------------------------------------------------------------------------------------------------------------- the L2 normalisation
@functools.lru_cache(maxsize=None)
def _l2_case(kind, case):
    given = sc.l2_inputs(kind, case)
    if kind == 'lattice':
        sc.l2_assert_lattice(*given)
    return given


def _l2_host(outs):
    return {n: None if t is None else t.cpu().numpy() for n, t in zip(('dx', 'dgamma'), outs)}


@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('dtype', sc.DTYPES)
@pytest.mark.parametrize('case', sorted(sc.L2_CASES))
def test_l2norm_backward_parity(ops, dev, case, dtype, kind):
    given = _l2_case(kind, case)
    x, gamma, dy = _up(given, dev)
    got = _l2_host(ops.l2norm_backward_nhwc(x, gamma, dy, dtype=dtype))
    sr.l2_check(case, got, *given, dtype, kind)
    # the forward test operator against the float64 forward: one rounding of the output on top of the float32 arithmetic
    y = ops.l2norm_nhwc(x, gamma, dtype=dtype).cpu().numpy()
    y64 = sr.l2_forward64(cgr.ROUND[dtype](given[0]), given[1])
    if kind == 'lattice':
        assert np.array_equal(y, y64)
    else:
        A = 8 * -(-given[0].shape[3] // 512) + 6          # the forward's lanes add 8 channels per pass of 512, then the butterfly
        uh = sr.cb.U_HALF_ULP[dtype]
        assert (np.abs(y - y64) <= uh * np.abs(y64) + (1 + uh) * (A / 2 + 4) * sr.EPS * np.abs(y64) + 2.0 ** -25).all()


@pytest.mark.parametrize('dtype', sc.DTYPES)
def test_l2norm_all_zero_pixel_between_live_ones(ops, dev, dtype):
    given = sc.l2_dead_pixel_inputs()
    x, gamma, dy = _up(given, dev)
    got = _l2_host(ops.l2norm_backward_nhwc(x, gamma, dy, dtype=dtype))
    sr.l2_check('dead pixel', got, *given, dtype, 'gauss')
    rnd = cgr.ROUND[dtype]
    want = rnd((rnd(given[2][0, 0, 1]) * given[1]) * (np.float32(1) / np.sqrt(np.float32(1e-12))))
    assert np.isfinite(got['dx']).all() and np.abs(got['dx'][0, 0, 1]).max() > 1e3
    assert np.array_equal(got['dx'][0, 0, 1], want)          # dy gamma 1e6: the same three float32 operations


def _l2_raw(tensors, outs, ws, dtype='bf16'):
    from ron_tensorflow_amd import _lib
    x, gamma, dy = tensors
    n, h, w, c = x.shape
    assert ws.numel() >= _lib.lib().ron_l2norm_backward_workspace_bytes(n, h, w, c, _lib.DTYPES[dtype])
    _lib.check(_lib.lib().ron_l2norm_backward_nhwc(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(dy), n, h, w, c, _lib.DTYPES[dtype], _lib.ptr(outs[0]),
                                                   _lib.ptr(outs[1]), _lib.ptr(ws), int(ws.numel()), _lib.current_stream()))
    return outs


@pytest.mark.parametrize('case', ['m5_c72', 'm1444_c512', 'm2049_c8'])
def test_l2norm_contract(ops, dev, case):
    """NaN-filled outputs, a workspace of 0xFF bytes, each output passed as NULL, two calls with the same bytes."""
    for kind in sc.KINDS:
        given = _l2_case(kind, case)
        tensors = _up(given, dev)
        x, gamma, dy = tensors
        want = _clones(ops.l2norm_backward_nhwc(x, gamma, dy))
        ws = torch.full((ops.l2norm_backward_workspace_bytes(*x.shape),), 0xFF, dtype=torch.uint8, device=dev)
        a = _l2_raw(tensors, [torch.full_like(x, NAN), torch.full_like(gamma, NAN)], ws)
        sr.l2_check(case, _l2_host(a), *given, 'bf16', kind)
        b = _l2_raw(tensors, [torch.full_like(x, NAN), torch.full_like(gamma, NAN)], ws)          # the workspace as the first call left it
        assert su.same_bytes(a, b) and su.same_bytes(a, want)
        only_dx = _l2_raw(tensors, [torch.full_like(x, NAN), None], ws.fill_(0xFF))
        only_dg = _l2_raw(tensors, [None, torch.full_like(gamma, NAN)], ws.fill_(0xFF))
        assert su.same_bytes([only_dx[0], only_dg[1]], want)
        dx, dg = ops.l2norm_backward_nhwc(x, gamma, dy, need=('dgamma',))
        assert dx is None and su.same_bytes([dg], want[1:])


def test_l2norm_stream_contract(ops, dev, side):
    given, poison = _l2_case('gauss', 'm257_c72'), _l2_case('lattice', 'm257_c72')
    _late(side, lambda t: list(ops.l2norm_backward_nhwc(t[0], t[1], t[2])), _up(given, dev), _up(poison, dev), 'l2norm_backward_nhwc')


# ------------------------------------------------------------------------------------------------------------ the padded convolutions
@functools.lru_cache(maxsize=8)
def _conv_case(kind, case, dtype, relu):
    return sc.padded_reference(kind, case, dtype, relu)


def _conv_host(outs):
    return {n: None if t is None else t.cpu().numpy() for n, t in zip(NAMES, outs)}


def _conv_call(ops, tensors, case, dtype, relu, **kw):
    stride, cpad = sc.PADDED_CASES[case][5:]
    x, w, y, dy = tensors
    return ops.conv2d_padded_backward_nhwc(x, w, dy, y if relu else None, stride=stride, cpad=cpad, relu=bool(relu), dtype=dtype, **kw)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('dtype', sc.DTYPES)
@pytest.mark.parametrize('case', sorted(sc.PADDED_CASES))
def test_padded_backward_parity(ops, dev, case, dtype, kind, relu):
    given, g = _conv_case(kind, case, dtype, relu)
    got = _conv_host(_conv_call(ops, _up(given, dev), case, dtype, relu))
    cgr.check('%s %s relu=%d' % (case, kind, relu), got, g, dtype, kind)


@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('case', ['s2_5x4', 's2_19', 'v_5x5'])
def test_padded_pixel_splits(ops, dev, case, kind):
    given, g = _conv_case(kind, case, 'bf16', 1)
    tensors = _up(given, dev)
    for sk in (-1, 1, 2, 7):
        a = _conv_call(ops, tensors, case, 'bf16', 1, splitk=sk)
        b = _conv_call(ops, tensors, case, 'bf16', 1, splitk=sk)
        cgr.check('%s %s splitk=%d' % (case, kind, sk), _conv_host(a), g, 'bf16', kind)
        assert _bytes(a) == _bytes(b), 'splitk %d: two calls differ' % sk


def _conv_raw(tensors, case, outs, ws, dtype='bf16', relu=1):
    from ron_tensorflow_amd import _lib
    n, h, w, cin, cout, stride, cpad = sc.PADDED_CASES[case]
    x, wt, y, dy = tensors
    d = _lib.ConvDesc(n, h, w, cin, cout, 3, 3, stride, 1, int(relu), 0, _lib.DTYPES[dtype], -1, 0, 0, 0, -1, 0)
    assert ws.numel() >= _lib.lib().ron_conv2d_padded_backward_workspace_bytes(C.byref(d), cpad)
    _lib.check(_lib.lib().ron_conv2d_padded_backward_nhwc(C.byref(d), cpad, _lib.ptr(x), _lib.ptr(wt), _lib.ptr(y if relu else None), _lib.ptr(dy),
                                                          _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(ws), int(ws.numel()),
                                                          _lib.current_stream()))
    return outs


def _fresh(tensors, fill):
    x, w, _, dy = tensors
    return [torch.full_like(x, fill), torch.full_like(w, fill), torch.full((dy.shape[3],), fill, dtype=torch.float32, device=x.device)]


def test_padded_outputs_and_workspace(ops, dev):
    """NaN-filled outputs and a workspace of 0xFF bytes, then the same buffer straight after a call of another shape."""
    sizes = {c: ops.conv2d_padded_backward_workspace_bytes(*sc.PADDED_CASES[c][:5], stride=sc.PADDED_CASES[c][5], cpad=sc.PADDED_CASES[c][6])
             for c in ('s2_5x4', 'v_5x5', 's2_2x2')}
    ws = torch.full((max(sizes.values()),), 0xFF, dtype=torch.uint8, device=dev)
    for case in ('v_5x5', 's2_5x4', 's2_2x2'):
        for kind in sc.KINDS:
            given, g = _conv_case(kind, case, 'bf16', 1)
            tensors = _up(given, dev)
            want = _bytes(_conv_call(ops, tensors, case, 'bf16', 1))
            if case == 'v_5x5':
                ws.fill_(0xFF)
            outs = _conv_raw(tensors, case, _fresh(tensors, NAN), ws)
            cgr.check('%s %s' % (case, kind), _conv_host(outs), g, 'bf16', kind)
            assert _bytes(outs) == want


@pytest.mark.parametrize('need', [('dx',), ('dw',), ('db',), ('dx', 'db'), ('dw', 'db')])
def test_padded_null_outputs_leave_the_others_unchanged(ops, dev, need):
    for case in ('s2_5x4', 'v_3x3'):
        given, _ = _conv_case('gauss', case, 'bf16', 1)
        tensors = _up(given, dev)
        full = dict(zip(NAMES, _bytes(_conv_call(ops, tensors, case, 'bf16', 1))))
        part = _conv_call(ops, tensors, case, 'bf16', 1, need=need)
        for name, t in zip(NAMES, part):
            if name in need:
                assert t.cpu().numpy().tobytes() == full[name], '%s differs when only %s is computed' % (name, need)
            else:
                assert t is None


@pytest.mark.parametrize('dtype', sc.DTYPES)
@pytest.mark.parametrize('kind', sc.KINDS)
def test_block12_route(ops, dev, kind, dtype):
    """pad2d(1) + 4x4 VALID on a 2x2 map through ron_conv2d_k2s2_backward_nhwc on w[1:3, 1:3]: the float64 reference of the padded
    4x4 convolution; the twelve outer taps of dw are exactly zero."""
    given = sc.block12_inputs(kind)
    g = sc.block12_grads64(*cgr.seen(*given, dtype, 1))
    x, w, y, dy = _up(given, dev)
    got = _conv_host(ops.conv2d_padded_backward_nhwc(x, w, dy, y, stride=1, cpad=1, relu=True, dtype=dtype))
    cgr.check('block12 %s' % kind, got, g, dtype, kind)
    outer = np.ones((4, 4), bool)
    outer[1:3, 1:3] = False
    assert not got['dw'][outer].any() and got['dw'][1:3, 1:3].any()
    with pytest.raises(Exception):
        ops.conv2d_padded_backward_nhwc(x, w[:, :, :, :], dy, y, stride=2, cpad=1)          # a 4x4 filter anywhere else


def test_padded_stream_contract(ops, dev, side):
    given, _ = _conv_case('gauss', 's2_5x4', 'bf16', 1)
    poison, _ = _conv_case('lattice', 's2_5x4', 'bf16', 1)
    _late(side, lambda t: list(_conv_call(ops, t, 's2_5x4', 'bf16', 1)), _up(given, dev), _up(poison, dev), 'conv2d_padded_backward_nhwc')


# ------------------------------------------------------------------------------------------------------------------------ autograd
def _t(rs, shape, scale, dev, grad=True):
    return torch.from_numpy((rs.randn(*shape) * scale).astype(np.float32)).to(dev).requires_grad_(grad)


def test_autograd_block4_branch(ops, dev):
    """conv (ReLU) -> l2norm_fn -> 3x3 head conv on a (1, 6, 6, 512) map: .backward() gives, bit for bit, the explicit calls."""
    rs = np.random.RandomState(11)
    x = _t(rs, (1, 6, 6, 512), 1.0, dev)
    w1, b1 = _t(rs, (3, 3, 512, 512), np.sqrt(2.0 / 4608), dev), _t(rs, (512,), 0.1, dev)
    gamma = torch.full((512,), 20.0, device=dev).requires_grad_(True)
    w2, b2 = _t(rs, (3, 3, 512, 24), np.sqrt(2.0 / 4608), dev), _t(rs, (24,), 0.1, dev)
    dy = _t(rs, (1, 6, 6, 24), 1.0, dev, grad=False)
    y1 = ops.conv2d_nhwc_fn(x, w1, b1, relu=True)
    y2 = ops.l2norm_nhwc_fn(y1, gamma)
    y3 = ops.conv2d_nhwc_fn(y2, w2, b2, relu=False)
    y3.backward(dy)
    with torch.no_grad():
        d2, dw2, db2 = ops.conv2d_backward_nhwc(y2.detach(), w2.detach(), dy, None, relu=False)
        d1, dgamma = ops.l2norm_backward_nhwc(y1.detach(), gamma.detach(), d2)
        dx, dw1, db1 = ops.conv2d_backward_nhwc(x.detach(), w1.detach(), d1, y1.detach(), relu=True)
    assert su.same_bytes([x.grad, w1.grad, b1.grad, gamma.grad, w2.grad, b2.grad], [dx, dw1, db1, dgamma, dw2, db2])
    assert float(gamma.grad.abs().max()) > 0 and float(x.grad.abs().max()) > 0


def test_autograd_pool5_to_block8(ops, dev):
    """maxpool3x3s1_fn -> conv (rate 6) -> 1x1 -> 1x1 -> padded 3x3 stride 2 on a (1, 5, 5, .) map against the explicit calls."""
    rs = np.random.RandomState(12)
    x = torch.from_numpy(np.maximum(rs.randn(1, 5, 5, 128), 0).astype(np.float32)).to(dev).requires_grad_(True)
    w6, b6 = _t(rs, (3, 3, 128, 256), np.sqrt(2.0 / 1152), dev), _t(rs, (256,), 0.1, dev)
    w7, b7 = _t(rs, (1, 1, 256, 256), np.sqrt(2.0 / 256), dev), _t(rs, (256,), 0.1, dev)
    w8a, b8a = _t(rs, (1, 1, 256, 64), np.sqrt(2.0 / 256), dev), _t(rs, (64,), 0.1, dev)
    w8b, b8b = _t(rs, (3, 3, 64, 128), np.sqrt(2.0 / 576), dev), _t(rs, (128,), 0.1, dev)
    dy = _t(rs, (1, 3, 3, 128), 1.0, dev, grad=False)
    p5 = ops.maxpool3x3s1_nhwc_fn(x)
    y6 = ops.conv2d_nhwc_fn(p5, w6, b6, relu=True, dilation=6)
    y7 = ops.conv2d_nhwc_fn(y6, w7, b7, relu=True)
    y8a = ops.conv2d_nhwc_fn(y7, w8a, b8a, relu=True)
    y8 = ops.conv2d_padded_nhwc_fn(y8a, w8b, b8b, stride=2, cpad=1, relu=True)
    assert tuple(y8.shape) == (1, 3, 3, 128)
    y8.backward(dy)
    with torch.no_grad():
        d8a, dw8b, db8b = ops.conv2d_padded_backward_nhwc(y8a.detach(), w8b.detach(), dy, y8.detach(), stride=2, cpad=1, relu=True)
        d7, dw8a, db8a = ops.conv2d_backward_nhwc(y7.detach(), w8a.detach(), d8a, y8a.detach(), relu=True)
        d6, dw7, db7 = ops.conv2d_backward_nhwc(y6.detach(), w7.detach(), d7, y7.detach(), relu=True)
        dp5, dw6, db6 = ops.conv2d_backward_nhwc(p5.detach(), w6.detach(), d6, y6.detach(), relu=True, dilation=6)
        dx = ops.maxpool3x3s1_backward_nhwc(x.detach(), dp5)
    assert su.same_bytes([x.grad, w6.grad, b6.grad, w7.grad, b7.grad, w8a.grad, b8a.grad, w8b.grad, b8b.grad],
                         [dx, dw6, db6, dw7, db7, dw8a, db8a, dw8b, db8b])
    assert float(x.grad.abs().max()) > 0
    # the forward of the padded convolution: the stride-1 SAME convolution of the same operands, sampled
    full = ops.conv2d_nhwc(y8a.detach(), w8b.detach().cpu().numpy(), b8b.detach().cpu().numpy(), relu=True)
    assert su.same_bytes([y8.detach()], [full[:, ::2, ::2].contiguous()])
    with pytest.raises(Exception):
        ops.conv2d_padded_nhwc_fn(y8a, w8b, b8b, stride=2, cpad=0)
