"""GPU tests of the 7 x 7 backward (fc6 of the `full` variant through ron_conv2d_backward_nhwc) and of the whole differentiable
chain with device weights only.

  * dx, dw and db of the three 7 x 7 shapes of tests/conv_fwd_cases.py against the float64 reference of tests/conv_grad_ref.py, with
    the grading of test_gpu_conv_backward.py: exact on the integer lattices, per element inside the derived bound on Gaussian data;
  * the contract at pad 3: pixel splits, NULL outputs, NaN-filled outputs, a poisoned workspace;
  * conv2d_nhwc_fn at k = 7 and one chain stem -> 3x3 -> pool -> dilated 3x3 -> 2x2 stride 2 -> 2x2 transposed -> 1x1 head through
    autograd: bit for bit the explicit forward / backward calls, no weight ever on the host."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_fwd_cases as cf  # noqa: E402
import conv_grad_cases as cg  # noqa: E402
import conv_grad_ref as ref  # noqa: E402

NAMES = ('dx', 'dw', 'db')
K7 = sorted(cf.K7_GRAD)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=8)
def _case(kind, case, dtype, relu):
    """Inputs and the float64 reference of one case, computed once and shared by the tests that use it (never modified)."""
    x, w, y, dy = cg.inputs(kind, cf.K7_GRAD[case])
    g = ref.grads64(*ref.seen(x, w, y, dy, dtype, relu), 1)
    if kind == 'lattice':
        cg.assert_lattice(w, g['dx'][0], g['dw'][0], g['db'][0])
    return (x, w, y, dy), g


def _up(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _host(outs):
    return {n: None if t is None else t.cpu().numpy() for n, t in zip(NAMES, outs)}


def _bytes(outs):
    return [None if t is None else t.cpu().numpy().tobytes() for t in outs]


def _call(ops, tensors, dtype, relu, **kw):
    x, w, y, dy = tensors
    return ops.conv2d_backward_nhwc(x, w, dy, y if relu else None, relu=bool(relu), dilation=1, dtype=dtype, **kw)


def _raw(ops, tensors, case, outs, workspace):
    """The C entry with caller-made outputs and workspace (bf16, ReLU, split by shape)."""
    from ron_tensorflow_amd import _lib
    n, h, w, cin, cout, k, rate = cf.K7_GRAD[case]
    x, wt, y, dy = tensors
    d = _lib.ConvDesc(n, h, w, cin, cout, k, k, 1, rate, 1, 0, _lib.DTYPES['bf16'], -1, 0, 0, 0, -1, 0)
    assert workspace.numel() >= _lib.lib().ron_conv2d_backward_workspace_bytes(C.byref(d)) > 0
    _lib.check(_lib.lib().ron_conv2d_backward_nhwc(C.byref(d), _lib.ptr(x), _lib.ptr(wt), _lib.ptr(y), _lib.ptr(dy), _lib.ptr(outs[0]),
                                                   _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(workspace), int(workspace.numel()),
                                                   _lib.current_stream()))
    return outs


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('kind', cg.KINDS)
@pytest.mark.parametrize('dtype', cg.DTYPES)
@pytest.mark.parametrize('case', K7)
def test_backward_parity_7x7(ops, dev, case, dtype, kind, relu):
    given, g = _case(kind, case, dtype, relu)
    got = _host(_call(ops, _up(given, dev), dtype, relu))
    ref.check('%s %s relu=%d' % (case, kind, relu), got, g, dtype, kind)


@pytest.mark.parametrize('kind', cg.KINDS)
@pytest.mark.parametrize('case', K7)
def test_pixel_splits_7x7(ops, dev, case, kind):
    """splitk -1 (by shape), 1 (off) and 3 (forced): exact on the lattice, inside the bound on gauss inputs, the same bytes twice."""
    given, g = _case(kind, case, 'bf16', 1)
    tensors = _up(given, dev)
    for sk in (-1, 1, 3):
        a = _call(ops, tensors, 'bf16', 1, splitk=sk)
        b = _call(ops, tensors, 'bf16', 1, splitk=sk)
        ref.check('%s %s splitk=%d' % (case, kind, sk), _host(a), g, 'bf16', kind)
        assert _bytes(a) == _bytes(b), 'splitk %d: two calls differ' % sk


# ------------------------------------------------------------------------------------------------------------------ contract
@pytest.mark.parametrize('case', K7)
def test_nan_outputs_and_a_poisoned_workspace_7x7(ops, dev, case):
    """Outputs pre-filled with NaN are overwritten and a workspace of 0xFF bytes (NaN in every 2- and 4-byte format) gives the result
    of the wrapper's own buffer: the pad-3 halos and guard pixels are all written by the call."""
    for kind in cg.KINDS:
        given, g = _case(kind, case, 'bf16', 1)
        tensors = _up(given, dev)
        x, w, _, dy = tensors
        want = _bytes(_call(ops, tensors, 'bf16', 1))
        n, h, wd, cin, cout, k, rate = cf.K7_GRAD[case]
        ws = torch.full((ops.conv2d_backward_workspace_bytes(n, h, wd, cin, cout, k),), 0xFF, dtype=torch.uint8, device=dev)
        nan = float('nan')
        outs = [torch.full_like(x, nan), torch.full_like(w, nan), torch.full((cout,), nan, dtype=torch.float32, device=dev)]
        outs = _raw(ops, tensors, case, outs, ws)
        ref.check('%s %s' % (case, kind), _host(outs), g, 'bf16', kind)
        assert _bytes(outs) == want


@pytest.mark.parametrize('need', [('dx',), ('dw',), ('db',), ('dx', 'db'), ('dw', 'db')])
def test_null_outputs_leave_the_others_unchanged_7x7(ops, dev, need):
    given, _ = _case('gauss', 'K7over', 'bf16', 1)
    tensors = _up(given, dev)
    full = dict(zip(NAMES, _bytes(_call(ops, tensors, 'bf16', 1))))
    part = _call(ops, tensors, 'bf16', 1, need=need)
    for name, t in zip(NAMES, part):
        if name in need:
            assert t.cpu().numpy().tobytes() == full[name], '%s differs when only %s is computed' % (name, need)
        else:
            assert t is None


# ------------------------------------------------------------------------------------------------------------------ autograd
def _param(rs, shape, scale, dev, grad=True):
    return torch.from_numpy((rs.randn(*shape) * scale).astype(np.float32)).to(dev).requires_grad_(grad)


def test_autograd_at_k7_is_the_explicit_calls(ops, dev):
    n, h, w, cin, cout, k, _ = cf.K7_GRAD['K7over']
    rs = np.random.RandomState(7)
    x = _param(rs, (n, h, w, cin), 1.0, dev)
    wt = _param(rs, (k, k, cin, cout), np.sqrt(2.0 / (k * k * cin)), dev)
    b = _param(rs, (cout,), 0.1, dev)
    dy = torch.from_numpy(rs.randn(n, h, w, cout).astype(np.float32)).to(dev)
    y = ops.conv2d_nhwc_fn(x, wt, b, relu=True)
    y.backward(dy)
    with torch.no_grad():
        ye = ops.conv2d_forward_nhwc(x.detach(), wt.detach(), b.detach(), relu=True)
        dx, dw, db = ops.conv2d_backward_nhwc(x.detach(), wt.detach(), dy, ye, relu=True)
    assert _bytes([y.detach(), x.grad, wt.grad, b.grad]) == _bytes([ye, dx, dw, db])
    assert float(wt.grad.abs().max()) > 0 and float(x.grad.abs().max()) > 0


def test_training_chain_through_autograd_is_the_explicit_calls(ops, dev):
    """image [2,16,32,3] -> stem -> 3x3 (64 -> 64: the resident-weight kernel) -> 2x2 pool -> 3x3 at dilation 2 (64 -> 128) -> 2x2 stride 2
    (128 -> 128) -> 2x2 transposed (128 -> 128) -> 1x1 head (128 -> 24, no ReLU).  Every weight is a device tensor; .backward() gives, bit
    for bit, the outputs of the explicit ron_*_forward / ron_*_backward calls in reverse order."""
    rs = np.random.RandomState(11)
    img = torch.from_numpy(rs.rand(2, 16, 32, 3).astype(np.float32) * 2 - 1).to(dev)
    P = {}
    for name, shape, fan in (('w1', (3, 3, 3, 64), 27), ('w2', (3, 3, 64, 64), 576), ('w3', (3, 3, 64, 128), 576), ('w4', (2, 2, 128, 128), 512),
                             ('w5', (2, 2, 128, 128), 128), ('w6', (1, 1, 128, 24), 128)):
        P[name] = _param(rs, shape, np.sqrt(2.0 / fan), dev)
        P['b' + name[1]] = _param(rs, (shape[2] if name == 'w5' else shape[3],), 0.1, dev)
    dy =torch.from_numpy(rs.randn(2, 8, 16, 24).astype(np.float32)).to(dev)
    a1 = ops.conv2d_nhwc_fn(img, P['w1'], P['b1'], relu=True)
    a2 = ops.conv2d_nhwc_fn(a1, P['w2'], P['b2'], relu=True)
    p2 = ops.maxpool2x2_nhwc_fn(a2)
    a3 = ops.conv2d_nhwc_fn(p2, P['w3'], P['b3'], relu=True, dilation=2)
    a4 = ops.conv2d_k2s2_nhwc_fn(a3, P['w4'], P['b4'], relu=True)
    a5 = ops.conv2d_k2s2_nhwc_fn(a4, P['w5'], P['b5'], relu=True, transpose=True)
    out = ops.conv2d_nhwc_fn(a5, P['w6'], P['b6'], relu=False)
    assert tuple(out.shape) == (2, 8, 16, 24)
    out.backward(dy)
    with torch.no_grad():
        D = {k: v.detach() for k, v in P.items()}
        e1 = ops.conv2d_forward_nhwc(img, D['w1'], D['b1'], relu=True)
        e2 = ops.conv2d_forward_nhwc(e1, D['w2'], D['b2'], relu=True)
        q2 = ops.maxpool2x2_nhwc(e2)
        e3 = ops.conv2d_forward_nhwc(q2, D['w3'], D['b3'], relu=True, dilation=2)
        e4 = ops.conv2d_forward_nhwc(e3, D['w4'], D['b4'], relu=True, stride=2)
        e5 = ops.conv2d_forward_nhwc(e4, D['w5'], D['b5'], relu=True, stride=2, transpose=True)
        eo = ops.conv2d_forward_nhwc(e5, D['w6'], D['b6'], relu=False)
        g5, dw6, db6 = ops.conv2d_backward_nhwc(e5, D['w6'], dy, None, relu=False)
        g4, dw5, db5 = ops.conv2d_k2s2_backward_nhwc(e4, D['w5'], g5, e5, relu=True, transpose=True)
        g3, dw4, db4 = ops.conv2d_k2s2_backward_nhwc(e3, D['w4'], g4, e4, relu=True)
        gq, dw3, db3 = ops.conv2d_backward_nhwc(q2, D['w3'], g3, e3, relu=True, dilation=2)
        g2 = ops.maxpool2x2_backward_nhwc(e2, gq)
        g1, dw2, db2 = ops.conv2d_backward_nhwc(e1, D['w2'], g2, e2, relu=True)
        dw1, db1 = ops.conv2d_stem_backward_nhwc(img, g1, e1, relu=True)
    assert _bytes([out.detach()]) == _bytes([eo])
    got = [P[k].grad for k in ('w1', 'b1', 'w2', 'b2', 'w3', 'b3', 'w4', 'b4', 'w5', 'b5', 'w6', 'b6')]
    assert all(g is not None and float(g.abs().max()) > 0 for g in got)
    assert _bytes(got) == _bytes([dw1, db1, dw2, db2, dw3, db3, dw4, db4, dw5, db5, dw6, db6])
