"""GPU parity per element of the convolution backward (ron_conv2d_backward_nhwc): dx, dw and db against the float64 reference of
tests/conv_grad_ref.py on the cases of tests/conv_grad_cases.py, twice -

  kind 'lattice'  integer inputs whose every product and partial sum is exact in any accumulation order: the three outputs must
                  EQUAL the reference (np.array_equal): what catches flipped taps, swapped channels, the mask, halos, lost pixels;
  kind 'gauss'    Gaussian inputs graded per element by the derived bound (conv_bounds.ratio <= 1, no exclusions): what catches a
                  missing rounding.

and the contract of the entry point: every pixel split gives the exact result and the same bytes on every call, outputs are fully
overwritten, nothing is assumed about the workspace, NULL outputs leave the others unchanged, the work runs on the caller's stream
without a host synchronisation, and the autograd function is exactly two explicit calls.

Each gauss case prints its largest ratios (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_grad_cases as cg  # noqa: E402
import conv_grad_ref as ref  # noqa: E402
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


@functools.lru_cache(maxsize=8)
def _case(kind, case, dtype, relu):
    """Inputs and the float64 reference of one case, computed once and shared by the tests that use it (never modified)."""
    x, w, y, dy = cg.inputs(kind, case)
    g = ref.grads64(*ref.seen(x, w, y, dy, dtype, relu), cg.CASES[case][6])
    if kind == 'lattice':
        cg.assert_lattice(w, g['dx'][0], g['dw'][0], g['db'][0])
    return (x, w, y, dy), g


def _up(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _host(outs):
    return {n: None if t is None else t.cpu().numpy() for n, t in zip(NAMES, outs)}


def _call(ops, tensors, case, dtype, relu, **kw):
    x, w, y, dy = tensors
    return ops.conv2d_backward_nhwc(x, w, dy, y if relu else None, relu=bool(relu), dilation=cg.CASES[case][6], dtype=dtype, **kw)


def _raw(ops, tensors, case, dtype, relu, outs, workspace, splitk=-1):
    """The C entry with caller-made outputs and workspace (the wrapper allocates its own)."""
    from ron_tensorflow_amd import _lib
    n, h, w, cin, cout, k, rate = cg.CASES[case]
    x, wt, y, dy = tensors
    d = _lib.ConvDesc(n, h, w, cin, cout, k, k, 1, rate, int(relu), 0, _lib.DTYPES[dtype], -1, 0, 0, 0, splitk, 0)
    assert workspace.numel() >= _lib.lib().ron_conv2d_backward_workspace_bytes(C.byref(d))
    _lib.check(_lib.lib().ron_conv2d_backward_nhwc(C.byref(d), _lib.ptr(x), _lib.ptr(wt), _lib.ptr(y if relu else None), _lib.ptr(dy),
                                                   _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(workspace),
                                                   int(workspace.numel()), _lib.current_stream()))
    return outs


def _bytes(outs):
    return [None if t is None else t.cpu().numpy().tobytes() for t in outs]


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('kind', cg.KINDS)
@pytest.mark.parametrize('dtype', cg.DTYPES)
@pytest.mark.parametrize('case', sorted(cg.CASES))
def test_backward_parity(ops, dev, case, dtype, kind, relu):
    given, g = _case(kind, case, dtype, relu)
    got = _host(_call(ops, _up(given, dev), case, dtype, relu))
    ref.check('%s %s relu=%d' % (case, kind, relu), got, g, dtype, kind)
    if case == 'A':          # a 1 x 1 map: the eight taps that only see the halo
        off_centre = np.ones((3, 3), bool)
        off_centre[1, 1] = False
        assert not got['dw'][off_centre].any()


@pytest.mark.parametrize('kind', cg.KINDS)
@pytest.mark.parametrize('case', ['B', 'F', 'G'])
def test_pixel_splits(ops, dev, case, kind):
    """splitk -1 (by shape), 1 (off), 2 and 7 (forced): the exact result on the lattice, inside the bound on gauss inputs, and the
    same bytes from two calls of each setting."""
    given, g = _case(kind, case, 'bf16', 1)
    tensors = _up(given, dev)
    for sk in (-1, 1, 2, 7):
        a = _call(ops, tensors, case, 'bf16', 1, splitk=sk)
        b = _call(ops, tensors, case, 'bf16', 1, splitk=sk)
        ref.check('%s %s splitk=%d' % (case, kind, sk), _host(a), g, 'bf16', kind)
        assert _bytes(a) == _bytes(b), 'splitk %d: two calls differ' % sk


# ------------------------------------------------------------------------------------------------------------------ contract
def _fresh_outputs(tensors, fill):
    x, w, _, dy = tensors
    return [torch.full_like(x, fill), torch.full_like(w, fill), torch.full((dy.shape[3],), fill, dtype=torch.float32, device=x.device)]


@pytest.mark.parametrize('case', ['B', 'C', 'E'])
def test_outputs_prefilled_with_nan_are_overwritten(ops, dev, case):
    given, g = _case('lattice', case, 'bf16', 1)
    tensors = _up(given, dev)
    ws = torch.empty((ops.conv2d_backward_workspace_bytes(*cg.CASES[case][:6], dilation=cg.CASES[case][6]),), dtype=torch.uint8, device=dev)
    outs = _raw(ops, tensors, case, 'bf16', 1, _fresh_outputs(tensors, float('nan')), ws)
    ref.check(case, _host(outs), g, 'bf16', 'lattice')


def test_nothing_is_assumed_about_the_workspace(ops, dev):
    """A workspace of 0xFF bytes (NaN in every 2- and 4-byte format), then the same buffer straight after a call of another shape
    (D: dilation 6, 192 outputs; then B): results as with the wrapper's own buffer."""
    nbytes = max(ops.conv2d_backward_workspace_bytes(*cg.CASES[c][:6], dilation=cg.CASES[c][6]) for c in 'BD')
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    for case in ('D', 'B'):
        for kind in cg.KINDS:
            given, g = _case(kind, case, 'bf16', 1)
            tensors = _up(given, dev)
            want = _bytes(_call(ops, tensors, case, 'bf16', 1))
            if case == 'D':
                ws.fill_(0xFF)
            outs = _raw(ops, tensors, case, 'bf16', 1, _fresh_outputs(tensors, float('nan')), ws)
            ref.check('%s %s' % (case, kind), _host(outs), g, 'bf16', kind)
            assert _bytes(outs) == want


@pytest.mark.parametrize('need', [('dx',), ('dw',), ('db',), ('dx', 'db'), ('dw', 'db')])
def test_null_outputs_leave_the_others_unchanged(ops, dev, need):
    for case in ('B', 'F'):
        given, _ = _case('gauss', case, 'bf16', 1)
        tensors = _up(given, dev)
        full = dict(zip(NAMES, _bytes(_call(ops, tensors, case, 'bf16', 1))))
        part = _call(ops, tensors, case, 'bf16', 1, need=need)
        for name, t in zip(NAMES, part):
            if name in need:
                assert t.cpu().numpy().tobytes() == full[name], '%s differs when only %s is computed' % (name, need)
            else:
                assert t is None


def _late_setup(ops, dev):
    given, _ = _case('gauss', 'B', 'bf16', 1)
    poison, _ = _case('lattice', 'B', 'bf16', 1)          # another valid case of the same shapes
    x, xp = _up(given, dev), _up(poison, dev)

    def entry(t):
        return list(_call(ops, t, 'B', 'bf16', 1))
    expected = [t.clone() for t in entry(x)]
    bufs = [t.clone() for t in xp]
    poisoned = [t.clone() for t in entry(bufs)]
    torch.cuda.synchronize()
    assert not su.same_bytes(expected, poisoned)

    def fill():
        for b, t in zip(bufs, x):
            b.copy_(t, non_blocking=True)
    return entry, x, bufs, expected, fill


def _clones(tensors):
    return [t.clone() for t in tensors]


def test_stream_contract_late_inputs(ops, dev, side):
    """On a stalled side stream, with the real inputs copied into the buffers behind the stall: the call does not wait for the host
    and reads nothing early - the result has the default-stream result's bytes."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev)
    got = su.run_late(side, fill, lambda: entry(bufs), _clones, label='conv2d_backward_nhwc')
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


def test_stream_contract_control_misdirected(ops, dev, side):
    """Positive control: the same late inputs with the call on the default stream must NOT give the expected result."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev)
    got = su.run_misdirected(side, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), 'a call on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(_clones(bufs), _clones(x))


# ------------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize('x_needs_grad', [False, True])
def test_autograd_chain_is_two_explicit_calls(ops, dev, x_needs_grad):
    """conv 64 -> 64 (ReLU, bias) -> conv 64 -> 24 (no ReLU, bias) on case B's map: .backward() gives, bit for bit, what two explicit
    conv2d_backward_nhwc calls give; tensors that do not require grad get None."""
    n, h, w = cg.CASES['B'][:3]
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.randn(n, h, w, 64).astype(np.float32)).to(dev).requires_grad_(x_needs_grad)
    w1 = torch.from_numpy((rs.randn(3, 3, 64, 64) * np.sqrt(2.0 / 576)).astype(np.float32)).to(dev).requires_grad_(True)
    b1 = torch.from_numpy((rs.randn(64) * 0.1).astype(np.float32)).to(dev).requires_grad_(True)
    w2 = torch.from_numpy((rs.randn(3, 3, 64, 24) * np.sqrt(2.0 / 576)).astype(np.float32)).to(dev).requires_grad_(True)
    b2 = torch.from_numpy((rs.randn(24) * 0.1).astype(np.float32)).to(dev)              # does not require grad
    dy = torch.from_numpy(rs.randn(n, h, w, 24).astype(np.float32)).to(dev)
    y1 = ops.conv2d_nhwc_fn(x, w1, b1, relu=True)
    y2 = ops.conv2d_nhwc_fn(y1, w2, b2, relu=False)
    y2.backward(dy)
    with torch.no_grad():
        dx2, dw2, db2 = ops.conv2d_backward_nhwc(y1.detach(), w2.detach(), dy, None, relu=False, need=('dx', 'dw'))
        assert db2 is None
        dx1, dw1, db1 = ops.conv2d_backward_nhwc(x.detach(), w1.detach(), dx2, y1.detach(), relu=True,
                                                 need=('dx', 'dw', 'db') if x_needs_grad else ('dw', 'db'))
    assert b2.grad is None
    assert _bytes([w2.grad, w1.grad, b1.grad]) == _bytes([dw2, dw1, db1])
    if x_needs_grad:
        assert _bytes([x.grad]) == _bytes([dx1])
    else:
        assert x.grad is None and dx1 is None
    assert float(w1.grad.abs().max()) > 0 and float(w2.grad.abs().max()) > 0
