"""GPU tests of the training forward ron_conv2d_forward_nhwc (ops.conv2d_forward_nhwc): device weights, packed on the stream.

  * the same bytes as the host-packed test operator ops.conv2d_nhwc on the same values - every case, dtype, ReLU and bias setting;
  * per element inside the derived bound of tests/conv_bounds.py against its float64 conv_op on Gaussian data, and EQUAL to it on
    the integer lattices (what catches a transposed, shifted or dropped weight whatever the host pack does);
  * the contract: y fully overwritten, nothing assumed about the workspace, nothing written outside it, nothing cached between
    calls, the work on the caller's stream without a host synchronisation.

Each gauss case prints its largest ratio (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_bounds as cb  # noqa: E402
import conv_fwd_cases as cf  # noqa: E402
import stream_util as su  # noqa: E402
from conv_grad_ref import ROUND  # noqa: E402

# one more shape than the table of the CPU tests needs to name: a 3x3 over 64 channels on a map the 8 x 32 tile divides, which the
# planner gives to the resident-weight kernel - the launch that reads a second, differently laid out weight image
CASES = dict(cf.CASES, c64=(1, 8, 32, 64, 64, 3, 1, 1, 0))
CONTRACT = ('B', 'K7over', 'cout1', 'cout65', 'c64', 'stem', 'stemrag', 's2', 't2')


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


@functools.lru_cache(maxsize=None)
def _inputs(kind, case):
    return cf.inputs(kind, CASES[case])


@functools.lru_cache(maxsize=8)
def _raw_ref(kind, case, dtype):
    """conv_op of the operands as the kernels see them, without bias and activation: (conv, conv of magnitudes, K) in float64,
    computed once per case and shared (never modified); _ref adds the bias and the ReLU as conv_op itself does."""
    x, w, _ = _inputs(kind, case)
    n, h, wd, cin, cout, k, rate, stride, tr = CASES[case]
    return cb.conv_op(ROUND[dtype](x), ROUND[dtype](w), None, stride=stride, rate=rate, relu=False, transpose=bool(tr))


def _ref(kind, case, dtype, relu, bias):
    raw, mag, K = _raw_ref(kind, case, dtype)
    if bias is not None:
        raw, mag = raw + bias.astype(np.float64), mag + np.abs(bias.astype(np.float64))
    return (np.maximum(raw, 0) if relu else raw), mag, K


def _kw(case, dtype, relu):
    n, h, wd, cin, cout, k, rate, stride, tr = CASES[case]
    return dict(relu=bool(relu), dilation=rate, stride=stride, transpose=bool(tr), dtype=dtype)


def _up(arrays, dev):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _raw(ops, case, dtype, relu, x, w, b, y, ws):
    """The C entry with a caller-made output and workspace (the wrapper allocates its own)."""
    from ron_tensorflow_amd import _lib
    n, h, wd, cin, cout, k, rate, stride, tr = CASES[case]
    d = _lib.ConvDesc(n, h, wd, cin, cout, k, k, stride, rate, int(relu), tr, _lib.DTYPES[dtype], -1, 0, 0, 0, -1, 0)
    need = _lib.lib().ron_conv2d_forward_workspace_bytes(C.byref(d))
    assert 0 < need <= ws.numel()
    _lib.check(_lib.lib().ron_conv2d_forward_nhwc(C.byref(d), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), _lib.ptr(ws), int(ws.numel()),
                                                  _lib.current_stream()))
    return y


def _need(ops, case, dtype, relu):
    n, h, wd, cin, cout, k, rate, stride, tr = CASES[case]
    return ops.conv2d_forward_workspace_bytes(n, h, wd, cin, cout, k, stride=stride, dilation=rate, relu=bool(relu), transpose=bool(tr), dtype=dtype)


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('dtype', cf.DTYPES)
@pytest.mark.parametrize('case', sorted(CASES))
def test_forward_parity(ops, dev, case, dtype, relu):
    for kind in ('lattice', 'gauss'):
        x, w, b = _inputs(kind, case)
        xd, wd, bd = _up((x, w, b), dev)
        for bias in (True, False):
            y = ops.conv2d_forward_nhwc(xd, wd, bd if bias else None, **_kw(case, dtype, relu)).cpu().numpy()
            assert y.shape == cf.out_shape(CASES[case])
            host = ops.conv2d_nhwc(xd, w, b if bias else None, **_kw(case, dtype, relu)).cpu().numpy()
            tag = '%s %s %s relu=%d bias=%d' % (case, dtype, kind, relu, bias)
            assert np.array_equal(y, host), '%s: %d elements differ from the host-packed operator' % (tag, int((y != host).sum()))
            ref64, S, K = _ref(kind, case, dtype, relu, b if bias else None)
            if kind == 'lattice':
                assert np.abs(ref64).max() < 256 and np.array_equal(ref64, np.round(ref64)) and ref64.any()
                assert np.array_equal(y, ref64.astype(np.float32)), '%s: differs from the exact integer result in %d elements' % (
                    tag, int((y != ref64).sum()))
            else:
                r = cb.ratio(y, ref64, S, K, dtype)
                print('%s: largest error / bound %.3f at %s' % ((tag,) + cb.worst(r)))
                assert r.max() <= 1.0, '%s: error / bound %g at %s' % ((tag,) + cb.worst(r))


# ------------------------------------------------------------------------------------------------------------------ contract
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('case', CONTRACT)
def test_workspace_and_output_contract(ops, dev, case, relu):
    """y pre-filled with NaN comes back without one; a workspace of 0xFF bytes, of float32 NaNs and of 16-bit NaNs gives the bytes a
    zeroed one gives; carved at exactly the sizer's length out of a larger buffer, the bytes in front of and behind it are untouched."""
    x, w, b = _inputs('gauss', case)
    xd, wd, bd = _up((x, w, b), dev)
    need = _need(ops, case, 'bf16', relu)
    guard = 4096
    big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    ws = big[guard:guard + need]
    assert ws.data_ptr() % 256 == 0 and ws.numel() == need
    want = ops.conv2d_forward_nhwc(xd, wd, bd, **_kw(case, 'bf16', relu)).cpu().numpy()
    fills = {'zero': lambda: ws.zero_(), '0xFF': lambda: ws.fill_(0xFF),
             'fp32 NaN': lambda: ws[:need // 4 * 4].view(torch.int32).fill_(0x7FC00000),
             '16-bit NaN': lambda: ws[:need // 2 * 2].view(torch.int16).fill_(0x7FC0),
             'fp16 NaN': lambda: ws[:need // 2 * 2].view(torch.int16).fill_(0x7E00)}
    for name, fill in fills.items():
        fill()
        y = torch.full(cf.out_shape(CASES[case]), float('nan'), dtype=torch.float32, device=dev)
        got = _raw(ops, case, 'bf16', relu, xd, wd, bd, y, ws).cpu().numpy()
        assert not np.isnan(got).any(), '%s: %d NaN survive in y' % (name, int(np.isnan(got).sum()))
        assert got.tobytes() == want.tobytes(), 'workspace of %s: the result differs' % name
    edges = torch.cat([big[:guard], big[guard + need:]]).cpu().numpy()
    assert (edges == 0xA5).all(), 'bytes outside the workspace were written'


@pytest.mark.parametrize('case', CONTRACT)
def test_nothing_is_cached_between_calls(ops, dev, case):
    """Two calls give the same bytes; after w.mul_(2) IN PLACE (the same pointer, as the optimizer leaves it) the third call is the
    convolution of the new weights: doubling is exact in every format and commutes with the ReLU, so without a bias y doubles exactly."""
    x, w, _ = _inputs('gauss', case)
    xd, wd = _up((x, w), dev)
    kw = _kw(case, 'bf16', 1)
    a = ops.conv2d_forward_nhwc(xd, wd, None, **kw).cpu().numpy()
    b = ops.conv2d_forward_nhwc(xd, wd, None, **kw).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    wd.mul_(2)
    c = ops.conv2d_forward_nhwc(xd, wd, None, **kw).cpu().numpy()
    assert a.any() and np.array_equal(c, 2 * a), 'the third call did not follow the weights changed in place'


def _late_setup(ops, dev, case):
    given, poison = _inputs('gauss', case), _inputs('lattice', case)          # two valid sets of values of the same shapes
    x, xp = _up(given, dev), _up(poison, dev)
    kw = _kw(case, 'bf16', 1)

    def entry(t):
        return [ops.conv2d_forward_nhwc(t[0], t[1], t[2], **kw)]
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


@pytest.mark.parametrize('case', ['B', 'stem', 't2'])
def test_stream_contract_late_inputs(ops, dev, side, case):
    """On a stalled side stream, with x, w and bias copied into their buffers behind the stall: the call does not wait for the host and
    reads nothing early - not the weights either, which it packs on the stream."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev, case)
    got = su.run_late(side, fill, lambda: entry(bufs), _clones, label='conv2d_forward_nhwc %s' % case)
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


def test_stream_contract_control_misdirected(ops, dev, side):
    """Positive control: the same late inputs with the call on the default stream must NOT give the expected result."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev, 'B')
    got = su.run_misdirected(side, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), 'a call on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(_clones(bufs), _clones(x))
