"""GPU parity per element of the stem backward (ron_conv2d_stem_backward_nhwc): dw and db against the float64 reference of
tests/stem_grad_ref.py on the cases of tests/stem_grad_cases.py, twice -

  kind 'lattice'  integer inputs whose every product and partial sum is exact in any accumulation order: both outputs must EQUAL
                  the reference (np.array_equal): what catches flipped or transposed taps, the k order, taps that leak into a
                  neighbouring row or image, the mask, lost pixels;
  kind 'gauss'    Gaussian inputs graded per element by the derived bound (conv_bounds.ratio <= 1, no exclusions): what catches a
                  missing rounding.

and the contract of the entry point: every pixel split gives the exact result and the same bytes on every call, outputs are fully
overwritten, nothing is assumed about the workspace, a NULL output leaves the other unchanged, the work runs on the caller's stream
without a host synchronisation, and the autograd function at cin 3 is exactly the explicit call.

Each gauss case prints its largest ratios (pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_grad_ref as cgr  # noqa: E402
import stem_grad_cases as sc  # noqa: E402
import stem_grad_ref as ref  # noqa: E402
import stream_util as su  # noqa: E402

NAMES = ('dw', 'db')


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


@functools.lru_cache(maxsize=64)
def _case(kind, case, dtype, relu):
    """Inputs and the float64 reference of one case, computed once and shared by the tests that use it (never modified)."""
    x, y, dy = sc.inputs(kind, case)
    xs, dz = ref.seen(x, y, dy, dtype, relu)
    if kind == 'lattice':
        sc.assert_lattice(x, dz, list(cgr.ROUND.values()))
    return (x, y, dy), ref.grads64(xs, dz)


def _up(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _host(outs):
    return {n: None if t is None else t.cpu().numpy() for n, t in zip(NAMES, outs)}


def _call(ops, tensors, dtype, relu, **kw):
    x, y, dy = tensors
    return ops.conv2d_stem_backward_nhwc(x, dy, y if relu else None, relu=bool(relu), dtype=dtype, **kw)


def _raw(tensors, case, dtype, relu, outs, workspace, splitk=-1):
    """The C entry with caller-made outputs and workspace (the wrapper allocates its own)."""
    from ron_tensorflow_amd import _lib
    n, h, w = sc.CASES[case]
    x, y, dy = tensors
    d = _lib.ConvDesc(n, h, w, 3, 64, 3, 3, 1, 1, int(relu), 0, _lib.DTYPES[dtype], -1, 0, 0, 0, splitk, 0)
    assert workspace.numel() >= _lib.lib().ron_conv2d_stem_backward_workspace_bytes(C.byref(d))
    _lib.check(_lib.lib().ron_conv2d_stem_backward_nhwc(C.byref(d), _lib.ptr(x), _lib.ptr(y if relu else None), _lib.ptr(dy),
                                                        _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(workspace),
                                                        int(workspace.numel()), _lib.current_stream()))
    return outs


def _bytes(outs):
    return [None if t is None else t.cpu().numpy().tobytes() for t in outs]


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('dtype', sc.DTYPES)
@pytest.mark.parametrize('case', sorted(sc.CASES))
def test_stem_backward_parity(ops, dev, case, dtype, kind, relu):
    given, g = _case(kind, case, dtype, relu)
    got = _host(_call(ops, _up(given, dev), dtype, relu))
    cgr.check('%s %s relu=%d' % (case, kind, relu), got, g, dtype, kind)
    if case == 'A':          # a 1 x 1 map: the eight taps that only see what lies outside it
        off_centre = np.ones((3, 3), bool)
        off_centre[1, 1] = False
        assert not got['dw'][off_centre].any() and got['dw'][1, 1].any()


@pytest.mark.parametrize('kind', sc.KINDS)
@pytest.mark.parametrize('case', ['B', 'G'])
def test_pixel_splits(ops, dev, case, kind):
    """splitk -1 (by shape), 1 (off), 2, 7 and 1000 (forced; capped at the number of steps): the exact result on the lattice, inside
    the bound on gauss inputs, and the same bytes from two calls of each setting."""
    given, g = _case(kind, case, 'bf16', 1)
    tensors = _up(given, dev)
    for sk in (-1, 1, 2, 7, 1000):
        a = _call(ops, tensors, 'bf16', 1, splitk=sk)
        b = _call(ops, tensors, 'bf16', 1, splitk=sk)
        cgr.check('%s %s splitk=%d' % (case, kind, sk), _host(a), g, 'bf16', kind)
        assert _bytes(a) == _bytes(b), 'splitk %d: two calls differ' % sk


# ------------------------------------------------------------------------------------------------------------------ contract
def _fresh_outputs(dev, fill):
    return [torch.full((3, 3, 3, 64), fill, dtype=torch.float32, device=dev), torch.full((64,), fill, dtype=torch.float32, device=dev)]


@pytest.mark.parametrize('case', ['A', 'B', 'G'])
def test_outputs_prefilled_with_nan_are_overwritten(ops, dev, case):
    given, g = _case('lattice', case, 'bf16', 1)
    tensors = _up(given, dev)
    ws = torch.empty((ops.conv2d_stem_backward_workspace_bytes(*sc.CASES[case]),), dtype=torch.uint8, device=dev)
    outs = _raw(tensors, case, 'bf16', 1, _fresh_outputs(dev, float('nan')), ws)
    cgr.check(case, _host(outs), g, 'bf16', 'lattice')


@pytest.mark.parametrize('case', ['B', 'G'])
def test_nothing_is_assumed_about_the_workspace(ops, dev, case):
    """A workspace of 0xFF bytes (NaN in every 2- and 4-byte format) gives the bytes of a zeroed one."""
    nbytes = ops.conv2d_stem_backward_workspace_bytes(*sc.CASES[case])
    for kind in sc.KINDS:
        given, g = _case(kind, case, 'bf16', 1)
        tensors = _up(given, dev)
        zeroed = _raw(tensors, case, 'bf16', 1, _fresh_outputs(dev, float('nan')), torch.zeros((nbytes,), dtype=torch.uint8, device=dev))
        poisoned = _raw(tensors, case, 'bf16', 1, _fresh_outputs(dev, float('nan')), torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev))
        cgr.check('%s %s' % (case, kind), _host(poisoned), g, 'bf16', kind)
        assert _bytes(poisoned) == _bytes(zeroed)


@pytest.mark.parametrize('need', [('dw',), ('db',)])
def test_null_output_leaves_the_other_unchanged(ops, dev, need):
    for case in ('B', 'G'):
        given, _ = _case('gauss', case, 'bf16', 1)
        tensors = _up(given, dev)
        full = dict(zip(NAMES, _bytes(_call(ops, tensors, 'bf16', 1))))
        part = _call(ops, tensors, 'bf16', 1, need=need)
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
        return list(_call(ops, t, 'bf16', 1))
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
    got = su.run_late(side, fill, lambda: entry(bufs), _clones, label='conv2d_stem_backward_nhwc')
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


def test_stream_contract_control_misdirected(ops, dev, side):
    """Positive control: the same late inputs with the call on the default stream must NOT give the expected result."""
    entry, x, bufs, expected, fill = _late_setup(ops, dev)
    got = su.run_misdirected(side, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), 'a call on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(_clones(bufs), _clones(x))


# ------------------------------------------------------------------------------------------------------------------ autograd
def _param(rs, shape, scale, dev, grad=True):
    return torch.from_numpy((rs.randn(*shape) * scale).astype(np.float32)).to(dev).requires_grad_(grad)


def test_autograd_at_cin_3_is_the_explicit_call(ops, dev):
    rs = np.random.RandomState(11)
    n, h, w = sc.CASES['B']
    img = torch.from_numpy((60.0 * rs.randn(n, h, w, 3)).astype(np.float32)).to(dev)
    w1, b1 = _param(rs, (3, 3, 3, 64), 0.01, dev), _param(rs, (64,), 0.1, dev)
    dy = torch.from_numpy(rs.randn(n, h, w, 64).astype(np.float32)).to(dev)
    y = ops.conv2d_nhwc_fn(img, w1, b1, relu=True)
    y.backward(dy)
    with torch.no_grad():
        dw, db = ops.conv2d_stem_backward_nhwc(img, dy, y.detach(), relu=True)
    assert img.grad is None
    assert _bytes([w1.grad, b1.grad]) == _bytes([dw, db])
    assert float(w1.grad.abs().max()) > 0 and float(b1.grad.abs().max()) > 0


def test_autograd_refuses_the_gradient_of_the_image(ops, dev):
    from ron_tensorflow_amd import _lib
    rs = np.random.RandomState(12)
    n, h, w = sc.CASES['B']
    img = _param(rs, (n, h, w, 3), 60.0, dev)
    w1, b1 = _param(rs, (3, 3, 3, 64), 0.01, dev), _param(rs, (64,), 0.1, dev)
    y = ops.conv2d_nhwc_fn(img, w1, b1, relu=True)
    with pytest.raises(_lib.RonError):
        y.backward(torch.ones_like(y))


def test_autograd_chain_from_the_image_to_pool1(ops, dev):
    """image -> conv1_1 -> conv1_2 -> pool1 at (2, 6, 10): .backward() gives w1, b1, w2, b2 gradients equal, byte for byte, to the
    explicit calls of the three backward entries in sequence."""
    rs = np.random.RandomState(13)
    n, h, w = 2, 6, 10
    img = torch.from_numpy((60.0 * rs.randn(n, h, w, 3)).astype(np.float32)).to(dev)
    w1, b1 = _param(rs, (3, 3, 3, 64), 0.01, dev), _param(rs, (64,), 0.1, dev)
    w2, b2 = _param(rs, (3, 3, 64, 64), np.sqrt(2.0 / 576), dev), _param(rs, (64,), 0.1, dev)
    dy = torch.from_numpy(rs.randn(n, h // 2, w // 2, 64).astype(np.float32)).to(dev)
    y1 = ops.conv2d_nhwc_fn(img, w1, b1, relu=True)
    y2 = ops.conv2d_nhwc_fn(y1, w2, b2, relu=True)
    ops.maxpool2x2_nhwc_fn(y2).backward(dy)
    with torch.no_grad():
        d2 = ops.maxpool2x2_backward_nhwc(y2.detach(), dy)
        dx2, dw2, db2 = ops.conv2d_backward_nhwc(y1.detach(), w2.detach(), d2, y2.detach(), relu=True)
        dw1, db1 = ops.conv2d_stem_backward_nhwc(img, dx2, y1.detach(), relu=True)
    assert _bytes([w1.grad, b1.grad, w2.grad, b2.grad]) == _bytes([dw1, db1, dw2, db2])
    for t in (w1.grad, b1.grad, w2.grad, b2.grad):
        assert float(t.abs().max()) > 0
