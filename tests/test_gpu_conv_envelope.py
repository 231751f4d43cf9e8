"""GPU parity at the last value of every geometry field of the convolution entry points (cases: tests/conv_envelope_cases.py; what
lies beyond is refused, tests/test_conv_envelope_cpu.py): dilation 31, 15 x 15 filters, SAME padding 62 and 63, stride 7, the 7 x 7
stride-7 transposed convolution - against the float64 reference of tests/conv_bounds.py, twice:

  kind 'lattice'  exact-integer inputs: the result must EQUAL the reference, in every dtype;
  kind 'gauss'    Gaussian inputs graded per element by the derived bound (ratio <= 1, no exclusions).

Every descriptor here is inside the envelope.  Each gauss case prints its largest ratio (pytest -s)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_bounds as cb  # noqa: E402
import conv_envelope_cases as ce  # noqa: E402
import conv_grad_cases as cg  # noqa: E402
import conv_grad_ref as gref  # noqa: E402
from test_gpu_conv import ROUND  # noqa: E402
from test_gpu_conv_exact import ALL4, KINDS, _grade  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=8)
def _case(kind, dtype, name, draw=0, relu=True, pool=False, bias=True):
    """Inputs and the float64 reference of one case, computed once and shared by the launches that use it (never modified)."""
    x, wt, b, res = ce.inputs(kind, name, draw)
    if not bias:
        b = None
    rnd = ROUND[dtype]
    ref = ce.reference(name, rnd(x), rnd(wt), b, None if res is None else rnd(res), relu=relu, pool=pool)
    return (x, wt, b, res), ref


def _run(ops, dev, kind, dtype, name, tag, tile_cfg=-1, splitk=-1):
    n, h, w, cin, cout, k, stride, dilation, transpose = ce.EDGE[name]
    top = 0.0
    for draw in range(ce.draws(name) if kind == 'lattice' else 1):
        (x, wt, b, res), (ref, S, K) = _case(kind, dtype, name, draw)
        got = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), wt, b, residual=None if res is None else torch.from_numpy(res).to(dev),
                              stride=stride, dilation=dilation, relu=True, transpose=bool(transpose), dtype=dtype, tile_cfg=tile_cfg,
                              splitk=splitk).cpu().numpy()
        top = max(top, _grade('%s %s %s' % (name, tag, kind), got, ref, S, K, dtype, kind))
    return top


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('name', ce.BY_SHAPE)
def test_edge_by_shape(ops, dev, name, dtype, kind):
    _run(ops, dev, kind, dtype, name, 'by shape')


@pytest.mark.parametrize('splitk', [1, 3])          # (varies fastest: the two launches share one reference)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('name', ce.SPLITK)
def test_edge_forced_splitk(ops, dev, name, splitk, dtype, kind):
    assert ops.conv_plan(*ce.EDGE[name][:5], k=ce.EDGE[name][5], dilation=ce.EDGE[name][7], dtype=dtype, splitk=splitk)['splitk'] == splitk
    _run(ops, dev, kind, dtype, name, 'splitk %d' % splitk, splitk=splitk)


@pytest.mark.parametrize('name,cfg', [(name, cfg) for name in sorted(ce.TAPS_INNER) for cfg in ce.TAPS_INNER[name]])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
def test_edge_taps_innermost(ops, dev, name, cfg, dtype, kind):
    """The chunk-major / taps-innermost K order (tile configurations 7 and 9, split-K off) where the planner accepts it for the shape:
    225 taps, and taps 31 pixels apart."""
    plan = ops.conv_plan(*ce.EDGE[name][:5], k=ce.EDGE[name][5], dilation=ce.EDGE[name][7], dtype=dtype, tile_cfg=cfg, splitk=1)
    assert plan['tile_cfg'] == cfg and plan['taps_inner'] == 1 and plan['splitk'] == 1
    _run(ops, dev, kind, dtype, name, 'cfg %d' % cfg, tile_cfg=cfg, splitk=1)


@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('tap', [(0, 0), (0, 14), (14, 0), (14, 14)], ids=lambda t: '%d_%d' % t)
def test_k15_corner_taps(ops, dev, tap, dtype):
    """A 15 x 15 filter whose only weight is one corner tap (the identity over the channels): the output is the input moved by exactly
    that tap, zeros where it falls into the halo - which names a mis-indexed tap instead of reporting a sum."""
    n, h, w, cin, cout, k, stride, dilation, transpose = ce.EDGE['k15']
    x = ce.inputs('lattice', 'k15')[0]
    want = ce.shifted(x, k, dilation, *tap)
    assert want.any()
    got = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), ce.one_hot_weights(k, cin, cout, *tap), None, relu=False, dtype=dtype).cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, 'tap %s %s: %d elements differ, first at %s: got %r, the shifted input %r' % (
        tap, dtype, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
def test_two_head_outputs_at_dilation_31(ops, dev, dtype, kind):
    """ron_conv2d_heads_nhwc: dil31 with its first 30 output channels split 6 / 24 into two fp32 tensors."""
    n, h, w, cin, cout, k, stride, dilation, transpose = ce.EDGE['dil31']
    (x, wt, b, _), _ = _case(kind, dtype, 'dil31')
    wt, b = np.ascontiguousarray(wt[..., :30]), b[:30]
    ref, S, K = cb.conv_op(ROUND[dtype](x), ROUND[dtype](wt), b, rate=dilation, relu=False)
    y1, y2 = ops.conv2d_heads_nhwc(torch.from_numpy(x).to(dev), wt, 6, bias=b, dilation=dilation, dtype=dtype)
    _grade('heads dil31 first %s' % kind, y1.cpu().numpy(), ref[..., :6], S[..., :6], K, dtype, kind, out_dtype='fp32')
    _grade('heads dil31 second %s' % kind, y2.cpu().numpy(), ref[..., 6:], S[..., 6:], K, dtype, kind, out_dtype='fp32')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
def test_fused_pool_at_dilation_31(ops, dev, dtype, kind):
    """ron_conv2d_pool2_nhwc: dil31 with the fused 2x2 pool and the un-pooled map from the same launch, against the float64 convolution
    and its pool64."""
    n, h, w, cin, cout, k, stride, dilation, transpose = ce.EDGE['dil31']
    (x, wt, b, _), (full, S, K) = _case(kind, dtype, 'dil31')
    yp, yf = ops.conv2d_pool2_nhwc(torch.from_numpy(x).to(dev), wt, b, relu=True, dtype=dtype, dilation=dilation)
    _grade('pool2 dil31 full %s' % kind, yf.cpu().numpy(), full, S, K, dtype, kind)
    _grade('pool2 dil31 pooled %s' % kind, yp.cpu().numpy(), cb.pool64(full), cb.pool64(S), K, dtype, kind)
    # ... and the one-output form of the fused pool
    got = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), wt, b, dilation=dilation, relu=True, dtype=dtype, pool=True).cpu().numpy()
    _grade('pool dil31 %s' % kind, got, cb.pool64(full), cb.pool64(S), K, dtype, kind)


# ----------------------------------------------------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=4)
def _bcase(kind, name, dtype, relu):
    shape = ce.BACKWARD[name]
    x, w, y, dy = cg.inputs(kind, shape)
    g = gref.grads64(*gref.seen(x, w, y, dy, dtype, relu), shape[6])
    if kind == 'lattice':
        cg.assert_lattice(w, g['dx'][0], g['dw'][0], g['db'][0])
    return (x, w, y, dy), g


def _backward(ops, dev, kind, name, dtype, relu, splitk=-1):
    (x, w, y, dy), g = _bcase(kind, name, dtype, relu)
    tx, tw, ty, tdy = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, w, y, dy)]
    outs = ops.conv2d_backward_nhwc(tx, tw, tdy, ty if relu else None, relu=bool(relu), dilation=ce.BACKWARD[name][6], dtype=dtype, splitk=splitk)
    got = {key: t.cpu().numpy() for key, t in zip(('dx', 'dw', 'db'), outs)}
    gref.check('%s %s relu=%d splitk=%d' % (name, kind, relu, splitk), got, g, dtype, kind)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('kind', cg.KINDS)
@pytest.mark.parametrize('dtype', cg.DTYPES)
@pytest.mark.parametrize('name', sorted(ce.BACKWARD))
def test_backward_at_dilation_31(ops, dev, name, dtype, kind, relu):
    _backward(ops, dev, kind, name, dtype, relu)


@pytest.mark.parametrize('kind', cg.KINDS)
@pytest.mark.parametrize('splitk', [-1, 2])
def test_backward_pixel_splits_at_dilation_31(ops, dev, splitk, kind):
    _backward(ops, dev, kind, 'dil31', 'bf16', 1, splitk=splitk)
