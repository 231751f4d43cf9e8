"""GPU: the 256 x 224 form of the four-wave 256 x 256 conv tile (convolutions of 193 .. 224 output channels: the class heads).

The narrower tile changes which columns a workgroup computes, not the order in which an output element accumulates its K steps, so
every output must be BIT-IDENTICAL to the same launch on the 256-column tile (RON_IGEMM224=0, read by the library per call), and
inside the per-element bound of tests/conv_bounds.py.  Shapes: the smallest at which the tile can go wrong - one exact tile, a row
tail, two K chunks per tap with split-K slabs, a member of a grouped launch, full and partial channel vectors of the last lanes
(a lane owns seven adjacent channels: 210 = 30 x 7 has none partial, 193 and 222 have) - with the head layers' fp32 output and
with the storage-type output."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_bounds as cb  # noqa: E402
from oracle import ron_forward as orf  # noqa: E402

ROUND = {'bf16': orf.round_bf16, 'fp16': orf.round_f16}
CFG256 = 0          # kCfgIgemm256: forced, these maps are far too small for the picker to choose it


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


def _operands(n, h, w, cin, cout, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, h, w, cin).astype(np.float32)
    wt = (rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = (rs.randn(cout) * 0.1).astype(np.float32)
    return x, wt, b


def _both_widths(monkeypatch, run):
    """run() on the 224-column form and on the 256-column tile."""
    monkeypatch.delenv('RON_IGEMM224', raising=False)
    new = run()
    monkeypatch.setenv('RON_IGEMM224', '0')
    old = run()
    monkeypatch.delenv('RON_IGEMM224', raising=False)
    return new, old


def _in_bound(got, dtype, x, wt, b, relu, out_dtype):
    rnd = ROUND[dtype]
    ref, S, K = cb.conv_op(rnd(x), rnd(wt), b, relu=relu)
    top, at = cb.worst(cb.ratio(got, ref, S, K, dtype, out_dtype))
    print('%s K=%d cout=%d: largest error / bound %.3f at %s' % (dtype, K, wt.shape[3], top, at))
    assert top <= 1.0, 'error / bound = %.3f at %s' % (top, at)


# n, h, w, cin, cout, splitk
CASES = {
    'exact_tile_210': (1, 16, 16, 64, 210, 1),          # M = 256: one tile, 9 K steps, no partial channel vector
    'cout_224': (1, 16, 16, 64, 224, 1),                # every lane of the tile stores
    'cout_193': (1, 16, 16, 64, 193, 1),                # lower edge of the range: the last storing lane holds 4 of 7 channels
    'cout_222': (1, 16, 16, 64, 222, 1),                # the last lane holds 5 of 7
    'row_tail': (3, 10, 10, 64, 210, 1),                # M = 300: the second tile has 44 rows, the rest carry offset -1
    'two_chunks_splitk2': (3, 10, 10, 128, 210, 2),     # two K chunks per tap; slabs and the finalize pass see 224-wide tiles
}


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_224_form_is_the_256_tile_bit_for_bit(ops, dev, monkeypatch, case, dtype):
    n, h, w, cin, cout, sk = CASES[case]
    x, wt, b = _operands(n, h, w, cin, cout, seed=len(case) + cout)
    xd = torch.from_numpy(x).to(dev)
    plan = _both_widths(monkeypatch, lambda: ops.conv_plan_n_tile(n, h, w, cin, cout, dtype=dtype, tile_cfg=CFG256, splitk=sk))
    assert plan == (224, 256), plan
    # fp32 output written by the epilogue (the head layers), no ReLU
    head = lambda: ops.conv2d_f32out_nhwc([dict(x=xd, w=wt, bias=b, tile_cfg=CFG256, splitk=sk)], dtype=dtype)[0].cpu().numpy()
    new, old = _both_widths(monkeypatch, head)
    assert new.shape == (n, h, w, cout)
    assert np.array_equal(new, old), '%d of %d fp32 outputs differ from the 256-column tile' % ((new != old).sum(), new.size)
    _in_bound(new, dtype, x, wt, b, relu=False, out_dtype='fp32')
    # storage-type output with ReLU
    body = lambda: ops.conv2d_nhwc(xd, wt, b, relu=True, dtype=dtype, tile_cfg=CFG256, splitk=sk).cpu().numpy()
    new, old = _both_widths(monkeypatch, body)
    assert np.array_equal(new, old), '%d of %d outputs differ from the 256-column tile' % ((new != old).sum(), new.size)
    _in_bound(new, dtype, x, wt, b, relu=True, out_dtype=None)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_residual_epilogue_on_224_columns(ops, dev, monkeypatch, dtype):
    """relu(relu(conv + b) + residual): the row loop that loads a lane's seven residual values as one vector."""
    x, wt, b = _operands(1, 16, 16, 64, 210, seed=3)
    res = np.maximum(np.random.RandomState(4).randn(1, 16, 16, 210), 0).astype(np.float32)
    xd, rd = torch.from_numpy(x).to(dev), torch.from_numpy(res).to(dev)
    run = lambda: ops.conv2d_nhwc(xd, wt, b, residual=rd, relu=True, dtype=dtype, tile_cfg=CFG256, splitk=1).cpu().numpy()
    new, old = _both_widths(monkeypatch, run)
    assert np.array_equal(new, old)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16', 'f16x3', 'fp32'])
def test_which_launches_take_the_224_form(ops, monkeypatch, dtype):
    """The plan, without a launch: 193 .. 224 output channels of bf16 / f16 on the four-wave 256 x 256 configuration, nothing else."""
    monkeypatch.delenv('RON_IGEMM224', raising=False)
    half = dtype in ('bf16', 'fp16')
    cin = 64 if half else 32
    for cout, want in ((192, 256), (193, 224), (210, 224), (224, 224), (225, 256)):
        got = ops.conv_plan_n_tile(1, 16, 16, cin, cout, dtype=dtype, tile_cfg=CFG256, splitk=1)
        assert got == (want if half else 256), (cout, got)
    if not half:
        return
    # picked by shape: 150 tiles of 256 rows run the 256 x 256 configuration (taps innermost) without split-K -> 224 columns
    p = ops.conv_plan(24, 40, 40, 64, 210, dtype=dtype)
    assert (p['tile_cfg'], p['splitk']) == (7, 1), p
    assert ops.conv_plan_n_tile(24, 40, 40, 64, 210, dtype=dtype) == 224
    # ... 100 tiles with a long K split it themselves: such launches keep the 256 columns they were measured with
    p = ops.conv_plan(16, 40, 40, 1024, 210, dtype=dtype)
    assert p['tile_cfg'] == 0 and p['splitk'] > 1, p
    assert ops.conv_plan_n_tile(16, 40, 40, 1024, 210, dtype=dtype) == 256
    # other tile configurations are not touched
    assert ops.conv_plan_n_tile(1, 16, 16, 64, 210, dtype=dtype, tile_cfg=2, splitk=1) == 128


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_member_of_a_256_group(ops, dev, monkeypatch, dtype):
    """One grouped launch of 256 x 256 tiles with a 256-column member and a 210-column member (10 x 10, n = 3: a row tail in both):
    each member bit-identical to its launch alone, and to the group with every member on 256 columns."""
    xa, wa, ba = _operands(3, 10, 10, 64, 256, seed=11)
    xb, wb, bb = _operands(3, 10, 10, 64, 210, seed=12)
    xad, xbd = torch.from_numpy(xa).to(dev), torch.from_numpy(xb).to(dev)
    convs = [dict(x=xad, w=wa, bias=ba, tile_cfg=CFG256, splitk=1), dict(x=xbd, w=wb, bias=bb, tile_cfg=CFG256, splitk=1)]
    tiles = []

    def group():
        ys, t = ops.conv2d_f32out_nhwc(convs, grouped=True, dtype=dtype, with_tiles=True)
        tiles.append(t)
        return [y.cpu().numpy() for y in ys]
    new, old = _both_widths(monkeypatch, group)
    # the launch itself says which tile each member ran on: the 210-column member on 224 columns, and on 256 when switched off
    assert tiles == [[256, 224], [256, 256]], tiles
    ys, t = ops.conv2d_f32out_nhwc(convs, grouped=False, dtype=dtype, with_tiles=True)
    assert t == [256, 224], t
    alone = [y.cpu().numpy() for y in ys]
    for k in range(2):
        assert np.array_equal(new[k], alone[k]), 'member %d differs from its own launch' % k
        assert np.array_equal(new[k], old[k]), 'member %d differs from the 256-column group' % k
    _in_bound(new[0], dtype, xa, wa, ba, relu=False, out_dtype='fp32')
    _in_bound(new[1], dtype, xb, wb, bb, relu=False, out_dtype='fp32')
