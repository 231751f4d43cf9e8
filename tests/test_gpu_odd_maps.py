"""GPU: the kernels on maps that are not even / not tile multiples (what SSD-300 brings: 300 -> 150 -> 75 -> 38 -> 19 ...).

  * the stand-alone SAME 2x2 pool on odd maps (ceil; the last window holds one row / column) in all four dtypes;
  * conv + fused SAME pool on odd maps in every row-gather tile configuration, with and without the un-pooled second output: bit-identical
    to the stand-alone pool of the same configuration's un-pooled output, and one exact-integer case in which a tile row that is no pixel
    of the map ("phantom": relu(bias + the taps that reach back into the map)) would win the max if it were computed as it stands;
  * the conv1_1 stem kernel at widths that are not a multiple of 32 (300: a 12-column last tile; 44), bf16 / fp16 / f16x3, per element
    against the float64 reference of tests/conv_bounds.py and exactly on the integer lattice; width 320 against recorded checksums of the
    kernels as they were before the ragged tile (tests/golden/g9_stem_320_crc.npz, recorded by tests/golden/make_stem320_crc.py)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_bounds as cb  # noqa: E402
import ssd300_ref  # noqa: E402
from oracle import ron_forward as orf  # noqa: E402

ROUND = {'fp32': lambda a: np.asarray(a, np.float32), 'bf16': orf.round_bf16, 'fp16': orf.round_f16, 'f16x3': orf.round_f16x3}
ALL4 = ['fp32', 'bf16', 'fp16', 'f16x3']
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_stem320_crc as stem320  # noqa: E402
# row-gather tile configurations (csrc/conv_mfma.h) with a fused-pool epilogue -> an output width each of them tiles;
# 10 = the four-wave 256 x 128 tile (bf16 / f16 / f16x3), 0 / 7 run on the four-wave 256 x 256 tile in those dtypes
POOL_CFGS = {-1: 256, 0: 256, 1: 256, 2: 256, 3: 64, 7: 256, 9: 256, 10: 128}
CFG_DTYPE = [(c, d) for c in sorted(POOL_CFGS) for d in ALL4 if not (c == 10 and d == 'fp32')]      # (fp32 has no four-wave 256 x 128 tile)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('hw', [(75, 75), (3, 5), (7, 2), (1, 1), (38, 38)], ids=lambda s: '%dx%d' % s)
def test_same_pool_on_odd_maps(ops, dev, hw, dtype):
    """Two different images, negative values included: a tap read from the halo (zero), the next row or the next image would show."""
    x = np.random.RandomState(hw[0] * 100 + hw[1]).randn(2, hw[0], hw[1], 32).astype(np.float32) - np.float32(1.5)
    x[1] += np.float32(3.0)
    got = ops.maxpool2x2_nhwc(torch.from_numpy(x).to(dev), dtype=dtype).cpu().numpy()
    want = ssd300_ref.max_pool2x2_same_np(ROUND[dtype](x))
    assert got.shape == want.shape == (2, (hw[0] + 1) // 2, (hw[1] + 1) // 2, 32)
    assert np.array_equal(got, want)


def _conv_case(shape, cout, seed):
    n, h, w, cin = shape
    rs = np.random.RandomState(seed)
    x = rs.randn(n, h, w, cin).astype(np.float32)
    wt = (rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = (rs.randn(cout) * 0.1).astype(np.float32) + np.float32(0.5)          # a bias that is not negligible: phantom rows are relu(bias + ...)
    return x, wt, b


@pytest.mark.parametrize('cfg,dtype', CFG_DTYPE)
@pytest.mark.parametrize('shape', [(2, 75, 75, 256), (2, 5, 7, 64)], ids=lambda s: 'x'.join(map(str, s)))
def test_fused_same_pool_on_odd_maps(ops, dev, shape, cfg, dtype):
    cout = POOL_CFGS[cfg]
    x, wt, b = _conv_case(shape, cout, 7 + cfg)
    xd = torch.from_numpy(x).to(dev)
    n, h, w, _ = shape
    got = ops.conv2d_nhwc(xd, wt, b, relu=True, dtype=dtype, tile_cfg=cfg, pool=True).cpu().numpy()
    assert got.shape == (n, (h + 1) // 2, (w + 1) // 2, cout)
    # with the un-pooled map as the launch's second output: the pooled map is the SAME pool of that map, bit for bit (phantom rows
    # are not stored and do not enter the max)
    yp, yf = ops.conv2d_pool2_nhwc(xd, wt, b, relu=True, dtype=dtype, tile_cfg=cfg)
    assert tuple(yf.shape) == (n, h, w, cout)
    assert np.array_equal(yp.cpu().numpy(), ssd300_ref.max_pool2x2_same_np(yf.cpu().numpy()))        # (values already in the storage type)
    assert np.array_equal(yp.cpu().numpy(), ops.maxpool2x2_nhwc(yf, dtype=dtype).cpu().numpy())
    if cfg >= 0:
        # a forced tile configuration adds its products in one order whatever the epilogue: the three launches agree bit for bit
        # (left to itself the library may pick another configuration for a launch that cannot split K)
        full = ops.conv2d_nhwc(xd, wt, b, relu=True, dtype=dtype, tile_cfg=cfg, splitk=1)
        want = ops.maxpool2x2_nhwc(full, dtype=dtype).cpu().numpy()
        assert np.array_equal(got, want), 'fused SAME pool differs from the pool of the un-pooled output'
        assert torch.equal(yf, full), 'second (un-pooled) output differs from the plain convolution'
        assert np.array_equal(yp.cpu().numpy(), want)
    # against the float64 reference too, per element (SAME pool of reference and magnitudes: monotone, 1-Lipschitz)
    rnd = ROUND[dtype]
    ref, S, K = cb.conv_op(rnd(x), rnd(wt), b)
    pool = ssd300_ref.max_pool2x2_same_np
    top, at = cb.worst(cb.ratio(got, pool(ref), pool(S), K, dtype))
    print('RATIO fused SAME pool %s cfg %d %s: largest error / bound %.3f' % ('x'.join(map(str, shape)), cfg, dtype, top))
    assert top <= 1.0, (top, at)


def _phantom_case(n, h, w, cin, cout):
    """Integer lattice on which a phantom row wins if it is included: activations in [0, 2], weights in {-1, 0} (<= 64 non-zeros per
    output channel), bias +200.  A pixel of the map is 200 - (sum over the taps inside the map) in [72, 200]; a row below / right of
    an odd map computed as it stands sees at most three of the nine taps, so it is LARGER than its window's real pixels."""
    x = cb.lattice_acts((n, h, w, cin), seed=11, lo=0, hi=2)
    wt = -np.abs(cb.lattice_weights(3, 3, cin, cout, seed=11))
    b = np.full((cout,), 200.0, np.float32)
    return x, wt, b


@pytest.mark.parametrize('cfg,dtype', CFG_DTYPE)
def test_phantom_rows_never_win_the_max(ops, dev, cfg, dtype):
    cout = POOL_CFGS[cfg]
    x, wt, b = _phantom_case(2, 5, 7, 64, cout)
    full = np.maximum(cb.conv64(x, wt) + b, 0)
    assert 0 < full.min() and full.max() <= 200 and np.array_equal(full, np.round(full))
    want = ssd300_ref.max_pool2x2_same_np(full.astype(np.float32))
    # the mutant: the map continued by one row / column of "relu(bias + taps over the zero halo)", pooled VALID
    xp = np.pad(x, ((0, 0), (0, 1), (0, 1), (0, 0)))
    ext = np.maximum(cb.conv64(xp, wt) + b, 0)
    mutant = ext.reshape(2, 3, 2, 4, 2, cout).max(axis=(2, 4))
    assert (mutant[:, -1] > want[:, -1]).any() and (mutant[:, :, -1] > want[:, :, -1]).any(), 'the case must be able to show a phantom row'
    xd = torch.from_numpy(x).to(dev)
    got = ops.conv2d_nhwc(xd, wt, b, relu=True, dtype=dtype, tile_cfg=cfg, pool=True).cpu().numpy()
    assert np.array_equal(got, want)
    yp, yf = ops.conv2d_pool2_nhwc(xd, wt, b, relu=True, dtype=dtype, tile_cfg=cfg)
    assert np.array_equal(yp.cpu().numpy(), want) and np.array_equal(yf.cpu().numpy(), full.astype(np.float32))


# --------------------------------------------------------------------------------------------------------------------- #
# conv1_1 stem kernel with a ragged last tile
# --------------------------------------------------------------------------------------------------------------------- #
def _stem_inputs(kind, n, h, w, seed=7):
    if kind == 'lattice':
        x = cb.lattice_acts((n, h, w, 3), seed=seed, lo=-3, hi=3)
        wt = cb.lattice_weights(3, 3, 3, 64, seed=seed)
        b = cb.lattice_bias(64, seed=seed, nonzero=True)
    else:
        rs = np.random.RandomState(seed)
        x = (rs.uniform(0, 255, (n, h, w, 3)) - np.array([123., 117., 104.])).astype(np.float32)
        wt = (rs.randn(3, 3, 3, 64) * np.sqrt(2.0 / 27)).astype(np.float32)
        b = (rs.randn(64) * 0.1).astype(np.float32)
    return x, wt, b


@pytest.mark.parametrize('kind', ['lattice', 'gauss'])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16', 'f16x3'])
@pytest.mark.parametrize('hw', [(6, 300), (5, 44), (3, 12), (4, 33)], ids=lambda s: '%dx%d' % s)
def test_stem_ragged_width(ops, dev, hw, dtype, kind):
    """Widths 300 (9 full tiles + 12 columns), 44, 12 (one ragged tile) and 33 (one column in the last tile), two images: every
    element against the float64 reference - exactly on the lattice, under the derived bound otherwise.  A store past the row's end
    would land in the next row's pixels / the next image (both are checked: the whole tensor is compared)."""
    x, wt, b = _stem_inputs(kind, 2, hw[0], hw[1])
    rnd = ROUND[dtype]
    ref, S, K = cb.conv_op(rnd(x), rnd(wt), b)
    got = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), wt, b, relu=True, dtype=dtype).cpu().numpy()
    assert got.shape == ref.shape
    if kind == 'lattice':
        assert np.array_equal(got, ref)
        return
    top, at = cb.worst(cb.ratio(got, ref, S, K, dtype))
    print('RATIO stem %dx%d %s: largest error / bound %.3f at %s' % (hw[0], hw[1], dtype, top, at))
    assert top <= 1.0, (top, at)
    # the implicit-GEMM path (im2col + a K = 32 GEMM, what fp32 runs) on the same problem, under the same bound
    same = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), wt, b, relu=True, dtype=dtype, tile_cfg=3).cpu().numpy()
    assert cb.ratio(same, ref, S, K, dtype).max() <= 1.0


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_stem_ragged_tile_computes_what_a_full_tile_computes(ops, dev, dtype):
    """A 44-wide image is the first 44 columns of a 64-wide one: columns 0 .. 42 see the same 3 x 3 neighbourhoods, so the ragged tile
    (columns 32 .. 43) must give the bits the full tile gives.  (f16x3: at widths that are a multiple of 32 the single-operator entry
    runs im2col + GEMM; the network test compares its stem kernel at 300 with G9.)"""
    x, wt, b = _stem_inputs('gauss', 2, 6, 64, seed=9)
    wide = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), wt, b, relu=True, dtype=dtype).cpu().numpy()
    narrow = ops.conv2d_nhwc(torch.from_numpy(np.ascontiguousarray(x[:, :, :44])).to(dev), wt, b, relu=True, dtype=dtype).cpu().numpy()
    assert np.array_equal(narrow[:, :, :43], wide[:, :, :43])


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_stem_width_320_is_what_it_was(ops, dev, dtype):
    """Width 320 (full tiles only): the output's checksum recorded from the kernel before it learnt the ragged tile."""
    g = np.load(os.path.join(HERE, 'golden', 'g9_stem_320_crc.npz'))
    assert int(g['seed']) == stem320.SEED
    x, wt, b = stem320.op_inputs()
    got = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), wt, b, relu=True, dtype=dtype).cpu().numpy()
    assert got.shape == (2, 8, 320, 64)
    assert int(stem320.crc(got)) == int(g[dtype]), 'the stem kernel at width 320 no longer computes what it did'


def test_split_precision_stem_width_320_is_what_it_was(dev):
    """The f16x3 stem kernel (stem_conv_split_kernel) runs at this width inside the graph only: conv1_1 of a RON-320 context."""
    g = np.load(os.path.join(HERE, 'golden', 'g9_stem_320_crc.npz'))
    a = stem320.context_conv1_1('f16x3')
    assert a.shape == (1, 320, 320, 64) and float(np.abs(a).max()) > 0
    assert int(stem320.crc(a)) == int(g['f16x3_conv1_1']), 'the split-precision stem kernel at width 320 no longer computes what it did'
