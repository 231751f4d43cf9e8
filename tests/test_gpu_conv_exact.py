"""GPU parity per element: every conv kernel family against the float64 reference of tests/conv_bounds.py, twice -

  kind 'lattice'  inputs on an integer lattice (activations in [-2, 2], weights in {-1, 0, 1} with <= 64 non-zeros per output channel,
                  integer bias / residual): every product and partial sum is exact in any accumulation order, so the result must
                  EQUAL the reference (np.array_equal) in fp32, bf16, fp16 and f16x3 alike;
  kind 'gauss'    the Gaussian inputs of tests/test_gpu_conv.py, graded per element by the derived bound (ratio <= 1): what catches
                  rounding-mode, scaling and bias errors that integers cannot show.

Each case prints its largest ratio (pytest -s; the table of DESIGN.md "Parity per element")."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_bounds as cb  # noqa: E402
from test_gpu_conv import C64_SHAPES, CONV_SHAPES, HALO_SHAPES, IGEMM_CFGS, PATCH_SHAPES, ROUND, _patch_cfg  # noqa: E402

ALL4 = ['fp32', 'bf16', 'fp16', 'f16x3']
KINDS = ['lattice', 'gauss']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


def _sid(s):
    return 'x'.join(map(str, s))


def _grade(tag, got, ref, S, K, dtype, kind, out_dtype=None, extra=0.0):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if kind == 'lattice':
        assert np.abs(ref).max() < 256 and np.abs(ref).max() > 0
        bad = np.argwhere(got != ref)
        assert bad.size == 0, '%s %s: %d elements differ from the exact result, first at %s: got %r, exact %r' % (
            tag, dtype, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])
        return 0.0
    r = cb.ratio(got, ref, S, K, dtype, out_dtype, extra)
    top, at = cb.worst(r)
    print('RATIO %s %s K=%d: largest error / bound %.3f at %s (got %r, float64 %r)' % (tag, dtype, K, top, at, float(got[at]), float(ref[at])))
    assert top <= 1.0, '%s %s: error / bound = %.3f at %s: got %r, float64 %r' % (tag, dtype, top, at, float(got[at]), float(ref[at]))
    return top


@functools.lru_cache(maxsize=2)
def _case(kind, dtype, n, h, w, cin, cout, k, seed, draw, residual, transpose, center_from, pool, stride, bias, rate, relu):
    """Inputs + float64 reference of one case, kept across the tile configurations / split-K factors that share it."""
    given, (xs, ws, bs, rs_) = _inputs(kind, dtype, n, h, w, cin, cout, k, seed, draw, residual, transpose, center_from, pool, stride, bias)
    return given, cb.conv_op(xs, ws, bs, rs_, stride=2 if transpose else stride, rate=rate, relu=relu, pool=pool, transpose=transpose)


def _inputs(kind, dtype, n, h, w, cin, cout, k, seed, draw=0, residual=False, transpose=False, center_from=0, pool=False, stride=1,
            bias=True):
    """(x, weights, bias, residual) as float32 arrays the entry points take, and the same as the kernel sees them (rounded)."""
    rnd = ROUND[dtype]
    ho, wo = (h * 2, w * 2) if transpose else (h // stride, w // stride)
    if kind == 'lattice':
        x = cb.lattice_acts((n, h, w, cin), seed)
        if transpose:
            wt = cb.lattice_deconv_weights(cin, cout, seed=seed)
        elif center_from:
            wt = cb.lattice_centre_weights(cin, cout, center_from, seed=seed)
        else:
            wt = cb.lattice_weights(k, k, cin, cout, draw=draw, seed=seed)
        b = cb.lattice_bias(cout, seed) if bias else None
        res = cb.lattice_residual((n, ho, wo, cout), seed) if residual else None
    else:
        rs = np.random.RandomState(seed)
        x = rs.randn(n, h, w, cin).astype(np.float32)
        if transpose:
            wt = (rs.randn(2, 2, cout, cin) * np.sqrt(2.0 / cin)).astype(np.float32)
        else:
            wt = (rs.randn(k, k, cin, cout) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
            if center_from:
                centre = wt[1, 1, :, center_from:].copy()
                wt[:, :, :, center_from:] = 0
                wt[1, 1, :, center_from:] = centre * 3
        b = (rs.randn(cout) * 0.1).astype(np.float32) if bias else None
        res = np.maximum(rs.randn(n, ho, wo, cout), 0).astype(np.float32) if residual else None
    seen = (rnd(x), rnd(wt), b, None if res is None else rnd(res))
    return (x, wt, b, res), seen


def _run(ops, dev, kind, dtype, tag, n, h, w, cin, cout, k=3, stride=1, rate=1, relu=True, residual=False, pool=False, transpose=False,
         tile_cfg=-1, splitk=-1, center_from=0, in_cstride=0, in_coff=0, seed=0, bias=True):
    """One convolution through ron_conv2d_nhwc, graded.  On the lattice: as many shifted weight draws as it takes to give every
    (tap, input channel) index a non-zero weight in some output channel - asserted before the GPU is touched."""
    draws = 1
    if kind == 'lattice' and not transpose and not center_from:
        draws = cb.lattice_draws(k, k, cin, cout)
        cb.assert_lattice([cb.lattice_weights(k, k, cin, cout, draw=d, seed=seed) for d in range(draws)])
    elif kind == 'lattice' and transpose:            # each of the four taps is a 1x1 convolution of its own
        wd = cb.lattice_deconv_weights(cin, cout, seed=seed)
        for t in range(4):
            cb.assert_lattice([wd[t // 2, t % 2].T[None, None]])
    elif kind == 'lattice':                          # 3x3 columns cover all nine taps, the centre-tap-only columns their one tap
        wc = cb.lattice_centre_weights(cin, cout, center_from, seed=seed)
        centre = np.zeros((3, 3, cin), bool)
        centre[1, 1] = True
        cb.assert_lattice([wc[..., :center_from]])
        cb.assert_lattice([wc[..., center_from:]], covered=centre)
        assert not wc[..., center_from:][~centre].any()
    top = 0.0
    for draw in range(draws):
        (x, wt, b, res), (ref, S, K) = _case(kind, dtype, n, h, w, cin, cout, k, seed, draw, residual, transpose, center_from, pool, stride,
                                             bias, rate, relu)
        if kind == 'lattice':
            assert S.max() <= 2 * 64 + 8 + 8
        # in_cstride / in_coff: the entry packs x into channels [in_coff, in_coff + cin) of a tensor in_cstride channels wide
        got = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), wt, b, residual=None if res is None else torch.from_numpy(res).to(dev),
                              stride=2 if transpose else stride, dilation=rate, relu=relu, transpose=transpose, dtype=dtype, tile_cfg=tile_cfg,
                              splitk=splitk, pool=pool, in_cstride=in_cstride, in_coff=in_coff, center_from=center_from).cpu().numpy()
        top = max(top, _grade(tag, got, ref, S, K, dtype, kind))
    return top


# --------------------------------------------------------------------------------------------------------------------- #
# the shape lists of tests/test_gpu_conv.py
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=_sid)
def test_conv_shapes(ops, dev, shape, dtype, kind):
    n, h, w, cin, cout, k, stride, rate = shape
    _run(ops, dev, kind, dtype, 'conv ' + _sid(shape), n, h, w, cin, cout, k, stride, rate, seed=sum(shape))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('cfg', IGEMM_CFGS)
def test_every_row_gather_tile(ops, dev, cfg, dtype, kind):
    """Ragged multi-tile problem (M = 429, Cout 192 -> padded), K = 18 steps, then K of one and two steps without bias / ReLU."""
    _run(ops, dev, kind, dtype, 'igemm cfg %d' % cfg, 3, 13, 11, 128, 192, tile_cfg=cfg, seed=40 + cfg)
    for cin in (64, 128):
        _run(ops, dev, kind, dtype, 'igemm cfg %d 1x1 cin %d' % (cfg, cin), 2, 9, 9, cin, 256, k=1, relu=False, bias=False, tile_cfg=cfg, seed=cin)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('shape', PATCH_SHAPES, ids=_sid)
def test_patch_kernel(ops, dev, shape, dtype, kind):
    n, h, w, cin, cout = shape
    _run(ops, dev, kind, dtype, 'patch ' + _sid(shape), n, h, w, cin, cout, tile_cfg=_patch_cfg(cout), seed=sum(shape))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
def test_patch_kernel_slice_residual_pool(ops, dev, dtype, kind):
    _run(ops, dev, kind, dtype, 'patch cfg 5 residual', 2, 40, 40, 128, 128, residual=True, tile_cfg=5, seed=91)
    _run(ops, dev, kind, dtype, 'patch cfg 5 residual, slice 64..192 of 320', 2, 40, 40, 128, 128, residual=True, tile_cfg=5, in_cstride=320,
         in_coff=64, seed=92)
    for (h, w) in ((16, 64), (32, 32), (8, 96)):
        _run(ops, dev, kind, dtype, 'patch cfg 5 pool %dx%d' % (h, w), 2, h, w, 64, 128, pool=True, tile_cfg=5, seed=h)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('shape', C64_SHAPES, ids=_sid)
def test_resident_weight_kernel(ops, dev, shape, dtype, kind):
    n, h, w, cout = shape
    _run(ops, dev, kind, dtype, 'c64 ' + _sid(shape), n, h, w, 64, cout, tile_cfg=8, seed=sum(shape))
    if n <= 3:
        _run(ops, dev, kind, dtype, 'c64 plain ' + _sid(shape), n, h, w, 64, cout, tile_cfg=8, relu=False, bias=False, seed=sum(shape) + 1)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ['bf16', 'fp16', 'f16x3'])
def test_tile_256x128(ops, dev, dtype, kind):
    """Tile configuration 10 (the assembly K loop): ragged M, Cout below the tile width, K of 18 / 1 / 2 / 5 steps with a residual,
    split-K, the fused pool."""
    _run(ops, dev, kind, dtype, 'cfg 10', 3, 13, 11, 128, 100, tile_cfg=10, seed=90)
    chunk = 32 if dtype == 'f16x3' else 64
    for steps in (1, 2, 5):
        _run(ops, dev, kind, dtype, 'cfg 10 1x1 %d steps residual' % steps, 2, 9, 15, chunk * steps, 128, k=1, relu=False, bias=False,
             residual=True, tile_cfg=10, seed=steps)
    for sk in (1, 2, 3, 5, -1):
        _run(ops, dev, kind, dtype, 'cfg 10 splitk %d' % sk, 3, 13, 11, 128, 200, tile_cfg=10, splitk=sk, seed=92)
    _run(ops, dev, kind, dtype, 'cfg 10 pool', 2, 32, 48, 128, 128, tile_cfg=10, pool=True, seed=93)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('shape', HALO_SHAPES, ids=_sid)
def test_halo_shapes(ops, dev, shape, dtype, kind):
    """Position-major rows with skipped halo filter rows: chosen and forced tiles, every split-K factor, a residual."""
    n, h, w, cin, cout, k, rate = shape
    for cfg in ((-1, 0, 1) if cout % 256 == 0 else (-1, 1)):
        for sk in (1, 2, 5, -1):
            _run(ops, dev, kind, dtype, 'halo %s cfg %d splitk %d' % (_sid(shape), cfg, sk), n, h, w, cin, cout, k, 1, rate, tile_cfg=cfg,
                 splitk=sk, seed=sum(shape))
    for sk in (1, 3):
        _run(ops, dev, kind, dtype, 'halo %s residual splitk %d' % (_sid(shape), sk), n, h, w, cin, cout, k, 1, rate, residual=True, splitk=sk,
             seed=sum(shape) + 1)


# --------------------------------------------------------------------------------------------------------------------- #
# split-K, fused pool, residual, transposed conv, centre-tap-only columns
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('splitk', [1, 2, 3, 7, -1])
def test_split_k(ops, dev, splitk, dtype, kind):
    for cout, relu, with_res in ((20, False, False), (128, True, True), (210, False, False)):
        _run(ops, dev, kind, dtype, 'splitk %d cout %d' % (splitk, cout), 2, 5, 5, 256, cout, relu=relu, residual=with_res, splitk=splitk, seed=60 + cout)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('cfg', [-1, 0, 1, 3, 7, 9])
def test_fused_maxpool(ops, dev, cfg, dtype, kind):
    _run(ops, dev, kind, dtype, 'pool cfg %d' % cfg, 3, 12, 20, 64, 64 if cfg == 3 else 256, tile_cfg=cfg, pool=True, seed=70)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
def test_residual_epilogue_and_plain(ops, dev, dtype, kind):
    _run(ops, dev, kind, dtype, 'no bias no relu', 2, 10, 10, 128, 128, relu=False, bias=False, seed=5)
    _run(ops, dev, kind, dtype, 'residual', 2, 10, 10, 128, 128, residual=True, seed=6)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('residual', [False, True], ids=['plain', 'residual'])
def test_transposed_2x2(ops, dev, residual, dtype, kind):
    _run(ops, dev, kind, dtype, 'deconv' + (' residual' if residual else ''), 3, 5, 5, 128, 128, k=2, transpose=True, residual=residual, seed=41)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('cfg', [0, 7, 2, 9])
def test_centre_tap_only_columns(ops, dev, cfg, dtype, kind):
    _run(ops, dev, kind, dtype, 'center_from cfg %d' % cfg, 5, 20, 20, 128, 512, tile_cfg=cfg, splitk=1, center_from=256, seed=70 + cfg)


# --------------------------------------------------------------------------------------------------------------------- #
# two head tensors from one convolution (fp32 outputs: u = 0)
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('kind', KINDS + ['gauss_scaled'])
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('heads', [(84, 16), (486, 24), (21, 4), (126, 24)], ids=lambda h: '%d+%d' % h)
def test_two_head_outputs(ops, dev, heads, dtype, kind):
    """'gauss_scaled': the second head's weights and bias are 1/64 of the first's - each head is graded against its own elements,
    not against the maximum of a tensor."""
    from ron_tensorflow_amd._lib import RonError
    n_cls, n_loc = heads
    cin, cout = 128, n_cls + n_loc
    (x, wt, b, _), (xs, ws, bs, _) = _inputs('lattice' if kind == 'lattice' else 'gauss', dtype, 2, 8, 8, cin, cout, 3, seed=n_cls)
    if kind == 'lattice':
        cb.assert_lattice([wt])
    if kind == 'gauss_scaled':
        wt[..., n_cls:] /= 64
        b[n_cls:] /= 64
        ws, bs = ROUND[dtype](wt), b
    ref, S, K = cb.conv_op(xs, ws, bs, relu=False)
    packed = -(-n_cls // 8) * 8 + n_loc
    npad = -(-packed // (64 if packed <= 64 else 128)) * (64 if packed <= 64 else 128)
    ran = 0
    for cfg in (-1, 1, 0, 10):
        if cfg == 10 and dtype == 'fp32':
            continue                                     # the 256 x 128 tile is the assembly loop of the 16-bit types
        for splitk in (1, 3, -1):
            try:
                y1, y2 = ops.conv2d_heads_nhwc(torch.from_numpy(x).to(dev), wt, n_cls, bias=b, dtype=dtype, tile_cfg=cfg, splitk=splitk)
            except RonError:
                assert (cfg == 0 and npad % 256 != 0) or (cfg in (1, 10) and npad % 128 != 0)
                continue
            ran += 1
            tag = 'heads %d+%d cfg %d splitk %d %s' % (n_cls, n_loc, cfg, splitk, kind)
            _grade(tag + ' first', y1.cpu().numpy(), ref[..., :n_cls], S[..., :n_cls], K, dtype, kind.split('_')[0], out_dtype='fp32')
            _grade(tag + ' second', y2.cpu().numpy(), ref[..., n_cls:], S[..., n_cls:], K, dtype, kind.split('_')[0], out_dtype='fp32')
    assert ran >= 3


# --------------------------------------------------------------------------------------------------------------------- #
# the 3-channel stem: stem_conv_kernel (width % 32 == 0) and the im2col path
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', ALL4)
@pytest.mark.parametrize('hw', [(16, 20), (12, 64), (7, 96)], ids=_sid)
def test_stem_3_channels(ops, dev, hw, dtype, kind):
    rnd = ROUND[dtype]
    if kind == 'lattice':
        x = cb.lattice_acts((2, hw[0], hw[1], 3), seed=7, lo=-3, hi=3)
        wt = cb.lattice_weights(3, 3, 3, 64, seed=7)
        cb.assert_lattice([wt])
        b = cb.lattice_bias(64, seed=7, nonzero=True)
        assert (b != 0).all()
    else:
        rs = np.random.RandomState(7)
        x = (rs.uniform(0, 255, (2, hw[0], hw[1], 3)) - np.array([123., 117., 104.])).astype(np.float32)
        wt = (rs.randn(3, 3, 3, 64) * np.sqrt(2.0 / 27)).astype(np.float32)
        b = (rs.randn(64) * 0.1).astype(np.float32)
    ref, S, K = cb.conv_op(rnd(x), rnd(wt), b)
    got = ops.conv2d_nhwc(torch.from_numpy(x).to(dev), wt, b, relu=True, dtype=dtype).cpu().numpy()
    _grade('stem %dx%d' % hw, got, ref, S, K, dtype, kind)


# --------------------------------------------------------------------------------------------------------------------- #
# stem2_kernel: image -> conv1_1 -> conv1_2 -> pool1 in one kernel, through the network context
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope='module')
def weights_reduced():
    from ron_tensorflow_amd.weights import synthetic_weights
    return synthetic_weights('reducedfc', seed=1)


@pytest.mark.parametrize('kind', ['lattice', 'gauss', 'gauss_low_contrast'])
@pytest.mark.parametrize('no_stem2', [False, True], ids=['stem2', 'separate'])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_two_layer_stem_to_pool1(dev, weights_reduced, dtype, n, no_stem2, kind):
    """pool1 of a RONNet(reducedfc, fuse_pools=True) against the float64 conv -> conv -> pool of the same conv1_1 / conv1_2 weights:
    bit-exact on the lattice (non-zero conv1_1 bias: a halo position computed as relu(bias) instead of zero would show at every border
    pixel), inside the two-layer bound on synthetic images and on a low-contrast image (where that halo matters most)."""
    from ron_tensorflow_amd.nets import nets_factory
    from ron_tensorflow_amd.weights import synthetic_images
    rnd = ROUND[dtype]
    weights = dict(weights_reduced)
    s = 'ron_320_vgg/conv1/'
    if kind == 'lattice':
        w1, b1, w2, b2 = cb.stem2_lattice()
        cb.assert_lattice([w1], nnz=2)
        cb.assert_lattice([w2], nnz=24)
        weights.update({s + 'conv1_1/weights': w1, s + 'conv1_1/biases': b1, s + 'conv1_2/weights': w2, s + 'conv1_2/biases': b2})
        img = cb.lattice_acts((n, 320, 320, 3), seed=n, lo=-3, hi=3)
    else:
        w1, b1, w2, b2 = (np.array(weights[s + k], np.float32) for k in ('conv1_1/weights', 'conv1_1/biases', 'conv1_2/weights', 'conv1_2/biases'))
        img = synthetic_images(n, seed=12)
        if kind == 'gauss_low_contrast':
            img = (np.random.RandomState(3).randn(n, 320, 320, 3) * 2).astype(np.float32)
            b1 = (np.abs(b1) * 50 + 0.02).astype(np.float32)            # conv1_1 weights carry the 1/64 input scale: outputs of ~0.05
            weights[s + 'conv1_1/biases'] = b1
    ref, S, K, extra = cb.stem2_op(rnd(img), rnd(w1), b1, rnd(w2), b2, dtype)
    if kind == 'lattice':
        a1 = cb.conv_op(img, w1, b1)[0]
        assert a1.min() >= 0 and a1.max() <= 8 and S.max() <= 24 * 8 + 8
    cls = nets_factory.get_network('ron_320_vgg')
    net = cls(variant='reducedfc', dtype=dtype, max_batch=n, device=dev, fuse_pools=True)
    net.no_stem2 = no_stem2
    net.load_weights(weights)
    try:
        assert ('conv1_1+conv1_2+pool1' in net.launch_plan()) == (not no_stem2), net.launch_plan()[:4]
        net.forward_heads(torch.from_numpy(img).to(dev))
        got = net.end_point('pool1', n).cpu().numpy()
    finally:
        net.close()
    _grade('stem2 n=%d %s %s' % (n, 'separate' if no_stem2 else 'fused', kind), got, ref, S, K, dtype, kind.split('_')[0], extra=extra)
