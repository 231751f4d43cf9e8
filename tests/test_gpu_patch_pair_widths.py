"""GPU: the skinny-head pair of the halo-patch kernel at the widths its members need (32 + 48 computed columns instead of 64 + 64).

Two 3x3 convolutions over channel slices of one tensor, one launch of conv3x3_patch_pair_kernel.  The weights are staged 64 rows per
tap as before; a member of up to 32 output channels multiplies one column block per wave (4 x 2 waves), one of up to 48 three blocks
per wave (8 x 1 waves).  Which columns a wave multiplies changes, the K order of an output element does not: every output must be
bit-identical to the 64 + 64 form of the same launch and inside the per-element bound of tests/conv_bounds.py."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import conv_bounds as cb  # noqa: E402
from oracle import ron_forward as orf  # noqa: E402

ROUND = {'bf16': orf.round_bf16, 'fp16': orf.round_f16}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


# (cout of the first member, of the second, columns the members must multiply)
PAIRS = [(20, 40, [32, 48]),      # the block4 score pair: objectness_score and loc_pred
         (32, 48, [32, 48]),      # exact widths: every lane of the last block stores
         (17, 33, [32, 48]),      # one channel into the second block / the third block
         (40, 20, [48, 32]),      # the other order
         (33, 49, [64, 64])]      # too wide for 32 / 48: the pair stays at 64 + 64


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
@pytest.mark.parametrize('pair', PAIRS, ids=lambda p: '%d_%d' % (p[0], p[1]))
def test_pair_at_its_own_widths_is_the_64_wide_pair_bit_for_bit(ops, dev, pair, dtype):
    ca, cb_, want = pair
    n, h, w, cin = 2, 8, 8, 64
    rs = np.random.RandomState(ca * 100 + cb_)
    x = rs.randn(n, h, w, 2 * cin).astype(np.float32)            # the members read channels [0, 64) and [64, 128)
    wa = (rs.randn(3, 3, cin, ca) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    wb = (rs.randn(3, 3, cin, cb_) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    ba, bb = (rs.randn(ca) * 0.1).astype(np.float32), (rs.randn(cb_) * 0.1).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    ya, yb, cols = ops.conv2d_patch_pair_nhwc(xd, cin, wa, ba, 0, wb, bb, cin, dtype=dtype)
    za, zb, wide = ops.conv2d_patch_pair_nhwc(xd, cin, wa, ba, 0, wb, bb, cin, dtype=dtype, full_width=True)
    assert cols == want and wide == [64, 64], (cols, wide)
    rnd = ROUND[dtype]
    for got, old, xs, wt, b in ((ya, za, x[..., :cin], wa, ba), (yb, zb, x[..., cin:], wb, bb)):
        got, old = got.cpu().numpy(), old.cpu().numpy()
        assert np.array_equal(got, old), '%d of %d outputs differ from the 64-wide pair' % ((got != old).sum(), got.size)
        ref, S, K = cb.conv_op(rnd(xs), rnd(wt), b, relu=False)
        top, at = cb.worst(cb.ratio(got, ref, S, K, dtype, 'fp32'))
        print('%s cout=%d: largest error / bound %.3f at %s' % (dtype, wt.shape[3], top, at))
        assert top <= 1.0, 'error / bound = %.3f at %s' % (top, at)


def test_other_dtypes_keep_64_columns(ops, dev):
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.randn(1, 8, 8, 64).astype(np.float32)).to(dev)
    wa, wb = (rs.randn(3, 3, 32, 20) * 0.05).astype(np.float32), (rs.randn(3, 3, 32, 40) * 0.05).astype(np.float32)
    for dtype in ('fp32', 'f16x3'):
        assert ops.conv2d_patch_pair_nhwc(x, 32, wa, None, 0, wb, None, 32, dtype=dtype)[2] == [64, 64]
