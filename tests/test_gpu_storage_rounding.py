"""The rounding contract of csrc/storage_device.h on the GPU: every path that turns an fp32 value into a storage-type (bf16 / fp16)
value gives, for every finite input, round-to-nearest-even with overflow to +-inf - the bits of the torch CPU cast
`x.to(dtype).float()` (checked on the CPU against the bit-trick rounding on 2.6 M finite values: no tolerance, np.array_equal on
the uint32 views).

One tensor of special values, n = 256, h = w = 1, c = 64 (16 384 values), goes down each path:

  forward boundary   ops.maxpool2x2_nhwc(x) on the 1 x 1 map: y = round(x)            (elementwise.hip: HIP's conversions)
  round_storage      ops.maxpool2x2_backward_nhwc(zeros, dy): dx = round(dy)          (op_backward.hip; ssd_backward.hip, batchnorm.hip)
  round_bits, pack8  ops.conv2d_forward_nhwc, 1 x 1 identity weight, 64 -> 64, no bias, no ReLU: y = round(x)   (the halo pack)

The values: ties at the midpoint of the dropped bits with an even and an odd kept mantissa, each +- 1 ulp of fp32; +-0; the largest
fp32 that still rounds to the largest finite storage value and the next one, which rounds to inf; fp32 subnormals; fp32 normals that
round into fp16's subnormal range; random finite bit patterns from a fixed seed.  The convolution takes only the values whose
rounded result is finite and normal in the storage type (the others are replaced by 1): an inf times the zero weights is a NaN, the
sign of a zero sum depends on the other 63 products, and how the matrix pipe treats subnormal operands is not asserted here.
No NaN inputs: the paths differ there by design (storage_device.h)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

N, C = 256, 64
TORCH = {'bf16': torch.bfloat16, 'f16': torch.float16}
# dropped mantissa bits of a normal value, smallest normal and largest finite value of the storage type as fp32 bits
DROPPED = {'bf16': 16, 'f16': 13}
MIN_NORMAL = {'bf16': 0x00800000, 'f16': 0x38800000}
MAX_FINITE = {'bf16': 0x7F7F0000, 'f16': 0x477FE000}


@functools.lru_cache(maxsize=None)
def special_bits(dtype):
    """The 16 384 fp32 bit patterns of the test, all finite."""
    drop = DROPPED[dtype]
    half = 1 << (drop - 1)
    bits = []
    # ties (and +- 1 ulp of fp32) over the storage type's normal range, kept mantissa even, odd, all ones (the carry into the exponent)
    exps = range(1, 255) if dtype == 'bf16' else range(113, 143)
    for e in exps:
        for kept in (0, 1, 2, 3, (1 << (23 - drop)) - 2, (1 << (23 - drop)) - 1):
            mid = (e << 23) | (kept << drop) | half
            bits += [mid - 1, mid, mid + 1]
    bits += [0x00000000]
    # the largest value that stays finite, the first that becomes inf, and the largest finite fp32
    edge = MAX_FINITE[dtype] | (half - 1)
    bits += [MAX_FINITE[dtype], edge - 1, edge, edge + 1, edge + 2, 0x7F7FFFFF]
    # fp32 subnormals (bf16 keeps them as subnormals of its own: ties there too)
    bits += [0x00000001, 0x00000002, 0x00007FFF, 0x00008000, 0x00008001, 0x00017FFF, 0x00018000, 0x00018001, 0x00400000, 0x007F7FFF,
             0x007F8000, 0x007FFFFF, 0x00800000]
    if dtype == 'f16':
        # fp32 normals in fp16's subnormal range (spacing 2^-24) and below it: ties between multiples of 2^-24, +- 1 ulp
        for k in range(0, 40):
            v = np.float32((2 * k + 1) * 2.0 ** -25)
            b = int(v.view(np.uint32))
            bits += [b - 1, b, b + 1]
        bits += [0x33000000 - 1, 0x33000000, 0x33000001, 0x32FFFFFF, 0x387FFFFF, 0x387FF000, 0x387FEFFF, 0x387FF001]
    bits = np.array(bits, dtype=np.uint32)
    bits = np.concatenate([bits, bits | np.uint32(0x80000000)])          # both signs
    rs = np.random.RandomState(20261021)
    fill = N * C - bits.size
    assert fill >= 4000, fill
    rnd = rs.randint(0, 1 << 32, size=fill, dtype=np.uint64).astype(np.uint32)
    if dtype == 'f16':
        # half of them with an exponent fp16 can hold (2^-27 .. 2^17), or nearly all random patterns would be 0 or inf
        e = rs.randint(100, 145, size=fill).astype(np.uint32)
        rnd = np.where(np.arange(fill) % 2 == 0, (rnd & np.uint32(0x807FFFFF)) | (e << np.uint32(23)), rnd)
    rnd = np.where((rnd & np.uint32(0x7F800000)) == np.uint32(0x7F800000), rnd & np.uint32(0xBFFFFFFF), rnd)      # finite
    bits = np.concatenate([bits, rnd])
    rs.shuffle(bits)
    assert bits.size == N * C and np.isfinite(bits.view(np.float32)).all()
    return bits


@functools.lru_cache(maxsize=None)
def case(dtype):
    """(x [N,1,1,C] fp32, its rounding's uint32 bits) - the reference is computed once per dtype and never written to."""
    x = torch.from_numpy(special_bits(dtype).view(np.float32).reshape(N, 1, 1, C).copy())
    want = x.to(TORCH[dtype]).float().numpy().view(np.uint32)
    want.setflags(write=False)
    return x, want


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


def check(got, want, x, what):
    got = got.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    xb = x.numpy().view(np.uint32).ravel()
    print('%s: %d of %d values differ%s' % (what, bad.size, want.size, ''.join(
        '\n  x %08x  got %08x  want %08x' % (xb[i], got.ravel()[i], want.ravel()[i]) for i in bad[:16])))
    assert np.array_equal(got, want), what


def test_the_values_cover_what_they_claim():
    for dtype in TORCH:
        x, want = case(dtype)
        r = want.view(np.float32)
        assert np.isinf(r).any() and (r == 0).any() and (want == 0x80000000).any()
        mag = want & 0x7FFFFFFF
        assert ((mag > 0) & (mag < MIN_NORMAL[dtype])).any(), 'no subnormal result'
        assert (mag == MAX_FINITE[dtype]).any()


@pytest.mark.parametrize('dtype', sorted(TORCH))
def test_forward_boundary(dev, ops, dtype):
    x, want = case(dtype)
    check(ops.maxpool2x2_nhwc(x.to(dev), dtype=dtype), want, x, 'forward boundary %s' % dtype)


@pytest.mark.parametrize('dtype', sorted(TORCH))
def test_round_storage(dev, ops, dtype):
    x, want = case(dtype)
    dx = ops.maxpool2x2_backward_nhwc(torch.zeros(N, 1, 1, C, device=dev), x.to(dev), dtype=dtype)
    check(dx, want, x, 'round_storage %s' % dtype)


@pytest.mark.parametrize('dtype', sorted(TORCH))
def test_round_bits_pack8(dev, ops, dtype):
    x, want = case(dtype)
    mag = want & 0x7FFFFFFF
    fit = torch.from_numpy((mag >= MIN_NORMAL[dtype]) & (mag <= MAX_FINITE[dtype]))
    assert int(fit.sum()) > N * C // 4
    xc = torch.where(fit, x, torch.ones_like(x))
    wantc = xc.to(TORCH[dtype]).float().numpy().view(np.uint32)
    w = torch.eye(C, device=dev).reshape(1, 1, C, C)
    y = ops.conv2d_forward_nhwc(xc.to(dev), w, None, relu=False, dtype=dtype)
    check(y, wantc, xc, 'round_bits / pack8 %s' % dtype)
