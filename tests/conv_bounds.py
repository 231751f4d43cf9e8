"""Float64 references of the convolution-type operations with a PER-ELEMENT error bound, and the exact-integer ("lattice") inputs.

Plain helper module (numpy only).  For one operation, given the operands AS THE KERNEL SEES THEM (already rounded to the storage
type with oracle.ron_forward.round_bf16 / round_f16 / round_f16x3; the bias stays float32, the kernels read it as such):

  ref64   the result in float64
  S       the same operation on |x|, |w|, |bias|, |residual|: the sum of magnitudes behind each output element
  K       the number of products behind each output element (kh * kw * cin; cin for the transposed 2x2 convolution)

and the check, per element, no exclusions (``ratio`` returns error / bound, above 1 fails):

    |got - ref64| <= u * |ref64| + (1 + u) * K * 2^-23 * S        (+ 2^-25 for fp16 outputs: the subnormal quantum)

Derivation:
  1. bf16 x bf16 and f16 x f16 products are exact in float32; K float32 additions of exact products in ANY order (split-K partial
     sums, the bias and residual additions included) err by at most one ulp each, relative to a partial sum <= S: K * 2^-23 * S.
     (Round-to-nearest gives half an ulp per addition; the other half pays for the bias / residual additions and keeps the
     textbook form.)  fp32 mode: the products round too -> 2K.
  2. ReLU and the 2x2 max-pool are monotone and 1-Lipschitz: they leave the bound unchanged (pool: ref and S are both max-pooled).
  3. The epilogue rounds the float32 value v to the storage type to nearest even: |got - v| <= u |v| <= u (|ref| + E), u = half
     an ulp relative to the value: 2^-8 bf16, 2^-11 fp16, 0 where the output is float32.
  4. f16x3 (two f16 planes per value): a stored value keeps 22 bits with an absolute floor of 2^-25, for operands and output:
     the bound gains 2 * 2^-22 * S + 2^-24.
  5. None of these constants is fitted to a kernel.

Two layers in one kernel (stem2: image -> conv1_1 -> conv1_2 -> pool1): conv1_1's result is rounded to the storage type inside the
kernel.  ``stem2_op`` takes layer one in float64 (a1), its bound delta1 = u |a1| + (1 + u) * 27 * 2^-23 * S1, feeds the UNROUNDED a1
to layer two, and layer two's accumulation term gains conv(delta1, |w2|): what the perturbation of its input can add to an output.
"""
import numpy as np

F64 = np.float64
U_HALF_ULP = {'fp32': 0.0, 'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11, 'f16x3': 0.0}
EPS32 = 2.0 ** -23


# --------------------------------------------------------------------------------------------------------------------- #
# float64 operations (NHWC, HWIO; TensorFlow SAME padding as oracle.ron_forward.conv2d_np)
# --------------------------------------------------------------------------------------------------------------------- #
def _same_pad(k, rate):
    total = (k - 1) * rate
    return total // 2, total - total // 2


def conv64(x, w, stride=1, rate=1):
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    n, h, wd, cin = x.shape
    kh, kw, _, cout = w.shape
    if stride == 1:
        pt, pb = _same_pad(kh, rate)
        pl, pr = _same_pad(kw, rate)
        xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))
        ho, wo = h, wd
    else:
        assert kh == stride and kw == stride and h % stride == 0 and wd % stride == 0 and rate == 1
        xp, ho, wo = x, h // stride, wd // stride
    out = np.zeros((n * ho * wo, cout), F64)
    for ky in range(kh):
        for kx in range(kw):
            if not w[ky, kx].any():
                continue
            patch = xp[:, ky * rate: ky * rate + (ho - 1) * stride + 1: stride, kx * rate: kx * rate + (wo - 1) * stride + 1: stride, :]
            out += patch.reshape(-1, cin) @ w[ky, kx]
    return out.reshape(n, ho, wo, cout)


def deconv64(x, w, stride=2):
    """kernel == stride transposed conv, w [kh, kw, Cout, Cin]."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    n, h, wd, cin = x.shape
    kh, kw, cout, _ = w.shape
    assert kh == stride and kw == stride
    out = np.zeros((n, h * stride, wd * stride, cout), F64)
    flat = x.reshape(-1, cin)
    for ky in range(kh):
        for kx in range(kw):
            out[:, ky::stride, kx::stride, :] = (flat @ w[ky, kx].T).reshape(n, h, wd, cout)
    return out


def pool64(x):
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))


def conv_op(x, w, bias=None, residual=None, stride=1, rate=1, relu=True, pool=False, transpose=False):
    """relu?(conv(x, w) + bias), then relu(. + residual) when a residual is given, then the 2x2 max-pool when `pool`
    -> (ref64, S, K).  The residual sum always ends in its ReLU (the reverse connection, conv_device.h), whatever `relu` says."""
    def run(x_, w_, b_, r_, act):
        y = deconv64(x_, w_, stride) if transpose else conv64(x_, w_, stride, rate)
        if b_ is not None:
            y = y + np.asarray(b_, F64)
        if act and relu:
            y = np.maximum(y, 0)
        if r_ is not None:
            y = y + np.asarray(r_, F64)
            if act:
                y = np.maximum(y, 0)
        return pool64(y) if pool else y
    ref = run(x, w, bias, residual, True)
    mag = run(np.abs(x), np.abs(w), None if bias is None else np.abs(bias), None if residual is None else np.abs(residual), False)
    w = np.asarray(w)
    k = w.shape[3] if transpose else w.shape[0] * w.shape[1] * w.shape[2]
    return ref, mag, k


def acc_term(S, K, dtype):
    """What the float32 accumulation (and, for f16x3, the 22-bit operands / output) may add, before the output rounding."""
    e = (2 * K if dtype == 'fp32' else K) * EPS32 * S
    if dtype == 'f16x3':
        e = e + 2 * 2.0 ** -22 * S + 2.0 ** -24
    return e


def bound(ref64, S, K, dtype, out_dtype=None, extra=0.0):
    """The per-element bound.  `dtype`: the arithmetic (operands); `out_dtype`: the storage type of the output (default: the same;
    'fp32' for the head tensors).  `extra`: an additional accumulation-side term (stem2: conv(delta1, |w2|))."""
    out_dtype = dtype if out_dtype is None else out_dtype
    u = U_HALF_ULP[out_dtype]
    b = u * np.abs(ref64) + (1 + u) * (acc_term(S, K, dtype) + extra)
    if out_dtype == 'fp16':
        b = b + 2.0 ** -25
    return b


def ratio(got, ref64, S, K, dtype, out_dtype=None, extra=0.0):
    """error / bound per element (0 / 0 = 0): the test asserts ratio(...).max() <= 1.  The check is `err <= bound`, no exclusions:
    wherever that is not true - a NaN or an infinite output included - the ratio is +inf (never NaN, so max() cannot lose it)."""
    err = np.abs(np.asarray(got, F64) - ref64)
    b = bound(ref64, S, K, dtype, out_dtype, extra)
    assert err.shape == b.shape, (err.shape, b.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        inside = err <= b                                   # False for NaN
        r = np.where(err == 0, 0.0, err / np.where(b > 0, b, np.finfo(F64).tiny))
    return np.where(inside, r, np.where(np.isfinite(r) & (r > 1.0), r, np.inf))


def worst(r):
    """(largest ratio, its index) for the report a test prints."""
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), tuple(int(v) for v in i)


def stem2_op(img, w1, b1, w2, b2, dtype, halo='zero', pool=True):
    """image -> relu(conv1_1 + b1) -> [rounded to `dtype` in the kernel] -> relu(conv1_2 + b2) -> 2x2 max-pool, in float64
    -> (ref64, S2, K2, extra) for bound(ref64, S2, K2, dtype, extra=extra); see the module docstring.
    halo='relu_bias' is the MUTANT in which conv1_2 sees relu(b1) instead of zero outside the image (tests/test_conv_bounds_cpu.py)."""
    a1, s1, k1 = conv_op(img, w1, b1, relu=True)
    delta1 = bound(a1, s1, k1, dtype)
    ref, s2, k2 = conv_op(a1, w2, b2, relu=True, pool=pool)
    if halo == 'relu_bias':
        n, h, w, c = a1.shape
        padded = np.broadcast_to(np.maximum(np.asarray(b1, F64), 0), (n, h + 2, w + 2, c)).copy()
        padded[:, 1:-1, 1:-1, :] = a1
        full = conv64(padded, w2)[:, 1:-1, 1:-1, :]          # SAME conv of the padded map, cropped = VALID conv over the halo
        ref = np.maximum(full + np.asarray(b2, F64), 0)
        ref = pool64(ref) if pool else ref
    extra = conv64(delta1, np.abs(w2))
    return ref, s2, k2, (pool64(extra) if pool else extra)


# --------------------------------------------------------------------------------------------------------------------- #
# exact-integer inputs: every product and partial sum is an integer below 2^8, whatever the accumulation order
# --------------------------------------------------------------------------------------------------------------------- #
def lattice_weights(kh, kw, cin, cout, nnz=64, draw=0, seed=0):
    """HWIO weights in {-1, 0, +1}: output channel n has its non-zeros at the flat (tap, channel) indices o_n + j * step,
    step = ceil(K / nnz), o_n = (n + draw * cout) mod step: at most `nnz` per output channel, and over ceil(step / cout) draws
    every K index is non-zero in some output channel (lattice_draws / assert_lattice)."""
    K = kh * kw * cin
    step = -(-K // nnz)
    rs = np.random.RandomState(1000 * seed + draw)
    w = np.zeros((K, cout), np.float32)
    for n in range(cout):
        idx = np.arange((n + draw * cout) % step, K, step)
        w[idx, n] = rs.choice([-1.0, 1.0], size=idx.size)
    return w.reshape(kh, kw, cin, cout)


def lattice_draws(kh, kw, cin, cout, nnz=64):
    """How many shifted draws cover every K index."""
    step = -(-(kh * kw * cin) // nnz)
    return -(-step // cout)


def lattice_centre_weights(cin, cout, center_from, nnz=64, seed=0):
    """3x3 HWIO lattice weights whose output channels >= center_from live in the centre tap only (a 1x1 branch packed beside 3x3 ones)."""
    w = lattice_weights(3, 3, cin, cout, nnz, seed=seed)
    w[:, :, :, center_from:] = 0
    w[1, 1, :, center_from:] = lattice_weights(1, 1, cin, cout - center_from, nnz, seed=seed + 1)[0, 0]
    return w


def lattice_deconv_weights(cin, cout, nnz=64, seed=0):
    """[2, 2, Cout, Cin] for the transposed 2x2 convolution: each tap is a 1x1 lattice of its own."""
    w = np.zeros((2, 2, cout, cin), np.float32)
    for t in range(4):
        w[t // 2, t % 2] = lattice_weights(1, 1, cin, cout, nnz, seed=seed + t)[0, 0].T
    return w


def lattice_acts(shape, seed=0, lo=-2, hi=2):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float32)


def lattice_bias(cout, seed=0, nonzero=False):
    rs = np.random.RandomState(seed + 77)
    b = rs.randint(-8, 9, size=cout).astype(np.float32)
    if nonzero:
        b[b == 0] = 3.0
    return b


def lattice_residual(shape, seed=0):
    return np.random.RandomState(seed + 99).randint(0, 9, size=shape).astype(np.float32)


def assert_lattice(ws, nnz=64, covered=None):
    """The generator's two conditions on a list of HWIO weight draws of one layer: at most `nnz` non-zeros per output channel in
    each draw, and every (tap, input channel) index (or those where `covered` [kh, kw, cin] is True) non-zero in some output channel
    of some draw."""
    seen = np.zeros(ws[0].shape[:3], bool)
    for w in ws:
        assert set(np.unique(w)) <= {-1.0, 0.0, 1.0}
        per_out = (w != 0).reshape(-1, w.shape[3]).sum(axis=0)
        assert per_out.max() <= nnz, 'more than %d non-zeros in an output channel: %d' % (nnz, per_out.max())
        seen |= (w != 0).any(axis=3)
    want = np.ones_like(seen) if covered is None else covered
    assert (seen | ~want).all(), '%d K indices carry no weight in any output channel' % int((~seen & want).sum())


def stem2_lattice(seed=0):
    """(w1, b1, w2, b2) of the fused two-layer stem: conv1_1 two non-zeros per output channel + bias in [1, 2] -> 0 <= a1 <= 8, all 27
    (tap, channel) indices covered over the 64 outputs; conv1_2 24 non-zeros per output channel over K = 576, bias in [-8, 8]."""
    rs = np.random.RandomState(seed + 5)
    w1 = np.zeros((27, 64), np.float32)
    for n in range(64):
        w1[n % 27, n] = rs.choice([-1.0, 1.0])
        w1[(n + 13) % 27, n] = rs.choice([-1.0, 1.0])
    b1 = rs.randint(1, 3, size=64).astype(np.float32)
    w2 = lattice_weights(3, 3, 64, 64, nnz=24, seed=seed + 6)
    b2 = lattice_bias(64, seed + 7)
    return w1.reshape(3, 3, 3, 64), b1, w2, b2
