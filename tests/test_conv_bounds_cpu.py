"""The per-element conv check checks itself (numpy only, no GPU): honest emulations of the kernels' arithmetic - float32 accumulation
in two different orders, round to nearest even - pass the bound of tests/conv_bounds.py and are bit-exact on the integer lattice;
every mutant (a subtly wrong kernel) fails the bound on Gaussian inputs AND fails np.array_equal on the lattice inputs.  It also
pins the lattice generator's two conditions (<= 64 non-zeros per output channel, every K index covered)."""
import numpy as np
import pytest

import conv_bounds as cb
from oracle import ron_forward as orf

F32 = np.float32


def trunc_bf16(a):
    return (np.ascontiguousarray(a, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def emulate(x, w, b, order='taps', mutant=None, rnd=orf.round_bf16):
    """3x3 SAME conv + bias + ReLU as a 16-bit kernel computes it: exact products, float32 accumulation (order 'taps': tap after tap;
    'splitk': taps reversed, the channels in two halves summed apart and added at the end, the bias last), output rounded by `rnd`."""
    x, w, b = np.asarray(x, F32), np.array(w, F32), np.array(b, F32)
    n, h, wd, cin = x.shape
    cout = w.shape[3]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    patch = {(ky, kx): xp[:, ky:ky + h, kx:kx + wd, :] for ky in range(3) for kx in range(3)}
    if mutant == 'drop_bias':
        b[5] = 0
    if mutant == 'drop_k':
        w[DROP_K[0], DROP_K[1], DROP_K[2], :16] = 0
    if mutant == 'swap_centre':
        w[1, 1, [SWAP[0], SWAP[1]], :] = w[1, 1, [SWAP[1], SWAP[0]], :]
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]

    def accumulate(wt):
        if order == 'taps':
            acc = np.zeros((n, h, wd, cout), F32)
            for t in taps:
                acc += patch[t] @ wt[t]
            return acc
        half = cin // 2
        lo, hi = np.zeros((n, h, wd, cout), F32), np.zeros((n, h, wd, cout), F32)
        for t in taps[::-1]:
            lo += patch[t][..., :half] @ wt[t][:half]
            hi += patch[t][..., half:] @ wt[t][half:]
        return hi + lo

    acc = accumulate(w)
    if mutant == 'corner_tap':                         # output pixel (0, 0) of image 0 misses its centre tap
        acc[0, 0, 0] -= patch[(1, 1)][0, 0, 0] @ w[1, 1]
    if mutant == 'last_row_taps':                      # the top-left and the bottom-right tap exchanged, last image row only
        w2 = w.copy()
        w2[0, 0], w2[2, 2] = w[2, 2], w[0, 0]
        acc[:, -1] = accumulate(w2)[:, -1]
    y = np.maximum(acc, 0) + b if mutant == 'relu_before_bias' else np.maximum(acc + b, 0)
    return trunc_bf16(y) if mutant == 'truncate' else rnd(y)


DROP_K = (0, 0, 0)       # (ky, kx, channel) of the dropped K element (output channel 0 of the lattice has a weight there)
SWAP = (0, 1)            # the two input channels exchanged inside the centre tap
MUTANTS = ['drop_bias', 'truncate', 'drop_k', 'corner_tap', 'swap_centre', 'relu_before_bias', 'last_row_taps']


def _gauss(cin, cout=64, seed=0):
    rs = np.random.RandomState(seed)
    x = orf.round_bf16(rs.randn(2, 12, 10, cin))
    w = orf.round_bf16(rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin)))
    b = (rs.randn(cout) * 0.1).astype(F32)
    return x, w, b


def _lattice(cin, cout=64):
    x = cb.lattice_acts((2, 12, 10, cin), seed=1)
    w = cb.lattice_weights(3, 3, cin, cout)
    b = cb.lattice_bias(cout, nonzero=True)
    return x, w, b


@pytest.mark.parametrize('cin', [64, 512])
@pytest.mark.parametrize('order', ['taps', 'splitk'])
def test_honest_arithmetic_passes(cin, order):
    x, w, b = _gauss(cin)
    ref, S, K = cb.conv_op(x, w, b)
    r = cb.ratio(emulate(x, w, b, order), ref, S, K, 'bf16')
    print('honest bf16, K = %d, order %s: largest ratio %.3f at %s' % ((K, order) + cb.worst(r)))
    assert r.max() <= 1.0
    r16 = cb.ratio(emulate(orf.round_f16(x), orf.round_f16(w), b, order, rnd=orf.round_f16), *cb.conv_op(orf.round_f16(x), orf.round_f16(w), b), 'fp16')
    assert r16.max() <= 1.0
    # fp32 output of 16-bit operands (the head tensors): u = 0, the accumulation term alone
    r32 = cb.ratio(emulate(x, w, b, order, rnd=lambda a: a), ref, S, K, 'bf16', out_dtype='fp32')
    assert r32.max() <= 1.0
    xl, wl, bl = _lattice(cin)
    assert np.array_equal(emulate(xl, wl, bl, order), cb.conv_op(xl, wl, bl)[0])


@pytest.mark.parametrize('where', ['one', 'all'])
@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf], ids=['nan', 'inf', '-inf'])
def test_non_finite_output_fails_bound_and_lattice(bad, where):
    """`|got - ref| <= bound` is false for a NaN: one NaN / infinite element, or a tensor full of them, must fail - in every output
    type, fp32 outputs (the head tensors) included - and the reported largest ratio must be +inf, not NaN and not the clean value."""
    x, w, b = _gauss(64)
    ref, S, K = cb.conv_op(x, w, b)
    for out_dtype, rnd in (('bf16', orf.round_bf16), ('fp32', lambda a: a)):
        got = emulate(x, w, b, rnd=rnd).copy()
        assert cb.ratio(got, ref, S, K, 'bf16', out_dtype).max() <= 1.0
        if where == 'one':
            got[1, 7, 3, 11] = bad
        else:
            got[:] = bad
        r = cb.ratio(got, ref, S, K, 'bf16', out_dtype)
        assert not np.isnan(r).any() and r.max() == np.inf and cb.worst(r)[0] == np.inf
        assert (r[1, 7, 3, 11] == np.inf) and (where == 'all' or np.isfinite(np.delete(r.ravel(), np.ravel_multi_index((1, 7, 3, 11), r.shape))).all())
    xl, wl, bl = _lattice(64)
    gl = emulate(xl, wl, bl).copy()
    gl[(0, 0, 0, 0) if where == 'one' else Ellipsis] = bad
    assert not np.array_equal(gl, cb.conv_op(xl, wl, bl)[0])


@pytest.mark.parametrize('mutant', MUTANTS)
def test_mutant_fails_bound_and_lattice(mutant):
    cin = 512 if mutant == 'drop_k' else 64            # one K element of 4608 / of 576
    x, w, b = _gauss(cin)
    ref, S, K = cb.conv_op(x, w, b)
    assert cb.ratio(emulate(x, w, b), ref, S, K, 'bf16').max() <= 1.0
    r = cb.ratio(emulate(x, w, b, mutant=mutant), ref, S, K, 'bf16')
    print('%s: largest ratio %.2f at %s' % ((mutant,) + cb.worst(r)))
    assert r.max() > 1.0, 'the per-element bound lets %s through' % mutant
    xl, wl, bl = _lattice(cin)
    refl = cb.conv_op(xl, wl, bl)[0]
    assert np.array_equal(emulate(xl, wl, bl), refl)
    assert not np.array_equal(emulate(xl, wl, bl, mutant=mutant), refl) or mutant == 'truncate', 'the lattice case lets %s through' % mutant
    if mutant == 'truncate':
        # integers below 256 are exact in bf16 whatever the rounding mode: the lattice cannot see it (the bound above does)
        assert np.array_equal(emulate(xl, wl, bl, mutant=mutant), refl)


def test_lattice_generator_conditions():
    """|out| <= 2 * 64 + 8 + 8 < 256, every (tap, channel) index covered - also where 64 * Cout < K (several draws)."""
    for (kh, cin, cout) in ((3, 512, 128), (3, 64, 20), (7, 64, 128), (1, 192, 256), (2, 128, 128), (7, 512, 16), (3, 512, 40)):
        draws = cb.lattice_draws(kh, kh, cin, cout)
        ws = [cb.lattice_weights(kh, kh, cin, cout, draw=d) for d in range(draws)]
        cb.assert_lattice(ws)
        if 64 * cout < kh * kh * cin:
            assert draws > 1
            with pytest.raises(AssertionError):
                cb.assert_lattice(ws[:-1])                      # one draw fewer does not cover K
    x = cb.lattice_acts((2, 12, 12, 512), seed=3)
    w = cb.lattice_weights(3, 3, 512, 128)
    b = cb.lattice_bias(128)
    res = cb.lattice_residual((2, 12, 12, 128))
    ref, S, _ = cb.conv_op(x, w, b, residual=res)
    assert S.max() <= 2 * 64 + 8 + 8 and np.abs(ref).max() < 256
    plain = cb.conv_op(x, w, b)[0]
    assert np.array_equal(orf.round_bf16(plain), plain)         # exact in bf16's 8 significant bits
    assert 0.2 < np.mean(plain > 0) < 0.8 and len(np.unique(plain)) > 30
    wc = cb.lattice_centre_weights(128, 512, 256)
    covered = np.zeros((3, 3, 128), bool)
    covered[1, 1] = True
    cb.assert_lattice([wc[..., 256:]], covered=covered)
    cb.assert_lattice([wc[..., :256]])
    assert not wc[0, 0, :, 256:].any()
    wd = cb.lattice_deconv_weights(128, 128)
    for t in range(4):
        cb.assert_lattice([wd[t // 2, t % 2].T[None, None]])


def _stem2_emulate(img, w1, b1, w2, b2, halo_relu_bias=False):
    """stem2 as the kernel computes it: conv1_1 in float32, rounded to bf16, zero outside the image, conv1_2 + pool in float32."""
    a1 = emulate_valid(np.pad(img, ((0, 0), (1, 1), (1, 1), (0, 0))), w1, b1)
    n, h, w, _ = img.shape
    if halo_relu_bias:
        full = np.broadcast_to(orf.round_bf16(np.maximum(b1, 0)), (n, h + 2, w + 2, 64)).copy()
    else:
        full = np.zeros((n, h + 2, w + 2, 64), F32)
    full[:, 1:-1, 1:-1] = a1
    return orf.max_pool2x2_np(emulate_valid(full, w2, b2))


def emulate_valid(xp, w, b):
    n, hp, wp, _ = xp.shape
    acc = np.zeros((n, hp - 2, wp - 2, w.shape[3]), F32)
    for ky in range(3):
        for kx in range(3):
            acc += np.asarray(xp[:, ky:ky + hp - 2, kx:kx + wp - 2, :], F32) @ np.asarray(w[ky, kx], F32)
    return orf.round_bf16(np.maximum(acc + np.asarray(b, F32), 0))


def test_two_layer_stem_reference_and_halo_mutant():
    rs = np.random.RandomState(4)
    # a low-contrast image (whitened values of a few units): conv1_1's outputs are then of the size of relu(b1), which is where a
    # wrong halo shows; at +-130 the rounding of conv1_1's own outputs (delta1) is larger than the whole halo error
    img = orf.round_bf16(rs.randn(2, 16, 32, 3) * 2)
    w1 = orf.round_bf16(rs.randn(3, 3, 3, 64) * np.sqrt(2.0 / 27))
    b1 = np.abs(rs.randn(64) * 0.5).astype(F32) + 0.5
    w2 = orf.round_bf16(rs.randn(3, 3, 64, 64) * np.sqrt(2.0 / 576))
    b2 = (rs.randn(64) * 0.1).astype(F32)
    ref, S, K, extra = cb.stem2_op(img, w1, b1, w2, b2, 'bf16')
    r = cb.ratio(_stem2_emulate(img, w1, b1, w2, b2), ref, S, K, 'bf16', extra=extra)
    print('honest two-layer stem: largest ratio %.3f at %s' % cb.worst(r))
    assert r.max() <= 1.0
    r = cb.ratio(_stem2_emulate(img, w1, b1, w2, b2, halo_relu_bias=True), ref, S, K, 'bf16', extra=extra)
    print('conv1_1 halo = relu(bias): largest ratio %.1f at %s' % cb.worst(r))
    assert r.max() > 1.0
    interior = r[:, 1:-1, 1:-1]
    assert interior.max() <= 1.0                                    # only the border of pool1 sees the halo
    # the float64 mutant reference of the helper says the same
    assert cb.ratio(orf.round_bf16(cb.stem2_op(img, w1, b1, w2, b2, 'bf16', halo='relu_bias')[0]), ref, S, K, 'bf16', extra=extra).max() > 1.0
    # lattice: image integers in [-3, 3]; 0 <= a1 <= 8; |out| < 256; every index of both layers covered
    imgl = cb.lattice_acts((2, 16, 32, 3), seed=2, lo=-3, hi=3)
    w1l, b1l, w2l, b2l = cb.stem2_lattice()
    cb.assert_lattice([w1l], nnz=2)
    cb.assert_lattice([w2l], nnz=24)
    assert b1l.min() >= 1 and b1l.max() <= 2
    a1 = cb.conv_op(imgl, w1l, b1l)[0]
    refl, Sl, _, _ = cb.stem2_op(imgl, w1l, b1l, w2l, b2l, 'bf16')
    assert a1.min() >= 0 and a1.max() <= 8 and a1.max() >= 4 and Sl.max() <= 24 * 8 + 8
    assert np.array_equal(_stem2_emulate(imgl, w1l, b1l, w2l, b2l), refl)
    bad = _stem2_emulate(imgl, w1l, b1l, w2l, b2l, halo_relu_bias=True)
    assert not np.array_equal(bad, refl)
    assert np.array_equal(bad[:, 1:-1, 1:-1], refl[:, 1:-1, 1:-1])
