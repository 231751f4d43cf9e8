"""Cases and inputs of the training-forward tests (tests/test_conv_fwd_cpu.py, tests/test_gpu_conv_forward.py,
tests/test_gpu_conv7_backward.py).

Plain helper module (numpy only).  A case is (n, h, w, cin, cout, k, dilation, stride, transpose) - n, h, w are the INPUT's - the
smallest shapes at which each decision of ron_conv2d_forward_nhwc can go wrong: the seven of conv_grad_cases.CASES plus the 7 x 7
filter, one output channel, a column tile with one live column, the stem and both 2 x 2 stride-2 forms."""
import numpy as np

import conv_bounds as cb
import conv_grad_cases as cg

CASES = {name: c + (1, 0) for name, c in cg.CASES.items()}
CASES.update({
    'K7over': (2, 5, 7, 64, 24, 7, 1, 1, 0),         # the 7 x 7 filter overhangs the map on every side
    'K7fc6': (1, 10, 10, 128, 192, 7, 1, 1, 0),      # fc6's own map (`full`)
    'fc6red': (1, 10, 10, 64, 64, 3, 3, 1, 0),       # fc6 of `reducedfc`: 3 x 3 at dilation 3
    'cout1': (2, 3, 5, 64, 1, 3, 1, 1, 0),           # one output channel: 63 zero rows in the packed block, 4-byte loads of w
    'cout65': (2, 4, 6, 128, 65, 1, 1, 1, 0),        # a 1 x 1 whose second column block holds one live row
    'stem': (2, 8, 32, 3, 64, 3, 1, 1, 0),           # the stem, whole 32-pixel tiles
    'stemrag': (2, 9, 37, 3, 64, 3, 1, 1, 0),        # ... and a ragged width
    's2': (2, 6, 8, 64, 24, 2, 1, 2, 0),             # 2 x 2 stride 2
    's2min': (1, 2, 2, 128, 128, 2, 1, 2, 0),        # ... one output pixel
    't2': (2, 3, 5, 64, 128, 2, 1, 2, 1),            # 2 x 2 stride 2 transposed
    't2min': (1, 1, 1, 128, 256, 2, 1, 2, 1),        # ... one input pixel
})
# the three 7 x 7 shapes of the backward tests: the two above and one with three images and a cout that is no multiple of 64
K7_GRAD = {'K7over': CASES['K7over'][:7], 'K7fc6': CASES['K7fc6'][:7], 'K7three': (3, 4, 4, 64, 70, 7, 1)}
DTYPES = ('bf16', 'fp16')


def out_shape(case):
    n, h, w, cin, cout, k, rate, stride, tr = CASES[case] if isinstance(case, str) else case
    return (n, h * stride, w * stride, cout) if tr else (n, h // stride, w // stride, cout)


def w_shape(case):
    n, h, w, cin, cout, k, rate, stride, tr = CASES[case] if isinstance(case, str) else case
    return (k, k, cout, cin) if tr else (k, k, cin, cout)


def inputs(kind, case, seed=0):
    """(x, w, bias) float32.  lattice: integers whose every partial sum is exact in float32 and whose result a bf16 holds (|y| <= 2 * 64
    + 8 < 256): x in [-2, 2], w in {-1, 0, 1} with at most 64 non-zeros per output channel, bias in [-8, 8].  gauss: N(0, 1)
    activations, He-scaled weights, a bias of about 0.1."""
    n, h, w, cin, cout, k, rate, stride, tr = CASES[case] if isinstance(case, str) else case
    rs = np.random.RandomState(300 + seed)
    if kind == 'lattice':
        x = cb.lattice_acts((n, h, w, cin), seed=seed)
        wt = cb.lattice_deconv_weights(cin, cout, seed=seed) if tr else cb.lattice_weights(k, k, cin, cout, seed=seed)
        b = cb.lattice_bias(cout, seed=seed)
    else:
        x = rs.randn(n, h, w, cin).astype(np.float32)
        fan = cin if tr else k * k * cin
        wt = (rs.randn(*w_shape(case)) * np.sqrt(2.0 / fan)).astype(np.float32)
        b = (rs.randn(cout) * 0.1).astype(np.float32)
    return x, np.ascontiguousarray(wt), b
