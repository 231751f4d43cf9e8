"""Cases and inputs of the stem-backward tests (tests/test_stem_grad_cpu.py, tests/test_gpu_stem_backward.py).

Plain helper module (numpy only).  A case is (n, h, w) of the 3 -> 64 channel, 3x3 stem convolution: the smallest shapes at which
each decision of ron_conv2d_stem_backward_nhwc can go wrong.  The kernel walks the pixels in dense order, 32 to a K step."""
import numpy as np

CASES = {
    'A': (1, 1, 1),        # only the centre tap sees the map: the other eight taps of dw must be exactly 0
    'B': (2, 5, 7),        # 70 pixels, not a multiple of 32; steps straddle rows and images
    'C': (3, 3, 3),        # three images inside one K step: no tap may leak into a neighbour image
    'D': (1, 1, 33),       # one row longer than a step: no vertical taps
    'E': (1, 33, 1),       # one column: no horizontal taps
    'F': (1, 8, 32),       # rows equal to the step
    'G': (2, 40, 40),      # 100 steps: the by-shape split and forced splits
}
KINDS = ('lattice', 'gauss')
DTYPES = ('bf16', 'fp16')
CIN, COUT = 3, 64
MAX_PRODUCT = 302          # 151 * 2
MAX_PIXELS = 3200          # 302 * 3200 < 2^24


def inputs(kind, case, seed=0):
    """(x, y, dy) float32: x [n,h,w,3], y (a forward output: >= 0, exact zeros where the ReLU cut) and dy [n,h,w,64].

    lattice: x integers in [-128, 151] (an image after mean subtraction: exact in bf16 and fp16), dy integers in [-2, 2],
    y = relu(integers in [-1, 3]), 40 % exact zeros.  gauss: x = 60 randn (not storage-exact: a missing rounding of x shows)."""
    n, h, w = CASES[case] if isinstance(case, str) else case
    rs = np.random.RandomState(300 + seed)
    if kind == 'lattice':
        x = rs.randint(-128, 152, size=(n, h, w, CIN)).astype(np.float32)
        dy = rs.randint(-2, 3, size=(n, h, w, COUT)).astype(np.float32)
        y = np.maximum(rs.randint(-1, 4, size=(n, h, w, COUT)), 0).astype(np.float32)
    else:
        x = (60.0 * rs.randn(n, h, w, CIN)).astype(np.float32)
        dy = rs.randn(n, h, w, COUT).astype(np.float32)
        y = np.maximum(rs.randn(n, h, w, COUT), 0).astype(np.float32)
    return x, y, dy


def assert_lattice(x, dz, round_fns):
    """The conditions under which the lattice results are exact in any accumulation order: x and dz integers the storage types hold
    exactly, every product at most 302 in magnitude, at most 3200 pixels: every partial sum is an integer below 302 * 3200 < 2^24."""
    for a in (x, dz):
        assert np.array_equal(a, np.round(a))
        for rnd in round_fns:
            assert np.array_equal(rnd(a), a), 'a lattice value is not exact in a storage type'
    assert np.abs(x).max() * np.abs(dz).max() <= MAX_PRODUCT
    pixels = x.shape[0] * x.shape[1] * x.shape[2]
    assert pixels <= MAX_PIXELS and MAX_PRODUCT * MAX_PIXELS < 2 ** 24
