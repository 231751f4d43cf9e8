"""Cases and inputs of the convolution-backward tests (tests/test_conv_grad_cpu.py, tests/test_gpu_conv_backward.py).

Plain helper module (numpy only).  A case is (n, h, w, cin, cout, k, dilation): the smallest shapes at which each decision of
ron_conv2d_backward_nhwc can go wrong."""
import numpy as np

import conv_bounds as cb

CASES = {
    'A': (1, 1, 1, 64, 64, 3, 1),        # only the centre tap sees the map: the other eight dw taps must be exactly 0
    'B': (2, 5, 7, 64, 24, 3, 1),        # non-square, 70 pixels (not a multiple of 32), cout padded from 24
    'C': (3, 3, 3, 128, 126, 3, 1),      # three images sharing halos, cout 126
    'D': (1, 10, 10, 64, 192, 3, 6),     # halo wider than half the map, cout not a multiple of 128
    'E': (2, 19, 19, 192, 64, 1, 1),     # 1x1 (pad 0), odd map, cin not a multiple of 128
    'F': (1, 38, 38, 320, 256, 3, 1),    # several tiles in both channel axes with a partial one; pixels enough for the by-shape split
    'G': (2, 40, 40, 64, 64, 3, 1),      # few tiles, many pixels: the large-split regime
}
SMALL = ('A', 'B', 'C', 'D', 'E')
KINDS = ('lattice', 'gauss')
DTYPES = ('bf16', 'fp16')


def inputs(kind, case, seed=0):
    """(x, w, y, dy) float32: x [n,h,w,cin], w HWIO, y (a forward output: >= 0, exact zeros where the ReLU cut) and dy [n,h,w,cout].

    lattice: x, dy integers in [-2, 2]; y = relu(integers in [-1, 3]), 40 % exact zeros; w in {-1, 0, 1} with at most 64 non-zeros per
    INPUT channel (the data gradient sums over taps and output channels: conv_bounds.lattice_weights bounds the non-zeros of the
    forward's output channels, so it is drawn for the swapped shape and transposed): |dx| <= 2 * 64, every partial sum an integer."""
    n, h, w, cin, cout, k, _ = CASES[case] if isinstance(case, str) else case      # (a case of another table: tests/conv_envelope_cases.py)
    rs = np.random.RandomState(100 + seed)
    if kind == 'lattice':
        x = rs.randint(-2, 3, size=(n, h, w, cin)).astype(np.float32)
        dy = rs.randint(-2, 3, size=(n, h, w, cout)).astype(np.float32)
        y = np.maximum(rs.randint(-1, 4, size=(n, h, w, cout)), 0).astype(np.float32)
        wt = np.ascontiguousarray(cb.lattice_weights(k, k, cout, cin, seed=seed).transpose(0, 1, 3, 2))
    else:
        x = rs.randn(n, h, w, cin).astype(np.float32)
        dy = rs.randn(n, h, w, cout).astype(np.float32)
        y = np.maximum(rs.randn(n, h, w, cout), 0).astype(np.float32)
        wt = (rs.randn(k, k, cin, cout) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
    return x, wt, y, dy


def assert_lattice(w, dx, dw, db):
    """The conditions under which the lattice results are exact in any accumulation order: integers, dx below 2^8 (a bf16 holds it),
    dw and db below 2^24 (an fp32 sum holds every partial sum)."""
    assert set(np.unique(w)) <= {-1.0, 0.0, 1.0}
    assert (w != 0).sum(axis=(0, 1, 3)).max() <= 64, 'more than 64 non-zeros in an input channel'
    for a in (dx, dw, db):
        assert np.array_equal(a, np.round(a))
    assert 0 < np.abs(dx).max() < 256, np.abs(dx).max()
    assert 0 < np.abs(dw).max() < 2 ** 24 and 0 < np.abs(db).max() < 2 ** 24
