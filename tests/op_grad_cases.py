"""Cases and inputs of the pool-backward and 2x2 stride-2 convolution-backward tests (tests/test_op_grad_cpu.py,
tests/test_gpu_op_backward.py).  Plain helper module (numpy only): the smallest shapes at which each decision of
ron_maxpool2x2_backward_nhwc and ron_conv2d_k2s2_backward_nhwc can go wrong."""
import numpy as np

import conv_bounds as cb
import conv_grad_cases as cg
import op_grad_ref as ogr

DTYPES = cg.DTYPES
KINDS = cg.KINDS

# ---------------------------------------------------------------------------------------------------------------- the pool: (n, h, w, c)
POOL_CASES = {
    'one': (1, 1, 1, 8),            # a window of one element
    'window': (1, 2, 2, 8),         # one full window
    'odd': (2, 5, 7, 8),            # odd in both axes, two images: nothing crosses rows or images
    'c72': (1, 4, 6, 72),           # channels not a multiple of 64
    'oddrows': (2, 9, 8, 64),       # odd rows, even columns
    'wide': (1, 38, 38, 512),       # a whole-network width, more lanes than one workgroup
}
POOL_KINDS = ('gauss', 'relu')


def pool_inputs(kind, case, seed=0):
    """(x, dy) float32: x Gaussian ('gauss') or relu(Gaussian) ('relu': half of it exact zeros, so whole windows tie), dy Gaussian."""
    n, h, w, c = POOL_CASES[case]
    rs = np.random.RandomState(300 + seed)
    x = rs.randn(n, h, w, c).astype(np.float32)
    if kind == 'relu':
        x = np.maximum(x, 0)
    dy = rs.randn(n, (h + 1) // 2, (w + 1) // 2, c).astype(np.float32)
    return x, dy


def assert_pool_ties(dtype, seed=0):
    """The relu(gauss) inputs of this seed hold, over the cases, four-way ties and two-way ties of the maximum whose first member is
    not position (0,0): the windows at which 'first maximum' differs from every other choice."""
    four = two = 0
    for case in POOL_CASES:
        a, b = ogr.pool_ties(pool_inputs('relu', case, seed)[0], dtype)
        four, two = four + a, two + b
    assert four >= 1 and two >= 1, (dtype, four, two)
    return four, two


# one window per image, positions in window order; `want` = the position that takes the gradient
_D = np.float32(2.0 ** -12)         # 1 + 2^-12 rounds to 1 in bf16 and in fp16
POOL_HAND = (
    ('all equal', (3.0, 3.0, 3.0, 3.0), 0),
    ('tie at 1 and 2', (1.0, 5.0, 5.0, 2.0), 1),
    ('tie only after rounding, the later value larger in fp32', (0.5, 1.0, 0.25, np.float32(1.0) + _D), 1),
    ('-0.0 against +0.0', (-1.0, -0.0, 0.0, -2.0), 1),
    ('+0.0 against -0.0', (-1.0, -3.0, 0.0, -0.0), 2),
    ('all negative', (-3.0, -1.0, -2.0, -4.0), 1),
)


def pool_hand_inputs():
    """(x [6,2,2,8], dy [6,1,1,8], want [6]): the hand windows, the same in all 8 channels, dy distinct per element."""
    x = np.zeros((len(POOL_HAND), 2, 2, 8), np.float32)
    for i, (_, vals, _) in enumerate(POOL_HAND):
        x[i] = np.asarray(vals, np.float32).reshape(2, 2, 1)
    dy = (np.arange(len(POOL_HAND) * 8, dtype=np.float32).reshape(-1, 1, 1, 8) + 1) * np.float32(0.25)
    return x, dy, np.array([w for _, _, w in POOL_HAND])


# ------------------------------------------------------------------------------------------------- k2s2: (n, h, w, cin, cout, transpose)
K2S2_CASES = {
    'c_one': (1, 2, 2, 64, 64, 0),            # one window
    'c_k30': (2, 6, 10, 64, 24, 0),           # 30 output pixels, fewer than one K step; padded cout
    'c_126': (3, 4, 4, 128, 126, 0),          # cout one short of the 128-wide tile
    'c_tiles': (1, 10, 10, 320, 192, 0),      # several tiles with a partial one
    'c_split': (2, 40, 40, 64, 64, 0),        # enough pixels for the by-shape split
    't_one': (1, 1, 1, 64, 64, 1),            # a single input pixel
    't_k30': (2, 3, 5, 64, 128, 1),           # odd non-square map, 30 input pixels, fewer than one K step
    't_192': (3, 2, 2, 192, 64, 1),           # cin 192 not a multiple of 128, three images
    't_net': (1, 20, 20, 512, 512, 1),        # the network's own last deconvolution at batch 1
    't_split': (2, 19, 19, 128, 64, 1),       # odd map, split regime
}


def k2s2_shapes(case):
    """(x shape, w shape, dy shape)"""
    n, h, w, cin, cout, tr = K2S2_CASES[case]
    if tr:
        return (n, h, w, cin), (2, 2, cout, cin), (n, 2 * h, 2 * w, cout)
    return (n, h, w, cin), (2, 2, cin, cout), (n, h // 2, w // 2, cout)


def k2s2_inputs(kind, case, seed=0):
    """(x, w, y, dy) float32 in the layouts of the entry point, following conv_grad_cases.inputs.

    lattice: x, dy integers in [-2, 2]; y = relu(integers in [-1, 3]), 40 % exact zeros; w in {-1, 0, 1} with at most 64 non-zeros
    per INPUT channel over all taps and output channels, so at most 64 non-zeros enter any dx sum: |dx| <= 2 * 64."""
    cin, cout, tr = K2S2_CASES[case][3:]
    xshape, wshape, yshape = k2s2_shapes(case)
    rs = np.random.RandomState(200 + seed)
    if kind == 'lattice':
        x = rs.randint(-2, 3, size=xshape).astype(np.float32)
        dy = rs.randint(-2, 3, size=yshape).astype(np.float32)
        y = np.maximum(rs.randint(-1, 4, size=yshape), 0).astype(np.float32)
        wt = cb.lattice_weights(2, 2, cout, cin, seed=seed)          # [2,2,cout,cin]: <= 64 non-zeros per cin
        if not tr:
            wt = np.ascontiguousarray(wt.transpose(0, 1, 3, 2))
    else:
        x = rs.randn(*xshape).astype(np.float32)
        dy = rs.randn(*yshape).astype(np.float32)
        y = np.maximum(rs.randn(*yshape), 0).astype(np.float32)
        wt = (rs.randn(*wshape) * np.sqrt(2.0 / ((1 if tr else 4) * cin))).astype(np.float32)
    return x, wt, y, dy


def k2s2_assert_lattice(case, w, g):
    """conv_grad_cases.assert_lattice on the weights seen as HWIO with the INPUT channel on axis 2."""
    hwio = w.transpose(0, 1, 3, 2) if K2S2_CASES[case][5] else w
    cg.assert_lattice(hwio, g['dx'][0], g['dw'][0], g['db'][0])
