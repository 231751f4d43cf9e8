"""Cases and inputs of the SSD-backward tests (tests/test_ssd_grad_cpu.py, tests/test_gpu_ssd_backward.py).

Plain helper module (numpy only): the smallest shapes at which each decision of ron_maxpool3x3s1_backward_nhwc,
ron_l2norm_backward_nhwc and ron_conv2d_padded_backward_nhwc can go wrong."""
import numpy as np

import conv_grad_cases as cg
import ssd_grad_ref as sr

DTYPES = ('bf16', 'fp16')
KINDS = ('lattice', 'gauss')

# --------------------------------------------------------------------------------------------------------------------- the pool
POOL_CASES = {              # (n, h, w, c)
    'one': (1, 1, 1, 8),           # every window is the position itself
    'two': (1, 2, 2, 8),           # every window is the whole map
    'rows': (2, 3, 5, 8),          # two images: a window must not reach the next one
    'odd': (2, 7, 6, 16),
    'c72': (1, 4, 4, 72),          # 18 groups of 4 channels: lanes of one pixel straddle a wave
    'pool5': (1, 19, 19, 512),     # pool5 of SSD-300: more than one block
    'c64': (2, 5, 9, 64),          # two images, odd sides, a pixel's lanes fill a quarter of a workgroup
}
POOL_KINDS = ('gauss', 'relu', 'coarse')


def pool_inputs(kind, case):
    """(x, dy) float32: Gaussian x (negative borders, hardly a tie), relu(Gaussian) (half of it exact zeros: all-zero windows, and
    maxima that collide after rounding on the larger maps) or 'coarse', relu(Gaussian) in steps of 1/2: tied maxima in every case,
    most of them not at their window's first position."""
    shape = POOL_CASES[case]
    rs = np.random.RandomState(300 + sorted(POOL_CASES).index(case))
    x = rs.randn(*shape).astype(np.float32)
    if kind != 'gauss':
        x = np.maximum(x, 0)
    if kind == 'coarse':
        x = (np.round(x * 2) / 2).astype(np.float32)
    return x, rs.randn(*shape).astype(np.float32)


# hand windows on a 3x3 map of 8 channels: (label, the nine values row-major, the window (oy, ox) that carries dy, the position that gets it)
POOL_HAND = (
    ('all equal', [1.0] * 9, (1, 1), (0, 0)),
    # 1 + 2^-12 rounds to 1 in bf16 and fp16: a tie after rounding, the later value larger in float32
    ('tie after rounding', [0.0, 1.0, 1.0 + 2.0 ** -12, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], (1, 1), (0, 1)),
    ('-0.0 against +0.0', [-1.0, -0.0, -1.0, -1.0, 0.0, -1.0, -1.0, -1.0, -1.0], (1, 1), (0, 1)),
    # the corner window holds (0,0) (0,1) (1,0) (1,1) only: its maximum is negative, the padding is not a zero
    ('all negative at a corner', [-3.0, -2.0, -5.0, -1.0, -4.0, -5.0, -5.0, -5.0, -5.0], (0, 0), (1, 0)),
)


def pool_hand_inputs():
    """(x [4,3,3,8], dy [4,3,3,8]): one image per hand window; dy = 1 .. 8 over the channels at the one window, 0 elsewhere."""
    x = np.stack([np.repeat(np.asarray(v, np.float32).reshape(3, 3, 1), 8, axis=2) for _, v, _, _ in POOL_HAND])
    dy = np.zeros_like(x)
    for i, (_, _, (oy, ox), _) in enumerate(POOL_HAND):
        dy[i, oy, ox] = np.arange(1, 9, dtype=np.float32)
    return x, dy


def pool_hand_expected():
    dx = np.zeros((len(POOL_HAND), 3, 3, 8), np.float32)
    for i, (_, _, _, (r, q)) in enumerate(POOL_HAND):
        dx[i, r, q] = np.arange(1, 9, dtype=np.float32)
    return dx


# --------------------------------------------------------------------------------------------------------- the L2 normalisation
L2_PIXELS = {1: (1, 1, 1), 3: (1, 1, 3), 4: (1, 2, 2), 5: (1, 5, 1), 257: (1, 1, 257), 38 * 38: (1, 38, 38)}
L2_CASES = {'m%d_c%d' % (m, c): nhw + (c,) for m, nhw in L2_PIXELS.items() for c in (8, 72, 512)}
# the partial-sum table has min(M, 2048) rows: M = 1 above gives it one row; these give it its full height, with a wave that walks
# two pixels and waves that walk one (2049), and with every wave walking three or two (4100)
L2_CASES['m2049_c8'] = (1, 3, 683, 8)
L2_CASES['m4100_c16'] = (2, 50, 41, 16)


def l2_inputs(kind, case, seed=0):
    """(x, gamma, dy) float32.  gauss: x = relu(Gaussian) + a few negative values, gamma in [1, 20] (SSD initialises it to 20).
    lattice: every pixel holds 4 or 16 entries of +-1 or one entry of +-2 (inv = 0.5 or 0.25 exactly), gamma in {1, 2}, dy in
    {-1, 0, 1}: dx and dgamma are exact in float32, bf16 and fp16 in any summation order (l2_assert_lattice)."""
    n, h, w, c = L2_CASES[case] if isinstance(case, str) else case
    rs = np.random.RandomState(500 + seed)
    if kind == 'gauss':
        x = rs.randn(n, h, w, c).astype(np.float32)
        x = np.where(rs.rand(n, h, w, c) < 0.8, np.maximum(x, 0), x).astype(np.float32)
        x[..., 0] = np.abs(x[..., 0]) + 0.125          # no pixel is all zero by accident: the clamped branch has its own case
        return x, rs.uniform(1.0, 20.0, size=c).astype(np.float32), rs.randn(n, h, w, c).astype(np.float32)
    m = n * h * w
    x = np.zeros((m, c), np.float32)
    for p in range(m):
        kind_p = rs.randint(3) if c >= 16 else rs.choice([0, 2])
        count = (4, 16, 1)[kind_p]
        idx = rs.choice(c, size=count, replace=False)
        x[p, idx] = rs.choice([-1.0, 1.0], size=count) * (2.0 if count == 1 else 1.0)
    gamma = rs.choice([1.0, 2.0], size=c).astype(np.float32)
    dy = rs.randint(-1, 2, size=(n, h, w, c)).astype(np.float32)
    return x.reshape(n, h, w, c), gamma, dy


def l2_assert_lattice(x, gamma, dy):
    """The conditions that make the lattice exact: ss in {4, 16}, so inv and u are powers of two; every product and partial sum a
    multiple of 1/16 below 2^7 for dx (8 significant bits: a bf16 holds it) and a multiple of 1/4 below 2^24 for dgamma."""
    ss = (x.astype(np.float64) ** 2).sum(axis=-1)
    assert set(np.unique(ss)) <= {4.0, 16.0}
    assert set(np.unique(gamma)) <= {1.0, 2.0} and set(np.unique(dy)) <= {-1.0, 0.0, 1.0}
    ref = sr.l2_backward64(x, gamma, dy)
    for dtype in DTYPES:
        d = sr.l2_deliver(ref, dtype)
        assert np.array_equal(d['dx'], ref['dx']) and np.array_equal(d['dgamma'], ref['dgamma'])
    assert np.array_equal(ref['dx'] * 64, np.round(ref['dx'] * 64)) and np.abs(ref['dx']).max() < 4
    assert np.array_equal(ref['dgamma'] * 4, np.round(ref['dgamma'] * 4))
    return ref


def l2_dead_pixel_inputs(c=72):
    """(1, 1, 5, c) gauss inputs whose pixel 1 is all zero (post-ReLU) and whose pixel 3 holds nothing but 2^-21 in two channels
    (ss = 2^-41 < 1e-12 with u far from zero): the clamped branch between live pixels.  Their dy is scaled by 2^-10 so that
    dy gamma 1e6 stays inside fp16."""
    x, gamma, dy = l2_inputs('gauss', (1, 1, 5, c), seed=3)
    x[0, 0, 1] = 0
    x[0, 0, 3] = 0
    x[0, 0, 3, 2:4] = 2.0 ** -21
    dy[0, 0, 1] *= 2.0 ** -10
    dy[0, 0, 3] *= 2.0 ** -10
    return x, gamma, dy


# ------------------------------------------------------------------------------------------------------- the padded convolutions
PADDED_CASES = {            # (n, h, w, cin, cout, stride, cpad)
    's2_3x3': (1, 3, 3, 64, 64, 2, 1),
    's2_5x4': (2, 5, 4, 64, 128, 2, 1),        # odd rows, even columns, two images
    's2_2x2': (1, 2, 2, 128, 256, 2, 1),       # one output pixel, three input pixels it never samples
    's2_1x1': (1, 1, 1, 64, 64, 2, 1),
    's2_19': (1, 19, 19, 256, 512, 2, 1),      # block8 of SSD-300
    'v_5x5': (1, 5, 5, 128, 256, 1, 0),        # block10 of SSD-300
    'v_3x3': (2, 3, 3, 128, 256, 1, 0),        # block11 of SSD-300: one output pixel per image
}


def padded_inputs(kind, case, seed=0):
    """(x, w, y, dy): conv_grad_cases.inputs of the full-resolution problem, y and dy sampled down to [n,ho,wo,cout]."""
    n, h, w, cin, cout, stride, cpad = PADDED_CASES[case]
    x, wt, y, dy = cg.inputs(kind, (n, h, w, cin, cout, 3, 1), seed=seed)
    ho, wo = sr.out_hw(h, w, stride, cpad)
    o = 1 - cpad
    pick = lambda a: np.ascontiguousarray(a[:, o::stride, o::stride][:, :ho, :wo])
    return x, wt, pick(y), pick(dy)


def padded_reference(kind, case, dtype, relu):
    n, h, w, cin, cout, stride, cpad = PADDED_CASES[case]
    x, wt, y, dy = padded_inputs(kind, case)
    g = sr.grads64_padded(*sr.cgr.seen(x, wt, y, dy, dtype, relu), stride, cpad)
    if kind == 'lattice':
        padded_assert_lattice(wt, g)
    return (x, wt, y, dy), g


def padded_assert_lattice(w, g):
    """conv_grad_cases.assert_lattice, except that a gradient may be all zero where the case has a single output pixel."""
    assert set(np.unique(w)) <= {-1.0, 0.0, 1.0}
    assert (w != 0).sum(axis=(0, 1, 3)).max() <= 64
    for name in ('dx', 'dw', 'db'):
        a = g[name][0]
        assert np.array_equal(a, np.round(a))
    assert np.abs(g['dx'][0]).max() < 256 and np.abs(g['dw'][0]).max() < 2 ** 24 and np.abs(g['db'][0]).max() < 2 ** 24
    assert np.abs(g['dx'][0]).max() > 0 and np.abs(g['dw'][0]).max() > 0


def block12_inputs(kind, seed=0):
    """(x [1,2,2,64], w [4,4,64,128], y, dy [1,1,1,128]) of pad2d(1) + 4x4 VALID on a 2x2 map (block12 of SSD-512, narrower)."""
    rs = np.random.RandomState(700 + seed)
    cin, cout = 64, 128
    if kind == 'lattice':
        x = rs.randint(-2, 3, size=(1, 2, 2, cin)).astype(np.float32)
        w = rs.choice([-1.0, 0.0, 0.0, 1.0], size=(4, 4, cin, cout)).astype(np.float32)
        y = np.maximum(rs.randint(-1, 4, size=(1, 1, 1, cout)), 0).astype(np.float32)
        dy = rs.randint(-2, 3, size=(1, 1, 1, cout)).astype(np.float32)
    else:
        x = rs.randn(1, 2, 2, cin).astype(np.float32)
        w = (rs.randn(4, 4, cin, cout) * np.sqrt(2.0 / (16 * cin))).astype(np.float32)
        y = np.maximum(rs.randn(1, 1, 1, cout), 0).astype(np.float32)
        dy = rs.randn(1, 1, 1, cout).astype(np.float32)
    return x, w, y, dy


def block12_grads64(xs, ws, dz):
    """{'dx', 'dw', 'db': (ref64, S, K)} of the padded 4x4 convolution, written out: y[co] = sum xs[r, q, ci] ws[r + 1, q + 1, ci, co]."""
    xs, ws, dz = (np.asarray(a, np.float64) for a in (xs, ws, dz))

    def run(x_, w_, z_):
        zz = z_.reshape(-1)
        dx = np.einsum('rqio,o->rqi', w_[1:3, 1:3], zz)[None]
        dw = np.zeros_like(w_)
        dw[1:3, 1:3] = np.einsum('rqi,o->rqio', x_[0], zz)
        return dx, dw, zz.copy()
    ref = run(xs, ws, dz)
    mag = run(np.abs(xs), np.abs(ws), np.abs(dz))
    return {name: (r, s, k) for name, r, s, k in zip(('dx', 'dw', 'db'), ref, mag, (ws.shape[3], 1, 1))}
