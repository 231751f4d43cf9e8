"""The argument envelope of the convolution entry points: its limits, the cases that sit on them and the descriptors beyond them
(tests/test_conv_envelope_cpu.py, tests/test_gpu_conv_envelope.py).

Plain helper module (numpy only).  The kernels carry their small geometry fields in bitfields (csrc/conv_device.h, ConvArgs); LIMITS
is the largest value of each, EDGE holds for every field the smallest shape at which its top bit matters - the far taps land INSIDE
the map, so a kernel that dropped the bit would read other pixels - and REFUSED the first values beyond, which every entry point
answers with RON_ERR_INVALID.  The same numbers stand in include/ron_hip.h (ron_conv_desc), INTEGRATION.md and csrc/conv_mfma.h."""
import numpy as np

import conv_bounds as cb

F64 = np.float64

# inclusive ranges of the descriptor-level quantities
LIMITS = {
    'kh': (1, 15),
    'kw': (1, 15),
    'stride': (1, 7),
    'transposed_kernel': (1, 7),       # conv2d_transpose: kernel == stride
    'dilation': (1, 31),
    'cpad': (0, 63),                   # SAME padding (kh - 1) * dilation / 2
    'relu': (0, 1),
    'pool': (0, 1),
    'transpose': (0, 1),
}

# (n, h, w, cin, cout, k, stride, dilation, transpose)
EDGE = {
    'dil31': (1, 32, 32, 64, 64, 3, 1, 31, 0),       # dil bit 4, cpad 31: pixel 0 reads pixel 31
    'cpad62': (1, 3, 64, 64, 64, 5, 1, 31, 0),       # cpad bit 5, taps at +-31 and +-62 in a 64-wide row
    'cpad63': (1, 3, 64, 64, 64, 7, 1, 21, 0),       # the last value of cpad (7x7 at dilation 21): pixel 0 reads pixel 63
    'cpad32': (2, 5, 40, 64, 24, 5, 1, 16, 0),       # the first value that needs cpad bit 5; cout padded from 24
    'k15': (1, 8, 9, 64, 64, 15, 1, 1, 0),           # kh, kw bit 3: 225 taps, map smaller than the filter
    'k15d4': (1, 30, 16, 64, 64, 15, 1, 4, 0),       # cpad 28 with 15 filter rows
    'k7d9': (2, 28, 28, 64, 128, 7, 1, 9, 0),        # fc6-like halo-row skipping at a large rate
    's7': (2, 14, 21, 64, 64, 7, 7, 1, 0),           # stride bit 2
    'up7': (1, 2, 3, 64, 128, 7, 7, 1, 1),           # up bit 2: the pixel-shuffle epilogue at 49 taps
    'up7res': (1, 2, 3, 64, 128, 7, 7, 1, 1),        # ... with the in-place add of the reverse connection
    # cout 256: the shapes above at a width both taps-innermost tile configurations (7: 256 x 256, 9: 128 x 128) accept; k15 and dil31
    # themselves are 64 wide, which neither does (TAPS_INNER below)
    'dil31n256': (1, 32, 32, 64, 256, 3, 1, 31, 0),
    'k15n256': (1, 8, 9, 64, 256, 15, 1, 1, 0),
}
RESIDUAL = ('up7res',)
BY_SHAPE = ('dil31', 'cpad62', 'cpad63', 'cpad32', 'k15', 'k15d4', 'k7d9', 's7', 'up7', 'up7res')     # run with the by-shape plan, every dtype
SPLITK = ('k15', 'k7d9', 'dil31')                                                           # ... and with forced split-K 1 and 3
# taps-innermost tile configurations ron_conv_plan accepts with splitk = 1 (checked in the dry run): the N tile must divide the padded cout
TAPS_INNER = {'k15': (), 'dil31': (), 'k7d9': (9,), 'dil31n256': (7, 9), 'k15n256': (7, 9)}

# backward: (n, h, w, cin, cout, k, dilation), the format of tests/conv_grad_cases.py
BACKWARD = {
    'dil31': (1, 32, 32, 64, 64, 3, 31),
    'k1d31': (2, 5, 7, 64, 24, 1, 31),       # 1x1: pad 0, the dilation must not matter
}

# the first values beyond each limit: overrides of BASE, the fields of ron_conv_desc
BASE = dict(n=1, h=8, w=8, cin=64, cout=64, kh=3, kw=3, stride=1, dilation=1, relu=1, transpose=0, pool=0)
REFUSED = {
    'dilation 32': dict(h=40, w=40, dilation=32),
    'dilation 64': dict(h=72, w=72, dilation=64),
    '5x5 dilation 32 (cpad 64)': dict(h=8, w=72, kh=5, kw=5, dilation=32),
    '7x7 dilation 22 (cpad 66)': dict(h=8, w=72, kh=7, kw=7, dilation=22),
    '16x16': dict(h=16, w=16, kh=16, kw=16),
    '17x17': dict(h=18, w=18, kh=17, kw=17),
    '8x8 stride 8': dict(h=16, w=16, kh=8, kw=8, stride=8),
    'transposed 8x8 stride 8': dict(h=2, w=2, cout=128, kh=8, kw=8, stride=8, transpose=1),
    'relu 2': dict(relu=2),
    'relu -1': dict(relu=-1),
    'pool 2': dict(pool=2),
    'pool -1': dict(pool=-1),
    'transpose 2': dict(h=2, w=2, cout=128, kh=2, kw=2, stride=2, transpose=2),
    'transpose -1': dict(h=2, w=2, cout=128, kh=2, kw=2, stride=2, transpose=-1),
    'dilation 0': dict(dilation=0),
    'dilation -1': dict(dilation=-1),
    'stride 0': dict(stride=0),
    'stride -1': dict(stride=-1),
    'kh 0': dict(kh=0, kw=0),
    'kh -1': dict(kh=-1, kw=-1),
    'n 0': dict(n=0),
    'h 0': dict(h=0),
    'w 0': dict(w=0),
    'w -1': dict(w=-1),
    'cin 0': dict(cin=0),
    'cin -64': dict(cin=-64),
    'cout 0': dict(cout=0),
    'cout -64': dict(cout=-64),
    # even filters at stride 1: TensorFlow's SAME pads one pixel more behind than in front, the shared halo has one width
    '2x2 stride 1': dict(kh=2, kw=2),
    '4x4 stride 1': dict(kh=4, kw=4),
    # one padding field for both axes
    '3x5': dict(kh=3, kw=5),
}
# the 2x2 stride-2 backward pair keeps its own, stricter checks; beyond them: the flags
REFUSED_K2S2 = {
    'k2s2 relu 2': dict(h=4, w=4, kh=2, kw=2, stride=2, relu=2),
    'k2s2 transpose 2': dict(h=4, w=4, kh=2, kw=2, stride=2, transpose=2),
    'k2s2 pool 2': dict(h=4, w=4, kh=2, kw=2, stride=2, pool=2),
    'k2s2 n 0': dict(n=0, h=4, w=4, kh=2, kw=2, stride=2),
}


def descriptor(over):
    d = dict(BASE)
    d.update(over)
    return d


def edge_descriptor(name):
    n, h, w, cin, cout, k, stride, dilation, transpose = EDGE[name]
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, kh=k, kw=k, stride=stride, dilation=dilation, relu=1, transpose=transpose, pool=0)


# --------------------------------------------------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------------------------------------------------- #
def out_hw(shape):
    n, h, w, cin, cout, k, stride, dilation, transpose = shape
    return (h * stride, w * stride) if transpose else (h // stride, w // stride)


def lattice_deconv_weights(k, cin, cout, seed=0):
    """[k, k, Cout, Cin] for the kernel == stride transposed convolution: each tap is a 1x1 lattice of its own."""
    w = np.zeros((k, k, cout, cin), np.float32)
    for t in range(k * k):
        w[t // k, t % k] = cb.lattice_weights(1, 1, cin, cout, seed=seed + t)[0, 0].T
    return w


def draws(name):
    """How many shifted lattice draws give every (tap, channel) index a non-zero weight in some output channel."""
    n, h, w, cin, cout, k, stride, dilation, transpose = EDGE[name]
    return 1 if transpose else cb.lattice_draws(k, k, cin, cout)


def inputs(kind, name, draw=0):
    """(x, w, bias, residual or None) float32 as the entry points take them; w HWIO, [k, k, Cout, Cin] for a transposed case.

    lattice: x integers in [-2, 2], w in {-1, 0, 1} with at most 64 non-zeros per output channel, integer bias in [-8, 8] and residual
    in [0, 8]: every partial sum is an integer below 2^8 in any order."""
    shape = EDGE[name]
    n, h, w, cin, cout, k, stride, dilation, transpose = shape
    ho, wo = out_hw(shape)
    seed = sum(shape)
    if kind == 'lattice':
        x = cb.lattice_acts((n, h, w, cin), seed)
        wt = lattice_deconv_weights(k, cin, cout, seed) if transpose else cb.lattice_weights(k, k, cin, cout, draw=draw, seed=seed)
        b = cb.lattice_bias(cout, seed)
        res = cb.lattice_residual((n, ho, wo, cout), seed) if name in RESIDUAL else None
    else:
        rs = np.random.RandomState(seed)
        x = rs.randn(n, h, w, cin).astype(np.float32)
        if transpose:
            wt = (rs.randn(k, k, cout, cin) * np.sqrt(2.0 / cin)).astype(np.float32)
        else:
            wt = (rs.randn(k, k, cin, cout) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
        b = (rs.randn(cout) * 0.1).astype(np.float32)
        res = np.maximum(rs.randn(n, ho, wo, cout), 0).astype(np.float32) if name in RESIDUAL else None
    return x, wt, b, res


def one_hot_weights(k, cin, cout, ky, kx):
    """All of the filter's weight in ONE tap: channel c of the input goes to channel c of the output (cin == cout)."""
    assert cin == cout
    w = np.zeros((k, k, cin, cout), np.float32)
    w[ky, kx] = np.eye(cin, dtype=np.float32)
    return w


def shifted(x, k, dilation, ky, kx):
    """What a stride-1 SAME convolution with one_hot_weights(.., ky, kx) returns: x moved by that tap, zeros from the halo."""
    n, h, w, c = x.shape
    p = (k - 1) * dilation // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    return xp[:, ky * dilation: ky * dilation + h, kx * dilation: kx * dilation + w, :]


def reference(name, xs, ws, b, res, relu=True, pool=False):
    """conv_bounds.conv_op of the case on operands as the kernel sees them -> (ref64, S, K)."""
    n, h, w, cin, cout, k, stride, dilation, transpose = EDGE[name]
    return cb.conv_op(xs, ws, b, res, stride=stride, rate=dilation, relu=relu, pool=pool, transpose=bool(transpose))


# --------------------------------------------------------------------------------------------------------------------- #
# mutants: the operation a kernel would run whose field were one bit narrower
# --------------------------------------------------------------------------------------------------------------------- #
def direct64(x, w, step, dilation, pad, kh, kw, ho, wo):
    """out[n, oy, ox] = sum over ky < kh, kx < kw of x[n, oy * step + ky * dilation - pad, ox * step + kx * dilation - pad] @ w[ky, kx],
    zero outside the map: the convolution as the kernel indexes it, every geometry field a parameter of its own."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    n, h, wd, cin = x.shape
    cout = w.shape[3]
    reach_y = max(pad, (ho - 1) * step + (kh - 1) * dilation - pad - (h - 1), 0)
    reach_x = max(pad, (wo - 1) * step + (kw - 1) * dilation - pad - (wd - 1), 0)
    xp = np.pad(x, ((0, 0), (pad, reach_y), (pad, reach_x), (0, 0)))
    out = np.zeros((n * ho * wo, cout), F64)
    for ky in range(kh):
        for kx in range(kw):
            y0, x0 = ky * dilation, kx * dilation            # (+ pad of the padded array - pad of the operation)
            patch = xp[:, y0: y0 + (ho - 1) * step + 1: step, x0: x0 + (wo - 1) * step + 1: step, :]
            out += patch.reshape(-1, cin) @ w[ky, kx]
    return out.reshape(n, ho, wo, cout)


def deconv_taps64(x, w, up, taps):
    """The kernel == stride transposed convolution with only the taps ky, kx < `taps` decoded (the others never stored)."""
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    n, h, wd, cin = x.shape
    cout = w.shape[2]
    out = np.zeros((n, h * up, wd * up, cout), F64)
    flat = x.reshape(-1, cin)
    for ky in range(taps):
        for kx in range(taps):
            out[:, ky::up, kx::up, :] = (flat @ w[ky, kx].T).reshape(n, h, wd, cout)
    return out


MUTANTS = {
    # mutant: (the EDGE case that has to catch it, the wrap)
    'dilation & 15': 'dil31',
    'k & 7': 'k15',
    'stride & 3': 's7',
    'up & 3': 'up7',
    'cpad & 31 (62)': 'cpad62',
    'cpad & 31 (63)': 'cpad63',
    'cpad & 31 (32)': 'cpad32',
    'relu dropped': 'dil31',
    None: None,                  # the operation itself (direct64 must agree with conv_bounds.conv_op)
}


def mutant64(mutant, name, xs, ws, b, res):
    """The float64 result of EDGE[name] (bias, ReLU, residual as conv_bounds.conv_op applies them) under `mutant`; None: unmutated."""
    n, h, w, cin, cout, k, stride, dilation, transpose = EDGE[name]
    relu = mutant != 'relu dropped'
    if transpose:
        y = deconv_taps64(xs, ws, stride, (stride & 3) if mutant == 'up & 3' else stride)
    else:
        ho, wo = out_hw(EDGE[name])
        pad = (k - 1) * dilation // 2 if stride == 1 else 0
        kk, step, dil = k, stride, dilation
        if mutant == 'dilation & 15':
            dil = dilation & 15
        elif mutant == 'k & 7':
            kk = k & 7
        elif mutant == 'stride & 3':
            step = stride & 3
        elif mutant is not None and mutant.startswith('cpad & 31'):
            pad = pad & 31
        y = direct64(xs, ws, step, dil, pad, kk, kk, ho, wo)
    y = y + np.asarray(b, F64)
    if relu:
        y = np.maximum(y, 0)
    if res is not None:
        y = np.maximum(y + np.asarray(res, F64), 0)
    return y
