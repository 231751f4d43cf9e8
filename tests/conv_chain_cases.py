"""Cases and inputs of the convolution-chain tests (tests/test_conv_chain_cpu.py, tests/test_gpu_conv_chain.py).

Plain helper module (numpy only).  A case is ((n, h, w, cin), layers); a layer is ('c', k, dilation, cout, relu, bias, tap) or
('p',).  The smallest shapes at which each decision of ron_conv_chain_forward / ron_conv_chain_backward can go wrong."""
import numpy as np

import conv_grad_cases as cg


def c(k, cout, dilation=1, relu=1, bias=1, tap=0):
    return ('c', k, dilation, cout, relu, bias, tap)


P = ('p',)

_MINI = [c(3, 64), c(3, 64, tap=1), P, c(3, 128), P, c(3, 192, dilation=3, tap=1), c(1, 65, relu=0)]

CASES = {
    # paddings 1 -> 3 -> 0: both re-halo directions; a tap in front of a pool; a last cout that is no multiple of 64
    'mini': ((2, 12, 20, 64), _MINI),
    # odd pools (5 x 7 -> 3 x 4 -> 2 x 2), the 7 x 7 route with the filter overhanging the map, three images
    'odd': ((3, 5, 7, 64), [c(3, 64), P, c(7, 64, tap=1), P, c(1, 24)]),
    # a pool first, a pool last, two pools in a row, a pool behind a convolution without ReLU
    'pools': ((2, 9, 6, 128), [P, P, c(3, 64, relu=0), P]),
    # `mini` with a tap on every convolution (dtaps are given for every second one only: DTAPS_GIVEN)
    'alltaps': ((2, 12, 20, 64), [l if l == P else l[:6] + (1,) for l in _MINI]),
}
# a single convolution for each case of the convolution-backward tests: the chain must equal the per-operator entry points
ONE = {'one%s' % name: ((n, h, w, cin), [c(k, cout, dilation=rate)]) for name, (n, h, w, cin, cout, k, rate) in cg.CASES.items()}
CASES.update(ONE)
DTYPES = ('bf16', 'fp16')


def dtap_given(case, layer):
    """Whether the tests hand the backward a gradient for this tap: every tap, except in `alltaps` every second tapped layer only."""
    if case != 'alltaps':
        return True
    tapped = [i for i, l in enumerate(CASES[case][1]) if l != P and l[6]]
    return tapped.index(layer) % 2 == 0


def shapes(case):
    """[(n, h, w, c) of every layer's output]"""
    (n, h, w, ch), layers = CASES[case] if isinstance(case, str) else case
    out = []
    for l in layers:
        if l == P:
            h, w = (h + 1) // 2, (w + 1) // 2
        else:
            ch = l[3]
        out.append((n, h, w, ch))
    return out


def layer_dicts(case):
    """The layer list in the form ops.conv_chain_* take"""
    _, layers = CASES[case] if isinstance(case, str) else case
    return [{'kind': 'pool', 'tap': False} if l == P else
            {'kind': 'conv', 'k': l[1], 'dilation': l[2], 'cout': l[3], 'relu': bool(l[4]), 'bias': bool(l[5]), 'tap': bool(l[6])} for l in layers]


def inputs(case, seed=0):
    """(x, weights, biases, dy, dtaps) float32, gauss as in conv_fwd_cases.inputs: N(0, 1) activations and gradients, He-scaled
    weights, biases of about 0.1; weights / biases / dtaps have one entry per layer (None for pools, layers without a bias, and taps
    that are absent or not given)."""
    (n, h, w, ch), layers = CASES[case] if isinstance(case, str) else case
    rs = np.random.RandomState(500 + seed)
    x = rs.randn(n, h, w, ch).astype(np.float32)
    ws, bs, dtaps = [], [], []
    out = shapes(case)
    for i, l in enumerate(layers):
        if l == P:
            ws.append(None); bs.append(None); dtaps.append(None)
            continue
        _, k, rate, cout, relu, bias, tap = l
        ws.append((rs.randn(k, k, ch, cout) * np.sqrt(2.0 / (k * k * ch))).astype(np.float32))
        bs.append((rs.randn(cout) * 0.1).astype(np.float32) if bias else None)
        given = tap and (not isinstance(case, str) or dtap_given(case, i))
        dtaps.append(rs.randn(*out[i]).astype(np.float32) if given else None)
        ch = cout
    dy = rs.randn(*out[-1]).astype(np.float32)
    return x, ws, bs, dy, dtaps
