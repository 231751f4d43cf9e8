"""Cases and inputs of the head-chain tests (tests/test_head_chain_cpu.py, tests/test_gpu_head_chain.py).

Plain helper module (numpy only).  A case is ((n, h, w, cin), layers); a layer is ('c', k, dilation, cout, relu, bias, tap), ('p',),
('b', relu) - training-mode batch normalisation with bn_cases.EPS / DECAY - or ('2', cout, cout2, relu, bias), the two-branch
3x3 | 1x1 convolution.  The smallest shapes at which each decision of ron_head_chain_forward / ron_head_chain_backward can go wrong."""
import numpy as np

import bn_cases as bc
from conv_chain_cases import P, c


def b(relu=1):
    return ('b', relu)


def pair(cout, cout2, relu=0, bias=1):
    return ('2', cout, cout2, relu, bias)


CASES = {
    # _objectness + _objectness_score.  M = 120 with c = 64: two slices at 16 lanes per row
    'objness': ((2, 6, 10, 64), [c(3, 64, relu=0, bias=0), b(), c(3, 12, relu=0)]),
    # pred_cls_module.  Concat widths 128 and 192 (a partly filled channel tile of the statistics), the gradient split at channels 64
    # and 128, a pair as the first layer (dx = the fp32 sum of two data gradients), a pair behind a BN
    'cls': ((2, 6, 10, 64), [pair(64, 64), b(), pair(128, 64), b(), c(3, 18, relu=0)]),
    # _conv_left: BN last; odd M = 105
    'left': ((3, 5, 7, 64), [c(3, 64, relu=0, bias=0), b()]),
    # BN first (x enters through the halo pack), without ReLU, in front of a 1x1 (a halo-0 consumer)
    'bnfirst': ((2, 4, 4, 128), [b(0), c(1, 64)]),
    # BN behind a pool, a pool behind a BN, BN behind a BN
    'bnpool': ((2, 9, 6, 64), [c(3, 64), P, b(), P, b(0)]),
    # a pair as the last layer (dy enters its two joins as channel slices of a dense tensor), behind a ReLU layer
    'pairlast': ((1, 4, 4, 64), [c(3, 64), pair(64, 64, relu=1)]),
    # the geometry of the real heads' statistics: c = 512 is 64 lanes per row, 4 rows per workgroup; M = 9 is below 4 workgroup rows
    'wide': ((1, 3, 3, 64), [c(1, 512, relu=0, bias=0), b(), c(1, 8)]),
}
# a single BN for the shapes of the batch-normalisation tests: the chain must equal the per-operator entry points
BN1 = {'bn1_%s' % name: (shape, [b()]) for name, shape in bc.SHAPES.items()}
DTYPES = ('bf16', 'fp16')


def _case(case):
    if not isinstance(case, str):
        return case
    return CASES[case] if case in CASES else BN1[case]


def shapes(case):
    """[(n, h, w, c) of every layer's output]"""
    (n, h, w, ch), layers = _case(case)
    out = []
    for l in layers:
        if l == P:
            h, w = (h + 1) // 2, (w + 1) // 2
        elif l[0] == 'c':
            ch = l[3]
        elif l[0] == '2':
            ch = l[1] + l[2]
        out.append((n, h, w, ch))
    return out


def layer_dicts(case):
    """The layer list in the form ops.head_chain_* take"""
    _, layers = _case(case)
    out = []
    for l in layers:
        if l == P:
            out.append({'kind': 'pool', 'tap': False})
        elif l[0] == 'c':
            out.append({'kind': 'conv', 'k': l[1], 'dilation': l[2], 'cout': l[3], 'relu': bool(l[4]), 'bias': bool(l[5]), 'tap': bool(l[6])})
        elif l[0] == 'b':
            out.append({'kind': 'bn', 'relu': bool(l[1]), 'eps': bc.EPS, 'decay': bc.DECAY, 'tap': False})
        else:
            out.append({'kind': 'pair', 'cout': l[1], 'cout2': l[2], 'relu': bool(l[3]), 'bias': bool(l[4]), 'tap': False})
    return out


def inputs(case, seed=0):
    """(x, params, dy) float32: x and dy N(0, 1) and He-scaled weights with biases of about 0.1 as in conv_chain_cases.inputs; gamma
    about 1 +- 0.2, beta about +- 0.1, moving statistics that are not (0, 1).  params has one dict per layer (None for pools) with
    'w', 'bias', 'w2', 'bias2', 'gamma', 'beta', 'moving_mean', 'moving_var' as the layer's kind has them."""
    (n, h, w, ch), layers = _case(case)
    rs = np.random.RandomState(700 + seed)
    f = np.float32
    x = rs.randn(n, h, w, ch).astype(f)
    params = []
    for l in layers:
        if l == P:
            params.append(None)
        elif l[0] == 'c':
            _, k, rate, cout, relu, bias, tap = l
            p = {'w': (rs.randn(k, k, ch, cout) * np.sqrt(2.0 / (k * k * ch))).astype(f)}
            if bias:
                p['bias'] = (rs.randn(cout) * 0.1).astype(f)
            params.append(p)
            ch = cout
        elif l[0] == '2':
            _, cout, cout2, relu, bias = l
            p = {'w': (rs.randn(3, 3, ch, cout) * np.sqrt(2.0 / (9 * ch))).astype(f), 'w2': (rs.randn(1, 1, ch, cout2) * np.sqrt(2.0 / ch)).astype(f)}
            if bias:
                p['bias'] = (rs.randn(cout) * 0.1).astype(f)
                p['bias2'] = (rs.randn(cout2) * 0.1).astype(f)
            params.append(p)
            ch = cout + cout2
        else:
            params.append({'gamma': (1.0 + 0.2 * rs.uniform(-1, 1, ch)).astype(f), 'beta': (0.1 * rs.uniform(-1, 1, ch)).astype(f),
                           'moving_mean': rs.randn(ch).astype(f), 'moving_var': (np.abs(rs.randn(ch)) + 0.5).astype(f)})
    dy = rs.randn(*shapes(case)[-1]).astype(f)
    return x, params, dy
