"""The cases of the batch-normalisation tests (tests/test_bn_cpu.py, tests/test_gpu_batchnorm.py): shapes, inputs and the mutant table.

Shapes are the smallest at which each mechanism of csrc/batchnorm.hip can go wrong, not the workload's: with bn_ref.geometry, M one
below, at and one above the rows of a wave, of a workgroup and of a slice, and just above two slices with a ragged tail, for c = 8
(2 lanes per row, 128 rows per workgroup), c = 72 (18 of 32 lanes hold channels) and c = 1024 (4 channel tiles); M = 1 (variance 0,
Bessel factor max(M - 1, 1)) and M = 2; the network's coarsest map (2 x 5 x 5 x 512, odd) and 2 x 40 x 40 x 512 (200 slices).

Kinds of inputs:
  gauss     x = N(m_c, s_c) per channel, gamma of both signs, dy = N(0, 1): graded by the bounds of bn_ref
  tiny      gauss with x scaled by 2^-8: var is of the size of eps, so where eps enters matters
  lattice   M a power of two, eps = 0, every channel holds +a and -a in equal number (a a power of two), gamma, beta, dy small
            integers: every count in the merge tree is a power of two, so mean = 0, var = a^2, rstd = 1 / a, xhat = +-1, y, dbeta,
            dgamma and the float32 value of dx are exact - the outputs must EQUAL the reference
  offset    fp16 values 2048 + 2 {-1, 0, 1} / bf16 values 256 + 2 {-1, 0, 1}, M = 4096: a float32 E[x^2] - mean^2 loses the variance
"""
import numpy as np

import bn_ref as br

DTYPES = ('bf16', 'fp16')
EPS, DECAY = 1e-5, 0.997          # ron_arg_scope's


def _shapes():
    out = {'m1': (1, 1, 1, 8), 'm2': (1, 1, 2, 8), 'coarse': (2, 5, 5, 512), 'scale40': (2, 40, 40, 512)}
    for c in (8, 72, 1024):
        g = br.geometry(1, 1, 1, c)
        marks = {1, 2, 2 * g['slice_rows'] + 3}
        for unit in (g['rows_per_wave'], g['rpb'], g['slice_rows']):
            marks |= {unit - 1, unit, unit + 1}
        for m in sorted(v for v in marks if v >= 1):
            out['c%d_m%d' % (c, m)] = (1, 1, m, c)
    return out


SHAPES = _shapes()
LATTICE = {'l_c8_m8': (1, 1, 8, 8), 'l_c8_m1024': (1, 32, 32, 8), 'l_c72_m64': (1, 8, 8, 72), 'l_c1024_m32': (2, 4, 4, 1024)}
OFFSET_SHAPE = (1, 64, 64, 8)
OFFSET_BASE = {'fp16': 2048.0, 'bf16': 256.0}


def _rs(shape, salt=0):
    return np.random.RandomState((sum(shape) * 7919 + shape[3] * 31 + shape[2] + salt) % (2 ** 31))


def inputs(kind, shape, dtype='bf16'):
    """dict(x, gamma, beta, dy, moving_mean, moving_var, eps) of float32 arrays; x and dy already hold storage-type values only for
    the lattice and offset kinds (the others are rounded by the operator)."""
    n, h, w, c = shape
    rs = _rs(shape)
    f = np.float32
    if kind in ('gauss', 'tiny'):
        x = (rs.randn(*shape) * (0.5 + rs.rand(c)) + rs.randn(c)).astype(f)
        if kind == 'tiny':
            x = x * f(2.0 ** -8)
        return dict(x=x, gamma=(rs.randn(c) * 0.5 + np.where(rs.rand(c) < 0.8, 1.0, -1.0)).astype(f), beta=(rs.randn(c) * 0.3).astype(f),
                    dy=rs.randn(*shape).astype(f), moving_mean=rs.randn(c).astype(f), moving_var=(np.abs(rs.randn(c)) + 0.5).astype(f), eps=EPS)
    m = n * h * w
    if kind == 'lattice':
        assert m & (m - 1) == 0 and m >= 2
        a = 2.0 ** (np.arange(c) % 4 - 1)
        sign = np.stack([rs.permutation(np.repeat([1.0, -1.0], m // 2)) for _ in range(c)], axis=1)
        return dict(x=(sign * a).reshape(shape).astype(f), gamma=rs.choice([-2.0, -1.0, 1.0, 2.0, 3.0], size=c).astype(f),
                    beta=rs.randint(-2, 3, size=c).astype(f), dy=rs.randint(-3, 4, size=shape).astype(f),
                    moving_mean=rs.randint(-4, 5, size=c).astype(f), moving_var=rs.randint(1, 5, size=c).astype(f), eps=0.0)
    assert kind == 'offset'
    x = (OFFSET_BASE[dtype] + 2.0 * rs.randint(-1, 2, size=shape)).astype(f)
    assert np.array_equal(br.ROUND[dtype](x), x)
    return dict(x=x, gamma=np.ones(c, f), beta=np.zeros(c, f), dy=rs.randn(*shape).astype(f), moving_mean=np.zeros(c, f),
                moving_var=np.ones(c, f), eps=EPS)


def assert_lattice(given, fwd, bwd):
    """The conditions that make the lattice outputs exact: the float64 results are float32 values."""
    c = given['x'].shape[-1]
    assert not fwd['mean'].any() and np.array_equal(fwd['var'], (2.0 ** (np.arange(c) % 4 - 1)) ** 2)
    assert set(np.unique(np.abs(fwd['xhat']))) == {1.0}
    for name, a in (('y', fwd['y']), ('dbeta', bwd['dbeta']), ('dgamma', bwd['dgamma']), ('dx', bwd['dx'])):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), name
    assert bwd['dbeta'].any() and bwd['dgamma'].any() and bwd['dx'].any()


# --------------------------------------------------------------------------------------------------------------------- the mutants
# name -> (the case that rejects it: kind, shape name or shape, relu), in the order of the issue's table
MUTANTS = {
    'moving_var_biased': ('gauss', 'm2', 1),
    'normalise_unbiased': ('gauss', 'm2', 0),
    'decay_as_momentum': ('gauss', 'c72_m9', 1),
    'eps_outside_sqrt': ('tiny', 'c72_m33', 0),
    'mask_dy': ('gauss', 'c72_m67', 1),
    'mask_dropped': ('gauss', 'c72_m67', 1),
    'dz_unrounded': ('gauss', 'c72_m67', 1),
    'dbeta_term_dropped': ('gauss', 'c72_m67', 1),
    'dgamma_term_dropped': ('gauss', 'c72_m67', 1),
    'y_unrounded': ('gauss', 'c72_m33', 1),
    'last_slice_dropped': ('gauss', 'c72_m67', 1),
    'naive_variance': ('offset', OFFSET_SHAPE, 0),
}


def run64(given, dtype, relu, mutant=None, decay=DECAY):
    """What the operator pair delivers, computed in float64 (float32 where the mutant is about float32) from the definitions, or with
    one `mutant` of MUTANTS: dict(y, mean, var, moving_mean, moving_var, dx, dgamma, dbeta), the backward on the forward's own y, mean
    and var."""
    rnd = br.ROUND[dtype]
    xs = rnd(given['x'])
    eps, ga, be = given['eps'], given['gamma'], given['beta']
    fwd = br.forward64(xs, ga, be, relu, eps)
    rows = fwd['rows']
    mean, var = fwd['mean'], fwd['var']
    if mutant == 'naive_variance':
        mean, var = (a.astype(np.float64) for a in br.stats_emulate32(xs, order='naive'))
    if mutant == 'last_slice_dropped':
        mean, var = (a.astype(np.float64) for a in br.stats_emulate32(xs, drop_last_slice=True))
    norm_var = var * rows / max(rows - 1, 1) if mutant == 'normalise_unbiased' else var
    rstd = 1.0 / (np.sqrt(norm_var) + eps) if mutant == 'eps_outside_sqrt' else 1.0 / np.sqrt(norm_var + np.float64(np.float32(eps)))
    v = ga.astype(np.float64) * ((xs.astype(np.float64) - mean) * rstd) + be
    y64 = np.maximum(v, 0) if relu else v
    y = y64.astype(np.float32) if mutant == 'y_unrounded' else rnd(y64.astype(np.float32))
    d = np.float64(np.float32(decay))
    keep, take = (1 - d, d) if mutant == 'decay_as_momentum' else (d, 1 - d)
    mv_stat = var if mutant == 'moving_var_biased' else var * rows / max(rows - 1, 1)
    out = dict(y=y, mean=mean, var=var, moving_mean=keep * given['moving_mean'] + take * mean, moving_var=keep * given['moving_var'] + take * mv_stat)
    dz = br.dz_of(y, given['dy'], dtype, relu, mask={'mask_dy': 'dy', 'mask_dropped': None}.get(mutant, 'y'), round_dz=mutant != 'dz_unrounded')
    mean32, var32 = mean.astype(np.float32), var.astype(np.float32)
    bwd = br.backward64(xs, dz, ga, mean32, var32, eps)
    dx = bwd['dx']
    if mutant == 'dbeta_term_dropped':
        dx = bwd['scale'] * (dz.reshape(rows, -1) - bwd['xhat'] * bwd['g'])
    if mutant == 'dgamma_term_dropped':
        dx = bwd['scale'] * (dz.reshape(rows, -1) - bwd['b'])
    out.update(dx=rnd(dx.reshape(xs.shape).astype(np.float32)), dgamma=bwd['dgamma'], dbeta=bwd['dbeta'], mean32=mean32, var32=var32)
    return out


def grade(tag, got, given, dtype, relu, decay=DECAY, verbose=False):
    """Every check a delivered result has to pass (got: the dict of run64, mean32 / var32 being what the backward was given): the
    forward, the moving statistics and the backward inside their bounds, y and dx storage-type values.  Raises AssertionError."""
    rnd = br.ROUND[dtype]
    xs = rnd(given['x'])
    eps = given['eps']
    br.grade_forward(tag, got, xs, given['gamma'], given['beta'], relu, eps, dtype, verbose)
    fwd = br.forward64(xs, given['gamma'], given['beta'], relu, eps)
    e_mean, e_var, _ = br.stat_bounds(xs, fwd)
    rows = fwd['rows']
    bessel = rows / max(rows - 1, 1)
    want_mm, want_mv = br.moving64(given['moving_mean'], given['moving_var'], fwd['mean'], fwd['var'], rows, decay)
    r_mm = br.ratio(got['moving_mean'], want_mm, br.moving_bound(decay, given['moving_mean'], fwd['mean'], want_mm, e_mean)).max()
    r_mv = br.ratio(got['moving_var'], want_mv, br.moving_bound(decay, given['moving_var'], fwd['var'] * bessel, want_mv, e_var * bessel)).max()
    assert r_mm <= 1.0 and r_mv <= 1.0, '%s: moving statistics outside their bound (mean %.3f, var %.3f)' % (tag, r_mm, r_mv)
    assert np.array_equal(rnd(got['y']), got['y']), '%s: y holds values the storage type does not have' % tag
    assert np.array_equal(rnd(got['dx']), got['dx']), '%s: dx holds values the storage type does not have' % tag
    dz = br.dz_of(got['y'], given['dy'], dtype, relu)
    top = br.grade_backward(tag, got, xs, dz, given['gamma'], got['mean32'], got['var32'], eps, dtype, verbose)
    return dict(top, moving_mean=r_mm, moving_var=r_mv)
