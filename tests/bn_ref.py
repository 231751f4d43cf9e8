"""Float64 reference of training-mode batch normalisation (ron_batchnorm_train_nhwc / ron_batchnorm_backward_nhwc), the float32
emulation of the kernel's statistics, and PER-ELEMENT error bounds in the manner of tests/conv_bounds.py.

Plain helper module (numpy only).  Everything takes the operands AS THE KERNEL SEES THEM: xs = round(x) to the storage type; gamma,
beta and the statistics stay float32.  With M = n h w rows and one column per channel:

  forward64    mean, var (biased), rstd, v = gamma (xs - mean) rstd + beta, y = act(v)        (nothing rounded)
  moving64     decay m + (1 - decay) statistic, the variance Bessel-corrected: M / max(M - 1, 1)
  backward64   dz = round(dy (y > 0)) or round(dy); xhat; dbeta = sum dz; dgamma = sum dz xhat;
               dx = gamma rstd (dz - dbeta / M - xhat dgamma / M)                               (dx not rounded)

The geometry (``geometry``: csrc/batchnorm.hip, plan_bn) decides the accumulation order and so the accumulation lengths:
a lane adds every rpb-th row of its slice, shifted by the first value it meets (K): s1 = sum(xs - K), s2 = sum((xs - K)^2), and ends
with (count, K + s1 / count, s2 - s1^2 / count); Chan's formula merges the rpb row lanes of a workgroup, then the slices, behind a
binary tree of D = log2(rpb) + 2 + 8 levels.  ``stats_emulate32`` does exactly that in float32.

Bounds (first order in e = 2^-23, ONE float32 ulp per operation where round-to-nearest gives half: the other half pays for the
second-order terms, as in conv_bounds; no constant is fitted to a kernel, no element is excluded).  Per channel, with n_l, A1_l =
sum |xs - K|, S2_l = sum (xs - K)^2 of lane l, R = max |xs|, rng = max xs - min xs, a1 = max_l A1_l:

  a lane      s1 errs by n_l e A1_l (the subtraction and n_l - 1 additions of magnitudes <= A1_l), so its mean by e (2 A1_l + R);
              s2 by (n_l + 2) e S2_l; M2 = s2 - s1 (s1 / n_l) with s1^2 / n_l <= S2_l (Cauchy-Schwarz) by e (3 n_l + 6) S2_l
  a merge     mean = ma + delta f: the children's errors averaged with weights (1 - f, f), plus 3 e |delta| f + e |mean|:
              after D levels every node's mean is within  Em = e (2 a1 + R + D (3 rng + R))
              M2 = Ma + Mb + delta^2 w, w = na nb / n: the children's errors, 2 |delta| w (2 Em + e |delta|), 4 e delta^2 w and
              2 e M2.  Over the tree sum(delta^2 w) <= M2, sum(w) <= M D / 4, so sum(|delta| w) <= sqrt(M2 M D) / 2 and
              E_M2 = e (sum_l (3 n_l + 6) S2_l + (6 + 2 D) M2) + 2 Em sqrt(M2 M D)
  mean, var   E_mean = Em;  E_var = E_M2 / M + e var
  rstd        1 / sqrt(var + eps): relative  rho = E_var / (2 (var + eps)) + 4 e  (the addition, the root, the division, one spare)
  y           xhat = (xs - mean) rstd errs by rstd (E_mean + e |xs - mean|) + |xhat| (rho + e); v by |gamma| that
              + e (2 |gamma xhat| + |beta|); ReLU is 1-Lipschitz; the output rounding adds u |ref| + u E_v (u: half an ulp of the
              storage type; + 2^-25 for fp16, the subnormal quantum)
  moving      (1 - decay) E_stat + e (|decay m| + 2 |statistic| + |result|)
  backward    (mean and var are INPUTS there: the reference reads the same float32 values, so only rho = 4 e remains)
              dbeta: L e sum |dz|, L = max n_l + D additions on the longest path; dgamma: sum |dz xhat| (rho + 3 e + L e)
              dx: t = dz - b - xhat g, b = dbeta / M, g = dgamma / M, the three terms that cancel carried as A = |dz| + |b| + |xhat g|:
              E_t = E_b + |xhat| E_g + |g xhat| (rho + 2 e) + 3 e A, E_b = E_dbeta / M + e |b|, E_g = E_dgamma / M + e |g|;
              E = |gamma| rstd E_t + |dx| (rho + 2 e), then the output rounding as for y
"""
import numpy as np

import conv_bounds as cb
from oracle import ron_forward as orf

F64, F32 = np.float64, np.float32
ROUND = {'bf16': orf.round_bf16, 'fp16': orf.round_f16}
E32 = cb.EPS32
MAX_SLICES = 1024
THREADS = 256


# --------------------------------------------------------------------------------------------------------------------- geometry
def _pow2_ceil(v):
    p = 1
    while p < v:
        p *= 2
    return p


def geometry(n, h, w, c):
    """The launch geometry of csrc/batchnorm.hip (plan_bn): a function of the shape alone."""
    rows, cg = n * h * w, c // 4
    lpr = min(64, _pow2_ceil(cg))
    rpb = THREADS // lpr
    slice_rows = max(rpb * 4, _pow2_ceil(-(-rows // MAX_SLICES)))
    slices = -(-rows // slice_rows)
    part = -(-slices * 2 * c * 4 // 256) * 256
    fin = -(-2 * c * 4 // 256) * 256
    return dict(rows=rows, c=c, cg=cg, lpr=lpr, rows_per_wave=64 // lpr, rpb=rpb, tiles=-(-cg // lpr), slice_rows=slice_rows, slices=slices,
                depth=int(np.log2(rpb)) + 2 + 8, workspace_bytes=part + fin)


def lanes(geo):
    """(slice, first row, step, count) of every lane that holds rows, in slice order then row-lane order."""
    for s in range(geo['slices']):
        r0 = s * geo['slice_rows']
        cnt = min(geo['slice_rows'], geo['rows'] - r0)
        for rl in range(min(geo['rpb'], cnt)):
            yield s, r0 + rl, geo['rpb'], -(-(cnt - rl) // geo['rpb'])


def _lane_rows(x2, first, step, count):
    return x2[first: first + (count - 1) * step + 1: step]


# --------------------------------------------------------------------------------------------------------------- float64 reference
def forward64(xs, gamma, beta, relu, eps):
    x2 = np.asarray(xs, F64).reshape(-1, xs.shape[-1])
    mean = x2.mean(axis=0)
    var = ((x2 - mean) ** 2).mean(axis=0)
    rstd = 1.0 / np.sqrt(var + F64(F32(eps)))
    xhat = (x2 - mean) * rstd
    v = np.asarray(gamma, F64) * xhat + np.asarray(beta, F64)
    y = np.maximum(v, 0) if relu else v
    return dict(mean=mean, var=var, rstd=rstd, xhat=xhat.reshape(xs.shape), v=v.reshape(xs.shape), y=y.reshape(xs.shape), rows=x2.shape[0])


def moving64(moving_mean, moving_var, mean, var, rows, decay):
    d = F64(F32(decay))
    return (d * np.asarray(moving_mean, F64) + (1 - d) * mean,
            d * np.asarray(moving_var, F64) + (1 - d) * var * rows / max(rows - 1, 1))


def dz_of(y, dy, dtype, relu, mask='y', round_dz=True):
    """dz as the kernel forms it (float32).  `mask` 'y' (the contract), 'dy' or None and round_dz=False are the mutants."""
    dy = np.asarray(dy, F32)
    if relu and mask == 'y':
        dy = np.where(np.asarray(y) > 0, dy, F32(0))
    elif relu and mask == 'dy':
        dy = np.where(dy > 0, dy, F32(0))
    return ROUND[dtype](dy) if round_dz else dy


def backward64(xs, dz, gamma, mean, var, eps):
    c = xs.shape[-1]
    x2, z2 = np.asarray(xs, F64).reshape(-1, c), np.asarray(dz, F64).reshape(-1, c)
    rows = x2.shape[0]
    rstd = 1.0 / np.sqrt(np.asarray(var, F64) + F64(F32(eps)))
    xhat = (x2 - np.asarray(mean, F64)) * rstd
    dbeta, dgamma = z2.sum(axis=0), (z2 * xhat).sum(axis=0)
    b, g = dbeta / rows, dgamma / rows
    scale = np.asarray(gamma, F64) * rstd
    dx = scale * (z2 - b - xhat * g)
    return dict(dbeta=dbeta, dgamma=dgamma, dx=dx.reshape(xs.shape), xhat=xhat, rstd=rstd, scale=scale, b=b, g=g,
                abs_dz=np.abs(z2).sum(axis=0), abs_dzx=np.abs(z2 * xhat).sum(axis=0),
                A=(np.abs(z2) + np.abs(b) + np.abs(xhat * g)), rows=rows)


# ------------------------------------------------------------------------------------------------------------ float32 emulation
def _chan(a, b):
    (na, ma, Ma), (nb, mb, Mb) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = F32(na) + F32(nb)
    f = F32(nb) / n
    w = F32(na) * f
    delta = mb - ma
    return n, ma + delta * f, (Ma + Mb) + (delta * delta) * w


def _tree(nodes):
    """lane i with lane i + stride, the stride halving: len(nodes) a power of two."""
    nodes = list(nodes)
    off = len(nodes) // 2
    while off >= 1:
        for i in range(off):
            nodes[i] = _chan(nodes[i], nodes[i + off])
        off //= 2
    return nodes[0]


def stats_emulate32(xs, order='kernel', drop_last_slice=False):
    """(mean, var) in float32.  order 'kernel': the lanes, shifts and merge trees of csrc/batchnorm.hip; 'sequential': one lane adds
    every row (shifted by the first) - the longest accumulation a call can have; 'naive': the MUTANT E[x^2] - mean^2 from plain float32
    sums.  drop_last_slice: the MUTANT that forgets the last (partial) slice and divides by the rows it saw."""
    n, h, w, c = xs.shape
    x2 = np.asarray(xs, F32).reshape(-1, c)
    rows = x2.shape[0]
    if order == 'naive':
        s1 = np.cumsum(x2, axis=0, dtype=F32)[-1]
        s2 = np.cumsum(x2 * x2, axis=0, dtype=F32)[-1]
        mean = s1 / F32(rows)
        return mean, s2 / F32(rows) - mean * mean

    def lane(r):
        k, cnt = r[0], F32(r.shape[0])
        d = r[1:] - k
        zero = np.zeros((c,), F32)
        s1 = np.cumsum(d, axis=0, dtype=F32)[-1] if len(d) else zero
        s2 = np.cumsum(d * d, axis=0, dtype=F32)[-1] if len(d) else zero
        q = s1 / cnt
        return cnt, k + q, np.maximum(s2 - s1 * q, F32(0))
    if order == 'sequential':
        _, mean, m2 = lane(x2)
        return mean, m2 / F32(rows)
    geo = geometry(n, h, w, c)
    empty = (F32(0), np.zeros((c,), F32), np.zeros((c,), F32))
    per_slice = [[] for _ in range(geo['slices'])]
    for s, first, step, count in lanes(geo):
        per_slice[s].append(lane(_lane_rows(x2, first, step, count)))
    if drop_last_slice and geo['slices'] > 1:
        per_slice, rows = per_slice[:-1], (geo['slices'] - 1) * geo['slice_rows']
    sl = [_tree(p + [empty] * (geo['rpb'] - len(p))) for p in per_slice]
    sl += [empty] * (MAX_SLICES - len(sl))
    threads = [_chan(_chan(sl[4 * t], sl[4 * t + 1]), _chan(sl[4 * t + 2], sl[4 * t + 3])) for t in range(THREADS)]
    cnt, mean, m2 = _tree(threads)
    assert cnt == rows
    return mean, m2 / F32(rows)


# -------------------------------------------------------------------------------------------------------------------- the bounds
def stat_bounds(xs, fwd):
    """(E_mean, E_var) per channel: see the module docstring."""
    n, h, w, c = xs.shape
    geo = geometry(n, h, w, c)
    x2 = np.asarray(xs, F64).reshape(-1, c)
    rows, D = geo['rows'], geo['depth']
    lane_m2, a1, longest = np.zeros(c), np.zeros(c), 0
    for _, first, step, count in lanes(geo):
        d = _lane_rows(x2, first, step, count) - x2[first]
        lane_m2 += (3 * count + 6) * (d * d).sum(axis=0)
        a1 = np.maximum(a1, np.abs(d).sum(axis=0))
        longest = max(longest, count)
    R, rng = np.abs(x2).max(axis=0), x2.max(axis=0) - x2.min(axis=0)
    em = E32 * (2 * a1 + R + D * (3 * rng + R))
    m2 = fwd['var'] * rows
    e_m2 = E32 * (lane_m2 + (6 + 2 * D) * m2) + 2 * em * np.sqrt(m2 * rows * D)
    return em, e_m2 / rows + E32 * fwd['var'], longest + D


def _deliver(ref, e_value, dtype):
    u = cb.U_HALF_ULP[dtype]
    b = u * np.abs(ref) + (1 + u) * e_value
    return b + 2.0 ** -25 if dtype == 'fp16' else b


def y_bound(xs, gamma, beta, fwd, eps, dtype, e_mean, e_var):
    c = xs.shape[-1]
    x2 = np.asarray(xs, F64).reshape(-1, c)
    rho = e_var / (2 * (fwd['var'] + F64(F32(eps)))) + 4 * E32
    xhat = fwd['xhat'].reshape(-1, c)
    e_xhat = fwd['rstd'] * (e_mean + E32 * np.abs(x2 - fwd['mean'])) + np.abs(xhat) * (rho + E32)
    ga, be = np.abs(np.asarray(gamma, F64)), np.abs(np.asarray(beta, F64))
    e_v = ga * e_xhat + E32 * (2 * ga * np.abs(xhat) + be)
    return _deliver(fwd['y'], e_v.reshape(xs.shape), dtype)


def moving_bound(decay, moving, stat, result, e_stat):
    d = F64(F32(decay))
    return (1 - d) * e_stat + E32 * (np.abs(d * np.asarray(moving, F64)) + 2 * np.abs(stat) + np.abs(result))


def backward_bounds(xs, gamma, bwd, dtype, length):
    """dict(dbeta, dgamma, dx) of per-element bounds; `length`: the additions on the longest path (stat_bounds' third result)."""
    rho = 4 * E32
    rows = bwd['rows']
    e_db = length * E32 * bwd['abs_dz']
    e_dg = bwd['abs_dzx'] * (rho + 3 * E32 + length * E32)
    e_b, e_g = e_db / rows + E32 * np.abs(bwd['b']), e_dg / rows + E32 * np.abs(bwd['g'])
    xhat = np.abs(bwd['xhat'])
    e_t = e_b + xhat * e_g + np.abs(bwd['g']) * xhat * (rho + 2 * E32) + 3 * E32 * bwd['A']
    dx = bwd['dx'].reshape(-1, xs.shape[-1])
    e_dx = np.abs(bwd['scale']) * e_t + np.abs(dx) * (rho + 2 * E32)
    return dict(dbeta=e_db, dgamma=e_dg, dx=_deliver(bwd['dx'], e_dx.reshape(xs.shape), dtype))


def ratio(got, ref, bound):
    """error / bound per element (0 / 0 = 0; +inf wherever `err <= bound` is not true, NaN included): assert ratio(...).max() <= 1."""
    err = np.abs(np.asarray(got, F64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(invalid='ignore', divide='ignore'):
        inside = err <= bound
        r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(F64).tiny))
    return np.where(inside, r, np.where(np.isfinite(r) & (r > 1.0), r, np.inf))


def grade_forward(tag, got, xs, gamma, beta, relu, eps, dtype, verbose=True):
    """got: dict(y, mean, var) as delivered.  Returns the largest ratio per output; asserts every one <= 1."""
    fwd = forward64(xs, gamma, beta, relu, eps)
    e_mean, e_var, _ = stat_bounds(xs, fwd)
    top = {'mean': ratio(got['mean'], fwd['mean'], e_mean).max(), 'var': ratio(got['var'], fwd['var'], e_var).max(),
           'y': ratio(got['y'], fwd['y'], y_bound(xs, gamma, beta, fwd, eps, dtype, e_mean, e_var)).max()}
    if verbose:
        print('%s forward: ' % tag + ', '.join('%s %.4f' % kv for kv in sorted(top.items())))
    for name, r in top.items():
        assert r <= 1.0, '%s: %s is outside its bound (ratio %.3f)' % (tag, name, r)
    return top


def grade_backward(tag, got, xs, dz, gamma, mean, var, eps, dtype, verbose=True):
    """got: dict of the delivered outputs (None: not computed).  mean, var: what the call was given."""
    n, h, w, c = xs.shape
    geo = geometry(n, h, w, c)
    length = -(-geo['slice_rows'] // geo['rpb']) + geo['depth']
    bwd = backward64(xs, dz, gamma, mean, var, eps)
    bounds = backward_bounds(xs, gamma, bwd, dtype, length)
    top = {name: ratio(got[name], bwd[name], bounds[name]).max() for name in ('dx', 'dgamma', 'dbeta') if got.get(name) is not None}
    if verbose:
        print('%s backward: ' % tag + ', '.join('%s %.4f' % kv for kv in sorted(top.items())))
    for name, r in top.items():
        assert r <= 1.0, '%s: %s is outside its bound (ratio %.3f)' % (tag, name, r)
    return top
