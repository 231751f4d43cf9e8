"""References of the backward of the SSD-only operators (include/ron_hip.h: ron_maxpool3x3s1_backward_nhwc,
ron_l2norm_backward_nhwc, ron_conv2d_padded_backward_nhwc), their error bounds and the mutants the tests have to kill.

Plain helper module (numpy only), built on tests/conv_bounds.py and tests/conv_grad_ref.py.

The pool (3x3, stride 1, SAME).  Float32 in the stated order, so the result is exact and the tests compare with np.array_equal:
xs = round(x); the window of output (oy, ox) holds the in-bounds positions of rows oy-1 .. oy+1, columns ox-1 .. ox+1; its
round(dy) goes to the first position, row-major, whose xs equals the window's maximum (start at the first in-bounds position, take
over on > only); a position adds what the windows hand it in row-major order of (oy, ox), starting from 0.f, and rounds once.
Two independent statements of it: `pool3_backward` scatters (windows in row-major order, np.add.at applies repeated indices in
order), `pool3_backward_loops` gathers per input position with explicit loops.

The L2 normalisation.  Float64, on xs = round(x), dz = round(dy), gamma as given:
    ss = sum_c xs^2;  inv = 1 / sqrt(max(ss, T));  u = xs inv;  g = dz gamma;  t = sum_c g u          T = float32(1e-12)
    dx = inv (g - u t)  where ss >= T,  inv g  elsewhere;      dgamma[c] = sum_p dz u
Bound, first order, one float32 ulp e = 2^-23 per operation (no fitted constant, no element excluded).  The kernel's sums: a lane
adds its 4 IT channels (IT = ceil(c / 256) rounded up to a power of two) and a butterfly adds 64 lanes: A = 4 IT + 6 additions on
a path.  Products of two storage-type values are exact in float32.
    ss     A e ss                                      (all terms positive)
    inv    r_inv = (A / 2 + 2) e  relative             (half of ss's, the square root, the division)
    u      r_u = r_inv + e
    t      r_t T_,  T_ = sum_c |g u|,  r_t = A e + (e [g] + r_u + e [the product])
    dx     inv [ 2 e |g| + |u| r_t T_ + |u t| (r_u + 2 e) ] + |dx| (r_inv + e)        the cancellation carries |g| + |u| sum|g u|
           clamped branch: |dx| (r_inv + 2 e);  then the rounding to the storage type: u_half |ref| + (1 + u_half) E (+ 2^-25, fp16)
    dgamma (B + 1) e S + r_u S,  S = sum_p |dz u|,  B = ceil(M / W) + ceil(W / 8) + 8: a wave's pixels, a run of table rows, the runs
           (W = min(M, 2048) table rows)

The padded convolutions.  Float64 by the scatter identity on top of conv_grad_ref: dz is scattered to (o + s oy, o + s ox), o = 1 -
cpad, of a zero map of the input's size and conv_grad_ref.grads64 does the rest - the bounds are conv_bounds' with the K of the
FULL-RESOLUTION problem (that is what the kernels add up, zero terms included)."""
import numpy as np

import conv_bounds as cb
import conv_grad_ref as cgr

F64 = np.float64
F32 = np.float32
ROUND = cgr.ROUND
EPS = 2.0 ** -23
CLAMP = float(np.float32(1e-12))
L2_MAX_WAVES = 2048
L2_RUNS = 8


# --------------------------------------------------------------------------------------------------------------------- #
# the pool
# --------------------------------------------------------------------------------------------------------------------- #
POOL_MUTANTS = ('last_maximum', 'unrounded_compare', 'padding_is_zero', 'window_shifted', 'reads_next_row', 'ties_share',
                'overwrite', 'dy_unrounded', 'sum_unrounded')
TAPS = tuple((dr, dc) for dr in (-1, 0, 1) for dc in (-1, 0, 1))


def _windows(xs, mutant):
    """For every window (n, oy, ox) and tap: the flat pixel index it reads [9, n, h, w], whether it takes part [9, n, h, w] and
    whether it is a real position of the map that may receive the gradient."""
    n, h, w, _ = xs.shape
    i, oy, ox = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing='ij')
    flat, part, real = [], [], []
    for dr, dc in TAPS:
        rr, cc = oy + dr, ox + dc + (1 if mutant == 'window_shifted' else 0)
        p = (i * h + rr) * w + cc
        inb = (rr >= 0) & (rr < h) & (cc >= 0) & (cc < w)
        if mutant == 'reads_next_row':          # the flat address is read whatever row / image it falls in
            on = (p >= 0) & (p < n * h * w)
            flat.append(np.where(on, p, -1)), part.append(on), real.append(on)
        elif mutant == 'padding_is_zero':
            flat.append(np.where(inb, p, -1)), part.append(np.ones_like(inb)), real.append(inb)
        else:
            flat.append(np.where(inb, p, -1)), part.append(inb), real.append(inb)
    return np.stack(flat), np.stack(part), np.stack(real)


def pool3_backward(x, dy, dtype, mutant=None):
    """dx float32 [n,h,w,c]: the scatter statement; `mutant`: one wrong decision of POOL_MUTANTS."""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    rnd = ROUND[dtype]
    xs = x if mutant == 'unrounded_compare' else rnd(x)
    g = dy if mutant == 'dy_unrounded' else rnd(dy)
    n, h, w, c = x.shape
    flat, part, real = _windows(xs, mutant)
    xf = np.concatenate([xs.reshape(-1, c), np.zeros((1, c), F32)])          # index -1: a padding position (read as 0 by one mutant)
    best = np.zeros((n, h, w, c), F32)
    at = np.full((n, h, w, c), -1, np.int64)
    for k in range(9):
        v = xf[flat[k]]
        on = part[k][..., None]
        take = on & ((at < 0) | ((v >= best) if mutant == 'last_maximum' else (v > best)))
        best = np.where(take, v, best)
        at = np.where(take, k, at)
    out = np.zeros((n * h * w + 1, c), F32)
    ch = np.broadcast_to(np.arange(c), (n, h, w, c))
    if mutant == 'ties_share':
        ties = np.stack([part[k][..., None] & (xf[flat[k]] == best) for k in range(9)])
        share = (g / ties.sum(axis=0).astype(F32)).astype(F32)
        for k in range(9):
            tgt = np.where(ties[k] & real[k][..., None], flat[k][..., None], -1)
            np.add.at(out, (tgt.reshape(-1), ch.reshape(-1)), share.reshape(-1))
    else:
        tgt = np.take_along_axis(np.broadcast_to(flat[..., None], (9, n, h, w, c)), at[None], axis=0)[0]
        ok = np.take_along_axis(np.broadcast_to(real[..., None], (9, n, h, w, c)), at[None], axis=0)[0]
        tgt = np.where(ok, tgt, -1)
        if mutant == 'overwrite':
            out[tgt.reshape(-1), ch.reshape(-1)] = g.reshape(-1)
        else:
            np.add.at(out, (tgt.reshape(-1), ch.reshape(-1)), g.reshape(-1))          # windows in row-major order, float32 additions
    dx = out[:-1].reshape(n, h, w, c)
    return dx if mutant == 'sum_unrounded' else rnd(dx)


def pool3_backward_loops(x, dy, dtype):
    """The same rule as a gather with explicit loops: every input position asks each window that contains it."""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    xs, g = ROUND[dtype](x), ROUND[dtype](dy)
    n, h, w, c = x.shape
    dx = np.zeros(x.shape, F32)
    for i in range(n):
        for r in range(h):
            for q in range(w):
                for ch in range(c):
                    total = F32(0)
                    for oy in range(max(r - 1, 0), min(r + 2, h)):
                        for ox in range(max(q - 1, 0), min(q + 2, w)):
                            best, at = None, None
                            for yy in range(max(oy - 1, 0), min(oy + 2, h)):
                                for xx in range(max(ox - 1, 0), min(ox + 2, w)):
                                    if best is None or xs[i, yy, xx, ch] > best:
                                        best, at = xs[i, yy, xx, ch], (yy, xx)
                            if at == (r, q):
                                total = F32(total + g[i, oy, ox, ch])
                    dx[i, r, q, ch] = total
    return ROUND[dtype](dx)


def pool3_forward(x, dtype):
    """The pool itself on xs (padding excluded): what ron_maxpool3x3s1_nhwc gives for non-negative inputs."""
    xs = ROUND[dtype](np.asarray(x, F32))
    n, h, w, c = xs.shape
    p = np.full((n, h + 2, w + 2, c), -np.inf, F32)
    p[:, 1:-1, 1:-1] = xs
    return np.max(np.stack([p[:, a:a + h, b:b + w] for a in range(3) for b in range(3)]), axis=0)


def pool3_late_ties(x, dtype):
    """Windows whose maximum is shared by several positions and does not sit at the window's first in-bounds position."""
    xs = ROUND[dtype](np.asarray(x, F32))
    n, h, w, c = xs.shape
    flat, part, _ = _windows(xs, None)
    xf = np.concatenate([xs.reshape(-1, c), np.full((1, c), -np.inf, F32)])
    vals = np.stack([np.where(part[k][..., None], xf[flat[k]], -np.inf) for k in range(9)])
    top = vals.max(axis=0)
    is_top = vals == top
    first_in = np.argmax(part, axis=0)[..., None]
    first_top = np.argmax(is_top, axis=0)
    return int(((is_top.sum(axis=0) >= 2) & (first_top != first_in)).sum())


# --------------------------------------------------------------------------------------------------------------------- #
# the L2 normalisation
# --------------------------------------------------------------------------------------------------------------------- #
L2_MUTANTS = ('projection_dropped', 'inv_missing', 'inv_twice', 'gamma_missing', 'dgamma_from_xs', 'clamp_ignored', 'clamped_pixel_projected',
              'dy_unrounded', 'table_row_dropped')


def l2_forward64(xs, gamma):
    xs = np.asarray(xs, F64)
    ss = (xs * xs).sum(axis=-1, keepdims=True)
    return xs / np.sqrt(np.maximum(ss, CLAMP)) * np.asarray(gamma, F64)


def l2_rows(m):
    return min(m, L2_MAX_WAVES)


def l2_backward64(xs, gamma, dz, mutant=None):
    """dict(dx [n,h,w,c], dgamma [c]) in float64 plus the magnitudes the bound needs."""
    xs, dz, gamma = np.asarray(xs, F64), np.asarray(dz, F64), np.asarray(gamma, F64)
    c = xs.shape[-1]
    ss = (xs * xs).sum(axis=-1, keepdims=True)
    live = ss >= CLAMP
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = 1.0 / np.sqrt(ss if mutant == 'clamp_ignored' else np.maximum(ss, CLAMP))          # the mutant: 1 / 0 at an all-zero pixel
        u = xs * inv
    g = dz if mutant == 'gamma_missing' else dz * gamma
    t = (g * u).sum(axis=-1, keepdims=True)
    proj = np.where(live, u * t, 0.0)
    if mutant == 'projection_dropped':
        proj = 0.0 * proj
    if mutant == 'clamped_pixel_projected':
        proj = u * t
    dx = inv * (g - proj)
    if mutant == 'inv_missing':
        dx = g - proj
    if mutant == 'inv_twice':
        dx = inv * inv * (g - proj)
    prod = dz * (xs if mutant == 'dgamma_from_xs' else u)
    flatp = prod.reshape(-1, c)
    if mutant == 'table_row_dropped':
        rows = l2_rows(flatp.shape[0])
        keep = np.arange(flatp.shape[0]) % rows != rows - 1
        flatp = flatp[keep] if rows > 1 else 0.0 * flatp
    return dict(dx=dx, dgamma=flatp.sum(axis=0), live=live, inv=inv, u=u, g=g, t=t, T=np.abs(g * u).sum(axis=-1, keepdims=True),
                S=np.abs(dz * u).reshape(-1, c).sum(axis=0))


def l2_lengths(m, c):
    """(A, B): additions on the longest path of a pixel's sums and of dgamma (module docstring)."""
    it = -(-c // 256)
    it = 1 << (it - 1).bit_length()
    rows = l2_rows(m)
    return 4 * it + 6, -(-m // rows) + -(-rows // L2_RUNS) + L2_RUNS


def l2_bounds(ref, dtype):
    """dict(dx, dgamma) of per-element bounds for the float64 reference `ref` of l2_backward64."""
    dx = ref['dx']
    m, c = int(np.prod(dx.shape[:-1])), dx.shape[-1]
    A, B = l2_lengths(m, c)
    r_inv = (A / 2 + 2) * EPS
    r_u = r_inv + EPS
    r_t = A * EPS + (EPS + r_u + EPS)
    g, u, t, T, inv = np.abs(ref['g']), np.abs(ref['u']), np.abs(ref['t']), ref['T'], ref['inv']
    e_live = inv * (2 * EPS * g + u * r_t * T + u * t * (r_u + 2 * EPS)) + np.abs(dx) * (r_inv + EPS)
    e_dead = np.abs(dx) * (r_inv + 2 * EPS)
    E = np.where(ref['live'], e_live, e_dead)
    uh = cb.U_HALF_ULP[dtype]
    b = uh * np.abs(dx) + (1 + uh) * E
    if dtype == 'fp16':
        b = b + 2.0 ** -25
    return dict(dx=b, dgamma=((B + 1) * EPS + r_u) * ref['S'])


def l2_ratio(got, ref, bound):
    """error / bound per element (0 / 0 = 0; +inf wherever `err <= bound` is not true, NaN included)."""
    err = np.abs(np.asarray(got, F64) - ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        inside = err <= bound
        r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(F64).tiny))
    return np.where(inside, r, np.where(np.isfinite(r) & (r > 1.0), r, np.inf))


def l2_seen(x, dy, dtype, round_dz=True):
    rnd = ROUND[dtype]
    return rnd(np.asarray(x, F32)), (rnd(np.asarray(dy, F32)) if round_dz else np.asarray(dy, F32))


def l2_deliver(ref, dtype):
    """A float64 reference as the entry point would hand it over."""
    return dict(dx=ROUND[dtype](ref['dx'].astype(F32)), dgamma=ref['dgamma'].astype(F32))


def l2_grade(tag, got, x, gamma, dy, dtype, kind, verbose=True):
    """{'dx' | 'dgamma': largest error / bound} of the outputs present in `got`: lattice inputs must EQUAL the reference (0 or inf),
    gauss inputs are graded by the derived bound."""
    xs, dz = l2_seen(x, dy, dtype)
    ref = l2_backward64(xs, gamma, dz)
    bounds = l2_bounds(ref, dtype)
    out = {}
    for name in ('dx', 'dgamma'):
        if got.get(name) is None:
            continue
        gv = np.asarray(got[name])
        assert gv.shape == ref[name].shape, (name, gv.shape, ref[name].shape)
        if kind == 'lattice':
            out[name] = 0.0 if np.array_equal(gv, ref[name]) else np.inf
            continue
        top, where = cb.worst(l2_ratio(gv, ref[name], bounds[name]))
        if verbose:
            print('RATIO l2norm %s %s %s: largest error / bound %.3f at %s (got %r, float64 %r)' % (tag, name, dtype, top, where,
                                                                                                     float(gv[where]), float(ref[name][where])))
        out[name] = top
    return out


def l2_check(tag, got, x, gamma, dy, dtype, kind):
    for name, top in l2_grade(tag, got, x, gamma, dy, dtype, kind).items():
        assert top <= 1.0, '%s %s %s (%s): error / bound = %s' % (tag, name, dtype, kind, top)


def l2_mutant(name, x, gamma, dy, dtype):
    xs, dz = l2_seen(x, dy, dtype, round_dz=name != 'dy_unrounded')
    return l2_deliver(l2_backward64(xs, gamma, dz, mutant=name), dtype)


# --------------------------------------------------------------------------------------------------------------------- #
# the padded 3x3 convolutions
# --------------------------------------------------------------------------------------------------------------------- #
PADDED_MUTANTS = ('offset_for_valid', 'scatter_stride_1', 'last_row_col_dropped', 'mask_full_resolution', 'not_zeroed')


def out_hw(h, w, stride, cpad, k=3):
    return (h + 2 * cpad - k) // stride + 1, (w + 2 * cpad - k) // stride + 1


def scatter(dz, h, w, stride, cpad, mutant=None):
    """dz [n,ho,wo,cout] at (o + stride oy, o + stride ox) of a zero [n,h,w,cout] map."""
    dz = np.asarray(dz)
    n, ho, wo, cout = dz.shape
    o = 1 - cpad
    if mutant == 'offset_for_valid':
        o = 0
    if mutant == 'scatter_stride_1':
        stride = 1
    if mutant == 'last_row_col_dropped':
        dz = dz.copy()
        if h % 2 == 1 and stride == 2:
            dz[:, ho - 1] = 0
        if w % 2 == 1 and stride == 2:
            dz[:, :, wo - 1] = 0
    full = np.zeros((n, h, w, cout), dz.dtype)
    if mutant == 'not_zeroed':          # whatever the buffer held: here the neighbouring sample
        full = np.repeat(np.repeat(dz, stride, axis=1), stride, axis=2)
        full = np.pad(full, ((0, 0), (o, h), (o, w), (0, 0)), mode='edge')[:, :h, :w].copy()
    full[:, o:o + stride * ho:stride, o:o + stride * wo:stride] = dz
    return full


def padded_seen(x, w, y, dy, dtype, relu, h, wd, stride, cpad, mutant=None):
    """(xs, ws, dz) with dz [n,ho,wo,cout]: the mask is y > 0 at the operator's own output position."""
    if mutant == 'mask_full_resolution' and relu:
        n, ho, wo, cout = y.shape
        o = 1 - cpad
        i, oy, ox = np.meshgrid(np.arange(n), np.arange(ho), np.arange(wo), indexing='ij')
        p = (i * h + o + stride * oy) * wd + o + stride * ox          # the pixel index of the full-resolution position, read in y
        yf = np.concatenate([y.reshape(-1, cout), np.zeros((int(p.max()) + 1, cout), y.dtype)])
        y = yf[p]
    return cgr.seen(x, w, y, dy, dtype, relu)


def grads64_padded(xs, ws, dz, stride, cpad, mutant=None):
    n, h, w, _ = xs.shape
    return cgr.grads64(xs, ws, scatter(dz, h, w, stride, cpad, mutant), 1)


def padded_mutant(name, x, w, y, dy, dtype, relu, stride, cpad):
    """(dx, dw, db) as the entry point would deliver them with one wrong decision, or None where it changes nothing by construction."""
    n, h, wd, _ = x.shape
    ho, wo = dy.shape[1:3]
    if name == 'offset_for_valid' and cpad != 0:
        return None
    if name == 'scatter_stride_1' and (stride == 1 or (ho == 1 and wo == 1)):
        return None
    if name == 'last_row_col_dropped' and (stride == 1 or (h % 2 == 0 and wd % 2 == 0)):
        return None
    if name == 'mask_full_resolution' and (not relu or (ho == 1 and wo == 1 and n == 1 and cpad == 1)):
        return None
    if name == 'not_zeroed' and ho == h and wo == wd:
        return None
    xs, ws, dz = padded_seen(x, w, y, dy, dtype, relu, h, wd, stride, cpad, name)
    g = grads64_padded(xs, ws, dz, stride, cpad, name)
    return cgr.deliver(g, dtype)
