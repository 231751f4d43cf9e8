"""Float64 reference of the convolution backward (ron_conv2d_backward_nhwc, include/ron_hip.h) with per-element bounds, a float32
emulation with selectable accumulation order, and the mutants the tests have to kill.

Plain helper module (numpy only), built on tests/conv_bounds.py.  The operator, on operands AS THE KERNEL SEES THEM:

    dz = round(dy * (y > 0))  (relu)  or  round(dy);        xs = round(x), ws = round(w)
    dx = round(conv_SAME(dz, w')),  w'[ky,kx,co,ci] = ws[kh-1-ky, kw-1-kx, ci, co]          K = kh * kw * cout
    dw[ky,kx,ci,co] = sum_{n,y,x} xs[n, y + ky*r - p, x + kx*r - p, ci] * dz[n,y,x,co]      K = n * h * w, fp32, not rounded
    db[co] = sum dz[..., co]                                                               K = n * h * w

Grading is conv_bounds.ratio <= 1 per element, no exclusions: bound(ref, S, K, dtype) for dx, bound(ref, S, K, dtype, 'fp32') for dw
and db.  The derivation of conv_bounds.py carries over unchanged: products of two storage-type values are exact in float32, K float32
additions in any order (the slab sums of the pixel slices included) err by at most K * 2^-23 * S, dx is rounded once, dw and db are
not.  No constant is fitted."""
import numpy as np

import conv_bounds as cb
from oracle import ron_forward as orf

F64 = np.float64
ROUND = {'bf16': orf.round_bf16, 'fp16': orf.round_f16}
STEP = 32          # pixels per K step of the weight-gradient kernel


def seen(x, w, y, dy, dtype, relu, mask='y', round_dz=True):
    """(xs, ws, dz) float32: what the kernels multiply.  mask 'y' is the operator; 'dy' and 'none' are mutants."""
    rnd = ROUND[dtype]
    dz = np.asarray(dy, np.float32)
    if relu and mask != 'none':
        dz = np.where((y if mask == 'y' else dy) > 0, dz, np.float32(0))
    return rnd(x), rnd(w), (rnd(dz) if round_dz else dz)


def flipped(ws):
    """w'[ky,kx,co,ci] = ws[kh-1-ky, kw-1-kx, ci, co]"""
    return np.ascontiguousarray(np.flip(np.asarray(ws), (0, 1)).transpose(0, 1, 3, 2))


def dw64(xs, dz, k, rate):
    xs, dz = np.asarray(xs, F64), np.asarray(dz, F64)
    n, h, w, cin = xs.shape
    cout = dz.shape[3]
    p = (k - 1) * rate // 2
    xp = np.pad(xs, ((0, 0), (p, p), (p, p), (0, 0)))
    out = np.zeros((k, k, cin, cout), F64)
    flat = dz.reshape(-1, cout)
    for ky in range(k):
        for kx in range(k):
            out[ky, kx] = xp[:, ky * rate: ky * rate + h, kx * rate: kx * rate + w, :].reshape(-1, cin).T @ flat
    return out


def grads64(xs, ws, dz, rate=1):
    """{'dx': (ref64, S, K), 'dw': ..., 'db': ...} from the kernel-visible operands."""
    k = ws.shape[0]
    n, h, w, _ = xs.shape
    axs, aws, adz = np.abs(np.asarray(xs, F64)), np.abs(np.asarray(ws, F64)), np.abs(np.asarray(dz, F64))
    return {
        'dx': (cb.conv64(dz, flipped(ws), rate=rate), cb.conv64(adz, flipped(aws), rate=rate), k * k * ws.shape[3]),
        'dw': (dw64(xs, dz, k, rate), dw64(axs, adz, k, rate), n * h * w),
        'db': (np.asarray(dz, F64).sum(axis=(0, 1, 2)), adz.sum(axis=(0, 1, 2)), n * h * w),
    }


OUT_DTYPE = {'dx': None, 'dw': 'fp32', 'db': 'fp32'}


def deliver(ref, dtype):
    """A float64 reference as the entry point would hand it over: dx rounded to the storage type, dw / db as float32."""
    return {'dx': ROUND[dtype](ref['dx'][0].astype(np.float32)), 'dw': ref['dw'][0].astype(np.float32), 'db': ref['db'][0].astype(np.float32)}


def grade(tag, got, ref, dtype, kind, verbose=True):
    """{'dx' | 'dw' | 'db': largest error / bound} of the outputs present in `got` (None = not computed); asserts nothing: see check."""
    out = {}
    for name, g in got.items():
        if g is None:
            continue
        r64, S, K = ref[name]
        g = np.asarray(g)
        assert g.shape == r64.shape, (name, g.shape, r64.shape)
        if kind == 'lattice':
            out[name] = 0.0 if np.array_equal(g, r64) else np.inf
            continue
        top, at = cb.worst(cb.ratio(g, r64, S, K, dtype, OUT_DTYPE[name]))
        if verbose:
            print('RATIO %s %s %s K=%d: largest error / bound %.3f at %s (got %r, float64 %r)' % (tag, name, dtype, K, top, at, float(g[at]), float(r64[at])))
        out[name] = top
    return out


def check(tag, got, ref, dtype, kind):
    """The tests' assertion: lattice outputs EQUAL the exact result, gauss outputs are inside the bound per element."""
    for name, top in grade(tag, got, ref, dtype, kind).items():
        if kind == 'lattice':
            assert top == 0.0, '%s %s %s: differs from the exact integer result in %d elements' % (
                tag, name, dtype, int((np.asarray(got[name]) != ref[name][0]).sum()))
        else:
            assert top <= 1.0, '%s %s %s: error / bound = %.3f' % (tag, name, dtype, top)


# --------------------------------------------------------------------------------------------------------------------- #
# halo geometry of the kernels (csrc/conv_mfma.h TensorView): the flat halo-pixel index of every map pixel
# --------------------------------------------------------------------------------------------------------------------- #
def halo_index(n, h, w, p):
    """(q [n,h,w] int64, pixels): pixel (i, y, x) sits at row i * (h + p) + p + y, column p + x of rows w + p long."""
    i, y, x = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), indexing='ij')
    q = (i * (h + p) + p + y) * (w + p) + p + x
    return q.astype(np.int64), (n * (h + p) + p) * (w + p) + p


def dw_emulate32(xs, dz, k, rate, order='pixel', slices=1):
    """The weight gradient accumulated in float32: products one pixel at a time in flat halo order ('pixel'), in reverse
    ('reverse'), or 32-pixel steps summed first ('step'); the pixel range cut into `slices` partial sums added in slice order."""
    xs, dz = np.asarray(xs, np.float32), np.asarray(dz, np.float32)
    n, h, w, cin = xs.shape
    cout = dz.shape[3]
    p = (k - 1) * rate // 2
    xp = np.pad(xs, ((0, 0), (p, p), (p, p), (0, 0)))
    q, pixels = halo_index(n, h, w, p)
    steps = -(-pixels // STEP)
    per = -(-steps // slices)
    sl = (q // STEP // per).reshape(-1)
    zf = dz.reshape(-1, cout)
    out = np.zeros((k, k, cin, cout), np.float32)
    for ky in range(k):
        for kx in range(k):
            xf = xp[:, ky * rate: ky * rate + h, kx * rate: kx * rate + w, :].reshape(-1, cin)
            total = np.zeros((cin, cout), np.float32)
            for s in range(int(sl.max()) + 1):
                idx = np.nonzero(sl == s)[0]
                if order == 'reverse':
                    idx = idx[::-1]
                acc = np.zeros((cin, cout), np.float32)
                if order == 'step':
                    for c0 in range(0, len(idx), STEP):
                        j = idx[c0:c0 + STEP]
                        acc += (xf[j].T.astype(F64) @ zf[j].astype(F64)).astype(np.float32)
                else:
                    for j in idx:
                        acc += np.outer(xf[j], zf[j])
                total += acc
            out[ky, kx] = total
    return out


# --------------------------------------------------------------------------------------------------------------------- #
# mutants: one wrong decision each; outputs as the entry point would deliver them
# --------------------------------------------------------------------------------------------------------------------- #
MUTANTS = ('taps_not_flipped', 'not_swapped', 'mask_dy', 'mask_dropped', 'dz_unrounded', 'halo_wrap', 'last_step_dropped',
           'slice_dropped', 'db_unrounded', 'dilation_ignored')


def _wrapped(xs, dz, ws, k, rate):
    """Halo not zero: the tensors as DENSE pixel lists, a tap that leaves a row lands in the neighbouring row / image."""
    n, h, w, cin = xs.shape
    cout = dz.shape[3]
    p = (k - 1) * rate // 2
    xf, zf = np.asarray(xs, F64).reshape(-1, cin), np.asarray(dz, F64).reshape(-1, cout)
    m = xf.shape[0]

    def shift(a, o):          # b[i] = a[i + o], zero outside the list
        b = np.zeros_like(a)
        if o >= 0:
            b[:m - o] = a[o:] if o < m else 0
        else:
            b[-o:] = a[:m + o] if -o < m else 0
        return b
    dw = np.zeros((k, k, cin, cout), F64)
    dx = np.zeros((m, cin), F64)
    wf = flipped(ws).astype(F64)
    for ky in range(k):
        for kx in range(k):
            o = (ky * rate - p) * w + (kx * rate - p)
            if abs(o) < m:
                dw[ky, kx] = shift(xf, o).T @ zf
                dx += shift(zf, o) @ wf[ky, kx]
    return dx.reshape(xs.shape), dw


def mutant(name, x, w, y, dy, dtype, relu, rate):
    """(dx, dw, db) float32 of the mutated operator (name None: the operator itself), or None where the mutant changes nothing by
    construction (e.g. 'dilation_ignored' at dilation 1)."""
    k = w.shape[0]
    n, h, wd, cin = x.shape
    cout = w.shape[3]
    rnd = ROUND[dtype]
    mask = {'mask_dy': 'dy', 'mask_dropped': 'none'}.get(name, 'y')
    if name in ('mask_dy', 'mask_dropped') and not relu:
        return None
    xs, ws, dz = seen(x, w, y, dy, dtype, relu, mask=mask, round_dz=name != 'dz_unrounded')
    use_rate = rate
    if name == 'dilation_ignored':
        if rate == 1:
            return None
        use_rate = 1
    g = grads64(xs, ws, dz, use_rate)
    dx, dw, db = g['dx'][0], g['dw'][0], g['db'][0]
    if name == 'taps_not_flipped':
        if k == 1:
            return None
        dx = cb.conv64(dz, np.asarray(ws).transpose(0, 1, 3, 2), rate=rate)
    elif name == 'not_swapped':
        if cin != cout:
            return None
        dx = cb.conv64(dz, np.flip(np.asarray(ws), (0, 1)), rate=rate)
    elif name == 'halo_wrap':
        if k == 1:
            return None
        dx, dw = _wrapped(xs, dz, ws, k, rate)
    elif name in ('last_step_dropped', 'slice_dropped'):
        q, pixels = halo_index(n, h, wd, (k - 1) * rate // 2)
        steps = -(-pixels // STEP)
        if name == 'last_step_dropped':
            if pixels % STEP == 0:
                return None
            keep = q // STEP < steps - 1
        else:
            if steps < 2:
                return None
            keep = q // STEP < -(-steps // 2)          # the second of two slices is lost
        dw = dw64(xs, np.where(keep[..., None], dz, np.float32(0)), k, rate)
    elif name == 'db_unrounded':
        db = seen(x, w, y, dy, dtype, relu, round_dz=False)[2].astype(F64).sum(axis=(0, 1, 2))
    return rnd(dx.astype(np.float32)), dw.astype(np.float32), db.astype(np.float32)
