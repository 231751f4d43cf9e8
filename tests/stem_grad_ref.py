"""Float64 reference of the stem backward (ron_conv2d_stem_backward_nhwc, include/ron_hip.h), a dense-pixel formulation that
mirrors the kernel's walk, and the mutants the tests have to kill.

Plain helper module (numpy only), built on tests/conv_grad_ref.py (`seen`, `dw64`, `grade`, `check`) and tests/conv_bounds.py, which
are shape-generic.  The operator, on operands AS THE KERNEL SEES THEM:

    xs = round(x),  dz = round(dy * (y > 0))  (relu)  or  round(dy)
    dw[ky,kx,c,co] = sum_{n,i,j} xs[n, i + ky - 1, j + kx - 1, c] * dz[n,i,j,co]      K = n * h * w, fp32, not rounded
    db[co] = sum dz[..., co]                                                          K = n * h * w

Grading: conv_bounds.ratio <= 1 per element with bound(ref, S, K, dtype, 'fp32'), no exclusions (conv_grad_ref.check); on the lattice
inputs equality.  The bound's derivation carries over unchanged: products of two storage-type values are exact in float32 and the
K float32 additions, in any order and over any pixel slices, err by at most K * 2^-23 * S.  No constant is fitted."""
import numpy as np

import conv_grad_ref as cgr

F64 = np.float64
STEP = 32          # pixels per K step of the kernel, in DENSE pixel order
_NO_W = np.zeros((1,), np.float32)


def seen(x, y, dy, dtype, relu, **kw):
    """(xs, dz) float32: what the kernel multiplies (conv_grad_ref.seen without weights)."""
    xs, _, dz = cgr.seen(x, _NO_W, y, dy, dtype, relu, **kw)
    return xs, dz


def grads64(xs, dz):
    """{'dw': (ref64, S, K), 'db': ...} from the kernel-visible operands."""
    n, h, w, _ = xs.shape
    axs, adz = np.abs(np.asarray(xs, F64)), np.abs(np.asarray(dz, F64))
    return {
        'dw': (cgr.dw64(xs, dz, 3, 1), cgr.dw64(axs, adz, 3, 1), n * h * w),
        'db': (np.asarray(dz, F64).sum(axis=(0, 1, 2)), adz.sum(axis=(0, 1, 2)), n * h * w),
    }


def dw_dense(xs, dz, row_test=True, col_test=True, keep=None):
    """The weight gradient the way the kernel walks it: flat pixel p = (img * h + row) * w + col, tap (ky, kx) reads pixel
    p + (ky - 1) * w + (kx - 1) when row + ky - 1 is a row of the map (`row_test`) and col + kx - 1 a column (`col_test`).  Without
    a test the tap lands in the neighbouring row / image (the mutants); a pixel outside the tensor reads zero.  `keep`: a mask over
    the flat pixels (lost steps / slices)."""
    n, h, w, cin = xs.shape
    cout = dz.shape[3]
    xf, zf = np.asarray(xs, F64).reshape(-1, cin), np.asarray(dz, F64).reshape(-1, cout)
    if keep is not None:
        zf = np.where(keep[:, None], zf, 0.0)
    total = n * h * w
    p = np.arange(total)
    col, row = p % w, (p // w) % h
    out = np.zeros((3, 3, cin, cout), F64)
    for ky in range(3):
        for kx in range(3):
            t = p + (ky - 1) * w + (kx - 1)
            ok = (t >= 0) & (t < total)
            if row_test:
                ok &= (row + ky - 1 >= 0) & (row + ky - 1 < h)
            if col_test:
                ok &= (col + kx - 1 >= 0) & (col + kx - 1 < w)
            out[ky, kx] = xf[np.clip(t, 0, total - 1)][ok].T @ zf[ok]
    return out


def deliver(ref):
    return {'dw': ref['dw'][0].astype(np.float32), 'db': ref['db'][0].astype(np.float32)}


MUTANTS = ('taps_flipped', 'kykx_transposed', 'k_channel_major', 'row_wrap', 'image_wrap', 'mask_dy', 'mask_dropped', 'dz_unrounded',
           'x_unrounded', 'last_step_dropped', 'slice_dropped', 'db_unrounded')
ROUNDING_MUTANTS = ('dz_unrounded', 'x_unrounded', 'db_unrounded')


def mutant(name, x, y, dy, dtype, relu):
    """{'dw', 'db'} float32 of the mutated operator (name None: the operator itself), or None where the mutant changes nothing by
    construction."""
    n, h, w, _ = x.shape
    mask = {'mask_dy': 'dy', 'mask_dropped': 'none'}.get(name, 'y')
    if name in ('mask_dy', 'mask_dropped') and not relu:
        return None
    xs, dz = seen(x, y, dy, dtype, relu, mask=mask, round_dz=name != 'dz_unrounded')
    if name == 'x_unrounded':
        xs = np.asarray(x, np.float32)
    g = grads64(xs, dz)
    dw, db = g['dw'][0], g['db'][0]
    if name == 'taps_flipped':
        dw = dw[::-1, ::-1]
    elif name == 'kykx_transposed':
        dw = dw.transpose(1, 0, 2, 3)
    elif name == 'k_channel_major':          # the GEMM's row (tap * 3 + c) stored where row (c * 9 + tap) belongs
        dw = dw.reshape(9, 3, -1).transpose(1, 0, 2).reshape(dw.shape)
    elif name == 'row_wrap':
        dw = dw_dense(xs, dz, col_test=False)
    elif name == 'image_wrap':
        dw = dw_dense(xs, dz, row_test=False)
    elif name in ('last_step_dropped', 'slice_dropped'):
        pixels = n * h * w
        steps = -(-pixels // STEP)
        step_of = np.arange(pixels) // STEP
        if name == 'last_step_dropped':
            if pixels % STEP == 0:
                return None
            keep = step_of < steps - 1
        else:
            if steps < 2:
                return None
            keep = step_of < -(-steps // 2)          # the second of two slices is lost
        dw = dw_dense(xs, dz, keep=keep)
        db = np.where(keep[:, None], np.asarray(dz, F64).reshape(pixels, -1), 0.0).sum(axis=0)
    elif name == 'db_unrounded':
        db = seen(x, y, dy, dtype, relu, round_dz=False)[1].astype(F64).sum(axis=(0, 1, 2))
    return {'dw': np.ascontiguousarray(dw).astype(np.float32), 'db': db.astype(np.float32)}
