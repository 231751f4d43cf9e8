"""Float64 references of the pool backward (ron_maxpool2x2_backward_nhwc) and of the 2x2 stride-2 convolution backwards
(ron_conv2d_k2s2_backward_nhwc, include/ron_hip.h), and the mutants the tests have to kill.

Plain helper module (numpy only), built on tests/conv_bounds.py and tests/conv_grad_ref.py.

The pool.  xs = round(x) to the storage type; the window of output (i, j) holds the positions (2i, 2j) (2i, 2j+1) (2i+1, 2j)
(2i+1, 2j+1) that exist (SAME: ceil(h/2) x ceil(w/2) windows, the last of an odd map holds one row / column); round(dy) goes to the
FIRST position in that order whose xs equals the window's maximum - a later position takes over only when it is greater (>) - and 0
to the others.  The result is exact: the tests compare with np.array_equal.

The 2x2 stride-2 operators, on operands AS THE KERNEL SEES THEM (xs, ws, dz of conv_grad_ref.seen):

    convolution   y[n,i,j,co] = sum xs[n,2i+ky,2j+kx,ci] ws[ky,kx,ci,co]
        dx = deconv64(dz, ws)                               K = cout
        dw[ky,kx,ci,co] = sum xs[n,2i+ky,2j+kx,ci] dz[n,i,j,co]     K = n (h/2) (w/2), fp32, not rounded
        db[co] = sum dz[..., co]                            K = n (h/2) (w/2)
    transposed    y[n,2i+ky,2j+kx,co] = sum xs[n,i,j,ci] ws[ky,kx,co,ci]
        dx = conv64(dz, ws, stride=2)                       K = 4 cout
        dw[ky,kx,co,ci] = sum dz[n,2i+ky,2j+kx,co] xs[n,i,j,ci]     K = n h w
        db[co] = sum dz[..., co]                            K = 4 n h w

None of it goes through the space-to-depth identity the kernels use.  Grading is conv_grad_ref.check unchanged."""
import numpy as np

import conv_bounds as cb
import conv_grad_ref as cgr

F64 = np.float64
ROUND = cgr.ROUND
STEP = cgr.STEP
ORDER = ((0, 0), (0, 1), (1, 0), (1, 1))


# --------------------------------------------------------------------------------------------------------------------- #
# the pool
# --------------------------------------------------------------------------------------------------------------------- #
def _positions(a, fill):
    """[4, n, oh, ow, c]: the four positions of every window in ORDER (`fill` where a position does not exist), and which exist."""
    n, h, w, c = a.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    p = np.full((n, 2 * oh, 2 * ow, c), fill, a.dtype)
    p[:, :h, :w] = a
    e = np.zeros((1, 2 * oh, 2 * ow, 1), bool)
    e[:, :h, :w] = True
    return (np.stack([p[:, dy::2, dx::2] for dy, dx in ORDER]), np.stack([np.broadcast_to(e[:, dy::2, dx::2], (n, oh, ow, c)) for dy, dx in ORDER]))


def _scatter(vals, shape):
    """[4, n, oh, ow, c] values per window position -> the map [n, h, w, c]"""
    n, h, w, c = shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = np.zeros((n, 2 * oh, 2 * ow, c), vals.dtype)
    for k, (dy, dx) in enumerate(ORDER):
        out[:, dy::2, dx::2] = vals[k]
    return np.ascontiguousarray(out[:, :h, :w])


POOL_MUTANTS = ('last_maximum', 'unrounded_compare', 'start_at_zero', 'edge_reads_on', 'dy_unrounded', 'ties_share')


def pool_backward(x, dy, dtype, mutant=None):
    """dx float32 [n,h,w,c], vectorised; `mutant`: one wrong decision of POOL_MUTANTS."""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    rnd = ROUND[dtype]
    xs = x if mutant == 'unrounded_compare' else rnd(x)
    n, h, w, c = x.shape
    pos, exists = _positions(xs, np.float32(0))
    if mutant == 'edge_reads_on':
        # a position that does not exist is read where it would be in memory: the next row, the next image, zero behind the tensor
        flat = np.concatenate([xs.reshape(-1), np.zeros((w + 2) * c, np.float32)])
        i, oy, ox, ch = np.meshgrid(np.arange(n), np.arange((h + 1) // 2), np.arange((w + 1) // 2), np.arange(c), indexing='ij')
        p00 = ((i * h + 2 * oy) * w + 2 * ox) * c + ch
        pos = np.stack([flat[p00 + (dy_ * w + dx_) * c] for dy_, dx_ in ORDER])
    g = dy if mutant == 'dy_unrounded' else rnd(dy)
    if mutant == 'start_at_zero':
        best, at = np.zeros_like(pos[0]), np.zeros(pos[0].shape, np.int64)
        first = 0
    else:
        best, at = pos[0].copy(), np.zeros(pos[0].shape, np.int64)
        first = 1
    for k in range(first, 4):
        live = np.ones_like(exists[k]) if mutant == 'edge_reads_on' else exists[k]
        take = live & ((pos[k] >= best) if mutant == 'last_maximum' else (pos[k] > best))
        best = np.where(take, pos[k], best)
        at = np.where(take, k, at)
    if mutant == 'ties_share':
        vals = np.stack([np.where(exists[k] & (pos[k] == best), g, np.float32(0)) for k in range(4)])
    else:
        vals = np.stack([np.where((at == k) & exists[k], g, np.float32(0)) for k in range(4)])
    return _scatter(vals.astype(np.float32), x.shape)


def pool_backward_loops(x, dy, dtype):
    """The same rule with explicit loops over windows and channels (the second, independent statement of it)."""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    xs, g = ROUND[dtype](x), ROUND[dtype](dy)
    n, h, w, c = x.shape
    dx = np.zeros(x.shape, np.float32)
    for i in range(n):
        for oy in range((h + 1) // 2):
            for ox in range((w + 1) // 2):
                for ch in range(c):
                    best, at = None, None
                    for ky, kx in ORDER:
                        yy, xx = 2 * oy + ky, 2 * ox + kx
                        if yy < h and xx < w and (best is None or xs[i, yy, xx, ch] > best):
                            best, at = xs[i, yy, xx, ch], (yy, xx)
                    dx[i, at[0], at[1], ch] = g[i, oy, ox, ch]
    return dx


def pool_ties(x, dtype):
    """(four-way ties, two-way ties of the maximum whose first member is not position (0,0)) counted over full windows."""
    pos, exists = _positions(ROUND[dtype](np.asarray(x, np.float32)), np.float32(0))
    full = exists.all(axis=0)
    top = pos.max(axis=0)
    is_top = pos == top
    count = is_top.sum(axis=0)
    four = int((full & (count == 4)).sum())
    two_late = int((full & (count == 2) & ~is_top[0]).sum())
    return four, two_late


# --------------------------------------------------------------------------------------------------------------------- #
# the 2x2 stride-2 convolution and transposed convolution
# --------------------------------------------------------------------------------------------------------------------- #
def _tap_products(fine, coarse):
    """out[ky,kx,a,b] = sum over coarse pixels of fine[n,2i+ky,2j+kx,a] * coarse[n,i,j,b]"""
    fine, coarse = np.asarray(fine, F64), np.asarray(coarse, F64)
    out = np.zeros((2, 2, fine.shape[3], coarse.shape[3]), F64)
    flat = coarse.reshape(-1, coarse.shape[3])
    for ky in range(2):
        for kx in range(2):
            out[ky, kx] = fine[:, ky::2, kx::2, :].reshape(-1, fine.shape[3]).T @ flat
    return out


def _grads(xs, ws, dz, transpose):
    if transpose:
        return cb.conv64(dz, ws, stride=2), _tap_products(dz, xs), np.asarray(dz, F64).sum(axis=(0, 1, 2))
    return cb.deconv64(dz, ws), _tap_products(xs, dz), np.asarray(dz, F64).sum(axis=(0, 1, 2))


def grads64_k2s2(xs, ws, dz, transpose):
    """{'dx': (ref64, S, K), 'dw': ..., 'db': ...} from the kernel-visible operands."""
    n, h, w, _ = np.asarray(xs).shape
    ref = _grads(xs, ws, dz, transpose)
    mag = _grads(np.abs(np.asarray(xs, F64)), np.abs(np.asarray(ws, F64)), np.abs(np.asarray(dz, F64)), transpose)
    cout = ws.shape[2] if transpose else ws.shape[3]
    if transpose:
        ks = (4 * cout, n * h * w, 4 * n * h * w)
    else:
        ks = (cout, n * (h // 2) * (w // 2), n * (h // 2) * (w // 2))
    return {name: (r, s, k) for name, r, s, k in zip(('dx', 'dw', 'db'), ref, mag, ks)}


K2S2_MUTANTS = ('taps_kx_ky', 'w_axes_swapped', 'mask_dy', 'mask_dropped', 'dz_unrounded', 'db_one_tap', 'last_step_dropped')


def k2s2_mutant(name, x, w, y, dy, dtype, relu, transpose):
    """(dx, dw, db) float32 of the mutated operator as the entry point would deliver them (name None: the operator itself), or None
    where the mutant changes nothing by construction."""
    rnd = ROUND[dtype]
    if name in ('mask_dy', 'mask_dropped') and not relu:
        return None
    mask = {'mask_dy': 'dy', 'mask_dropped': 'none'}.get(name, 'y')
    xs, ws, dz = cgr.seen(x, w, y, dy, dtype, relu, mask=mask, round_dz=name != 'dz_unrounded')
    dx, dw, db = _grads(xs, ws, dz, transpose)
    n, h, wd, cin = xs.shape
    if name == 'taps_kx_ky':
        wt = np.ascontiguousarray(np.asarray(ws).transpose(1, 0, 2, 3))
        dx, dw, _ = _grads(xs, wt, dz, transpose)
        dw = dw.transpose(1, 0, 2, 3)
    elif name == 'w_axes_swapped':
        if not transpose or ws.shape[2] != ws.shape[3]:
            return None
        dx, dw, _ = _grads(xs, np.ascontiguousarray(np.asarray(ws).transpose(0, 1, 3, 2)), dz, transpose)
        dw = dw.transpose(0, 1, 3, 2)
    elif name == 'db_one_tap':
        if not transpose:
            return None
        db = np.asarray(dz, F64)[:, 0::2, 0::2].sum(axis=(0, 1, 2))
    elif name == 'last_step_dropped':
        H, W = (h, wd) if transpose else (h // 2, wd // 2)
        pixels = n * H * W
        if pixels % STEP == 0:
            return None
        keep = (np.arange(pixels) // STEP < -(-pixels // STEP) - 1).reshape(n, H, W, 1)
        if transpose:
            dw = _tap_products(dz, np.where(keep, xs, np.float32(0)))
        else:
            dw = _tap_products(xs, np.where(keep, dz, np.float32(0)))
    return rnd(dx.astype(np.float32)), dw.astype(np.float32), db.astype(np.float32)
