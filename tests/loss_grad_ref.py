"""CPU references of the gradient of RONNet.losses with respect to the head tensors (ron_losses_grad; no GPU, no TensorFlow).

  * ``grads_ref``       float64, analytic, on flat float32 inputs; the sets come from encode_ref.loss_masks, the smooth-L1 branch is
                        taken on the float32 difference as the forward takes it.
  * ``grads_torch``     the second, independent reference: torch-CPU float64 autograd through a torch restatement of the loss on the
                        same masks (cross_entropy; modified_smooth_l1 as nets/custom_layers.py:31-49 writes it, its 0 / 1 `sign`
                        tensor a constant).
  * ``grads_emulated``  float32 emulation of the kernel's arithmetic, with the mutants of ``MUTANTS`` as switches.
  * ``grad_bound``      bound of |kernel - float64 reference| per element of the class and objectness gradients (DESIGN.md section
                        4.3, "Loss gradients").  The localisation gradient needs none: it is a chain of single, correctly rounded
                        float32 operations and must equal the emulation bit for bit.

Every function returns a dict with 'd_cls' [rows, C], 'd_obj' [rows, 2], 'd_loc' [rows, 4], 'scales' [3] (class, objectness,
localisation), 'square' (bool [rows, 4]: the coordinates in the quadratic branch), 'counts' and 'masks'.
"""
import numpy as np

import encode_ref as er

F = np.float32
U = 2.0 ** -24
EXP_ULP = 2.0           # accuracy granted to the device's expf, in ulp of its result (DESIGN.md section 4.3 grants the forward the same)
MUTANTS = ('keep_one_hot', 'mean_all_rows', 'le_kink', 'ignored_as_negative', 'loc_all_positives', 'no_zero_scale', 'no_max')
ONE_NINTH = F(1.0) / F(9.0)


def _masks(gclasses, objness_pred, rand_obj, rand_cls, objness_threshold, negative_ratio):
    return er.loss_masks(gclasses, objness_pred, rand_obj, rand_cls, objness_threshold, negative_ratio)


def _labels(mk, C):
    """Clipped class label per row (C = out of range: the row is NaN) and objectness label per row."""
    return np.clip(mk['g'], 0, C).astype(np.int64), mk['pos'].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ float64, analytic
def _softmax_grad64(x32, label, s):
    x = np.asarray(x32, F).astype(np.float64)
    C = x.shape[1]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    onehot = (np.arange(C)[None, :] == label[:, None]).astype(np.float64)
    with np.errstate(invalid='ignore'):
        g = (p - onehot) * s
    g[label >= C] = np.nan
    return g, p


def grads_ref(logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_obj, rand_cls,
              objness_threshold=0.03, negative_ratio=3., alpha=1. / 3, beta=1. / 3):
    x, xo = np.asarray(logits, F), np.asarray(objness_logits, F)
    rows, C = x.shape
    mk = _masks(gclasses, objness_pred, rand_obj, rand_cls, objness_threshold, negative_ratio)
    n_pos, n_cls_pos, n_obj_set, n_cls_set = (int(mk['counts'][i]) for i in (0, 2, 4, 5))
    w_cls, w_obj, w_loc = er._loss_weights(alpha, beta)
    with np.errstate(divide='ignore', invalid='ignore'):
        s_cls = np.float64(w_cls) / np.float64(n_cls_set) if n_pos > 0 else np.float64(0)
        s_obj = np.float64(w_obj) / np.float64(n_obj_set) if n_pos > 0 else np.float64(0)
        s_loc = np.float64(w_loc) / np.float64(n_cls_pos) if n_cls_pos > 0 else np.float64(0)
    lab, olab = _labels(mk, C)
    d_cls, d_obj, d_loc = np.zeros((rows, C)), np.zeros((rows, 2)), np.zeros((rows, 4))
    p_cls, p_obj = np.zeros((rows, C)), np.zeros((rows, 2))
    cs, os_, lp = mk['cls_set'], mk['obj_set'], mk['cls_pos']
    if cs.any():
        d_cls[cs], p_cls[cs] = _softmax_grad64(x[cs], lab[cs], s_cls)
    if os_.any():
        d_obj[os_], p_obj[os_] = _softmax_grad64(xo[os_], olab[os_], s_obj)
    d32 = np.asarray(localisations, F) - np.asarray(glocalisations, F)
    with np.errstate(invalid='ignore'):
        square = np.abs(d32) < ONE_NINTH
    d64 = np.asarray(localisations, F).astype(np.float64) - np.asarray(glocalisations, F).astype(np.float64)
    with np.errstate(invalid='ignore'):
        d_loc[lp] = np.where(square[lp], 9.0 * d64[lp], np.copysign(1.0, d64[lp])) * s_loc
    return dict(d_cls=d_cls, d_obj=d_obj, d_loc=d_loc, scales=np.array([s_cls, s_obj, s_loc]), square=square, counts=mk['counts'],
                masks=mk, softmax=(p_cls, p_obj), labels=(lab, olab))


# ------------------------------------------------------------------------------------------------------------ float64, torch autograd
def grads_torch(logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_obj, rand_cls,
                objness_threshold=0.03, negative_ratio=3., alpha=1. / 3, beta=1. / 3):
    """d (each term) / d (its head tensor) by torch-CPU float64 autograd.  Rows whose label is out of range are left out of the sum
    (torch refuses them) and keep the set's size in the mean; their gradient rows are returned as NaN."""
    import torch
    import torch.nn.functional as TF
    mk = _masks(gclasses, objness_pred, rand_obj, rand_cls, objness_threshold, negative_ratio)
    C = np.asarray(logits).shape[1]
    n_pos, n_cls_pos, n_obj_set, n_cls_set = (int(mk['counts'][i]) for i in (0, 2, 4, 5))
    w_cls, w_obj, w_loc = er._loss_weights(alpha, beta)
    lab, olab = _labels(mk, C)
    leaf = lambda a: torch.from_numpy(np.asarray(a, F).astype(np.float64)).requires_grad_(True)
    x, xo, pl = leaf(logits), leaf(objness_logits), leaf(localisations)
    tl = torch.from_numpy(np.asarray(glocalisations, F).astype(np.float64))
    valid = mk['cls_set'] & (lab < C)
    total = torch.zeros((), dtype=torch.float64)
    if n_pos > 0 and valid.any():
        sel = torch.from_numpy(valid)
        total = total + w_cls * TF.cross_entropy(x[sel], torch.from_numpy(lab)[sel], reduction='sum') / n_cls_set
    if n_pos > 0 and mk['obj_set'].any():
        sel = torch.from_numpy(mk['obj_set'])
        total = total + w_obj * TF.cross_entropy(xo[sel], torch.from_numpy(olab)[sel], reduction='mean')
    if n_cls_pos > 0:
        sel = torch.from_numpy(mk['cls_pos'])
        with np.errstate(invalid='ignore'):
            sign = torch.from_numpy((np.abs(np.asarray(localisations, F) - np.asarray(glocalisations, F)) < ONE_NINTH)
                                    .astype(np.float64))[sel]              # tf.cast(tf.less(...)): a constant of the graph
        sigma2 = 9.0
        diff = pl[sel] - tl[sel]
        opt1 = (diff * diff) * (0.5 * sigma2)
        opt2 = diff.abs() - 0.5 / sigma2
        res = opt1 * sign + opt2 * (sign - 1.0).abs()
        total = total + w_loc * res.sum(dim=1).mean()
    if total.requires_grad:
        total.backward()
    g = [t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape)) for t in (x, xo, pl)]
    g[0][mk['cls_set'] & (lab >= C)] = np.nan
    return dict(d_cls=g[0], d_obj=g[1], d_loc=g[2])


# ------------------------------------------------------------------------------------------------------------ float32 emulation
def _softmax_grad32(x32, label, s, mut):
    x = np.asarray(x32, F)
    C = x.shape[1]
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        mx = x.max(axis=1) if 'no_max' not in mut else np.zeros(x.shape[0], F)
        e = np.exp(x - mx[:, None])
        tot = np.zeros(x.shape[0], F)
        for i in range(C):                                  # in index order, as cross_entropy of csrc/targets.hip adds them
            tot = tot + e[:, i]
        p = e / tot[:, None]
        onehot = (np.arange(C)[None, :] == label[:, None]).astype(F)
        q = p if 'keep_one_hot' in mut else p - onehot
        g = q * F(s)
    assert e.dtype == F and p.dtype == F and g.dtype == F
    g[label >= C] = np.nan
    return g


def grads_emulated(logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_obj, rand_cls,
                   objness_threshold=0.03, negative_ratio=3., alpha=1. / 3, beta=1. / 3, mut=()):
    x, xo = np.asarray(logits, F), np.asarray(objness_logits, F)
    rows, C = x.shape
    g_in = np.asarray(gclasses).reshape(-1)
    if 'ignored_as_negative' in mut:
        g_in = np.maximum(g_in, 0)
    mk = _masks(g_in, objness_pred, rand_obj, rand_cls, objness_threshold, negative_ratio)
    n_pos, n_cls_pos, n_obj_set, n_cls_set = (int(mk['counts'][i]) for i in (0, 2, 4, 5))
    loc_rows = mk['pos'] if 'loc_all_positives' in mut else mk['cls_pos']
    n_loc = n_pos if 'loc_all_positives' in mut else n_cls_pos
    if 'mean_all_rows' in mut:
        n_cls_set = n_obj_set = n_loc = rows
    w_cls, w_obj, w_loc = (F(w) for w in er._loss_weights(alpha, beta))
    keep = 'no_zero_scale' in mut
    with np.errstate(divide='ignore', invalid='ignore'):
        s_cls = w_cls / F(n_cls_set) if (n_pos > 0 or keep) else F(0)
        s_obj = w_obj / F(n_obj_set) if (n_pos > 0 or keep) else F(0)
        s_loc = w_loc / F(n_loc) if (n_loc > 0 or keep) else F(0)
    lab, olab = _labels(mk, C)
    d_cls, d_obj, d_loc = np.zeros((rows, C), F), np.zeros((rows, 2), F), np.zeros((rows, 4), F)
    cs, os_ = mk['cls_set'], mk['obj_set']
    if cs.any():
        d_cls[cs] = _softmax_grad32(x[cs], lab[cs], s_cls, mut)
    if os_.any():
        d_obj[os_] = _softmax_grad32(xo[os_], olab[os_], s_obj, mut)
    d = np.asarray(localisations, F) - np.asarray(glocalisations, F)
    with np.errstate(invalid='ignore'):
        square = (np.abs(d) <= ONE_NINTH) if 'le_kink' in mut else (np.abs(d) < ONE_NINTH)
        val = np.where(square, (F(9.0) * d) * s_loc, np.copysign(F(1.0), d) * s_loc)
    assert val.dtype == F
    d_loc[loc_rows] = val[loc_rows]
    return dict(d_cls=d_cls, d_obj=d_obj, d_loc=d_loc, scales=np.array([s_cls, s_obj, s_loc], F), square=square, counts=mk['counts'],
                masks=mk)


# ------------------------------------------------------------------------------------------------------------ the bound
def _rows_bound(x32, label, s64, p64):
    """Per element of (softmax(x)[k] - [k == l]) * s for rows x [R, C], against the float64 value.  With u = 2^-24, m = max x,
    z_k = x_k - m, e_k = exp(z_k), S = sum e_k, p_k = e_k / S, q_k = p_k - [k == l]:
        fl(x_k - m)         one rounding: the argument of expf is off by u |z_k|, so e_k by a factor exp(u |z_k|): u |z_k| (1 + 1e-4)
        expf                EXP_ULP ulp of its result, an ulp being at most 2u relative: a_k = u |z_k| + 2 EXP_ULP u relative on e_k,
                            and 2^-126 absolute where the result is subnormal (it may be flushed to zero)
        the sum             C - 1 ordered additions of positive terms: r = sum_k e_k a_k / S + (C - 1) u relative on S
        e_k / S             a correctly rounded division (v_div_scale / v_div_fmas / v_div_fixup: IEEE; no reciprocal sequence): u
                            so p_k is off by p_k (a_k + r + u), second-order terms covered by the factor 1.0001
        p_k - [k == l]      one subtraction: u |q_k|  (exact for k != l)
        * s                 s = fl(w / n) carries u, the product u: 2u |q_k s|, plus 2^-126 where the product is subnormal
    (the quotient likewise: 2^-126).
    """
    x = np.asarray(x32, F).astype(np.float64)
    C = x.shape[1]
    z = x - x.max(axis=1, keepdims=True)
    e = np.exp(z)
    S = e.sum(axis=1, keepdims=True)
    a = U * np.abs(z) + 2 * EXP_ULP * U
    r = (e * a).sum(axis=1, keepdims=True) / S + (C - 1) * U
    onehot = (np.arange(C)[None, :] == label[:, None]).astype(np.float64)
    q = np.abs(p64 - onehot)
    s = abs(float(s64))
    tiny = 2.0 ** -126
    with np.errstate(invalid='ignore', over='ignore'):
        b = s * ((p64 * (a + r + U) + tiny / S + tiny) * 1.0001 + U * q) + 2 * U * q * s + tiny
    return b


def grad_bound(logits, objness_logits, ref):
    """(bound_cls [rows, C], bound_obj [rows, 2]) for a result of grads_ref; 0 outside the sets (those elements are exactly 0)."""
    x, xo = np.asarray(logits, F), np.asarray(objness_logits, F)
    mk = ref['masks']
    lab, olab = ref['labels']
    b_cls, b_obj = np.zeros(x.shape), np.zeros(xo.shape)
    cs, os_ = mk['cls_set'], mk['obj_set']
    if cs.any():
        b_cls[cs] = _rows_bound(x[cs], lab[cs], ref['scales'][0], ref['softmax'][0][cs])
    if os_.any():
        b_obj[os_] = _rows_bound(xo[os_], olab[os_], ref['scales'][1], ref['softmax'][1][os_])
    return b_cls, b_obj


def within(got, ref, bound):
    """got within bound of ref; NaN exactly where ref is NaN."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return bool((np.abs(got - ref)[~nan] <= bound[~nan]).all())
