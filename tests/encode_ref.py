"""CPU references of RONNet.bboxes_encode and RONNet.losses (no GPU, no TensorFlow).

Encode, twice:
  * ``encode_np``     vectorised numpy float32, operation by operation what the reference's graph computes:
                      tf_ssd_bboxes_encode (nets/ssd_common.py:337-414: the anchors re-derived from their corners, :372-388),
                      tf_ssd_bboxes_encode_layer (:77-147), do_dual_max_match (:49-75), iou_matrix (:27-47).
                      It takes a set of mutant names (``MUTANTS``): each one breaks one decision; tests/encode_cases.py holds a
                      case for every one of them.
  * ``encode_scalar`` plain loops, one anchor and one box at a time, written from the prose description of the matching rules
                      and not from ``encode_np``.
Losses: ``losses_ref`` evaluates ron_losses (nets/ron_vgg_320.py:635-778) with modified_smooth_l1 (nets/custom_layers.py:31-49) in
float64 on the float32 inputs, every mask taken in float32 as the reference takes it; ``losses_bound`` is the error bound of the
float32 kernels against it; ``losses_emulated`` is a CPU emulation of the kernels' arithmetic with two mutants.
"""
import numpy as np

F = np.float32
RON_MAX_GT = 256
MUTANTS = ('high_strict', 'last_gt', 'last_anchor', 'no_claims', 'no_inside', 'le_max', 'keep_padding')
LOGF_ULP = 2.0          # accuracy assumed for the device's logf, in ulp of its result


# ------------------------------------------------------------------------------------------------------------ anchors
class AnchorTable(object):
    """The flat per-image anchor list (layers in the order given, inside a layer row, column, anchor)."""

    def __init__(self, anchors, allowed_borders, img_shape):
        self.shapes = [(int(y.shape[0]), int(y.shape[1]), int(np.size(h))) for (y, x, h, w) in anchors]
        self.sizes = [a * b * c for (a, b, c) in self.shapes]
        self.total = int(sum(self.sizes))
        self.raw = [tuple(np.asarray(t, F) for t in layer) for layer in anchors]
        yc, xc, hh, ww, lo_y, lo_x, hi_y, hi_x = [], [], [], [], [], [], [], []
        H, W = int(img_shape[0]), int(img_shape[1])
        for (y, x, h, w), b in zip(self.raw, allowed_borders):
            y, x = y.reshape(y.shape[0], y.shape[1], 1), x.reshape(x.shape[0], x.shape[1], 1)
            # ssd_common.py:375-381: numpy float32 (a Python 2. does not widen a float32 array)
            ymin_, xmin_, ymax_, xmax_ = y - h / 2., x - w / 2., y + h / 2., x + w / 2.
            for dst, v in ((yc, (ymin_ + ymax_) / 2), (xc, (xmin_ + xmax_) / 2), (hh, ymax_ - ymin_), (ww, xmax_ - xmin_)):
                assert v.dtype == F
                dst.append(v.reshape(-1))
            n = yc[-1].size
            # :112-115: Python float (double) arithmetic, then the comparison's operand becomes float32
            lo_y.append(np.full(n, F(-b * 1. / H))); lo_x.append(np.full(n, F(-b * 1. / W)))
            hi_y.append(np.full(n, F((H + b) * 1. / H))); hi_x.append(np.full(n, F((W + b) * 1. / W)))
        self.yc, self.xc, self.h, self.w = (np.concatenate(v) for v in (yc, xc, hh, ww))
        self.lo_y, self.lo_x, self.hi_y, self.hi_x = (np.concatenate(v) for v in (lo_y, lo_x, hi_y, hi_x))
        # :105-108
        self.ymin, self.xmin = self.yc - self.h / 2., self.xc - self.w / 2.
        self.ymax, self.xmax = self.yc + self.h / 2., self.xc + self.w / 2.
        assert self.ymin.dtype == F and self.lo_y.dtype == F

    def inside(self, mut=()):
        if 'no_inside' in mut:
            return np.ones(self.total, bool)
        if 'le_max' in mut:
            return (self.ymin >= self.lo_y) & (self.xmin >= self.lo_x) & (self.ymax <= self.hi_y) & (self.xmax <= self.hi_x)
        return (self.ymin >= self.lo_y) & (self.xmin >= self.lo_x) & (self.ymax < self.hi_y) & (self.xmax < self.hi_x)

    def split(self, flat, n=None):
        """[N, total, ...] (or [total, ...]) -> per-layer list [N, H, W, A, ...]."""
        out, o = [], 0
        for (fh, fw, a), sz in zip(self.shapes, self.sizes):
            if n is None:
                out.append(flat[o:o + sz].reshape((fh, fw, a) + flat.shape[1:]))
            else:
                out.append(flat[:, o:o + sz].reshape((n, fh, fw, a) + flat.shape[2:]))
            o += sz
        return out


def present_rows(labels):
    """Rows in front of the first padding row (label 0)."""
    z = np.flatnonzero(np.asarray(labels) == 0)
    return int(z[0]) if z.size else int(np.size(labels))


# ------------------------------------------------------------------------------------------------------------ encode, vectorised
def overlap_matrix(bboxes, tab, mut=()):
    """iou_matrix(bboxes, anchors) * inside (ssd_common.py:27-47, :118): [G, total] float32."""
    bb = np.asarray(bboxes, F).reshape(-1, 4)
    gy0, gx0, gy1, gx1 = (bb[:, i:i + 1] for i in range(4))
    ih = np.maximum(np.minimum(gy1, tab.ymax[None]) - np.maximum(gy0, tab.ymin[None]), F(0))
    iw = np.maximum(np.minimum(gx1, tab.xmax[None]) - np.maximum(gx0, tab.xmin[None]), F(0))
    inter = ih * iw
    area_g = (gx1 - gx0) * (gy1 - gy0)
    area_a = ((tab.xmax - tab.xmin) * (tab.ymax - tab.ymin))[None]
    union = (area_g + area_a) - inter
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = np.where(union == 0, F(0), inter / union)
    ov = iou * tab.inside(mut).astype(F)[None]
    assert ov.dtype == F
    return ov


def _first_max(a, axis, last=False):
    if not last:
        return np.argmax(a, axis=axis)
    n = a.shape[axis]
    return n - 1 - np.argmax(np.flip(a, axis=axis), axis=axis)


def encode_np(labels, bboxes, tab, positive_threshold=0.5, ignore_threshold=0.3, prior_scaling=(0.1, 0.1, 0.2, 0.2), mut=()):
    """One image: flat (gclasses int64 [T], glocalisations [T, 4], gscores [T], gbboxes [T, 4], match index [T])."""
    labels = np.asarray(labels, np.int64).reshape(-1)
    bboxes = np.asarray(bboxes, F).reshape(-1, 4)
    g = labels.size if 'keep_padding' in mut else present_rows(labels)
    T = tab.total
    corners = np.stack([tab.ymin, tab.xmin, tab.ymax, tab.xmax], axis=-1)
    if g == 0:                  # the defined extension: no box, every anchor negative
        return np.zeros(T, np.int64), np.zeros((T, 4), F), np.zeros(T, F), corners, np.full(T, -1, np.int64)
    labels, bboxes = labels[:g], bboxes[:g]
    high, low = F(positive_threshold), F(ignore_threshold)
    ov = overlap_matrix(bboxes, tab, mut)
    # do_dual_max_match :53-63
    best_gt = _first_max(ov, 0, last='last_gt' in mut)
    match = ov.max(axis=0)
    less = match < low
    between = ((match <= high) if 'high_strict' in mut else (match < high)) & (match >= low)
    m = np.where(less, -1, best_gt)
    m = np.where(between, -2, m)
    score = match
    # :67-75, gt_max_first
    if 'no_claims' not in mut:
        best_anchor = _first_max(ov, 1, last='last_anchor' in mut)
        claim = np.full(T, g, np.int64)
        np.minimum.at(claim, best_anchor, np.arange(g))
        claimed = claim < g
        m = np.where(claimed, claim, m)
        score = np.where(claimed, ov[np.minimum(claim, g - 1), np.arange(T)], match)
    # tf_ssd_bboxes_encode_layer :123-147
    row = np.maximum(m, 0)
    mask = m > -1
    gclasses = labels[row] * mask.astype(np.int64) + (-1 * (m < -1).astype(np.int64))
    fy0, fx0, fy1, fx1 = (bboxes[row, i] for i in range(4))
    ps = [F(p) for p in prior_scaling]
    with np.errstate(divide='ignore', invalid='ignore'):
        cy = ((fy1 + fy0) / F(2) - tab.yc) / tab.h / ps[0]
        cx = ((fx1 + fx0) / F(2) - tab.xc) / tab.w / ps[1]
        fh = np.log((fy1 - fy0) / tab.h) / ps[2]
        fw = np.log((fx1 - fx0) / tab.w) / ps[3]
        gloc = mask.astype(F)[:, None] * np.stack([cx, cy, fw, fh], axis=-1)
    assert gloc.dtype == F and score.dtype == F
    return gclasses, gloc, score.astype(F), corners, m.astype(np.int64)


def encode_batch(glabels, gbboxes, tab, fn=None, **kw):
    """A padded batch [N, G] / [N, G, 4] -> the four per-layer lists [N, H, W, A, ...] (fn: encode_np or encode_scalar)."""
    fn = fn or encode_np
    glabels, gbboxes = np.asarray(glabels), np.asarray(gbboxes, F)
    per = [fn(glabels[i], gbboxes[i], tab, **kw)[:4] for i in range(glabels.shape[0])]
    n = len(per)
    return tuple(tab.split(np.stack([p[k] for p in per]), n) for k in range(4))


# ------------------------------------------------------------------------------------------------------------ encode, scalar
def encode_scalar(labels, bboxes, tab, positive_threshold=0.5, ignore_threshold=0.3, prior_scaling=(0.1, 0.1, 0.2, 0.2)):
    """The same function from its description, one anchor and one box at a time (float32 scalars)."""
    two, zero = F(2), F(0)
    high, low = F(positive_threshold), F(ignore_threshold)
    ps = [F(p) for p in prior_scaling]
    boxes = []
    for lab, bb in zip(np.asarray(labels).reshape(-1), np.asarray(bboxes, F).reshape(-1, 4)):
        if int(lab) == 0:
            break
        boxes.append((int(lab), F(bb[0]), F(bb[1]), F(bb[2]), F(bb[3])))
    # anchors from the raw per-layer (y, x, h, w), in order
    anchors = []
    for li, (y, x, h, w) in enumerate(tab.raw):
        lo_y, lo_x, hi_y, hi_x = None, None, None, None
        fh, fw, na = tab.shapes[li]
        y, x = y.reshape(fh, fw), x.reshape(fh, fw)
        o = sum(tab.sizes[:li])
        lo_y, lo_x, hi_y, hi_x = tab.lo_y[o], tab.lo_x[o], tab.hi_y[o], tab.hi_x[o]
        for r in range(fh):
            for c in range(fw):
                for k in range(na):
                    ay, ax, ah, aw = F(y[r, c]), F(x[r, c]), F(h[k]), F(w[k])
                    t0, l0, b0, r0 = ay - ah / two, ax - aw / two, ay + ah / two, ax + aw / two
                    yc, xc, hh, ww = (t0 + b0) / two, (l0 + r0) / two, b0 - t0, r0 - l0
                    top, left, bot, right = yc - hh / two, xc - ww / two, yc + hh / two, xc + ww / two
                    ins = bool(top >= lo_y and left >= lo_x and bot < hi_y and right < hi_x)
                    anchors.append((yc, xc, hh, ww, top, left, bot, right, ins))
    T = len(anchors)
    gclasses = np.zeros(T, np.int64)
    gloc = np.zeros((T, 4), F)
    gscores = np.zeros(T, F)
    corners = np.array([[a[4], a[5], a[6], a[7]] for a in anchors], F).reshape(T, 4)
    index = np.full(T, -1, np.int64)
    if not boxes:
        return gclasses, gloc, gscores, corners, index

    def iou(box, a):
        _, gy0, gx0, gy1, gx1 = box
        if not a[8]:
            return zero
        ih = min(gy1, a[6]) - max(gy0, a[4])
        iw = min(gx1, a[7]) - max(gx0, a[5])
        ih = ih if ih > zero else zero
        iw = iw if iw > zero else zero
        inter = F(ih * iw)
        union = F(F((gx1 - gx0) * (gy1 - gy0)) + F((a[7] - a[5]) * (a[6] - a[4]))) - inter
        return zero if union == zero else F(inter / union)

    best_of_box = [(-1.0, -1)] * len(boxes)           # (overlap, anchor): the lowest anchor of maximal overlap
    per_anchor = []
    for ai, a in enumerate(anchors):
        best, best_g = None, -1
        for gi, box in enumerate(boxes):
            v = iou(box, a)
            if best is None or v > best:
                best, best_g = v, gi
            if v > best_of_box[gi][0]:
                best_of_box[gi] = (v, ai)
        per_anchor.append((best, best_g))
    claimed_by = {}
    for gi in range(len(boxes) - 1, -1, -1):          # the lowest box is written last and wins
        claimed_by[best_of_box[gi][1]] = gi
    with np.errstate(divide='ignore', invalid='ignore'):
        for ai, a in enumerate(anchors):
            match, m = per_anchor[ai]
            score = match
            if ai in claimed_by:
                m = claimed_by[ai]
                score = iou(boxes[m], a)
            elif match < low:
                m = -1
            elif match < high:
                m = -2
            index[ai] = m
            gscores[ai] = score
            lab, gy0, gx0, gy1, gx1 = boxes[max(m, 0)]
            gclasses[ai] = lab if m > -1 else (-1 if m < -1 else 0)
            keep = F(1) if m > -1 else F(0)
            cy = F(F(F(F(gy1 + gy0) / two - a[0]) / a[2]) / ps[0])
            cx = F(F(F(F(gx1 + gx0) / two - a[1]) / a[3]) / ps[1])
            th = F(np.log(F((gy1 - gy0) / a[2])) / ps[2])
            tw = F(np.log(F((gx1 - gx0) / a[3])) / ps[3])
            gloc[ai] = [keep * cx, keep * cy, keep * tw, keep * th]
    return gclasses, gloc, gscores, corners, index


# ------------------------------------------------------------------------------------------------------------ the w / h bound
def loc_reference64(gbboxes_row, tab, index, prior_scaling=(0.1, 0.1, 0.2, 0.2)):
    """float64 value of the w / h targets on the same float32 inputs, and the per-element bound of a float32 evaluation
    ("Encode: the w / h targets"):
        q  = fl(g / a)              one rounding: q = (g / a)(1 + d), |d| <= 2^-24, i.e. at most 2^-24 (1 + 2^-24) behind the logarithm
        L  = logf(q)                LOGF_ULP ulp of L
        v  = fl(L / ps)             one rounding: 2^-24 |v|
    Returns (w64, h64, bound_w, bound_h) for the anchors with index > -1 (NaN elsewhere)."""
    bb = np.asarray(gbboxes_row, F).reshape(-1, 4)
    row = np.maximum(index, 0)
    ps = [float(F(p)) for p in prior_scaling]
    out = []
    with np.errstate(divide='ignore', invalid='ignore'):
        for lo, hi, size, p in ((1, 3, tab.w, ps[3]), (0, 2, tab.h, ps[2])):
            g32 = bb[row, hi] - bb[row, lo]               # fl(max - min): an input of the formula, as the kernel forms it
            L = np.log(g32.astype(np.float64) / size.astype(np.float64))
            v = L / p
            ulp = np.spacing(np.abs(L).astype(F)).astype(np.float64)
            bound = (2.0 ** -24 * (1 + 2.0 ** -24) + LOGF_ULP * ulp) / p * (1 + 2.0 ** -23) + 2.0 ** -24 * np.abs(v)
            out.append((np.where(index > -1, v, np.nan), np.where(index > -1, bound, np.nan)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ------------------------------------------------------------------------------------------------------------ losses
LOSS_COUNTS = ('n_pos', 'n_neg', 'n_cls_pos', 'n_cls_neg', 'n_objness_set', 'n_cls_set')


def flatten_rows(per_layer, width=None):
    """Per-layer [N, H, W, A(, width)] -> [rows(, width)] in the reference's order (:660-675: layer by layer)."""
    if width is None:
        return np.concatenate([np.asarray(t).reshape(-1) for t in per_layer])
    return np.concatenate([np.asarray(t).reshape(-1, width) for t in per_layer])


def loss_masks(gclasses, objness_pred, rand_obj, rand_cls, objness_threshold=0.03, negative_ratio=3.):
    """The sets of ron_losses, taken in float32 / integers exactly as specified.  Flat inputs.  Returns a dict."""
    g = np.asarray(gclasses).reshape(-1)
    op = np.asarray(objness_pred, F).reshape(-1)
    pos, neg = g > 0, g == 0
    n_pos, n_neg = int(pos.sum()), int(neg.sum())

    def prob(npos, nneg):
        want = int(F(negative_ratio) * F(npos))               # float32 product, truncated
        sel = min(want, nneg)
        return F(sel) / F(nneg) if nneg > 0 else F(0)        # tfe.safe_divide
    p_obj = prob(n_pos, n_neg)
    obj_set = (neg & (np.asarray(rand_obj, F) < p_obj)) | pos
    om = op > F(objness_threshold)
    cls_pos, cls_neg = pos & om, neg & om
    n_cls_pos, n_cls_neg = int(cls_pos.sum()), int(cls_neg.sum())
    p_cls = prob(n_cls_pos, n_cls_neg)
    cls_set = (cls_neg & (np.asarray(rand_cls, F) < p_cls)) | cls_pos
    counts = np.array([n_pos, n_neg, n_cls_pos, n_cls_neg, int(obj_set.sum()), int(cls_set.sum())], np.int32)
    return dict(g=g, pos=pos, neg=neg, obj_set=obj_set, cls_set=cls_set, cls_pos=cls_pos, counts=counts, p_obj=p_obj, p_cls=p_cls)


def _lse_rows(x64, label):
    mx = x64.max(axis=1)
    return np.log(np.exp(x64 - mx[:, None]).sum(axis=1)) + mx - x64[np.arange(x64.shape[0]), label]


def smooth_l1_rows(pred, target, dtype=np.float64):
    """modified_smooth_l1 with sigma 3, summed over the four coordinates.  The branch is taken on the float32 difference."""
    d32 = np.asarray(pred, F) - np.asarray(target, F)
    small = np.abs(d32) < F(1.0) / F(9.0)
    d = (np.asarray(pred, F).astype(dtype) - np.asarray(target, F).astype(dtype))
    v = np.where(small, d * d * dtype(4.5), np.abs(d) - dtype(0.5) / dtype(9.0))
    return v.sum(axis=1, dtype=dtype)


def _loss_weights(alpha, beta):
    a, b = F(alpha), F(beta)
    return float(F(1.0 - float(a) - float(b))), float(a), float(b)


def losses_ref(logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_obj, rand_cls,
               objness_threshold=0.03, negative_ratio=3., alpha=1. / 3, beta=1. / 3):
    """float64 reference on flat float32 inputs: (losses float64 [4], counts int32 [6], terms) where `terms` holds what the bound
    needs: the selected rows' float64 values."""
    x = np.asarray(logits, F)
    C = x.shape[1]
    mk = loss_masks(gclasses, objness_pred, rand_obj, rand_cls, objness_threshold, negative_ratio)
    g = np.asarray(gclasses).reshape(-1)
    n_pos, n_cls_pos = int(mk['counts'][0]), int(mk['counts'][2])
    w_cls, w_obj, w_loc = _loss_weights(alpha, beta)
    ce = _lse_rows(x[mk['cls_set']].astype(np.float64), np.clip(g[mk['cls_set']], 0, C))
    oe = _lse_rows(np.asarray(objness_logits, F)[mk['obj_set']].astype(np.float64), mk['pos'][mk['obj_set']].astype(np.int64))
    le = smooth_l1_rows(np.asarray(localisations, F)[mk['cls_pos']], np.asarray(glocalisations, F)[mk['cls_pos']])
    with np.errstate(divide='ignore', invalid='ignore'):
        l_cls = w_cls * (ce.sum() / np.float64(ce.size)) if n_pos > 0 else 0.0
        l_obj = w_obj * (oe.sum() / np.float64(oe.size)) if n_pos > 0 else 0.0
        l_loc = w_loc * (le.sum() / np.float64(le.size)) if n_cls_pos > 0 else 0.0
    out = np.array([l_cls, l_obj, l_loc, l_cls + l_obj + l_loc], np.float64)
    return out, mk['counts'], dict(ce=ce, oe=oe, le=le, masks=mk, weights=(w_cls, w_obj, w_loc))


def losses_bound(logits, localisations, objness_logits, glocalisations, terms):
    """Bound of |float32 kernel - float64 reference| for the three terms and their sum ("Losses").

    One cross-entropy row of C classes, u = 2^-24:
        x_i - max         one rounding; the argument of expf is off by u |x_i - max|, expf itself by EXP_ULP ulp
        sum of C terms    each <= 1, summed in order: (C - 1) u relative on the running sum, which is <= C
        logf              the sum's relative error e_s moves the logarithm by e_s; logf adds LOGF_ULP ulp of its result
        (L + max) - x_l   two roundings on magnitudes <= |L| + |max| + |x_l|
    One smooth-L1 row: d = fl(p - t) relative u; the square branch has three roundings on top of 2u from d (5u relative), the linear
    branch two (u |d| + u |value|); the four coordinates are added in float32 (3 u on the row's sum).
    The rows are added in float64 (per workgroup tree, then a fixed-order pass): 2^-53 * log2-depth * sum, negligible, included as
    2^-40 relative.  The mean: one rounding of the sum to float32, one division, one product with the weight: 3 u relative.
    """
    u = 2.0 ** -24
    EXP_ULP = 2.0
    mk = terms['masks']

    def ce_rows_bound(x32, label, value):
        x = x32.astype(np.float64)
        C = x.shape[1]
        mx = x.max(axis=1)
        z = x - mx[:, None]
        e = np.exp(z)
        s = e.sum(axis=1)
        # error of each exp term (relative): u |z| (argument) + EXP_ULP * 2u (ulp of a float32 is at most 2u relative) + u (z's rounding feeds |z| u, already counted)
        abs_terms = (e * (u * np.abs(z) + EXP_ULP * 2 * u)).sum(axis=1)
        rel_s = abs_terms / s + (C - 1) * u
        L = np.log(s)
        logf_err = LOGF_ULP * np.spacing(np.abs(L).astype(F)).astype(np.float64)
        tail = 2 * u * (np.abs(L) + np.abs(mx) + np.abs(x[np.arange(x.shape[0]), label]))
        return (rel_s * 1.0001 + logf_err + tail) * (1 + 1e-6)

    g_cls = np.clip(mk['g'], 0, None)
    x = np.asarray(logits, F)[mk['cls_set']]
    b_ce = ce_rows_bound(x, np.clip(g_cls[mk['cls_set']], 0, x.shape[1] - 1), terms['ce'])
    xo = np.asarray(objness_logits, F)[mk['obj_set']]
    b_oe = ce_rows_bound(xo, mk['pos'][mk['obj_set']].astype(np.int64), terms['oe'])
    p = np.asarray(localisations, F)[mk['cls_pos']].astype(np.float64)
    t = np.asarray(glocalisations, F)[mk['cls_pos']].astype(np.float64)
    d = np.abs(p - t)
    d32 = np.abs(np.asarray(localisations, F)[mk['cls_pos']] - np.asarray(glocalisations, F)[mk['cls_pos']])
    small = d32 < F(1.0) / F(9.0)
    per = np.where(small, 5 * u * d * d * 4.5, u * d + 2 * u * np.maximum(d, 0.5 / 9.0))
    b_le = per.sum(axis=1) + 3 * u * terms['le'] if per.size else np.zeros(0)
    out = []
    for (vals, b, w) in ((terms['ce'], b_ce, terms['weights'][0]), (terms['oe'], b_oe, terms['weights'][1]),
                         (terms['le'], b_le, terms['weights'][2])):
        if vals.size == 0:
            out.append(0.0)
            continue
        mean_abs = np.abs(vals).sum() / vals.size
        out.append(abs(w) * (b.sum() / vals.size + (2.0 ** -40 + 3 * u * (1 + 1e-6)) * mean_abs))
    total = sum(out) + 2 * u * sum(abs(w) * (np.abs(v).sum() / max(v.size, 1)) for v, w in
                                   zip((terms['ce'], terms['oe'], terms['le']), terms['weights']))
    return np.array(out + [total], np.float64)


def losses_emulated(logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_obj, rand_cls,
                    objness_threshold=0.03, negative_ratio=3., alpha=1. / 3, beta=1. / 3, mutant=None):
    """CPU emulation of the kernels' arithmetic: float32 rows, float64 accumulation.  Mutants: 'half_accumulate' adds the rows in
    float16, 'no_max' leaves the maximum subtraction out of the cross-entropy."""
    x = np.asarray(logits, F)
    C = x.shape[1]
    mk = loss_masks(gclasses, objness_pred, rand_obj, rand_cls, objness_threshold, negative_ratio)
    g = np.asarray(gclasses).reshape(-1)

    def ce32(x32, label):
        with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
            mx = x32.max(axis=1) if mutant != 'no_max' else np.zeros(x32.shape[0], F)
            s = np.zeros(x32.shape[0], F)
            for i in range(x32.shape[1]):
                s = s + np.exp(x32[:, i] - mx)
            return (np.log(s) + mx) - x32[np.arange(x32.shape[0]), label]

    def acc(v):
        if mutant == 'half_accumulate':
            s = np.float16(0)
            for t in v:
                s = np.float16(s + np.float16(t))
            return float(s)
        return float(np.asarray(v, np.float64).sum())
    ce = ce32(x[mk['cls_set']], np.clip(g[mk['cls_set']], 0, C - 1))
    oe = ce32(np.asarray(objness_logits, F)[mk['obj_set']], mk['pos'][mk['obj_set']].astype(np.int64))
    p, t = np.asarray(localisations, F)[mk['cls_pos']], np.asarray(glocalisations, F)[mk['cls_pos']]
    d = p - t
    sign = (np.abs(d) < F(1.0) / F(9.0)).astype(F)
    sl = (d * d) * F(4.5) * sign + (np.abs(d) - F(0.5) / F(9.0)) * np.abs(sign - F(1))
    le = ((sl[:, 0] + sl[:, 1]) + sl[:, 2]) + sl[:, 3] if sl.size else np.zeros(0, F)
    w_cls, w_obj, w_loc = (F(w) for w in _loss_weights(alpha, beta))
    n_pos, n_cls_pos = int(mk['counts'][0]), int(mk['counts'][2])
    with np.errstate(divide='ignore', invalid='ignore'):
        l_cls = w_cls * (F(acc(ce)) / F(ce.size)) if n_pos > 0 else F(0)
        l_obj = w_obj * (F(acc(oe)) / F(oe.size)) if n_pos > 0 else F(0)
        l_loc = w_loc * (F(acc(le)) / F(le.size)) if n_cls_pos > 0 else F(0)
    return np.array([l_cls, l_obj, l_loc, (l_cls + l_obj) + l_loc], F), mk['counts']
