"""CPU references of ron_preprocess_for_train (no GPU, no TensorFlow): preprocessing/ssd_vgg_preprocessing.py:297-356 with
ssd_random_expand, ssd_random_sample_patch and random_flip_left_right of preprocessing/tf_image.py:284-467.

The random draws are an input: RON_TRAIN_DRAWS uniform floats in [0, 1) per image at fixed slots (include/ron_hip.h).

Geometry, twice:
  * ``geometry_np``      vectorised numpy float32 over the boxes, the three tf.while_loops written as ``while condition: body`` the
                         way the graph states them.  It records a trace of every attempt and takes a set of mutant names
                         (``MUTANTS``), each of which breaks one decision; tests/train_pre_cases.py holds a case for every mutant.
  * ``geometry_scalar``  plain loops over one box at a time, written from the prose description of the rules (do-while loops, an
                         index computed per slot) and not from ``geometry_np``.
Pixels: ``pixels_ref`` materialises the float32 canvas, slices the window, flips it, resizes it with oracle.preprocess.resize_bilinear,
multiplies by 255 and subtracts the means.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.preprocess import resize_bilinear  # noqa: E402

F = np.float32
RON_MAX_GT = 256
RON_TRAIN_DRAWS = 5 + 10 * 10 * 12
RON_TRAIN_GEOM = 12
MEANS = (123., 117., 104.)
MIN_IOUS = tuple(F(v) for v in (0.4, 0.5, 0.6, 0.7, 0.8, 0.9))
GEOMETRY_MUTANTS = ('le_expand', 'le_flip', 'le_center', 'le_iou', 'ge_aspect', 'raw_window', 'sequential_draws', 'keep_padding',
                    'zero_trip')
PIXEL_MUTANTS = ('resize_before_flip', 'whiten_first')
MUTANTS = GEOMETRY_MUTANTS + PIXEL_MUTANTS
GEOM_COLUMNS = ('expanded', 'canvas_h', 'canvas_w', 'img_y', 'img_x', 'crop_y', 'crop_x', 'crop_h', 'crop_w', 'flip')

SIZE_SPAN, SIZE_MIN = F(0.999) - F(0.1), F(0.1)


def present_rows(labels):
    """Rows in front of the first padding row (label 0)."""
    z = np.flatnonzero(np.asarray(labels) == 0)
    return int(z[0]) if z.size else int(np.size(labels))


def int_draw(u, m):
    """tf.random_uniform([1], 0, m, tf.int32) from a uniform float."""
    return min(int(F(u) * F(m)), m - 1)


def size_draw(u, size):
    """tf.random_uniform([1], 0.1, 0.999)[0] * size."""
    return (F(u) * SIZE_SPAN + SIZE_MIN) * F(size)


# ------------------------------------------------------------------------------------------------------------ geometry, vectorised
class _Slots(object):
    """The draws of the patch loops: fixed slots, or (mutant) consumed one after the other."""

    def __init__(self, d, sequential):
        self.d, self.sequential, self.next = d, sequential, 5

    def attempt(self, o, c):
        self.base = 5 + (o * 10 + c) * 12

    def size_pair(self, t):
        if self.sequential:
            self.next += 2
            return self.d[self.next - 2], self.d[self.next - 1]
        return self.d[self.base + 2 * t], self.d[self.base + 2 * t + 1]

    def position(self):
        if self.sequential:
            self.next += 2
            return self.d[self.next - 2], self.d[self.next - 1]
        return self.d[self.base + 10], self.d[self.base + 11]


def jaccard(roi, b):
    """jaccard_with_anchors (tf_image.py:332-343): roi [4], b [K, 4] -> [K]."""
    ih = np.maximum(np.minimum(roi[2], b[:, 2]) - np.maximum(roi[0], b[:, 0]), F(0))
    iw = np.maximum(np.minimum(roi[3], b[:, 3]) - np.maximum(roi[1], b[:, 1]), F(0))
    inter = ih * iw
    union = (roi[3] - roi[1]) * (roi[2] - roi[0]) + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter)
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / union


def geometry_np(h, w, labels, bboxes, draws, mut=()):
    """One image.  Returns a dict: geom int32 [RON_TRAIN_GEOM], labels int32 [G], bboxes float32 [G, 4] (kept rows first, zeros
    behind), count, and trace: the attempts of the patch loops."""
    d = np.asarray(draws, F).reshape(-1)
    assert d.size == RON_TRAIN_DRAWS
    labels = np.asarray(labels, np.int32).reshape(-1)
    G = labels.size
    p = G if 'keep_padding' in mut else present_rows(labels)
    lab, b = labels[:p], np.asarray(bboxes, F).reshape(G, 4)[:p].copy()
    less = lambda x, y, site: (x <= y) if site in mut else (x < y)
    at_least_once = 'zero_trip' not in mut
    slots = _Slots(d, 'sequential_draws' in mut)
    trace = dict(attempts=[], outer=0)

    # ssd_random_expand
    expanded = not less(d[0], F(0.5), 'le_expand')
    H, W, img_y, img_x = h, w, 0, 0
    if expanded:
        img_x, img_y = int_draw(d[1], w), int_draw(d[2], h)
        H, W = 2 * h, 2 * w
        b = (b * np.array([h, w, h, w], F) + np.array([img_y, img_x, img_y, img_x], F)) / np.array([H, W, H, W], F)
    assert b.dtype == F
    fH, fW = F(H), F(W)
    iou_index = min(int(d[3] * F(6)), 5)
    min_iou = MIN_IOUS[iou_index]
    cen_x, cen_y = (b[:, 1] + b[:, 3]) / F(2), (b[:, 0] + b[:, 2]) / F(2)

    def sample_width_height(att):
        index, sw, sh = 0, fW, fH
        wide = (lambda x, y: x >= y) if 'ge_aspect' in mut else (lambda x, y: x > y)
        while ((wide(sw, sh * F(2)) or wide(sh, sw * F(2))) and index < 5) or (at_least_once and index < 1):
            u_w, u_h = slots.size_pair(index)
            sw, sh = size_draw(u_w, W), size_draw(u_h, H)
            index += 1
        att.update(sw=sw, sh=sh, tries=index)
        return int(sw), int(sh)

    def check_roi_center(o):
        index, roi, mask = 0, np.zeros(4, F), np.zeros(p, bool)
        raw = (0, 0, 0, 0)
        while (mask.sum() < 1 and index < 10) or (at_least_once and index < 1):
            att = dict(o=o, c=index)
            slots.attempt(o, index)
            isw, ish = sample_width_height(att)
            u_x, u_y = slots.position()
            x, y = int_draw(u_x, W - isw), int_draw(u_y, H - ish)
            roi = np.array([F(y) / fH, F(x) / fW, F(y + ish) / fH, F(x + isw) / fW], F)
            if 'le_center' in mut:
                mask = (cen_y >= roi[0]) & (cen_x >= roi[1]) & (cen_y <= roi[2]) & (cen_x <= roi[3])
            else:
                mask = (cen_y > roi[0]) & (cen_x > roi[1]) & (cen_y < roi[2]) & (cen_x < roi[3])
            raw = (y, x, ish, isw)
            att.update(isw=isw, ish=ish, x=x, y=y, roi=roi, mask=mask.copy(), cen_y=cen_y, cen_x=cen_x)
            trace['attempts'].append(att)
            index += 1
        return roi, mask, raw

    # check_roi_overlap
    index, roi, mask, raw = 0, np.array([0, 0, 1, 1], F), np.ones(p, bool), (0, 0, H, W)
    while (less(jaccard(roi, b[mask]), min_iou, 'le_iou').sum() > 0 and index < 10) or (at_least_once and index < 1):
        roi, mask, raw = check_roi_center(index)
        index += 1
    trace['outer'] = index
    trace['final_jaccard'] = jaccard(roi, b[mask])
    trace['min_iou'] = min_iou
    trace['roi'] = roi
    trace['canvas_boxes'] = b.copy()
    if mask.sum() > 0:
        if 'raw_window' in mut:
            win = [int(v) for v in raw]
        else:
            win = [int(roi[0] * fH), int(roi[1] * fW), int((roi[2] - roi[0]) * fH), int((roi[3] - roi[1]) * fW)]
        klab, kb = lab[mask], b[mask]
    else:
        win, klab, kb = [0, 0, H, W], lab, b
    trace['window'] = list(win)
    trace['raw'] = raw
    if win[2] < 1 or win[3] < 1:
        win, klab, kb = [0, 0, H, W], lab, b
        trace['unchanged'] = True
    else:
        trace['unchanged'] = False
        kb = kb * np.array([H, W, H, W], F) - np.array([win[0], win[1], win[0], win[1]], F)
        trace['unclipped'] = kb.copy()
        kb = np.stack([np.maximum(F(0), kb[:, 0]), np.maximum(F(0), kb[:, 1]),
                       np.minimum(F(win[2]), kb[:, 2]), np.minimum(F(win[3]), kb[:, 3])], axis=-1)
        kb = kb / np.array([win[2], win[3], win[2], win[3]], F)
    flip = bool(less(d[4], F(0.5), 'le_flip'))
    if flip:
        kb = np.stack([kb[:, 0], F(1) - kb[:, 3], kb[:, 2], F(1) - kb[:, 1]], axis=-1)
    assert kb.dtype == F
    k = klab.size
    out_l, out_b = np.zeros(G, np.int32), np.zeros((G, 4), F)
    out_l[:k], out_b[:k] = klab, kb.reshape(-1, 4)
    geom = np.zeros(RON_TRAIN_GEOM, np.int32)
    geom[:] = [int(expanded), H, W, img_y, img_x, win[0], win[1], win[2], win[3], int(flip), iou_index, index]
    return dict(geom=geom, labels=out_l, bboxes=out_b, count=k, trace=trace)


# ------------------------------------------------------------------------------------------------------------ geometry, scalar
def geometry_scalar(h, w, labels, bboxes, draws):
    """The same function from its description, one box at a time (float32 scalars).  Returns (geom[:10], labels, bboxes, count)."""
    d = [F(v) for v in np.asarray(draws, F).reshape(-1)]
    labels = [int(v) for v in np.asarray(labels).reshape(-1)]
    G = len(labels)
    raw_boxes = np.asarray(bboxes, F).reshape(G, 4)
    boxes = []                                            # present rows: [label, ymin, xmin, ymax, xmax]
    for i in range(G):
        if labels[i] == 0:
            break
        boxes.append([labels[i]] + [F(v) for v in raw_boxes[i]])
    half, one, two, zero = F(0.5), F(1), F(2), F(0)

    expanded = 0 if d[0] < half else 1
    H, W, oy, ox = h, w, 0, 0
    if expanded:
        ox = min(int(F(d[1] * F(w))), w - 1)
        oy = min(int(F(d[2] * F(h))), h - 1)
        H, W = 2 * h, 2 * w
        for bx in boxes:
            bx[1] = F(F(F(bx[1] * F(h)) + F(oy)) / F(H))
            bx[2] = F(F(F(bx[2] * F(w)) + F(ox)) / F(W))
            bx[3] = F(F(F(bx[3] * F(h)) + F(oy)) / F(H))
            bx[4] = F(F(F(bx[4] * F(w)) + F(ox)) / F(W))
    fH, fW = F(H), F(W)
    min_iou = [F(0.4), F(0.5), F(0.6), F(0.7), F(0.8), F(0.9)][min(int(F(d[3] * F(6))), 5)]
    centres = [(F(F(bx[1] + bx[3]) / two), F(F(bx[2] + bx[4]) / two)) for bx in boxes]
    span = F(F(0.999) - F(0.1))

    def overlap(r, bx):
        top, left = max(r[0], bx[1]), max(r[1], bx[2])
        bottom, right = min(r[2], bx[3]), min(r[3], bx[4])
        ih, iw = F(bottom - top), F(right - left)
        ih = ih if ih > zero else zero
        iw = iw if iw > zero else zero
        inter = F(ih * iw)
        area_r = F(F(r[3] - r[1]) * F(r[2] - r[0]))
        area_b = F(F(bx[3] - bx[1]) * F(bx[4] - bx[2]))
        with np.errstate(divide='ignore', invalid='ignore'):
            return F(inter / F(area_r + F(area_b - inter)))

    kept, r = [], None
    outer = 0
    while True:                                           # the overlap loop: at least one pass, at most ten
        inner = 0
        while True:                                       # the centre loop: at least one pass, at most ten
            base = 5 + (outer * 10 + inner) * 12
            for t in range(5):                            # up to five tries for an aspect within [1/2, 2]; the fifth is taken anyway
                sw = F(F(F(d[base + 2 * t] * span) + F(0.1)) * fW)
                sh = F(F(F(d[base + 2 * t + 1] * span) + F(0.1)) * fH)
                if not (sw > F(sh * two) or sh > F(sw * two)):
                    break
            isw, ish = int(sw), int(sh)
            x = min(int(F(d[base + 10] * F(W - isw))), W - isw - 1)
            y = min(int(F(d[base + 11] * F(H - ish))), H - ish - 1)
            r = (F(F(y) / fH), F(F(x) / fW), F(F(y + ish) / fH), F(F(x + isw) / fW))
            kept = [i for i, (cy, cx) in enumerate(centres) if cy > r[0] and cx > r[1] and cy < r[2] and cx < r[3]]
            inner += 1
            if kept or inner == 10:
                break
        outer += 1
        if outer == 10 or not any(overlap(r, boxes[i]) < min_iou for i in kept):
            break
    if kept:
        win = (int(F(r[0] * fH)), int(F(r[1] * fW)), int(F(F(r[2] - r[0]) * fH)), int(F(F(r[3] - r[1]) * fW)))
    else:
        win, kept = (0, 0, H, W), list(range(len(boxes)))
    out = []
    if win[2] < 1 or win[3] < 1:
        win = (0, 0, H, W)
        out = [list(bx) for bx in boxes]
    else:
        ch, cw = F(win[2]), F(win[3])
        for i in kept:
            lab, y0, x0, y1, x1 = boxes[i]
            y0, y1 = F(F(y0 * fH) - F(win[0])), F(F(y1 * fH) - F(win[0]))
            x0, x1 = F(F(x0 * fW) - F(win[1])), F(F(x1 * fW) - F(win[1]))
            y0, x0 = (y0 if y0 > zero else zero), (x0 if x0 > zero else zero)
            y1, x1 = (y1 if y1 < ch else ch), (x1 if x1 < cw else cw)
            out.append([lab, F(y0 / ch), F(x0 / cw), F(y1 / ch), F(x1 / cw)])
    flip = 1 if d[4] < half else 0
    if flip:
        out = [[lab, y0, F(one - x1), y1, F(one - x0)] for (lab, y0, x0, y1, x1) in out]
    out_l, out_b = np.zeros(G, np.int32), np.zeros((G, 4), F)
    for i, row in enumerate(out):
        out_l[i], out_b[i] = row[0], row[1:]
    geom = np.array([expanded, H, W, oy, ox, win[0], win[1], win[2], win[3], flip], np.int32)
    return geom, out_l, out_b, len(out)


def geometry_batch(hw, glabels, gbboxes, draws, fn=None):
    """A padded batch through the scalar reference (or fn): (geom [N, 10], labels [N, G], bboxes [N, G, 4], counts [N])."""
    fn = fn or geometry_scalar
    per = [fn(int(hw[i][0]), int(hw[i][1]), glabels[i], gbboxes[i], draws[i]) for i in range(len(hw))]
    return (np.stack([q[0] for q in per]), np.stack([q[1] for q in per]), np.stack([q[2] for q in per]),
            np.array([q[3] for q in per], np.int32))


# ------------------------------------------------------------------------------------------------------------ pixels
def canvas_fill(image):
    """The mean colour of the uint8 image in [0, 1]: exact integer sums, one correctly rounded quotient per channel."""
    h, w = image.shape[:2]
    sums = np.asarray(image, np.uint64).reshape(-1, 3).sum(axis=0, dtype=np.uint64)
    return np.array([F(np.float64(int(s)) / (255.0 * h * w)) for s in sums], F)


def pixels_ref(image, geom, out_shape, means=MEANS, mut=()):
    """One uint8 HWC image and its geometry row -> float32 [out_h, out_w, 3]."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    h, w = image.shape[:2]
    expanded, H, W, img_y, img_x, cy, cx, ch, cw, flip = [int(v) for v in geom[:10]]
    m = np.asarray(means, F)
    if 'whiten_first' in mut:                                     # the eval kernel's order of operations
        img = image.astype(F) - m
        fill = canvas_fill(image) * F(255) - m
    else:
        img = image.astype(F) * (F(1) / F(255))                   # convert_image_dtype
        fill = canvas_fill(image)
    if expanded:
        assert (H, W) == (2 * h, 2 * w)
        canvas = np.empty((H, W, 3), F)
        canvas[:] = fill
        canvas[img_y:img_y + h, img_x:img_x + w] = img
    else:
        assert (H, W) == (h, w)
        canvas = img
    patch = canvas[cy:cy + ch, cx:cx + cw]
    assert patch.shape[:2] == (ch, cw)
    if 'resize_before_flip' in mut:
        res = resize_bilinear(patch, out_shape)
        res = res[:, ::-1] if flip else res
    else:
        res = resize_bilinear(patch[:, ::-1] if flip else patch, out_shape)
    if 'whiten_first' in mut:
        return np.ascontiguousarray(res, F)
    out = res * F(255) - m
    assert out.dtype == F
    return np.ascontiguousarray(out)
