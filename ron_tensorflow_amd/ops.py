"""Host-side wrappers of the post-processing and single-operator entry points.

Each function takes/returns torch tensors on the GPU (device containers only) and calls one
C-ABI entry point of libron_hip.so.  Names follow the reference's numpy module
(``nets/np_methods.py``) where a function replaces one of its steps.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import Detections, Heads, PostCfg, check, current_stream, lib, ptr


# --------------------------------------------------------------------------- #
# anchors (host)                       replaces nets/ron_vgg_320.py:285-355
# --------------------------------------------------------------------------- #
def anchor_one_layer(img_shape, feat_shape, sizes, ratios, step, offset=0.5, dtype=np.float32):
    """(y, x, h, w) with the reference's shapes: y, x [H, W, 1]; h, w [A]."""
    fh, fw = int(feat_shape[0]), int(feat_shape[1])
    na = len(sizes) * len(ratios)
    y = np.empty((fh, fw, 1), np.float32)
    x = np.empty((fh, fw, 1), np.float32)
    h = np.empty((na,), np.float32)
    w = np.empty((na,), np.float32)
    sz = (C.c_double * len(sizes))(*[float(s) for s in sizes])
    rt = (C.c_double * len(ratios))(*[float(r) for r in ratios])
    check(lib().ron_anchor_one_layer(int(img_shape[0]), int(img_shape[1]), fh, fw, sz, len(sizes), rt, len(ratios),
                                     float(step), float(offset), ptr(y), ptr(x), ptr(h), ptr(w)))
    return y.astype(dtype, copy=False), x.astype(dtype, copy=False), h.astype(dtype, copy=False), w.astype(dtype, copy=False)


def anchors_to_device(anchors, device):
    """List of (y, x, h, w) numpy -> list of 4-tuples of flat float32 device tensors."""
    out = []
    for (y, x, h, w) in anchors:
        out.append(tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(device)
                         for a in (y, x, h, w)))
    return out


# --------------------------------------------------------------------------- #
# detection records
# --------------------------------------------------------------------------- #
class DetectionBuffers(object):
    """Fixed-capacity per-image detection lists (SURVEY.md 8b "detection record")."""
    FIELDS = ('classes', 'scores', 'bboxes', 'anchor_index', 'count')

    def __init__(self, n, capacity, device):
        self.n, self.capacity = n, capacity
        self.classes = torch.zeros((n, capacity), dtype=torch.int32, device=device)
        self.scores = torch.zeros((n, capacity), dtype=torch.float32, device=device)
        self.bboxes = torch.zeros((n, capacity, 4), dtype=torch.float32, device=device)
        self.anchor_index = torch.zeros((n, capacity), dtype=torch.int32, device=device)
        self.count = torch.zeros((n,), dtype=torch.int32, device=device)

    def narrow(self, n):
        """The first `n` images of this set as a DetectionBuffers over the same memory (leading-dimension views)."""
        assert 1 <= n <= self.n
        if n == self.n:
            return self
        v = object.__new__(DetectionBuffers)
        v.n, v.capacity = n, self.capacity
        for f in self.FIELDS:
            setattr(v, f, getattr(self, f)[:n])
        return v

    def record_stream(self, stream):
        """Tell the caching allocator that `stream` uses these tensors (they were allocated on another stream)."""
        for f in self.FIELDS:
            getattr(self, f).record_stream(stream)

    def c_struct(self):
        return Detections(self.capacity, ptr(self.classes), ptr(self.scores), ptr(self.bboxes),
                          ptr(self.anchor_index), ptr(self.count))

    def to_lists(self):
        """Host copy: list (per image) of dicts with the `count` valid rows."""
        cnt = self.count.cpu().numpy()
        cl, sc, bb, ai = (t.cpu().numpy() for t in (self.classes, self.scores, self.bboxes, self.anchor_index))
        return [dict(classes=cl[i, :cnt[i]].astype(np.int64), scores=sc[i, :cnt[i]], bboxes=bb[i, :cnt[i]],
                     anchor_index=ai[i, :cnt[i]].astype(np.int64)) for i in range(self.n)]


def _fill_heads(cls, obj, loc, anchors_dev, num_classes):
    h = Heads()
    h.num_layers = len(cls)
    h.num_classes = num_classes
    keep = []
    for i in range(len(cls)):
        c = cls[i]
        assert c.dtype == torch.float32 and c.is_cuda and c.dim() == 5, 'cls[%d] must be a float32 GPU tensor [N,H,W,A,C]' % i
        h.feat_h[i], h.feat_w[i], h.num_anchors[i] = c.shape[1], c.shape[2], c.shape[3]
        tensors = [c.contiguous(), None if obj is None else obj[i].contiguous(), loc[i].contiguous()]
        keep.append(tensors)
        h.cls[i] = tensors[0].data_ptr()
        h.obj[i] = None if tensors[1] is None else tensors[1].data_ptr()
        h.loc[i] = tensors[2].data_ptr()
        if anchors_dev is not None:
            ay, ax, ah, aw = anchors_dev[i]
            h.anchor_y[i], h.anchor_x[i] = ay.data_ptr(), ax.data_ptr()
            h.anchor_h[i], h.anchor_w[i] = ah.data_ptr(), aw.data_ptr()
    return h, keep


_WORKSPACES = collections.OrderedDict()
_MAX_WORKSPACES = 8


def _workspace(device, nbytes):
    """Scratch of the post-processing entry points, one per (device, stream): calls on different streams never share
    candidate lists, and a regrown buffer is dropped on the stream that was its only user.  At most _MAX_WORKSPACES
    entries, least recently used first out, so short-lived streams do not pin scratch for the life of the process; an
    entry is (buffer, stream object): holding the stream keeps its handle from being recycled for another stream while
    the allocator still attributes the buffer to it."""
    stream = torch.cuda.current_stream(device)
    key = (device.type, device.index, stream.cuda_stream)
    ent = _WORKSPACES.get(key)
    if ent is None or ent[0].numel() < nbytes:
        ent = (torch.empty((int(nbytes),), dtype=torch.uint8, device=device), stream)
        _WORKSPACES[key] = ent
    _WORKSPACES.move_to_end(key)
    while len(_WORKSPACES) > _MAX_WORKSPACES:
        _WORKSPACES.popitem(last=False)
    return ent[0]


def _sized_workspace(device, nbytes):
    """The scratch for the result of a *_workspace_bytes entry; a negative result raises with the library's message."""
    if nbytes < 0:
        check(-1)
    return _workspace(device, nbytes)


def post_np(cls, obj, loc, anchors_dev, num_classes=None, objectness_thres=0.03, select_threshold=0.01,
            nms_threshold=0.45, top_k=400, bbox_img=(0., 0., 1., 1.), prior_scaling=(0.1, 0.1, 0.2, 0.2),
            cls_is_prob=False, obj_is_prob=False, loc_decoded=False, want_sorted=False):
    """np_methods pipeline on the GPU (ron_post_np): per-layer lists of GPU tensors in, DetectionBuffers out.

    select -> clip -> sort(top_k) -> class-aware IoU NMS -> resize, nets/np_methods.py:56-242, with the softmax
    and the objectness gate of eval_ron_network.py:227-229 in front when logits are given.
    Returns (detections, sorted_or_None, n_candidates[int32 N]).
    """
    n = cls[0].shape[0]
    dev = cls[0].device
    if num_classes is None:
        num_classes = int(cls[0].shape[-1])          # RONParams.num_classes = the class tensors' last axis
    heads, keep = _fill_heads(cls, obj, loc, None if loc_decoded else anchors_dev, num_classes)
    cfg = PostCfg()
    # select_threshold None / 0: the arg-max branch of ssd_bboxes_select_layer (np_methods.py:82-89)
    cfg.objectness_thres, cfg.select_threshold, cfg.nms_threshold = objectness_thres, (select_threshold or 0.0), nms_threshold
    cfg.top_k = top_k
    for i in range(4):
        cfg.bbox_img[i] = bbox_img[i]
        cfg.prior_scaling[i] = prior_scaling[i]
    cfg.input_flags = ((_lib.RON_IN_CLS_IS_PROB if cls_is_prob else 0) | (_lib.RON_IN_OBJ_IS_PROB if obj_is_prob else 0) |
                       (_lib.RON_IN_LOC_DECODED if loc_decoded else 0))
    nbytes = lib().ron_post_np_workspace_bytes(C.byref(heads), n)
    ws = _sized_workspace(dev, nbytes)
    out = DetectionBuffers(n, top_k, dev)
    srt = DetectionBuffers(n, top_k, dev) if want_sorted else None
    n_cand = torch.zeros((n,), dtype=torch.int32, device=dev)
    out_c = out.c_struct()
    srt_c = srt.c_struct() if srt is not None else None
    check(lib().ron_post_np(C.byref(heads), n, C.byref(cfg), ptr(ws), nbytes, C.byref(out_c),
                            C.byref(srt_c) if srt_c is not None else None, ptr(n_cand), current_stream()))
    del keep
    return out, srt, n_cand


def np_sort_nms(classes, scores, bboxes, top_k=400, nms_threshold=0.45, n_valid=None, want_sorted=False):
    """bboxes_sort -> bboxes_nms (np_methods.py:137-150, :229-242) on explicit lists [N, K] / [N, K, 4]."""
    n, n_in = scores.shape
    dev = scores.device
    classes = classes.to(torch.int32).contiguous()
    scores = scores.contiguous()
    bboxes = bboxes.contiguous()
    nbytes = lib().ron_np_sort_nms_workspace_bytes(n, n_in)
    ws = _workspace(dev, nbytes)
    out = DetectionBuffers(n, top_k, dev)
    srt = DetectionBuffers(n, top_k, dev) if want_sorted else None
    out_c = out.c_struct()
    srt_c = srt.c_struct() if srt is not None else None
    check(lib().ron_np_sort_nms(ptr(classes), ptr(scores), ptr(bboxes), ptr(n_valid), n, n_in, top_k,
                                float(nms_threshold), ptr(ws), nbytes, C.byref(out_c),
                                C.byref(srt_c) if srt_c is not None else None, current_stream()))
    return out, srt


def bboxes_decode_layer(loc, anchor_dev, prior_scaling=(0.1, 0.1, 0.2, 0.2)):
    """ssd_bboxes_decode for one layer (np_methods.py:23-53 == ssd_common.py:448-474), batch capable."""
    loc = loc.contiguous()
    n, fh, fw, a, _ = loc.shape
    out = torch.empty_like(loc)
    ps = (C.c_float * 4)(*prior_scaling)
    ay, ax, ah, aw = anchor_dev
    check(lib().ron_bboxes_decode_layer(ptr(loc), n, fh, fw, a, ptr(ay), ptr(ax), ptr(ah), ptr(aw), ps, ptr(out),
                                        current_stream()))
    return out


def bboxes_filter_min(scores, bboxes, top_k, minsize=0.03):
    """RONNet.bboxes_filter_min on tensors (nets/ron_vgg_320.py:217-233): scores [B, N], bboxes [B, N, 4] -> per list the rows with
    w > minsize and h > minsize in their order (tf.boolean_mask), zero padded to top_k rows - or to the longest list's count when that
    is larger (tfe_tensors.pad_axis only ever pads).  The reference squeezes axis 0, i.e. takes B = 1; any B works here.
    The output length depends on the data, so this call reads the counts back (one host synchronisation), like a TF session run."""
    scores = scores.to(torch.float32).contiguous()
    bboxes = bboxes.to(torch.float32).contiguous()
    assert scores.dim() == 2 and bboxes.shape == scores.shape + (4,), 'scores [B, N], bboxes [B, N, 4]'
    b, n = scores.shape
    if n == 0:                                  # nothing to filter: top_k rows of padding (pad_axis)
        return (torch.zeros((b, int(top_k)), dtype=torch.float32, device=scores.device),
                torch.zeros((b, int(top_k), 4), dtype=torch.float32, device=scores.device))
    rows = max(n, int(top_k))
    out_s = torch.empty((b, rows), dtype=torch.float32, device=scores.device)
    out_b = torch.empty((b, rows, 4), dtype=torch.float32, device=scores.device)
    counts = torch.empty((b,), dtype=torch.int32, device=scores.device)
    check(lib().ron_bboxes_filter_min(ptr(scores), ptr(bboxes), b, n, float(minsize), ptr(out_s), ptr(out_b), rows, ptr(counts), current_stream()))
    keep = max(int(counts.max().item()), int(top_k))
    return out_s[:, :keep], out_b[:, :keep]


def softmax_last(x, pick=-1):
    """slim.softmax over the last axis; pick >= 0 keeps only that channel (shape [..., 1])."""
    x = x.contiguous()
    c = x.shape[-1]
    rows = x.numel() // c
    out = torch.empty(x.shape if pick < 0 else x.shape[:-1] + (1,), dtype=torch.float32, device=x.device)
    check(lib().ron_softmax_last(ptr(x), rows, c, pick, ptr(out), current_stream()))
    return out


# --------------------------------------------------------------------------- #
# label side: per-anchor targets and the held-out loss
# --------------------------------------------------------------------------- #
def _anchor_heads(anchors_dev, shapes):
    """A Heads that carries shapes [(H, W, A)] and anchor pointers only (what ron_bboxes_encode reads)."""
    h = Heads()
    h.num_layers = len(shapes)
    for i, (fh, fw, a) in enumerate(shapes):
        h.feat_h[i], h.feat_w[i], h.num_anchors[i] = fh, fw, a
        ay, ax, ah, aw = anchors_dev[i]
        h.anchor_y[i], h.anchor_x[i], h.anchor_h[i], h.anchor_w[i] = ay.data_ptr(), ax.data_ptr(), ah.data_ptr(), aw.data_ptr()
    return h


def bboxes_encode(glabels, gbboxes, anchors_dev, shapes, img_shape, allowed_borders, positive_threshold=0.5,
                  ignore_threshold=0.3, prior_scaling=(0.1, 0.1, 0.2, 0.2), heads=None):
    """tf_ssd_bboxes_encode for a padded batch (ron_bboxes_encode): glabels int32 [N, G] (0 = padding), gbboxes [N, G, 4] on the GPU;
    anchors_dev as anchors_to_device gives them, shapes [(H, W, A)] per layer (or `heads`: a Heads that already holds both).
    Returns four per-layer lists: gclasses int64 [N,H,W,A], glocalisations [N,H,W,A,4], gscores [N,H,W,A], gbboxes [N,H,W,A,4]."""
    assert glabels.is_cuda and glabels.dtype == torch.int32 and glabels.dim() == 2, 'glabels must be an int32 GPU tensor [N, G]'
    assert gbboxes.is_cuda and gbboxes.dtype == torch.float32 and tuple(gbboxes.shape) == tuple(glabels.shape) + (4,), \
        'gbboxes must be a float32 GPU tensor [N, G, 4]'
    glabels, gbboxes = glabels.contiguous(), gbboxes.contiguous()
    n, g = glabels.shape
    dev = glabels.device
    if heads is None:
        heads = _anchor_heads(anchors_dev, shapes)
    shapes = [(int(heads.feat_h[i]), int(heads.feat_w[i]), int(heads.num_anchors[i])) for i in range(heads.num_layers)]
    assert len(allowed_borders) >= len(shapes), 'one allowed border per feature layer'
    out = _lib.Targets()
    gcl, glo, gsc, gbb = [], [], [], []
    for i, (fh, fw, a) in enumerate(shapes):
        gcl.append(torch.empty((n, fh, fw, a), dtype=torch.int64, device=dev))
        glo.append(torch.empty((n, fh, fw, a, 4), dtype=torch.float32, device=dev))
        gsc.append(torch.empty((n, fh, fw, a), dtype=torch.float32, device=dev))
        gbb.append(torch.empty((n, fh, fw, a, 4), dtype=torch.float32, device=dev))
        out.gclasses[i], out.glocalisations[i] = gcl[i].data_ptr(), glo[i].data_ptr()
        out.gscores[i], out.gbboxes[i] = gsc[i].data_ptr(), gbb[i].data_ptr()
    nbytes = lib().ron_bboxes_encode_workspace_bytes(n, g)
    ws = _sized_workspace(dev, nbytes)
    borders = (C.c_int32 * len(shapes))(*[int(b) for b in allowed_borders[:len(shapes)]])
    ps = (C.c_float * 4)(*prior_scaling)
    check(lib().ron_bboxes_encode(C.byref(heads), n, ptr(glabels), ptr(gbboxes), g, int(img_shape[0]), int(img_shape[1]), borders,
                                  float(positive_threshold), float(ignore_threshold), ps, ptr(ws), nbytes, C.byref(out),
                                  current_stream()))
    return gcl, glo, gsc, gbb


def _check_layer_tensors(i, *specs):
    """Every (name, tensor, shape, dtype) of layer i is a GPU tensor of that shape and type."""
    for name, t, want, dt in specs:
        assert t.is_cuda and t.dtype == dt and tuple(t.shape) == want, '%s[%d] must be a %s GPU tensor %s' % (name, i, dt, want)


def _grad_outputs(out_grads, names, likes, dev):
    """The per-layer gradient lists of a *_grad call, one per list of `likes`: `out_grads` checked, or new tensors."""
    if out_grads is None:
        out_grads = tuple([torch.empty(t.shape, dtype=torch.float32, device=dev) for t in lst] for lst in likes)
    for i in range(len(likes[0])):
        for name, grads, like in zip(names, out_grads, likes):
            t = grads[i]
            assert t.is_cuda and t.dtype == torch.float32 and t.shape == like[i].shape and t.is_contiguous(), \
                '%s[%d] must be a contiguous float32 GPU tensor %s' % (name, i, tuple(like[i].shape))
    return out_grads


LOSS_COUNTS = ('n_pos', 'n_neg', 'n_cls_pos', 'n_cls_neg', 'n_objness_set', 'n_cls_set')


def _losses_call(grad, logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_objness, rand_cls,
                 objness_threshold, negative_ratio, alpha, beta, out_grads=None):
    """ron_losses (grad False) or ron_losses_grad (grad True) on checked arguments."""
    n = logits[0].shape[0]
    dev = logits[0].device
    heads, keep = _fill_heads(logits, objness_logits, localisations, None, int(logits[0].shape[-1]))
    tg = _lib.Targets()
    objp = (C.c_void_p * _lib.RON_MAX_LAYERS)()
    rows = 0
    for i in range(len(logits)):
        shp = tuple(logits[i].shape[:4])
        _check_layer_tensors(i, ('objness_logits', objness_logits[i], shp + (2,), torch.float32),
                             ('localisations', localisations[i], shp + (4,), torch.float32),
                             ('glocalisations', glocalisations[i], shp + (4,), torch.float32),
                             ('gclasses', gclasses[i], shp, torch.int64))
        op = objness_pred[i]
        assert op.is_cuda and op.dtype == torch.float32 and op.numel() == gclasses[i].numel(), 'objness_pred[%d]: one float32 per anchor' % i
        tensors = [op.contiguous(), gclasses[i].contiguous(), glocalisations[i].contiguous()]
        keep.append(tensors)
        objp[i], tg.gclasses[i], tg.glocalisations[i] = tensors[0].data_ptr(), tensors[1].data_ptr(), tensors[2].data_ptr()
        rows += gclasses[i].numel()
    for name, t in (('rand_objness', rand_objness), ('rand_cls', rand_cls)):
        assert t.is_cuda and t.dtype == torch.float32 and t.numel() == rows, '%s must hold one float32 per anchor of the batch (%d)' % (name, rows)
    rand_objness, rand_cls = rand_objness.contiguous(), rand_cls.contiguous()
    cfg = _lib.LossCfg(float(objness_threshold), float(negative_ratio), float(alpha), float(beta))
    nbytes = (lib().ron_losses_grad_workspace_bytes if grad else lib().ron_losses_workspace_bytes)(C.byref(heads), n)
    ws = _sized_workspace(dev, nbytes)
    out = torch.empty((4,), dtype=torch.float32, device=dev)
    counts = torch.empty((6,), dtype=torch.int32, device=dev)
    if not grad:
        check(lib().ron_losses(C.byref(heads), objp, C.byref(tg), n, ptr(rand_objness), ptr(rand_cls), C.byref(cfg), ptr(ws), nbytes,
                               ptr(out), ptr(counts), current_stream()))
        del keep
        return out, counts
    hg = _lib.HeadGrads()
    d_cls, d_obj, d_loc = _grad_outputs(out_grads, ('d_logits', 'd_objness_logits', 'd_localisations'),
                                        (logits, objness_logits, localisations), dev)
    for i in range(len(logits)):
        hg.d_cls[i], hg.d_obj[i], hg.d_loc[i] = d_cls[i].data_ptr(), d_obj[i].data_ptr(), d_loc[i].data_ptr()
    check(lib().ron_losses_grad(C.byref(heads), objp, C.byref(tg), n, ptr(rand_objness), ptr(rand_cls), C.byref(cfg), ptr(ws), nbytes,
                                ptr(out), ptr(counts), C.byref(hg), current_stream()))
    del keep
    return out, counts, d_cls, d_obj, d_loc


def losses(logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_objness, rand_cls,
           objness_threshold=0.03, negative_ratio=3., alpha=1. / 3, beta=1. / 3):
    """ron_losses over the whole batch (nets/ron_vgg_320.py:635-778): per-layer lists of GPU tensors [N,H,W,A,*]; rand_objness /
    rand_cls: one float32 in [0, 1) per row, flattened (layer, image, row, column, anchor).  Returns (losses float32 [4]:
    cross_entropy_pos, cross_entropy_objectness, localization, total; counts int32 [6]: LOSS_COUNTS), both on the GPU."""
    return _losses_call(False, logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_objness, rand_cls,
                        objness_threshold, negative_ratio, alpha, beta)


def losses_grad(logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_objness, rand_cls,
                objness_threshold=0.03, negative_ratio=3., alpha=1. / 3, beta=1. / 3, out=None):
    """ron_losses_grad: the arguments of `losses`; returns (losses [4], counts [6], d_logits, d_objness_logits, d_localisations).
    The first two are bit for bit those of `losses`; the last three are per-layer lists of new float32 GPU tensors shaped like
    `logits`, `objness_logits` and `localisations`: the gradient of the class term, the objectness term and the localisation term
    with respect to its own head tensor (and, each term reading one tensor, of the total).  Every element is written by the call;
    `out`, when given, is (d_logits, d_objness_logits, d_localisations) to write into instead of new tensors."""
    return _losses_call(True, logits, localisations, objness_logits, objness_pred, gclasses, glocalisations, rand_objness, rand_cls,
                        objness_threshold, negative_ratio, alpha, beta, out_grads=out)


SSD_LOSS_COUNTS = ('n_pos', 'n_cand', 'k', 'n_mined')
SSD_MINING = {'batch': _lib.RON_SSD_MINING_BATCH, 'layer': _lib.RON_SSD_MINING_LAYER}


def _ssd_losses_call(grad, logits, localisations, gclasses, glocalisations, gscores, mining, match_threshold, negative_ratio, alpha,
                     want_nvalues, out_grads=None):
    """ron_ssd_losses (grad False) or ron_ssd_losses_grad (grad True) on checked arguments."""
    if mining not in SSD_MINING:
        raise ValueError("mining must be 'batch' or 'layer', not %r" % (mining,))
    n = logits[0].shape[0]
    dev = logits[0].device
    heads, keep = _fill_heads(logits, None, localisations, None, int(logits[0].shape[-1]))
    tg = _lib.Targets()
    rows = 0
    for i in range(len(logits)):
        shp = tuple(logits[i].shape[:4])
        _check_layer_tensors(i, ('localisations', localisations[i], shp + (4,), torch.float32),
                             ('glocalisations', glocalisations[i], shp + (4,), torch.float32),
                             ('gscores', gscores[i], shp, torch.float32), ('gclasses', gclasses[i], shp, torch.int64))
        tensors = [gclasses[i].contiguous(), glocalisations[i].contiguous(), gscores[i].contiguous()]
        keep.append(tensors)
        tg.gclasses[i], tg.glocalisations[i], tg.gscores[i] = (t.data_ptr() for t in tensors)
        rows += gclasses[i].numel()
    cfg = _lib.SsdLossCfg(SSD_MINING[mining], float(match_threshold), float(negative_ratio), float(alpha))
    nbytes = (lib().ron_ssd_losses_grad_workspace_bytes if grad else lib().ron_ssd_losses_workspace_bytes)(C.byref(heads), n)
    ws = _sized_workspace(dev, nbytes)
    segs = 1 if mining == 'batch' else len(logits)
    out = torch.empty((4,), dtype=torch.float32, device=dev)
    counts = torch.empty((segs, 4), dtype=torch.int32, device=dev)
    nvalues = torch.empty((rows,), dtype=torch.float32, device=dev) if want_nvalues else None
    if not grad:
        check(lib().ron_ssd_losses(C.byref(heads), C.byref(tg), n, C.byref(cfg), ptr(ws), nbytes, ptr(out), ptr(counts), ptr(nvalues),
                                   current_stream()))
        del keep
        return out, counts, nvalues
    hg = _lib.HeadGrads()
    d_cls, d_loc = _grad_outputs(out_grads, ('d_logits', 'd_localisations'), (logits, localisations), dev)
    for i in range(len(logits)):
        hg.d_cls[i], hg.d_loc[i] = d_cls[i].data_ptr(), d_loc[i].data_ptr()
    check(lib().ron_ssd_losses_grad(C.byref(heads), C.byref(tg), n, C.byref(cfg), ptr(ws), nbytes, ptr(out), ptr(counts), ptr(nvalues),
                                    C.byref(hg), current_stream()))
    del keep
    return out, counts, nvalues, d_cls, d_loc


def ssd_losses(logits, localisations, gclasses, glocalisations, gscores, mining='batch', match_threshold=0.5, negative_ratio=3.,
               alpha=1., nvalues=False):
    """ron_ssd_losses (nets/ssd_vgg_300.py:580-659 with mining 'batch', nets/ssd_vgg_512.py:516-607 with 'layer'): per-layer lists of
    GPU tensors [N,H,W,A,*].  Returns (losses float32 [4]: cross_entropy_pos, cross_entropy_neg, localization, total; counts int32
    [S, 4]: SSD_LOSS_COUNTS per segment, S = 1 or the number of layers; nvalues), all on the GPU; `nvalues` is None unless asked
    for: float32 [rows], every row's mining value (its background probability when it is a candidate, else 1)."""
    return _ssd_losses_call(False, logits, localisations, gclasses, glocalisations, gscores, mining, match_threshold, negative_ratio,
                            alpha, nvalues)


def ssd_losses_grad(logits, localisations, gclasses, glocalisations, gscores, mining='batch', match_threshold=0.5, negative_ratio=3.,
                    alpha=1., nvalues=False, out=None):
    """ron_ssd_losses_grad: the arguments of `ssd_losses`; returns (losses [4], counts [S, 4], nvalues, d_logits, d_localisations).
    The first three are bit for bit those of `ssd_losses`; the last two are per-layer lists of new float32 GPU tensors shaped like
    `logits` and `localisations`: the gradient of the two cross-entropy terms and of the localisation term (and, each reading one
    tensor, of the total).  Every element is written by the call; `out`, when given, is (d_logits, d_localisations) to write
    into instead of new tensors."""
    return _ssd_losses_call(True, logits, localisations, gclasses, glocalisations, gscores, mining, match_threshold, negative_ratio,
                            alpha, nvalues, out_grads=out)


# --------------------------------------------------------------------------- #
# single operators (parity tests of the conv kernels)
# --------------------------------------------------------------------------- #
def conv2d_nhwc(x, w, bias=None, residual=None, stride=1, dilation=1, relu=True, transpose=False, dtype='bf16',
                tile_cfg=-1, splitk=-1, pool=False, in_cstride=0, in_coff=0, center_from=0):
    """x GPU fp32 [N,H,W,Cin]; w, bias host numpy (HWIO, or [kh,kw,Cout,Cin] when transpose)."""
    x = x.contiguous()
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, h, wd, cin = x.shape
    kh, kw = w.shape[:2]
    cout = w.shape[2] if transpose else w.shape[3]
    d = _lib.ConvDesc(n, h, wd, cin, cout, kh, kw, stride, dilation, int(relu), int(transpose), _lib.DTYPES[dtype], tile_cfg, in_cstride, in_coff, int(pool), splitk, center_from)
    ho, wo = (h * stride, wd * stride) if transpose else (h // stride, wd // stride)
    if pool:
        ho, wo = (ho + 1) // 2, (wo + 1) // 2         # SAME: ceil
    y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    r = None if residual is None else residual.contiguous()
    check(lib().ron_conv2d_nhwc(C.byref(d), ptr(x), ptr(w), ptr(b), ptr(r), ptr(y), current_stream()))
    return y


def conv2d_pool2_nhwc(x, w, bias=None, relu=True, dtype='bf16', tile_cfg=-1, dilation=1):
    """3x3-style stride-1 convolution with the fused SAME 2x2 pool AND the un-pooled map from the same launch (ron_conv2d_pool2_nhwc:
    what the graph does for conv4_3 / conv5_3 with fuse_pools): (pooled [N,ceil(H/2),ceil(W/2),Cout], full [N,H,W,Cout])."""
    x = x.contiguous()
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, h, wd, cin = x.shape
    kh, kw, _, cout = w.shape
    d = _lib.ConvDesc(n, h, wd, cin, cout, kh, kw, 1, dilation, int(relu), 0, _lib.DTYPES[dtype], tile_cfg, 0, 0, 1, 1, 0)
    yp = torch.empty((n, (h + 1) // 2, (wd + 1) // 2, cout), dtype=torch.float32, device=x.device)
    yf = torch.empty((n, h, wd, cout), dtype=torch.float32, device=x.device)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    check(lib().ron_conv2d_pool2_nhwc(C.byref(d), ptr(x), ptr(w), ptr(b), ptr(yp), ptr(yf), current_stream()))
    return yp, yf


def conv_plan(n, h, w, cin, cout, k=3, stride=1, dilation=1, dtype='bf16', tile_cfg=-1, splitk=-1, pool=False, center_from=0, transpose=False):
    """How conv2d_nhwc would run this convolution (ron_conv_plan): dict(tile_cfg, splitk, tile_order, taps_inner)."""
    d = _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, dilation, 1, int(transpose), _lib.DTYPES[dtype], tile_cfg, 0, 0, int(pool), splitk, center_from)
    out = (C.c_int32 * 4)()
    check(lib().ron_conv_plan(C.byref(d), out))
    return dict(tile_cfg=out[0], splitk=out[1], tile_order=out[2], taps_inner=out[3])


def conv_plan_n_tile(n, h, w, cin, cout, k=3, dtype='bf16', tile_cfg=-1, splitk=-1):
    """Columns of the tile conv2d_nhwc would run this convolution on (ron_conv_plan_n_tile): 64 / 128 / 256, 224 for the 256 x 224 form
    of the four-wave tile, 0 for the kernels that are not the row-gather kernel."""
    d = _lib.ConvDesc(n, h, w, cin, cout, k, k, 1, 1, 1, 0, _lib.DTYPES[dtype], tile_cfg, 0, 0, 0, splitk, 0)
    out = C.c_int32(0)
    check(lib().ron_conv_plan_n_tile(C.byref(d), C.byref(out)))
    return out.value


def conv2d_f32out_nhwc(convs, grouped=False, dtype='bf16', with_tiles=False):
    """One or two head convolutions with fp32 outputs written by the kernel (ron_conv2d_f32out_nhwc).  convs: a list of one or two
    dict(x=GPU fp32 [N,H,W,Cin], w=HWIO numpy, bias=numpy or None, tile_cfg=-1, splitk=-1); grouped: both as one grouped launch of
    256 x 256 tiles.  Returns the list of outputs [N,H,W,Cout] fp32; with_tiles: (outputs, [column-tile width each ran on])."""
    args, keep, ys = [], [], []
    for cv in convs:
        x = cv['x'].contiguous()
        w = np.ascontiguousarray(cv['w'], dtype=np.float32)
        n, h, wd, cin = x.shape
        kh, kw, _, cout = w.shape
        d = _lib.ConvDesc(n, h, wd, cin, cout, kh, kw, 1, 1, 0, 0, _lib.DTYPES[dtype], cv.get('tile_cfg', -1), 0, 0, 0, cv.get('splitk', -1), 0)
        b = None if cv.get('bias') is None else np.ascontiguousarray(cv['bias'], dtype=np.float32)
        y = torch.empty((n, h, wd, cout), dtype=torch.float32, device=x.device)
        keep += [x, w, b, d]
        ys.append(y)
        args += [C.byref(d), ptr(x), ptr(w), ptr(b), ptr(y)]
    if len(convs) == 1:
        args += [None, None, None, None, None]
    tiles = (C.c_int32 * 2)()
    check(lib().ron_conv2d_f32out_nhwc(*args, int(grouped), tiles, current_stream()))
    return (ys, [tiles[k] for k in range(len(convs))]) if with_tiles else ys


def conv2d_patch_pair_nhwc(x, cin, wa, ba, coff_a, wb, bb, coff_b, dtype='bf16', full_width=False):
    """Two 3x3 head convolutions over the channel slices [coff, coff + cin) of one tensor x (GPU fp32 [N,H,W,C]) as one launch of the
    halo-patch pair kernel (ron_conv2d_patch_pair_nhwc) -> (ya, yb, [columns each member multiplied])."""
    x = x.contiguous()
    n, h, wd, cs = x.shape
    ws = [np.ascontiguousarray(w, dtype=np.float32) for w in (wa, wb)]
    bs = [None if b is None else np.ascontiguousarray(b, dtype=np.float32) for b in (ba, bb)]
    ds = [_lib.ConvDesc(n, h, wd, cin, w.shape[3], 3, 3, 1, 1, 0, 0, _lib.DTYPES[dtype], -1, cs, coff, 0, 1, 0) for w, coff in zip(ws, (coff_a, coff_b))]
    ys = [torch.empty((n, h, wd, w.shape[3]), dtype=torch.float32, device=x.device) for w in ws]
    cols = (C.c_int32 * 2)()
    check(lib().ron_conv2d_patch_pair_nhwc(C.byref(ds[0]), C.byref(ds[1]), ptr(x), ptr(ws[0]), ptr(bs[0]), ptr(ws[1]), ptr(bs[1]),
                                           ptr(ys[0]), ptr(ys[1]), int(full_width), cols, current_stream()))
    return ys[0], ys[1], [cols[0], cols[1]]


def conv2d_heads_nhwc(x, w, split_first, bias=None, dilation=1, relu=False, dtype='bf16', tile_cfg=-1, splitk=-1):
    """One convolution, two fp32 head tensors (ron_conv2d_heads_nhwc: what the SSD-512 graph does with the class and box convolutions of
    a feature layer, nets/ssd_vgg_300.py:403-431): w HWIO with cout = both heads' channels, the first `split_first` of them -> y_first."""
    x = x.contiguous()
    w = np.ascontiguousarray(w, dtype=np.float32)
    n, h, wd, cin = x.shape
    kh, kw, _, cout = w.shape
    d = _lib.ConvDesc(n, h, wd, cin, cout, kh, kw, 1, dilation, int(relu), 0, _lib.DTYPES[dtype], tile_cfg, 0, 0, 0, splitk, 0)
    y1 = torch.empty((n, h, wd, split_first), dtype=torch.float32, device=x.device)
    y2 = torch.empty((n, h, wd, cout - split_first), dtype=torch.float32, device=x.device)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    check(lib().ron_conv2d_heads_nhwc(C.byref(d), int(split_first), ptr(x), ptr(w), ptr(b), ptr(y1), ptr(y2), current_stream()))
    return y1, y2


def maxpool2x2_nhwc(x, dtype='bf16'):
    """slim.max_pool2d [2, 2] stride 2 SAME: [N, ceil(H/2), ceil(W/2), C] (an odd map's last window holds one row / column)."""
    x = x.contiguous()
    n, h, w, c = x.shape
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=torch.float32, device=x.device)
    check(lib().ron_maxpool2x2_nhwc(ptr(x), n, h, w, c, _lib.DTYPES[dtype], ptr(y), current_stream()))
    return y


# --------------------------------------------------------------------------- #
# convolution backward (ron_conv2d_backward_nhwc): a real entry point - it enqueues on the current stream and never synchronises
# --------------------------------------------------------------------------- #
def _backward_desc(n, h, w, cin, cout, k, dilation, relu, dtype, splitk):
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, 1, dilation, int(relu), 0, _lib.DTYPES[dtype], -1, 0, 0, 0, splitk, 0)


def _desc_workspace_bytes(op, d, *extra):
    """ron_<op>_workspace_bytes of a descriptor (and the operator's arguments behind it); raises on one the library refuses."""
    nbytes = getattr(lib(), 'ron_%s_workspace_bytes' % op)(C.byref(d), *extra)
    if nbytes < 0:
        raise _lib.RonError('libron_hip: %s' % lib().ron_last_error().decode())
    return int(nbytes)


def _conv_backward_call(op, describe, x, w, dy, y, relu, need, workspace, extra=()):
    """What conv2d_backward_nhwc, conv2d_k2s2_backward_nhwc and conv2d_padded_backward_nhwc (`op`: the name without _nhwc; `extra`:
    the operator's arguments between the descriptor and x) share: the arguments made contiguous
    GPU tensors, `describe(x, w, dy)` (the operator's shape assertions; returns cout and a function that builds the descriptor),
    the checks of y and need, the workspace, the outputs and the call of ron_<op>_nhwc."""
    x, dy = x.contiguous(), dy.contiguous()
    dev = x.device
    if not hasattr(w, 'data_ptr'):
        w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(dev)
    w = w.contiguous()
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and w.dtype == torch.float32 and x.is_cuda and dy.is_cuda and w.is_cuda
    cout, desc = describe(x, w, dy)
    if relu and y is None:
        raise _lib.RonError('%s_nhwc: relu=True needs the forward output y (the mask is y > 0)' % op)
    if y is not None:
        y = y.contiguous()
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(dy.shape)
    unknown = set(need) - {'dx', 'dw', 'db'}
    assert not unknown, 'need: unknown output(s) %s' % sorted(unknown)
    d = desc()
    nbytes = _desc_workspace_bytes(op, d, *extra)
    ws = _workspace(dev, nbytes) if workspace is None else workspace
    dx = torch.empty_like(x) if 'dx' in need else None
    dw = torch.empty_like(w) if 'dw' in need else None
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if 'db' in need else None
    check(getattr(lib(), 'ron_%s_nhwc' % op)(C.byref(d), *extra, ptr(x), ptr(w), ptr(y if relu else None), ptr(dy), ptr(dx), ptr(dw), ptr(db),
                                              ptr(ws), int(ws.numel()), current_stream()))
    return dx, dw, db


def _needed_grads(ctx, has_bias):
    """The `need` of a convolution's autograd backward: the gradients autograd asks for (db only where there is a bias)."""
    return tuple(name for name, on in zip(('dx', 'dw', 'db'), (ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                                               has_bias and ctx.needs_input_grad[2])) if on)


def conv2d_backward_workspace_bytes(n, h, w, cin, cout, k=3, dilation=1, relu=True, dtype='bf16', splitk=-1):
    """Bytes of workspace conv2d_backward_nhwc needs for this convolution (host arithmetic; raises on a descriptor it refuses)."""
    return _desc_workspace_bytes('conv2d_backward', _backward_desc(n, h, w, cin, cout, k, dilation, relu, dtype, splitk))


def conv2d_backward_nhwc(x, w, dy, y=None, relu=True, dilation=1, dtype='bf16', splitk=-1, need=('dx', 'dw', 'db'), workspace=None):
    """Gradients of y = act(conv_SAME(x, w) + bias), stride 1: (dx, dw, db), None for those not in `need`.

    x [N,H,W,Cin], dy and y [N,H,W,Cout] GPU fp32; w HWIO [k,k,Cin,Cout], a GPU fp32 tensor (a numpy array is uploaded).  With
    `relu` the mask is y > 0, so the forward output is required.  Operands are rounded to `dtype` (bf16 / fp16), sums are fp32 in a
    fixed order: dx comes back as storage-type values in fp32, dw [k,k,Cin,Cout] and db [Cout] as unrounded fp32 sums.
    `splitk`: pixel slices of the weight gradient (-1 by shape, 1 off, S forced).  `workspace`: a uint8 GPU tensor of at least
    conv2d_backward_workspace_bytes(...) bytes, or None for the cached per-device, per-stream buffer."""
    def describe(x, w, dy):
        n, h, wd, cin = x.shape
        k, cout = w.shape[0], w.shape[3]
        assert tuple(w.shape) == (k, k, cin, cout) and tuple(dy.shape) == (n, h, wd, cout)
        return cout, lambda: _backward_desc(n, h, wd, cin, cout, k, dilation, relu, dtype, splitk)
    return _conv_backward_call('conv2d_backward', describe, x, w, dy, y, relu, need, workspace)


def _stem_desc(n, h, w, relu, dtype, splitk):
    return _backward_desc(n, h, w, 3, 64, 3, 1, relu, dtype, splitk)


def conv2d_stem_backward_workspace_bytes(n, h, w, relu=True, dtype='bf16', splitk=-1):
    """Bytes of workspace conv2d_stem_backward_nhwc needs (host arithmetic; raises on a descriptor the library refuses)."""
    return _desc_workspace_bytes('conv2d_stem_backward', _stem_desc(n, h, w, relu, dtype, splitk))


def conv2d_stem_backward_nhwc(x, dy, y=None, relu=True, dtype='bf16', splitk=-1, need=('dw', 'db'), workspace=None):
    """Weight and bias gradients of the 3-channel stem y = act(conv_SAME(x, w) + bias), 3x3, 3 -> 64 channels (conv1_1): (dw, db),
    None for those not in `need`.  There is no gradient with respect to the image, hence no w.

    x [N,H,W,3], dy and y [N,H,W,64] GPU fp32.  Everything else as conv2d_backward_nhwc: the mask is y > 0 with `relu`, operands are
    rounded to `dtype` (bf16 / fp16), dw [3,3,3,64] and db [64] are unrounded fp32 sums in a fixed order; `splitk`: pixel slices (-1 by
    shape, 1 off, S forced); `workspace`: a uint8 GPU tensor of at least conv2d_stem_backward_workspace_bytes(...) bytes, or None
    for the cached per-device, per-stream buffer."""
    x, dy = x.contiguous(), dy.contiguous()
    dev = x.device
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and x.is_cuda and dy.is_cuda
    n, h, wd, cin = x.shape
    if cin != 3 or tuple(dy.shape) != (n, h, wd, 64):
        raise _lib.RonError('conv2d_stem_backward_nhwc: x %s, dy %s: the 3 -> 64 channel stem only' % (tuple(x.shape), tuple(dy.shape)))
    if relu and y is None:
        raise _lib.RonError('conv2d_stem_backward_nhwc: relu=True needs the forward output y (the mask is y > 0)')
    if y is not None:
        y = y.contiguous()
        assert y.dtype == torch.float32 and tuple(y.shape) == tuple(dy.shape)
    unknown = set(need) - {'dw', 'db'}
    assert not unknown, 'need: unknown output(s) %s' % sorted(unknown)
    d = _stem_desc(n, h, wd, relu, dtype, splitk)
    nbytes = _desc_workspace_bytes('conv2d_stem_backward', d)
    ws = _workspace(dev, nbytes) if workspace is None else workspace
    dw = torch.empty((3, 3, 3, 64), dtype=torch.float32, device=dev) if 'dw' in need else None
    db = torch.empty((64,), dtype=torch.float32, device=dev) if 'db' in need else None
    check(lib().ron_conv2d_stem_backward_nhwc(C.byref(d), ptr(x), ptr(y if relu else None), ptr(dy), ptr(dw), ptr(db), ptr(ws),
                                              int(ws.numel()), current_stream()))
    return dw, db


# --------------------------------------------------------------------------- #
# convolution forward for training (ron_conv2d_forward_nhwc): device weights, the current stream, no synchronisation
# --------------------------------------------------------------------------- #
def _forward_desc(n, h, w, cin, cout, k, stride, dilation, relu, transpose, dtype):
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, dilation, int(relu), int(transpose), _lib.DTYPES[dtype], -1, 0, 0, 0, -1, 0)


def conv2d_forward_workspace_bytes(n, h, w, cin, cout, k=3, stride=1, dilation=1, relu=True, transpose=False, dtype='bf16'):
    """Bytes of workspace conv2d_forward_nhwc needs for this convolution (n, h, w: the input x; host arithmetic; raises on a
    descriptor the library refuses)."""
    return _desc_workspace_bytes('conv2d_forward', _forward_desc(n, h, w, cin, cout, k, stride, dilation, relu, transpose, dtype))


def conv2d_forward_nhwc(x, w, bias=None, relu=True, dilation=1, stride=1, transpose=False, dtype='bf16', workspace=None):
    """y = act(conv(x, w) + bias) from DEVICE weights: the training forward.  x [N,H,W,Cin], w HWIO [k,k,Cin,Cout] ([2,2,Cout,Cin] with
    `transpose`) and bias [Cout] or None are GPU fp32 tensors; nothing is copied to the host, the call enqueues on the current stream
    and never synchronises.  Stride-1 SAME 1x1 / 3x3 (any dilation) / 7x7, the 3 -> 64 channel stem, and the 2x2 stride-2 convolution
    (`stride=2`) and transposed convolution (`stride=2, transpose=True`); bf16 / fp16.  The arithmetic and the result's bytes are
    conv2d_nhwc's.  `workspace`: a uint8 GPU tensor of at least conv2d_forward_workspace_bytes(...) bytes, or None for the cached
    per-device, per-stream buffer."""
    for name, t in (('x', x), ('w', w), ('bias', bias)):
        if t is not None and not (hasattr(t, 'is_cuda') and t.is_cuda and t.dtype == torch.float32):
            raise _lib.RonError('conv2d_forward_nhwc: %s must be a GPU fp32 tensor (host weights: conv2d_nhwc)' % name)
    x, w = x.contiguous(), w.contiguous()
    bias = None if bias is None else bias.contiguous()
    n, h, wd, cin = x.shape
    k = w.shape[0]
    cout = w.shape[2] if transpose else w.shape[3]
    assert tuple(w.shape) == ((k, k, cout, cin) if transpose else (k, k, cin, cout)), 'w %s does not belong to x %s' % (tuple(w.shape), tuple(x.shape))
    assert bias is None or tuple(bias.shape) == (cout,)
    d = _forward_desc(n, h, wd, cin, cout, k, stride, dilation, relu, transpose, dtype)
    nbytes = _desc_workspace_bytes('conv2d_forward', d)
    ws = _workspace(x.device, nbytes) if workspace is None else workspace
    ho, wo = (h * stride, wd * stride) if transpose else (h // stride, wd // stride)
    y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
    check(lib().ron_conv2d_forward_nhwc(C.byref(d), ptr(x), ptr(w), ptr(bias), ptr(y), ptr(ws), int(ws.numel()), current_stream()))
    return y


class _Conv2dNhwcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, relu, dilation, dtype):
        y = conv2d_forward_nhwc(x.detach(), w.detach(), None if bias is None else bias.detach(), relu=relu, dilation=dilation, dtype=dtype)
        ctx.save_for_backward(x, w, y)
        ctx.cfg = (relu, dilation, dtype, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        relu, dilation, dtype, has_bias = ctx.cfg
        need = _needed_grads(ctx, has_bias)
        if x.shape[3] == 3:          # the stem: an entry point of its own, which has no gradient with respect to the image
            if 'dx' in need:
                raise _lib.RonError('conv2d_nhwc_fn: no gradient with respect to the input of the 3-channel stem (the image)')
            if tuple(w.shape) != (3, 3, 3, 64) or dilation != 1:
                raise _lib.RonError('conv2d_nhwc_fn: w %s, dilation %d: the backward of a 3-channel input exists for the 3x3, 3 -> 64 '
                                    'stem only' % (tuple(w.shape), dilation))
            dw, db = conv2d_stem_backward_nhwc(x, dy, y, relu=relu, dtype=dtype, need=need) if need else (None, None)
            return None, dw, db, None, None, None
        dx, dw, db = conv2d_backward_nhwc(x, w, dy, y, relu=relu, dilation=dilation, dtype=dtype, need=need) if need else (None, None, None)
        return dx, dw, db, None, None, None


def conv2d_nhwc_fn(x, w, bias, relu=True, dilation=1, dtype='bf16'):
    """act(conv_SAME(x, w) + bias), stride 1, as a torch.autograd.Function: x [N,H,W,Cin], w HWIO, bias [Cout] or None, GPU fp32 tensors.

    k = 1, 3 (any dilation) or 7 (dilation 1).  The forward is ONE ron_conv2d_forward_nhwc call (conv2d_forward_nhwc): the weights
    stay on the device and are packed there, on the current stream, without a synchronisation - the training path; its result has the
    bytes of conv2d_nhwc's.  The backward is ONE ron_conv2d_backward_nhwc call on the
    current stream, computing only the gradients autograd asks for; tensors that do not require grad get None.  A 3-channel x (the
    image in front of conv1_1) has ONE ron_conv2d_stem_backward_nhwc call instead, for dw and db; asking for its dx raises RonError."""
    return _Conv2dNhwcFn.apply(x, w, bias, relu, dilation, dtype)


# --------------------------------------------------------------------------- #
# convolution chain (ron_conv_chain_forward / ron_conv_chain_backward): a sequence of stride-1 convolutions and 2x2 pools, forward in
# one call and backward in one call, activations and gradients kept as storage-type halo tensors in one workspace in between
# --------------------------------------------------------------------------- #
def chain_conv(cout, k=3, dilation=1, relu=True, bias=True, tap=False, name=None):
    """One convolution layer of a chain's layer list (`name`: the variable scope, for callers that map layers to variables)."""
    return {'kind': 'conv', 'k': int(k), 'dilation': int(dilation), 'cout': int(cout), 'relu': bool(relu), 'bias': bool(bias),
            'tap': bool(tap), 'name': name}


def chain_pool(name=None):
    """One 2x2 stride-2 SAME max-pool layer of a chain's layer list."""
    return {'kind': 'pool', 'tap': False, 'name': name}


def _chain_desc(n, h, w, cin, layers, dtype):
    d = _lib.ChainDesc()
    d.n, d.h, d.w, d.cin, d.dtype, d.num_layers = int(n), int(h), int(w), int(cin), _lib.DTYPES[dtype], len(layers)
    if len(layers) > _lib.RON_CHAIN_MAX_LAYERS:
        raise _lib.RonError('conv chain: %d layers, at most %d' % (len(layers), _lib.RON_CHAIN_MAX_LAYERS))
    for i, l in enumerate(layers):
        if l['kind'] == 'pool':
            d.layers[i] = _lib.ChainLayer(_lib.RON_CHAIN_POOL2, 0, 0, 0, 0, 0, int(bool(l.get('tap', False))))
        elif l['kind'] == 'conv':
            d.layers[i] = _lib.ChainLayer(_lib.RON_CHAIN_CONV, l['k'], l.get('dilation', 1), l['cout'], int(l.get('relu', True)),
                                          int(l.get('bias', True)), int(bool(l.get('tap', False))))
        else:
            raise _lib.RonError('conv chain: layer %d: unknown kind %r' % (i, l['kind']))
    return d


def conv_chain_shapes(n, h, w, cin, layers, dtype='bf16'):
    """The output shape (n, h, w, c) of every layer of the chain (ron_conv_chain_shape); raises on a descriptor the library refuses."""
    d = _chain_desc(n, h, w, cin, layers, dtype)
    out = []
    for i in range(len(layers)):
        s = (C.c_int64 * 4)()
        check(lib().ron_conv_chain_shape(C.byref(d), i, s))
        out.append(tuple(int(v) for v in s))
    return out


def conv_chain_workspace_bytes(n, h, w, cin, layers, dtype='bf16'):
    """Bytes of the workspace conv_chain_forward and conv_chain_backward share for this chain (host arithmetic; raises on a descriptor
    the library refuses)."""
    return _desc_workspace_bytes('conv_chain', _chain_desc(n, h, w, cin, layers, dtype))


def _chain_ptrs(tensors, count):
    """A host array of `count` device pointers (None entries: NULL), or NULL for None."""
    if tensors is None:
        return None
    assert len(tensors) == count, '%d entries for %d layers' % (len(tensors), count)
    return (C.c_void_p * count)(*[None if t is None else t.data_ptr() for t in tensors])


def _chain_check(what, tensors):
    for t in tensors:
        if t is not None and not (hasattr(t, 'is_cuda') and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.RonError('%s: every tensor must be a contiguous GPU fp32 tensor' % what)


def conv_chain_forward(x, layers, weights, biases, dtype='bf16', workspace=None):
    """The chain's forward: x [N,H,W,Cin] GPU fp32, `layers` a list of chain_conv(...) / chain_pool() entries, `weights` / `biases`
    lists with one GPU fp32 tensor per layer (None for pools; biases None where a layer has none).  Returns (y, taps, workspace): y
    the last layer's output, taps a list with the fp32 output of every tapped layer (None elsewhere), and the workspace that now
    holds the activations conv_chain_backward reads (`workspace`: a uint8 GPU tensor of at least conv_chain_workspace_bytes(...)
    bytes, or None to allocate one).  ONE ron_conv_chain_forward call on the current stream, no synchronisation."""
    assert x.dim() == 4
    x = x.contiguous()
    _chain_check('conv_chain_forward', [x] + list(weights) + list(biases))
    n, h, w, cin = x.shape
    d = _chain_desc(n, h, w, cin, layers, dtype)
    nbytes = _desc_workspace_bytes('conv_chain', d)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device) if workspace is None else workspace
    shapes = conv_chain_shapes(n, h, w, cin, layers, dtype)
    taps = [torch.empty(shapes[i], dtype=torch.float32, device=x.device) if l.get('tap') else None for i, l in enumerate(layers)]
    y = torch.empty(shapes[-1], dtype=torch.float32, device=x.device)
    L = len(layers)
    check(lib().ron_conv_chain_forward(C.byref(d), ptr(x), _chain_ptrs(weights, L), _chain_ptrs(biases, L), _chain_ptrs(taps, L), ptr(y),
                                       ptr(ws), int(ws.numel()), current_stream()))
    return y, taps, ws


def conv_chain_backward(x_shape, layers, weights, dy, dtaps, workspace, dtype='bf16', need_dx=True, need_dw=None, need_db=None):
    """The chain's backward from the workspace conv_chain_forward filled: x_shape the forward's x.shape, dy the gradient of y, dtaps a
    list with the gradient of every tap (None: none) or None.  need_dx, need_dw[i], need_db[i] say what is computed (default: dx,
    every dw, and db of every layer with a bias).  Returns (dx, dws, dbs) with None for what was not asked for.  ONE
    ron_conv_chain_backward call on the current stream; it may be repeated and gives the same bytes."""
    n, h, w, cin = x_shape
    L = len(layers)
    dy = dy.contiguous()
    dtaps = None if dtaps is None else [None if t is None else t.contiguous() for t in dtaps]
    _chain_check('conv_chain_backward', [dy] + list(weights) + list(dtaps or []))
    d = _chain_desc(n, h, w, cin, layers, dtype)
    shapes = conv_chain_shapes(n, h, w, cin, layers, dtype)
    assert tuple(dy.shape) == shapes[-1], 'dy %s, the chain ends in %s' % (tuple(dy.shape), shapes[-1])
    for i, t in enumerate(dtaps or []):
        assert t is None or (layers[i].get('tap') and tuple(t.shape) == shapes[i]), 'dtaps[%d]' % i
    dev = dy.device
    conv = [l['kind'] == 'conv' for l in layers]
    need_dw = [conv[i] for i in range(L)] if need_dw is None else [bool(v) and conv[i] for i, v in enumerate(need_dw)]
    need_db = [conv[i] and layers[i].get('bias', True) for i in range(L)] if need_db is None else [bool(v) and conv[i] for i, v in enumerate(need_db)]
    dx = torch.empty((n, h, w, cin), dtype=torch.float32, device=dev) if need_dx else None
    dws = [torch.empty(tuple(weights[i].shape), dtype=torch.float32, device=dev) if need_dw[i] else None for i in range(L)]
    dbs = [torch.empty((layers[i]['cout'],), dtype=torch.float32, device=dev) if need_db[i] else None for i in range(L)]
    check(lib().ron_conv_chain_backward(C.byref(d), ptr(dy), _chain_ptrs(dtaps, L), _chain_ptrs(weights, L), ptr(dx), _chain_ptrs(dws, L),
                                        _chain_ptrs(dbs, L), ptr(workspace), int(workspace.numel()), current_stream()))
    return dx, dws, dbs


class _ConvChainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, layers, dtype, nw, *params):
        weights, biases = list(params[:nw]), list(params[nw:])
        det = lambda ts: [None if t is None else t.detach().contiguous() for t in ts]
        y, taps, ws = conv_chain_forward(x.detach(), layers, det(weights), det(biases), dtype=dtype)
        ctx.save_for_backward(*[t for t in weights if t is not None])
        ctx.cfg = (tuple(x.shape), layers, dtype, nw, [t is not None for t in weights], ws)
        ctx.tapped = [i for i, l in enumerate(layers) if l.get('tap')]
        ctx.y_shape = tuple(y.shape)
        ctx.set_materialize_grads(False)        # an output nobody used has no gradient: dtaps[i] stays NULL
        return (y,) + tuple(taps[i] for i in ctx.tapped)

    @staticmethod
    def backward(ctx, dy, *dtap_list):
        x_shape, layers, dtype, nw, has_w, ws = ctx.cfg
        saved = iter(ctx.saved_tensors)
        weights = [next(saved).detach().contiguous() if h else None for h in has_w]
        L = len(layers)
        dtaps = [None] * L
        for i, g in zip(ctx.tapped, dtap_list):
            dtaps[i] = g
        need = ctx.needs_input_grad
        need_dw = [bool(need[4 + i]) for i in range(L)]
        need_db = [bool(need[4 + nw + i]) for i in range(L)]
        if dy is None:          # only the taps carry gradients
            dy = torch.zeros(ctx.y_shape, dtype=torch.float32, device=ws.device)
        dx, dws, dbs = conv_chain_backward(x_shape, layers, weights, dy, dtaps, ws, dtype=dtype, need_dx=bool(need[0]), need_dw=need_dw,
                                           need_db=need_db)
        return (dx, None, None, None) + tuple(dws) + tuple(dbs)


def conv_chain_fn(x, layers, weights, biases, dtype='bf16'):
    """The chain as a torch.autograd.Function: returns (y, *taps), the taps in layer order.  x [N,H,W,Cin], weights[i] HWIO and
    biases[i] [Cout] GPU fp32 tensors (None for pools and for layers without a bias).  The forward is ONE ron_conv_chain_forward
    call into a workspace of its own, the backward ONE ron_conv_chain_backward call reading that workspace; it computes dx, dw[i] and
    db[i] only where autograd asks (needs_input_grad).  The results have the bytes of conv2d_nhwc_fn / maxpool2x2_nhwc_fn chained layer
    by layer."""
    L = len(layers)
    assert len(weights) == L and len(biases) == L
    return _ConvChainFn.apply(x, layers, dtype, L, *(list(weights) + list(biases)))


# --------------------------------------------------------------------------- #
# head chain (ron_head_chain_forward / ron_head_chain_backward): the convolution chain plus training-mode batch normalisation and the
# two-branch 3x3 | 1x1 convolution, so that every branch of a reverse-connection module is one chain.  `params` is a list with one
# dict per layer (or None): 'w', 'bias' (conv, pair), 'w2', 'bias2' (pair), 'gamma', 'beta', 'moving_mean', 'moving_var' (bn)
# --------------------------------------------------------------------------- #
_HEAD_IN = ('w', 'bias', 'w2', 'bias2', 'gamma', 'beta')                            # what the forward reads and autograd differentiates
_HEAD_GRAD = {'w': 'dw', 'bias': 'dbias', 'w2': 'dw2', 'bias2': 'dbias2', 'gamma': 'dgamma', 'beta': 'dbeta'}


def chain_bn(relu=True, eps=1e-5, decay=0.997, name=None):
    """One training-mode batch normalisation layer (then ReLU when `relu`) of a head chain's layer list."""
    return {'kind': 'bn', 'relu': bool(relu), 'eps': float(eps), 'decay': float(decay), 'tap': False, 'name': name}


def chain_conv_pair(cout, cout2, relu=False, bias=True, name=None):
    """One two-branch layer of a head chain's layer list: concat(conv3x3 -> cout channels, conv1x1 -> cout2 channels)."""
    return {'kind': 'pair', 'cout': int(cout), 'cout2': int(cout2), 'relu': bool(relu), 'bias': bool(bias), 'tap': False, 'name': name}


def _head_chain_desc(n, h, w, cin, layers, dtype):
    d = _lib.HeadChainDesc()
    d.n, d.h, d.w, d.cin, d.dtype, d.num_layers = int(n), int(h), int(w), int(cin), _lib.DTYPES[dtype], len(layers)
    if len(layers) > _lib.RON_CHAIN_MAX_LAYERS:
        raise _lib.RonError('head chain: %d layers, at most %d' % (len(layers), _lib.RON_CHAIN_MAX_LAYERS))
    for i, l in enumerate(layers):
        tap = int(bool(l.get('tap', False)))
        if l['kind'] == 'pool':
            d.layers[i] = _lib.HeadChainLayer(_lib.RON_CHAIN_POOL2, 0, 0, 0, 0, 0, tap, 0, 0.0, 0.0)
        elif l['kind'] == 'conv':
            d.layers[i] = _lib.HeadChainLayer(_lib.RON_CHAIN_CONV, l['k'], l.get('dilation', 1), l['cout'], int(l.get('relu', True)),
                                              int(l.get('bias', True)), tap, 0, 0.0, 0.0)
        elif l['kind'] == 'pair':
            d.layers[i] = _lib.HeadChainLayer(_lib.RON_CHAIN_CONV_PAIR, 0, 0, l['cout'], int(l.get('relu', False)), int(l.get('bias', True)),
                                              tap, l['cout2'], 0.0, 0.0)
        elif l['kind'] == 'bn':
            d.layers[i] = _lib.HeadChainLayer(_lib.RON_CHAIN_BN, 0, 0, 0, int(l.get('relu', True)), 0, tap, 0, float(l.get('eps', 1e-5)),
                                              float(l.get('decay', 0.997)))
        else:
            raise _lib.RonError('head chain: layer %d: unknown kind %r' % (i, l['kind']))
    return d


def head_chain_shapes(n, h, w, cin, layers, dtype='bf16'):
    """The output shape (n, h, w, c) of every layer of the head chain (ron_head_chain_shape); raises on a refused descriptor."""
    d = _head_chain_desc(n, h, w, cin, layers, dtype)
    out = []
    for i in range(len(layers)):
        s = (C.c_int64 * 4)()
        check(lib().ron_head_chain_shape(C.byref(d), i, s))
        out.append(tuple(int(v) for v in s))
    return out


def head_chain_workspace_bytes(n, h, w, cin, layers, dtype='bf16'):
    """Bytes of the workspace head_chain_forward and head_chain_backward share for this chain (host arithmetic; raises on a refused
    descriptor)."""
    return _desc_workspace_bytes('head_chain', _head_chain_desc(n, h, w, cin, layers, dtype))


def _head_ptrs(L, **columns):
    """The host array of ron_head_chain_ptrs: columns[name] is a list with one tensor (or None) per layer."""
    table = (_lib.HeadChainPtrs * L)()
    for name, tensors in columns.items():
        assert len(tensors) == L, '%s: %d entries for %d layers' % (name, len(tensors), L)
        for i, t in enumerate(tensors):
            if t is not None:
                setattr(table[i], name, t.data_ptr())
    return table


def _head_column(params, name):
    return [None if p is None else p.get(name) for p in params]


def head_chain_forward(x, layers, params, dtype='bf16', workspace=None):
    """The head chain's forward: x [N,H,W,Cin] GPU fp32, `layers` a list of chain_conv / chain_pool / chain_bn / chain_conv_pair
    entries, `params` one dict of GPU fp32 tensors per layer (None for pools).  A bn layer's 'moving_mean' / 'moving_var' (both or
    neither) are updated IN PLACE.  Returns (y, taps, stats, workspace): taps[i] the fp32 output of a tapped convolution, stats[i] the
    batch (mean, var) of a bn layer (None elsewhere), and the workspace that now holds what head_chain_backward reads.  ONE
    ron_head_chain_forward call on the current stream, no synchronisation."""
    assert x.dim() == 4 and len(params) == len(layers)
    x = x.contiguous()
    L = len(layers)
    cols = {name: _head_column(params, name) for name in _HEAD_IN + ('moving_mean', 'moving_var')}
    _chain_check('head_chain_forward', [x] + [t for col in cols.values() for t in col])
    n, h, w, cin = x.shape
    d = _head_chain_desc(n, h, w, cin, layers, dtype)
    nbytes = _desc_workspace_bytes('head_chain', d)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device) if workspace is None else workspace
    shapes = head_chain_shapes(n, h, w, cin, layers, dtype)
    new = lambda shape: torch.empty(shape, dtype=torch.float32, device=x.device)
    taps = [new(shapes[i]) if l.get('tap') else None for i, l in enumerate(layers)]
    stats = [(new((shapes[i][3],)), new((shapes[i][3],))) if l['kind'] == 'bn' else None for i, l in enumerate(layers)]
    y = new(shapes[-1])
    table = _head_ptrs(L, tap=taps, mean=[None if s is None else s[0] for s in stats], var=[None if s is None else s[1] for s in stats], **cols)
    check(lib().ron_head_chain_forward(C.byref(d), ptr(x), table, ptr(y), ptr(ws), int(ws.numel()), current_stream()))
    return y, taps, stats, ws


def head_chain_backward(x_shape, layers, params, dy, dtaps, workspace, dtype='bf16', need_dx=True, need=None):
    """The head chain's backward from the workspace head_chain_forward filled.  `need`: per layer the names of the parameters whose
    gradients are computed (default: every parameter the layer has in `params` among w, bias, w2, bias2, gamma, beta).  Returns
    (dx, grads): grads[i] a dict {'dw': ..., 'dbias': ..., 'dw2': ..., 'dbias2': ..., 'dgamma': ..., 'dbeta': ...} with the requested
    entries (None for a layer without parameters).  ONE ron_head_chain_backward call on the current stream; it may be repeated and
    gives the same bytes."""
    n, h, w, cin = x_shape
    L = len(layers)
    assert len(params) == L
    dy = dy.contiguous()
    dtaps = [None] * L if dtaps is None else [None if t is None else t.contiguous() for t in dtaps]
    cols = {name: _head_column(params, name) for name in ('w', 'w2', 'gamma')}
    _chain_check('head_chain_backward', [dy] + dtaps + [t for col in cols.values() for t in col])
    d = _head_chain_desc(n, h, w, cin, layers, dtype)
    shapes = head_chain_shapes(n, h, w, cin, layers, dtype)
    assert tuple(dy.shape) == shapes[-1], 'dy %s, the chain ends in %s' % (tuple(dy.shape), shapes[-1])
    for i, t in enumerate(dtaps):
        assert t is None or (layers[i].get('tap') and tuple(t.shape) == shapes[i]), 'dtaps[%d]' % i
    dev = dy.device
    grads = []
    for i in range(L):
        have = [name for name in _HEAD_IN if params[i] is not None and params[i].get(name) is not None]
        want = have if need is None else [name for name in have if name in (need[i] or ())]
        grads.append({_HEAD_GRAD[name]: torch.empty(tuple(params[i][name].shape), dtype=torch.float32, device=dev) for name in want} or None)
    dx = torch.empty((n, h, w, cin), dtype=torch.float32, device=dev) if need_dx else None
    out_cols = {g: [None if gr is None else gr.get(g) for gr in grads] for g in _HEAD_GRAD.values()}
    table = _head_ptrs(L, dtap=dtaps, **cols, **out_cols)
    check(lib().ron_head_chain_backward(C.byref(d), ptr(dy), table, ptr(dx), ptr(workspace), int(workspace.numel()), current_stream()))
    return dx, grads


class _HeadChainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, layers, dtype, buffers, slots, *flat):
        L = len(layers)
        params = [None] * L
        for (i, name), t in zip(slots, flat):
            params[i] = params[i] or {}
            params[i][name] = t.detach().contiguous()
        for i, b in enumerate(buffers):
            if b is not None:
                params[i] = dict(params[i] or {}, moving_mean=b[0], moving_var=b[1])
        y, taps, _, ws = head_chain_forward(x.detach(), layers, params, dtype=dtype)
        ctx.save_for_backward(*flat)
        ctx.cfg = (tuple(x.shape), layers, dtype, slots, ws)
        ctx.tapped = [i for i, l in enumerate(layers) if l.get('tap')]
        ctx.y_shape = tuple(y.shape)
        ctx.set_materialize_grads(False)        # an output nobody used has no gradient: its dtap stays NULL
        return (y,) + tuple(taps[i] for i in ctx.tapped)

    @staticmethod
    def backward(ctx, dy, *dtap_list):
        x_shape, layers, dtype, slots, ws = ctx.cfg
        L = len(layers)
        params, need = [None] * L, [set() for _ in range(L)]
        for k, ((i, name), t) in enumerate(zip(slots, ctx.saved_tensors)):
            params[i] = params[i] or {}
            params[i][name] = t.detach().contiguous()
            if ctx.needs_input_grad[5 + k]:
                need[i].add(name)
        dtaps = [None] * L
        for i, g in zip(ctx.tapped, dtap_list):
            dtaps[i] = g
        if dy is None:          # only the taps carry gradients
            dy = torch.zeros(ctx.y_shape, dtype=torch.float32, device=ws.device)
        dx, grads = head_chain_backward(x_shape, layers, params, dy, dtaps, ws, dtype=dtype, need_dx=bool(ctx.needs_input_grad[0]), need=need)
        flat = tuple(None if grads[i] is None else grads[i].get(_HEAD_GRAD[name]) for i, name in slots)
        return (dx, None, None, None, None) + flat


def head_chain_fn(x, layers, params, dtype='bf16'):
    """The head chain as a torch.autograd.Function: returns (y, *taps), the taps in layer order.  `params` as in head_chain_forward;
    w, bias, w2, bias2, gamma, beta get gradients where autograd asks for them, 'moving_mean' / 'moving_var' are plain buffers that
    the forward updates in place and that get none.  The forward is ONE ron_head_chain_forward call into a workspace of its own, the
    backward ONE ron_head_chain_backward call reading it.  The results have the bytes of conv2d_nhwc_fn, batchnorm_nhwc_fn,
    maxpool2x2_nhwc_fn (and torch.cat for a pair) chained layer by layer."""
    L = len(layers)
    assert len(params) == L
    slots = [(i, name) for i in range(L) for name in _HEAD_IN if params[i] is not None and params[i].get(name) is not None]
    buffers = [None if p is None or p.get('moving_mean') is None else (p['moving_mean'], p['moving_var']) for p in params]
    return _HeadChainFn.apply(x, layers, dtype, buffers, slots, *[params[i][name] for i, name in slots])


# --------------------------------------------------------------------------- #
# backward of the 2x2 pool and of the 2x2 stride-2 convolutions (ron_maxpool2x2_backward_nhwc, ron_conv2d_k2s2_backward_nhwc):
# real entry points like the convolution backward - they enqueue on the current stream and never synchronise
# --------------------------------------------------------------------------- #
def maxpool2x2_backward_nhwc(x, dy, dtype='bf16'):
    """Gradient of maxpool2x2_nhwc at its input: x [N,H,W,C] (the pool's input), dy [N,ceil(H/2),ceil(W/2),C] GPU fp32 -> dx
    [N,H,W,C].  round(dy) goes to the first position (row-major in the window) whose rounded input equals the window's maximum,
    zero to the others (TensorFlow's MaxPoolGrad); every element of dx is written."""
    x, dy = x.contiguous(), dy.contiguous()
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and x.is_cuda and dy.is_cuda
    n, h, w, c = x.shape
    assert tuple(dy.shape) == (n, (h + 1) // 2, (w + 1) // 2, c), 'dy %s does not belong to x %s' % (tuple(dy.shape), tuple(x.shape))
    dx = torch.empty_like(x)
    check(lib().ron_maxpool2x2_backward_nhwc(ptr(x), ptr(dy), n, h, w, c, _lib.DTYPES[dtype], ptr(dx), current_stream()))
    return dx


def _k2s2_desc(n, h, w, cin, cout, relu, transpose, dtype, splitk):
    return _lib.ConvDesc(n, h, w, cin, cout, 2, 2, 2, 1, int(relu), int(transpose), _lib.DTYPES[dtype], -1, 0, 0, 0, splitk, 0)


def conv2d_k2s2_backward_workspace_bytes(n, h, w, cin, cout, relu=True, transpose=False, dtype='bf16', splitk=-1):
    """Bytes of workspace conv2d_k2s2_backward_nhwc needs (n, h, w: the input x; host arithmetic; raises on a refused descriptor)."""
    return _desc_workspace_bytes('conv2d_k2s2_backward', _k2s2_desc(n, h, w, cin, cout, relu, transpose, dtype, splitk))


def conv2d_k2s2_backward_nhwc(x, w, dy, y=None, relu=True, transpose=False, dtype='bf16', splitk=-1, need=('dx', 'dw', 'db'), workspace=None):
    """Gradients of the 2x2 stride-2 convolution (x [N,H,W,Cin], w HWIO [2,2,Cin,Cout], y and dy [N,H/2,W/2,Cout]) or, with
    `transpose`, of the 2x2 stride-2 transposed convolution (w [2,2,Cout,Cin], y and dy [N,2H,2W,Cout]): (dx, dw, db), None for
    those not in `need`.  Everything else as conv2d_backward_nhwc: GPU fp32 tensors (a numpy w is uploaded), the mask is y > 0
    with `relu`, dx comes back as storage-type values in fp32, dw (shaped like w) and db [Cout] as unrounded fp32 sums."""
    def describe(x, w, dy):
        n, h, wd, cin = x.shape
        cout = w.shape[2] if transpose else w.shape[3]
        assert tuple(w.shape) == ((2, 2, cout, cin) if transpose else (2, 2, cin, cout)), 'w %s' % (tuple(w.shape),)
        assert tuple(dy.shape) == ((n, 2 * h, 2 * wd, cout) if transpose else (n, h // 2, wd // 2, cout)), 'dy %s' % (tuple(dy.shape),)
        return cout, lambda: _k2s2_desc(n, h, wd, cin, cout, relu, transpose, dtype, splitk)
    return _conv_backward_call('conv2d_k2s2_backward', describe, x, w, dy, y, relu, need, workspace)


class _MaxPool2x2NhwcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.save_for_backward(x)
        ctx.dtype = dtype
        return maxpool2x2_nhwc(x.detach(), dtype=dtype)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return (maxpool2x2_backward_nhwc(x, dy, ctx.dtype) if ctx.needs_input_grad[0] else None), None


def maxpool2x2_nhwc_fn(x, dtype='bf16'):
    """maxpool2x2_nhwc as a torch.autograd.Function: the forward is the test operator ron_maxpool2x2_nhwc (it synchronises), the
    backward ONE ron_maxpool2x2_backward_nhwc call on the current stream (none when x does not require grad)."""
    return _MaxPool2x2NhwcFn.apply(x, dtype)


class _Conv2dK2s2NhwcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, relu, transpose, dtype):
        y = conv2d_forward_nhwc(x.detach(), w.detach(), None if bias is None else bias.detach(), relu=relu, stride=2, transpose=transpose,
                                dtype=dtype)
        ctx.save_for_backward(x, w, y)
        ctx.cfg = (relu, transpose, dtype, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        relu, transpose, dtype, has_bias = ctx.cfg
        need = _needed_grads(ctx, has_bias)
        dx, dw, db = (conv2d_k2s2_backward_nhwc(x, w, dy, y, relu=relu, transpose=transpose, dtype=dtype, need=need) if need
                      else (None, None, None))
        return dx, dw, db, None, None, None


def conv2d_k2s2_nhwc_fn(x, w, bias, relu=True, transpose=False, dtype='bf16'):
    """act(conv(x, w) + bias) for the 2x2 stride-2 convolution (w HWIO) or, with `transpose`, the 2x2 stride-2 transposed
    convolution (w [2,2,Cout,Cin]) as a torch.autograd.Function on GPU fp32 tensors.  The forward is ONE ron_conv2d_forward_nhwc call
    (device weights, the current stream, no synchronisation; its transposed form wants Cout a multiple of 128); the backward is ONE
    ron_conv2d_k2s2_backward_nhwc call on the current stream, computing only the gradients autograd asks for."""
    return _Conv2dK2s2NhwcFn.apply(x, w, bias, relu, transpose, dtype)


# --------------------------------------------------------------------------- #
# training-mode batch normalisation (ron_batchnorm_train_nhwc, ron_batchnorm_backward_nhwc): real entry points like the convolution
# backward - they enqueue on the current stream and never synchronise
# --------------------------------------------------------------------------- #
def _bn_desc(n, h, w, c, relu, eps, decay, dtype):
    return _lib.BnDesc(n, h, w, c, _lib.DTYPES[dtype], int(relu), float(eps), float(decay))


def _bn_vectors(c, dev, **named):
    """Per-channel arguments made contiguous and checked: float32 GPU tensors [c] (None stays None)."""
    out = []
    for name, t in named.items():
        if t is not None:
            t = t.contiguous()
            assert t.is_cuda and t.device == dev and t.dtype == torch.float32 and tuple(t.shape) == (c,), \
                '%s must be a float32 GPU tensor [%d]' % (name, c)
        out.append(t)
    return out


def batchnorm_workspace_bytes(n, h, w, c, relu=True, eps=1e-5, decay=0.997, dtype='bf16'):
    """Bytes of workspace batchnorm_train_nhwc and batchnorm_backward_nhwc need (host arithmetic; raises on a refused descriptor)."""
    return _desc_workspace_bytes('batchnorm', _bn_desc(n, h, w, c, relu, eps, decay, dtype))


def batchnorm_train_nhwc(x, gamma, beta, moving_mean=None, moving_var=None, relu=True, eps=1e-5, decay=0.997, dtype='bf16',
                         workspace=None):
    """Batch normalisation with batch statistics: (y, mean, var), new GPU fp32 tensors.

    x [N,H,W,C] GPU fp32 (a convolution's output; it is rounded to `dtype`), gamma and beta [C].  mean and the BIASED var [C] are
    those of the batch; y = round(act(gamma (xs - mean) / sqrt(var + eps) + beta)) comes back as storage-type values in fp32.
    `moving_mean` / `moving_var` [C], both or neither, are updated IN PLACE: m = decay m + (1 - decay) statistic, the variance
    Bessel-corrected (slim.batch_norm's decay; torch's momentum is 1 - decay).  `workspace`: a uint8 GPU tensor of at least
    batchnorm_workspace_bytes(...) bytes, or None for the cached per-device, per-stream buffer."""
    x = x.contiguous()
    dev = x.device
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
    n, h, w, c = x.shape
    gamma, beta = _bn_vectors(c, dev, gamma=gamma, beta=beta)
    for name, t in (('moving_mean', moving_mean), ('moving_var', moving_var)):        # updated in place: no copies
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (c,) and t.is_contiguous()), \
            '%s must be a contiguous float32 GPU tensor [%d]' % (name, c)
    d = _bn_desc(n, h, w, c, relu, eps, decay, dtype)
    ws = _sized_workspace(dev, lib().ron_batchnorm_workspace_bytes(C.byref(d))) if workspace is None else workspace
    y = torch.empty_like(x)
    mean = torch.empty((c,), dtype=torch.float32, device=dev)
    var = torch.empty((c,), dtype=torch.float32, device=dev)
    check(lib().ron_batchnorm_train_nhwc(C.byref(d), ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(var), ptr(moving_mean),
                                         ptr(moving_var), ptr(ws), int(ws.numel()), current_stream()))
    return y, mean, var


def batchnorm_backward_nhwc(x, y, dy, gamma, mean, var, relu=True, eps=1e-5, dtype='bf16', need=('dx', 'dgamma', 'dbeta'), workspace=None):
    """Gradients of batchnorm_train_nhwc: (dx, dgamma, dbeta), None for those not in `need`.

    x, dy (and y, the forward's output: required with `relu`, the mask is y > 0) [N,H,W,C] GPU fp32; gamma and the forward's mean
    and var [C].  dx comes back as storage-type values in fp32 - the dy of conv2d_backward_nhwc(relu=False) for the convolution in
    front - dgamma and dbeta [C] as unrounded fp32 sums in a fixed order."""
    x, dy = x.contiguous(), dy.contiguous()
    dev = x.device
    assert x.is_cuda and dy.is_cuda and x.dtype == torch.float32 and dy.dtype == torch.float32 and x.shape == dy.shape and x.dim() == 4
    n, h, w, c = x.shape
    if relu and y is None:
        raise _lib.RonError('batchnorm_backward_nhwc: relu=True needs the forward output y (the mask is y > 0)')
    if y is not None:
        y = y.contiguous()
        assert y.is_cuda and y.dtype == torch.float32 and y.shape == x.shape
    gamma, mean, var = _bn_vectors(c, dev, gamma=gamma, mean=mean, var=var)
    unknown = set(need) - {'dx', 'dgamma', 'dbeta'}
    assert not unknown, 'need: unknown output(s) %s' % sorted(unknown)
    d = _bn_desc(n, h, w, c, relu, eps, 0.0, dtype)
    ws = _sized_workspace(dev, lib().ron_batchnorm_workspace_bytes(C.byref(d))) if workspace is None else workspace
    names = [name for name in ('dx', 'dgamma', 'dbeta') if name in need]
    likes = {'dx': x, 'dgamma': gamma, 'dbeta': gamma}
    grads = _grad_outputs(None, names, tuple([likes[name]] for name in names), dev) if names else ()
    got = {name: g[0] for name, g in zip(names, grads)}
    dx, dgamma, dbeta = got.get('dx'), got.get('dgamma'), got.get('dbeta')
    check(lib().ron_batchnorm_backward_nhwc(C.byref(d), ptr(x), ptr(y if relu else None), ptr(dy), ptr(gamma), ptr(mean), ptr(var),
                                            ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), int(ws.numel()), current_stream()))
    return dx, dgamma, dbeta


class _BatchNormNhwcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, relu, eps, decay, dtype):
        y, mean, var = batchnorm_train_nhwc(x.detach(), gamma.detach(), beta.detach(), moving_mean, moving_var, relu=relu, eps=eps,
                                            decay=decay, dtype=dtype)
        ctx.save_for_backward(x, gamma, y, mean, var)
        ctx.cfg = (relu, eps, dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, y, mean, var = ctx.saved_tensors
        relu, eps, dtype = ctx.cfg
        need = tuple({'dx': 'dx', 'dw': 'dgamma', 'db': 'dbeta'}[name] for name in _needed_grads(ctx, True))     # (x, gamma, beta)
        dx, dgamma, dbeta = (batchnorm_backward_nhwc(x, y, dy, gamma, mean, var, relu=relu, eps=eps, dtype=dtype, need=need) if need
                             else (None, None, None))
        return dx, dgamma, dbeta, None, None, None, None, None, None


def batchnorm_nhwc_fn(x, gamma, beta, moving_mean, moving_var, relu=True, eps=1e-5, decay=0.997, dtype='bf16'):
    """batchnorm_train_nhwc as a torch.autograd.Function: x [N,H,W,C], gamma and beta [C] GPU fp32 tensors; moving_mean /
    moving_var [C] (both, or both None) are plain buffers updated in place by the forward.  Forward and backward are ONE library
    call each on the current stream; the backward computes only the gradients autograd asks for."""
    return _BatchNormNhwcFn.apply(x, gamma, beta, moving_mean, moving_var, relu, eps, decay, dtype)


# --------------------------------------------------------------------------- #
# the SSD-only operators (ron_maxpool3x3s1_*, ron_l2norm_*, ron_conv2d_padded_backward_nhwc): the forwards are test operators (they
# synchronise), the backwards real entry points like the convolution backward - they enqueue on the current stream and never synchronise
# --------------------------------------------------------------------------- #
def maxpool3x3s1_nhwc(x, dtype='bf16'):
    """slim.max_pool2d [3, 3] stride 1 SAME (pool5 of SSD) through the graph's kernel: [N,H,W,C] -> [N,H,W,C].  That kernel starts
    its maximum at 0, so this is TensorFlow's pool for NON-NEGATIVE x only (what pool5 sees behind a ReLU)."""
    x = x.contiguous()
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 4
    n, h, w, c = x.shape
    y = torch.empty_like(x)
    check(lib().ron_maxpool3x3s1_nhwc(ptr(x), n, h, w, c, _lib.DTYPES[dtype], ptr(y), current_stream()))
    return y


def maxpool3x3s1_backward_nhwc(x, dy, dtype='bf16'):
    """Gradient of the 3x3 stride-1 SAME max-pool at its input: x, dy [N,H,W,C] GPU fp32 -> dx [N,H,W,C].  Each window hands
    round(dy) to the first of its in-bounds positions (row-major) whose rounded input equals the window's maximum; a position
    adds what up to nine windows hand it in fp32 and rounds once (include/ron_hip.h); every element of dx is written."""
    x, dy = x.contiguous(), dy.contiguous()
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and x.is_cuda and dy.is_cuda and x.dim() == 4
    assert dy.shape == x.shape, 'dy %s does not belong to x %s' % (tuple(dy.shape), tuple(x.shape))
    n, h, w, c = x.shape
    dx = torch.empty_like(x)
    check(lib().ron_maxpool3x3s1_backward_nhwc(ptr(x), ptr(dy), n, h, w, c, _lib.DTYPES[dtype], ptr(dx), current_stream()))
    return dx


class _MaxPool3x3s1NhwcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.save_for_backward(x)
        ctx.dtype = dtype
        return maxpool3x3s1_nhwc(x.detach(), dtype=dtype)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return (maxpool3x3s1_backward_nhwc(x, dy, ctx.dtype) if ctx.needs_input_grad[0] else None), None


def maxpool3x3s1_nhwc_fn(x, dtype='bf16'):
    """maxpool3x3s1_nhwc as a torch.autograd.Function: the forward is the test operator ron_maxpool3x3s1_nhwc (non-negative x; it
    synchronises), the backward ONE ron_maxpool3x3s1_backward_nhwc call on the current stream (none when x does not require grad)."""
    return _MaxPool3x3s1NhwcFn.apply(x, dtype)


def _l2_gamma(gamma, c, dev):
    if not hasattr(gamma, 'data_ptr'):
        gamma = torch.from_numpy(np.ascontiguousarray(gamma, dtype=np.float32)).to(dev)
    return _bn_vectors(c, dev, gamma=gamma)[0]


def l2norm_nhwc(x, gamma, dtype='bf16'):
    """custom_layers.l2_normalization(scaling=True) over the channels (block4 of SSD) through the graph's kernel: x [N,H,W,C] GPU
    fp32, gamma [C] (a GPU fp32 tensor; a numpy array is uploaded) -> y = round(xs / sqrt(max(sum xs^2, 1e-12)) * gamma)."""
    x = x.contiguous()
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 4
    n, h, w, c = x.shape
    gamma = _l2_gamma(gamma, c, x.device)
    y = torch.empty_like(x)
    check(lib().ron_l2norm_nhwc(ptr(x), ptr(gamma), n, h, w, c, _lib.DTYPES[dtype], ptr(y), current_stream()))
    return y


def l2norm_backward_workspace_bytes(n, h, w, c, dtype='bf16'):
    """Bytes of workspace l2norm_backward_nhwc needs (host arithmetic; raises on a shape the library refuses)."""
    nbytes = lib().ron_l2norm_backward_workspace_bytes(n, h, w, c, _lib.DTYPES[dtype])
    if nbytes < 0:
        raise _lib.RonError('libron_hip: %s' % lib().ron_last_error().decode())
    return int(nbytes)


def l2norm_backward_nhwc(x, gamma, dy, dtype='bf16', need=('dx', 'dgamma'), workspace=None):
    """Gradients of l2norm_nhwc: (dx, dgamma), None for those not in `need`.  x, dy [N,H,W,C], gamma [C] GPU fp32.  dx comes back
    as storage-type values in fp32, dgamma [C] as an unrounded fp32 sum in a fixed order; a pixel whose sum of squares is below
    1e-12 takes the clamped branch (include/ron_hip.h).  `workspace`: a uint8 GPU tensor of at least
    l2norm_backward_workspace_bytes(...) bytes, or None for the cached per-device, per-stream buffer."""
    x, dy = x.contiguous(), dy.contiguous()
    dev = x.device
    assert x.is_cuda and dy.is_cuda and x.dtype == torch.float32 and dy.dtype == torch.float32 and x.shape == dy.shape and x.dim() == 4
    n, h, w, c = x.shape
    gamma = _l2_gamma(gamma, c, dev)
    unknown = set(need) - {'dx', 'dgamma'}
    assert not unknown, 'need: unknown output(s) %s' % sorted(unknown)
    ws = _workspace(dev, l2norm_backward_workspace_bytes(n, h, w, c, dtype)) if workspace is None else workspace
    dx = torch.empty_like(x) if 'dx' in need else None
    dgamma = torch.empty_like(gamma) if 'dgamma' in need else None
    check(lib().ron_l2norm_backward_nhwc(ptr(x), ptr(gamma), ptr(dy), n, h, w, c, _lib.DTYPES[dtype], ptr(dx), ptr(dgamma), ptr(ws),
                                         int(ws.numel()), current_stream()))
    return dx, dgamma


class _L2NormNhwcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, dtype):
        ctx.save_for_backward(x, gamma)
        ctx.dtype = dtype
        return l2norm_nhwc(x.detach(), gamma.detach(), dtype=dtype)

    @staticmethod
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        need = tuple(name for name, on in zip(('dx', 'dgamma'), ctx.needs_input_grad[:2]) if on)
        dx, dgamma = l2norm_backward_nhwc(x, gamma, dy, dtype=ctx.dtype, need=need) if need else (None, None)
        return dx, dgamma, None


def l2norm_nhwc_fn(x, gamma, dtype='bf16'):
    """l2norm_nhwc as a torch.autograd.Function: x [N,H,W,C], gamma [C] GPU fp32 tensors.  The forward is the test operator
    ron_l2norm_nhwc (it synchronises), the backward ONE ron_l2norm_backward_nhwc call on the current stream, computing only the
    gradients autograd asks for."""
    return _L2NormNhwcFn.apply(x, gamma, dtype)


def _padded_desc(n, h, w, cin, cout, stride, relu, dtype, splitk):
    return _lib.ConvDesc(n, h, w, cin, cout, 3, 3, stride, 1, int(relu), 0, _lib.DTYPES[dtype], -1, 0, 0, 0, splitk, 0)


def _padded_out_hw(h, w, k, stride, cpad):
    return (h + 2 * cpad - k) // stride + 1, (w + 2 * cpad - k) // stride + 1


def _is_block12(k, stride, cpad, h, w):
    """pad2d(1) + 4x4 VALID on a 2x2 map (block12 of SSD-512): only the filter's inner 2x2 taps meet data."""
    return k == 4 and stride == 1 and cpad == 1 and h == 2 and w == 2


def conv2d_padded_backward_workspace_bytes(n, h, w, cin, cout, stride=2, cpad=1, relu=True, dtype='bf16', splitk=-1):
    """Bytes of workspace conv2d_padded_backward_nhwc needs for a 3x3 convolution (n, h, w: the input x; host arithmetic; raises on
    what the library refuses)."""
    return _desc_workspace_bytes('conv2d_padded_backward', _padded_desc(n, h, w, cin, cout, stride, relu, dtype, splitk), int(cpad))


def conv2d_padded_backward_nhwc(x, w, dy, y=None, stride=2, cpad=1, relu=True, dtype='bf16', splitk=-1, need=('dx', 'dw', 'db'),
                                workspace=None):
    """Gradients of the padded convolutions of the SSD extra blocks, y = act(conv_VALID(pad2d(x, cpad), w, stride) + bias):
    (dx, dw, db), None for those not in `need`.  3x3 filters with (stride, cpad) = (2, 1) or (1, 0): ONE
    ron_conv2d_padded_backward_nhwc call; x [N,H,W,Cin], w HWIO [3,3,Cin,Cout], y and dy [N,Ho,Wo,Cout] with
    Ho = (H + 2 cpad - 3) // stride + 1.  A 4x4 filter with cpad 1 on a 2x2 map (block12 of SSD-512) meets data in its inner 2x2
    taps only: ONE ron_conv2d_k2s2_backward_nhwc call on w[1:3, 1:3], sliced and re-embedded on the device, dw zero in the twelve
    outer taps.  Anything else raises RonError.  Everything else as conv2d_backward_nhwc."""
    k = w.shape[0]
    if _is_block12(k, stride, cpad, x.shape[1], x.shape[2]):
        if not hasattr(w, 'data_ptr'):
            w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(x.device)
        assert tuple(w.shape[:2]) == (4, 4)
        dx, dwi, db = conv2d_k2s2_backward_nhwc(x, w[1:3, 1:3].contiguous(), dy, y, relu=relu, dtype=dtype, splitk=splitk, need=need,
                                                workspace=workspace)
        dw = None
        if dwi is not None:
            dw = torch.zeros_like(w)
            dw[1:3, 1:3] = dwi
        return dx, dw, db
    if k != 3 or tuple(w.shape[:2]) != (3, 3):
        raise _lib.RonError('conv2d_padded_backward_nhwc: filter %s, stride %d, cpad %d on a %d x %d map: 3x3 filters, or the 4x4 '
                            'filter with cpad 1 on a 2x2 map' % (tuple(w.shape[:2]), stride, cpad, x.shape[1], x.shape[2]))

    def describe(x, w, dy):
        n, h, wd, cin = x.shape
        cout = w.shape[3]
        assert tuple(w.shape) == (3, 3, cin, cout), 'w %s' % (tuple(w.shape),)
        if (stride, cpad) in ((2, 1), (1, 0)) and min(h, wd) + 2 * cpad >= 3:
            assert tuple(dy.shape) == (n,) + _padded_out_hw(h, wd, 3, stride, cpad) + (cout,), 'dy %s' % (tuple(dy.shape),)
        return cout, lambda: _padded_desc(n, h, wd, cin, cout, stride, relu, dtype, splitk)
    return _conv_backward_call('conv2d_padded_backward', describe, x, w, dy, y, relu, need, workspace, extra=(int(cpad),))


class _Conv2dPaddedNhwcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, cpad, relu, dtype):
        b = None if bias is None else bias.detach().cpu().numpy()
        wh = w.detach().cpu().numpy()
        k, (h, wd) = w.shape[0], x.shape[1:3]
        if _is_block12(k, stride, cpad, h, wd):
            y = conv2d_nhwc(x.detach(), wh[1:3, 1:3], b, stride=2, relu=relu, dtype=dtype)
        elif tuple(w.shape[:2]) == (3, 3) and (stride, cpad) in ((2, 1), (1, 0)) and min(h, wd) + 2 * cpad >= 3:
            # the stride-1 SAME convolution sampled at (o + stride oy, o + stride ox): the same values
            o = 1 - cpad
            ho, wo = _padded_out_hw(h, wd, 3, stride, cpad)
            full = conv2d_nhwc(x.detach(), wh, b, relu=relu, dtype=dtype)
            y = full[:, o::stride, o::stride][:, :ho, :wo].contiguous()
        else:
            raise _lib.RonError('conv2d_padded_nhwc_fn: filter %s, stride %d, cpad %d on a %d x %d map: 3x3 with (stride, cpad) = (2, 1) '
                                'or (1, 0), or 4x4 with cpad 1 on a 2x2 map' % (tuple(w.shape[:2]), stride, cpad, h, wd))
        ctx.save_for_backward(x, w, y)
        ctx.cfg = (stride, cpad, relu, dtype, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, cpad, relu, dtype, has_bias = ctx.cfg
        need = _needed_grads(ctx, has_bias)
        dx, dw, db = (conv2d_padded_backward_nhwc(x, w, dy, y, stride=stride, cpad=cpad, relu=relu, dtype=dtype, need=need) if need
                      else (None, None, None))
        return dx, dw, db, None, None, None, None


def conv2d_padded_nhwc_fn(x, w, bias, stride=2, cpad=1, relu=True, dtype='bf16'):
    """act(conv_VALID(pad2d(x, cpad), w, stride) + bias) for the convolutions of the SSD extra blocks as a torch.autograd.Function on GPU
    fp32 tensors: 3x3 with (stride, cpad) = (2, 1) or (1, 0), or 4x4 with cpad 1 on a 2x2 map (block12 of SSD-512); anything else
    raises RonError.  The forward of the 3x3 forms is ron_conv2d_nhwc at stride 1, sliced (host weights, synchronises: tests and
    small experiments); the backward is ONE entry-point call on the current stream (conv2d_padded_backward_nhwc)."""
    return _Conv2dPaddedNhwcFn.apply(x, w, bias, stride, cpad, relu, dtype)


# --------------------------------------------------------------------------- #
# the training update (ron_optimizer_step): one rule applied to a whole list of variables, a real entry point like the batch
# normalisation - it enqueues on the current stream and never synchronises
# --------------------------------------------------------------------------- #
def _opt_table(tensors, slots=2):
    """The host table of ron_optimizer_step: `tensors` is a list of (var, grad, slot0, slot1, weight_decay), the first four float32
    GPU tensors of one size (slots the rule does not use may be None).  Returns (table, n, device)."""
    n = len(tensors)
    table = (_lib.OptTensor * max(n, 1))()
    dev = None
    for i, (var, grad, slot0, slot1, wd) in enumerate(tensors):
        used = (var, grad) + (slot0, slot1)[:slots]
        for t in used:
            assert t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == var.numel(), \
                'tensor %d: var, grad and the slots the rule uses must be contiguous float32 GPU tensors of one size' % i
            assert dev is None or t.device == dev, 'tensor %d lives on another device' % i
            dev = t.device
        p = [C.c_void_p(t.data_ptr()) if t is not None else None for t in (var, grad, slot0, slot1)]
        table[i] = _lib.OptTensor(p[0], p[1], p[2] if slots >= 1 else None, p[3] if slots >= 2 else None, var.numel(), float(wd))
    return table, n, dev


def optimizer_plan(counts):
    """(launches, work units, table entries per launch, elements per work unit) of ron_optimizer_step for a list of element counts."""
    table = (_lib.OptTensor * max(len(counts), 1))()
    for i, c in enumerate(counts):
        table[i].count = int(c)
    out = (C.c_int64 * 4)()
    check(lib().ron_optimizer_plan(table, len(counts), out))
    return tuple(int(v) for v in out)


def optimizer_workspace_bytes(counts):
    """Bytes of workspace optimizer_step needs for reg_loss (host arithmetic on the counts; raises on a refused list)."""
    table = (_lib.OptTensor * max(len(counts), 1))()
    for i, c in enumerate(counts):
        table[i].count = int(c)
    nbytes = lib().ron_optimizer_workspace_bytes(table, len(counts))
    if nbytes < 0:
        check(-1)
    return int(nbytes)


def optimizer_step(rule, tensors, learning_rate, step=1, momentum=0.9, decay=0.9, beta1=0.9, beta2=0.999, epsilon=0.0,
                   want_reg_loss=False, workspace=None):
    """ONE ron_optimizer_step on the current stream: `rule` ('sgd' | 'momentum' | 'rmsprop' | 'adam') applied IN PLACE to every entry
    of `tensors`, a list of (var, grad, slot0, slot1, weight_decay) - float32 GPU tensors of one size each; slots the rule does not
    use may be None (momentum: slot0 = m; rmsprop: slot0 = ms, slot1 = mom; adam: slot0 = m, slot1 = v).  g' = g + weight_decay w where
    weight_decay != 0; TensorFlow 1.x's dense apply kernels in fp32, one rounding per operation (include/ron_hip.h).  `step` (>= 1)
    is Adam's.  Returns the regularisation loss sum (weight_decay / 2) sum(w^2) of the weights before the update as a GPU scalar when
    `want_reg_loss`, else None.  `workspace`: a uint8 GPU tensor of optimizer_workspace_bytes(...) bytes, or None for the cached
    per-device, per-stream buffer (only touched with want_reg_loss)."""
    if rule not in _lib.OPT_RULES:
        raise _lib.RonError('optimizer_step: unknown rule %r (sgd, momentum, rmsprop, adam)' % (rule,))
    code = _lib.OPT_RULES[rule]
    table, n, dev = _opt_table(tensors, (0, 1, 2, 2)[code])
    cfg = _lib.OptCfg(code, float(momentum), float(decay), float(beta1), float(beta2), float(epsilon))
    reg, ws, nbytes = None, None, 0
    if want_reg_loss and n:
        ws = _sized_workspace(dev, lib().ron_optimizer_workspace_bytes(table, n)) if workspace is None else workspace
        nbytes = int(ws.numel())
        reg = torch.empty((), dtype=torch.float32, device=dev)
    check(lib().ron_optimizer_step(C.byref(cfg), table, n, float(learning_rate), int(step), ptr(reg), ptr(ws), nbytes, current_stream()))
    return reg
