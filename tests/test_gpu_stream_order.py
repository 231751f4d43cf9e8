"""GPU: the stream contract of include/ron_hip.h on a stalled side stream ("Stream contract").

Every stand-alone entry point (through its Python wrapper, which passes torch's current stream) and every context call runs on a
stream that is busy with a long, finite stall, with its real inputs X copied into the input buffers only behind that stall; until
then the buffers (and, for a context, its activations) hold another valid case X'.  The result must equal, bit for bit, the one
computed from X on the default stream: the values themselves are graded by the parity tests, here only the order is.  A kernel,
memset or helper that went to another stream, a side lane that did not wait for its reference map, or scratch shared between streams
runs during the stall and gives the result of X' (or is overwritten).  Entries not documented to synchronise must also return
while the stall is pending.  Three positive controls make the mistake on purpose (the call goes to the default stream) and must
NOT give the expected result; no test passes with an expired stall (tests/stream_util.py)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_cases as ec  # noqa: E402
import match_cases as mc  # noqa: E402
import ssd_loss_cases as sc  # noqa: E402
import stream_util as su  # noqa: E402
import train_pre_cases as tc  # noqa: E402
from oracle import anchors as oanchors  # noqa: E402
from oracle import np_post, synth  # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
DET_FIELDS = ('classes', 'scores', 'bboxes', 'anchor_index', 'count')
HOST_MS = {}              # label -> host milliseconds of the call on the idle default stream (what a stall has to outlast)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def report_stall_against_enqueue_times():
    """Prints, behind the module's tests, the figures DESIGN.md quotes: the slowest host call on the idle default stream and the
    slowest stall-to-last-enqueue time on the stalled stream.  Every run_late() has asserted that its own stall outlasted its enqueue."""
    yield
    held = {e[0] for e in ENTRIES if e[2]}
    free = {k: v for k, v in su.ENQUEUE_MS.items() if k not in held}
    if HOST_MS and free:
        slow_host, slow_enq = max(HOST_MS, key=HOST_MS.get), max(free, key=free.get)
        print('\nstream contract: stall %g ms; slowest host call on the idle default stream: %s, %.3f ms; slowest enqueue on the stalled '
              'stream among the calls that do not hold the host: %s, %.3f ms' % (su.STALL_MS, slow_host, HOST_MS[slow_host], slow_enq,
                                                                                free[slow_enq]))


@pytest.fixture(scope='module')
def side(dev):
    return su.independent_stream(dev, 0)


@pytest.fixture(scope='module')
def side2(dev):
    return su.independent_stream(dev, 1)


@pytest.fixture(scope='module')
def adev(dev):
    from ron_tensorflow_amd import ops
    return ops.anchors_to_device(oanchors.anchors_all_layers(), dev)


def _up(arrays, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _det(d):
    return [getattr(d, f) for f in DET_FIELDS]


def _clones(tensors):
    return [t.clone() for t in tensors]


# --------------------------------------------------------------------------------------------------------------- the pattern
def expect_and_poison(label, entry, x, xp, host_inputs=False):
    """Steps 1 and 2 of the pattern, on the default stream: `expected` from the real inputs x, then the input buffers left holding
    the poison xp, whose result must differ.  Returns (expected, input buffers)."""
    expected = _clones(entry(x))
    torch.cuda.synchronize()
    bufs = xp if host_inputs else _clones(xp)
    t0 = time.perf_counter()
    out = entry(bufs)
    HOST_MS[label] = (time.perf_counter() - t0) * 1e3
    poisoned = _clones(out)
    torch.cuda.synchronize()
    assert not su.same_bytes(expected, poisoned), '%s: the poison gives the expected result, it cannot show a misordered read' % label
    return expected, bufs


def check_late(stream, label, entry, x, xp, blocks_host=False, host_inputs=False, stall_ms=None):
    """The whole pattern for one entry: entry(list of inputs) -> list of output tensors.  x / xp: the real case and the poison,
    device tensors (or, host_inputs, host arrays that the wrapper uploads itself: then that upload, made on the stalled stream,
    is the late input)."""
    expected, bufs = expect_and_poison(label, entry, x, xp, host_inputs)

    def fill():
        if not host_inputs:
            for b, t in zip(bufs, x):
                b.copy_(t, non_blocking=True)

    got = su.run_late(stream, fill, lambda: entry(x if host_inputs else bufs), _clones, blocks_host=blocks_host, stall_ms=stall_ms,
                      label=label)
    print('%s: host call %.3f ms on the idle default stream, %.3f ms from stall to last enqueue on the stalled stream (stall %g ms)'
          % (label, HOST_MS[label], su.ENQUEUE_MS[label], su.STALL_MS if stall_ms is None else stall_ms))
    assert su.same_bytes(got, expected), '%s: the result on the stalled stream differs from the default-stream result' % label
    return expected


def check_misdirected(stream, label, entry, x, xp):
    """Positive control: the same late inputs, the call on the default stream.  It must NOT give the expected result."""
    expected, bufs = expect_and_poison(label, entry, x, xp)

    def fill():
        for b, t in zip(bufs, x):
            b.copy_(t, non_blocking=True)

    got = su.run_misdirected(stream, fill, lambda: entry(bufs), _clones)
    assert not su.same_bytes(got, expected), '%s: a call on the wrong stream went unnoticed: the harness cannot fail' % label
    assert su.same_bytes(_clones(bufs), _clones(x))          # the late inputs did arrive, after the misdirected call had read


# --------------------------------------------------------------------------------------------------------------- stand-alone entries
def _heads(seed, batch=1, bg=8.0, ob=-4.0, loc_scale=1.0, cls_scale=1.0):
    cls, obj, loc = synth.head_tensors(seed, batch=batch, bg=bg, ob=ob)
    return ([c * np.float32(cls_scale) for c in cls], obj, [l * np.float32(loc_scale) for l in loc])


def _split(flat, *counts):
    out, lo = [], 0
    for c in counts:
        out.append(list(flat[lo:lo + c]))
        lo += c
    return out


def _entry_softmax(dev, adev):
    from ron_tensorflow_amd import ops
    return (lambda t: [ops.softmax_last(t[0])],) + tuple([synth.head_tensors(s, batch=2)[0][1]] for s in (1, 2))


def _entry_softmax_pick(dev, adev):
    from ron_tensorflow_amd import ops
    return (lambda t: [ops.softmax_last(t[0], pick=1)],) + tuple([synth.head_tensors(s, batch=2)[1][2]] for s in (1, 2))


def _entry_decode(dev, adev):
    from ron_tensorflow_amd import ops
    return (lambda t: [ops.bboxes_decode_layer(t[0], adev[1])],) + tuple([synth.head_tensors(s, batch=2)[2][1]] for s in (3, 4))


def _post_np_out(res):
    out, srt, ncand = res
    return _det(out) + (_det(srt) if srt is not None else []) + [ncand]


def _entry_post_np_logits(dev, adev):
    """One image with ~190 k candidates (more than kPartMin = 16384 of csrc/postproc.hip): topk_partial_kernel runs."""
    from ron_tensorflow_amd import ops

    def entry(t):
        cls, obj, loc = _split(t, 4, 4, 4)
        return _post_np_out(ops.post_np(cls, obj, loc, adev))
    return (entry,) + tuple(sum(_heads(s, 1, bg=4.0, ob=-2.0), []) for s in (103, 113))


def _entry_post_np_probabilities(dev, adev):
    from ron_tensorflow_amd import ops

    def entry(t):
        cls, obj, loc = _split(t, 4, 4, 4)
        return _post_np_out(ops.post_np(cls, obj, loc, adev, cls_is_prob=True, obj_is_prob=True))

    def make(seed):
        cls, obj, loc = _heads(seed, 2)
        return [np_post.softmax_last(c) for c in cls] + [np_post.objectness_from_logits(o) for o in obj] + loc
    return entry, make(100), make(110)


def _entry_post_np_want_sorted(dev, adev):
    from ron_tensorflow_amd import ops

    def entry(t):
        cls, obj, loc = _split(t, 4, 4, 4)
        return _post_np_out(ops.post_np(cls, obj, loc, adev, want_sorted=True))
    return (entry,) + tuple(sum(_heads(s, 2, bg=7.0, ob=-3.0), []) for s in (102, 112))


def _entry_post_np_loc_decoded(dev, adev):
    from ron_tensorflow_amd import ops
    anchors = oanchors.anchors_all_layers()

    def entry(t):
        cls, obj, loc = _split(t, 4, 4, 4)
        return _post_np_out(ops.post_np(cls, obj, loc, None, loc_decoded=True))

    def make(seed):
        cls, obj, loc = _heads(seed, 2)
        return cls + obj + [np_post.bboxes_decode_layer(l, a) for l, a in zip(loc, anchors)]
    return entry, make(104), make(114)


def _boxes(rs, shape, lo=0.05, hi=0.3):
    yx = rs.uniform(0, 0.7, shape + (2,))
    return np.concatenate([yx, yx + rs.uniform(lo, hi, shape + (2,))], -1).astype(np.float32)


def _entry_np_sort_nms(dev, adev):
    from ron_tensorflow_amd import ops

    def entry(t):
        out, srt = ops.np_sort_nms(t[0], t[1], t[2], want_sorted=True)
        return _det(out) + _det(srt)

    def make(seed):
        rs = np.random.RandomState(seed)
        return [rs.randint(1, 21, (2, 1500)).astype(np.int32), rs.uniform(0, 1, (2, 1500)).astype(np.float32), _boxes(rs, (2, 1500))]
    return entry, make(5), make(6)


def _entry_bboxes_filter_min(dev, adev):
    from ron_tensorflow_amd import ops

    def make(seed):
        rs = np.random.RandomState(seed)
        return [rs.uniform(0, 1, (2, 300)).astype(np.float32), _boxes(rs, (2, 300), 0.0, 0.08)]      # about 40 % of the rows pass
    return (lambda t: list(ops.bboxes_filter_min(t[0], t[1], top_k=50)),) + (make(7), make(8))


def _entry_tfe_detected_bboxes(dev, adev):
    from ron_tensorflow_amd import tfe
    anchors = oanchors.anchors_all_layers()

    def entry(t):
        pred, dec = _split(t, 4, 4)
        ds, db = tfe.detected_bboxes(pred, dec, num_classes=21, select_threshold=0.01, nms_threshold=0.4, clipping_bbox=[0., 0., 1., 1.],
                                     top_k=200, keep_top_k=100, nms_mode='min')
        return [torch.stack([ds[c] for c in range(1, 21)]), torch.stack([db[c] for c in range(1, 21)])]

    def make(seed):
        cls, obj, loc = _heads(seed, 2, loc_scale=0.2)
        gated = [(np_post.objectness_from_logits(o) > 0.03).astype(np.float32) * np_post.softmax_last(c) for c, o in zip(cls, obj)]
        return gated + [np_post.bboxes_decode_layer(l, a) for l, a in zip(loc, anchors)]
    return entry, make(200), make(210)


def _entry_post_eval(mode):
    def build(dev, adev):
        from ron_tensorflow_amd import ron_eval
        anchors = oanchors.anchors_all_layers()

        def entry(t):
            pred, objp, dec = _split(t, 4, 4, 4)
            return _det(ron_eval.post_eval(pred, objp, dec, None, [(375, 500), (500, 333)], objectness_thres=0.5, select_threshold=0.3,
                                           nms_threshold=0.4, keep_top_k=20, nms_mode='union', nms_by_class=mode))

        def make(seed):
            cls, obj, loc = _heads(seed, 2, bg=2.0, ob=1.0, loc_scale=0.2, cls_scale=3.0)
            return ([np_post.softmax_last(c) for c in cls] + [np_post.objectness_from_logits(o) for o in obj] +
                    [np_post.bboxes_decode_layer(l, a) for l, a in zip(loc, anchors)])
        return entry, make(300), make(310)
    return build


def _entry_pack_records(dev, adev):
    from ron_tensorflow_amd import ops, parallel

    def entry(t):
        det = object.__new__(ops.DetectionBuffers)               # a DetectionBuffers over the five given tensors
        det.n, det.capacity = t[1].shape
        for f, v in zip(DET_FIELDS, t):
            setattr(det, f, v)
        return [parallel.pack_detections(det)]

    def make(seed):
        rs = np.random.RandomState(seed)
        count = rs.randint(1, 400, (2,)).astype(np.int32)
        live = np.arange(400)[None, :] < count[:, None]
        return [np.where(live, rs.randint(1, 21, (2, 400)), 0).astype(np.int32), np.where(live, rs.uniform(0, 1, (2, 400)), 0).astype(np.float32),
                (_boxes(rs, (2, 400)) * live[..., None]).astype(np.float32), np.where(live, rs.randint(0, 21250, (2, 400)), 0).astype(np.int32),
                count]
    return entry, make(9), make(10)


def _entry_bboxes_matching(dev, adev):
    from ron_tensorflow_amd import metrics
    make = lambda seed: [a.astype(np.int32) if a.dtype == np.int64 else a for a in mc.random_inputs(seed, 2, 20, 50, 12)]
    return (lambda t: list(metrics.bboxes_matching(t[0], t[1], t[2], t[3], t[4], 0.5)),) + (make(11), make(12))


def _entry_bboxes_encode(dev, adev):
    from ron_tensorflow_amd import ops
    anchors = ec.ron320_anchors()
    a_dev = ops.anchors_to_device(anchors, dev)
    shapes = [(int(np.shape(y)[0]), int(np.shape(y)[1]), int(np.size(h))) for (y, x, h, w) in anchors]

    def entry(t):
        return sum(ops.bboxes_encode(t[0], t[1], a_dev, shapes, (320, 320), ec.RON_BORDERS), [])
    return (entry,) + tuple(list(ec.random_ground_truth(s, 2, 7, counts=[3, 7])) for s in (13, 14))


LOSS_KEYS = ('logits', 'localisations', 'objness_logits', 'objness_pred', 'gclasses', 'glocalisations')
LOSS_SHAPES = [(5, 5, 10), (10, 10, 10)]           # 2500 rows for two images: several workgroups per kernel


def _loss_inputs(seed):
    d = ec.loss_inputs(seed, n=2, shapes=LOSS_SHAPES)
    return sum((d[k] for k in LOSS_KEYS), []) + [d['rand_objness'], d['rand_cls']]


def _loss_args(t):
    per = _split(t, 2, 2, 2, 2, 2, 2)
    return dict(zip(LOSS_KEYS, per), rand_objness=t[12], rand_cls=t[13])


def _entry_losses(dev, adev):
    from ron_tensorflow_amd import ops
    return (lambda t: list(ops.losses(**_loss_args(t))),) + (_loss_inputs(15), _loss_inputs(16))


def _entry_losses_grad(dev, adev):
    from ron_tensorflow_amd import ops

    def entry(t):
        a = _loss_args(t)
        out = tuple([torch.full(x.shape, SENTINEL, dtype=torch.float32, device=dev) for x in a[k]]
                    for k in ('logits', 'objness_logits', 'localisations'))
        losses, counts, d_cls, d_obj, d_loc = ops.losses_grad(**a, out=out)
        return [losses, counts] + d_cls + d_obj + d_loc
    return entry, _loss_inputs(15), _loss_inputs(16)


SSD_KEYS = ('logits', 'localisations', 'gclasses', 'glocalisations', 'gscores')
SSD_ROWS = [64, 256, 514]


def _ssd_inputs(mining, seed):
    case = sc.random_case('stream_order', mining, 2, SSD_ROWS, 21, seed, pos_rate=0.05)
    return sum((getattr(case, k) for k in SSD_KEYS), [])


def _entry_ssd_losses(mining):
    def build(dev, adev):
        from ron_tensorflow_amd import ops

        def entry(t):
            losses, counts, nv = ops.ssd_losses(**dict(zip(SSD_KEYS, _split(t, 3, 3, 3, 3, 3))), mining=mining, nvalues=True)
            return [losses, counts, nv]
        return entry, _ssd_inputs(mining, 17), _ssd_inputs(mining, 18)
    return build


def _ssd_grad_entry(dev, mining):
    from ron_tensorflow_amd import ops

    def entry(t):
        a = dict(zip(SSD_KEYS, _split(t, 3, 3, 3, 3, 3)))
        out = tuple([torch.full(x.shape, SENTINEL, dtype=torch.float32, device=dev) for x in a[k]] for k in ('logits', 'localisations'))
        losses, counts, nv, d_cls, d_loc = ops.ssd_losses_grad(**a, mining=mining, nvalues=True, out=out)
        return [losses, counts, nv] + d_cls + d_loc
    return entry


def _entry_ssd_losses_grad(mining):
    return lambda dev, adev: (_ssd_grad_entry(dev, mining), _ssd_inputs(mining, 17), _ssd_inputs(mining, 18))


PRE_SIZES = [(33, 21), (12, 19), (5, 7)]
PRE_OUT = (20, 12)
MEANS = (123., 117., 104.)


def _packed(seed):
    """(packed uint8, offsets int64 [n], hw int32 [n, 2]) of three seeded images of PRE_SIZES, as numpy."""
    imgs = [tc.random_image(seed + i, h, w) for i, (h, w) in enumerate(PRE_SIZES)]
    sizes = np.array([a.size for a in imgs], np.int64)
    return [np.concatenate([a.reshape(-1) for a in imgs]), np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64),
            np.array(PRE_SIZES, np.int32)]


def _entry_preprocess_eval(dev, adev):
    from ron_tensorflow_amd import _lib

    def entry(t):
        out = torch.full((len(PRE_SIZES),) + PRE_OUT + (3,), SENTINEL, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ron_preprocess_eval(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), len(PRE_SIZES), PRE_OUT[0], PRE_OUT[1],
                                                  (C.c_float * 3)(*MEANS), _lib.ptr(out), _lib.current_stream()))
        return [out]
    return entry, _packed(40), _packed(50)


def _entry_preprocess_eval_geom(dev, adev):
    from ron_tensorflow_amd import _lib
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp

    def entry(t):
        out = torch.full((len(PRE_SIZES),) + PRE_OUT + (3,), SENTINEL, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ron_preprocess_eval_geom(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), len(PRE_SIZES),
                                                       PRE_OUT[0], PRE_OUT[1], (C.c_float * 3)(*MEANS), _lib.ptr(out), _lib.current_stream()))
        return [out]
    geom = lambda mode: np.array([pp.eval_geometry(h, w, PRE_OUT, mode)[0] for h, w in PRE_SIZES], np.int32)
    return entry, _packed(40) + [geom(pp.Resize.CENTRAL_CROP)], _packed(50) + [geom(pp.Resize.PAD_AND_RESIZE)]


def _entry_preprocess_eval_wrapper(dev, adev):
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp
    imgs = lambda seed: [tc.random_image(seed + i, h, w) for i, (h, w) in enumerate(PRE_SIZES)]
    return (lambda t: [pp.preprocess_for_eval_batch(t, PRE_OUT, pp.Resize.WARP_RESIZE, device=dev)],) + (imgs(40), imgs(50))


def _geometry_inputs(seed):
    items = tc.random_images(seed, 4, g_choices=(3,))
    for it in items:                                   # at least one present row per image, so that the boxes matter
        it[3][0] = max(int(it[3][0]), 1)
        if not it[4][0].any():
            it[4][0] = np.array([0.2, 0.3, 0.7, 0.6], np.float32)
    return [np.array([[h, w] for (h, w, _, _, _, _) in items], np.int32), np.stack([i[3] for i in items]),
            np.stack([i[4] for i in items]), np.stack([i[5] for i in items])]


def _entry_train_geometry(dev, adev):
    from ron_tensorflow_amd import _lib

    def entry(t):
        n, g = t[1].shape
        geom = torch.full((n, _lib.RON_TRAIN_GEOM), -7, dtype=torch.int32, device=dev)
        gl, gb = torch.full((n, g), -7, dtype=torch.int32, device=dev), torch.full((n, g, 4), SENTINEL, dtype=torch.float32, device=dev)
        counts = torch.full((n,), -7, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().ron_train_geometry(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), n, g, _lib.ptr(t[3]), _lib.ptr(geom),
                                                 _lib.ptr(gl), _lib.ptr(gb), _lib.ptr(counts), _lib.current_stream()))
        return [geom, gl, gb, counts]
    return entry, _geometry_inputs(77), _geometry_inputs(78)


def _entry_preprocess_train(dev, adev):
    """The pixel kernels on hand-made geometry tables of tests/train_pre_cases.py (expand with a window across the fill + flip: the
    channel sums, their memset and both kernels run)."""
    from ron_tensorflow_amd import _lib
    lib = _lib.lib()
    h0, h1, h2 = PRE_SIZES
    combined = np.stack([tc.geom_row(h0[0], h0[1], True, (20, 11), (10, 5, 40, 30), True), tc.geom_row(h1[0], h1[1], crop=(2, 3, 9, 15), flip=True),
                         tc.geom_row(h2[0], h2[1], True, (4, 6), (2, 1, 8, 13), True)])
    plain = np.stack([tc.geom_row(h, w, True, (1, 1), (0, 0, h + 2, w + 2)) for h, w in PRE_SIZES])

    def entry(t):
        n = len(PRE_SIZES)
        nbytes = lib.ron_preprocess_train_workspace_bytes(n)
        ws = torch.full((int(nbytes),), 0xAB, dtype=torch.uint8, device=dev)       # the call zeroes its workspace itself
        out = torch.full((n,) + PRE_OUT + (3,), SENTINEL, dtype=torch.float32, device=dev)
        _lib.check(lib.ron_preprocess_train(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), n, PRE_OUT[0], PRE_OUT[1],
                                            (C.c_float * 3)(*MEANS), _lib.ptr(ws), _lib.ptr(out), _lib.current_stream()))
        return [out]
    return entry, _packed(40) + [combined], _packed(50) + [plain]


def _entry_preprocess_train_wrapper(dev, adev):
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp

    def entry(t):
        imgs, gl, gb, draws = t
        return list(pp.ron_preprocess_for_train_batch(imgs, gl, gb, PRE_OUT, draws=draws, device=dev))

    def make(seed):
        hw, gl, gb, draws = _geometry_inputs(seed)
        return [[tc.random_image(seed + i, int(h), int(w)) for i, (h, w) in enumerate(hw)], gl, gb, draws]
    return entry, make(77), make(78)


# name -> (builder(dev, adev) -> (entry, X, X'), blocks the host by contract, the wrapper uploads host arrays itself)
ENTRIES = [
    ('softmax_last', _entry_softmax, False, False),
    ('softmax_last_pick', _entry_softmax_pick, False, False),
    ('bboxes_decode_layer', _entry_decode, False, False),
    ('post_np_from_logits_topk_partial', _entry_post_np_logits, False, False),
    ('post_np_from_probabilities', _entry_post_np_probabilities, False, False),
    ('post_np_want_sorted', _entry_post_np_want_sorted, False, False),
    ('post_np_loc_decoded', _entry_post_np_loc_decoded, False, False),
    ('np_sort_nms', _entry_np_sort_nms, False, False),
    ('bboxes_filter_min', _entry_bboxes_filter_min, True, False),                      # reads the counts back (ops.bboxes_filter_min)
    ('tfe_detected_bboxes_ron_post_tfe', _entry_tfe_detected_bboxes, False, False),
    ('ron_post_eval_agnostic', _entry_post_eval(False), False, False),
    ('ron_post_eval_by_class', _entry_post_eval(True), False, False),
    ('ron_post_eval_by_class_scores', _entry_post_eval('scores'), False, False),
    ('parallel_pack_records', _entry_pack_records, False, False),
    ('metrics_bboxes_matching', _entry_bboxes_matching, False, False),
    ('bboxes_encode', _entry_bboxes_encode, False, False),
    ('losses', _entry_losses, False, False),
    ('losses_grad', _entry_losses_grad, False, False),
    ('ssd_losses_batch', _entry_ssd_losses('batch'), False, False),
    ('ssd_losses_layer', _entry_ssd_losses('layer'), False, False),
    ('ssd_losses_grad_batch', _entry_ssd_losses_grad('batch'), False, False),
    ('ssd_losses_grad_layer', _entry_ssd_losses_grad('layer'), False, False),
    ('ron_preprocess_eval', _entry_preprocess_eval, False, False),
    ('ron_preprocess_eval_geom', _entry_preprocess_eval_geom, False, False),
    ('preprocess_for_eval_batch', _entry_preprocess_eval_wrapper, True, True),         # packs and uploads the images
    ('ron_train_geometry', _entry_train_geometry, False, False),
    ('ron_preprocess_train', _entry_preprocess_train, False, False),
    ('ron_preprocess_for_train_batch', _entry_preprocess_train_wrapper, True, True),   # packs and uploads images, ground truth, draws
]


@pytest.mark.parametrize('name,build,blocks,host_inputs', ENTRIES, ids=[e[0] for e in ENTRIES])
def test_entry_late_inputs(dev, side, adev, name, build, blocks, host_inputs):
    entry, x, xp = build(dev, adev)
    if not host_inputs:
        x, xp = _up(x, dev), _up(xp, dev)
    expected = check_late(side, name, entry, x, xp, blocks_host=blocks, host_inputs=host_inputs)
    if name == 'post_np_from_logits_topk_partial':
        assert int(expected[-1].max()) > 16384, 'no image has more than kPartMin candidates: topk_partial_kernel did not run'


# --------------------------------------------------------------------------------------------------------------- positive controls
def test_control_misdirected_softmax_last(dev, side, adev):
    entry, x, xp = _entry_softmax(dev, adev)
    check_misdirected(side, 'control softmax_last', entry, _up(x, dev), _up(xp, dev))


def test_control_misdirected_post_np_from_logits(dev, side, adev):
    entry, x, xp = _entry_post_np_logits(dev, adev)
    check_misdirected(side, 'control post_np', entry, _up(x, dev), _up(xp, dev))


def test_control_misdirected_detect(dev, side, ron_single):
    net, x, xp = ron_single
    check_misdirected(side, 'control RONNet.detect', lambda t: _det(net.detect(t[0])), [x], [xp])


# --------------------------------------------------------------------------------------------------------------- contexts
def _ron(dev, multi_stream):
    from ron_tensorflow_amd import weights as W
    from ron_tensorflow_amd.nets import nets_factory
    net = nets_factory.get_network('ron_320_vgg')(variant='reducedfc', dtype='bf16', max_batch=2, device=dev, multi_stream=multi_stream)
    net.load_weights(W.synthetic_weights('reducedfc', seed=1))
    x, xp = (torch.from_numpy(W.synthetic_images(2, seed=s)).to(dev) for s in (21, 22))
    return net, x, xp


@pytest.fixture(scope='module')
def ron_single(dev):
    net, x, xp = _ron(dev, False)
    yield net, x, xp
    net.close()


@pytest.fixture(scope='module')
def ron_multi(dev):
    net, x, xp = _ron(dev, True)
    yield net, x, xp
    net.close()


@pytest.fixture(scope='module')
def ssd300(dev):
    from ron_tensorflow_amd import weights as W
    from ron_tensorflow_amd.nets import nets_factory
    cls = nets_factory.get_network('ssd_300_vgg')
    net = cls(cls.default_params._replace(num_classes=21), dtype='fp32', max_batch=1, device=dev)
    net.load_weights(W.ssd300_synthetic_weights(seed=6))
    x, xp = (torch.from_numpy(W.synthetic_images(1, seed=s, img_shape=(300, 300))).to(dev) for s in (4, 5))
    yield net, x, xp
    net.close()


def _heads_out(res):
    return sum((list(lst) for lst in res if lst is not None), [])


def _tfe_out(res):
    ds, db = res
    keys = sorted(ds)
    return [torch.stack([ds[c] for c in keys]), torch.stack([db[c] for c in keys])]


def _context_calls(net, coarse, vgg):
    """name -> entry(list with the image batch) for the calls of one context; the end points are read behind a forward pass on
    the same stream: `coarse` is the input of a coarse scale's heads, `vgg` a map of the backbone."""
    def end_point(name):
        def entry(t):
            net.forward_heads(t[0])
            return [net.end_point(name, t[0].shape[0])]
        return entry
    return {'forward_heads': lambda t: _heads_out(net.forward_heads(t[0])),
            'end_point_' + coarse: end_point(coarse),
            'end_point_' + vgg: end_point(vgg),
            'detect': lambda t: _det(net.detect(t[0])),
            'detect_tfe': lambda t: _tfe_out(net.detect_tfe(t[0]))}


RON_CALLS = ('forward_heads', 'end_point_block7_ref', 'end_point_conv4_3', 'detect', 'detect_tfe')
SSD_CALLS = ('forward_heads', 'end_point_block7', 'end_point_conv4_3', 'detect', 'detect_tfe')


def _ron_context_case(side, tag, fixture, call):
    """The call with n = max_batch = 2 on the stalled stream, the context's activations holding another batch; then with n = 1 through
    the same stream (the post-processing workspace is laid out for max_batch and cleans itself for calls of any n)."""
    net, x, xp = fixture
    entry = _context_calls(net, 'block7_ref', 'conv4_3')[call]
    check_late(side, '%s %s n=2' % (tag, call), entry, [x], [xp])
    check_late(side, '%s %s n=1' % (tag, call), entry, [x[:1].clone()], [xp[:1].clone()])


@pytest.mark.parametrize('call', RON_CALLS)
def test_ron_single_stream_context(side, ron_single, call):
    _ron_context_case(side, 'ron single-stream', ron_single, call)


@pytest.mark.parametrize('call', RON_CALLS)
def test_ron_multi_stream_context(side, ron_multi, call):
    """RON_CFG_MULTI_STREAM: the head branches of block7 / 6 / 5 run on the context's side streams, forked behind their reference
    maps and joined before control returns.  A lane that did not wait for `lane_ready` would start during the stall, on activations
    that hold the other batch."""
    _ron_context_case(side, 'ron multi-stream', ron_multi, call)


@pytest.mark.parametrize('call', SSD_CALLS)
def test_ssd300_context(side, ssd300, call):
    net, x, xp = ssd300
    check_late(side, 'ssd300 %s' % call, _context_calls(net, 'block7', 'conv4_3')[call], [x], [xp])


# --------------------------------------------------------------------------------------------------------------- slot set-up
def _hip_runtime():
    """The HIP runtime this process has ALREADY loaded (torch's, which libron_hip.so resolves to as well), opened by the path it was
    mapped from: never a second copy."""
    from ron_tensorflow_amd import _lib
    _lib.lib()
    with open('/proc/self/maps') as f:
        paths = sorted({line.split()[-1] for line in f if 'libamdhip64' in line})
    assert len(paths) == 1, 'expected one HIP runtime in the process, found %r' % (paths,)
    return C.CDLL(paths[0])


def _raw_hipmemset_behind_a_busy_null_stream(dev, side):
    """What the runtime's synchronous-looking hipMemset does with the null stream busy: (the memory was zero when the call had
    returned, the host was held until the stall had ended).  Read from an independent stream, at once; the buffer is torch's and both
    answers are valid outcomes, so nothing can fault.  A record for DESIGN.md, not an assertion on the runtime."""
    hip = _hip_runtime()
    hip.hipMemset.restype = C.c_int
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    buf = torch.full((1 << 22,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    marker = su.stall(torch.cuda.default_stream(dev))
    pending = marker.query() is False
    rc = hip.hipMemset(C.c_void_p(buf.data_ptr()), 0, buf.numel())
    held = marker.query() is True
    with torch.cuda.stream(side):
        snap = buf.clone()
    side.synchronize()
    torch.cuda.synchronize()
    assert rc == 0 and pending, su.INCONCLUSIVE
    assert not bool(buf.any())                                 # ... and it is zero in the end
    return not bool(snap.any()), held


def test_slot_setup_is_complete_when_ron_clone_returns(dev, side, ron_single):
    """ron_clone zeroes the new slot's activations (halos stay zero forever) and post-processing workspace through the null stream
    and returns; the slot is then used at once on a non-blocking stream, which does not wait for the null stream.  With the default
    (null) stream stalled, the zeroing is queued behind the stall: ron_clone may only return once the stall is over.  That is
    asserted BEFORE the slot is used (a slot that ran on unset memory could do anything), then two detect calls on the clone on an
    independent stream, with no synchronise in between, must both equal the owner's result."""
    net, x, _ = ron_single
    complete, held = _raw_hipmemset_behind_a_busy_null_stream(dev, side)
    print('hipMemset behind a busy null stream: memory zero on return %s, host held until the stall ended %s' % (complete, held))
    ref = _clones(_det(net.detect(x)))
    torch.cuda.synchronize()
    marker = su.stall(torch.cuda.default_stream(dev))
    pending = marker.query() is False
    slot = net.clone()
    over = marker.query() is True
    if not (pending and over):
        torch.cuda.synchronize()                               # only on the failing path: the slot is not touched then
    assert pending, su.INCONCLUSIVE
    assert over, ('ron_clone returned while the null stream, and with it the zeroing of the slot, was still held back: a slot used at '
                  'once on a non-blocking stream runs on non-zero halos and has its counters wiped afterwards')
    # at once, with no synchronise; the default stream busy again, so that nothing else of the set-up can hide behind it
    marker = su.stall(torch.cuda.default_stream(dev))
    with torch.cuda.stream(side):
        first = _clones(_det(slot.detect(x)))
        second = _clones(_det(slot.detect(x)))
    side.synchronize()
    pending = marker.query() is False
    torch.cuda.synchronize()
    assert pending, su.INCONCLUSIVE
    assert su.same_bytes(first, ref), 'first detect of a fresh slot differs from the owner'
    assert su.same_bytes(second, ref), 'second detect of a fresh slot differs from the owner'
    assert int(ref[-1].sum()) > 0
    slot.close()
    net._slots.remove(slot)


# --------------------------------------------------------------------------------------------------------------- per-stream scratch
def _two_stream_cases(dev, adev):
    post_np, a, b = _entry_post_np_want_sorted(dev, adev)
    post_eval, c, d = _entry_post_eval(False)(dev, adev)
    return {'post_np': (post_np, a, b), 'ron_post_eval': (post_eval, c, d),
            'ssd_losses_grad': (_ssd_grad_entry(dev, 'batch'), _ssd_inputs('batch', 17), _ssd_inputs('batch', 18))}


@pytest.mark.parametrize('name', ['post_np', 'ron_post_eval', 'ssd_losses_grad'])
def test_two_streams_at_once(dev, side, side2, adev, name):
    """The same entry on two independent streams with different inputs, both stalled, the stream issued first stalled longer: the
    completion order is the reverse of the issue order, and each result is its own (ops._workspace keeps one scratch buffer per
    stream; ssd_losses_grad also writes into the caller's gradient buffers)."""
    entry, xa, xb = _two_stream_cases(dev, adev)[name]
    xa, xb = _up(xa, dev), _up(xb, dev)
    want_a, want_b = _clones(entry(xa)), _clones(entry(xb))
    buf_a, buf_b = _clones(xb), _clones(xa)                   # each stream's buffers hold the other stream's case until the fill
    for s, buf in ((side, buf_a), (side2, buf_b)):            # once per stream outside the timed window (allocator pools, scratch)
        with torch.cuda.stream(s):
            _clones(entry(buf))
    torch.cuda.synchronize()
    assert not su.same_bytes(want_a, want_b)
    got, markers = [], []
    with su.quiet_host():
        for s, buf, x, ms in ((side, buf_a, xa, 500.0), (side2, buf_b, xb, 200.0)):
            with torch.cuda.stream(s):
                markers.append(su.stall(s, ms))
                for bb, t in zip(buf, x):
                    bb.copy_(t, non_blocking=True)
                got.append(_clones(entry(buf)))
        pending = [m.query() is False for m in markers]       # both calls were enqueued while both streams were held
    side2.synchronize()
    reversed_order = markers[0].query() is False
    side.synchronize()
    assert all(pending), su.INCONCLUSIVE
    assert reversed_order, 'the stream issued second did not finish first'
    assert su.same_bytes(got[0], want_a) and su.same_bytes(got[1], want_b)


def test_workspace_eviction_with_work_queued(dev, side, side2, adev):
    """ops._workspace keeps _MAX_WORKSPACES buffers, least recently used first out.  post_np on _MAX_WORKSPACES + 2 streams, all
    stalled, evicts the buffers of the first two while their work is still queued; then a larger call on the first stream regrows its
    buffer.  Every result equals its default-stream value.  (Streams that share a hardware queue are fine here: the stalls are finite
    and nothing waits across streams.)"""
    from ron_tensorflow_amd import ops
    n_streams = ops._MAX_WORKSPACES + 2
    assert n_streams <= 12                                    # with the default stream and a context's lanes: at most 16 per process
    streams = [side, side2]
    for _ in range(64):                                       # torch hands out pooled streams: take them until the handles are distinct
        s = torch.cuda.Stream(device=dev)
        if len(streams) < n_streams and s.cuda_stream not in [t.cuda_stream for t in streams] + [0]:
            streams.append(s)
    assert len({s.cuda_stream for s in streams}) == n_streams, 'fewer than %d distinct streams' % n_streams
    entry = lambda t: _post_np_out(ops.post_np(*_split(t, 4, 4, 4), adev))
    cases = [_up(sum(_heads(400 + i, 1), []), dev) for i in range(n_streams)]
    larger = _up(sum(_heads(399, 2), []), dev)
    want = [_clones(entry(c)) for c in cases]
    want_larger = _clones(entry(larger))
    for s, c in zip(streams, cases):                          # once per stream outside the timed window (allocator pools)
        with torch.cuda.stream(s):
            _clones(entry(c))
    torch.cuda.synchronize()
    assert all(not su.same_bytes(want[0], w) for w in want[1:])
    ops._WORKSPACES.clear()
    got, markers = [], []
    with su.quiet_host():
        for s, c in zip(streams, cases):
            with torch.cuda.stream(s):
                markers.append(su.stall(s))
                got.append(_clones(entry(c)))
        keys = [k[2] for k in ops._WORKSPACES]
        with torch.cuda.stream(streams[0]):
            got_larger = _clones(entry(larger))
        pending = [m.query() is False for m in markers]
    torch.cuda.synchronize()
    assert all(pending), su.INCONCLUSIVE
    assert len(keys) == ops._MAX_WORKSPACES and streams[0].cuda_stream not in keys and streams[1].cuda_stream not in keys
    for i in range(n_streams):
        assert su.same_bytes(got[i], want[i]), 'stream %d' % i
    assert su.same_bytes(got_larger, want_larger)
    ops._WORKSPACES.clear()
    del streams
