"""GPU: the select front end is ONE function of its inputs whichever form they come in.  Class logits or their softmax
(ops.softmax_last), objectness logit pairs or P(object): the four combinations give the same bytes out of ron_post_tfe,
ron_post_eval and ron_post_np.  The heads are small and awkward on purpose: a first layer of 300 anchors (one full 256-thread
block and a block of 44 lanes: a wave with masked lanes), a second of 18 (the layer lookup has to move), anchors whose background
logit dominates (the early exit of the logit path, which the probability path does not have) and objectness around the gate."""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

SHAPES = [(10, 10, 3), (3, 3, 2)]       # (H, W, A): 300 + 18 anchors
BATCH = 2
OBJ_THR, SEL_THR = 0.03, 0.01
FORMS = list(itertools.product((False, True), (False, True)))      # (cls_is_prob, obj_is_prob)


def _anchors(dev):
    from ron_tensorflow_amd import ops
    sizes = [(np.float32([0.30, 0.40, 0.25]), np.float32([0.30, 0.25, 0.40])), (np.float32([0.6, 0.8]), np.float32([0.6, 0.5]))]
    out = []
    for (fh, fw, _), (h, w) in zip(SHAPES, sizes):
        y, x = np.mgrid[0:fh, 0:fw]
        out.append((((y + 0.5) / fh).astype(np.float32), ((x + 0.5) / fw).astype(np.float32), h, w))
    return ops.anchors_to_device(out, dev)


@pytest.fixture(scope='module', params=[21, 3], ids=['C21', 'C3'])
def heads(request):
    """Both forms of every head tensor, made once per class count."""
    from ron_tensorflow_amd import ops
    assert torch.cuda.is_available()
    dev = torch.device('cuda:0')
    nc = request.param
    rs = np.random.RandomState(7 + nc)
    adev = _anchors(dev)
    cls, obj, loc = [], [], []
    for fh, fw, a in SHAPES:
        z = (rs.randn(BATCH, fh, fw, a, nc) * 2).astype(np.float32)
        # per image: about half of the anchors are background-dominated by far more than -log(0.01) - the logit path leaves them early
        z[..., 0] += np.where(rs.rand(BATCH, fh, fw, a) < 0.5, 12.0, 0.0).astype(np.float32)
        cls.append(z)
        # P(object) = sigmoid(t): 0.03 is t = -3.48, so the gate cuts through the middle of these
        t = (rs.randn(BATCH, fh, fw, a) * 1.5 - 3.5).astype(np.float32)
        obj.append(np.stack([np.zeros_like(t), t], axis=-1))
        loc.append((rs.randn(BATCH, fh, fw, a, 4) * 0.2).astype(np.float32))
    to_dev = lambda lst: [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in lst]  # noqa: E731
    cls_d, obj_d, loc_d = to_dev(cls), to_dev(obj), to_dev(loc)
    h = dict(nc=nc, cls={False: cls_d, True: [ops.softmax_last(c) for c in cls_d]},
             obj={False: obj_d, True: [ops.softmax_last(o, pick=1) for o in obj_d]},
             dec=[ops.bboxes_decode_layer(l, an) for l, an in zip(loc_d, adev)])
    # the inputs do what the docstring says, per image
    for i in range(BATCH):
        z = np.concatenate([c[i].reshape(-1, nc) for c in cls])
        p = np.concatenate([c[i].reshape(-1, nc) for c in (t.cpu().numpy() for t in h['cls'][True])])
        o = np.concatenate([t[i].cpu().numpy().reshape(-1) for t in h['obj'][True]])
        skipped = z[:, 1:].max(-1) - z.max(-1) < np.log(SEL_THR) - 1e-2
        assert skipped.any() and (p[:, 1:] > SEL_THR).any(), 'image %d: early exits and passing classes' % i
        assert (o > OBJ_THR).any() and (o <= OBJ_THR).any(), 'image %d: objectness on both sides of the gate' % i
    return h


def _bytes(tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in tensors]


def _same_for_all_forms(run):
    """run(cls_is_prob, obj_is_prob) -> list of tensors; every form's bytes equal the logit form's.  Returns the logit form's tensors."""
    first = run(False, False)
    ref = _bytes(first)
    for cp, op in FORMS[1:]:
        got = _bytes(run(cp, op))
        for k, (g, r) in enumerate(zip(got, ref)):
            assert g == r, 'output %d differs with cls_is_prob=%s obj_is_prob=%s' % (k, cp, op)
    return first


def test_post_tfe_same_for_every_input_form(heads):
    from ron_tensorflow_amd import tfe

    def run(cp, op):
        return list(tfe.post_tfe(heads['cls'][cp], heads['obj'][op], heads['dec'], None, num_classes=heads['nc'], objectness_thres=OBJ_THR,
                                 select_threshold=SEL_THR, nms_threshold=0.4, clipping_bbox=[0., 0., 1., 1.], top_k=200, keep_top_k=100,
                                 cls_is_prob=cp, obj_is_prob=op, loc_decoded=True))
    scores, _ = _same_for_all_forms(run)
    assert int((scores > 0).sum()) > 0


@pytest.mark.parametrize('nms_by_class', [False, 'scores'], ids=['nms_mode0', 'nms_mode4'])
def test_post_eval_same_for_every_input_form(heads, nms_by_class):
    from ron_tensorflow_amd import ron_eval

    def run(cp, op):
        out = ron_eval.post_eval(heads['cls'][cp], heads['obj'][op], heads['dec'], None, [(320, 320)] * BATCH, num_classes=heads['nc'],
                                 objectness_thres=OBJ_THR, select_threshold=SEL_THR, nms_threshold=0.4, keep_top_k=20, nms_mode='min',
                                 cls_is_prob=cp, obj_is_prob=op, loc_decoded=True, nms_by_class=nms_by_class)
        return [getattr(out, f) for f in out.FIELDS]
    first = _same_for_all_forms(run)
    assert int(first[-1].sum()) > 0


@pytest.mark.parametrize('select_threshold', [SEL_THR, 0.0], ids=['thr0.01', 'argmax'])
def test_post_np_same_for_every_input_form(heads, select_threshold):
    from ron_tensorflow_amd import ops

    def run(cp, op):
        out, srt, n_cand = ops.post_np(heads['cls'][cp], heads['obj'][op], heads['dec'], None, num_classes=heads['nc'],
                                       objectness_thres=OBJ_THR, select_threshold=select_threshold, nms_threshold=0.45, top_k=400,
                                       cls_is_prob=cp, obj_is_prob=op, loc_decoded=True, want_sorted=True)
        return [getattr(out, f) for f in out.FIELDS] + [getattr(srt, f) for f in srt.FIELDS] + [n_cand]
    first = _same_for_all_forms(run)
    assert int(first[4].sum()) > 0 and int(first[-1].sum()) > 0
