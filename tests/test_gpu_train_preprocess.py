"""GPU: ron_train_geometry / ron_preprocess_train / ron_preprocess_for_train against the CPU references of tests/train_pre_ref.py.

Every comparison is np.array_equal: the geometry is integer decisions on correctly rounded float32 operations, the pixels are the
same float32 operations in the same order as the reference that materialises the canvas, and the fill is one correctly rounded
quotient of exact integer sums."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_pre_cases as tc  # noqa: E402
import train_pre_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu

GEOM_CASES = tc.geometry_cases()
PIXEL_CASES = tc.pixel_cases()
PIXEL_BATCHES = tc.pixel_batches()


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _geometry(dev, hw, gl, gb, draws, g=None, n=None, null=None):
    """ron_train_geometry through ctypes: (status, geom, labels, boxes, counts) as numpy."""
    import torch
    from ron_tensorflow_amd import _lib
    hw, gl, gb, draws = np.asarray(hw, np.int32), np.asarray(gl, np.int32), np.asarray(gb, np.float32), np.asarray(draws, np.float32)
    N, G = gl.shape
    t = dict(hw=torch.from_numpy(hw).to(dev), gl=torch.from_numpy(gl).to(dev), gb=torch.from_numpy(gb).to(dev),
             draws=torch.from_numpy(draws).to(dev),
             geom=torch.full((N, tr.RON_TRAIN_GEOM), -7, dtype=torch.int32, device=dev),
             gl_out=torch.full((N, G), -7, dtype=torch.int32, device=dev),
             gb_out=torch.full((N, G, 4), -7.0, dtype=torch.float32, device=dev),
             counts=torch.full((N,), -7, dtype=torch.int32, device=dev))
    p = {k: (None if k == null else _lib.ptr(v)) for k, v in t.items()}
    rc = _lib.lib().ron_train_geometry(p['hw'], p['gl'], p['gb'], N if n is None else n, G if g is None else g, p['draws'], p['geom'],
                                       p['gl_out'], p['gb_out'], p['counts'], _lib.current_stream())
    torch.cuda.synchronize()
    return rc, t['geom'].cpu().numpy(), t['gl_out'].cpu().numpy(), t['gb_out'].cpu().numpy(), t['counts'].cpu().numpy()


def _pixels(dev, images, geom, out_shape, means=tr.MEANS):
    """ron_preprocess_train through ctypes on a hand-made geometry table."""
    import torch
    from ron_tensorflow_amd import _lib
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp
    lib = _lib.lib()
    n = len(images)
    packed, d_off, d_hw = pp._pack([np.ascontiguousarray(im) for im in images], dev)
    d_geom = torch.from_numpy(np.ascontiguousarray(geom, np.int32)).to(dev)
    nbytes = lib.ron_preprocess_train_workspace_bytes(n)
    assert nbytes >= n * 3 * 8
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)          # the call zeroes its workspace itself
    out = torch.full((n, out_shape[0], out_shape[1], 3), float('nan'), dtype=torch.float32, device=dev)
    m = (C.c_float * 3)(*means)
    _lib.check(lib.ron_preprocess_train(_lib.ptr(packed), _lib.ptr(d_off), _lib.ptr(d_hw), _lib.ptr(d_geom), n, out_shape[0],
                                        out_shape[1], m, _lib.ptr(ws), _lib.ptr(out), _lib.current_stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize('case', GEOM_CASES, ids=[c.name for c in GEOM_CASES])
def test_geometry_cases(dev, case):
    rc, geom, gl, gb, counts = _geometry(dev, [[case.h, case.w]], case.glabels[None], case.gbboxes[None], case.draws[None])
    assert rc == 0
    g, l, b, k = tr.geometry_scalar(case.h, case.w, case.glabels, case.gbboxes, case.draws)
    assert np.array_equal(geom[0, :10], g), (geom[0], g)
    assert np.array_equal(gl[0], l) and np.array_equal(gb[0], b) and counts[0] == k
    full = tc.reference(case)
    assert np.array_equal(geom[0], full['geom'])                      # the diagnostic columns too: min_iou index, overlap rounds


@pytest.fixture(scope='module')
def random_inputs():
    """256 seeded images, 7 x 9 to 64 x 48, G = 1, 3 and 64 with 0 .. G present rows, and the scalar reference of each (once)."""
    items = tc.random_images(77, 256)
    by_g = {}
    for it in items:
        by_g.setdefault(it[2], []).append(it)
    out = {}
    for g, lst in by_g.items():
        hw = np.array([[h, w] for (h, w, _, _, _, _) in lst], np.int32)
        gl, gb, d = np.stack([i[3] for i in lst]), np.stack([i[4] for i in lst]), np.stack([i[5] for i in lst])
        gl[0] = 0                                                       # both ends of 0 .. G are there whatever the seed drew
        gl[1] = np.maximum(gl[1], 1)
        gb[1] = np.where(gb[1].any(axis=1, keepdims=True), gb[1], np.array([0.2, 0.3, 0.7, 0.6], np.float32))
        out[g] = (hw, gl, gb, d, tr.geometry_batch(hw, gl, gb, d))
    return out


@pytest.mark.parametrize('g', [1, 3, 64])
def test_geometry_random_images(dev, random_inputs, g):
    hw, gl, gb, d, ref = random_inputs[g]
    assert sum(len(v[0]) for v in random_inputs.values()) == 256
    present = np.array([tr.present_rows(r) for r in gl])
    assert present.min() == 0 and present.max() == g
    rc, geom, l, b, counts = _geometry(dev, hw, gl, gb, d)
    assert rc == 0
    assert np.array_equal(geom[:, :10], ref[0])
    assert np.array_equal(l, ref[1]) and np.array_equal(b, ref[2]) and np.array_equal(counts, ref[3])


def test_geometry_max_gt_rows(dev):
    """G = RON_MAX_GT: every lane holds four boxes, present rows end inside a lane's second slab."""
    (h, w, g, gl, gb, d), = tc.random_images(5, 1, g_choices=(tr.RON_MAX_GT,))
    gl[:150] = np.maximum(gl[:150], 1)
    gb[:150] = np.where(gb[:150].any(axis=1, keepdims=True), gb[:150], np.array([0.2, 0.2, 0.6, 0.7], np.float32))
    gl[150:] = 0
    rc, geom, l, b, counts = _geometry(dev, [[h, w]], gl[None], gb[None], d[None])
    ref = tr.geometry_scalar(h, w, gl, gb, d)
    assert rc == 0 and np.array_equal(geom[0, :10], ref[0]) and np.array_equal(l[0], ref[1]) and np.array_equal(b[0], ref[2])
    assert counts[0] == ref[3]


def test_geometry_argument_errors(dev):
    from ron_tensorflow_amd import _lib
    lib = _lib.lib()
    c = GEOM_CASES[0]
    args = ([[c.h, c.w]], c.glabels[None], c.gbboxes[None], c.draws[None])
    for kw, text in ((dict(g=0), b'not in [1, 256]'), (dict(g=tr.RON_MAX_GT + 1), b'not in [1, 256]'), (dict(n=0), b'batch 0'),
                     (dict(null='draws'), b'null input'), (dict(null='counts'), b'null output')):
        rc = _geometry(dev, *args, **kw)[0]
        assert rc == -1, kw
        assert text in lib.ron_last_error(), (kw, lib.ron_last_error())
    assert lib.ron_preprocess_train_workspace_bytes(0) == -1
    assert b'batch 0' in lib.ron_last_error()
    assert lib.ron_preprocess_train(None, None, None, None, 1, 16, 16, None, None, None, None) == -1
    assert b'null input' in lib.ron_last_error()


# ------------------------------------------------------------------------------------------------------------ pixels
@pytest.mark.parametrize('case', PIXEL_CASES, ids=[c.name for c in PIXEL_CASES])
def test_pixel_cases(dev, case):
    got = _pixels(dev, case.images, case.geom, case.out_shape)
    assert np.array_equal(got[0], tr.pixels_ref(case.images[0], case.geom[0], case.out_shape))


@pytest.mark.parametrize('batch', PIXEL_BATCHES, ids=['%s_%dx%d' % (b[0], b[3][0], b[3][1]) for b in PIXEL_BATCHES])
def test_pixel_batches(dev, batch):
    name, imgs, geoms, out_shape = batch
    got = _pixels(dev, imgs, geoms, out_shape)
    assert got.shape == (3,) + tuple(out_shape) + (3,) and np.isfinite(got).all()
    for i in range(3):
        assert np.array_equal(got[i], tr.pixels_ref(imgs[i], geoms[i], out_shape)), (name, i)


# ------------------------------------------------------------------------------------------------------------ Python layer
def _batch_inputs(seed=9, n=5, g=3):
    items = tc.random_images(seed, n, g_choices=(g,), lo=(9, 11), hi=(40, 36))
    imgs = [tc.random_image(seed * 100 + i, it[0], it[1]) for i, it in enumerate(items)]
    return imgs, np.stack([it[3] for it in items]), np.stack([it[4] for it in items]), np.stack([it[5] for it in items])


def _reference_batch(imgs, gl, gb, draws, out_shape):
    hw = [im.shape[:2] for im in imgs]
    geom, l, b, k = tr.geometry_batch(hw, gl, gb, draws)
    return np.stack([tr.pixels_ref(im, g, out_shape) for im, g in zip(imgs, geom)]), l, b, k, geom


def test_batch_with_given_draws_equals_the_references(dev):
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp
    imgs, gl, gb, draws = _batch_inputs()
    out = pp.ron_preprocess_for_train_batch(imgs, gl, gb, out_shape=(20, 12), draws=draws, device=dev)
    got = [t.cpu().numpy() for t in out]
    ref = _reference_batch(imgs, gl, gb, draws, (20, 12))
    assert ref[4][:, 0].any() and not ref[4][:, 0].all()               # expanded and plain images in one batch
    assert got[1].dtype == np.int32 and got[3].dtype == np.int32 and got[4].shape == (5, tr.RON_TRAIN_GEOM)
    assert np.array_equal(got[4][:, :10], ref[4]) and np.array_equal(got[3], ref[3])
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[0], ref[0])


def test_generator_draws_are_reproducible_and_differ_between_seeds(dev):
    import torch
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp
    imgs, gl, gb, _ = _batch_inputs(seed=10)

    def run(seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        return [t.cpu().numpy() for t in pp.ron_preprocess_for_train_batch(imgs, gl, gb, (16, 16), generator=gen, device=dev)]
    a, b, c = run(1), run(1), run(2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[4], c[4]) and not np.array_equal(a[0], c[0])
    # ... and they are the draws torch.rand makes from that generator
    draws = torch.rand((len(imgs), tr.RON_TRAIN_DRAWS), dtype=torch.float32, device=dev,
                       generator=torch.Generator(device=dev).manual_seed(1)).cpu().numpy()
    ref = _reference_batch(imgs, gl, gb, draws, (16, 16))
    assert np.array_equal(a[4][:, :10], ref[4]) and np.array_equal(a[0], ref[0]) and np.array_equal(a[2], ref[2])


def test_single_image_signature_returns_trimmed_rows(dev):
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp
    case = next(c for c in GEOM_CASES if c.name.startswith('j_'))
    img = tc.random_image(4, case.h, case.w)
    labels, boxes = case.glabels[:1].astype(np.int64), case.gbboxes[:1]          # ragged rows, int64 labels, as the reference takes them
    image, l, b = pp.ron_preprocess_for_train(img, labels, boxes, (16, 16), draws=case.draws, device=dev)
    g, rl, rb, k = tr.geometry_scalar(case.h, case.w, labels, boxes, case.draws)
    assert k == 1 and tuple(l.shape) == (1,) and tuple(b.shape) == (1, 4) and tuple(image.shape) == (16, 16, 3)
    assert np.array_equal(l.cpu().numpy(), rl[:k]) and np.array_equal(b.cpu().numpy(), rb[:k])
    assert np.array_equal(image.cpu().numpy(), tr.pixels_ref(img, g, (16, 16)))
    chw = pp.ron_preprocess_for_train(img, labels, boxes, (16, 16), data_format='NCHW', draws=case.draws, device=dev)[0]
    assert np.array_equal(chw.cpu().numpy(), image.permute(2, 0, 1).cpu().numpy())
    # an image whose boxes are all dropped ... cannot happen (the whole image comes back); one without boxes gives empty rows
    image, l, b = pp.ron_preprocess_for_train(img, np.zeros(0, np.int64), np.zeros((0, 4), np.float32), (16, 16), draws=case.draws,
                                              device=dev)
    assert tuple(l.shape) == (0,) and tuple(b.shape) == (0, 4)


def test_preprocess_image_dispatches_both_ways(dev):
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp
    case = next(c for c in GEOM_CASES if c.name.startswith('i_'))
    img = tc.random_image(6, case.h, case.w)
    labels, boxes = case.glabels, case.gbboxes
    train = pp.preprocess_image(img, labels, boxes, (16, 16), 'NHWC', is_training=True, draws=case.draws, device=dev)
    want = pp.ron_preprocess_for_train(img, labels, boxes, (16, 16), draws=case.draws, device=dev)
    assert len(train) == 3 and all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(train, want))
    ev = pp.preprocess_image(img, labels, boxes, (16, 16), 'NHWC', is_training=False, device=dev)
    want = pp.preprocess_for_eval(img, labels, boxes, (16, 16), device=dev)
    assert len(ev) == 4 and np.array_equal(ev[0].cpu().numpy(), want[0].cpu().numpy())
    assert np.array_equal(ev[2], want[2]) and np.array_equal(ev[3], want[3])
    assert not np.array_equal(train[0].cpu().numpy(), ev[0].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ into bboxes_encode
def test_batch_outputs_go_unchanged_into_bboxes_encode(dev):
    """320 x 320 training batch -> ops.bboxes_encode on RON-320's anchors == tests/encode_ref.py on the CPU reference's boxes, under
    the comparison rule of tests/test_gpu_encode.py (exact classes, scores, corners and centres; w / h inside their bound)."""
    import encode_cases as ec
    import encode_ref as er
    from test_gpu_encode import _check, _to_np
    from ron_tensorflow_amd import ops
    from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp
    imgs, gl, gb, draws = _batch_inputs(seed=12, n=4, g=8)
    out, d_gl, d_gb, counts, geom = pp.ron_preprocess_for_train_batch(imgs, gl, gb, (320, 320), draws=draws, device=dev)
    assert tuple(out.shape) == (4, 320, 320, 3)
    ref = tr.geometry_batch([im.shape[:2] for im in imgs], gl, gb, draws)
    assert ref[3].max() > 0
    anchors = ec.ron320_anchors()
    tab = er.AnchorTable(anchors, ec.RON_BORDERS, (320, 320))
    got = ops.bboxes_encode(d_gl, d_gb, ops.anchors_to_device(anchors, dev), tab.shapes, (320, 320), ec.RON_BORDERS)
    _check(_to_np(got), ref[1], ref[2], tab)
