"""GPU: RONNet.bboxes_encode / ron_bboxes_encode against the numpy float32 reference (tests/encode_ref.py).

Bit-exact (np.array_equal): gclasses, gscores, gbboxes and the cx / cy targets - every operation behind them is one correctly
rounded float32 operation.  The w / h targets go through logf: they are held to the per-element bound of DESIGN.md section 4 around
the float64 value of the same formula (encode_ref.loc_reference64), and so is the numpy reference itself."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_cases as ec  # noqa: E402
import encode_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ec.encode_cases()


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _net(dev, img_shape, borders):
    from ron_tensorflow_amd.nets.ron_vgg_320 import RONNet
    return RONNet(RONNet.default_params._replace(img_shape=tuple(img_shape), allowed_borders=list(borders)), dtype='fp32',
                  max_batch=1, device=dev)


def _check(got, glabels, gbboxes, tab, low=0.3, high=0.5):
    """got: four per-layer lists of numpy arrays [N, H, W, A, ...]."""
    n = glabels.shape[0]
    per = [er.encode_np(glabels[i], gbboxes[i], tab, high, low) for i in range(n)]           # the reference, once per image
    ref = tuple(tab.split(np.stack([p[k] for p in per]), n) for k in range(4))
    for l in range(len(tab.shapes)):
        assert got[0][l].dtype == np.int64 and got[0][l].shape == (n,) + tab.shapes[l]
        assert np.array_equal(got[0][l], ref[0][l]), 'gclasses, layer %d' % l
        assert np.array_equal(got[2][l], ref[2][l]), 'gscores, layer %d' % l
        assert np.array_equal(got[3][l], ref[3][l]), 'gbboxes, layer %d' % l
        assert np.array_equal(got[1][l][..., :2], ref[1][l][..., :2], equal_nan=True), 'cx / cy, layer %d' % l
        assert np.array_equal(np.isnan(got[1][l]), np.isnan(ref[1][l])), 'NaN positions, layer %d' % l
    # w / h: float64 value of the same formula, per-element bound; the numpy reference lies inside it too
    flat = lambda per_layer, i: np.concatenate([t[i].reshape(-1, 4) for t in per_layer])
    for i in range(n):
        if er.present_rows(glabels[i]) == 0:
            assert not flat(got[1], i).any()
            continue
        m = per[i][4]
        w64, h64, bw, bh = er.loc_reference64(gbboxes[i], tab, m)
        g, r = flat(got[1], i), flat(ref[1], i)
        for col, v64, bound in ((2, w64, bw), (3, h64, bh)):
            ok = np.isfinite(v64)
            assert (np.abs(g[ok, col] - v64[ok]) <= bound[ok]).all(), ('kernel outside the bound', i, col)
            assert (np.abs(r[ok, col] - v64[ok]) <= bound[ok]).all(), ('numpy reference outside the bound', i, col)
            assert np.array_equal(g[~ok, col], r[~ok, col], equal_nan=True)        # 0, -inf (zero-sized box) or NaN: exact


def _to_np(out):
    return tuple([t.cpu().numpy() for t in lst] for lst in out)


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_cases_through_ronnet(dev, case):
    import torch
    net = _net(dev, case.img_shape, case.borders)
    tab = ec.table(case)
    out = net.bboxes_encode(torch.from_numpy(case.glabels).to(dev), torch.from_numpy(case.gbboxes).to(dev), case.anchors,
                            positive_threshold=case.high, ignore_threshold=case.low)
    _check(_to_np(out), case.glabels, case.gbboxes, tab, case.low, case.high)


def test_single_image_form_has_no_batch_axis(dev):
    case = CASES[0]
    net = _net(dev, case.img_shape, case.borders)
    out = net.bboxes_encode(case.glabels[0].astype(np.int64), case.gbboxes[0], case.anchors)      # numpy, int64 labels, as the reference takes them
    tab = ec.table(case)
    assert all(tuple(t.shape) == s for t, s in zip(out[0], tab.shapes))
    assert all(tuple(t.shape) == s + (4,) for t, s in zip(out[1], tab.shapes))
    got = tuple([t.cpu().numpy()[None] for t in lst] for lst in out)
    _check(got, case.glabels, case.gbboxes, tab)


@pytest.fixture(scope='module')
def ron_table():
    return er.AnchorTable(ec.ron320_anchors(), ec.RON_BORDERS, (320, 320))


@pytest.mark.parametrize('n,g', [(1, 1), (3, 1), (1, 7), (3, 7), (1, er.RON_MAX_GT), (3, er.RON_MAX_GT)])
def test_ron320_anchors(dev, ron_table, n, g):
    """21 250 anchors: no multiple of the workgroup size, so the last workgroup of every image is ragged."""
    import torch
    gl, gb = ec.random_ground_truth(40 + n + g, n, g, counts=[g] + [max(1, g // 2)] * (n - 1))
    net = _net(dev, (320, 320), ec.RON_BORDERS)
    out = net.bboxes_encode(torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev), net.anchors((320, 320)))
    _check(_to_np(out), gl, gb, ron_table)


def _c_call(dev, tab, anchors, gl, gb, borders, img_shape, num_layers=None, g=None, null_layer=None):
    """ron_bboxes_encode through ctypes; returns (status, outputs as numpy)."""
    import torch
    from ron_tensorflow_amd import _lib, ops
    lib = _lib.lib()
    n = gl.shape[0]
    adev = ops.anchors_to_device(anchors, dev)
    hd = ops._anchor_heads(adev, tab.shapes)
    if num_layers is not None:
        hd.num_layers = num_layers
    tg = _lib.Targets()
    outs = ([], [], [], [])
    for l, shp in enumerate(tab.shapes):
        for k, (extra, dt) in enumerate((((), torch.int64), ((4,), torch.float32), ((), torch.float32), ((4,), torch.float32))):
            outs[k].append(torch.zeros((n,) + shp + extra, dtype=dt, device=dev))
        tg.gclasses[l], tg.glocalisations[l] = outs[0][l].data_ptr(), outs[1][l].data_ptr()
        tg.gscores[l], tg.gbboxes[l] = outs[2][l].data_ptr(), outs[3][l].data_ptr()
    if null_layer is not None:
        tg.gscores[null_layer] = None
    g = gl.shape[1] if g is None else g
    nbytes = max(8, n * gl.shape[1] * 8)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    d_gl, d_gb = torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev)
    borders_c = (C.c_int32 * len(borders))(*borders)
    ps = (C.c_float * 4)(0.1, 0.1, 0.2, 0.2)
    rc = lib.ron_bboxes_encode(C.byref(hd), n, _lib.ptr(d_gl), _lib.ptr(d_gb), g, img_shape[0], img_shape[1], borders_c, 0.5, 0.3, ps,
                               _lib.ptr(ws), nbytes, C.byref(tg), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, _to_np(outs)


def test_c_entry_batch_with_an_empty_image_between_two(dev, ron_table):
    from ron_tensorflow_amd import _lib
    gl, gb = ec.random_ground_truth(77, 3, 7, counts=[5, 0, 7])
    assert _lib.lib().ron_bboxes_encode_workspace_bytes(3, 7) == 3 * 7 * 8
    rc, got = _c_call(dev, ron_table, ec.ron320_anchors(), gl, gb, ec.RON_BORDERS, (320, 320))
    assert rc == 0
    _check(got, gl, gb, ron_table)
    for l in range(4):
        assert not got[0][l][1].any() and not got[1][l][1].any() and not got[2][l][1].any()


def test_c_entry_argument_errors(dev, ron_table):
    from ron_tensorflow_amd import _lib
    lib = _lib.lib()
    gl, gb = ec.random_ground_truth(78, 1, 4)
    anchors = ec.ron320_anchors()
    for kw, text in ((dict(g=0), b'not in [1, 256]'), (dict(g=er.RON_MAX_GT + 1), b'not in [1, 256]'),
                     (dict(null_layer=2), b'null target pointer of layer 2'), (dict(num_layers=_lib.RON_MAX_LAYERS + 1), b'layers not in')):
        rc, _ = _c_call(dev, ron_table, anchors, gl, gb, ec.RON_BORDERS, (320, 320), **kw)
        assert rc == -1, kw
        assert text in lib.ron_last_error(), (kw, lib.ron_last_error())
    assert lib.ron_bboxes_encode_workspace_bytes(1, 0) == -1
