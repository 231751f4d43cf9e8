"""GPU: SSDNet.bboxes_encode of SSD-300 and SSD-512 against the numpy float32 reference (tests/encode_ref.py) called with the
thresholds 0.5 / 0.5 (no ignore band) and a border of 1 << 24 (no anchor is ever outside).

Exactness as in test_gpu_encode.py: gclasses, gscores, gbboxes and the cx / cy targets are bit-exact; the w / h targets go through
logf and are held to the per-element bound around the float64 value of the same formula."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encode_cases as ec  # noqa: E402
import encode_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu
NO_BORDER = 1 << 24


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _net(dev, name):
    from ron_tensorflow_amd.nets import ssd_vgg_300, ssd_vgg_512
    mod = {'ssd300': ssd_vgg_300, 'ssd512': ssd_vgg_512}[name]
    return mod.SSDNet(dtype='fp32', max_batch=1, device=dev)


def _check(got, glabels, gbboxes, tab):
    n = glabels.shape[0]
    per = [er.encode_np(glabels[i], gbboxes[i], tab, 0.5, 0.5) for i in range(n)]
    ref = tuple(tab.split(np.stack([p[k] for p in per]), n) for k in range(4))
    for l in range(len(tab.shapes)):
        assert got[0][l].dtype == np.int64 and got[0][l].shape == (n,) + tab.shapes[l]
        assert np.array_equal(got[0][l], ref[0][l]), 'gclasses, layer %d' % l
        assert np.array_equal(got[2][l], ref[2][l]), 'gscores, layer %d' % l
        assert np.array_equal(got[3][l], ref[3][l]), 'gbboxes, layer %d' % l
        assert np.array_equal(got[1][l][..., :2], ref[1][l][..., :2], equal_nan=True), 'cx / cy, layer %d' % l
        assert np.array_equal(np.isnan(got[1][l]), np.isnan(ref[1][l])), 'NaN positions, layer %d' % l
        assert not (got[0][l] < 0).any()                                      # 0.5 / 0.5: no ignore band, no ignored anchor
    flat = lambda per_layer, i: np.concatenate([t[i].reshape(-1, 4) for t in per_layer])
    for i in range(n):
        if er.present_rows(glabels[i]) == 0:
            assert not flat(got[1], i).any()
            continue
        w64, h64, bw, bh = er.loc_reference64(gbboxes[i], tab, per[i][4])
        g, r = flat(got[1], i), flat(ref[1], i)
        for col, v64, bound in ((2, w64, bw), (3, h64, bh)):
            ok = np.isfinite(v64)
            assert (np.abs(g[ok, col] - v64[ok]) <= bound[ok]).all(), ('kernel outside the bound', i, col)
            assert np.array_equal(g[~ok, col], r[~ok, col], equal_nan=True)


def _to_np(out):
    return tuple([t.cpu().numpy() for t in lst] for lst in out)


@pytest.mark.parametrize('name,size,total', [('ssd300', 300, 8732), ('ssd512', 512, 24564)])
def test_ssd_anchors_batched_and_single(dev, name, size, total):
    import torch
    net = _net(dev, name)
    anchors = net.anchors((size, size))
    tab = er.AnchorTable(anchors, [NO_BORDER] * len(anchors), (size, size))
    assert tab.total == total and tab.inside().all()
    gl, gb = ec.random_ground_truth(90 + size, 3, 7, counts=[7, 0, 3])
    gb[0, 0] = [-0.2, -0.1, 0.6, 0.5]                                         # a box over the image's edge: its anchors stay inside
    out = net.bboxes_encode(torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev), anchors)
    got = _to_np(out)
    _check(got, gl, gb, tab)
    assert sum(int((g[0] > 0).sum()) for g in got[0]) > 0 and not any(g[1].any() for g in got[0])
    # one image, numpy inputs, int64 labels, as the reference takes them: no batch axis, the same bytes as the batched row
    single = net.bboxes_encode(gl[0].astype(np.int64), gb[0], anchors)
    assert all(tuple(t.shape) == s for t, s in zip(single[0], tab.shapes))
    for k in range(4):
        for l in range(len(tab.shapes)):
            assert single[k][l].cpu().numpy().tobytes() == got[k][l][0].tobytes(), (k, l)
