"""Golden G9 (tests/golden/make_golden_ssd300.py: the reference's torch VGG16 on a 300^2 image, its pool3 the ceil pool 75 -> 38) and
the check of a tensor against it: the one tests/g8_util.py applies to G8, on this file."""
import os

import numpy as np

from oracle import synth

G9 = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g9_vgg_backbone_300.npz'))
SIZE = 300


def check_tensor(name, a, tol=1e-5, sum_tol=1e-6):
    """a [1,H,W,C] against G9's record of module `name`: shape; the sampled values within `tol` of the tensor's largest value; the
    float64 sum and sum of squares over the WHOLE tensor within `sum_tol` / 2 `sum_tol`, relative (a wrong edge row or column of an
    odd map moves them by far more).  Returns (sample error, sum error, sum-of-squares error)."""
    key = '%d/%s' % (SIZE, name)
    assert tuple(G9[key + '/shape']) == a.shape, (key, a.shape)
    iy, ix = synth.g8_sample_index(a.shape[1]), synth.g8_sample_index(a.shape[2])
    want = G9[key + '/sample']
    got = a[:, iy][:, :, ix]
    err = float(np.abs(got - want).max()) / float(np.abs(want).max())
    s1, s2 = G9[key + '/sum']
    d1 = abs(a.sum(dtype=np.float64) - s1) / s1
    d2 = abs((a.astype(np.float64) ** 2).sum() - s2) / s2
    assert err <= tol, '%s: sampled values off by %.3g of the tensor scale' % (key, err)
    assert d1 <= sum_tol and d2 <= 2 * sum_tol, '%s: whole-tensor sums off by %.3g / %.3g' % (key, d1, d2)
    return err, d1, d2
