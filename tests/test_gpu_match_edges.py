"""GPU parity of ron_bboxes_matching at its decision points: every case of tests/match_cases.py (A threshold, B ties, C nothing to
match, D state, E degenerate boxes, F extent) through metrics.bboxes_matching, n_gbboxes / tp / fp bit-equal to the oracle; the same
cases stacked along N in one launch; the wrapper's relabelling, layout and dtype branches; and the family-D list through the
streaming accumulators down to the two AP values worked out by hand in tests/test_match_cases_cpu.py."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import match_cases as mc  # noqa: E402
from test_match_cases_cpu import D_AP07, D_AP12, D_FP, D_NGB, D_TP, chain  # noqa: E402

CASES = mc.match_cases()
GROUPS = mc.stack_groups(CASES)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def metrics():
    from ron_tensorflow_amd import metrics as _metrics
    return _metrics


@pytest.fixture(scope='module')
def oracle_results():
    """The oracle on every case, once."""
    return {c.name: mc.oracle(c) for c in CASES}


def _run(metrics, dev, sc, bb, gl, gb, gd, thr):
    out = metrics.bboxes_matching(torch.from_numpy(sc).to(dev), torch.from_numpy(bb).to(dev), gl, gb, gd, thr)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.bool and out[2].dtype == torch.bool
    return tuple(t.cpu().numpy() for t in out)


def _diff(got, ref):
    return [name for name, a, b in zip(('n_gbboxes', 'tp', 'fp'), got, ref) if a.shape != b.shape or not np.array_equal(a, b)]


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_case_vs_oracle(metrics, dev, oracle_results, case):
    args = (case.scores, case.bboxes, case.glabels, case.gbboxes, case.gdifficults, case.threshold)
    got = _run(metrics, dev, *args)
    ref = oracle_results[case.name]
    bad = _diff(got, ref)
    assert not bad, '%s: %s differ; tp %s vs %s, fp %s vs %s, n %s vs %s' % (
        case.name, bad, got[1].astype(int).tolist(), ref[1].astype(int).tolist(), got[2].astype(int).tolist(), ref[2].astype(int).tolist(),
        got[0].tolist(), ref[0].tolist())
    again = _run(metrics, dev, *args)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), 'second call differs'


@pytest.mark.parametrize('group', GROUPS, ids=['L%d_K%d_G%d_thr%g' % (g[2].shape[1], g[2].shape[2], g[4].shape[1], g[7]) for g in GROUPS])
def test_stacked_cases(metrics, dev, oracle_results, group):
    """Cases of equal (L, K, G, threshold) as the images of ONE launch: no flag, count or argmax leaks from a list or an image into
    the next.  Forwards and backwards, so that every case has stood behind every other kind of neighbour."""
    cs, offs, sc, bb, gl, gb, gd, thr = group
    got = _run(metrics, dev, sc, bb, gl, gb, gd, thr)
    rev = _run(metrics, dev, *(np.ascontiguousarray(a[::-1]) for a in (sc, bb, gl, gb, gd)), thr)
    n = sc.shape[0]
    bad = []
    for c, a, b in zip(cs, offs[:-1], offs[1:]):
        ref = oracle_results[c.name]
        if _diff([x[a:b] for x in got], ref):
            bad.append(c.name)
        if _diff([x[::-1][a:b] for x in rev], ref):
            bad.append(c.name + ' (reversed)')
    assert not bad and n == offs[-1], bad


def _wrapper_inputs():
    """Two images, lists of labels 15, 3, 7; ground truth of those labels, of labels 1, 2, 16, 20 (which belong to no list; 1, 2 and 3
    are the values the relabelling itself writes), and padding.  Every list has a tp, a duplicate, a hit on a difficult box."""
    A, B, C = mc.D_A, mc.D_B, mc.D_C
    im0 = [(1, A, 0), (15, A, 0), (3, A, 0), (2, B, 0), (7, B, 0), (15, C, 1), (3, C, 2), (16, A, 0), (7, C, 255), (0, [0] * 4, 0)]
    im1 = [(20, B, 0), (7, A, 0), (3, B, 1), (15, B, 0), (2, A, 0), (0, [0] * 4, 0), (0, [0] * 4, 0), (1, C, 0), (3, A, 0), (15, C, 0)]
    g, k = 10, 6
    gl, gb, gd = np.zeros((2, g), np.int64), np.zeros((2, g, 4), np.float32), np.zeros((2, g), np.int64)
    for i, im in enumerate((im0, im1)):
        for j, (lab, box, d) in enumerate(im):
            gl[i, j], gb[i, j], gd[i, j] = lab, box, d
    dets = [A, mc.inside(A, 0.9), B, C, mc.inside(B, 0.4)]
    sc, bb = np.zeros((2, 3, k), np.float32), np.zeros((2, 3, k, 4), np.float32)
    sc[:, :] = mc.det_scores(len(dets), k)
    bb[:, :, :len(dets)] = np.asarray(dets, np.float32)
    return sc, bb, gl, gb, gd


LABELS = [15, 3, 7]


def _dicts(dev, sc, bb):
    return ({c: torch.from_numpy(sc[:, l]).to(dev) for l, c in enumerate(LABELS)},
            {c: torch.from_numpy(bb[:, l]).to(dev) for l, c in enumerate(LABELS)})


def _check_dicts(got, ref):
    d_n, d_tp, d_fp = got
    assert sorted(d_n) == sorted(d_tp) == sorted(d_fp) == sorted(LABELS)
    for l, c in enumerate(LABELS):
        assert d_n[c].dtype == torch.int64 and d_tp[c].dtype == torch.bool
        assert np.array_equal(d_n[c].cpu().numpy(), ref[0][:, l]), ('n_gbboxes', c)
        assert np.array_equal(d_tp[c].cpu().numpy(), ref[1][:, l]), ('tp', c)
        assert np.array_equal(d_fp[c].cpu().numpy(), ref[2][:, l]), ('fp', c)


@pytest.fixture(scope='module')
def wrapper_ref():
    sc, bb, gl, gb, gd = _wrapper_inputs()
    ref = mc.oracle_dense(sc, bb, gl, gb, gd, 0.5, labels=LABELS)
    assert mc.same_result(ref, mc.match_ref(sc, bb, gl, gb, gd, 0.5, labels=LABELS))
    # the inputs do what they were built for: per list a tp and a duplicate; difficult values 1, 2, 255 all count as difficult
    assert ref[1].any(-1).all() and ref[2].any(-1).all()
    assert ref[0].tolist() == [[1, 1, 1], [2, 1, 1]]
    return ref


def test_wrapper_relabels_arbitrary_labels(metrics, dev, wrapper_ref):
    sc, bb, gl, gb, gd = _wrapper_inputs()
    d_s, d_b = _dicts(dev, sc, bb)
    _check_dicts(metrics.bboxes_matching_batch(LABELS, d_s, d_b, gl, gb, gd), wrapper_ref)
    # the result depends on the label list: with labels 1, 2, 3 the same arrays match other boxes
    plain = metrics.bboxes_matching_batch([1, 2, 3], {c: d_s[k] for c, k in zip((1, 2, 3), LABELS)},
                                          {c: d_b[k] for c, k in zip((1, 2, 3), LABELS)}, gl, gb, gd)
    ref = mc.oracle_dense(sc, bb, gl, gb, gd, 0.5, labels=[1, 2, 3])
    assert not mc.same_result(ref, wrapper_ref)
    for l, c in enumerate((1, 2, 3)):
        assert np.array_equal(plain[0][c].cpu().numpy(), ref[0][:, l]) and np.array_equal(plain[1][c].cpu().numpy(), ref[1][:, l])
        assert np.array_equal(plain[2][c].cpu().numpy(), ref[2][:, l])


@pytest.mark.parametrize('gl_kind', ['int64_numpy', 'int32_torch_host', 'int64_torch_device', 'int32_numpy_strided'])
def test_wrapper_label_dtypes(metrics, dev, wrapper_ref, gl_kind):
    sc, bb, gl, gb, gd = _wrapper_inputs()
    if gl_kind == 'int32_torch_host':
        gl = torch.from_numpy(gl.astype(np.int32))
    elif gl_kind == 'int64_torch_device':
        gl = torch.from_numpy(gl).to(dev)
    elif gl_kind == 'int32_numpy_strided':
        wide = np.full((2, 20), 15, np.int32)
        wide[:, ::2] = gl
        gl = wide[:, ::2]
        assert not gl.flags['C_CONTIGUOUS']
    d_s, d_b = _dicts(dev, sc, bb)
    _check_dicts(metrics.bboxes_matching_batch(LABELS, d_s, d_b, gl, gb, gd), wrapper_ref)


def test_wrapper_difficult_values_and_dtypes(metrics, dev, wrapper_ref):
    """gdifficults 2 and 255 are difficult (tf.cast(.., tf.bool)), whatever the type they arrive in."""
    sc, bb, gl, gb, gd = _wrapper_inputs()
    assert {0, 1, 2, 255} <= set(gd.reshape(-1).tolist())
    d_s, d_b = _dicts(dev, sc, bb)
    for conv in (lambda a: a, lambda a: a.astype(np.uint8), lambda a: torch.from_numpy(a.astype(np.int32)).to(dev),
                 lambda a: torch.from_numpy(a.astype(np.float32))):
        _check_dicts(metrics.bboxes_matching_batch(LABELS, d_s, d_b, gl, gb, conv(gd)), wrapper_ref)


def test_wrapper_non_contiguous_views(metrics, dev, wrapper_ref):
    """scores / bboxes as strided views of larger device tensors (dense and dict entry), ground truth as strided numpy views."""
    sc, bb, gl, gb, gd = _wrapper_inputs()
    n, nl, k = sc.shape
    big_s = torch.full((n, nl, 2 * k), 7.0, device=dev)
    big_b = torch.full((n, nl, k, 8), 0.25, device=dev)
    big_s[:, :, ::2] = torch.from_numpy(sc).to(dev)
    big_b[..., ::2] = torch.from_numpy(bb).to(dev)
    s_view, b_view = big_s[:, :, ::2], big_b[..., ::2]
    assert not s_view.is_contiguous() and not b_view.is_contiguous()
    gb_wide = np.full((2, 10, 8), 0.5, np.float32)
    gb_wide[..., ::2] = gb
    gd_t = np.ascontiguousarray(gd.T).T
    assert not gd_t.flags['C_CONTIGUOUS']
    remap = np.zeros_like(gl)
    for i, c in enumerate(LABELS):
        remap[gl == c] = i + 1
    got = metrics.bboxes_matching(s_view, b_view, remap, gb_wide[..., ::2], gd_t)
    assert not _diff([t.cpu().numpy() for t in got], wrapper_ref)
    d_s = {c: s_view[:, l] for l, c in enumerate(LABELS)}
    d_b = {c: b_view[:, l] for l, c in enumerate(LABELS)}
    _check_dicts(metrics.bboxes_matching_batch(LABELS, d_s, d_b, gl, gb_wide[..., ::2], gd_t), wrapper_ref)


def test_state_walk_chain_to_ap(metrics, dev):
    case = [c for c in CASES if c.name == 'D/state_walk'][0]
    n_gb, tp, fp = metrics.bboxes_matching(torch.from_numpy(case.scores).to(dev), torch.from_numpy(case.bboxes).to(dev), case.glabels,
                                           case.gbboxes, case.gdifficults, case.threshold)
    assert n_gb.cpu().tolist() == [[D_NGB]] and tp[0, 0].int().cpu().tolist() == D_TP and fp[0, 0].int().cpu().tolist() == D_FP
    ap07, ap12 = chain(n_gb, tp, fp, torch.from_numpy(case.scores).to(dev))
    assert abs(ap07 - D_AP07) < 1e-12 and ap12 == D_AP12
