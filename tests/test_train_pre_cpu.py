"""CPU: the two restatements of ron_preprocess_for_train's geometry (tests/train_pre_ref.py) agree, every hand-built case of
tests/train_pre_cases.py sits at the decision point it names, and every mutant of the references is told apart by a case."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_pre_cases as tc  # noqa: E402
import train_pre_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM_CASES = tc.geometry_cases()
PIXEL_CASES = tc.pixel_cases()


def _agree(h, w, gl, gb, d):
    a = tr.geometry_np(h, w, gl, gb, d)
    g, l, b, k = tr.geometry_scalar(h, w, gl, gb, d)
    assert np.array_equal(a['geom'][:10], g), (a['geom'], g)
    assert np.array_equal(a['labels'], l) and np.array_equal(a['bboxes'], b) and a['count'] == k
    return a


@pytest.mark.parametrize('case', GEOM_CASES, ids=[c.name for c in GEOM_CASES])
def test_geometry_case_sits_where_it_says_and_both_references_agree(case):
    r = _agree(case.h, case.w, case.glabels, case.gbboxes, case.draws)
    case.condition(case, r)
    for m in case.catches:
        assert not tc.same_result(r, tc.reference(case, mut=(m,))), 'mutant %s survives %s' % (m, case.name)
    # the shape of every result: kept rows in front, zeros behind, a window inside the canvas
    k, g = r['count'], r['geom']
    assert (r['labels'][:k] != 0).all() and not r['labels'][k:].any() and not r['bboxes'][k:].any()
    assert g[5] >= 0 and g[6] >= 0 and g[7] >= 1 and g[8] >= 1 and g[5] + g[7] <= g[1] and g[6] + g[8] <= g[2]


def test_references_agree_on_500_random_images():
    seen = dict(expanded=0, flip=0, cropped=0, whole=0, dropped=0, rounds=set())
    for (h, w, g, gl, gb, d) in tc.random_images(2024, 500):
        r = _agree(h, w, gl, gb, d)
        geom = r['geom']
        assert geom[5] >= 0 and geom[6] >= 0 and geom[5] + geom[7] <= geom[1] and geom[6] + geom[8] <= geom[2]
        seen['expanded'] += int(geom[0]); seen['flip'] += int(geom[9])
        whole = tuple(geom[5:9]) == (0, 0, geom[1], geom[2])
        seen['whole'] += int(whole); seen['cropped'] += int(not whole)
        seen['dropped'] += int(r['count'] < tr.present_rows(gl))
        seen['rounds'].add(int(geom[11]))
    # the random set reaches every branch
    assert min(seen['expanded'], seen['flip'], seen['cropped'], seen['whole'], seen['dropped']) > 20, seen
    assert {1, 10} <= seen['rounds']


def test_every_mutant_is_killed_by_a_case():
    caught = {m for c in GEOM_CASES for m in c.catches} | {m for c in PIXEL_CASES for m in c.catches}
    assert caught == set(tr.MUTANTS)
    for m in tr.GEOMETRY_MUTANTS:
        killers = [c.name for c in GEOM_CASES if not tc.same_result(tc.reference(c), tc.reference(c, mut=(m,)))]
        assert killers, m


@pytest.mark.parametrize('case', PIXEL_CASES, ids=[c.name for c in PIXEL_CASES])
def test_pixel_case_sits_where_it_says(case):
    case.condition(case)
    ref = tr.pixels_ref(case.images[0], case.geom[0], case.out_shape)
    assert ref.shape == tuple(case.out_shape) + (3,) and ref.dtype == np.float32
    for m in case.catches:
        assert not np.array_equal(ref, tr.pixels_ref(case.images[0], case.geom[0], case.out_shape, mut=(m,))), m


def test_pixel_reference_identities():
    """A plain geometry of the output's own size returns the image: (u8 / 255) * 255 - mean."""
    img = tc.random_image(3, 16, 12)
    out = tr.pixels_ref(img, tc.geom_row(16, 12), (16, 12))
    assert np.abs(out - (img.astype(np.float32) - np.asarray(tr.MEANS, np.float32))).max() <= 2e-5
    # a window wholly in the fill is the constant mean colour
    g = tc.geom_row(16, 12, expanded=True, img=(15, 11), crop=(0, 0, 10, 8))
    out = tr.pixels_ref(img, g, (20, 12))
    want = tr.canvas_fill(img) * np.float32(255) - np.asarray(tr.MEANS, np.float32)
    assert np.array_equal(out, np.broadcast_to(want, out.shape))
    assert np.abs(tr.canvas_fill(img).astype(np.float64) * 255 - img.reshape(-1, 3).mean(axis=0)).max() < 1e-4


def test_pixel_batches_are_inside_their_canvases():
    for name, imgs, geoms, out in tc.pixel_batches():
        assert len(imgs) == 3 and geoms.shape == (3, tr.RON_TRAIN_GEOM)
        for im, g in zip(imgs, geoms):
            assert tr.pixels_ref(im, g, out).shape == tuple(out) + (3,)


def test_header_declares_the_new_entries():
    text = open(os.path.join(ROOT, 'include', 'ron_hip.h')).read()
    for name in ('ron_train_geometry', 'ron_preprocess_train_workspace_bytes', 'ron_preprocess_train'):
        assert re.search(r'\b%s\s*\(' % name, text), name
    assert re.search(r'#define\s+RON_TRAIN_DRAWS\s+%d\b' % tr.RON_TRAIN_DRAWS, text)
    assert re.search(r'#define\s+RON_TRAIN_GEOM\s+%d\b' % tr.RON_TRAIN_GEOM, text)
    from ron_tensorflow_amd import _lib
    assert _lib.RON_TRAIN_DRAWS == tr.RON_TRAIN_DRAWS and _lib.RON_TRAIN_GEOM == tr.RON_TRAIN_GEOM
