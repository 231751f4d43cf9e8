"""The post-processing families check themselves (numpy only, no GPU): every family of tests/post_cases.py fulfils the conditions it
states, every mutant - the oracle pipeline, subtly wrong - is caught by exactly the families built to catch it, and the naive scalar
restatement of the two TensorFlow NMS functions equals oracle/tfe_post.py and oracle/ron_eval_post.py bit for bit.

Measured: the whole file takes 41 s in one process on the development machine (16 CPUs, one used; a machine two thirds as fast is
still inside the minute).  The scalar NMS loops are most of it: the mutant table runs them on the cases named in SUBSET only."""
import functools

import numpy as np
import pytest

import post_cases as pc
from oracle import np_post, tfe_post

F32 = np.float32
K = pc.constants()


@functools.lru_cache(maxsize=None)
def family(name):
    return pc.FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def oracles(name):
    return [pc.oracle(c) for c in family(name)]


def test_constants_are_read_from_the_source():
    assert set(K) == {'kSelectCap', 'kSortCap', 'kPartMin', 'kPartChunks', 'kEvalCand', 'kSelectThreads', 'RON_MAX_TOPK', 'RON_MAX_CLASSES'}
    assert K['kSelectCap'] < K['kSortCap'] < K['kPartMin'] and K['kPartChunks'] * K['RON_MAX_TOPK'] <= K['kSortCap']
    assert pc.RON320.n == 21250 and pc.SSD512.n == 24564


def test_thresholds_as_float32():
    """Which float32 the comparisons use: the decimal rounded to nearest (C float fields on the device side, np.float32 in the oracle)."""
    pins = {0.01: 0x3C23D70A, 0.03: 0x3CF5C28F, 0.5: 0x3F000000, 0.6: 0x3F19999A, 0.95: 0x3F733333,
            0.3: 0x3E99999A, 0.4: 0x3ECCCCCD, 0.45: 0x3EE66666}
    import ctypes
    for x, bits in pins.items():
        assert int(pc.thr32(x).view(np.uint32)) == bits
        assert ctypes.c_float(x).value == float(pc.thr32(x))
        lo, eq, hi = pc.around(x)
        assert lo < eq < hi and pc.ulps(hi, eq) == 1 and pc.ulps(eq, lo) == 1
    assert float(pc.thr32(0.01)) < 0.01 and float(pc.thr32(0.6)) > 0.6         # below / above the decimal


# --------------------------------------------------------------------------- #
# the families fulfil their conditions
# --------------------------------------------------------------------------- #
def test_A_np_plateaus_cross_the_cut_and_the_path_constants():
    sizes = set()
    for c, o in zip(family('A_np'), oracles('A_np')):
        o, e, top_k = o[0], c['expect'], c['kw']['top_k']
        assert o['n_candidates'] == e['n_candidates'] and o['n_sorted'] == min(top_k, e['n_candidates'])
        assert e['n_above'] < top_k < e['n_candidates'] or (top_k == 1 and e['n_above'] == 0)
        sizes.add(e['n_candidates'] - e['n_above'])
        # the sorted list: the rows above, then plateau rows in POSITION order (anchor-major, class-minor)
        cls, sc, bb, ai = _select(c)
        cls, sc, bb, ai = np_post.bboxes_sort(cls, sc, bb, top_k=top_k, extra=ai)
        assert (sc[e['n_above']:] == e['plateau_value']).all() and (sc[:e['n_above']] == F32(0.75)).all()
        pos = ai[e['n_above']:] * (c['num_classes'] - 1) + cls[e['n_above']:] - 1
        assert (np.diff(pos) > 0).all()
        if c['all_equal']:
            assert pos[0] == 0 and pos[-1] == top_k - 1                       # the first positions: layer 0
    assert any(K['kSelectCap'] < s <= K['kSortCap'] for s in sizes) and any(K['kSortCap'] < s <= K['kPartMin'] for s in sizes)
    assert sum(s > K['kPartMin'] for s in sizes) >= 3 and max(sizes) == pc.RON320.n * 80
    assert {c['kw']['top_k'] for c in family('A_np')} == {1, 64, 400, K['RON_MAX_TOPK']}
    assert {c['layout'].name for c in family('A_np')} == {'ron320', 'ssd512'} and {c['num_classes'] for c in family('A_np')} == {2, 21, 81}


def _select(c):
    gated = c['pred'] if c['obj'] is None else np_post.objectness_gate(c['pred'], c['obj'], c['kw']['objectness_thres'])
    cls, sc, bb, ai = np_post.bboxes_select_image([p[0] for p in gated], [b[0] for b in c['boxes']], c['kw']['select_threshold'])
    return cls, sc, bb, ai


def test_A_tfe_plateau_inside_one_class_list():
    cases = family('A_tfe') + pc.family_A_tfe(2)[:1] + pc.family_A_tfe(81)[1:2] + pc.family_A_tfe(21, pc.SSD512)[2:]
    assert {(c['num_classes'], c['layout'].name) for c in cases} == {(21, 'ron320'), (2, 'ron320'), (81, 'ron320'), (21, 'ssd512')}
    for c in cases:
        (s, b), e, kw = pc.oracle(c), c['expect'], c['kw']
        assert e['n_list'] > K['kPartMin'] and e['n_above'] < kw['keep_top_k'] < kw['top_k']
        row = s[0, e['list_class'] - 1]
        assert row[0] == F32(0.75) and set(row) == {F32(0.75), F32(0.5)} and (np.diff(row) <= 0).all() and row[-1] == F32(0.5)   # keep_top_k cuts inside the plateau
        live = {e['list_class']} | ({e['second_class']} - {None})
        assert {k + 1 for k in range(c['num_classes'] - 1) if s[0, k].any()} == live            # every other list is empty
        if e['second_class']:
            s2 = s[0, e['second_class'] - 1]
            assert (s2 > 0).sum() > 10 and len(set(s2[s2 > 0])) == (s2 > 0).sum()


def test_A_eval_kept_rows_come_from_later_passes():
    for c in family('A_eval') + pc.family_A_eval(2)[:1] + pc.family_A_eval(81)[1:]:
        for by in (False, True, 'scores'):
            o = pc.oracle_eval(c, by)[0]
            rank = np.searchsorted(c['expect']['rows'], o['anchor_index'])             # all scores equal: rank = position
            assert c['expect']['n_plateau'] > 2 * K['kEvalCand']
            assert (rank >= K['kEvalCand']).any() and ((rank >= 2 * K['kEvalCand']).any() or len(rank) == c['kw']['keep_top_k'])
            assert (o['classes'] == c['expect']['label']).all()                        # two classes tie: the lowest wins


def test_A_list_sizes_and_special_scores():
    cs = family('A_list')
    ns = sorted(c['scores'].shape[0] for c in cs)
    assert ns[0] == 401 and K['kSelectCap'] + 1 in ns and K['kSortCap'] + 1 in ns and 20000 in ns
    for c in cs[:4]:
        assert len(set(c['scores'])) == 3
    sp = cs[4]['scores']
    assert sp.shape[0] > K['kSelectCap'] and np.isnan(sp).sum() == 100 and np.isinf(sp).sum() == 200 and (sp == 0).sum() == 200


def test_B_counts_are_exact_and_on_the_boundaries():
    ms = pc.counts_np()
    for k in ('kSelectCap', 'kSortCap', 'kPartMin'):
        assert {K[k] - 1, K[k], K[k] + 1} <= set(ms)
    assert {0, 1, 63, 64, 65, 399, 400, 401, pc.RON320.n * 20} <= set(ms) and len(ms) <= 32
    for c, o in zip(family('B_np'), oracles('B_np')):
        assert [r['n_candidates'] for r in o] == ms
        sel = [np.concatenate([p[i].reshape(-1, 21)[:, 1:].reshape(-1) for p in c['pred']]) for i in range(len(ms))]
        for i, m in enumerate(ms):
            v = sel[i][sel[i] > pc.LOW]
            assert v.shape[0] == m and len(set(v)) == (min(m, 1) if c['name'].endswith('equal') else m)
    c = family('B_tfe')[0]
    mt = pc.counts_tfe()
    for img in range(2):
        flat = np.concatenate([p[img].reshape(-1, 21) for p in c['pred']])
        assert [(flat[:, k + 1] > pc.LOW).sum() for k in range(len(mt))] == mt
    for c, o in zip(family('B_eval'), oracles('B_eval')):
        me = pc.counts_eval()
        assert {K['kEvalCand'], K['kEvalCand'] + 1, 2 * K['kEvalCand'], 2 * K['kEvalCand'] + 1} <= set(me)
        for img, m in enumerate(me):
            flat = np.concatenate([p[img].reshape(-1, 21) for p in c['pred']])
            assert (flat.max(1) > F32(0.6)).sum() == m
        # nothing reaches keep_top_k in the class-agnostic run: every pass is taken
        assert all(len(r['classes']) < c['kw']['keep_top_k'] for r in o)


def test_C_only_the_rows_above_every_threshold_pass():
    for c, o in zip(family('C_np'), oracles('C_np')):
        assert o[0]['n_candidates'] == c['expect']['n_candidates'] == 10
    for c, (s, b) in zip(family('C_tfe'), oracles('C_tfe')):
        assert int((s > 0).sum()) == c['expect']['n_pass'] >= 1
    for c, o in zip(family('C_eval'), oracles('C_eval')):
        assert [len(r['classes']) for r in o] == [c['expect']['n_pass']] * 2
    for c, (s, b) in zip(family('C_filter_min'), oracles('C_filter_min')):
        assert int((s > 0).sum()) == c['expect']['n_pass'] == 5 and s.shape == (1, 8)


@pytest.mark.parametrize('flavour', ['iou', 'min', 'union'])
@pytest.mark.parametrize('thr', pc.NMS_THRESHOLDS)
def test_D_pairs_lie_within_two_ulp_of_the_threshold(flavour, thr):
    hi, lo, dist, dis = pc.near_threshold_pairs(flavour, thr)
    n = hi.shape[0]
    assert n == 200
    q = np.array([pc.oracle_overlap(hi[k], lo[k], flavour)[0] for k in range(n)], F32)
    assert np.array_equal(pc.ulps(q, pc.thr32(thr)), dist) and (np.abs(dist) <= 2).all()
    assert (dist == 0).sum() >= n // 10 and (dist < 0).sum() >= n // 10 and (dist > 0).sum() >= n // 10 and dis.sum() >= 3
    # the quotient the generator reasons about IS the oracle's, and the reciprocal form disagrees where it says so
    for k in np.flatnonzero(dis):
        inter, den = pc.overlap_parts(hi[k], lo[k], flavour)
        assert (inter / den)[0] == q[k] and ((pc.rcp_quotient(inter, den)[0] < pc.thr32(thr)) != (q[k] < pc.thr32(thr)))
    # pairs do not interact: overlap exactly 0 between boxes of different pairs
    allb = np.concatenate([hi, lo])
    pair = np.concatenate([np.arange(n), np.arange(n)])
    for k in range(allb.shape[0]):
        ov = pc.oracle_overlap(allb[k], allb, flavour)
        assert (ov[pair != pair[k]] == 0).all()
    boxes, scores, pid, is_hi, _, _ = pc.pair_rows(flavour, thr)
    assert len(set(scores)) == 2 * n
    order = np.argsort(-scores, kind='stable')
    rank = np.empty(2 * n, int)
    rank[order] = np.arange(2 * n)
    r_hi, r_lo = rank[is_hi], rank[~is_hi]
    assert (r_hi < r_lo).all()
    assert ((r_hi >> 4) != (r_lo >> 4)).sum() >= 20 and ((r_hi >> 6) != (r_lo >> 6)).sum() >= 20       # slots and blocks straddled
    first = np.flatnonzero(is_hi) < np.flatnonzero(~is_hi)
    assert first.sum() == n // 2                                                                          # by position: half and half


@pytest.mark.parametrize('flavour,thr', [('iou', t) for t in pc.NMS_THRESHOLDS] + pc.CHAINS_TF)
def test_D_chain_links(flavour, thr):
    b, d = pc.chain_boxes(flavour, thr)
    assert b.shape[0] >= 160 and (np.abs(d) <= 2).all() and (d < 0).sum() > 20 and (d >= 0).sum() > 20
    for i in range(b.shape[0] - 2):
        assert pc.ulps(pc.oracle_overlap(b[i], b[i + 1], flavour)[0], pc.thr32(thr)) == d[i]
        assert pc.oracle_overlap(b[i], b[i + 2], flavour)[0] < 0.75 * thr              # second neighbours: far below


def test_D_chain_cases_follow_their_links():
    """Through every entry point the chain's kept rows are what its links say: box i survives iff box i - 1 was dropped or link i - 1 lies
    BELOW the threshold (second neighbours never suppress)."""
    n_cases = 0
    for fam in ('D_np', 'D_list', 'D_tfe', 'D_eval'):
        for c, o in zip(family(fam), oracles(fam)):
            if 'chain' not in c['expect']:
                continue
            d = c['expect']['chain']
            kept = {'np': lambda: len(o[0]['classes']), 'list': lambda: len(o['classes']), 'eval': lambda: len(o[0]['classes']),
                    'tfe': lambda: int((o[0] > 0).sum())}[c['kind']]()
            assert kept == pc.chain_kept(d) and (d < 0).sum() > 20 and (d >= 0).sum() > 20, c['name']
            n_cases += 1
    assert n_cases == 4 + 4 + 7 + 7


def test_D_cases_keep_what_the_pairs_say():
    for fam in ('D_np', 'D_list', 'D_tfe', 'D_eval'):
        for c, o in zip(family(fam), oracles(fam)):
            if 'n_kept' not in c['expect']:
                continue
            kept = {'np': lambda: len(o[0]['classes']), 'list': lambda: len(o['classes']), 'eval': lambda: len(o[0]['classes']),
                    'tfe': lambda: int((o[0] > 0).sum())}[c['kind']]()
            assert kept == c['expect']['n_kept'] and c['expect']['n_on'] >= 20, c['name']


def test_E_degenerate_boxes_are_what_they_claim():
    b = pc.degenerate_boxes()
    with np.errstate(all='ignore'):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert (area == 0).sum() >= 7 and ((area > 0) & (area < 1e-30)).sum() >= 8 and (area > 1e30).sum() >= 4
    assert ((area > 0) & (area < np.finfo(F32).tiny)).sum() >= 4                       # subnormal areas
    assert ((b[:, 2] < b[:, 0]) | (b[:, 3] < b[:, 1])).sum() >= 4                      # inverted
    rep = tfe_post.clip_with_repair((0., 0., 1., 1.), b[10:12])
    assert ((rep[:, 2] - rep[:, 0]) * (rep[:, 3] - rep[:, 1]) == 0).all()              # the TF clip repairs them to zero area
    # the np flavour meets a NaN overlap (0 / 0) and suppresses; the TF flavours meet a non-positive denominator
    with np.errstate(all='ignore'):
        assert np.isnan(np_post.bboxes_jaccard(b[7], b[8:9])).all()
    assert tfe_post.overlap_scores(b[7], b[8:9], 'union')[0] == 0 and tfe_post.overlap_scores(b[7], b[8:9], 'min')[0] == 0
    for c, o in zip(family('E_np'), oracles('E_np')):
        assert o[0]['n_candidates'] == c['expect']['n_candidates']                     # the NaN probabilities select nothing
    o = pc.oracle(pc.inf_offsets_case())[0]
    assert o['n_candidates'] == 24 and np.isfinite(o['bboxes']).all() and (o['bboxes'] == [0, 0, 1, 1]).all(1).any()


# --------------------------------------------------------------------------- #
# mutants
# --------------------------------------------------------------------------- #
def test_own_np_pipeline_equals_the_oracle():
    for fam in pc.FAMILIES:
        if family(fam)[0]['kind'] in ('np', 'list', 'filter_min'):
            for c, o in zip(family(fam), oracles(fam)):
                assert pc.same(pc.mutated(c, None), o), c['name']


# which family catches which mutant (True = at least one case of the family gives a different result).  The scalar TF pipelines
# are slow, so their mutants run on the cases / class lists / images named in SUBSET.  'chunk_merge' models the partial pass, which
# only ron_post_np has (ron_np_sort_nms, ron_post_tfe and ron_post_eval call topk_keys directly): it is a mutant of the np kind alone.
TABLE = {
    'np': {'ties_desc': {'A_np': 1, 'B_np': 1, 'C_np': 1, 'D_np': 0, 'E_np': 0},
           'ge_select': {'A_np': 0, 'B_np': 0, 'C_np': 1, 'D_np': 0, 'E_np': 0},
           'ge_objectness': {'A_np': 0, 'B_np': 0, 'C_np': 1, 'D_np': 0, 'E_np': 0},
           'nms_le': {'A_np': 0, 'B_np': 0, 'C_np': 0, 'D_np': 1, 'E_np': 0},
           'rcp_only': {'A_np': 0, 'B_np': 0, 'C_np': 0, 'D_np': 1, 'E_np': 1},
           'nan_keeps': {'A_np': 0, 'B_np': 0, 'C_np': 0, 'D_np': 0, 'E_np': 1},
           'chunk_merge': {'A_np': 1, 'B_np': 1, 'C_np': 0, 'D_np': 0, 'E_np': 0}},
    'list': {'ties_desc': {'A_list': 1, 'D_list': 0, 'E_list': 0},
             'nms_le': {'A_list': 0, 'D_list': 1, 'E_list': 0},
             'rcp_only': {'A_list': 0, 'D_list': 1, 'E_list': 1},
             'nan_keeps': {'A_list': 0, 'D_list': 0, 'E_list': 1}},
    'tfe': {'ties_desc': {'A_tfe': 1, 'B_tfe': 1, 'C_tfe': 0, 'E_tfe': 0},
            'ge_min_size': {'C_tfe': 1, 'E_tfe': 0},
            'nms_le': {'D_tfe': 1, 'E_tfe': 0},
            'rcp_only': {'D_tfe': 1, 'E_tfe': 1},
            'no_safe_divide': {'D_tfe': 0, 'E_tfe': 1}},
    'eval': {'ties_desc': {'A_eval': 1, 'B_eval': 1, 'C_eval': 0, 'E_eval': 0},
             'ge_select': {'C_eval': 1, 'E_eval': 0},
             'ge_objectness': {'C_eval': 1, 'E_eval': 0},
             'ge_min_size': {'C_eval': 1, 'E_eval': 0},
             'nms_le': {'D_eval': 1, 'E_eval': 0},
             'one_pass': {'A_eval': 1, 'B_eval': 1, 'C_eval': 0, 'D_eval': 0, 'E_eval': 0}},
    'filter_min': {'ge_min_size': {'C_filter_min': 1}},
}
SUBSET = {'A_tfe': dict(cases=[0], classes=[7]), 'B_tfe': dict(classes=[11, 17]), 'A_eval': dict(cases=[1]),
          'D_tfe': dict(cases=[2, 10, 14]), 'D_eval': dict(cases=[2, 14]), 'B_eval': dict(cases=[1], images=[5])}


def _caught(fam, mutant):
    sub = SUBSET.get(fam, {})
    cs = family(fam)
    for i in sub.get('cases', range(len(cs))):
        c = cs[i]
        if c['kind'] in ('np', 'list', 'filter_min'):
            if not pc.same(pc.mutated(c, mutant), oracles(fam)[i]):
                return True
        elif c['kind'] == 'tfe':
            if not pc.same(pc.naive_tfe(c, mutant, sub.get('classes')), _naive(fam, i)):
                return True
        elif not pc.same(pc.naive_eval(c, mutant, sub.get('images')), _naive(fam, i)):
            return True
    return False


@functools.lru_cache(maxsize=None)
def _naive(fam, i):
    c, sub = family(fam)[i], SUBSET.get(fam, {})
    return pc.naive_tfe(c, None, sub.get('classes')) if c['kind'] == 'tfe' else pc.naive_eval(c, None, sub.get('images'))


@pytest.mark.parametrize('kind', sorted(TABLE))
def test_mutant_table(kind):
    assert set(TABLE[kind]) == set({'np': pc.NP_MUTANTS, 'list': set(pc.NP_MUTANTS) - {'ge_select', 'ge_objectness', 'chunk_merge'}, 'tfe': pc.TFE_MUTANTS, 'filter_min': ('ge_min_size',),
                                    'eval': pc.EVAL_MUTANTS}[kind])
    got = {m: {fam: int(_caught(fam, m)) for fam in row} for m, row in TABLE[kind].items()}
    assert got == TABLE[kind]
    for m, row in TABLE[kind].items():
        assert any(row.values()), 'mutant %s is caught by no family' % m


def test_every_family_is_in_the_table():
    used = {fam for kind in TABLE.values() for row in kind.values() for fam in row}
    assert used == set(pc.FAMILIES)


# --------------------------------------------------------------------------- #
# the second reference of the TF flavours
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('fam', ['A_tfe', 'D_tfe', 'E_tfe', 'C_tfe'])
def test_naive_tfe_equals_the_oracle(fam):
    for c, o in zip(family(fam), oracles(fam)):
        live = pc.live_classes(c)
        assert pc.same(pc.naive_tfe(c), o), c['name']
        dead = [k for k in range(1, c['num_classes']) if k not in live]
        assert not o[0][:, [k - 1 for k in dead]].any()                    # the lists the naive run skipped are empty in the oracle


@pytest.mark.parametrize('fam', ['A_eval', 'D_eval', 'E_eval', 'C_eval'])
def test_naive_eval_equals_the_oracle(fam):
    for c, o in zip(family(fam), oracles(fam)):
        assert pc.same(pc.naive_eval(c), o), c['name']
