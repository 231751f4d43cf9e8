"""Cases of the training update (tests/optim_ref.py holds the references): builders, the named cases of the mutant table, `grade`
and the packing the GPU tests use.  Inputs are made once per case from a seed of their own and never modified.

  gauss     weights ~ N(0, 1), gradients ~ N(0, 1) (another draw per step), slots as a few steps would leave them (second moments
            positive); hyper-parameters LARGE (rate 2^-3 .. 2^-5 changing between the steps, decay 2^-2 on every other tensor, epsilon
            2^-4) so that each term of each rule moves the result by far more than its bound: what the mutants are told apart by;
  lattice   small integers and powers of two chosen so that every intermediate is an exact fp32 value in any order: the result must
            EQUAL the float64 definition.  rmsprop: decay 0 (ms = g^2, sqrt exact); adam: beta2 0, one step at step 1 (lr_t = 2 lr),
            gradients +-2^k (the division is exact);
  poison    a weight_decay == 0 tensor holding an infinite weight: g + 0 * w would turn its gradient into NaN."""
import numpy as np

import optim_ref as orf

U, E = orf.UNIT, orf.ENTRIES
BOLD = dict(momentum=0.5, decay=0.75, beta1=0.5, beta2=0.75, epsilon=0.0625)
BOLD_LRS = (0.125, 0.125, 0.03125)          # a rate change between the steps, as the schedule's
BOLD_WD = 0.25
SINGLE_COUNTS = (1, 3, 4, 5, U - 1, U, U + 1, 2 * U + 7)
LIST_LENGTHS = (1, E - 1, E, E + 1, 2 * E + 1)


def list_counts(n):
    """n tensors of 1 to 9 elements."""
    return [1 + (5 * i + 3) % 9 for i in range(n)]


def mixed_decay(n, wd=BOLD_WD):
    """A mix of zero and non-zero decay: every other tensor, starting with a decayed one."""
    return [wd if i % 2 == 0 else 0.0 for i in range(n)]


def gauss_case(rule, counts, wds, steps=1, lrs=BOLD_LRS, hyper=BOLD, first_step=1, seed=0):
    rs = np.random.RandomState(1000 * seed + 17 * len(counts) + int(sum(counts)) % 1000 + orf.RULES.index(rule))
    tensors = []
    for c, wd in zip(counts, wds):
        f = lambda scale=1.0: (rs.randn(c) * scale).astype(np.float32)
        second = rule in ('rmsprop', 'adam')          # slot0 of rmsprop and slot1 of adam are mean squares
        s0 = np.abs(f()) + np.float32(0.5) if rule == 'rmsprop' else f(0.5)
        s1 = np.abs(f()) + np.float32(0.5) if rule == 'adam' else f(0.5)
        tensors.append(dict(w=f(), s0=s0, s1=s1 if second else f(0.5), wd=wd, g=[f() for _ in range(steps)]))
    return dict(rule=rule, hyper=dict(hyper), tensors=tensors, lrs=[np.float32(x) for x in lrs[:steps]], first_step=first_step,
                default_wd=BOLD_WD, exact=False)


def lattice_case(rule, counts=(5, 8, 3), seed=3):
    rs = np.random.RandomState(seed + orf.RULES.index(rule))
    hyper = dict(momentum=0.5, decay=0.0, beta1=0.5, beta2=0.0, epsilon=0.0)
    steps = 1 if rule in ('rmsprop', 'adam') else 2
    tensors = []
    for i, c in enumerate(counts):
        ints = lambda lo, hi, mul: (rs.randint(lo, hi + 1, size=c) * mul).astype(np.float32)
        g = [(2.0 ** rs.randint(1, 4, size=c) * rs.choice([-1.0, 1.0], size=c)).astype(np.float32) for _ in range(steps)]
        w = ints(-8, 8, 16)
        if steps == 1:          # g' = g + w / 4 must stay a power of two: it is a divisor there
            w = (4 * g[0] * rs.choice([1.0, 3.0], size=c)).astype(np.float32)
        tensors.append(dict(w=w, s0=ints(-4, 4, 8), s1=ints(0, 4, 8), wd=0.25 if i % 2 == 0 else 0.0, g=g))
    return dict(rule=rule, hyper=hyper, tensors=tensors, lrs=[np.float32(0.5), np.float32(0.25)][:steps], first_step=1, default_wd=0.25,
                exact=True)


def poison_case():
    case = gauss_case('momentum', [6, 5], [BOLD_WD, 0.0], steps=2, seed=5)
    case['tensors'][1]['w'] = case['tensors'][1]['w'].copy()
    case['tensors'][1]['w'][2] = np.float32(np.inf)
    return case


# named cases: what the mutant table refers to
CASES = {
    'sgd': lambda: gauss_case('sgd', [6, 5, 9], mixed_decay(3), steps=3),
    'momentum': lambda: gauss_case('momentum', [6, 5, 9], mixed_decay(3), steps=3),
    'rmsprop': lambda: gauss_case('rmsprop', [6, 5, 9], mixed_decay(3), steps=3),
    'adam': lambda: gauss_case('adam', [6, 5, 9], mixed_decay(3), steps=3),
    'adam_late': lambda: gauss_case('adam', [6, 5], mixed_decay(2), steps=2, first_step=3),
    'poison': poison_case,
    'two_units': lambda: gauss_case('momentum', [U + 5, 3], mixed_decay(2), steps=1),
    'two_launches': lambda: gauss_case('momentum', list_counts(E + 2), mixed_decay(E + 2), steps=1),
    'lattice_sgd': lambda: lattice_case('sgd'), 'lattice_momentum': lambda: lattice_case('momentum'),
    'lattice_rmsprop': lambda: lattice_case('rmsprop'), 'lattice_adam': lambda: lattice_case('adam'),
}

# mutant -> the case that rejects it
MUTANTS = {
    'decoupled': 'momentum',                      # w -= lr wd w outside the accumulator: the same first step, another second one
    'decay_on_undecayed': 'sgd',
    'zero_times_w': 'poison',
    'dampening': 'momentum',
    'lr_in_accumulator': 'momentum',              # the same until the rate changes
    'nesterov': 'momentum',
    'rms_eps_outside': 'rmsprop',
    'adam_eps_inside': 'adam',
    'adam_no_bias_correction': 'adam',
    'adam_step_off_by_one': 'adam_late',
    'reg_no_half': 'sgd',
    'reg_from_updated': 'sgd',
    'reg_over_undecayed': 'sgd',
    'tail_dropped': 'sgd',
    'last_unit_dropped': 'two_units',
    'launch_boundary_skipped': 'two_launches',
}

_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = CASES[name]()
    return _CACHE[name]


def reference(c):
    """The float64 definition with its bounds, once per case object."""
    key = id(c)
    if key not in _CACHE:
        _CACHE[key] = (c, orf.run(c, 'bound'))
    return _CACHE[key][1]


def grade(label, got, c, verbose=False, exact_rules=None):
    """`got`: what orf.run returns (plain arrays).  Every step, every tensor, every element of w and the slots the rule uses within the
    derived bound of the float64 definition (equal on an exact case), reg_loss within its own.  Returns the largest ratios."""
    ref = reference(c)
    worst = dict(w=0.0, s0=0.0, s1=0.0, reg=0.0)
    assert len(got) == len(ref)
    kinds = ('w', 's0', 's1')[:1 + orf.SLOTS[c['rule']]]
    for k, (gs, rs) in enumerate(zip(got, ref)):
        for kind in kinds:
            for i, (a, r) in enumerate(zip(gs[kind], rs[kind])):
                a = orf.value(a)
                if c['exact']:
                    assert np.array_equal(np.asarray(a, np.float64), r.v), '%s: step %d, %s of tensor %d is not the exact value' % (label, k, kind, i)
                    continue
                q = orf.ratio(a, r)
                worst[kind] = max(worst[kind], float(q.max()))
                assert q.max() <= 1.0, '%s: step %d, %s of tensor %d: element %d is %.3g of its bound away (got %r, want %r +- %.3g)' % (
                    label, k, kind, i, int(q.argmax()), q.max(), float(np.asarray(a).reshape(-1)[q.argmax()]), float(r.v.reshape(-1)[q.argmax()]),
                    float(r.e.reshape(-1)[q.argmax()]))
        if gs.get('reg') is not None:
            q = float(orf.ratio(orf.value(gs['reg']), rs['reg']))
            if c['exact']:
                assert float(orf.value(gs['reg'])) == float(rs['reg'].v), '%s: step %d: reg_loss is not the exact value' % (label, k)
            worst['reg'] = max(worst['reg'], q)
            assert q <= 1.0, '%s: step %d: reg_loss %r, want %r +- %.3g' % (label, k, float(orf.value(gs['reg'])), float(rs['reg'].v), float(rs['reg'].e))
    if verbose:
        print('%s: largest error / bound: %s' % (label, ', '.join('%s %.3f' % (k, worst[k]) for k in kinds + ('reg',))))
    return worst


# ------------------------------------------------------------------------------------------------------------------------- packing
SENTINEL = np.uint32(0x7FC0BEEF)          # a NaN nobody computes
FRONT = BACK = 4                           # floats of sentinel in front of the first and behind the last tensor


def pack(arrays):
    """One buffer per kind: the tensors at consecutive 16-byte-aligned offsets, as close as the contract allows (a tensor starts 16
    bytes behind its neighbour's last whole vector), the gaps and both ends holding SENTINEL.  Returns (uint32 view of the float32
    buffer, offsets in floats)."""
    offsets, at = [], FRONT
    for a in arrays:
        offsets.append(at)
        at += (a.size + 3) // 4 * 4
    buf = np.full(at + BACK, SENTINEL, np.uint32)
    for a, off in zip(arrays, offsets):
        buf[off:off + a.size] = np.asarray(a, np.float32).view(np.uint32)
    return buf, offsets


def sentinels_intact(buf, arrays, offsets):
    """Every word of `buf` (uint32) outside the tensors still holds SENTINEL."""
    outside = np.ones(buf.size, bool)
    for a, off in zip(arrays, offsets):
        outside[off:off + a.size] = False
    return bool((buf[outside] == SENTINEL).all())
