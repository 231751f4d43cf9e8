"""GPU parity of the training update (ron_optimizer_step) against the float32 emulation of tests/optim_ref.py on the cases of
tests/optim_cases.py: the updated weights and slots and reg_loss must EQUAL the emulation bit for bit (and, with that, sit inside the
derived bounds of the float64 definition, whose largest ratios each case prints: pytest -s).

Every case packs var, grad and the slots in one buffer per kind, the tensors at consecutive 16-byte-aligned offsets as close as the
contract allows, the gaps and both ends holding a sentinel: after the call every sentinel word and every word of grad is unchanged.

  single tensors of 1, 3, 4, 5, U - 1, U, U + 1, 2U + 7 elements and lists of 1, E - 1, E, E + 1, 2E + 1 tensors of 1 to 9 elements (U
  elements per work unit, E table entries per launch, from ron_optimizer_plan), all four rules, decayed and undecayed tensors mixed;
  the lattice cases (exact against the definition, and one by hand); three steps across the schedule's rate change; Adam at step 1 and
  at a large step; the workspace (untouched without reg_loss, not read with it), the same bytes on every call; the stream contract;
  one chain through the existing operators into Optimizer.apply_gradients."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import optim_cases as oc  # noqa: E402
import optim_ref as orf  # noqa: E402
import stream_util as su  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from ron_tensorflow_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def side(dev):
    return su.independent_stream(dev, 0)


@pytest.fixture(scope='module', autouse=True)
def geometry_is_the_library_s(ops):
    """U and E of the emulation are the numbers ron_optimizer_plan reports."""
    launches, units, entries, unit = ops.optimizer_plan([1, 2 * orf.UNIT + 7])
    assert (entries, unit) == (orf.ENTRIES, orf.UNIT) and (launches, units) == (1, 4)


def _up(words, dev):
    """A uint32 numpy buffer as a float32 device tensor, bits untouched."""
    return torch.from_numpy(words.view(np.int32).copy()).to(dev).view(torch.float32)


def _down(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _gauss(rule, counts, wds, steps=1, first_step=1):
    return oc.gauss_case(rule, list(counts), list(wds), steps=steps, first_step=first_step)


@functools.lru_cache(maxsize=None)
def _emulated(key):
    """The emulation of a cached case, once."""
    return orf.emulate32(_CASES[key])


_CASES = {}


def _remember(case):
    _CASES[id(case)] = case
    return id(case)


def _device_run(ops, dev, case, want_reg=True, workspace=None):
    """Every step of a case on the device from packed buffers.  Returns (steps as orf.run returns them, float32 arrays; ok flags)."""
    rule, tensors = case['rule'], case['tensors']
    kinds = {k: [t[k] for t in tensors] for k in ('w', 's0', 's1')}
    packed = {k: oc.pack(v) for k, v in kinds.items()}
    dbuf = {k: _up(words, dev) for k, (words, _) in packed.items()}
    offsets = packed['w'][1]
    view = lambda buf: [buf[off:off + t['w'].size] for off, t in zip(offsets, tensors)]
    out = []
    for k, lr in enumerate(case['lrs']):
        gwords, goff = oc.pack([t['g'][k] for t in tensors])
        assert goff == offsets
        gbuf = _up(gwords, dev)
        before = {kind: _down(dbuf[kind]).copy() for kind in dbuf}
        table = [(w, g, s0, s1, t['wd']) for w, g, s0, s1, t in zip(view(dbuf['w']), view(gbuf), view(dbuf['s0']), view(dbuf['s1']), tensors)]
        reg = ops.optimizer_step(rule, table, float(lr), step=case['first_step'] + k, want_reg_loss=want_reg, workspace=workspace, **case['hyper'])
        after = {kind: _down(dbuf[kind]) for kind in dbuf}
        assert np.array_equal(_down(gbuf), gwords), 'step %d: the gradients were written' % k
        for kind in after:
            assert oc.sentinels_intact(after[kind], kinds[kind], offsets), 'step %d: a sentinel of %s was overwritten' % (k, kind)
        for kind in ('s0', 's1')[orf.SLOTS[rule]:]:
            assert np.array_equal(after[kind], before[kind]), 'step %d: %s is not a slot of %s and was written' % (k, kind, rule)
        cut = lambda words: [words[off:off + t['w'].size].view(np.float32).copy() for off, t in zip(offsets, tensors)]
        out.append(dict(w=cut(after['w']), s0=cut(after['s0']), s1=cut(after['s1']), reg=None if reg is None else np.float32(reg.item())))
    return out


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _assert_is_emulation(label, got, case, verbose=True):
    want = _emulated(_remember(case))
    kinds = ('w', 's0', 's1')[:1 + orf.SLOTS[case['rule']]]
    for k, (gs, ws) in enumerate(zip(got, want)):
        for kind in kinds:
            for i, (a, b) in enumerate(zip(gs[kind], ws[kind])):
                diff = np.flatnonzero(_bits(a) != _bits(b))
                assert diff.size == 0, '%s: step %d, %s of tensor %d: %d of %d elements differ from the emulation, the first at %d: %r, want %r' % (
                    label, k, kind, i, diff.size, a.size, diff[0], a[diff[0]], b[diff[0]])
        if gs['reg'] is not None:
            assert _bits(gs['reg']) == _bits(ws['reg']), '%s: step %d: reg_loss %r, the emulated tree gives %r' % (label, k, gs['reg'], ws['reg'])
    oc.grade(label, got, case, verbose=verbose)


# --------------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize('rule', orf.RULES)
@pytest.mark.parametrize('count', oc.SINGLE_COUNTS)
def test_single_tensors(ops, dev, count, rule):
    for wd in (oc.BOLD_WD, 0.0):
        case = _gauss(rule, (count,), (wd,))
        _assert_is_emulation('%s, one tensor of %d, decay %g' % (rule, count, wd), _device_run(ops, dev, case), case)


@pytest.mark.parametrize('rule', orf.RULES)
@pytest.mark.parametrize('n', oc.LIST_LENGTHS)
def test_lists(ops, dev, n, rule):
    case = _gauss(rule, tuple(oc.list_counts(n)), tuple(oc.mixed_decay(n)))
    _assert_is_emulation('%s, %d tensors' % (rule, n), _device_run(ops, dev, case), case)


@pytest.mark.parametrize('rule', orf.RULES)
def test_mixed_sizes_in_one_list(ops, dev, rule):
    """Every single size in ONE list (units of several tensors in one launch, the search over the table), without reg_loss too."""
    case = _gauss(rule, oc.SINGLE_COUNTS, tuple(oc.mixed_decay(len(oc.SINGLE_COUNTS))))
    _assert_is_emulation('%s, the sizes in one list' % rule, _device_run(ops, dev, case), case)
    _assert_is_emulation('%s, the sizes in one list, no reg_loss' % rule, _device_run(ops, dev, case, want_reg=False), case, verbose=False)


@pytest.mark.parametrize('name', ['poison', 'two_units', 'two_launches', 'adam_late'])
def test_named_cases_of_the_mutant_table(ops, dev, name):
    case = oc.case(name)
    _assert_is_emulation(name, _device_run(ops, dev, case), case)


@pytest.mark.parametrize('rule', orf.RULES)
def test_lattice_is_exact(ops, dev, rule):
    case = oc.case('lattice_' + rule)
    got = _device_run(ops, dev, case)
    want = orf.run(case, 'f64')
    for gs, ws in zip(got, want):
        for kind in ('w', 's0', 's1')[:1 + orf.SLOTS[rule]]:
            for a, b in zip(gs[kind], ws[kind]):
                assert np.array_equal(a.astype(np.float64), b), 'lattice %s: %s is not the exact value' % (rule, kind)
        assert float(gs['reg']) == ws['reg']


def test_lattice_by_hand(ops, dev):
    """w 8, g 2, m 4, decay 1/4, momentum 1/2, rate 1/2: g' = 2 + 8 / 4 = 4, m = 4 / 2 + 4 = 6, w = 8 - 6 / 2 = 5; undecayed: m = 4 / 2 + 2 = 4,
    w = 8 - 4 / 2 = 6; reg_loss = (1 / 8) (64 + 64 + 64) = 24 over the three decayed elements.  Then sgd, rmsprop and adam on one element each."""
    t = lambda *v: torch.tensor(v, dtype=torch.float32, device=dev)
    w, g, m = t(8, 8, 8), t(2, 2, 2), t(4, 4, 4)
    w2, g2, m2 = t(8), t(2), t(4)
    reg = ops.optimizer_step('momentum', [(w, g, m, None, 0.25), (w2, g2, m2, None, 0.0)], 0.5, momentum=0.5, want_reg_loss=True)
    assert w.tolist() == [5.0] * 3 and m.tolist() == [6.0] * 3 and w2.tolist() == [6.0] and m2.tolist() == [4.0] and reg.item() == 24.0
    w = t(8)
    ops.optimizer_step('sgd', [(w, t(2), None, None, 0.25)], 0.5)                                  # 8 - (2 + 2) / 2
    assert w.tolist() == [6.0]
    w, ms, mom = t(8), t(7), t(4)
    ops.optimizer_step('rmsprop', [(w, t(-4), ms, mom, 0.0)], 0.5, momentum=0.5, decay=0.0, epsilon=0.0)
    assert ms.tolist() == [16.0] and mom.tolist() == [1.5] and w.tolist() == [6.5]                  # mom = 4 / 2 + (-2) / 4; w = 8 - 1.5
    w, m, v = t(8), t(8), t(5)
    ops.optimizer_step('adam', [(w, t(4), m, v, 0.0)], 0.5, step=1, beta1=0.5, beta2=0.0, epsilon=0.0)
    assert m.tolist() == [6.0] and v.tolist() == [16.0] and w.tolist() == [6.5]                     # lr_t = 1; w = 8 - 6 / 4


@pytest.mark.parametrize('rule', orf.RULES)
def test_three_steps_across_the_schedule_s_rate_change(ops, dev, rule):
    """Steps 89999, 90000, 90001 of the reference's schedule (0.001, 0.001, 0.0001) with its hyper-parameters (momentum 0.9, decay 0.0005 on
    the decayed tensors; epsilon 1.0, the value slim's scripts use), and three steps of the large ones: still the emulation bit for bit."""
    from ron_tensorflow_amd import optim
    lrs = tuple(optim.learning_rate(s) for s in (89999, 90000, 90001))
    assert lrs == (float(np.float32(0.001)),) * 2 + (float(np.float32(0.001 * 0.1)),)
    counts = [9, 4, orf.UNIT + 3]
    case = oc.gauss_case(rule, counts, [0.0005, 0.0, 0.0005], steps=3, lrs=lrs, hyper=dict(orf.HYPER, epsilon=1.0), first_step=90000)
    _assert_is_emulation('%s, the schedule' % rule, _device_run(ops, dev, case), case)
    case = _gauss(rule, tuple(counts), (oc.BOLD_WD, 0.0, oc.BOLD_WD), steps=3)
    _assert_is_emulation('%s, three large steps' % rule, _device_run(ops, dev, case), case)


@pytest.mark.parametrize('first_step', [1, 2, 100000, 10 ** 9])
def test_adam_bias_correction(ops, dev, first_step):
    """Step 1 (lr_t = lr sqrt(1 - beta2) / (1 - beta1)), a large step (both powers gone: lr_t = lr), with TensorFlow's default betas."""
    case = oc.gauss_case('adam', [33, 6], [0.0, oc.BOLD_WD], steps=2, hyper=dict(orf.HYPER, epsilon=2.0 ** -20), first_step=first_step)
    assert float(orf.adam_lr(orf.Arith('f32'), 0.125, 0.9, 0.999, 10 ** 9)) == 0.125 != float(orf.adam_lr(orf.Arith('f32'), 0.125, 0.9, 0.999, 1))
    _assert_is_emulation('adam from step %d' % first_step, _device_run(ops, dev, case), case)


# -------------------------------------------------------------------------------------------------------------------- the contract
def _tensors(dev, case):
    return [[torch.from_numpy(t[k] if k != 'g' else t['g'][0]).to(dev) for k in ('w', 'g', 's0', 's1')] for t in case['tensors']]


def _raw_step(dev, case, tens, reg, ws):
    """The C entry with caller-made reg_loss and workspace (either may be None)."""
    from ron_tensorflow_amd import _lib
    n = len(tens)
    table = (_lib.OptTensor * n)()
    for i, ((w, g, s0, s1), t) in enumerate(zip(tens, case['tensors'])):
        table[i] = _lib.OptTensor(w.data_ptr(), g.data_ptr(), s0.data_ptr(), s1.data_ptr(), w.numel(), t['wd'])
    h = case['hyper']
    cfg = _lib.OptCfg(_lib.OPT_RULES[case['rule']], h['momentum'], h['decay'], h['beta1'], h['beta2'], h['epsilon'])
    _lib.check(_lib.lib().ron_optimizer_step(C.byref(cfg), table, n, float(case['lrs'][0]), case['first_step'], _lib.ptr(reg), _lib.ptr(ws),
                                             0 if ws is None else int(ws.numel()), _lib.current_stream()))


@pytest.mark.parametrize('rule', ['momentum', 'adam'])
def test_workspace_and_reproducibility(ops, dev, rule):
    """reg_loss == NULL leaves a poisoned workspace untouched; with reg_loss a workspace of 0xFF bytes (NaN in every format), then the
    same buffer straight after a call of another list, changes nothing; two calls from the same state give the same bytes."""
    counts = (5, 2 * orf.UNIT + 7, 3, orf.UNIT)
    case = _gauss(rule, counts, tuple(oc.mixed_decay(4)))
    other = _gauss(rule, (orf.UNIT + 1,) * 7, (oc.BOLD_WD,) * 7)
    nbytes = ops.optimizer_workspace_bytes([orf.UNIT + 1] * 7)
    assert nbytes >= ops.optimizer_workspace_bytes(list(counts)) == 256
    results = []
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    for attempt in range(3):
        tens = _tensors(dev, case)
        reg = torch.full((), float('nan'), device=dev)
        _raw_step(dev, case, tens, reg, ws)
        results.append([x.cpu().numpy().tobytes() for t in tens for x in t] + [reg.cpu().numpy().tobytes()])
        if attempt == 0:
            assert not bool((ws[:16] == 0xFF).all()), 'the workspace was not used: the test shows nothing'
            _raw_step(dev, other, _tensors(dev, other), reg.clone(), ws)          # the workspace now holds another list's values
    assert results[0] == results[1] == results[2]
    want = _emulated(_remember(case))[0]
    assert np.frombuffer(results[0][-1], np.float32)[0].view(np.uint32) == _bits(want['reg'])
    ws.fill_(0xFF)
    tens = _tensors(dev, case)
    _raw_step(dev, case, tens, None, ws)
    assert bool((ws == 0xFF).all()), 'reg_loss is NULL and the workspace was written'
    assert [x.cpu().numpy().tobytes() for t in tens for x in t] == results[0][:-1]
    tens = _tensors(dev, case)
    _raw_step(dev, case, tens, None, None)
    assert [x.cpu().numpy().tobytes() for t in tens for x in t] == results[0][:-1]


def _late_setup(ops, dev):
    counts = (orf.UNIT + 9, 7, 64)
    given, poison = _gauss('momentum', counts, tuple(oc.mixed_decay(3))), oc.gauss_case('momentum', list(counts), oc.mixed_decay(3), seed=9)
    flat = lambda case: [x for t in _tensors(dev, case) for x in t[:3]]          # w, g, m per tensor
    x, xp = flat(given), flat(poison)

    def entry(b):
        table, outs = [], []
        for i in range(len(counts)):
            w, m = b[3 * i].clone(), b[3 * i + 2].clone()          # the update is in place: on copies, made on the caller's stream
            table.append((w, b[3 * i + 1], m, None, given['tensors'][i]['wd']))
            outs += [w, m]
        reg = ops.optimizer_step('momentum', table, 0.125, want_reg_loss=True, **given['hyper'])
        return outs + [reg]
    clones = lambda ts: [t.clone() for t in ts]
    expected = clones(entry(x))
    bufs = clones(xp)
    poisoned = clones(entry(bufs))
    torch.cuda.synchronize()
    assert not su.same_bytes(expected, poisoned)

    def fill():
        for b, src in zip(bufs, x):
            b.copy_(src, non_blocking=True)
    return entry, x, bufs, expected, fill, clones


def test_stream_contract_late_inputs(ops, dev, side):
    """On a stalled side stream, with the real inputs copied into the buffers behind the stall: the call does not wait for the host
    and reads nothing early - the result has the default-stream result's bytes."""
    entry, x, bufs, expected, fill, clones = _late_setup(ops, dev)
    got = su.run_late(side, fill, lambda: entry(bufs), clones, label='optimizer_step')
    assert su.same_bytes(got, expected), 'the result on the stalled stream differs from the default-stream result'


def test_stream_contract_control_misdirected(ops, dev, side):
    """Positive control: the same late inputs with the call on the default stream must NOT give the expected result."""
    entry, x, bufs, expected, fill, clones = _late_setup(ops, dev)
    got = su.run_misdirected(side, fill, lambda: entry(bufs), clones)
    assert not su.same_bytes(got, expected), 'a call on the wrong stream went unnoticed: the harness cannot fail'
    assert su.same_bytes(clones(bufs), clones(x))


# --------------------------------------------------------------------------------------------------------------------- the chain
def test_reg_bbox_module_into_apply_gradients(ops, dev):
    """reg_bbox: conv3x3 (no bias, no activation) -> batch norm + ReLU -> conv3x3 + bias, 2 x 8 x 8, 64 -> 64 -> 24 channels, forward and
    backward with the explicit calls; then ONE Optimizer.apply_gradients (momentum) over {w0, gamma, beta, w1, b1}.  The result is the
    emulation applied to the gradients the device delivered, only the two `weights` decayed; the moving statistics are no variables of
    the update; state_dict / load_state_dict carry the slots."""
    from ron_tensorflow_amd import optim
    rs = np.random.RandomState(11)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    scope = 'ron_320_vgg/block7_box/reg_bbox/'
    host = {scope + 'Conv2d_0_3x3/weights': rs.randn(3, 3, 64, 64) * np.sqrt(2.0 / 576), scope + 'Conv2d_0_3x3/BatchNorm/gamma': 1.0 + 0.3 * rs.randn(64),
            scope + 'Conv2d_0_3x3/BatchNorm/beta': 0.2 * rs.randn(64), scope + 'Conv2d_0_3x3/BatchNorm/moving_mean': np.zeros(64),
            scope + 'Conv2d_0_3x3/BatchNorm/moving_variance': np.ones(64), scope + 'Conv2d_1_3x3/weights': rs.randn(3, 3, 64, 24) * np.sqrt(2.0 / 576),
            scope + 'Conv2d_1_3x3/biases': rs.randn(24) * 0.1}
    host = {k: v.astype(np.float32) for k, v in host.items()}
    var = {k: up(v) for k, v in host.items()}
    w0, gamma, beta, mm, mv, w1, b1 = var.values()
    x, g = up(rs.randn(2, 8, 8, 64)), up(rs.randn(2, 8, 8, 24))
    h = ops.conv2d_nhwc(x, host[scope + 'Conv2d_0_3x3/weights'], None, relu=False)
    y, mean, bvar = ops.batchnorm_train_nhwc(h, gamma, beta, mm, mv, relu=True)
    ops.conv2d_nhwc(y, host[scope + 'Conv2d_1_3x3/weights'], host[scope + 'Conv2d_1_3x3/biases'], relu=False)
    dy, dw1, db1 = ops.conv2d_backward_nhwc(y, w1, g, None, relu=False)
    dh, dgamma, dbeta = ops.batchnorm_backward_nhwc(h, y, dy, gamma, mean, bvar, relu=True)
    _, dw0, _ = ops.conv2d_backward_nhwc(x, w0, dh, None, relu=False, need=('dw',))
    trained = [k for k in var if 'moving_' not in k]
    grads = dict(zip(trained, (dw0, dgamma, dbeta, dw1, db1)))
    moving = [mm.clone(), mv.clone()]
    opt = optim.configure_optimizer('momentum')(var, weight_decay=0.0005)
    assert list(opt.variables) == trained and all(len(s) == 1 and not bool(s[0].any()) for s in opt.slots.values())
    with pytest.raises(KeyError):
        opt.apply_gradients({k: v for k, v in grads.items() if not k.endswith('biases')}, 0)
    regs = [opt.apply_gradients(grads, step, want_reg_loss=True) for step in (90000, 90001)]          # the same gradients, the rate drops
    assert opt.apply_gradients(grads, 90002) is None
    case = dict(rule='momentum', hyper=dict(orf.HYPER), first_step=1, exact=False, lrs=[np.float32(optim.learning_rate(s)) for s in (90000, 90001, 90002)],
                tensors=[dict(w=host[k].reshape(-1), g=[grads[k].cpu().numpy().reshape(-1)] * 3, s0=np.zeros(host[k].size, np.float32),
                              s1=np.zeros(host[k].size, np.float32), wd=0.0005 if k in (trained[0], trained[3]) else 0.0) for k in trained])
    want = orf.emulate32(case)
    for i, k in enumerate(trained):
        assert np.array_equal(_bits(var[k].cpu().numpy().reshape(-1)), _bits(want[2]['w'][i])), '%s is not the emulation of three steps' % k
        assert np.array_equal(_bits(opt.slots[k][0].cpu().numpy().reshape(-1)), _bits(want[2]['s0'][i])), 'the momentum of %s' % k
    assert [_bits(np.float32(r.item())) for r in regs] == [_bits(want[0]['reg']), _bits(want[1]['reg'])] and min(r.item() for r in regs) > 0
    assert su.same_bytes([mm, mv], moving), 'the moving statistics were updated by the optimizer'
    # an undecayed variable moved by its momentum alone
    k = trained[4]
    assert np.array_equal(want[0]['s0'][4], grads[k].cpu().numpy()) and np.array_equal(want[0]['w'][4], host[k] - np.float32(0.001) * grads[k].cpu().numpy())
    state = opt.state_dict()
    assert sorted(state['slots']) == sorted(k + '/momentum' for k in trained)
    again = optim.configure_optimizer('momentum')(var)
    again.load_state_dict(state)
    assert su.same_bytes([s[0] for s in again.slots.values()], [s[0] for s in opt.slots.values()])
    with pytest.raises(ValueError):
        optim.configure_optimizer('sgd')(var).load_state_dict(state)
