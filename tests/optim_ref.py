"""References of the training update (ron_optimizer_step, include/ron_hip.h): TensorFlow 1.x's dense apply kernels for sgd, momentum,
rmsprop and adam with slim's L2 regulariser folded into the gradient, and the regulariser's value.

The rules are written ONCE (`apply_rule`), over whatever arithmetic its arguments bring:

  float64 arrays     the definition (`run(case, 'f64')`);
  float32 arrays     numpy rounds once per operation, as the kernel does (compiled without contraction, correctly rounded division and
                     square root), in exactly the order of the header: the emulation, expected to EQUAL the device bit for bit;
  Bounded            a float64 value with a first-order bound on what any fp32 evaluation in that order can be away from it: every
                     operation passes its operands' bounds through its partial derivatives and adds ONE fp32 ulp (2^-23, relative)
                     of its own result - twice the half ulp a correctly rounded operation can cost, no fitted constant, no excluded
                     element.  Constants formed on the host in fp32 (1 - decay, lr_t) are operations like any other.

reg_loss is emulated apart (`reg_emulate32`): its value depends on the kernel's summation tree, which follows from the numbers
ron_optimizer_plan reports (UNIT elements per work unit; a lane of 256 adds its elements in order, 64 lanes meet in a shuffle tree,
4 waves as (0 + 1) + (2 + 3); one workgroup adds the units' values, thread t those of units t, t + 256, ..., then the same tree)."""
import math

import numpy as np

ULP = 2.0 ** -23
UNIT = 4096            # elements per work unit   } mirrored from csrc/optimizer.hip; tests/test_optim_cpu.py holds them against
ENTRIES = 64           # table entries per launch } ron_optimizer_plan
THREADS = 256
RULES = ('sgd', 'momentum', 'rmsprop', 'adam')
SLOTS = {'sgd': 0, 'momentum': 1, 'rmsprop': 2, 'adam': 2}
HYPER = dict(momentum=0.9, decay=0.9, beta1=0.9, beta2=0.999, epsilon=0.0)


# ------------------------------------------------------------------------------------------------------------------------ geometry
def geometry(counts):
    """What ron_optimizer_plan and ron_optimizer_workspace_bytes answer for a list of counts, and each tensor's units."""
    units = [(int(c) + UNIT - 1) // UNIT for c in counts]
    total = sum(units)
    return dict(launches=(len(counts) + ENTRIES - 1) // ENTRIES, units=total, entries=ENTRIES, unit=UNIT, per_tensor=units,
                workspace_bytes=(total * 4 + 255) // 256 * 256)


# ------------------------------------------------------------------------------------------------------------- bounded arithmetic
class Bounded(object):
    """v: float64 value; e: bound on |fp32 evaluation - v|, to first order."""
    __array_priority__ = 1000

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, Bounded) else Bounded(x)

    @staticmethod
    def _rounded(v, e):
        return Bounded(v, e + ULP * np.abs(v))

    def __add__(self, o):
        o = Bounded.of(o)
        return Bounded._rounded(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = Bounded.of(o)
        return Bounded._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Bounded.of(o) - self

    def __mul__(self, o):
        o = Bounded.of(o)
        return Bounded._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Bounded.of(o)
        return Bounded._rounded(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def sqrt(self):
        root = np.sqrt(self.v)
        # d sqrt = d / (2 sqrt(v)); at v = 0 an exact zero stays exact, anything else is unbounded to first order
        slope = np.where(self.e == 0, 0.0, self.e / np.where(root > 0, 2 * root, 0.0))
        return Bounded._rounded(root, slope)


def sqrt(x):
    return x.sqrt() if isinstance(x, Bounded) else np.sqrt(x)


class Arith(object):
    """How one mode forms constants and arrays."""
    def __init__(self, mode):
        assert mode in ('f64', 'f32', 'bound')
        self.mode = mode

    def const(self, x):          # x: a value the caller holds in fp32
        x = np.float32(x)
        return x if self.mode == 'f32' else (Bounded(np.float64(x)) if self.mode == 'bound' else np.float64(x))

    def array(self, a):
        a = np.asarray(a, np.float32)
        return a.copy() if self.mode == 'f32' else (Bounded(a.astype(np.float64)) if self.mode == 'bound' else a.astype(np.float64))

    def host_round(self, x):          # a double the host rounds to fp32 once
        if self.mode == 'f32':
            return np.float32(x)
        return Bounded(np.float64(x), ULP * abs(x)) if self.mode == 'bound' else np.float64(x)


def value(x):
    return x.v if isinstance(x, Bounded) else x


# --------------------------------------------------------------------------------------------------------------------- the rules
def adam_lr(ar, lr, beta1, beta2, step):
    """lr_t = lr sqrt(1 - beta2^step) / (1 - beta1^step): in double on the host from the fp32 values, rounded to fp32 once."""
    lr, b1, b2 = (float(np.float32(x)) for x in (lr, beta1, beta2))
    return ar.host_round(lr * math.sqrt(1.0 - b2 ** float(step)) / (1.0 - b1 ** float(step)))


def apply_rule(ar, rule, h, w, g, s0, s1, wd, lr, step, mutant=None):
    """One tensor, one step: (w, s0, s1) after the update.  `wd`: this tensor's weight_decay; `lr`: the fp32 rate of this step."""
    c = ar.const
    lr_c = c(lr)
    w_in = w
    with np.errstate(all='ignore'):
        if np.float32(wd) != 0 or mutant == 'zero_times_w':
            if mutant != 'decoupled':
                g = g + c(wd) * w
        if rule == 'sgd':
            w = w - lr_c * g
        elif rule == 'momentum':
            if mutant == 'dampening':
                s0 = c(h['momentum']) * s0 + (c(1) - c(h['momentum'])) * g
                w = w - lr_c * s0
            elif mutant == 'lr_in_accumulator':
                s0 = c(h['momentum']) * s0 + lr_c * g
                w = w - s0
            elif mutant == 'nesterov':
                s0 = c(h['momentum']) * s0 + g
                w = w - (lr_c * g + (lr_c * c(h['momentum'])) * s0)
            else:
                s0 = c(h['momentum']) * s0 + g
                w = w - lr_c * s0
        elif rule == 'rmsprop':
            omr = c(1) - c(h['decay'])
            s0 = s0 + omr * (g * g - s0)
            if mutant == 'rms_eps_outside':
                s1 = c(h['momentum']) * s1 + (lr_c * g) / (sqrt(s0) + c(h['epsilon']))
            else:
                s1 = c(h['momentum']) * s1 + (lr_c * g) / sqrt(s0 + c(h['epsilon']))
            w = w - s1
        else:
            assert rule == 'adam'
            k = {'adam_step_off_by_one': step - 1}.get(mutant, step)
            lr_t = lr_c if mutant == 'adam_no_bias_correction' else adam_lr(ar, lr, h['beta1'], h['beta2'], k)
            omb1, omb2 = c(1) - c(h['beta1']), c(1) - c(h['beta2'])
            s0 = s0 + omb1 * (g - s0)
            s1 = s1 + omb2 * (g * g - s1)
            if mutant == 'adam_eps_inside':
                w = w - (lr_t * s0) / sqrt(s1 + c(h['epsilon']))
            else:
                w = w - (lr_t * s0) / (sqrt(s1) + c(h['epsilon']))
        if mutant == 'decoupled' and np.float32(wd) != 0:
            w = w - (lr_c * c(wd)) * w_in
    return w, s0, s1


REG_OPS = 16 + 8 + 8 + 3          # a lane's additions, two trees, w * w, 0.5 * wd, the scaling (plus the final kernel's column)


def reg_value(ar, ws, wds, mutant=None, default_wd=0.0):
    """sum over tensors of (0.5 wd) sum(w^2) as a float64 (mode 'bound': with the bound of the kernel's tree, all terms being >= 0:
    every addition and product on a value's way costs one ulp of a partial sum that the total bounds)."""
    total = 0.0
    for w, wd in zip(ws, wds):
        wd = np.float32(wd)
        if wd == 0 and mutant == 'reg_over_undecayed':
            wd = np.float32(default_wd)
        if wd == 0:
            continue
        half = 1.0 if mutant == 'reg_no_half' else 0.5
        total += half * float(wd) * float(np.sum(np.square(value(w).astype(np.float64))))
    if ar.mode != 'bound':
        return np.float32(total) if ar.mode == 'f32' else total
    units = geometry([value(w).size for w in ws])['units']
    return Bounded(total, (REG_OPS + (units + THREADS - 1) // THREADS) * ULP * total)


def _tree(lanes):
    """[..., 256] float32 -> [...]: the shuffle tree of each wave (lane i += lane i + off, off = 32 .. 1), then (0 + 1) + (2 + 3)."""
    x = lanes.reshape(lanes.shape[:-1] + (4, 64))
    for off in (32, 16, 8, 4, 2, 1):
        x = x[..., :off] + x[..., off:2 * off]
    x = x[..., 0]
    return (x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])


def reg_emulate32(ws, wds):
    """reg_loss as the kernels add it, in float32: the units' values, then the final kernel's tree."""
    partial = []
    for w, wd in zip(ws, wds):
        w, wd = np.asarray(w, np.float32).reshape(-1), np.float32(wd)
        units = (w.size + UNIT - 1) // UNIT
        if wd == 0:
            partial.append(np.zeros(units, np.float32))          # written, never read for it
            continue
        padded = np.zeros(units * UNIT, np.float32)
        padded[:w.size] = w
        sq = (padded * padded).reshape(units, UNIT // (4 * THREADS), THREADS, 4)          # [unit, access, lane, element]
        acc = np.zeros((units, THREADS), np.float32)
        for v in range(sq.shape[1]):
            for e in range(4):
                acc = acc + sq[:, v, :, e]
        partial.append((np.float32(0.5) * wd) * _tree(acc))
    partial = np.concatenate(partial)
    rows = (partial.size + THREADS - 1) // THREADS
    padded = np.zeros(rows * THREADS, np.float32)
    padded[:partial.size] = partial
    acc = np.zeros(THREADS, np.float32)
    for row in padded.reshape(rows, THREADS):
        acc = acc + row
    return np.float32(_tree(acc))


# ---------------------------------------------------------------------------------------------------------------- a whole case
def dropped_mask(count, index, mutant):
    """Elements a geometry mutant leaves untouched in tensor `index` of `count` elements (None: none)."""
    keep = np.zeros(count, bool)
    if mutant == 'tail_dropped':
        keep[count - count % 4:] = True
    elif mutant == 'last_unit_dropped' and count > UNIT:
        keep[(count - 1) // UNIT * UNIT:] = True
    elif mutant == 'launch_boundary_skipped' and index == ENTRIES:
        keep[:] = True
    return keep if keep.any() else None


def run(case, mode, mutant=None):
    """Every step of a case: a list, per step, of dict(w, s0, s1: lists per tensor of what the arithmetic gives; reg).  A case is
    dict(rule, hyper, tensors=[dict(w, s0, s1, wd, g=[per step])], lrs=[fp32 rate per step], first_step (adam's step of step 0))."""
    ar, rule, h = Arith(mode), case['rule'], case['hyper']
    state = [[ar.array(t['w']), ar.array(t['s0']), ar.array(t['s1'])] for t in case['tensors']]
    wds = [t['wd'] for t in case['tensors']]
    out = []
    for k, lr in enumerate(case['lrs']):
        reg_before = reg_value(ar, [s[0] for s in state], wds, mutant, case.get('default_wd', 0.0))
        for i, t in enumerate(case['tensors']):
            wd = t['wd']
            if mutant == 'decay_on_undecayed' and np.float32(wd) == 0:
                wd = case.get('default_wd', 0.0)
            new = apply_rule(ar, rule, h, state[i][0], ar.array(t['g'][k]), state[i][1], state[i][2], wd, lr, case['first_step'] + k, mutant)
            keep = dropped_mask(np.asarray(t['w']).size, i, mutant)
            if keep is not None:
                new = [_where(keep, old, n) for old, n in zip(state[i], new)]
            state[i] = list(new)
        reg = reg_value(ar, [s[0] for s in state], wds, mutant, case.get('default_wd', 0.0)) if mutant == 'reg_from_updated' else reg_before
        out.append(dict(w=[s[0] for s in state], s0=[s[1] for s in state], s1=[s[2] for s in state], reg=reg))
    return out


def _where(keep, old, new):
    if isinstance(new, Bounded):
        old = Bounded.of(old)
        return Bounded(np.where(keep, old.v, new.v), np.where(keep, old.e, new.e))
    return np.where(keep, old, new)


def emulate32(case):
    """The float32 emulation of every step, reg_loss from the kernel's tree."""
    steps = run(case, 'f32')
    wds = [t['wd'] for t in case['tensors']]
    before = [np.asarray(t['w'], np.float32) for t in case['tensors']]
    for s in steps:
        s['reg'] = reg_emulate32(before, wds)
        before = s['w']
    return steps


def ratio(got, ref):
    """|got - ref.v| / ref.e per element; 0 where they are equal (infinities included), inf where they differ and the bound is 0."""
    got = np.asarray(got, np.float64)
    with np.errstate(all='ignore'):
        same = (got == ref.v) | (np.isnan(got) & np.isnan(ref.v))
        r = np.abs(got - ref.v) / ref.e
    r = np.where(same, 0.0, r)
    return np.where(np.isnan(r), np.inf, r)
