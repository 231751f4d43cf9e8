"""The tail of the reference's training step (ron_net.py:354-381) on the GPU: the piecewise learning rate, configure_optimizer and
apply_gradients, the latter as ONE ron_optimizer_step over all trainable variables (include/ron_hip.h).

    opt = configure_optimizer('momentum')(variables)            # variables: ordered {tf_name: float32 GPU tensor}, updated in place
    reg = opt.apply_gradients(grads, global_step, want_reg_loss=True)

Only the four rules with a dense TensorFlow 1.x kernel this library implements exist; there is no fall-back to torch.optim."""
import collections
import functools

import numpy as np
import torch

from . import _lib, ops

_SLOT_NAMES = {'sgd': (), 'momentum': ('momentum',), 'rmsprop': ('rms', 'momentum'), 'adam': ('m', 'v')}
_NOT_BUILT = ('adadelta', 'adagrad', 'ftrl')


def learning_rate(global_step, base=0.001, end=0.00001, boundaries=(90000, 115000), factors=(1., 0.1, 0.001)):
    """The schedule of ron_net.py:354-356 as a Python float holding an fp32 value: tf.train.piecewise_constant over `boundaries` (the
    first value holds while global_step <= boundaries[0]) of base * factor, formed in Python floats and rounded to fp32, then the
    maximum of that and `end`."""
    assert len(factors) == len(boundaries) + 1 and list(boundaries) == sorted(boundaries)
    values = [np.float32(base * f) for f in factors]
    index = sum(1 for b in boundaries if int(global_step) > b)
    return float(max(values[index], np.float32(end)))


def trainable_names(names, trainable_scopes=None):
    """tf_utils.get_variables_to_train on a list of variable names: slim never makes .../moving_mean and .../moving_variance
    trainable; `trainable_scopes` is a comma-separated list of prefixes (None: everything trainable), and, as there, the result is
    ordered by scope and a variable under two of the scopes is listed once per scope (which the update then refuses)."""
    names = [n for n in names if not (n.endswith('/moving_mean') or n.endswith('/moving_variance'))]
    if trainable_scopes is None:
        return names
    scopes = [s.strip() for s in trainable_scopes.split(',')]
    return [n for s in scopes for n in names if n.startswith(s)]


def decay_of(name, weight_decay):
    """ron_arg_scope puts l2_regularizer(weight_decay) on the `weights` of conv2d / conv2d_transpose only: biases, BatchNorm's and
    L2Normalization's gamma and beta get none."""
    return float(weight_decay) if name.endswith('/weights') else 0.0


class Optimizer(object):
    """One update rule over an ordered dict of tf_name -> float32 GPU tensor (updated in place).  Created by configure_optimizer."""

    def __init__(self, variables, weight_decay=0.0005, trainable_scopes=None, rule='momentum', momentum=0.9, decay=0.9, beta1=0.9,
                 beta2=0.999, epsilon=0.0, learning_rate_fn=learning_rate):
        if rule not in _lib.OPT_RULES:
            raise ValueError('Optimizer [%s] was not recognized' % rule)
        self.rule, self.weight_decay, self.learning_rate_fn = rule, float(weight_decay), learning_rate_fn
        self.hyper = dict(momentum=float(momentum), decay=float(decay), beta1=float(beta1), beta2=float(beta2), epsilon=float(epsilon))
        self.variables = collections.OrderedDict()
        for name in trainable_names(list(variables), trainable_scopes):
            v = variables[name]
            assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous(), '%s must be a contiguous float32 GPU tensor' % name
            self.variables[name] = v
        if not self.variables:
            raise ValueError('no variable to train (trainable_scopes=%r)' % (trainable_scopes,))
        # TensorFlow's initial slot values: zeros, RMSProp's mean square ones
        self.slots = collections.OrderedDict(
            (name, tuple((torch.ones_like if (rule, s) == ('rmsprop', 'rms') else torch.zeros_like)(v) for s in _SLOT_NAMES[rule]))
            for name, v in self.variables.items())

    def apply_gradients(self, grads, global_step, learning_rate=None, want_reg_loss=False):
        """ONE ron_optimizer_step on the current stream over every trainable variable.  `grads`: {tf_name: float32 GPU tensor shaped like
        the variable} (a missing name is an error; names that are not trained are ignored).  The rate is learning_rate_fn(global_step)
        unless given; Adam's step is global_step + 1.  Returns the regularisation loss (a GPU scalar: sum (weight_decay / 2) sum(w^2)
        over the decayed variables BEFORE the update) when want_reg_loss, else None."""
        missing = [name for name in self.variables if name not in grads]
        if missing:
            raise KeyError('apply_gradients: no gradient for %s' % ', '.join(missing[:4]) + (' ...' if len(missing) > 4 else ''))
        lr = self.learning_rate_fn(global_step) if learning_rate is None else learning_rate
        table = []
        for name, v in self.variables.items():
            g = grads[name]
            assert g.shape == v.shape, '%s: the gradient is %s, the variable %s' % (name, tuple(g.shape), tuple(v.shape))
            s = self.slots[name] + (None, None)
            table.append((v, g.contiguous(), s[0], s[1], decay_of(name, self.weight_decay)))
        return ops.optimizer_step(self.rule, table, lr, step=int(global_step) + 1, want_reg_loss=want_reg_loss, **self.hyper)

    def state_dict(self):
        """{'rule': ..., 'slots': {tf_name/slot_name: tensor (a copy)}}: TensorFlow's slot variables by their names."""
        return dict(rule=self.rule, slots=collections.OrderedDict(
            ('%s/%s' % (name, s), t.clone()) for name, ts in self.slots.items() for s, t in zip(_SLOT_NAMES[self.rule], ts)))

    def load_state_dict(self, state):
        if state['rule'] != self.rule:
            raise ValueError('the state is of rule %r, this optimizer of %r' % (state['rule'], self.rule))
        want = ['%s/%s' % (name, s) for name in self.slots for s in _SLOT_NAMES[self.rule]]
        if sorted(want) != sorted(state['slots']):
            raise KeyError('the state holds other slots than this optimizer: %s' % sorted(set(want) ^ set(state['slots']))[:4])
        for name, ts in self.slots.items():
            for s, t in zip(_SLOT_NAMES[self.rule], ts):
                t.copy_(state['slots']['%s/%s' % (name, s)])


def configure_optimizer(name, momentum=0.9, rmsprop_momentum=0.9, rmsprop_decay=0.9, adam_beta1=0.9, adam_beta2=0.999, opt_epsilon=None):
    """tf_utils.configure_optimizer (tf_utils.py:126-171): returns the constructor Optimizer(variables, weight_decay=0.0005,
    trainable_scopes=None) of the named rule.  The reference's drivers define no opt_epsilon flag, so 'rmsprop' and 'adam' need it
    explicitly; 'adadelta', 'adagrad' and 'ftrl' have no kernel here."""
    if name in _NOT_BUILT:
        raise NotImplementedError('optimizer %r is not built: sgd, momentum, rmsprop and adam are' % name)
    if name not in _lib.OPT_RULES:
        raise ValueError('Optimizer [%s] was not recognized' % name)
    if name in ('rmsprop', 'adam') and opt_epsilon is None:
        raise ValueError('optimizer %r needs opt_epsilon (the reference defines no default)' % name)
    hyper = {'sgd': {}, 'momentum': dict(momentum=momentum),
             'rmsprop': dict(momentum=rmsprop_momentum, decay=rmsprop_decay, epsilon=opt_epsilon),
             'adam': dict(beta1=adam_beta1, beta2=adam_beta2, epsilon=opt_epsilon)}[name]
    return functools.partial(Optimizer, rule=name, **hyper)
