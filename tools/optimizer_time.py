#!/usr/bin/env python3
"""Time per call of ron_optimizer_step over the trainable variables of RON-320 (`reducedfc` and `full`: names and shapes from
RONNet.variables(), the moving statistics left out as tf_utils.get_variables_to_train leaves them out): momentum 0.9, weight_decay
0.0005 on the `weights`, with and without reg_loss, beside two yardsticks in one process.

The entry is called through ctypes with every argument built once (no Python wrapper, no allocation in the timed window); a window
is `--steps` calls between two HIP events on one stream and the median over `--repeats` windows is reported.

Yardsticks:
  copy_us   a device-to-device copy, in the same process, that moves the update's MINIMUM traffic of 20 bytes per parameter (w, g, m
            read, w, m written): it reads and writes 10 bytes per parameter each;
  torch     torch.optim.SGD(momentum=0.9, weight_decay per group) on the same tensors with foreach=True and, where this torch accepts
            the tensors, fused=True.

    python tools/optimizer_time.py --out profiles/optimizer
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ron_tensorflow_amd import _lib, optim  # noqa: E402

VARIANTS = ('reducedfc', 'full')
WEIGHT_DECAY, MOMENTUM, RATE = 0.0005, 0.9, 0.001


def trainable_list(variant):
    """[(tf_name, element count)] of the variables the reference trains, in the graph's order."""
    from ron_tensorflow_amd.nets.ron_vgg_320 import RONNet
    net = RONNet(variant=variant, max_batch=1, device='cuda:0')
    shapes = dict(net.variables())
    names = optim.trainable_names([name for name, _ in net.variables()])
    net.close()
    out = []
    for name in names:
        count = 1
        for s in shapes[name]:
            count *= int(s)
        out.append((name, count))
    return out


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps            # microseconds per call


def median_of(fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window(fn, steps) for _ in range(repeats))


def guarded(what, fn):
    try:
        return round(fn(), 2)
    except Exception as e:          # noqa: BLE001 - whatever torch refuses is reported, not fatal
        print('torch %s failed: %s' % (what, str(e).splitlines()[0]), flush=True)
        return 'n/a'


def ratio(a, b):
    return 'n/a' if 'n/a' in (a, b) else round(a / b, 2)


def row_of(a, dev, lib, variant):
    listed = trainable_list(variant)
    n, params = len(listed), sum(c for _, c in listed)
    g = torch.Generator(device=dev).manual_seed(1)
    var = [torch.randn((c,), device=dev, generator=g) * 0.05 for _, c in listed]
    grad = [torch.randn((c,), device=dev, generator=g) * 0.01 for _, c in listed]
    slot = [torch.zeros((c,), device=dev) for _, c in listed]
    table = (_lib.OptTensor * n)()
    for i, (name, c) in enumerate(listed):
        table[i] = _lib.OptTensor(var[i].data_ptr(), grad[i].data_ptr(), slot[i].data_ptr(), None, c, optim.decay_of(name, WEIGHT_DECAY))
    plan = (C.c_int64 * 4)()
    _lib.check(lib.ron_optimizer_plan(table, n, plan))
    nbytes = lib.ron_optimizer_workspace_bytes(table, n)
    assert nbytes > 0, lib.ron_last_error().decode()
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    reg = torch.empty((), device=dev)
    cfg = _lib.OptCfg(_lib.OPT_RULES['momentum'], MOMENTUM, 0.9, 0.9, 0.999, 0.0)
    stream = _lib.current_stream()
    P = _lib.ptr

    def step():
        _lib.check(lib.ron_optimizer_step(C.byref(cfg), table, n, RATE, 1, None, None, 0, stream))

    def step_reg():
        _lib.check(lib.ron_optimizer_step(C.byref(cfg), table, n, RATE, 1, P(reg), P(ws), nbytes, stream))
    t_step = median_of(step, a.steps, a.warmup, a.repeats)
    t_reg = median_of(step_reg, a.steps, a.warmup, a.repeats)
    traffic = 20 * params
    src = torch.empty((traffic // 2,), dtype=torch.uint8, device=dev).zero_()
    dst = torch.empty_like(src)
    t_copy = median_of(lambda: dst.copy_(src, non_blocking=True), a.steps, a.warmup, a.repeats)
    del src, dst
    t_torch = {}
    for form in ('foreach', 'fused'):
        def torch_time(form=form):
            ps = [v.clone().requires_grad_(True) for v in var]
            for p, gr in zip(ps, grad):
                p.grad = gr
            groups = [dict(params=[p], weight_decay=optim.decay_of(name, WEIGHT_DECAY)) for p, (name, _) in zip(ps, listed)]
            # two groups (decayed / not), as a user would write it: one group per variable would undo the batching
            groups = [dict(params=[p for p, gp in zip(ps, groups) if (gp['weight_decay'] != 0) == flag], weight_decay=WEIGHT_DECAY if flag else 0.0)
                      for flag in (True, False)]
            opt = torch.optim.SGD(groups, lr=RATE, momentum=MOMENTUM, **{form: True})
            return median_of(opt.step, a.steps, a.warmup, a.repeats)
        t_torch[form] = 'n/a' if a.no_torch else guarded('SGD(%s=True)' % form, torch_time)
    row = dict(op='optimizer', variant=variant, rule='momentum', variables=n, parameters=params, launches=int(plan[0]), units=int(plan[1]),
               entries=int(plan[2]), unit=int(plan[3]), steps=a.steps, repeats=a.repeats, traffic_mb=round(traffic / 2 ** 20, 1),
               step_us=round(t_step, 2), step_reg_us=round(t_reg, 2), copy_us=round(t_copy, 2), gb_s=round(traffic / t_step / 1e3, 1),
               step_over_copy=round(t_step / t_copy, 2), step_reg_over_copy=round(t_reg / t_copy, 2), torch_foreach_us=t_torch['foreach'],
               torch_fused_us=t_torch['fused'], step_over_foreach=ratio(round(t_step, 2), t_torch['foreach']),
               step_over_fused=ratio(round(t_step, 2), t_torch['fused']))
    print(json.dumps(row), flush=True)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--variants', default=','.join(VARIANTS))
    ap.add_argument('--out', default=None, help='directory for optimizer.json and README.md')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    rows = []
    for variant in a.variants.split(','):
        rows.append(row_of(a, dev, _lib.lib(), variant))
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'optimizer.json'), 'w') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write('# profiles/optimizer - ron_optimizer_step\n\n'
                     '    python tools/optimizer_time.py --out profiles/optimizer\n\n'
                     'One MI355X, one process: the trainable variables of RON-320 (names and shapes from `RONNet.variables()`), momentum %g,\n'
                     'weight_decay %g on the `weights`.  The entry is called through ctypes with every argument built once; a window is %d calls\n'
                     'between two HIP events on one stream after %d warm-up calls, the median of %d windows is reported, in microseconds.\n'
                     'DESIGN.md section 4.10 reads the table.\n\n'
                     '`copy`: a device-to-device copy in the same process that reads and writes half of the minimum traffic of 20 bytes per\n'
                     'parameter each; GB/s = that traffic / time of the step without reg_loss.  `foreach` / `fused`: `torch.optim.SGD(momentum,\n'
                     'weight_decay)` on the same tensors in two parameter groups (decayed / not).\n\n' % (MOMENTUM, WEIGHT_DECAY, a.steps, a.warmup, a.repeats))
            fh.write('| list | variables | parameters | launches | units | step us | with reg_loss us | copy us | GB/s | step / copy | with reg / copy | foreach us | fused us |\n')
            fh.write('|' + '---|' * 13 + '\n')
            for r in rows:
                fh.write('| %s | %d | %d | %d | %d | %s | %s | %s | %s | %s | %s | %s | %s |\n' % (
                    r['variant'], r['variables'], r['parameters'], r['launches'], r['units'], r['step_us'], r['step_reg_us'], r['copy_us'], r['gb_s'],
                    r['step_over_copy'], r['step_reg_over_copy'], r['torch_foreach_us'], r['torch_fused_us']))
            fh.write('\nNot measured: hardware counters of the new kernels (fetch / write sizes, cache hit rates, occupancy).\n')


if __name__ == '__main__':
    main()
