#!/usr/bin/env python3
"""Time per call of ron_batchnorm_train_nhwc and ron_batchnorm_backward_nhwc at the four RON scales (40^2, 20^2, 10^2, 5^2) with 512
and 1024 channels, beside two yardsticks in one process: batch 32, bf16, ReLU on, the moving statistics updated.

The entries are called through ctypes with every argument built once (no Python wrapper, no allocation in the timed window); a
window is `--steps` calls between two HIP events on one stream and the median over `--repeats` windows is reported.

Yardsticks:
  copy_us   a device-to-device copy, in the same process, that moves the operator's MINIMUM traffic: it reads and writes traffic / 2
            bytes each.  Forward: x read for the statistics, x read again, y written = 3 tensors.  Backward: x, dy and y read twice,
            dx written = 7 tensors.  The copy, not a constant, is the yardstick for "bandwidth bound": both rates are traffic / time.
  torch_us  torch.nn.functional.batch_norm(training=True) then relu on bf16 channels_last tensors: the forward (batch_norm + relu), and
            torch.autograd.grad of it for input, weight and bias.

    python tools/batchnorm_time.py --out profiles/batchnorm
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

from ron_tensorflow_amd import _lib  # noqa: E402

SHAPES = [(hw, c) for hw in (40, 20, 10, 5) for c in (512, 1024)]


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
    except Exception as e:          # noqa: BLE001 - whatever torch / MIOpen refuses is reported, not fatal
        print('torch %s failed: %s' % (what, str(e).splitlines()[0]), flush=True)
        return 'n/a'


def ratio(a, b):
    return 'n/a' if 'n/a' in (a, b) else round(a / b, 2)


def copy_us(a, dev, traffic):
    src = torch.empty((traffic // 2,), dtype=torch.uint8, device=dev).zero_()
    dst = torch.empty_like(src)
    t = median_of(lambda: dst.copy_(src, non_blocking=True), a.steps, a.warmup, a.repeats)
    del src, dst
    return t


def rows_of(a, dev, lib):
    rows = []
    n = a.batch
    for hw, c in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn((n, hw, hw, c), device=dev, generator=g) * 1.5 + 0.5
        dy = torch.randn((n, hw, hw, c), device=dev, generator=g)
        gamma, beta = torch.rand((c,), device=dev, generator=g) + 0.5, torch.randn((c,), device=dev, generator=g) * 0.2
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, var, dgamma, dbeta = (torch.empty((c,), device=dev) for _ in range(4))
        mm, mv = torch.zeros((c,), device=dev), torch.ones((c,), device=dev)
        d = _lib.BnDesc(n, hw, hw, c, _lib.DTYPES[a.dtype], 1, 1e-5, 0.997)
        nbytes = lib.ron_batchnorm_workspace_bytes(C.byref(d))
        assert nbytes > 0, lib.ron_last_error().decode()
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        stream = _lib.current_stream()
        P = _lib.ptr

        def fwd():
            _lib.check(lib.ron_batchnorm_train_nhwc(C.byref(d), P(x), P(gamma), P(beta), P(y), P(mean), P(var), P(mm), P(mv), P(ws), nbytes, stream))

        def bwd():
            _lib.check(lib.ron_batchnorm_backward_nhwc(C.byref(d), P(x), P(y), P(dy), P(gamma), P(mean), P(var), P(dx), P(dgamma), P(dbeta), P(ws),
                                                       nbytes, stream))
        t_f = median_of(fwd, a.steps, a.warmup, a.repeats)
        t_b = median_of(bwd, a.steps, a.warmup, a.repeats)
        tensor = 4 * x.numel()
        c_f, c_b = copy_us(a, dev, 3 * tensor), copy_us(a, dev, 7 * tensor)
        tt_f = tt_b = 'n/a'
        if not a.no_torch:
            xt = x.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            dyt = dy.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            wt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
            rm, rv = torch.zeros((c,), device=dev), torch.ones((c,), device=dev)

            def torch_fwd():
                return torch.relu(torch.nn.functional.batch_norm(xt, rm, rv, wt, bt, training=True, momentum=0.003, eps=1e-5))
            with torch.no_grad():
                tt_f = guarded('batch_norm forward', lambda: median_of(torch_fwd, a.steps, a.warmup, a.repeats))

            def torch_bwd():
                out = torch_fwd()
                return median_of(lambda: torch.autograd.grad(out, (xt, wt, bt), dyt, retain_graph=True), a.steps, a.warmup, a.repeats)
            tt_b = guarded('batch_norm backward', torch_bwd)
            del xt, dyt
        row = dict(op='batchnorm', batch=n, h=hw, w=hw, c=c, dtype=a.dtype, steps=a.steps, repeats=a.repeats, tensor_mb=round(tensor / 2 ** 20, 1),
                   forward_us=round(t_f, 2), forward_copy_us=round(c_f, 2), forward_torch_us=tt_f, forward_gb_s=round(3 * tensor / t_f / 1e3, 1),
                   forward_over_copy=round(t_f / c_f, 2), forward_over_torch=ratio(round(t_f, 2), tt_f),
                   backward_us=round(t_b, 2), backward_copy_us=round(c_b, 2), backward_torch_us=tt_b, backward_gb_s=round(7 * tensor / t_b / 1e3, 1),
                   backward_over_copy=round(t_b / c_b, 2), backward_over_torch=ratio(round(t_b, 2), tt_b))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, dy, y, dx, ws
        torch.cuda.empty_cache()
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--out', default=None, help='directory for batchnorm_bs<batch>.json and README.md')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    rows = rows_of(a, dev, _lib.lib())
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'batchnorm_bs%d.json' % a.batch), 'w') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write('# profiles/batchnorm - ron_batchnorm_train_nhwc and ron_batchnorm_backward_nhwc\n\n'
                     '    python tools/batchnorm_time.py --out profiles/batchnorm\n\n'
                     'One MI355X, one process, batch %d, %s, ReLU on, moving statistics updated.  The entries are called through ctypes with every\n'
                     'argument built once; a window is %d calls between two HIP events on one stream after %d warm-up calls, the median of %d\n'
                     'windows is reported, in microseconds.  DESIGN.md section 4.9 reads the table.\n\n'
                     '`tensor`: one fp32 [n,h,w,c] tensor in MiB.  `copy`: a device-to-device copy in the same process that reads and writes half of\n'
                     'the operator\'s minimum traffic each (forward 3 tensors: x twice, y; backward 7: x, dy, y twice, dx); GB/s = that traffic /\n'
                     'time.  `torch`: `F.batch_norm(training=True)` + `relu` on bf16 channels_last tensors, forward, and `torch.autograd.grad` of it\n'
                     'for input, weight and bias.\n\n' % (a.batch, a.dtype, a.steps, a.warmup, a.repeats))
            fh.write('| shape | tensor MiB | fwd us | copy us | torch us | fwd GB/s | fwd / copy | fwd / torch | bwd us | copy us | torch us | bwd GB/s | bwd / copy | bwd / torch |\n')
            fh.write('|' + '---|' * 14 + '\n')
            for r in rows:
                fh.write('| %dx%dx%d | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |\n' % (
                    r['h'], r['w'], r['c'], r['tensor_mb'], r['forward_us'], r['forward_copy_us'], r['forward_torch_us'], r['forward_gb_s'],
                    r['forward_over_copy'], r['forward_over_torch'], r['backward_us'], r['backward_copy_us'], r['backward_torch_us'],
                    r['backward_gb_s'], r['backward_over_copy'], r['backward_over_torch']))
            fh.write('\nNot measured: hardware counters of the new kernels (fetch / write sizes, cache hit rates).\n')


if __name__ == '__main__':
    main()
