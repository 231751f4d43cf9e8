#!/usr/bin/env python3
"""Time per call of ron_maxpool2x2_backward_nhwc at the five pool shapes of RON-320 and of ron_conv2d_k2s2_backward_nhwc at the 2x2
stride-2 operators of the reverse connections, beside torch's own backward of the same operators, in one process: batch 32, bf16.

The entries are called through ctypes with every argument built once (no Python wrapper, no allocation in the timed window); a
window is `--steps` calls between two HIP events on one stream and the median over `--repeats` windows is reported.

Yardsticks:
  pool   torch_us  torch.autograd.grad of torch.nn.functional.max_pool2d(ceil_mode=True) on fp32 channels_last tensors (the same
                   memory layout and element type as the entry's);
         copy_us   a device-to-device copy, in the same process, that moves the bytes the entry moves: it reads and writes
                   (x + dy + dx) / 2 bytes each, so read + written = x + dy + dx.  The copy, not a constant, is the yardstick for
                   "bandwidth bound": both rates are traffic / time.
  k2s2   torch_*   torch.autograd.grad of conv2d(stride=2) / conv_transpose2d(stride=2) on bf16 channels_last tensors, for the
                   weight alone and for input + weight ("n/a" when torch cannot run the shape).

    python tools/op_backward_time.py --out profiles/op_backward
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ron_tensorflow_amd import _lib  # noqa: E402

# name, h = w, c
POOLS = [('pool1', 320, 64), ('pool2', 160, 128), ('pool3', 80, 256), ('pool4', 40, 512), ('pool5', 20, 512)]
# name, h = w of the input x, cin, cout, transpose
K2S2 = [('block7_reverse_conv_left', 10, 1024, 512, 0), ('block7_reverse_conv_left (full)', 10, 4096, 512, 0),
        ('block6_deconv_right', 5, 512, 512, 1), ('block5_deconv_right', 10, 512, 512, 1), ('block4_deconv_right', 20, 512, 512, 1)]


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


def pool_rows(a, dev, lib):
    rows = []
    n = a.batch
    for name, hw, c in POOLS:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.relu(torch.randn((n, hw, hw, c), device=dev, generator=g))
        dy = torch.randn((n, (hw + 1) // 2, (hw + 1) // 2, c), device=dev, generator=g)
        dx = torch.empty_like(x)
        stream = _lib.current_stream()
        P = _lib.ptr
        t_us = median_of(lambda: _lib.check(lib.ron_maxpool2x2_backward_nhwc(P(x), P(dy), n, hw, hw, c, _lib.DTYPES[a.dtype], P(dx), stream)),
                         a.steps, a.warmup, a.repeats)
        traffic = 4 * (x.numel() + dy.numel() + dx.numel())
        src = torch.empty((traffic // 2,), dtype=torch.uint8, device=dev).zero_()
        dst = torch.empty_like(src)
        t_copy = median_of(lambda: dst.copy_(src, non_blocking=True), a.steps, a.warmup, a.repeats)
        del src, dst

        def torch_pool():
            xt = x.permute(0, 3, 1, 2).requires_grad_(True)          # NHWC memory seen as a channels_last NCHW tensor: no copy
            dyt = dy.permute(0, 3, 1, 2)
            out = torch.nn.functional.max_pool2d(xt, 2, 2, ceil_mode=True)
            return median_of(lambda: torch.autograd.grad(out, (xt,), dyt, retain_graph=True), a.steps, a.warmup, a.repeats)
        t_torch = 'n/a' if a.no_torch else guarded('max_pool2d backward', torch_pool)
        row = dict(op='maxpool2x2_backward', shape=name, batch=n, h=hw, w=hw, c=c, dtype=a.dtype, steps=a.steps, repeats=a.repeats,
                   traffic_mb=round(traffic / 2 ** 20, 1), entry_us=round(t_us, 2), copy_us=round(t_copy, 2), torch_us=t_torch,
                   entry_gb_s=round(traffic / t_us / 1e3, 1), copy_gb_s=round(traffic / t_copy / 1e3, 1),
                   entry_over_copy=round(t_us / t_copy, 2), entry_over_torch=ratio(round(t_us, 2), t_torch))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, dy, dx
        torch.cuda.empty_cache()
    return rows


def k2s2_rows(a, dev, lib):
    rows = []
    n = a.batch
    for name, hw, cin, cout, tr in K2S2:
        g = torch.Generator(device=dev).manual_seed(1)
        ho = 2 * hw if tr else hw // 2
        x = torch.randn((n, hw, hw, cin), device=dev, generator=g)
        w = torch.randn((2, 2, cout, cin) if tr else (2, 2, cin, cout), device=dev, generator=g) * float(np.sqrt(2.0 / ((1 if tr else 4) * cin)))
        y = torch.relu(torch.randn((n, ho, ho, cout), device=dev, generator=g))
        dy = torch.randn((n, ho, ho, cout), device=dev, generator=g)
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty((cout,), device=dev)
        d = _lib.ConvDesc(n, hw, hw, cin, cout, 2, 2, 2, 1, 1, tr, _lib.DTYPES[a.dtype], -1, 0, 0, 0, -1, 0)
        nbytes = lib.ron_conv2d_k2s2_backward_workspace_bytes(C.byref(d))
        assert nbytes > 0, lib.ron_last_error().decode()
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        stream = _lib.current_stream()
        P = _lib.ptr

        def call(pdx, pdw, pdb):
            _lib.check(lib.ron_conv2d_k2s2_backward_nhwc(C.byref(d), P(x), P(w), P(y), P(dy), pdx, pdw, pdb, P(ws), nbytes, stream))
        t_dx = median_of(lambda: call(P(dx), None, None), a.steps, a.warmup, a.repeats)
        t_dw = median_of(lambda: call(None, P(dw), None), a.steps, a.warmup, a.repeats)
        t_all = median_of(lambda: call(P(dx), P(dw), P(db)), a.steps, a.warmup, a.repeats)
        t_tw = t_txw = 'n/a'
        if not a.no_torch:
            try:
                xt = x.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                wt = w.permute(3, 2, 0, 1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                dyt = dy.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
                out = (torch.nn.functional.conv_transpose2d if tr else torch.nn.functional.conv2d)(xt, wt, None, stride=2)
                t_tw = guarded('k2s2 dw', lambda: median_of(lambda: torch.autograd.grad(out, (wt,), dyt, retain_graph=True), a.steps, a.warmup, a.repeats))
                t_txw = guarded('k2s2 dx + dw', lambda: median_of(lambda: torch.autograd.grad(out, (xt, wt), dyt, retain_graph=True), a.steps, a.warmup, a.repeats))
            except Exception as e:          # noqa: BLE001
                print('torch k2s2 forward failed: %s' % str(e).splitlines()[0], flush=True)
        flops = 2.0 * n * hw * hw * cin * cout * (4 if tr else 1)
        row = dict(op='conv2d_k2s2_backward', shape=name, batch=n, h=hw, w=hw, cin=cin, cout=cout, transpose=tr, dtype=a.dtype, steps=a.steps,
                   repeats=a.repeats, workspace_mb=round(nbytes / 2 ** 20, 1), gflop_per_gradient=round(flops / 1e9, 2),
                   dx_only_us=round(t_dx, 2), dw_only_us=round(t_dw, 2), all_three_us=round(t_all, 2), torch_dw_us=t_tw, torch_dx_dw_us=t_txw,
                   dw_over_torch_dw=ratio(round(t_dw, 2), t_tw), all_over_torch_dx_dw=ratio(round(t_all, 2), t_txw))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, w, y, dy, dx, dw, db, ws
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
    ap.add_argument('--out', default=None, help='directory for op_backward_bs<batch>.json and README.md')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    pools = pool_rows(a, dev, lib)
    convs = k2s2_rows(a, dev, lib)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'op_backward_bs%d.json' % a.batch), 'w') as fh:
            for row in pools + convs:
                fh.write(json.dumps(row) + '\n')
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write('# profiles/op_backward - ron_maxpool2x2_backward_nhwc and ron_conv2d_k2s2_backward_nhwc\n\n'
                     '    python tools/op_backward_time.py --out profiles/op_backward\n\n'
                     'One MI355X, one process, batch %d, %s.  The entries are called through ctypes with every argument built once; a window is\n'
                     '%d calls between two HIP events on one stream after %d warm-up calls, the median of %d windows is reported, in\n'
                     'microseconds.  DESIGN.md section 4.8 reads the tables.\n\n'
                     'Pool backward.  `traffic` = x + dy + dx in MiB; `copy`: a device-to-device copy in the same process that reads and writes\n'
                     'traffic / 2 bytes each; both rates are traffic / time in GB/s.  `torch`: `torch.autograd.grad` of `max_pool2d(ceil_mode=True)`\n'
                     'on fp32 channels_last tensors.\n\n' % (a.batch, a.dtype, a.steps, a.warmup, a.repeats))
            fh.write('| shape | traffic MiB | entry us | copy us | torch us | entry GB/s | copy GB/s | entry / copy | entry / torch |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|\n')
            for r in pools:
                fh.write('| %s %dx%dx%d | %s | %s | %s | %s | %s | %s | %s | %s |\n' % (
                    r['shape'], r['h'], r['w'], r['c'], r['traffic_mb'], r['entry_us'], r['copy_us'], r['torch_us'], r['entry_gb_s'],
                    r['copy_gb_s'], r['entry_over_copy'], r['entry_over_torch']))
            fh.write('\n2x2 stride-2 operators.  `dx only`, `dw only`, `all three`: the entry with the other output pointers NULL; every form includes\n'
                     'the fp32 boundary conversions (packing dy, x and the weights, unpacking dx).  `torch dw`, `torch dx+dw`: `torch.autograd.grad`\n'
                     'of `conv2d(stride=2)` / `conv_transpose2d(stride=2)` on bf16 channels_last tensors.\n\n')
            fh.write('| shape | GFLOP | dx only | dw only | all three | torch dw | torch dx+dw | dw / torch dw | all three / torch dx+dw |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|\n')
            for r in convs:
                fh.write('| %s %dx%d %d->%d%s | %s | %s | %s | %s | %s | %s | %s | %s |\n' % (
                    r['shape'], r['h'], r['w'], r['cin'], r['cout'], ' transposed' if r['transpose'] else '', r['gflop_per_gradient'],
                    r['dx_only_us'], r['dw_only_us'], r['all_three_us'], r['torch_dw_us'], r['torch_dx_dw_us'], r['dw_over_torch_dw'],
                    r['all_over_torch_dx_dw']))
            fh.write('\nNot measured: hardware counters of the new kernels (fetch / write sizes, L2 hit rates); any pixel split other than the planner\'s.\n')


if __name__ == '__main__':
    main()
