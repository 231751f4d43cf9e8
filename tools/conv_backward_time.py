#!/usr/bin/env python3
"""Time per call of ron_conv2d_backward_nhwc per layer shape, beside the forward launch of the same descriptor and torch's own
convolution backward, in one process: batch 32, bf16.

Per shape the entry is called through ctypes with every argument built once (no Python wrapper, no allocation in the timed window)
in three forms - dx only, dw only, all three outputs (the other output pointers NULL); a window is `--steps` calls between two HIP
events on one stream and the median over `--repeats` windows is reported.  The entry converts at the fp32 boundary (it packs x, dy
and the weights on every call and unpacks dx), so `dw only` is pack(dy) + pack(x) + the weight-gradient kernel (+ the slab sum).

Yardsticks:
  forward_us   ron_conv2d_bench of the same descriptor: the forward launch ALONE on packed tensors (no boundary conversions), the
               same FLOPs as either gradient;
  torch_*_us   torch.nn.functional.conv2d on bf16 channels_last tensors, torch.autograd.grad for the weight only and for input +
               weight ("n/a" when torch cannot run the shape).

    python tools/conv_backward_time.py --out profiles/conv_backward
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

# name, h = w, cin, cout, k
SHAPES = [('conv1_2', 320, 64, 64, 3), ('conv2_2', 160, 128, 128, 3), ('conv3_3', 80, 256, 256, 3), ('conv4_3', 40, 512, 512, 3),
          ('conv5_3', 20, 512, 512, 3), ('fc7', 10, 1024, 1024, 1), ('block4_cls_pred', 40, 512, 210, 3)]


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


def torch_times(x, w, dy, k, steps, warmup, repeats):
    """(dw only, dx + dw) of torch's bf16 channels_last convolution backward, or ('n/a', 'n/a')."""
    try:
        xt = x.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        wt = w.permute(3, 2, 0, 1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        dyt = dy.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        out = torch.nn.functional.conv2d(xt, wt, None, padding=(k - 1) // 2)
        t_w = median_of(lambda: torch.autograd.grad(out, (wt,), dyt, retain_graph=True), steps, warmup, repeats)
        t_xw = median_of(lambda: torch.autograd.grad(out, (xt, wt), dyt, retain_graph=True), steps, warmup, repeats)
        return round(t_w, 2), round(t_xw, 2)
    except Exception as e:          # noqa: BLE001 - whatever torch / MIOpen refuses is reported, not fatal
        print('torch conv backward failed: %s' % str(e).splitlines()[0], flush=True)
        return 'n/a', 'n/a'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--only', default=None, help='comma-separated shape names')
    ap.add_argument('--out', default=None, help='directory for conv_backward_bs<batch>.json and README.md')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    n = a.batch
    rows = []
    for name, hw, cin, cout, k in SHAPES:
        if a.only and name not in a.only.split(','):
            continue
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn((n, hw, hw, cin), device=dev, generator=g)
        w = torch.randn((k, k, cin, cout), device=dev, generator=g) * float(np.sqrt(2.0 / (k * k * cin)))
        y = torch.relu(torch.randn((n, hw, hw, cout), device=dev, generator=g))
        dy = torch.randn((n, hw, hw, cout), device=dev, generator=g)
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty((cout,), device=dev)
        d = _lib.ConvDesc(n, hw, hw, cin, cout, k, k, 1, 1, 1, 0, _lib.DTYPES[a.dtype], -1, 0, 0, 0, -1, 0)
        nbytes = lib.ron_conv2d_backward_workspace_bytes(C.byref(d))
        assert nbytes > 0, lib.ron_last_error().decode()
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        stream = _lib.current_stream()
        P = _lib.ptr

        def call(pdx, pdw, pdb):
            _lib.check(lib.ron_conv2d_backward_nhwc(C.byref(d), P(x), P(w), P(y), P(dy), pdx, pdw, pdb, P(ws), nbytes, stream))
        t_dx = median_of(lambda: call(P(dx), None, None), a.steps, a.warmup, a.repeats)
        t_dw = median_of(lambda: call(None, P(dw), None), a.steps, a.warmup, a.repeats)
        t_all = median_of(lambda: call(P(dx), P(dw), P(db)), a.steps, a.warmup, a.repeats)
        ms = C.c_float(0)
        _lib.check(lib.ron_conv2d_bench(C.byref(d), a.warmup, a.steps, C.byref(ms)))
        t_fwd = ms.value * 1e3
        t_tw, t_txw = ('n/a', 'n/a') if a.no_torch else torch_times(x, w, dy, k, a.steps, a.warmup, a.repeats)
        flops = 2.0 * n * hw * hw * k * k * cin * cout
        row = dict(shape=name, batch=n, h=hw, w=hw, cin=cin, cout=cout, k=k, dtype=a.dtype, steps=a.steps, repeats=a.repeats,
                   workspace_mb=round(nbytes / 2 ** 20, 1), gflop_per_gradient=round(flops / 1e9, 2),
                   dx_only_us=round(t_dx, 2), dw_only_us=round(t_dw, 2), all_three_us=round(t_all, 2), forward_us=round(t_fwd, 2),
                   torch_dw_us=t_tw, torch_dx_dw_us=t_txw,
                   dw_over_forward=round(t_dw / t_fwd, 2), dw_over_torch_dw='n/a' if t_tw == 'n/a' else round(t_dw / t_tw, 2),
                   dw_tflops=round(flops / (t_dw * 1e-6) / 1e12, 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, w, y, dy, dx, dw, db, ws
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'conv_backward_bs%d.json' % n), 'w') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write('# profiles/conv_backward - ron_conv2d_backward_nhwc per layer shape\n\n'
                     '    python tools/conv_backward_time.py --out profiles/conv_backward\n\n'
                     'One MI355X, one process, batch %d, %s.  The entry is called through ctypes with every argument built once; a window is\n'
                     '%d calls between two HIP events on one stream after %d warm-up calls, the median of %d windows is reported, in\n'
                     'microseconds.  `dx only`, `dw only`, `all three`: the entry with the other output pointers NULL; every form includes the\n'
                     'fp32 boundary conversions of the entry (packing dy, x and the weights, unpacking dx).  `forward`: `ron_conv2d_bench` of the\n'
                     'same descriptor, the forward launch alone on packed tensors (the same FLOPs as either gradient).  `torch dw`, `torch dx+dw`:\n'
                     '`torch.autograd.grad` of `torch.nn.functional.conv2d` on bf16 channels_last tensors.  DESIGN.md section 4.7 reads the table.\n\n'
                     % (n, a.dtype, a.steps, a.warmup, a.repeats))
            fh.write('| shape | GFLOP | dx only | dw only | all three | forward | torch dw | torch dx+dw | dw / forward | dw / torch dw | dw TFLOP/s |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                fh.write('| %s %dx%d %d->%d k%d | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |\n' % (
                    r['shape'], r['h'], r['w'], r['cin'], r['cout'], r['k'], r['gflop_per_gradient'], r['dx_only_us'], r['dw_only_us'],
                    r['all_three_us'], r['forward_us'], r['torch_dw_us'], r['torch_dx_dw_us'], r['dw_over_forward'], r['dw_over_torch_dw'],
                    r['dw_tflops']))


if __name__ == '__main__':
    main()
