#!/usr/bin/env python3
"""Time per call of the backward of the SSD-only operators, beside torch's own backward of the same operators, in one process:
batch 32, bf16.

  ron_maxpool3x3s1_backward_nhwc   at pool5 of SSD-300 (19x19x512) and SSD-512 (32x32x512)
  ron_l2norm_backward_nhwc         at block4 of SSD-300 (38x38x512) and SSD-512 (64x64x512)
  ron_conv2d_padded_backward_nhwc  at block8 / block9 of both networks (pad2d(1) + 3x3 stride 2), beside ron_conv2d_backward_nhwc at
                                   the same full-resolution shape: by construction the two should be about level

The entries are called through ctypes with every argument built once (no Python wrapper, no allocation in the timed window); a
window is `--steps` calls between two HIP events on one stream and the median over `--repeats` windows is reported.

Yardsticks of the pool and the normalisation: copy_us, a device-to-device copy in the same process that reads and writes
(x + dy + dx) / 2 bytes each (the operators' minimum traffic: x and dy read, dx written), and torch_us, torch.autograd.grad of
max_pool2d(3, 1, 1) on fp32 channels_last tensors / of x * rsqrt(clamp_min(sum x^2, 1e-12)) * gamma on fp32 NHWC tensors.
Of the convolutions: torch.autograd.grad of conv2d(stride=2, padding=1) on bf16 channels_last tensors, input + weight.

    python tools/ssd_backward_time.py --out profiles/ssd_backward
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

POOLS = [('pool5 SSD-300', 19, 512), ('pool5 SSD-512', 32, 512)]
NORMS = [('block4 SSD-300', 38, 512), ('block4 SSD-512', 64, 512)]
# name, h = w of the input x, cin, cout
CONVS = [('block8 SSD-300', 19, 256, 512), ('block9 SSD-300', 10, 128, 256), ('block8 SSD-512', 32, 256, 512), ('block9 SSD-512', 16, 128, 256)]


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


def copy_us(traffic, dev, a):
    src = torch.empty((traffic // 2,), dtype=torch.uint8, device=dev).zero_()
    dst = torch.empty_like(src)
    return median_of(lambda: dst.copy_(src, non_blocking=True), a.steps, a.warmup, a.repeats)


def elementwise_row(op, name, n, hw, c, t_us, t_copy, t_torch, a, traffic):
    row = dict(op=op, shape=name, batch=n, h=hw, w=hw, c=c, dtype=a.dtype, steps=a.steps, repeats=a.repeats,
               traffic_mb=round(traffic / 2 ** 20, 1), entry_us=round(t_us, 2), copy_us=round(t_copy, 2), torch_us=t_torch,
               entry_gb_s=round(traffic / t_us / 1e3, 1), copy_gb_s=round(traffic / t_copy / 1e3, 1),
               entry_over_copy=round(t_us / t_copy, 2), entry_over_torch=ratio(round(t_us, 2), t_torch))
    print(json.dumps(row), flush=True)
    return row


def pool_rows(a, dev, lib):
    rows = []
    n, P, stream = a.batch, _lib.ptr, _lib.current_stream()
    for name, hw, c in POOLS:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.relu(torch.randn((n, hw, hw, c), device=dev, generator=g))
        dy = torch.randn((n, hw, hw, c), device=dev, generator=g)
        dx = torch.empty_like(x)
        t_us = median_of(lambda: _lib.check(lib.ron_maxpool3x3s1_backward_nhwc(P(x), P(dy), n, hw, hw, c, _lib.DTYPES[a.dtype], P(dx), stream)),
                         a.steps, a.warmup, a.repeats)
        traffic = 4 * 3 * x.numel()
        t_copy = copy_us(traffic, dev, a)

        def torch_pool():
            xt = x.permute(0, 3, 1, 2).requires_grad_(True)          # NHWC memory seen as a channels_last NCHW tensor: no copy
            out = torch.nn.functional.max_pool2d(xt, 3, 1, 1)
            dyt = dy.permute(0, 3, 1, 2)
            return median_of(lambda: torch.autograd.grad(out, (xt,), dyt, retain_graph=True), a.steps, a.warmup, a.repeats)
        t_torch = 'n/a' if a.no_torch else guarded('max_pool2d backward', torch_pool)
        rows.append(elementwise_row('maxpool3x3s1_backward', name, n, hw, c, t_us, t_copy, t_torch, a, traffic))
        del x, dy, dx
        torch.cuda.empty_cache()
    return rows


def norm_rows(a, dev, lib):
    rows = []
    n, P, stream = a.batch, _lib.ptr, _lib.current_stream()
    for name, hw, c in NORMS:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.relu(torch.randn((n, hw, hw, c), device=dev, generator=g))
        dy = torch.randn((n, hw, hw, c), device=dev, generator=g)
        gamma = torch.full((c,), 20.0, device=dev)
        dx, dgamma = torch.empty_like(x), torch.empty_like(gamma)
        nbytes = lib.ron_l2norm_backward_workspace_bytes(n, hw, hw, c, _lib.DTYPES[a.dtype])
        assert nbytes > 0, lib.ron_last_error().decode()
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        t_us = median_of(lambda: _lib.check(lib.ron_l2norm_backward_nhwc(P(x), P(gamma), P(dy), n, hw, hw, c, _lib.DTYPES[a.dtype], P(dx),
                                                                         P(dgamma), P(ws), nbytes, stream)), a.steps, a.warmup, a.repeats)
        t_dx = median_of(lambda: _lib.check(lib.ron_l2norm_backward_nhwc(P(x), P(gamma), P(dy), n, hw, hw, c, _lib.DTYPES[a.dtype], P(dx),
                                                                         None, P(ws), nbytes, stream)), a.steps, a.warmup, a.repeats)
        traffic = 4 * 3 * x.numel()
        t_copy = copy_us(traffic, dev, a)

        def torch_norm():
            xt, gt = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
            out = xt * torch.rsqrt(torch.clamp_min((xt * xt).sum(dim=-1, keepdim=True), 1e-12)) * gt
            return median_of(lambda: torch.autograd.grad(out, (xt, gt), dy, retain_graph=True), a.steps, a.warmup, a.repeats)
        t_torch = 'n/a' if a.no_torch else guarded('l2 normalisation backward', torch_norm)
        row = elementwise_row('l2norm_backward', name, n, hw, c, t_us, t_copy, t_torch, a, traffic)
        row['dx_only_us'] = round(t_dx, 2)
        row['workspace_mb'] = round(nbytes / 2 ** 20, 1)
        rows.append(row)
        del x, dy, dx, ws
        torch.cuda.empty_cache()
    return rows


def conv_rows(a, dev, lib):
    rows = []
    n, P, stream = a.batch, _lib.ptr, _lib.current_stream()
    for name, hw, cin, cout in CONVS:
        g = torch.Generator(device=dev).manual_seed(1)
        ho = (hw - 1) // 2 + 1
        x = torch.randn((n, hw, hw, cin), device=dev, generator=g)
        w = torch.randn((3, 3, cin, cout), device=dev, generator=g) * float(np.sqrt(2.0 / (9 * cin)))
        y = torch.relu(torch.randn((n, ho, ho, cout), device=dev, generator=g))
        dy = torch.randn((n, ho, ho, cout), device=dev, generator=g)
        yf = torch.relu(torch.randn((n, hw, hw, cout), device=dev, generator=g))
        dyf = torch.randn((n, hw, hw, cout), device=dev, generator=g)
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty((cout,), device=dev)
        d = _lib.ConvDesc(n, hw, hw, cin, cout, 3, 3, 2, 1, 1, 0, _lib.DTYPES[a.dtype], -1, 0, 0, 0, -1, 0)
        d1 = _lib.ConvDesc(n, hw, hw, cin, cout, 3, 3, 1, 1, 1, 0, _lib.DTYPES[a.dtype], -1, 0, 0, 0, -1, 0)
        nbytes = lib.ron_conv2d_padded_backward_workspace_bytes(C.byref(d), 1)
        assert nbytes > 0 and nbytes == lib.ron_conv2d_backward_workspace_bytes(C.byref(d1)), lib.ron_last_error().decode()
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        t_pad = median_of(lambda: _lib.check(lib.ron_conv2d_padded_backward_nhwc(C.byref(d), 1, P(x), P(w), P(y), P(dy), P(dx), P(dw), P(db), P(ws),
                                                                                 nbytes, stream)), a.steps, a.warmup, a.repeats)
        t_full = median_of(lambda: _lib.check(lib.ron_conv2d_backward_nhwc(C.byref(d1), P(x), P(w), P(yf), P(dyf), P(dx), P(dw), P(db), P(ws), nbytes,
                                                                           stream)), a.steps, a.warmup, a.repeats)
        t_torch = 'n/a'
        if not a.no_torch:
            def torch_conv():
                xt = x.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                wt = w.permute(3, 2, 0, 1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                dyt = dy.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
                out = torch.nn.functional.conv2d(xt, wt, None, stride=2, padding=1)
                return median_of(lambda: torch.autograd.grad(out, (xt, wt), dyt, retain_graph=True), a.steps, a.warmup, a.repeats)
            t_torch = guarded('conv2d(stride=2, padding=1) dx + dw', torch_conv)
        row = dict(op='conv2d_padded_backward', shape=name, batch=n, h=hw, w=hw, cin=cin, cout=cout, stride=2, cpad=1, dtype=a.dtype, steps=a.steps,
                   repeats=a.repeats, workspace_mb=round(nbytes / 2 ** 20, 1), padded_us=round(t_pad, 2), stride1_same_us=round(t_full, 2),
                   torch_dx_dw_us=t_torch, padded_over_stride1=round(t_pad / t_full, 2), padded_over_torch=ratio(round(t_pad, 2), t_torch))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, w, y, dy, yf, dyf, dx, dw, db, ws
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
    ap.add_argument('--out', default=None, help='directory for ssd_backward_bs<batch>.json and README.md')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    pools, norms, convs = pool_rows(a, dev, lib), norm_rows(a, dev, lib), conv_rows(a, dev, lib)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'ssd_backward_bs%d.json' % a.batch), 'w') as fh:
            for row in pools + norms + convs:
                fh.write(json.dumps(row) + '\n')
        with open(os.path.join(a.out, 'README.md'), 'w') as fh:
            fh.write('# profiles/ssd_backward - the backward of the SSD-only operators\n\n'
                     '    python tools/ssd_backward_time.py --out profiles/ssd_backward\n\n'
                     'One MI355X, one process, batch %d, %s.  The entries are called through ctypes with every argument built once; a window is\n'
                     '%d calls between two HIP events on one stream after %d warm-up calls, the median of %d windows is reported, in\n'
                     'microseconds.  DESIGN.md section 4.11 reads the tables.\n\n'
                     'Pool and L2 normalisation.  `traffic` = x + dy + dx in MiB (the minimum: x and dy read, dx written); `copy`: a\n'
                     'device-to-device copy in the same process that reads and writes traffic / 2 bytes each; both rates are traffic / time in\n'
                     'GB/s.  `torch`: `torch.autograd.grad` of `max_pool2d(3, 1, 1)` on fp32 channels_last tensors / of\n'
                     '`x * rsqrt(clamp_min(sum(x*x), 1e-12)) * gamma` on fp32 tensors (dx and dgamma).\n\n' % (a.batch, a.dtype, a.steps, a.warmup, a.repeats))
            fh.write('| operator | shape | traffic MiB | entry us | copy us | torch us | entry GB/s | copy GB/s | entry / copy | entry / torch |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|---|\n')
            for r in pools + norms:
                fh.write('| %s | %s %dx%dx%d | %s | %s | %s | %s | %s | %s | %s | %s |\n' % (
                    r['op'], r['shape'], r['h'], r['w'], r['c'], r['traffic_mb'], r['entry_us'], r['copy_us'], r['torch_us'], r['entry_gb_s'],
                    r['copy_gb_s'], r['entry_over_copy'], r['entry_over_torch']))
            fh.write('\nL2 normalisation with dgamma NULL (no table, no second kernel): %s.\n' % ', '.join(
                '%s %s us' % (r['shape'], r['dx_only_us']) for r in norms))
            fh.write('\nPadded 3x3 stride-2 convolutions, all three gradients.  `padded`: ron_conv2d_padded_backward_nhwc; `stride-1 SAME`:\n'
                     'ron_conv2d_backward_nhwc at the same full-resolution shape (the same kernels behind a pack that does not scatter);\n'
                     '`torch`: `torch.autograd.grad` of `conv2d(stride=2, padding=1)` on bf16 channels_last tensors, input + weight.\n\n')
            fh.write('| shape | workspace MiB | padded us | stride-1 SAME us | torch dx+dw us | padded / stride-1 | padded / torch |\n')
            fh.write('|---|---|---|---|---|---|---|\n')
            for r in convs:
                fh.write('| %s %dx%d %d->%d | %s | %s | %s | %s | %s | %s |\n' % (
                    r['shape'], r['h'], r['w'], r['cin'], r['cout'], r['workspace_mb'], r['padded_us'], r['stride1_same_us'], r['torch_dx_dw_us'],
                    r['padded_over_stride1'], r['padded_over_torch']))
            fh.write('\nNot measured: hardware counters of the new kernels (fetch / write sizes, L2 hit rates, VALU utilisation of the pool); fp16;\n'
                     'batch sizes other than %d; the plain VALID form (block10 / block11 of SSD-300: 5x5 and 3x3 maps).\n' % a.batch)


if __name__ == '__main__':
    main()
