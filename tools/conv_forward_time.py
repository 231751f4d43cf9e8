#!/usr/bin/env python3
"""Time per call of ron_conv2d_forward_nhwc (the training forward: device weights, packed on the stream) per layer shape of the
two RON-320 variants, as a whole and step by step, in one process: batch 32, bf16.

Per shape the entry is called through ctypes with every argument built once (no Python wrapper, no allocation in the timed window).
`whole` is ron_conv2d_forward_nhwc; `x pack`, `w pack` (weights, bias and, where the planner wants them, the resident-weight images),
`launch` and `unpack` are ron_conv2d_forward_parts_nhwc restricted to that step on the workspace a whole call has filled.  A window
is `--steps` calls between two HIP events on one stream; the median over `--repeats` windows is reported with the spread
(max - min) / median of the whole call's windows.

Yardsticks:
  bench_us    (a) ron_conv2d_bench of the same descriptor: the convolution launch ALONE on packed random tensors ("n/a": the 3-channel
              stem is not benchmarked through that entry);
  host_us     (b) ops.conv2d_nhwc - the test operator the autograd functions called before - fed the SAME device weights the way
              they fed it: w.cpu().numpy(), the host pack, an upload, a stream synchronisation.  Host wall clock around the call
              (it ends in a synchronise), median of `--host-calls` calls;
  copy_us     (c) the least traffic of the weight pack as a device-to-device copy: K * cout fp32 values read, the same number of
              storage-type values written (torch's elementwise cast copy);  w_pack_over_copy = w pack / copy.

    python tools/conv_forward_time.py --out profiles/conv_forward
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ron_tensorflow_amd import _lib, ops  # noqa: E402

# name, h = w of the input, cin, cout, k, dilation, stride, transpose: the distinct convolution shapes of RON-320 `reducedfc` and `full`
# between the image and the heads' inputs (the body, fc6 / fc7, the reverse connections), plus the widest head (cls_pred of block4)
SHAPES = [
    ('conv1_1 (stem)', 320, 3, 64, 3, 1, 1, 0), ('conv1_2', 320, 64, 64, 3, 1, 1, 0), ('conv2_1', 160, 64, 128, 3, 1, 1, 0),
    ('conv2_2', 160, 128, 128, 3, 1, 1, 0), ('conv3_1', 80, 128, 256, 3, 1, 1, 0), ('conv3_3', 80, 256, 256, 3, 1, 1, 0),
    ('conv4_1', 40, 256, 512, 3, 1, 1, 0), ('conv4_3 / block4_conv_left', 40, 512, 512, 3, 1, 1, 0),
    ('conv5_3 / block5_conv_left', 20, 512, 512, 3, 1, 1, 0),
    ('fc6 reducedfc', 10, 512, 1024, 3, 3, 1, 0), ('fc6 full', 10, 512, 4096, 7, 1, 1, 0),
    ('fc7 reducedfc', 10, 1024, 1024, 1, 1, 1, 0), ('fc7 full', 10, 4096, 4096, 1, 1, 1, 0),
    ('block6_conv_left reducedfc', 10, 1024, 512, 3, 1, 1, 0), ('block6_conv_left full', 10, 4096, 512, 3, 1, 1, 0),
    ('block7_conv_left reducedfc', 10, 1024, 512, 2, 1, 2, 0), ('block7_conv_left full', 10, 4096, 512, 2, 1, 2, 0),
    ('block6_deconv_right', 5, 512, 512, 2, 1, 2, 1), ('block5_deconv_right', 10, 512, 512, 2, 1, 2, 1),
    ('block4_deconv_right', 20, 512, 512, 2, 1, 2, 1), ('block4_cls_pred', 40, 512, 210, 3, 1, 1, 0),
]
PARTS = (('x_pack_us', 1), ('w_pack_us', 2), ('launch_us', 4), ('unpack_us', 8))


def windows(fn, steps, warmup, repeats):
    """microseconds per call of `repeats` windows of `steps` calls, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / steps)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-calls', type=int, default=3)
    ap.add_argument('--only', default=None, help='comma-separated substrings of shape names')
    ap.add_argument('--out', default=None, help='directory for conv_forward_bs<batch>.json and README.md')
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to report without one'
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    n = a.batch
    storage = torch.bfloat16 if a.dtype == 'bf16' else torch.float16
    rows = []
    for name, hw, cin, cout, k, dil, stride, tr in SHAPES:
        if a.only and not any(s in name for s in a.only.split(',')):
            continue
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn((n, hw, hw, cin), device=dev, generator=g)
        wshape = (k, k, cout, cin) if tr else (k, k, cin, cout)
        w = torch.randn(wshape, device=dev, generator=g) * float(np.sqrt(2.0 / ((1 if tr else k * k) * cin)))
        b = torch.randn((cout,), device=dev, generator=g) * 0.1
        ho = hw * 2 if tr else hw // stride
        y = torch.empty((n, ho, ho, cout), device=dev)
        d = _lib.ConvDesc(n, hw, hw, cin, cout, k, k, stride, dil, 1, tr, _lib.DTYPES[a.dtype], -1, 0, 0, 0, -1, 0)
        nbytes = lib.ron_conv2d_forward_workspace_bytes(C.byref(d))
        assert nbytes > 0, lib.ron_last_error().decode()
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        stream = _lib.current_stream()
        P = _lib.ptr

        def call(parts=15):
            _lib.check(lib.ron_conv2d_forward_parts_nhwc(C.byref(d), P(x), P(w), P(b), P(y), P(ws), nbytes, parts, stream))
        whole = windows(call, a.steps, a.warmup, a.repeats)
        t = {key: statistics.median(windows(lambda m=mask: call(m), a.steps, a.warmup, a.repeats)) for key, mask in PARTS}
        # the results must not differ from the operator the tests pin: the same bytes at the size that is timed
        kw = dict(stride=stride, dilation=dil, relu=True, transpose=bool(tr), dtype=a.dtype)
        w_host_path = lambda: ops.conv2d_nhwc(x, w.cpu().numpy(), b.cpu().numpy(), **kw)       # noqa: E731
        same = bool(torch.equal(w_host_path(), y))
        host = []
        for _ in range(a.host_calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w_host_path()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e6)
        if cin == 3:
            t_bench = 'n/a'
        else:
            ms = C.c_float(0)
            _lib.check(lib.ron_conv2d_bench(C.byref(d), a.warmup, a.steps, C.byref(ms)))
            t_bench = round(ms.value * 1e3, 2)
        src = w.reshape(-1)
        dst = torch.empty(src.shape, dtype=storage, device=dev)
        t_copy = statistics.median(windows(lambda: dst.copy_(src), a.steps, a.warmup, a.repeats))
        t_whole = statistics.median(whole)
        row = dict(shape=name, batch=n, h=hw, w=hw, cin=cin, cout=cout, k=k, dilation=dil, stride=stride, transpose=tr, dtype=a.dtype,
                   steps=a.steps, repeats=a.repeats, workspace_mb=round(nbytes / 2 ** 20, 1), weights_mb_fp32=round(w.numel() * 4 / 2 ** 20, 2),
                   whole_us=round(t_whole, 2), whole_spread=round((max(whole) - min(whole)) / t_whole, 3),
                   x_pack_us=round(t['x_pack_us'], 2), w_pack_us=round(t['w_pack_us'], 2), launch_us=round(t['launch_us'], 2),
                   unpack_us=round(t['unpack_us'], 2), bench_us=t_bench, host_us=round(statistics.median(host), 1),
                   copy_us=round(t_copy, 2), w_pack_over_copy=round(t['w_pack_us'] / t_copy, 2),
                   w_pack_gb_s=round(w.numel() * 6 / (t['w_pack_us'] * 1e-6) / 1e9, 1), host_over_whole=round(statistics.median(host) / t_whole, 1),
                   same_bytes_as_host_path=same)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, w, b, y, ws, src, dst
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'conv_forward_bs%d.json' % n), 'w') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')
        with open(os.path.join(a.out, 'table_bs%d.md' % n), 'w') as fh:
            fh.write('| shape | whole | spread | x pack | w pack | launch | unpack | (a) bench | (b) host path | (c) copy | w pack / copy | w pack GB/s | host / whole | same bytes |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                fh.write('| %s %dx%d %d->%d k%d | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |\n' % (
                    r['shape'], r['h'], r['w'], r['cin'], r['cout'], r['k'], r['whole_us'], r['whole_spread'], r['x_pack_us'], r['w_pack_us'],
                    r['launch_us'], r['unpack_us'], r['bench_us'], r['host_us'], r['copy_us'], r['w_pack_over_copy'], r['w_pack_gb_s'],
                    r['host_over_whole'], r['same_bytes_as_host_path']))


if __name__ == '__main__':
    main()
