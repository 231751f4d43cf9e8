#!/usr/bin/env python3
"""Time per call of ron_conv2d_stem_backward_nhwc (conv1_1: 3 -> 64 channels, 3x3) at 320 x 320, batch 32, bf16, with the ReLU
mask, beside two yardsticks in one process.

The entry is called through ctypes with every argument built once (no Python wrapper, no allocation in the timed window); a window
is `--steps` calls between two HIP events on one stream and the median over `--repeats` windows is reported (the window method of
tools/conv_backward_time.py).  Forms: dw + db (the layer's backward), dw only, db only, and dw + db at forced pixel splits.

Yardsticks:
  copy_us      a device-to-device copy, in the same process, that moves the operator's MINIMUM traffic, dy and y read once: it reads
               and writes one [n,h,w,64] fp32 tensor (as tools/batchnorm_time.py does).  The copy, not a constant, is the yardstick
               for "bandwidth bound": both rates are traffic / time;
  torch_dw_us  torch.autograd.grad of torch.nn.functional.conv2d for the weight on bf16 channels_last tensors (no mask, no bias
               gradient, half the bytes per element: not the same work, the nearest thing torch offers).

    python tools/stem_backward_time.py --out profiles/conv_backward
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from conv_backward_time import median_of  # noqa: E402
from ron_tensorflow_amd import _lib  # noqa: E402

SECTION = '## ron_conv2d_stem_backward_nhwc (conv1_1)'


def torch_dw_us(x, dy, a):
    try:
        xt = x.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        wt = torch.zeros((64, 3, 3, 3), dtype=torch.bfloat16, device=x.device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        dyt = dy.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        out = torch.nn.functional.conv2d(xt, wt, None, padding=1)
        return round(median_of(lambda: torch.autograd.grad(out, (wt,), dyt, retain_graph=True), a.steps, a.warmup, a.repeats), 2)
    except Exception as e:          # noqa: BLE001 - whatever torch / MIOpen refuses is reported, not fatal
        print('torch conv weight gradient failed: %s' % str(e).splitlines()[0], flush=True)
        return 'n/a'


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--splits', default='256,512,2048,4096', help='forced pixel splits timed beside the by-shape one')
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--out', default=None, help='directory for stem_backward_bs<batch>.json and its section of README.md')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    n, hw = a.batch, a.size
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((n, hw, hw, 3), device=dev, generator=g) * 60.0
    y = torch.relu(torch.randn((n, hw, hw, 64), device=dev, generator=g))
    dy = torch.randn((n, hw, hw, 64), device=dev, generator=g)
    dw, db = torch.empty((3, 3, 3, 64), device=dev), torch.empty((64,), device=dev)
    stream = _lib.current_stream()
    P = _lib.ptr

    def timed(splitk, pdw, pdb):
        d = _lib.ConvDesc(n, hw, hw, 3, 64, 3, 3, 1, 1, 1, 0, _lib.DTYPES[a.dtype], -1, 0, 0, 0, splitk, 0)
        nbytes = lib.ron_conv2d_stem_backward_workspace_bytes(C.byref(d))
        assert nbytes > 0, lib.ron_last_error().decode()
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        t = median_of(lambda: _lib.check(lib.ron_conv2d_stem_backward_nhwc(C.byref(d), P(x), P(y), P(dy), pdw, pdb, P(ws), nbytes, stream)),
                      a.steps, a.warmup, a.repeats)
        return t, nbytes

    t_both, nbytes = timed(-1, P(dw), P(db))
    t_dw, _ = timed(-1, P(dw), None)
    t_db, _ = timed(-1, None, P(db))
    forced = {}
    for s in [int(v) for v in a.splits.split(',') if v]:
        forced[str(s)] = round(timed(s, P(dw), P(db))[0], 2)
    tensor = y.numel() * 4
    src = y.reshape(-1).clone()
    dst = torch.empty_like(src)
    t_copy = median_of(lambda: dst.copy_(src, non_blocking=True), a.steps, a.warmup, a.repeats)
    del src, dst
    t_torch = 'n/a' if a.no_torch else torch_dw_us(x, dy, a)
    traffic = 2 * tensor + x.numel() * 4
    row = dict(shape='conv1_1', batch=n, h=hw, w=hw, cin=3, cout=64, k=3, dtype=a.dtype, relu=1, steps=a.steps, repeats=a.repeats,
               workspace_mb=round(nbytes / 2 ** 20, 2), slices=nbytes // (1792 * 4), tensor_mb=round(tensor / 2 ** 20, 1),
               dw_db_us=round(t_both, 2), dw_only_us=round(t_dw, 2), db_only_us=round(t_db, 2), forced_split_us=forced,
               copy_us=round(t_copy, 2), torch_dw_us=t_torch, dw_db_gb_s=round(traffic / t_both / 1e3, 1),
               copy_gb_s=round(2 * tensor / t_copy / 1e3, 1), dw_db_over_copy=round(t_both / t_copy, 2),
               dw_db_over_torch_dw='n/a' if t_torch == 'n/a' else round(t_both / t_torch, 2))
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'stem_backward_bs%d.json' % n), 'w') as fh:
            fh.write(json.dumps(row) + '\n')
        readme = os.path.join(a.out, 'README.md')
        head = open(readme).read().split(SECTION)[0].rstrip('\n') + '\n\n' if os.path.exists(readme) else ''
        with open(readme, 'w') as fh:          # this tool's section is the last one of the file and is replaced as a whole
            fh.write(head + SECTION + '\n\n'
                     '    python tools/stem_backward_time.py --out profiles/conv_backward\n\n'
                     'The same window method, batch %d, %d x %d, %s, ReLU mask on: `stem_backward_bs%d.json`.  `copy`: a device-to-device copy of\n'
                     'one [n,h,w,64] fp32 tensor in the same process: it reads and writes what the entry must at least read (dy and y once).\n'
                     '`torch dw`: `torch.autograd.grad` of `conv2d` for the weight on bf16 channels_last tensors (no mask, no bias gradient, half\n'
                     'the bytes per element).  Forced splits: `dw + db` with `splitk` set.  (tools/conv_backward_time.py rewrites this file:\n'
                     'run this tool after it.)\n\n' % (n, hw, hw, a.dtype, n))
            fh.write('| shape | tensor MiB | slices | dw + db | dw only | db only | copy | torch dw | dw+db GB/s | copy GB/s | dw+db / copy | dw+db / torch dw |\n')
            fh.write('|---|---|---|---|---|---|---|---|---|---|---|---|\n')
            fh.write('| conv1_1 %dx%d 3->64 k3 | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |\n\n' % (
                hw, hw, row['tensor_mb'], row['slices'], row['dw_db_us'], row['dw_only_us'], row['db_only_us'], row['copy_us'],
                row['torch_dw_us'], row['dw_db_gb_s'], row['copy_gb_s'], row['dw_db_over_copy'], row['dw_db_over_torch_dw']))
            fh.write('| forced split | ' + ' | '.join(forced) + ' |\n|---|' + '---|' * len(forced) + '\n| dw + db, us | '
                     + ' | '.join(str(v) for v in forced.values()) + ' |\n\n'
                     'Not measured: the two kernels apart (stem_wgrad_kernel, stem_wgrad_reduce_kernel: no kernel trace was taken), LDS\n'
                     'bank-conflict, L2 and MFMA-busy counters, fp16, any other batch or image size.  DESIGN.md section 4.7 reads the row.\n')


if __name__ == '__main__':
    main()
