#!/usr/bin/env python3
"""Time of the VGG body (conv1_2 .. fc7 with pool1 .. pool5) forward and backward, as ONE convolution chain
(ron_conv_chain_forward / ron_conv_chain_backward) beside the per-operator sequence it replaces, in one process: RON-320
`reducedfc` and `full` at 320 x 320, batch 32, bf16.

Both are called through ctypes with every argument built once (no Python wrapper, no allocation in the timed window).  The
per-operator sequence is what chaining ops.conv2d_nhwc_fn / ops.maxpool2x2_nhwc_fn executes: ron_conv2d_forward_nhwc and
ron_maxpool2x2_nhwc layer by layer forward; ron_conv2d_backward_nhwc and ron_maxpool2x2_backward_nhwc in reverse order backward,
with the fp32 add autograd makes where a tap's gradient joins.  It is unchanged code, so it is the yardstick taken on the same box
in the same run.  ron_maxpool2x2_nhwc is a test operator that allocates and synchronises, so the forward sequence is given twice:
`ops_fwd_us` with the pools and `ops_fwd_convs_us` WITHOUT them (the five pools left out entirely): the chain, which includes its
pools, must beat the second, smaller number.

A window is `--steps` calls between two HIP events on one stream; chain and sequence windows alternate; the median over `--repeats`
windows is reported with the spread (max - min) / median.  The equality assertion of tests/test_gpu_conv_chain.py is repeated at
the size that is timed: y, the taps, dx, every dw and db of the chain against the sequence's, torch.equal.

`copy_gb_s` is a device-to-device copy of 256 MiB (bytes read + bytes written over time); `min_traffic` lists, per new bandwidth
kernel, the least bytes its launches of one forward + backward must move, computed from the shapes; copy_us = those bytes at the
copy's rate.  The kernels' own times come from a kernel trace of `--calls N` (N forward + backward calls of the chain and nothing
else, under rocprofv3 --kernel-trace in a run of its own), folded into the table by `--trace CSV --calls N`.

    python tools/conv_chain_time.py --out profiles/conv_chain
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ron_tensorflow_amd import _lib, ops  # noqa: E402
from ron_tensorflow_amd.nets.ron_vgg_320 import vgg_body_chain  # noqa: E402

NEW_KERNELS = ('chain_join_kernel', 'chain_zero_kernel', 'chain_pool_bwd_kernel')


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


class Body(object):
    """The tensors and the prepared calls of one variant."""

    def __init__(self, variant, n, hw, dtype, dev):
        self.layers, self.names = vgg_body_chain(variant)
        self.n, self.hw, self.dtype, self.dev = n, hw, dtype, dev
        L = self.L = len(self.layers)
        g = torch.Generator(device=dev).manual_seed(1)
        rand = lambda *s: torch.randn(s, device=dev, generator=g)
        self.shapes = ops.conv_chain_shapes(n, hw, hw, 64, self.layers, dtype)
        ins = [(n, hw, hw, 64)] + self.shapes[:-1]
        self.x = torch.relu(rand(n, hw, hw, 64))            # conv1_1's output: behind a ReLU
        self.w, self.b = [None] * L, [None] * L
        for i, l in enumerate(self.layers):
            if l['kind'] == 'conv':
                cin, k = ins[i][3], l['k']
                self.w[i] = rand(k, k, cin, l['cout']) * float(np.sqrt(2.0 / (k * k * cin)))
                self.b[i] = rand(l['cout']) * 0.1
        self.dy = rand(*self.shapes[-1])
        self.dtap = [rand(*self.shapes[i]) if l.get('tap') else None for i, l in enumerate(self.layers)]
        new = lambda s: torch.empty(tuple(s), dtype=torch.float32, device=dev)
        # the chain's outputs and the sequence's: the same shapes
        self.c_y, self.c_dx = new(self.shapes[-1]), new(self.x.shape)
        self.c_taps = [new(self.shapes[i]) if l.get('tap') else None for i, l in enumerate(self.layers)]
        self.c_dw = [None if w is None else new(w.shape) for w in self.w]
        self.c_db = [None if b is None else new(b.shape) for b in self.b]
        self.act = [self.x] + [new(s) for s in self.shapes]
        self.grad = [new(s) for s in ins] + [self.dy]
        self.gsum = [new(self.shapes[i]) if l.get('tap') else None for i, l in enumerate(self.layers)]
        self.o_dw = [None if w is None else new(w.shape) for w in self.w]
        self.o_db = [None if b is None else new(b.shape) for b in self.b]
        lib = self.lib = _lib.lib()
        self.d = ops._chain_desc(n, hw, hw, 64, self.layers, dtype)
        self.ws_bytes = lib.ron_conv_chain_workspace_bytes(C.byref(self.d))
        assert self.ws_bytes > 0, lib.ron_last_error().decode()
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=dev)
        P = ops._chain_ptrs
        self.pw, self.pb, self.ptaps = P(self.w, L), P(self.b, L), P(self.c_taps, L)
        self.pdtap, self.pdw, self.pdb = P(self.dtap, L), P(self.c_dw, L), P(self.c_db, L)
        self.descs, fb, bb = [None] * L, 0, 0
        for i, l in enumerate(self.layers):
            if l['kind'] == 'conv':
                d = _lib.ConvDesc(n, ins[i][1], ins[i][2], ins[i][3], l['cout'], l['k'], l['k'], 1, l['dilation'], 1, 0, _lib.DTYPES[dtype],
                                  -1, 0, 0, 0, -1, 0)
                self.descs[i] = d
                fb = max(fb, lib.ron_conv2d_forward_workspace_bytes(C.byref(d)))
                bb = max(bb, lib.ron_conv2d_backward_workspace_bytes(C.byref(d)))
        self.ows = torch.empty((max(fb, bb),), dtype=torch.uint8, device=dev)
        self.ins = ins
        self.stream = _lib.current_stream()

    def chain_fwd(self):
        _lib.check(self.lib.ron_conv_chain_forward(C.byref(self.d), _lib.ptr(self.x), self.pw, self.pb, self.ptaps, _lib.ptr(self.c_y),
                                                   _lib.ptr(self.ws), self.ws_bytes, self.stream))

    def chain_bwd(self):
        _lib.check(self.lib.ron_conv_chain_backward(C.byref(self.d), _lib.ptr(self.dy), self.pdtap, self.pw, _lib.ptr(self.c_dx), self.pdw,
                                                    self.pdb, _lib.ptr(self.ws), self.ws_bytes, self.stream))

    def ops_fwd(self, pools=True):
        P, lib, dt = _lib.ptr, self.lib, _lib.DTYPES[self.dtype]
        for i, l in enumerate(self.layers):
            if l['kind'] == 'conv':
                _lib.check(lib.ron_conv2d_forward_nhwc(C.byref(self.descs[i]), P(self.act[i]), P(self.w[i]), P(self.b[i]), P(self.act[i + 1]),
                                                       P(self.ows), int(self.ows.numel()), self.stream))
            elif pools:
                n, h, w, c = self.ins[i]
                _lib.check(lib.ron_maxpool2x2_nhwc(P(self.act[i]), n, h, w, c, dt, P(self.act[i + 1]), self.stream))

    def ops_bwd(self):
        P, lib, dt = _lib.ptr, self.lib, _lib.DTYPES[self.dtype]
        for i in reversed(range(self.L)):
            l = self.layers[i]
            g = self.grad[i + 1]
            if l.get('tap') and i + 1 < self.L:
                g = torch.add(g, self.dtap[i], out=self.gsum[i])
            if l['kind'] == 'conv':
                _lib.check(lib.ron_conv2d_backward_nhwc(C.byref(self.descs[i]), P(self.act[i]), P(self.w[i]), P(self.act[i + 1]), P(g),
                                                        P(self.grad[i]), P(self.o_dw[i]), P(self.o_db[i]), P(self.ows), int(self.ows.numel()),
                                                        self.stream))
            else:
                n, h, w, c = self.ins[i]
                _lib.check(lib.ron_maxpool2x2_backward_nhwc(P(self.act[i]), P(g), n, h, w, c, dt, P(self.grad[i]), self.stream))

    def same_bytes(self):
        pairs = [('y', self.c_y, self.act[-1]), ('dx', self.c_dx, self.grad[0])]
        for i, l in enumerate(self.layers):
            if l.get('tap'):
                pairs.append(('tap %s' % l['name'], self.c_taps[i], self.act[i + 1]))
            if l['kind'] == 'conv':
                pairs.append(('dw %s' % l['name'], self.c_dw[i], self.o_dw[i]))
                pairs.append(('db %s' % l['name'], self.c_db[i], self.o_db[i]))
        return {name: bool(torch.equal(a, b)) for name, a, b in pairs}

    def min_traffic(self):
        """{kernel: least bytes one forward + backward moves through it}, from the shapes (csrc/conv_chain.hip)"""
        halo = lambda n, h, w, p: ((n * (h + p) + p) * (w + p) + p)
        out = dict.fromkeys(NEW_KERNELS, 0)
        pads = [(l['k'] - 1) * l['dilation'] // 2 if l['kind'] == 'conv' else 1 for l in self.layers]
        for i, l in enumerate(self.layers):
            n, h, w, c = self.ins[i]
            e_in = n * h * w * c
            e_out = int(np.prod(self.shapes[i]))
            last = i == self.L - 1
            if l['kind'] == 'pool':
                out['chain_pool_bwd_kernel'] += 2 * e_in + 2 * e_out + 2 * e_in
            else:
                cop = -(-l['cout'] // 64) * 64
                rows = -(-halo(n, h, w, pads[i]) // 32) * 32
                out['chain_join_kernel'] += (4 if last else 2) * e_out + 2 * e_out + (4 * e_out if l.get('tap') else 0) + 2 * rows * cop
                if not last and pads[i + 1] != 1:          # the forward's re-halo copy
                    out['chain_join_kernel'] += 2 * e_out + 2 * e_out
            if not last and self.layers[i + 1]['kind'] == 'conv' and (l['kind'] == 'pool' or pads[i + 1] == 1):
                p = pads[i + 1]
                n2, h2, w2, c2 = self.shapes[i]
                guard = -(-(p * (w2 + p) + p) // 2) * 2
                rows = -(-halo(n2, h2, w2, p) // 32) * 32 + 2 * guard
                out['chain_zero_kernel'] += 2 * c2 * (rows - n2 * h2 * w2)
        return out


def measure(a, variant, dev):
    B = Body(variant, a.batch, a.size, a.dtype, dev)
    runs = {'chain_fwd': B.chain_fwd, 'ops_fwd': B.ops_fwd, 'ops_fwd_convs': lambda: B.ops_fwd(pools=False), 'chain_bwd': B.chain_bwd,
            'ops_bwd': B.ops_bwd}
    for fn in runs.values():            # warm up every shape the timed windows use
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    same = B.same_bytes()
    t = {k: [] for k in runs}
    for _ in range(a.repeats):          # alternated: every repeat visits every run
        for k, fn in runs.items():
            t[k].append(window(fn, a.steps))
    src = torch.empty((256 << 20,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copy_us = statistics.median(window(lambda: dst.copy_(src), a.steps) for _ in range(a.repeats))
    gb_s = 2 * src.numel() / (copy_us * 1e-6) / 1e9
    med = {k: statistics.median(v) for k, v in t.items()}
    row = dict(variant=variant, batch=a.batch, size=a.size, dtype=a.dtype, steps=a.steps, repeats=a.repeats, layers=B.L,
               workspace_mb=round(B.ws_bytes / 2 ** 20, 1), all_same_bytes=all(same.values()), differing=[k for k, v in same.items() if not v],
               copy_gb_s=round(gb_s, 1))
    for k in runs:
        row[k + '_us'] = round(med[k], 1)
        row[k + '_spread'] = round((max(t[k]) - min(t[k])) / med[k], 3)
    row['fwd_ops_convs_over_chain'] = round(med['ops_fwd_convs'] / med['chain_fwd'], 2)
    row['fwd_ops_over_chain'] = round(med['ops_fwd'] / med['chain_fwd'], 2)
    row['bwd_ops_over_chain'] = round(med['ops_bwd'] / med['chain_bwd'], 2)
    row['min_traffic'] = {k: dict(mb=round(v / 1e6, 1), copy_us=round(v / (gb_s * 1e9) * 1e6, 1)) for k, v in B.min_traffic().items()}
    return row


def fold_trace(path, calls):
    """{kernel name up to its template arguments: microseconds per forward + backward call} of a rocprofv3 kernel trace"""
    per = {}
    with open(path, newline='') as fh:
        for r in csv.DictReader(fh):
            name = r['Kernel_Name'].replace('(anonymous namespace)::', '').replace('void ', '').replace('ron::', '')
            name = name.split('(')[0].split('<')[0].strip()
            per[name] = per.get(name, 0.0) + (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    return {k: round(v / calls, 1) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=320)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--variants', default='reducedfc,full')
    ap.add_argument('--calls', type=int, default=0, help='only this many forward + backward calls of the chain (for a kernel trace)')
    ap.add_argument('--trace', default=None, help='a rocprofv3 kernel-trace CSV of a --calls run: print microseconds per call per kernel')
    ap.add_argument('--out', default=None, help='directory for conv_chain_bs<batch>.json')
    a = ap.parse_args(argv)
    if a.trace:
        print(json.dumps(dict(calls=a.calls, kernel_us_per_call=fold_trace(a.trace, a.calls))))
        return
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to report without one'
    dev = torch.device('cuda:0')
    rows = []
    for variant in a.variants.split(','):
        if a.calls:
            B = Body(variant, a.batch, a.size, a.dtype, dev)
            for _ in range(a.calls):
                B.chain_fwd()
                B.chain_bwd()
            torch.cuda.synchronize()
            continue
        row = measure(a, variant, dev)
        print(json.dumps(row), flush=True)
        assert row['all_same_bytes'], 'the chain and the per-operator sequence differ: %s' % row['differing']
        rows.append(row)
        torch.cuda.empty_cache()
    if a.out and rows:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'conv_chain_bs%d.json' % a.batch), 'w') as fh:
            for row in rows:
                fh.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
