#!/usr/bin/env python3
"""Time of the four chains of each reverse-connection module of RON-320 (nets.ron_vgg_320.head_chains: left, objness, cls, reg at
40^2, 20^2, 10^2 and 5^2, 21 classes, 10 anchors), forward and backward, as ONE head chain (ron_head_chain_forward /
ron_head_chain_backward) beside the per-operator sequence it replaces, in one process: 320 x 320, batch 32, bf16.

Both are called through ctypes with every argument built once.  The per-operator sequence is what chaining ops.conv2d_nhwc_fn,
ops.batchnorm_nhwc_fn and torch.cat executes: ron_conv2d_forward_nhwc and ron_batchnorm_train_nhwc layer by layer forward (a pair:
two convolutions and torch.cat); ron_batchnorm_backward_nhwc and ron_conv2d_backward_nhwc in reverse order backward (a pair: the two
channel slices of the gradient made contiguous, two convolution backwards, and the fp32 add of the two data gradients).  It is
unchanged code, so it is the yardstick taken on the same box in the same run.

A window is `--steps` calls between two HIP events on one stream; chain and sequence windows alternate; the median over `--repeats`
windows is reported with the spread (max - min) / median.  The equality assertion of tests/test_gpu_head_chain.py is repeated at the
size that is timed (one forward + backward of each from the same moving statistics): y, mean, var, the moving statistics, dx and
every parameter gradient, torch.equal.

`copy_gb_s` is a device-to-device copy of 256 MiB (bytes read + bytes written over time); `min_traffic` lists, per batch-normalisation
kernel, the least bytes its launches of one forward + backward of ALL sixteen chains must move, computed from the shapes (2 bytes per
element of a halo tensor); copy_us = those bytes at the copy's rate (`--scales 40` keeps one scale, for both).  The kernels' own times come from a kernel trace of `--calls N`
(N forward + backward calls of every chain and nothing else, under rocprofv3 --kernel-trace in a run of its own), folded into the
table by `--trace CSV --calls N`.

    python tools/head_chain_time.py --out profiles/head_chain
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
from ron_tensorflow_amd.nets.ron_vgg_320 import head_chains  # noqa: E402

BN_KERNELS = ('bn_stats_kernel', 'bn_apply_kernel', 'bn_bwd_sums_kernel', 'bn_bwd_dx_kernel')
SCALES = (('block4', 40, 512), ('block5', 20, 512), ('block6', 10, 1024), ('block7', 5, 512))      # (layer, map side, the left chain's input channels)
GRADS = {'w': 'dw', 'bias': 'dbias', 'w2': 'dw2', 'bias2': 'dbias2', 'gamma': 'dgamma', 'beta': 'dbeta'}


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


class Chain(object):
    """The tensors and the prepared calls of one chain."""

    def __init__(self, layers, n, hw, cin, dtype, dev):
        self.layers, self.n, self.hw, self.cin, self.dtype = layers, n, hw, cin, dtype
        L = self.L = len(layers)
        g = torch.Generator(device=dev).manual_seed(1)
        rand = lambda *s: torch.randn(s, device=dev, generator=g)
        new = lambda s: torch.empty(tuple(s), dtype=torch.float32, device=dev)
        self.shapes = ops.head_chain_shapes(n, hw, hw, cin, layers, dtype)
        self.ins = [(n, hw, hw, cin)] + self.shapes[:-1]
        self.x = torch.relu(rand(n, hw, hw, cin))
        self.dy = rand(*self.shapes[-1])
        self.p, self.init = [], []
        for i, l in enumerate(layers):
            c = self.ins[i][3]
            if l['kind'] == 'bn':
                p = {'gamma': 1.0 + 0.2 * rand(c).clamp(-1, 1), 'beta': 0.1 * rand(c), 'moving_mean': rand(c), 'moving_var': rand(c).abs() + 0.5}
            else:
                p = {'w': rand(3, 3, c, l['cout']) * float(np.sqrt(2.0 / (9 * c)))}
                if l.get('bias', True):
                    p['bias'] = rand(l['cout']) * 0.1
                if l['kind'] == 'pair':
                    p['w2'] = rand(1, 1, c, l['cout2']) * float(np.sqrt(2.0 / c))
                    p['bias2'] = rand(l['cout2']) * 0.1
            self.p.append(p)
            self.init.append({k: v.clone() for k, v in p.items() if k.startswith('moving')})
        lib = self.lib = _lib.lib()
        self.stream = _lib.current_stream()
        # ---- the chain
        self.c_y, self.c_dx = new(self.shapes[-1]), new(self.x.shape)
        self.c_stats = [(new((self.ins[i][3],)), new((self.ins[i][3],))) if l['kind'] == 'bn' else None for i, l in enumerate(layers)]
        self.c_grads = [{GRADS[k]: new(v.shape) for k, v in p.items() if k in GRADS} for p in self.p]
        col = lambda name: [p.get(name) for p in self.p]
        self.d = ops._head_chain_desc(n, hw, hw, cin, layers, dtype)
        self.ws_bytes = lib.ron_head_chain_workspace_bytes(C.byref(self.d))
        assert self.ws_bytes > 0, lib.ron_last_error().decode()
        self.ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=dev)
        self.table = ops._head_ptrs(L, mean=[None if s is None else s[0] for s in self.c_stats], var=[None if s is None else s[1] for s in self.c_stats],
                                    **{name: col(name) for name in ('w', 'bias', 'w2', 'bias2', 'gamma', 'beta', 'moving_mean', 'moving_var')},
                                    **{g_: [gr.get(g_) for gr in self.c_grads] for g_ in GRADS.values()})
        # ---- the per-operator sequence, on moving statistics of its own
        self.o_moving = [{k: v.clone() for k, v in m.items()} for m in self.init]
        self.act = [self.x] + [new(s) for s in self.shapes]
        self.grad = [new(s) for s in self.ins] + [self.dy]
        self.o_stats = [(new((self.ins[i][3],)), new((self.ins[i][3],))) if l['kind'] == 'bn' else None for i, l in enumerate(layers)]
        self.o_grads = [{k: torch.empty_like(v) for k, v in gr.items()} for gr in self.c_grads]
        self.descs, self.tmp = [None] * L, [None] * L
        nbytes = 0
        for i, l in enumerate(layers):
            n_, h, w, c = self.ins[i]
            if l['kind'] == 'bn':
                d = _lib.BnDesc(n_, h, w, c, _lib.DTYPES[dtype], int(l['relu']), l['eps'], l['decay'])
                nbytes = max(nbytes, lib.ron_batchnorm_workspace_bytes(C.byref(d)))
                self.descs[i] = d
                continue
            cd = lambda k, cout: _lib.ConvDesc(n_, h, w, c, cout, k, k, 1, 1, int(l['relu']), 0, _lib.DTYPES[dtype], -1, 0, 0, 0, -1, 0)
            ds = [cd(3, l['cout'])] + ([cd(1, l['cout2'])] if l['kind'] == 'pair' else [])
            for d in ds:
                nbytes = max(nbytes, lib.ron_conv2d_forward_workspace_bytes(C.byref(d)), lib.ron_conv2d_backward_workspace_bytes(C.byref(d)))
            self.descs[i] = ds
            if l['kind'] == 'pair':          # the two branches' outputs, gradient slices and data gradients
                self.tmp[i] = dict(ya=new((n_, h, w, l['cout'])), yb=new((n_, h, w, l['cout2'])), ga=new((n_, h, w, l['cout'])),
                                   gb=new((n_, h, w, l['cout2'])), dxa=new(self.ins[i]), dxb=new(self.ins[i]))
        self.ows = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

    def reset_moving(self):
        for p, m, o in zip(self.p, self.init, self.o_moving):
            for k, v in m.items():
                p[k].copy_(v)
                o[k].copy_(v)

    def chain_fwd(self):
        _lib.check(self.lib.ron_head_chain_forward(C.byref(self.d), _lib.ptr(self.x), self.table, _lib.ptr(self.c_y), _lib.ptr(self.ws), self.ws_bytes,
                                                   self.stream))

    def chain_bwd(self):
        _lib.check(self.lib.ron_head_chain_backward(C.byref(self.d), _lib.ptr(self.dy), self.table, _lib.ptr(self.c_dx), _lib.ptr(self.ws),
                                                    self.ws_bytes, self.stream))

    def ops_fwd(self):
        P, lib, nb = _lib.ptr, self.lib, int(self.ows.numel())
        for i, l in enumerate(self.layers):
            p, x, y = self.p[i], self.act[i], self.act[i + 1]
            if l['kind'] == 'bn':
                m = self.o_moving[i]
                _lib.check(lib.ron_batchnorm_train_nhwc(C.byref(self.descs[i]), P(x), P(p['gamma']), P(p['beta']), P(y), P(self.o_stats[i][0]),
                                                        P(self.o_stats[i][1]), P(m['moving_mean']), P(m['moving_var']), P(self.ows), nb, self.stream))
            elif l['kind'] == 'conv':
                _lib.check(lib.ron_conv2d_forward_nhwc(C.byref(self.descs[i][0]), P(x), P(p['w']), P(p.get('bias')), P(y), P(self.ows), nb, self.stream))
            else:
                t = self.tmp[i]
                _lib.check(lib.ron_conv2d_forward_nhwc(C.byref(self.descs[i][0]), P(x), P(p['w']), P(p['bias']), P(t['ya']), P(self.ows), nb, self.stream))
                _lib.check(lib.ron_conv2d_forward_nhwc(C.byref(self.descs[i][1]), P(x), P(p['w2']), P(p['bias2']), P(t['yb']), P(self.ows), nb, self.stream))
                torch.cat([t['ya'], t['yb']], -1, out=y)

    def ops_bwd(self):
        P, lib, nb = _lib.ptr, self.lib, int(self.ows.numel())
        for i in reversed(range(self.L)):
            l, p, gr = self.layers[i], self.p[i], self.o_grads[i]
            x, y, g, dx = self.act[i], self.act[i + 1], self.grad[i + 1], self.grad[i]
            if l['kind'] == 'bn':
                _lib.check(lib.ron_batchnorm_backward_nhwc(C.byref(self.descs[i]), P(x), P(y), P(g), P(p['gamma']), P(self.o_stats[i][0]),
                                                           P(self.o_stats[i][1]), P(dx), P(gr['dgamma']), P(gr['dbeta']), P(self.ows), nb, self.stream))
            elif l['kind'] == 'conv':
                _lib.check(lib.ron_conv2d_backward_nhwc(C.byref(self.descs[i][0]), P(x), P(p['w']), P(y), P(g), P(dx), P(gr['dw']), P(gr.get('dbias')),
                                                        P(self.ows), nb, self.stream))
            else:
                t, ca = self.tmp[i], l['cout']
                t['ga'].copy_(g[..., :ca])
                t['gb'].copy_(g[..., ca:])
                _lib.check(lib.ron_conv2d_backward_nhwc(C.byref(self.descs[i][0]), P(x), P(p['w']), P(t['ya']), P(t['ga']), P(t['dxa']), P(gr['dw']),
                                                        P(gr['dbias']), P(self.ows), nb, self.stream))
                _lib.check(lib.ron_conv2d_backward_nhwc(C.byref(self.descs[i][1]), P(x), P(p['w2']), P(t['yb']), P(t['gb']), P(t['dxb']), P(gr['dw2']),
                                                        P(gr['dbias2']), P(self.ows), nb, self.stream))
                torch.add(t['dxa'], t['dxb'], out=dx)

    def same_bytes(self):
        """One forward + backward of each from the same moving statistics: {output: equal}"""
        self.reset_moving()
        self.chain_fwd(); self.chain_bwd(); self.ops_fwd(); self.ops_bwd()
        torch.cuda.synchronize()
        pairs = [('y', self.c_y, self.act[-1]), ('dx', self.c_dx, self.grad[0])]
        for i, l in enumerate(self.layers):
            if l['kind'] == 'bn':
                pairs += [('mean %d' % i, self.c_stats[i][0], self.o_stats[i][0]), ('var %d' % i, self.c_stats[i][1], self.o_stats[i][1])]
                pairs += [('%s %d' % (k, i), self.p[i][k], self.o_moving[i][k]) for k in ('moving_mean', 'moving_var')]
            pairs += [('%s %d' % (k, i), v, self.o_grads[i][k]) for k, v in self.c_grads[i].items()]
        return {name: bool(torch.equal(a, b)) for name, a, b in pairs}

    def min_traffic(self):
        """{kernel: least bytes one forward + backward moves through it}: 2 bytes per element read or written (csrc/batchnorm.hip)"""
        out = dict.fromkeys(BN_KERNELS, 0)
        for i, l in enumerate(self.layers):
            if l['kind'] == 'bn':
                e = int(np.prod(self.ins[i]))
                mask = 1 if l['relu'] else 0
                out['bn_stats_kernel'] += 2 * e
                out['bn_apply_kernel'] += 2 * e + 2 * e
                out['bn_bwd_sums_kernel'] += 2 * e * (2 + mask)
                out['bn_bwd_dx_kernel'] += 2 * e * (2 + mask) + 2 * e
        return out


def chains_of(a, dev):
    out = []
    for layer, hw, left_c in SCALES:
        if a.scales and str(hw) not in a.scales.split(','):
            continue
        hc = head_chains(10, a.classes, layer, top=layer == 'block7')
        for key in ('left', 'objness', 'cls', 'reg'):
            out.append(('%s %d^2' % (key, hw), Chain(hc[key][0], a.batch, hw, left_c if key == 'left' else 512, a.dtype, dev)))
    return out


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
    ap.add_argument('--classes', type=int, default=21)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--scales', default='', help='map sides to keep, e.g. 40 or 40,20 (default: all four)')
    ap.add_argument('--calls', type=int, default=0, help='only this many forward + backward calls of every chain (for a kernel trace)')
    ap.add_argument('--trace', default=None, help='a rocprofv3 kernel-trace CSV of a --calls run: print microseconds per call per kernel')
    ap.add_argument('--out', default=None, help='directory for head_chain_bs<batch>.json')
    a = ap.parse_args(argv)
    if a.trace:
        print(json.dumps(dict(calls=a.calls, kernel_us_per_call=fold_trace(a.trace, a.calls))))
        return
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is nothing to report without one'
    dev = torch.device('cuda:0')
    chains = chains_of(a, dev)
    if a.calls:
        for _ in range(a.calls):
            for _, ch in chains:
                ch.chain_fwd()
                ch.chain_bwd()
        torch.cuda.synchronize()
        return
    src = torch.empty((256 << 20,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copy_us = statistics.median(window(lambda: dst.copy_(src), a.steps) for _ in range(a.repeats))
    gb_s = 2 * src.numel() / (copy_us * 1e-6) / 1e9
    del src, dst
    rows, traffic = [], dict.fromkeys(BN_KERNELS, 0)
    for name, ch in chains:
        same = ch.same_bytes()
        runs = {'chain_fwd': ch.chain_fwd, 'ops_fwd': ch.ops_fwd, 'chain_bwd': ch.chain_bwd, 'ops_bwd': ch.ops_bwd}
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for _ in range(a.repeats):          # alternated: every repeat visits every run
            for k, fn in runs.items():
                t[k].append(window(fn, a.steps))
        med = {k: statistics.median(v) for k, v in t.items()}
        row = dict(chain=name, batch=a.batch, dtype=a.dtype, steps=a.steps, repeats=a.repeats, layers=ch.L, workspace_mb=round(ch.ws_bytes / 2 ** 20, 1),
                   all_same_bytes=all(same.values()), differing=[k for k, v in same.items() if not v])
        for k in runs:
            row[k + '_us'] = round(med[k], 1)
            row[k + '_spread'] = round((max(t[k]) - min(t[k])) / med[k], 3)
        row['fwd_ops_over_chain'] = round(med['ops_fwd'] / med['chain_fwd'], 2)
        row['bwd_ops_over_chain'] = round(med['ops_bwd'] / med['chain_bwd'], 2)
        print(json.dumps(row), flush=True)
        assert row['all_same_bytes'], 'the chain and the per-operator sequence differ: %s' % row['differing']
        rows.append(row)
        for k, v in ch.min_traffic().items():
            traffic[k] += v
    total = dict(chain='all %d' % len(rows), copy_gb_s=round(gb_s, 1),
                 min_traffic={k: dict(mb=round(v / 1e6, 1), copy_us=round(v / (gb_s * 1e9) * 1e6, 1)) for k, v in traffic.items()})
    for k in ('chain_fwd', 'ops_fwd', 'chain_bwd', 'ops_bwd'):
        total[k + '_us'] = round(sum(r[k + '_us'] for r in rows), 1)
    total['fwd_ops_over_chain'] = round(total['ops_fwd_us'] / total['chain_fwd_us'], 2)
    total['bwd_ops_over_chain'] = round(total['ops_bwd_us'] / total['chain_bwd_us'], 2)
    print(json.dumps(total), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, 'head_chain_bs%d.json' % a.batch), 'w') as fh:
            for row in rows + [total]:
                fh.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
