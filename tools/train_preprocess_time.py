#!/usr/bin/env python3
"""Time per call of the training preprocessing on the GPU: ron_train_geometry + ron_preprocess_train on an uploaded batch of
375 x 500 and 500 x 375 uint8 images with G ground-truth rows (warm-up, then HIP events around repeated calls on one stream,
bench.py's method; the median of several alternating repeats, with the spread), beside ron_preprocess_eval on the same batch - it
writes the same output bytes, so it is the yardstick - and the numpy reference of tests/train_pre_ref.py for the same work on the host.  One JSON line.

    python tools/train_preprocess_time.py --batch 32 --gt 8 --out profiles/train_preprocess/train_preprocess_bs32.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import train_pre_ref as tr  # noqa: E402
from encode_cases import random_ground_truth  # noqa: E402
from ron_tensorflow_amd import _lib  # noqa: E402
from ron_tensorflow_amd.preprocessing import ssd_vgg_preprocessing as pp  # noqa: E402


def time_gpu(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--gt', type=int, default=8)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    n, g, oh, ow = a.batch, a.gt, 320, 320
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, (375, 500, 3) if i % 2 == 0 else (500, 375, 3)).astype(np.uint8) for i in range(n)]
    gl, gb = random_ground_truth(3, n, g)
    draws = np.minimum(rs.uniform(0, 1, (n, tr.RON_TRAIN_DRAWS)).astype(np.float32), np.nextafter(np.float32(1), np.float32(0)))
    packed, d_off, d_hw = pp._pack(imgs, dev)
    d_gl, d_gb = torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev)
    geom = torch.empty((n, tr.RON_TRAIN_GEOM), dtype=torch.int32, device=dev)
    gl_out, gb_out = torch.empty_like(d_gl), torch.empty_like(d_gb)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    out = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)
    ws = torch.empty((lib.ron_preprocess_train_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    means = (C.c_float * 3)(*tr.MEANS)
    stream = _lib.current_stream()

    def geometry(d):
        _lib.check(lib.ron_train_geometry(_lib.ptr(d_hw), _lib.ptr(d_gl), _lib.ptr(d_gb), n, g, _lib.ptr(d), _lib.ptr(geom),
                                          _lib.ptr(gl_out), _lib.ptr(gb_out), _lib.ptr(counts), stream))

    def pixels():
        _lib.check(lib.ron_preprocess_train(_lib.ptr(packed), _lib.ptr(d_off), _lib.ptr(d_hw), _lib.ptr(geom), n, oh, ow, means,
                                            _lib.ptr(ws), _lib.ptr(out), stream))

    def evaluation():
        _lib.check(lib.ron_preprocess_eval(_lib.ptr(packed), _lib.ptr(d_off), _lib.ptr(d_hw), n, oh, ow, means, _lib.ptr(out), stream))

    row = dict(what='ron_preprocess_train', batch=n, gt=g, images='375x500 / 500x375 uint8', out='%dx%d' % (oh, ow), steps=a.steps,
               repeats=a.repeats, output_bytes=int(out.numel() * 4), source_bytes=int(packed.numel()))
    variants = []
    for name, d0 in (('train_ms', None), ('train_none_expanded_ms', 0.0), ('train_all_expanded_ms', 0.75)):
        d = draws.copy()
        if d0 is not None:
            d[:, 0] = d0
        variants.append((name, torch.from_numpy(d).to(dev)))
    d_random = variants[0][1]
    samples = {}
    for _ in range(a.repeats):                                        # the versions alternate inside every repeat
        samples.setdefault('eval_ms', []).append(time_gpu(evaluation, a.steps, a.warmup))
        for name, d_draws in variants:
            samples.setdefault(name, []).append(time_gpu(lambda: (geometry(d_draws), pixels()), a.steps, a.warmup))
        samples.setdefault('geometry_ms', []).append(time_gpu(lambda: geometry(d_random), a.steps, a.warmup))
        samples.setdefault('pixels_ms', []).append(time_gpu(pixels, a.steps, a.warmup))         # on the random draws' geometry
    for name, v in samples.items():
        row[name] = round(float(np.median(v)), 4)
        row[name + '_min_max'] = [round(min(v), 4), round(max(v), 4)]
    row['expanded_images'] = int(geom[:, 0].sum())
    row['kept_rows'] = int(counts.sum())
    row['train_over_eval'] = round(row['train_ms'] / row['eval_ms'], 3)
    row['train_over_eval_per_repeat'] = [round(t / e, 3) for t, e in zip(samples['train_ms'], samples['eval_ms'])]
    t0 = time.perf_counter()
    ref = tr.geometry_batch([im.shape[:2] for im in imgs], gl, gb, draws)
    for im, gm in zip(imgs, ref[0]):
        tr.pixels_ref(im, gm, (oh, ow))
    row['numpy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
