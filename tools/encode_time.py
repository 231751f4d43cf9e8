#!/usr/bin/env python3
"""Time per call of the label side at the RON-320 anchors: ron_bboxes_encode and ron_losses through their Python wrappers
(warm-up, then HIP events around repeated calls on one stream, bench.py's method), the numpy reference of tests/encode_ref.py for
the same work on the host, and one ron_post_tfe call on head tensors of the same batch for scale.  One JSON line per row.

    python tools/encode_time.py --batch 32 --gt 8,64 --out profiles/encode/encode_losses_bs32.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import encode_cases as ec  # noqa: E402
import encode_ref as er  # noqa: E402
from oracle import synth  # noqa: E402
from ron_tensorflow_amd import ops, tfe  # noqa: E402
from ron_tensorflow_amd.nets.ron_vgg_320 import RONNet  # noqa: E402


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
    ap.add_argument('--gt', default='8,64')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    n = a.batch
    net = RONNet(dtype='fp32', max_batch=1, device=dev)
    anchors = net.anchors((320, 320))
    adev = ops.anchors_to_device(anchors, dev)
    tab = er.AnchorTable(anchors, ec.RON_BORDERS, (320, 320))
    cls, obj, loc = ([torch.from_numpy(t).to(dev) for t in lst] for lst in synth.head_tensors(1, batch=n))
    objp = [ops.softmax_last(o, pick=1) for o in obj]
    rows = []
    post_ms = time_gpu(lambda: tfe.post_tfe(cls, obj, loc, adev, objectness_thres=0.03, min_size=0.03, cls_is_prob=False,
                                            obj_is_prob=False, loc_decoded=False, select_threshold=0.01, nms_threshold=0.4,
                                            clipping_bbox=[0., 0., 1., 1.], top_k=200, keep_top_k=100), a.steps, a.warmup)
    rows.append(dict(what='ron_post_tfe', batch=n, ms=round(post_ms, 4)))
    for g in [int(v) for v in a.gt.split(',')]:
        gl, gb = ec.random_ground_truth(g, n, g)
        d_gl, d_gb = torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev)
        enc = lambda: ops.bboxes_encode(d_gl, d_gb, adev, tab.shapes, (320, 320), ec.RON_BORDERS)
        enc_ms = time_gpu(enc, a.steps, a.warmup)
        gcl, glo, gsc, _ = enc()
        rnd = torch.rand((2, n * tab.total), device=dev)
        loss_ms = time_gpu(lambda: ops.losses(cls, loc, obj, objp, gcl, glo, rnd[0], rnd[1]), a.steps, a.warmup)
        t0 = time.perf_counter()
        ref = er.encode_batch(gl, gb, tab)
        enc_np = (time.perf_counter() - t0) * 1e3
        f = er.flatten_rows
        fi = dict(logits=f([t.cpu().numpy() for t in cls], 21), localisations=f([t.cpu().numpy() for t in loc], 4),
                  objness_logits=f([t.cpu().numpy() for t in obj], 2), objness_pred=f([t.cpu().numpy() for t in objp]),
                  gclasses=f(ref[0]), glocalisations=f(ref[1], 4), rand_obj=rnd[0].cpu().numpy(), rand_cls=rnd[1].cpu().numpy())
        t0 = time.perf_counter()
        er.losses_ref(**fi)
        loss_np = (time.perf_counter() - t0) * 1e3
        counts = ops.losses(cls, loc, obj, objp, gcl, glo, rnd[0], rnd[1])[1].cpu().numpy().tolist()
        rows.append(dict(what='ron_bboxes_encode', batch=n, gt=g, anchors=tab.total, ms=round(enc_ms, 4), numpy_ms=round(enc_np, 1),
                         output_bytes_per_anchor=8 + 16 + 4 + 16))
        rows.append(dict(what='ron_losses', batch=n, gt=g, ms=round(loss_ms, 4), numpy_float64_ms=round(loss_np, 1), counts=counts))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            for r in rows:
                fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
