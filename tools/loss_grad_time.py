#!/usr/bin/env python3
"""Time per call of ron_losses and ron_losses_grad on the same inputs, in one process: the RON-320 anchors at batch 32 with 21
classes, targets from ron_bboxes_encode.  The two entry points are called through ctypes with every argument built once (no Python
wrapper, no allocation inside the timed window); a window is `--steps` calls between two HIP events on one stream, the windows of
the two entries alternate, and the median over `--repeats` windows is reported with the smallest and the largest.  The forward in the
same run is the yardstick of the gradient call.

Bytes: the least traffic of the gradient call reads each head tensor once and writes each gradient once (rows * (C + 2 + 4) floats
each way); `hbm_share` is that over the time and over the 8.0 TB/s HBM peak.  The whole working set of this shape (about 150 MB) is
smaller than the 256 MiB Infinity Cache, so repeated calls need not go to HBM at all: the share says how far the call is from the
traffic bound, not what the HBM delivered.

`scale_pass_us` prices the alternative that was not built: unscaled gradients out of the forward's row pass and a scale pass over
them once the set sizes are known.  It is the time of that scale pass alone, stood in for by one in-place multiply of a flat tensor
of rows * (C + 6) floats by a device scalar (one streaming kernel, read + write), in the same alternation.

    python tools/loss_grad_time.py --out profiles/loss_grad/loss_grad_bs32.json
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import encode_cases as ec  # noqa: E402
import encode_ref as er  # noqa: E402
from oracle import synth  # noqa: E402
from ron_tensorflow_amd import _lib, ops  # noqa: E402
from ron_tensorflow_amd.nets.ron_vgg_320 import RONNet  # noqa: E402

HBM_PEAK = 8.0e12


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps            # microseconds per call


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--gt', type=int, default=8)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    n = a.batch
    net = RONNet(dtype='fp32', max_batch=1, device=dev)
    anchors = net.anchors((320, 320))
    adev = ops.anchors_to_device(anchors, dev)
    tab = er.AnchorTable(anchors, ec.RON_BORDERS, (320, 320))
    cls, obj, loc = ([torch.from_numpy(t).to(dev) for t in lst] for lst in synth.head_tensors(1, batch=n))
    num_classes = int(cls[0].shape[-1])
    objp = [ops.softmax_last(o, pick=1) for o in obj]
    gl, gb = ec.random_ground_truth(a.gt, n, a.gt)
    gcl, glo, _, _ = ops.bboxes_encode(torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev), adev, tab.shapes, (320, 320),
                                       ec.RON_BORDERS)
    rows = n * tab.total
    rnd = torch.rand((2, rows), device=dev)

    heads, keep = ops._fill_heads(cls, obj, loc, None, num_classes)
    tg, hg, objp_c = _lib.Targets(), _lib.HeadGrads(), (C.c_void_p * _lib.RON_MAX_LAYERS)()
    grads = [[torch.empty_like(t) for t in lst] for lst in (cls, obj, loc)]
    for i in range(len(cls)):
        objp_c[i], tg.gclasses[i], tg.glocalisations[i] = objp[i].data_ptr(), gcl[i].data_ptr(), glo[i].data_ptr()
        hg.d_cls[i], hg.d_obj[i], hg.d_loc[i] = grads[0][i].data_ptr(), grads[1][i].data_ptr(), grads[2][i].data_ptr()
    cfg = _lib.LossCfg(0.03, 3.0, 1. / 3, 1. / 3)
    lib = _lib.lib()
    nbytes = lib.ron_losses_grad_workspace_bytes(C.byref(heads), n)
    assert nbytes == lib.ron_losses_workspace_bytes(C.byref(heads), n) and nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = [(torch.empty((4,), dtype=torch.float32, device=dev), torch.empty((6,), dtype=torch.int32, device=dev)) for _ in range(2)]
    stream = _lib.current_stream()
    common = (C.byref(heads), objp_c, C.byref(tg), n, _lib.ptr(rnd[0]), _lib.ptr(rnd[1]), C.byref(cfg), _lib.ptr(ws), nbytes)

    def forward():
        _lib.check(lib.ron_losses(*common, _lib.ptr(out[0][0]), _lib.ptr(out[0][1]), stream))

    def gradient():
        _lib.check(lib.ron_losses_grad(*common, _lib.ptr(out[1][0]), _lib.ptr(out[1][1]), C.byref(hg), stream))

    flat = torch.zeros((rows * (num_classes + 6),), dtype=torch.float32, device=dev)
    one = torch.ones((), dtype=torch.float32, device=dev)

    def scale_pass():
        flat.mul_(one)

    for _ in range(a.warmup):
        forward()
        gradient()
        scale_pass()
    torch.cuda.synchronize()
    assert out[0][0].cpu().numpy().tobytes() == out[1][0].cpu().numpy().tobytes()          # the same losses, bit for bit
    assert torch.equal(out[0][1], out[1][1])
    t_fwd, t_grad, t_scale = [], [], []
    for _ in range(a.repeats):
        t_fwd.append(window(forward, a.steps))
        t_grad.append(window(gradient, a.steps))
        t_scale.append(window(scale_pass, a.steps))
    fwd, grad = statistics.median(t_fwd), statistics.median(t_grad)
    floats = rows * (num_classes + 2 + 4)
    min_bytes = 2 * 4 * floats
    counts = out[1][1].cpu().numpy().tolist()
    row = dict(what='ron_losses_grad vs ron_losses', batch=n, rows=rows, num_classes=num_classes, gt=a.gt, steps=a.steps,
               repeats=a.repeats, counts=dict(zip(ops.LOSS_COUNTS, counts)),
               ron_losses_us=round(fwd, 2), ron_losses_us_range=[round(min(t_fwd), 2), round(max(t_fwd), 2)],
               ron_losses_grad_us=round(grad, 2), ron_losses_grad_us_range=[round(min(t_grad), 2), round(max(t_grad), 2)],
               ratio=round(grad / fwd, 3), gradient_pass_us=round(grad - fwd, 2),
               scale_pass_us=round(statistics.median(t_scale), 2), min_bytes=min_bytes,
               hbm_share_of_call=round(min_bytes / (grad * 1e-6) / HBM_PEAK, 4),
               hbm_share_of_gradient_pass=round(min_bytes / (max(grad - fwd, 1e-3) * 1e-6) / HBM_PEAK, 4))
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(row) + '\n')
    del keep


if __name__ == '__main__':
    main()
