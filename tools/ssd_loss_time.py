#!/usr/bin/env python3
"""Time per call of ron_ssd_losses and ron_ssd_losses_grad beside two comparators, in one process:

  * SSD-300 at batch 32 (279 424 rows, one selection over the batch) and SSD-512 at batch 16 (393 024 rows, one selection per
    layer), 21 classes, random logits with a background offset, targets from ron_bboxes_encode (thresholds 0.5 / 0.5, no border)
    on `--gt` random boxes per image;
  * (a) ron_losses_grad on the RON-320 anchors at batch 32 (680 000 rows): the per-row scale of the existing loss path;
  * (b) a composition of the same formulas from torch operators on the GPU, what a user would write today: softmax, the k-th
    smallest value by torch.topk of the negated values (`torch_topk`: k is read back to the host, as topk needs a Python int) or by
    torch.sort and an index kept on the device (`torch_sort`: no host round trip), cross_entropy, and autograd for the gradients.
    The faster of the two is the comparator of the condition.

The entry points are called through ctypes with every argument built once; a window is `--steps` calls between two HIP events on one
stream, the windows of all candidates alternate, and the median over `--repeats` windows is reported with the smallest and largest.
The condition: each new call takes no longer than (b) of the same kind (losses only / losses and gradients), no margin beyond the
window spread: its largest window against the comparator's smallest.

    python tools/ssd_loss_time.py --out profiles/ssd_loss/ssd_loss.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import encode_cases as ec  # noqa: E402
import encode_ref as er  # noqa: E402
from oracle import synth  # noqa: E402
from ron_tensorflow_amd import _lib, ops  # noqa: E402
from ron_tensorflow_amd.nets import ssd_vgg_300, ssd_vgg_512  # noqa: E402
from ron_tensorflow_amd.nets.ron_vgg_320 import RONNet  # noqa: E402

SSD300_STEP_US = 1900.0          # the SSD-300 forward step at batch 32 the call would sit behind
NO_BORDER = 1 << 24


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps            # microseconds per call


def abs_smooth(d):
    a = d.abs()
    return 0.5 * ((a - 1) * torch.clamp(a, max=1.0) + a)


def torch_losses(logits, localisations, gclasses, glocalisations, gscores, mining, use_sort, match_threshold=0.5, negative_ratio=3.,
                 alpha=1.):
    """The same formulas from torch operators, segment by segment (the layers are concatenated for 'batch')."""
    n = logits[0].shape[0]
    C_ = logits[0].shape[-1]
    flat = lambda lst, w: [t.reshape(-1, w) if w else t.reshape(-1) for t in lst]
    x, s, g = flat(logits, C_), flat(gscores, 0), flat(gclasses, 0)
    lo, gl = flat(localisations, 4), flat(glocalisations, 4)
    if mining == 'batch':
        x, s, g, lo, gl = ([torch.cat(v)] for v in (x, s, g, lo, gl))
    total = [0., 0., 0.]
    for xi, si, gi, li, gli in zip(x, s, g, lo, gl):
        R = xi.shape[0]
        pmask = si > match_threshold
        nmask = ~pmask & (si > -0.5)
        fp, fn = pmask.to(xi.dtype), nmask.to(xi.dtype)
        n_pos = fp.sum()
        nvalues = torch.where(nmask, torch.softmax(xi.detach(), dim=1)[:, 0], 1. - fn)
        k = (negative_ratio * n_pos).to(torch.int32)
        n_cand = fn.sum().to(torch.int32)
        if mining == 'batch':
            k = torch.minimum(k + n, n_cand)
        else:
            k = torch.minimum(torch.clamp(k, min=max(R // 8, 4 * n)), 1 + n_cand)
        k = torch.clamp(k, max=R)
        if use_sort:
            ordered = torch.sort(nvalues).values
            t = ordered[torch.clamp(k - 1, min=0).long()]
            mined = nmask & (nvalues < t) & (k > 0)
        else:
            kk = int(k.item())
            if kk > 0:
                val, _ = torch.topk(-nvalues, kk)
                mined = nmask & (nvalues < -val[-1])
            else:
                mined = torch.zeros_like(nmask)
        fm = mined.to(xi.dtype)
        ce_pos = TF.cross_entropy(xi, torch.clamp(gi, min=0), reduction='none')
        ce_neg = TF.cross_entropy(xi, pmask.long(), reduction='none')
        sl = abs_smooth(li - gli).sum(dim=1)
        if mining == 'batch':
            total[0] = total[0] + (ce_pos * fp).sum() / n
            total[1] = total[1] + (ce_neg * fm).sum() / n
            total[2] = total[2] + alpha * (sl * fp).sum() / n
        else:
            total[0] = total[0] + (ce_pos * fp).sum() / torch.clamp(n_pos, min=1)
            total[1] = total[1] + (ce_neg * fm).sum() / torch.clamp(fm.sum(), min=1)
            total[2] = total[2] + alpha * (sl * fp).sum() / torch.clamp(4 * n_pos, min=1)
    return torch.stack([total[0], total[1], total[2], total[0] + total[1] + total[2]])


def ssd_setup(dev, mod, size, n, gt, num_classes=21):
    net = mod.SSDNet(dtype='fp32', max_batch=1, device=dev)
    anchors = net.anchors((size, size))
    adev = ops.anchors_to_device(anchors, dev)
    shapes = [(int(y.shape[0]), int(y.shape[1]), int(np.size(h))) for (y, x, h, w) in anchors]
    gl, gb = ec.random_ground_truth(gt, n, gt)
    gcl, glo, gsc, _ = ops.bboxes_encode(torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev), adev, shapes, (size, size),
                                         [NO_BORDER] * len(shapes), 0.5, 0.5)
    gen = torch.Generator(device=dev).manual_seed(size)
    cls, loc = [], []
    for (fh, fw, a) in shapes:
        c = torch.randn((n, fh, fw, a, num_classes), device=dev, generator=gen) * 2.0
        c[..., 0] += 4.0
        cls.append(c)
        loc.append(torch.randn((n, fh, fw, a, 4), device=dev, generator=gen))
    return dict(mining=net._mining, n=n, logits=cls, localisations=loc, gclasses=gcl, glocalisations=glo, gscores=gsc,
                rows=sum(int(t.numel()) for t in gcl), num_classes=num_classes)


def ssd_entries(d, dev):
    """(forward, gradient, outputs): the two C entries on arguments built once."""
    lib = _lib.lib()
    heads, keep = ops._fill_heads(d['logits'], None, d['localisations'], None, d['num_classes'])
    tg, hg = _lib.Targets(), _lib.HeadGrads()
    grads = [[torch.empty_like(t) for t in lst] for lst in (d['logits'], d['localisations'])]
    for i in range(len(d['logits'])):
        tg.gclasses[i], tg.glocalisations[i], tg.gscores[i] = (d[k][i].data_ptr() for k in ('gclasses', 'glocalisations', 'gscores'))
        hg.d_cls[i], hg.d_loc[i] = grads[0][i].data_ptr(), grads[1][i].data_ptr()
    cfg = _lib.SsdLossCfg(ops.SSD_MINING[d['mining']], 0.5, 3.0, 1.0)
    nbytes = lib.ron_ssd_losses_grad_workspace_bytes(C.byref(heads), d['n'])
    assert nbytes == lib.ron_ssd_losses_workspace_bytes(C.byref(heads), d['n']) and nbytes > 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    segs = 1 if d['mining'] == 'batch' else len(d['logits'])
    out = [(torch.empty((4,), dtype=torch.float32, device=dev), torch.empty((segs, 4), dtype=torch.int32, device=dev)) for _ in range(2)]
    stream = _lib.current_stream()
    common = (C.byref(heads), C.byref(tg), d['n'], C.byref(cfg), _lib.ptr(ws), nbytes)

    def forward():
        _lib.check(lib.ron_ssd_losses(*common, _lib.ptr(out[0][0]), _lib.ptr(out[0][1]), None, stream))

    def gradient():
        _lib.check(lib.ron_ssd_losses_grad(*common, _lib.ptr(out[1][0]), _lib.ptr(out[1][1]), None, C.byref(hg), stream))

    return forward, gradient, out, (keep, tg, hg, grads, ws, cfg, heads)


def ron_entry(dev, n, gt):
    """(a): ron_losses_grad on the RON-320 anchors, as tools/loss_grad_time.py calls it."""
    lib = _lib.lib()
    net = RONNet(dtype='fp32', max_batch=1, device=dev)
    anchors = net.anchors((320, 320))
    adev = ops.anchors_to_device(anchors, dev)
    tab = er.AnchorTable(anchors, ec.RON_BORDERS, (320, 320))
    cls, obj, loc = ([torch.from_numpy(t).to(dev) for t in lst] for lst in synth.head_tensors(1, batch=n))
    objp = [ops.softmax_last(o, pick=1) for o in obj]
    gl, gb = ec.random_ground_truth(gt, n, gt)
    gcl, glo, _, _ = ops.bboxes_encode(torch.from_numpy(gl).to(dev), torch.from_numpy(gb).to(dev), adev, tab.shapes, (320, 320),
                                       ec.RON_BORDERS)
    rows = n * tab.total
    rnd = torch.rand((2, rows), device=dev)
    heads, keep = ops._fill_heads(cls, obj, loc, None, int(cls[0].shape[-1]))
    tg, hg, objp_c = _lib.Targets(), _lib.HeadGrads(), (C.c_void_p * _lib.RON_MAX_LAYERS)()
    grads = [[torch.empty_like(t) for t in lst] for lst in (cls, obj, loc)]
    for i in range(len(cls)):
        objp_c[i], tg.gclasses[i], tg.glocalisations[i] = objp[i].data_ptr(), gcl[i].data_ptr(), glo[i].data_ptr()
        hg.d_cls[i], hg.d_obj[i], hg.d_loc[i] = grads[0][i].data_ptr(), grads[1][i].data_ptr(), grads[2][i].data_ptr()
    cfg = _lib.LossCfg(0.03, 3.0, 1. / 3, 1. / 3)
    nbytes = lib.ron_losses_grad_workspace_bytes(C.byref(heads), n)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = (torch.empty((4,), dtype=torch.float32, device=dev), torch.empty((6,), dtype=torch.int32, device=dev))
    stream = _lib.current_stream()

    def gradient():
        _lib.check(lib.ron_losses_grad(C.byref(heads), objp_c, C.byref(tg), n, _lib.ptr(rnd[0]), _lib.ptr(rnd[1]), C.byref(cfg),
                                       _lib.ptr(ws), nbytes, _lib.ptr(out[0]), _lib.ptr(out[1]), C.byref(hg), stream))

    return gradient, rows, (keep, tg, hg, objp_c, grads, ws, cfg, heads, objp, gcl, glo, rnd, out)


def measure(cands, steps, warmup, repeats):
    """cands: {name: (fn, steps divisor)}; alternating windows; {name: (median, smallest, largest)} in microseconds."""
    for fn, _ in cands.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(repeats):
        for k, (fn, div) in cands.items():
            times[k].append(window(fn, max(steps // div, 10)))
    return {k: (round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)) for k, v in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gt', type=int, default=8)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    rows_out = []
    ron_grad, ron_rows, ron_keep = ron_entry(dev, 32, a.gt)
    for what, mod, size, n in (('ssd300_bs32_batch', ssd_vgg_300, 300, 32), ('ssd512_bs16_layer', ssd_vgg_512, 512, 16)):
        d = ssd_setup(dev, mod, size, n, a.gt)
        forward, gradient, out, keep = ssd_entries(d, dev)
        leaf = dict(d)
        leaf['logits'] = [t.clone().requires_grad_(True) for t in d['logits']]
        leaf['localisations'] = [t.clone().requires_grad_(True) for t in d['localisations']]
        targs = lambda dd: (dd['logits'], dd['localisations'], dd['gclasses'], dd['glocalisations'], dd['gscores'], dd['mining'])
        res = {}

        def torch_fwd(use_sort):
            with torch.no_grad():
                res['fwd_sort' if use_sort else 'fwd_topk'] = torch_losses(*targs(d), use_sort)

        def torch_grad(use_sort):
            for t in leaf['logits'] + leaf['localisations']:
                t.grad = None
            torch_losses(*targs(leaf), use_sort)[3].backward()

        cands = {'ron_ssd_losses': (forward, 1), 'ron_ssd_losses_grad': (gradient, 1), 'ron_losses_grad_ron320_bs32': (ron_grad, 1),
                 'torch_topk_losses': (lambda: torch_fwd(False), 10), 'torch_sort_losses': (lambda: torch_fwd(True), 10),
                 'torch_topk_losses_and_grad': (lambda: torch_grad(False), 10), 'torch_sort_losses_and_grad': (lambda: torch_grad(True), 10)}
        t = measure(cands, a.steps, a.warmup, a.repeats)
        # the values behind the times: the two entries agree bit for bit, the composition within float32 accumulation of them
        assert out[0][0].cpu().numpy().tobytes() == out[1][0].cpu().numpy().tobytes() and torch.equal(out[0][1], out[1][1])
        ours = out[0][0].cpu().numpy()
        agree = {k: [float(x) for x in v.cpu().numpy()] for k, v in res.items()}
        b_fwd = min(('torch_topk_losses', 'torch_sort_losses'), key=lambda k: t[k][0])
        b_grad = min(('torch_topk_losses_and_grad', 'torch_sort_losses_and_grad'), key=lambda k: t[k][0])
        row = dict(what=what, mining=d['mining'], batch=n, rows=d['rows'], num_classes=d['num_classes'], gt=a.gt, steps=a.steps,
                   repeats=a.repeats, counts=out[0][1].cpu().numpy().tolist(), losses=[float(x) for x in ours], torch_losses=agree,
                   us={k: dict(median=v[0], smallest=v[1], largest=v[2]) for k, v in t.items()},
                   comparator_losses=b_fwd, comparator_losses_and_grad=b_grad,
                   condition_losses=bool(t['ron_ssd_losses'][2] <= t[b_fwd][1]),
                   condition_losses_and_grad=bool(t['ron_ssd_losses_grad'][2] <= t[b_grad][1]),
                   grad_call_vs_torch_losses_only=bool(t['ron_ssd_losses_grad'][2] <= t[b_fwd][1]),
                   us_per_1000_rows=dict(ron_ssd_losses_grad=round(t['ron_ssd_losses_grad'][0] / d['rows'] * 1e3, 4),
                                         ron_losses_grad_ron320=round(t['ron_losses_grad_ron320_bs32'][0] / ron_rows * 1e3, 4)),
                   share_of_ssd300_step=dict(ron_ssd_losses=round(t['ron_ssd_losses'][0] / SSD300_STEP_US, 4),
                                             ron_ssd_losses_grad=round(t['ron_ssd_losses_grad'][0] / SSD300_STEP_US, 4)))
        print(json.dumps(row), flush=True)
        rows_out.append(row)
        del keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            for row in rows_out:
                fh.write(json.dumps(row) + '\n')
    del ron_keep


if __name__ == '__main__':
    main()
