#!/usr/bin/env python3
"""Images/s and ms per batch of the TF-evaluation detection paths, synthetic weights, one stream:

  unfused : the reference driver's sequence (eval_ron_network.py:209-236): net -> bboxes_decode -> torch objectness gate ->
            detected_bboxes (ron_post_tfe)
  tfe     : RONNet.detect_tfe (ron_detect_tfe: forward + the same post-processing in one enqueue)
  np      : RONNet.detect (ron_detect, np_methods post-processing), for reference
  post_raw: (not in the default set) ron_post_tfe alone on the raw heads of one forward (tfe_select_kernel applies softmax, gate
            and decode): with a kernel trace, the one TF select kernel as ron_post_tfe and as ron_detect_tfe launch it, same heads

per variant (reducedfc / full), batch (1: the latency plan, 32) and regime: 'dense' = the synthetic weights as they are, 'biased'
= the Conv2d_pred_3x3 background bias raised (+10 instead of +8) so that the lists are sparse, like a trained net's.  Each
row also reports the regime's candidate density: the share of (anchor, class) pairs whose gated score passes select_threshold,
and the share of anchors the select kernel's early exit skips.  Prints a table and one JSON line per row.

    python tools/tfe_detect_time.py                                   # the full table
    python tools/tfe_detect_time.py --batches 1 --variants reducedfc --regimes dense --paths unfused,tfe,np,post_raw --steps 10
                                                                      # (a short run for a kernel trace)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ron_tensorflow_amd import ops, tfe  # noqa: E402
from ron_tensorflow_amd import weights as W  # noqa: E402
from ron_tensorflow_amd.nets import nets_factory  # noqa: E402

BG = {'dense': 8.0, 'biased': 10.0}
ARGS = dict(select_threshold=0.01, nms_threshold=0.4, clipping_bbox=[0., 0., 1., 1.], top_k=200, keep_top_k=100)
OBJ_THR = 0.03


def unfused(net, anchors, x):
    predictions, logits, objness_pred, objness_logits, localisations, _ = net.net(x, is_training=False, end_points=())
    localisations = net.bboxes_decode(localisations, anchors)
    gated = [(o > OBJ_THR).to(torch.float32) * predictions[k] for k, o in enumerate(objness_pred)]
    return net.detected_bboxes(gated, localisations, **ARGS)


def density(net, x):
    """(share of (anchor, class) pairs that pass, share of anchors the early exit skips) on the heads of `x`."""
    predictions, logits, objness_pred, _, _, _ = net.net(x, is_training=False, end_points=())
    nc = net.params.num_classes
    p = torch.cat([((o > OBJ_THR).to(torch.float32) * q).reshape(-1, nc)[:, 1:] for o, q in zip(objness_pred, predictions)])
    z = torch.cat([l.reshape(-1, nc) for l in logits])
    gap = z[:, 1:].max(-1).values - z.max(-1).values
    return float((p > ARGS['select_threshold']).float().mean()), float((gap < np.log(ARGS['select_threshold']) - 1e-2).float().mean())


def time_path(fn, steps, warmup):
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
    ap.add_argument('--batches', default='1,32')
    ap.add_argument('--variants', default='reducedfc,full')
    ap.add_argument('--regimes', default='dense,biased')
    ap.add_argument('--paths', default='unfused,tfe,np')
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--steps', type=int, default=0, help='timed steps per path (0: 100 at batch 1, 20 at batch 32)')
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args(argv)
    rows = []
    cls = nets_factory.get_network('ron_320_vgg')
    for variant in a.variants.split(','):
        for regime in a.regimes.split(','):
            weights = W.synthetic_weights(variant, bg=BG[regime])
            for batch in [int(b) for b in a.batches.split(',')]:
                net = cls(variant=variant, dtype=a.dtype, max_batch=batch, fuse_pools=True).load_weights(weights)
                anchors = net.anchors(net.params.img_shape)
                x = torch.from_numpy(W.synthetic_images(batch, seed=0)).cuda()
                heads = net.forward_heads(x)
                adev = ops.anchors_to_device(anchors, net.device)
                fns = {'unfused': lambda: unfused(net, anchors, x),
                       'post_raw': lambda: tfe.post_tfe(*heads, adev, objectness_thres=OBJ_THR, min_size=0.03, cls_is_prob=False,
                                                        obj_is_prob=False, loc_decoded=False, **ARGS),
                       'tfe': lambda: net.detect_tfe(x, objectness_thres=OBJ_THR, **ARGS),
                       'np': lambda: net.detect(x, objectness_thres=OBJ_THR, select_threshold=ARGS['select_threshold'])}
                steps = a.steps or (100 if batch == 1 else 20)
                row = dict(variant=variant, regime=regime, batch=batch, dtype=a.dtype, steps=steps)
                row['pass_share'], row['early_exit_share'] = density(net, x)
                for path in a.paths.split(','):
                    ms = time_path(fns[path], steps, a.warmup)
                    row[path + '_ms'] = round(ms, 4)
                    row[path + '_images_per_s'] = round(batch * 1000.0 / ms, 1)
                rows.append(row)
                print(json.dumps(row), flush=True)
                net.close()
    paths = a.paths.split(',')
    print('\n| variant | regime | batch | pass | early exit | ' + ' | '.join('%s ms (img/s)' % p for p in paths) + ' |')
    print('|' + '---|' * (5 + len(paths)))
    for r in rows:
        print('| %s | %s | %d | %.4f | %.3f | ' % (r['variant'], r['regime'], r['batch'], r['pass_share'], r['early_exit_share']) +
              ' | '.join('%.3f (%.0f)' % (r[p + '_ms'], r[p + '_images_per_s']) for p in paths) + ' |')


if __name__ == '__main__':
    main()
