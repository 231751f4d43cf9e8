#!/usr/bin/env python3
"""Generate golden G9 (SSD-300) under tests/golden/ from the REFERENCE's own code, like make_golden.py does for G1-G8.

  * g9_anchors_ssd300.npz      ``nets/ssd_vgg_300.py`` SSDNet().anchors((300, 300)) under the stubbed ``tensorflow``
  * g9_vgg_backbone_300.npz    the torch ``VGG16`` of ``convert_pytorch_vgg.py`` (pool3 = the ceil_mode pool: 75 -> 38) on G8's weight
                               seed and a seeded 300^2 image: all 20 taps, stored the way G8 stores them
  * g9_pipeline_ssd300.npz     ``nets/np_methods.py`` select -> clip -> sort(400) -> nms -> resize on the 8732 anchors, the fields of G5

Runs only where the reference is present; the reference's code is executed in memory, the .npz files hold arrays only.
Usage:  python tests/golden/make_golden_ssd300.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import ssd300_cases  # noqa: E402
from oracle import np_post, synth  # noqa: E402


def g9_anchors():
    mg.load_ref_ron()                      # installs the tensorflow stub and puts the reference on sys.path
    from nets import ssd_vgg_300
    layers = ssd_vgg_300.SSDNet().anchors((300, 300))
    assert len(layers) == 6 and sum(y.shape[0] * y.shape[1] * len(h) for y, x, h, w in layers) == ssd300_cases.N_ANCHORS
    out = {}
    for i, (y, x, h, w) in enumerate(layers):
        out['y%d' % i], out['x%d' % i], out['h%d' % i], out['w%d' % i] = y, x, h, w
    np.savez_compressed(os.path.join(HERE, 'g9_anchors_ssd300.npz'), **out)
    return layers


def g9_vgg_backbone():
    import torch
    ref = mg.load_ref_torch_vgg()
    seed_w, seed_x, size = 80, 85, 300
    model = ref.VGG16(ref.vgg(list(synth.VGG_CFG), 3))
    convs = [m for m in model.vgg if isinstance(m, torch.nn.Conv2d)]
    with torch.no_grad():
        for m, (w, b) in zip(convs, synth.vgg_backbone_weights_oihw(seed_w)):
            m.weight.copy_(torch.from_numpy(w))
            m.bias.copy_(torch.from_numpy(b))
    model.eval()
    taps = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: taps.append(out.detach().clone()))
             for m in model.vgg if not isinstance(m, torch.nn.Conv2d)]
    img = synth.vgg_backbone_image(seed_x, size)
    with torch.no_grad():
        model(torch.from_numpy(img).permute(0, 3, 1, 2).contiguous())
    for h in hooks:
        h.remove()
    assert len(taps) == len(synth.VGG_TAPS) == 20
    out = {'seed_weights': np.int64(seed_w), 'seed_image_%d' % size: np.int64(seed_x)}
    for name, t in zip(synth.VGG_TAPS, taps):
        a = t.permute(0, 2, 3, 1).contiguous().numpy()
        iy, ix = synth.g8_sample_index(a.shape[1]), synth.g8_sample_index(a.shape[2])
        out['%d/%s/shape' % (size, name)] = np.array(a.shape, dtype=np.int64)
        out['%d/%s/sample' % (size, name)] = a[:, iy][:, :, ix].copy()
        out['%d/%s/sum' % (size, name)] = np.array([a.sum(dtype=np.float64), (a.astype(np.float64) ** 2).sum()])
        print('%-8s %s' % (name, a.shape))
    np.savez_compressed(os.path.join(HERE, 'g9_vgg_backbone_300.npz'), **out)


def g9_pipeline(npm, anchors):
    out, names = {}, []
    rbbox_img = np.array([0., 0., 1., 1.], dtype=np.float32)
    for name, seed, bg, scale, thr, nms in ssd300_cases.G9_CASES:
        cls, loc = ssd300_cases.head_tensors(seed, bg, scale)
        pred = [np_post.softmax_last(x) for x in cls]
        c, s, b = npm.ssd_bboxes_select(pred, loc, anchors, select_threshold=thr, img_shape=(300, 300), num_classes=21, decode=True)
        n_cand = c.shape[0]
        b = npm.bboxes_clip(rbbox_img, b)
        c, s, b = npm.bboxes_sort(c, s, b, top_k=400)
        srt = (c.copy(), s.copy(), b.copy())
        assert len(np.unique(s)) == len(s), name          # the reference's argsort is unstable: tie-free cases only
        c, s, b = npm.bboxes_nms(c, s, b, nms_threshold=nms)
        b = npm.bboxes_resize(rbbox_img, b)
        names.append(name)
        out[name + '/params'] = np.array([seed, bg, scale, thr, nms], dtype=np.float64)
        out[name + '/n_cand'] = np.int64(n_cand)
        out[name + '/n_sorted'] = np.int64(srt[0].shape[0])
        out[name + '/classes'] = c.astype(np.int64)
        out[name + '/scores'] = s.astype(np.float32)
        out[name + '/bboxes'] = b.astype(np.float32).reshape(-1, 4)
        out[name + '/sorted_classes'] = srt[0].astype(np.int64)
        out[name + '/sorted_scores'] = srt[1].astype(np.float32)
        print('%-18s cand=%6d sorted=%3d kept=%3d' % (name, n_cand, srt[0].shape[0], c.shape[0]))
    out['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'g9_pipeline_ssd300.npz'), **out)


def main():
    npm = mg.load_np_methods()
    anchors = g9_anchors()
    g9_pipeline(npm, anchors)
    g9_vgg_backbone()
    for fn in sorted(os.listdir(HERE)):
        if fn.startswith('g9_'):
            print(fn, os.path.getsize(os.path.join(HERE, fn)), 'bytes')


if __name__ == '__main__':
    main()
