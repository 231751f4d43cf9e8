"""Seeded head tensors of SSD-300 (6 scales, 4 / 6 anchors per cell = 8732 anchors, no objectness) and the cases golden G9 holds:
shared by tests/golden/make_golden_ssd300.py (which ran the reference's np_methods on them) and the CPU / GPU tests."""
import numpy as np

FEAT_SHAPES = [(38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1)]
ANCHORS = [4, 6, 6, 6, 4, 4]
N_ANCHORS = sum(h * w * a for (h, w), a in zip(FEAT_SHAPES, ANCHORS))       # 8732

# name, seed, bg, cls_scale, select_thr, nms_thr.  All tie-free among the sorted scores (the reference's argsort is unstable);
# thr50_s93 uses the thresholds of notebooks/ssd_notebook.ipynb (select 0.5, nms 0.45, top_k 400).
G9_CASES = [
    ('ssd300_real_s90', 90, 8.0, 1.0, 0.01, 0.45),
    ('ssd300_mid_s91', 91, 6.0, 1.0, 0.01, 0.45),
    ('ssd300_dense_s92', 92, 4.0, 1.0, 0.01, 0.45),
    ('ssd300_thr50_s93', 93, 5.0, 3.0, 0.5, 0.45),
    ('ssd300_empty_s94', 94, 30.0, 1.0, 0.01, 0.45),
]


def head_tensors(seed, bg, cls_scale, num_classes=21):
    """Per layer, in order, from one RandomState(seed): cls = randn(1,h,w,a,21) * scale as float32, cls[..., 0] += bg, then
    loc = randn(1,h,w,a,4).  Returns (cls_logits, loc) lists."""
    rs = np.random.RandomState(seed)
    cls_l, loc_l = [], []
    for (h, w), a in zip(FEAT_SHAPES, ANCHORS):
        cls = (rs.randn(1, h, w, a, num_classes) * cls_scale).astype(np.float32)
        cls[..., 0] += np.float32(bg)
        cls_l.append(cls)
        loc_l.append(rs.randn(1, h, w, a, 4).astype(np.float32))
    return cls_l, loc_l
