"""Workspace sizes of the three post-processing forms (ron_post_np / ron_post_tfe / ron_post_eval) through the C ABI, no GPU: the
sizes are part of the ABI (callers allocate by them) and the offsets behind them are shared between ron_detect and
ron_detect_tfe.  Expected values are literals recorded from the library before the layouts were gathered into one struct per form;
a Python restatement of each layout formula has to agree with them."""
import ctypes as C

import pytest

RON_320 = [(5, 5, 10), (10, 10, 10), (20, 20, 10), (40, 40, 10)]                                   # 21 250 anchors
SSD_512 = [(64, 64, 4), (32, 32, 6), (16, 16, 6), (8, 8, 6), (4, 4, 6), (2, 2, 4), (1, 1, 4)]       # 24 564 anchors

COUNT_STRIDE = 32          # ints: one 128-byte line per counter
PART_CHUNKS, MAX_TOPK = 8, 512


def _align(v, a=256):
    return (v + a - 1) // a * a


def np_bytes(anchors, num_classes, n):
    """[candidate counts][survivor counts of the partial pass][keys: n x anchors x (C-1)][survivors: n x 8 x 512]"""
    return 2 * _align(n * COUNT_STRIDE * 4) + n * anchors * (num_classes - 1) * 8 + n * PART_CHUNKS * MAX_TOPK * 8


def tfe_bytes(anchors, num_classes, n):
    """[one int per (image, class) list][keys: lists x anchors]"""
    lists = n * (num_classes - 1)
    return _align(lists * 4) + lists * anchors * 8


def eval_bytes(anchors, num_classes, n, nms_mode):
    """[one 128-byte line per list][keys: lists x anchors][nms_mode | 4: best, n x anchors]"""
    lists = n * num_classes if nms_mode & 4 else n
    return _align(lists * COUNT_STRIDE * 4) + lists * anchors * 8 + (n * anchors * 8 if nms_mode & 4 else 0)


# (name, shape, num_classes, n) -> (np, tfe, eval, eval mode 0, eval mode 4)
CASES = [
    ('ron320_n1', RON_320, 21, 1, (3433280, 3400256, 170256, 170256, 3742816)),
    ('ron320_n32', RON_320, 21, 32, (109856768, 108802560, 5444096, 5444096, 119766016)),
    ('ssd512_n1', SSD_512, 21, 1, (3963520, 3930496, 196768, 196768, 4326080)),
    ('ssd512_n16', SSD_512, 21, 16, (63412224, 62885120, 3146240, 3146240, 69215232)),
    ('ron320_128_classes_n2', RON_320, 128, 2, (43246048, 43181024, 340256, 340256, 43892768)),
]


@pytest.fixture(scope='module')
def lib():
    from ron_tensorflow_amd import _lib
    return _lib.lib()


def _heads(shape, num_classes):
    from ron_tensorflow_amd import _lib
    h = _lib.Heads()
    h.num_layers, h.num_classes = len(shape), num_classes
    for i, (fh, fw, a) in enumerate(shape):
        h.feat_h[i], h.feat_w[i], h.num_anchors[i] = fh, fw, a
        h.cls[i] = h.obj[i] = h.loc[i] = 0x1000        # placeholders: the size functions never dereference them
    return h


def _sizes(lib, h, n):
    p = C.byref(h)
    return (lib.ron_post_np_workspace_bytes(p, n), lib.ron_post_tfe_workspace_bytes(p, n), lib.ron_post_eval_workspace_bytes(p, n),
            lib.ron_post_eval_workspace_bytes_mode(p, n, 0), lib.ron_post_eval_workspace_bytes_mode(p, n, 4))


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_workspace_bytes(lib, case):
    _, shape, num_classes, n, expected = case
    anchors = sum(fh * fw * a for fh, fw, a in shape)
    got = _sizes(lib, _heads(shape, num_classes), n)
    print(case[0], got)
    assert got == expected
    assert expected == (np_bytes(anchors, num_classes, n), tfe_bytes(anchors, num_classes, n), eval_bytes(anchors, num_classes, n, 0),
                        eval_bytes(anchors, num_classes, n, 0), eval_bytes(anchors, num_classes, n, 4))


def test_bad_arguments_give_minus_one(lib):
    assert _sizes(lib, _heads(RON_320, 21), 0) == (-1,) * 5
    assert _sizes(lib, _heads(RON_320, 1), 1) == (-1,) * 5
