"""CPU: the ron_detect_tfe entry point (fused forward + TF-evaluation post-processing) and its Python plumbing, no GPU."""
import ctypes as C
import os

import pytest


def _handle():
    from ron_tensorflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _cfg(**kw):
    from ron_tensorflow_amd import tfe
    args = dict(objectness_thres=0.03, select_threshold=0.01, nms_threshold=0.45, clipping_bbox=[0., 0., 1., 1.], top_k=400,
                keep_top_k=200, nms_mode='min', min_size=0.03, prior_scaling=(0.1, 0.1, 0.2, 0.2))
    args.update(kw)
    return tfe.tfe_cfg(**args)


def test_symbol_is_bound():
    from ron_tensorflow_amd import _lib
    handle = _handle()
    assert 'ron_detect_tfe' in _lib.SIGNATURES
    fn = handle.ron_detect_tfe
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    assert handle.ron_abi_version() == 2


def test_null_arguments_are_rejected_before_any_hip_call():
    """RON_ERR_INVALID with a message; a HIP call on this GPU-less machine would have come back as RON_ERR_HIP instead."""
    handle = _handle()
    cfg = _cfg()
    buf = (C.c_float * 16)()
    rc = handle.ron_detect_tfe(None, None, 1, C.byref(cfg), buf, buf, None)
    assert rc == -1
    assert b'NULL argument' in handle.ron_last_error()
    rc = handle.ron_detect_tfe(C.c_void_p(16), None, 1, None, buf, buf, None)
    assert rc == -1
    assert b'NULL argument' in handle.ron_last_error()


def test_cfg_builder():
    from ron_tensorflow_amd import tfe
    cfg = _cfg(select_threshold=None, clipping_bbox=None, min_size=None, nms_mode='union', top_k=512, keep_top_k=512)
    assert cfg.select_threshold == 0.0 and cfg.clip == 0 and cfg.min_size == -1.0
    assert cfg.nms_mode == tfe.NMS_MODES['union'] and cfg.top_k == 512 and cfg.keep_top_k == 512 and cfg.input_flags == 0
    assert abs(cfg.prior_scaling[2] - 0.2) < 1e-7
    with pytest.raises(ValueError):
        _cfg(nms_mode='iou')


def test_tfe_buffers_views():
    torch = pytest.importorskip('torch')
    from ron_tensorflow_amd import tfe
    buf = tfe.TfeBuffers(4, 21, 100, torch.device('cpu'))
    assert tuple(buf.scores.shape) == (4, 20, 100) and tuple(buf.bboxes.shape) == (4, 20, 100, 4)
    assert buf.narrow(4) is buf
    v = buf.narrow(2)
    assert v.n == 2 and v.scores.data_ptr() == buf.scores.data_ptr() and v.scores.is_contiguous()
    v.scores[1, 4, 7] = 0.5
    v.bboxes[1, 4, 7] = torch.tensor([0.1, 0.2, 0.3, 0.4])
    ds, db = v.as_dicts()
    assert sorted(ds) == list(range(1, 21))
    assert tuple(ds[5].shape) == (2, 100) and tuple(db[5].shape) == (2, 100, 4)
    assert float(ds[5][1, 7]) == 0.5 and float(buf.scores[1, 4, 7]) == 0.5
    assert float(db[5][1, 7, 3]) == pytest.approx(0.4)


def test_pipeline_rejects_unknown_post():
    from ron_tensorflow_amd import pipeline
    with pytest.raises(ValueError):
        pipeline.DetectPipeline(None, post='tf')
