"""Preprocessing on the GPU, reference names:
``preprocess_for_eval`` (preprocessing/ssd_vgg_preprocessing.py:358-425) for the eval driver's resize mode
(``Resize.WARP_RESIZE``, eval_ron_network.py:150-158) and the other three; ``ron_preprocess_for_train`` (:297-356), the
training chain expand -> patch -> flip -> resize with its random draws as an input; ``preprocess_image`` (:428-462)
dispatching between them.  JPEG decode stays on the host: the input here is the decoded uint8 RGB image."""
import ctypes as C

import numpy as np
import torch

from .._lib import RON_MAX_GT, RON_TRAIN_DRAWS, RON_TRAIN_GEOM, check, current_stream, lib, ptr

_R_MEAN, _G_MEAN, _B_MEAN = 123., 117., 104.          # ssd_vgg_preprocessing.py:30-32
EVAL_SIZE = (320, 320)


class Resize(object):                                 # ssd_vgg_preprocessing.py:22-27 (IntEnum there)
    NONE, CENTRAL_CROP, PAD_AND_RESIZE, WARP_RESIZE = 0, 1, 2, 3


def eval_geometry(h, w, out_shape, resize):
    """Geometry of one image for a resize mode: ({crop_y, crop_x, crop_h, crop_w, pad_y, pad_x, resized_h, resized_w},
    bbox transform).  The bbox transform maps relative (ymin, xmin, ymax, xmax) of the source image to the output the
    way tf_image.bboxes_crop_or_pad does (tf_image.py:141-166): returns (scale[4], offset[4]) with b' = b * scale + offset."""
    oh, ow = int(out_shape[0]), int(out_shape[1])
    one, zero = np.ones(4, np.float64), np.zeros(4, np.float64)
    if resize == Resize.WARP_RESIZE:
        return (0, 0, h, w, 0, 0, oh, ow), (one, zero)
    if resize == Resize.NONE:
        return (0, 0, h, w, 0, 0, h, w), (one, zero)
    if resize == Resize.PAD_AND_RESIZE:                                   # ssd_vgg_preprocessing.py:392-405
        factor = min(1.0, min(oh / h, ow / w))
        rh, rw = int(np.floor(factor * h)), int(np.floor(factor * w))
    elif resize == Resize.CENTRAL_CROP:
        rh, rw = h, w
    else:
        raise ValueError('unknown resize mode %r' % (resize,))
    # tf_image.resize_image_bboxes_with_crop_or_pad on the rh x rw image (tf_image.py:169-254)
    wd, hd = ow - rw, oh - rh
    crop_x, pad_x = max(-wd // 2, 0), max(wd // 2, 0)
    crop_y, pad_y = max(-hd // 2, 0), max(hd // 2, 0)
    hc, wc = min(oh, rh), min(ow, rw)
    # the crop is taken in resized coordinates; the kernel resizes the crop window of the SOURCE: scale 1 for CENTRAL_CROP, and
    # PAD_AND_RESIZE never crops (rh <= oh, rw <= ow)
    if resize == Resize.PAD_AND_RESIZE:
        geom = (0, 0, h, w, pad_y, pad_x, rh, rw)
    else:
        geom = (crop_y, crop_x, hc, wc, pad_y, pad_x, hc, wc)
    s1 = np.array([rh, rw, rh, rw], np.float64)
    o1 = np.array([-crop_y, -crop_x, -crop_y, -crop_x], np.float64)
    s2 = np.array([hc, wc, hc, wc], np.float64)
    o2 = np.array([pad_y, pad_x, pad_y, pad_x], np.float64)
    t = np.array([oh, ow, oh, ow], np.float64)
    # b -> ((b * s1 + o1) / s2 * s2 + o2) / t
    return geom, (s1 / t, (o1 + o2) / t)


def _uint8_images(images):
    arrs = []
    for im in images:
        a = im.detach().cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError('Input must be of size [height, width, C>0]')        # :374 (C = 3 on this path)
        if a.dtype != np.uint8:
            raise ValueError('decoded images are uint8')
        arrs.append(np.ascontiguousarray(a))
    return arrs


def _pack(arrs, dev):
    """One upload of the images' bytes back to back: (packed uint8, offsets int64 [N], hw int32 [N, 2]) on the device."""
    hw = np.array([[a.shape[0], a.shape[1]] for a in arrs], np.int32)
    sizes = np.array([a.size for a in arrs], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    packed = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(dev)
    return packed, torch.from_numpy(offsets).to(dev), torch.from_numpy(hw).to(dev)


def preprocess_for_eval_batch(images, out_shape=EVAL_SIZE, resize=Resize.WARP_RESIZE, device='cuda:0',
                              means=(_R_MEAN, _G_MEAN, _B_MEAN)):
    """List of HWC uint8 images (numpy or torch, any sizes) -> float32 GPU tensor [N, out_h, out_w, 3]: one packed
    upload, one launch.  All four modes of the reference (Resize.NONE needs equally sized images).  The upload comes from pageable host
    memory and holds the host until what is queued on the current stream has finished; the launch itself (ron_preprocess_eval_geom)
    does not synchronise."""
    if resize not in (Resize.WARP_RESIZE, Resize.NONE, Resize.CENTRAL_CROP, Resize.PAD_AND_RESIZE):
        raise ValueError('unknown resize mode %r' % (resize,))
    dev = torch.device(device)
    arrs = _uint8_images(images)
    hw = np.array([[a.shape[0], a.shape[1]] for a in arrs], np.int32)
    if resize == Resize.NONE:
        if len(set(map(tuple, hw.tolist()))) != 1:
            raise ValueError('Resize.NONE needs equally sized images in a batch')
        out_shape = (int(hw[0, 0]), int(hw[0, 1]))
    packed, d_off, d_hw = _pack(arrs, dev)
    out = torch.empty((len(arrs), int(out_shape[0]), int(out_shape[1]), 3), dtype=torch.float32, device=dev)
    m = (C.c_float * 3)(*means)
    d_geom = None
    if resize in (Resize.CENTRAL_CROP, Resize.PAD_AND_RESIZE):
        geom = np.array([eval_geometry(a.shape[0], a.shape[1], out_shape, resize)[0] for a in arrs], np.int32)
        d_geom = torch.from_numpy(geom).to(dev)
    with torch.cuda.device(dev):
        check(lib().ron_preprocess_eval_geom(ptr(packed), ptr(d_off), ptr(d_hw), ptr(d_geom), len(arrs), int(out_shape[0]),
                                             int(out_shape[1]), m, ptr(out), current_stream()))
    return out


def preprocess_for_eval(image, labels, bboxes, out_shape=EVAL_SIZE, data_format='NHWC', difficults=None,
                        resize=Resize.WARP_RESIZE, device='cuda:0'):
    """Reference signature for one image: returns (image [out_h, out_w, 3] float32 GPU, labels, bboxes, bbox_img).
    Difficult ground truth is removed when ``difficults`` is given (:415-419); bboxes are unchanged by a warp and follow
    the crop / pad otherwise, as does ``bbox_img`` (the image rectangle, :379-384, :413-414)."""
    img = preprocess_for_eval_batch([image], out_shape, resize, device)[0]
    if data_format == 'NCHW':
        img = img.permute(2, 0, 1).contiguous()
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    _, (scale, offset) = eval_geometry(a.shape[0], a.shape[1], a.shape[:2] if resize == Resize.NONE else out_shape, resize)
    bbox_img = (np.array([0., 0., 1., 1.]) * scale + offset).astype(np.float32)
    if bboxes is not None:
        bboxes = (np.asarray(bboxes, np.float64).reshape(-1, 4) * scale + offset).astype(np.float32)
    if difficults is not None and labels is not None:
        mask = ~np.asarray(difficults).astype(bool)
        labels = np.asarray(labels)[mask]
        bboxes = np.asarray(bboxes)[mask]
    return img, labels, bboxes, bbox_img


def _padded_ground_truth(glabels, gbboxes, n, dev):
    """Ground truth as the kernels take it: int32 [N, G] (0 = padding, present rows a prefix) and float32 [N, G, 4] on `dev`.
    Accepts the padded pair (numpy or torch) or one list per image of ragged rows."""
    if isinstance(glabels, (list, tuple)):
        rows = [np.asarray(l.detach().cpu() if isinstance(l, torch.Tensor) else l).reshape(-1) for l in glabels]
        boxes = [np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float32).reshape(-1, 4) for b in gbboxes]
        g = max(1, max(r.size for r in rows))
        gl, gb = np.zeros((len(rows), g), np.int32), np.zeros((len(rows), g, 4), np.float32)
        for i, (r, b) in enumerate(zip(rows, boxes)):
            if b.shape[0] != r.size:
                raise ValueError('image %d: %d labels, %d boxes' % (i, r.size, b.shape[0]))
            gl[i, :r.size], gb[i, :r.size] = r, b
        glabels, gbboxes = gl, gb
    gl = (glabels if isinstance(glabels, torch.Tensor) else torch.from_numpy(np.asarray(glabels))).to(dev).to(torch.int32).contiguous()
    gb = (gbboxes if isinstance(gbboxes, torch.Tensor) else torch.from_numpy(np.asarray(gbboxes, np.float32))).to(dev)
    gb = gb.to(torch.float32).contiguous()
    if gl.dim() != 2 or gl.shape[0] != n or tuple(gb.shape) != tuple(gl.shape) + (4,):
        raise ValueError('ground truth must be glabels [N, G] and gbboxes [N, G, 4] for the %d images' % n)
    if not 1 <= gl.shape[1] <= RON_MAX_GT:
        raise ValueError('%d ground-truth rows per image not in [1, %d]' % (gl.shape[1], RON_MAX_GT))
    return gl, gb


def ron_preprocess_for_train_batch(images, glabels, gbboxes, out_shape=EVAL_SIZE, draws=None, generator=None, device='cuda:0',
                                   means=(_R_MEAN, _G_MEAN, _B_MEAN)):
    """ron_preprocess_for_train (:297-356) for a batch: list of HWC uint8 images (any sizes) and their padded ground truth
    (glabels [N, G], 0 = padding; gbboxes [N, G, 4]) -> GPU tensors
        images [N, out_h, out_w, 3] float32, glabels int32 [N, G], gbboxes float32 [N, G, 4], counts int32 [N], geom int32 [N, 12]
    with the kept rows at the front (what RONNet.bboxes_encode / validation_losses take).  One packed upload, three launches
    (geometry, channel sums of the expanded images, pixels), no read-back; the uploads of host arrays (images, and ground truth / draws
    when given as numpy) come from pageable memory and hold the host until what is queued on the current stream has finished, the
    launches themselves do not synchronise.  The random decisions are `draws`
    ([N, RON_TRAIN_DRAWS] uniform floats in [0, 1), slot layout in include/ron_hip.h); drawn with torch.rand from `generator`
    (a generator of the target device) when not given."""
    dev = torch.device(device)
    arrs = _uint8_images(images)
    n = len(arrs)
    gl, gb = _padded_ground_truth(glabels, gbboxes, n, dev)
    g = int(gl.shape[1])
    oh, ow = int(out_shape[0]), int(out_shape[1])
    with torch.cuda.device(dev):
        if draws is None:
            draws = torch.rand((n, RON_TRAIN_DRAWS), dtype=torch.float32, device=dev, generator=generator)
        else:
            draws = (draws if isinstance(draws, torch.Tensor) else torch.from_numpy(np.asarray(draws, np.float32))).to(dev)
            draws = draws.to(torch.float32).contiguous()
            if tuple(draws.shape) != (n, RON_TRAIN_DRAWS):
                raise ValueError('draws must be [%d, %d]' % (n, RON_TRAIN_DRAWS))
        packed, d_off, d_hw = _pack(arrs, dev)
        geom = torch.empty((n, RON_TRAIN_GEOM), dtype=torch.int32, device=dev)
        gl_out, gb_out = torch.empty_like(gl), torch.empty_like(gb)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        out = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev)
        check(lib().ron_train_geometry(ptr(d_hw), ptr(gl), ptr(gb), n, g, ptr(draws), ptr(geom), ptr(gl_out), ptr(gb_out),
                                       ptr(counts), current_stream()))
        nbytes = lib().ron_preprocess_train_workspace_bytes(n)
        if nbytes < 0:
            check(-1)
        ws = torch.empty((int(nbytes),), dtype=torch.uint8, device=dev)
        m = (C.c_float * 3)(*means)
        check(lib().ron_preprocess_train(ptr(packed), ptr(d_off), ptr(d_hw), ptr(geom), n, oh, ow, m, ptr(ws), ptr(out),
                                         current_stream()))
    return out, gl_out, gb_out, counts, geom


def ron_preprocess_for_train(image, labels, bboxes, out_shape, data_format='NHWC', scope='ron_preprocessing_train',
                             draws=None, generator=None, device='cuda:0'):
    """Reference signature for one image (:297-356): returns (image [out_h, out_w, 3] float32 GPU, labels, bboxes) with the
    ground truth trimmed to the kept rows (GPU tensors, labels int32)."""
    labels = np.asarray(labels.detach().cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
    boxes = np.asarray(bboxes.detach().cpu() if isinstance(bboxes, torch.Tensor) else bboxes, np.float32).reshape(-1, 4)
    if draws is not None:
        draws = draws.reshape(1, -1) if isinstance(draws, torch.Tensor) else np.asarray(draws, np.float32).reshape(1, -1)
    img, gl, gb, counts, _ = ron_preprocess_for_train_batch([image], [labels], [boxes], out_shape, draws, generator, device)
    k = int(counts[0])                       # the one synchronisation: the reference returns ragged rows
    img = img[0]
    if data_format == 'NCHW':
        img = img.permute(2, 0, 1).contiguous()
    return img, gl[0, :k], gb[0, :k]


def preprocess_image(image, labels, bboxes, out_shape, data_format, is_training=False, **kwargs):
    """:428-462: ron_preprocess_for_train when training, preprocess_for_eval (with its keyword arguments) otherwise."""
    if is_training:
        return ron_preprocess_for_train(image, labels, bboxes, out_shape=out_shape, data_format=data_format, **kwargs)
    return preprocess_for_eval(image, labels, bboxes, out_shape=out_shape, data_format=data_format, **kwargs)
