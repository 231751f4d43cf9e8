#!/usr/bin/env python3
"""Records tests/golden/g9_stem_320_crc.npz: CRC-32 of the conv1_1 stem kernels' output at width 320 (full 32-pixel tiles only), from
whichever build of the library RON_HIP_LIB names - run against the library of the commit BEFORE the stem kernels learnt the ragged last
tile, so that tests/test_gpu_odd_maps.py can hold the current kernels to the same bits.  Needs a GPU.

  bf16, fp16   ron_conv2d_nhwc on a seeded 2 x 8 x 320 x 3 image (the single-operator entry runs the stem kernel at this width)
  f16x3        the conv1_1 end point of a RON-320 reducedfc context (the split-precision stem kernel runs inside the graph only at this
               width; the single-operator entry takes im2col + GEMM)

Usage:  RON_HIP_LIB=/path/to/older/libron_hip.so python tests/golden/make_stem320_crc.py [out.npz]"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 13


def op_inputs(seed=SEED):
    rs = np.random.RandomState(seed)
    x = (rs.uniform(0, 255, (2, 8, 320, 3)) - np.array([123., 117., 104.])).astype(np.float32)
    wt = (rs.randn(3, 3, 3, 64) * np.sqrt(2.0 / 27)).astype(np.float32)
    b = (rs.randn(64) * 0.1).astype(np.float32)
    return x, wt, b


def context_conv1_1(dtype='f16x3'):
    """conv1_1 of a RON-320 reducedfc context on a seeded 320 x 320 image, as dense fp32 [1, 320, 320, 64]."""
    from ron_tensorflow_amd import weights as W
    from ron_tensorflow_amd.nets import nets_factory
    cls = nets_factory.get_network('ron_320_vgg')
    net = cls(cls.default_params._replace(num_classes=21), variant='reducedfc', dtype=dtype, max_batch=1).load_weights(
        W.synthetic_weights('reducedfc', seed=1))
    net.forward_heads(torch.from_numpy(W.synthetic_images(1, seed=SEED)).cuda())
    a = net.end_point('conv1_1', 1).cpu().numpy()
    net.close()
    return a


def crc(a):
    return np.int64(zlib.crc32(np.ascontiguousarray(a, dtype=np.float32).tobytes()))


def main():
    from ron_tensorflow_amd import ops
    out = {'seed': np.int64(SEED)}
    x, wt, b = op_inputs()
    for dtype in ('bf16', 'fp16'):
        out[dtype] = crc(ops.conv2d_nhwc(torch.from_numpy(x).cuda(), wt, b, relu=True, dtype=dtype).cpu().numpy())
    out['f16x3_conv1_1'] = crc(context_conv1_1())
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'g9_stem_320_crc.npz')
    np.savez(path, **out)
    print({k: int(v) for k, v in out.items()}, 'library:', os.environ.get('RON_HIP_LIB', '(the tree\'s own)'))


if __name__ == '__main__':
    main()
