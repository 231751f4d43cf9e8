#!/usr/bin/env python3
"""Records tests/golden/g10_stem2_pool1_crc.npz: CRC-32 of pool1 as the fused stem (conv1_1 + conv1_2 + pool1 in one kernel) computes it,
from whichever build of the library RON_HIP_LIB names - run against the library of the commit BEFORE the fused stem moved its conv1_2
weights into registers and went to two workgroups per CU, so that tests/test_gpu_stem2_overlap.py can hold the current kernel to the
same bits.  Needs a GPU.

  pool1 of a RON-320 reducedfc context (fuse_pools=True) on synthetic_images(n, seed=12), n = 1, 2, 3 (400 / 800 / 1200 tiles of
  8 x 32 pixels: one round, 512 + 288, 2 x 512 + 176 on the kernel's 512 persistent workgroups), bf16 and fp16

Usage:  RON_HIP_LIB=/path/to/older/libron_hip.so python tests/golden/make_stem2_crc.py [out.npz]"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED = 12
BATCHES = (1, 2, 3)
DTYPES = ('bf16', 'fp16')


def make_net(dtype, max_batch=max(BATCHES)):
    from ron_tensorflow_amd import weights as W
    from ron_tensorflow_amd.nets import nets_factory
    cls = nets_factory.get_network('ron_320_vgg')
    return cls(cls.default_params._replace(num_classes=21), variant='reducedfc', dtype=dtype, max_batch=max_batch,
               fuse_pools=True).load_weights(W.synthetic_weights('reducedfc', seed=1))


def pool1(net, n):
    """pool1 of `net` on the seeded n-image batch, as dense fp32 [n, 160, 160, 64] on the host."""
    from ron_tensorflow_amd import weights as W
    net.forward_heads(torch.from_numpy(W.synthetic_images(n, seed=SEED)).cuda())
    return net.end_point('pool1', n).cpu().numpy()


def crc(a):
    return np.int64(zlib.crc32(np.ascontiguousarray(a, dtype=np.float32).tobytes()))


def main():
    out = {'seed': np.int64(SEED)}
    for dtype in DTYPES:
        net = make_net(dtype)
        assert 'conv1_1+conv1_2+pool1' in net.launch_plan(), 'the fused stem is not in this context\'s plan'
        for n in BATCHES:
            a = pool1(net, n)
            assert a.shape == (n, 160, 160, 64) and np.isfinite(a).all() and a.any()
            out['%s_n%d' % (dtype, n)] = crc(a)
        net.close()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'g10_stem2_pool1_crc.npz')
    np.savez(path, **out)
    print({k: int(v) for k, v in out.items()}, 'library:', os.environ.get('RON_HIP_LIB', '(the tree\'s own)'))


if __name__ == '__main__':
    main()
