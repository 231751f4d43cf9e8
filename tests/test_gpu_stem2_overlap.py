"""GPU: the fused stem (conv1_1 + conv1_2 + pool1, csrc/stem.hip stem2_kernel) with its conv1_2 weights in registers and two workgroups
of four waves per CU computes the bits the form before it computed (72 KB of weights in LDS, one workgroup of eight waves per CU).

Only which wave computes which output changed, so pool1 must be byte-identical for any input.  The network fixes 320 x 320, so the
shapes that matter are the batch sizes that change how the 8 x 32 pixel tiles meet the 512 persistent workgroups:
  n = 1   400 tiles: every workgroup runs once, and its prefetch of a next tile runs past the end;
  n = 2   800 tiles: 512 + 288;
  n = 3   1200 tiles: 2 x 512 + 176, a ragged third round.
The checksums (tests/golden/g10_stem2_pool1_crc.npz) were recorded by tests/golden/make_stem2_crc.py from the library of the commit
before the change (RON_HIP_LIB), never from the kernel under test."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_stem2_crc as stem2  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    g = np.load(os.path.join(HERE, 'golden', 'g10_stem2_pool1_crc.npz'))
    assert int(g['seed']) == stem2.SEED
    return g


@pytest.fixture(scope='module', params=stem2.DTYPES)
def net(request):
    assert torch.cuda.is_available()
    net = stem2.make_net(request.param)
    assert 'conv1_1+conv1_2+pool1' in net.launch_plan()
    yield request.param, net
    net.close()


@pytest.mark.parametrize('n', stem2.BATCHES)
def test_pool1_is_what_the_eight_wave_form_computed(net, golden, n):
    dtype, net = net
    a = stem2.pool1(net, n)
    assert a.shape == (n, 160, 160, 64) and float(np.abs(a).max()) > 0
    assert int(stem2.crc(a)) == int(golden['%s_n%d' % (dtype, n)]), 'pool1 of the fused stem (%s, %d images) changed' % (dtype, n)


def test_three_forwards_give_the_same_bytes(net):
    """A race in the pool staging or a missing barrier shows as run-to-run differences: the ragged three-round case, three times."""
    _, net = net
    runs = [stem2.pool1(net, 3).tobytes() for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


@pytest.mark.parametrize('dtype', stem2.DTYPES)
def test_two_workgroups_share_a_cu(dtype):
    """What the kernel is built around, asked of the runtime's occupancy query for the launch's own block and LDS size (the launch
    asks the same question once per device and fails on any other answer)."""
    from ron_tensorflow_amd import _lib
    per_cu = C.c_int32(-1)
    _lib.check(_lib.lib().ron_stem2_workgroups_per_cu(_lib.DTYPES[dtype], C.byref(per_cu)))
    assert per_cu.value == 2
