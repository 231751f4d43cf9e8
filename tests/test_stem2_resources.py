"""CPU test: what the fused stem kernel (csrc/stem.hip, stem2_kernel: conv1_1 + conv1_2 + pool1) costs a CU, read from the metadata
hipcc emits for gfx950 (no GPU).

The kernel keeps its share of the conv1_2 weights - 144 registers - for the whole life of a persistent workgroup and is built for two
workgroups of four waves per CU, i.e. two waves per SIMD: 256 registers per lane (arch + accumulation, one file on this chip) and no
more than half of the CU's 160 KB of LDS.  A build that spills a single register to scratch is not a slower version of the same
thing (round 6 measured 282 -> 451 us for 336 bytes of it), and one register over 256 halves the machine.  Resource figures only."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ron_tensorflow_amd', 'csrc')
HIPCC = '/opt/rocm/bin/hipcc'
FIELDS = ('private_segment_fixed_size', 'vgpr_count', 'agpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'max_flat_workgroup_size',
          'group_segment_fixed_size')


@pytest.fixture(scope='module')
def stem2_kernels():
    """{mangled name: {field: value}} of both stem2_kernel instantiations, from the amdhsa.kernels metadata of the device assembly."""
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'stem.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I.', '--cuda-device-only', '-S', '-o', out, 'stem.hip'],
                       cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            asm = f.read()
    meta = asm[asm.index('amdhsa.kernels:'):]
    found = {}
    for entry in re.split(r'\n  - ', meta)[1:]:                       # one YAML list item per kernel
        name = re.search(r'\.name:\s+(\S+)', entry)
        if name and 'stem2_kernel' in name.group(1):
            found[name.group(1)] = {k: int(v) for k, v in re.findall(r'\.(\w+):\s+(\d+)\s*(?:\n|$)', entry) if k in FIELDS}
    return found


def test_both_instantiations_are_in_the_build(stem2_kernels):
    assert len(stem2_kernels) == 2 and any('StemBF16' in n for n in stem2_kernels) and any('StemF16' in n for n in stem2_kernels), sorted(stem2_kernels)


def test_no_scratch_and_two_waves_per_simd(stem2_kernels):
    for name, m in stem2_kernels.items():
        print(name, m)
        assert m['private_segment_fixed_size'] == 0, '%s uses %d bytes of scratch per lane' % (name, m['private_segment_fixed_size'])
        assert m.get('vgpr_spill_count', 0) == 0 and m.get('sgpr_spill_count', 0) == 0, (name, m)
        assert m['vgpr_count'] + m.get('agpr_count', 0) <= 256, '%s: %d arch + %d accumulation registers' % (name, m['vgpr_count'], m.get('agpr_count', 0))
        assert m['max_flat_workgroup_size'] == 256, (name, m)
