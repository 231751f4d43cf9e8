"""CPU: the launch trace of the dry run (RON_PLAN_ONLY=1 RON_PLAN_TRACE=<file>, csrc/common.h) pins every host-side plan.

In a dry run the library makes every host decision and skips every HIP call; with RON_PLAN_TRACE set it writes one line per skipped
launch - kernel, grid, block, dynamic LDS bytes, size and CRC32C of every by-value argument - and one per asynchronous memset.
Device addresses come from a counter, so two runs give the same bytes, and two TREES that write the same trace launch the same
kernels with the same arguments.  tools/plan_sweep.cpp puts a `context variant dtype flags max_batch` line in front of each context
and a `pass <name>` line in front of each argument pass (conv_planner_arguments drives plan_conv / launch_conv_group through the
single-operator entry points with forced tile configurations and split factors, refusals and their messages included; the last two,
conv_forward_arguments and conv_chain_arguments, drive the training forward and the network-level chain).

What is hashed is well defined: every struct that reaches a kernel by value is declared without padding (RON_KERNEL_ARGS_BEGIN / _END,
csrc/common.h; the compiler refuses a padded one, and trace_launch refuses a struct that was not declared so), so a digest depends on
the argument values alone - not on the compiler, its flags, or the function a launch is written in.

EXPECTED holds the digest of every section of the `--quick` sweep, so a failure names the context or pass whose launches changed.
The literals were recorded when the argument structs lost their padding: against the trace of the tree before, 154 of 36090 lines
differ, each only in the CRC of a 48-byte ViewDev argument (elementwise.hip: pack_kernel, unpack_kernel, l2norm_kernel), whose 4
bytes of tail padding used to be hashed as they lay on the stack; every other line is byte for byte the one recorded before the conv
planner was gathered into one member plan (conv_mfma.hip plan_member).  After an INTENDED plan change, re-record them (the sweep
must have been built: tests/test_asan_plan_sweep.py, or `make -C ron_tensorflow_amd/csrc asan ASAN_ARGS=--quick`):

    python tests/test_plan_trace_cpu.py          # prints the EXPECTED table to paste below

Uses the build_asan/plan_sweep that tests/test_asan_plan_sweep.py builds (brought up to date with make first, so that a binary left
from another tree is not what gets checked) and skips like its second test when it is missing."""
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, 'ron_tensorflow_amd', 'csrc', 'build_asan', 'plan_sweep')

EXPECTED = {
    'context 0 1 0x1 1': '88379352323adc22',
    'context 0 3 0x1 1': 'a18d1e8cc533d0c9',
    'context 0 1 0x1 13': '8f016db494312d7b',
    'context 0 1 0x1 32': '1ebaa7a72971d9e1',
    'context 0 3 0x1 32': '755360dca32c2790',
    'context 0 1 0x21 1': 'df68ccd364ebe280',
    'context 0 1 0x21 13': '5b830fb086525fde',
    'context 0 1 0x21 32': 'c6600e73d8e93182',
    'context 0 1 0x41 1': '0dfbc1e7f0fc470d',
    'context 0 1 0x41 13': '8555a68f62b4a6c2',
    'context 0 1 0x41 32': 'b1728df4f03a051c',
    'context 0 1 0x9 1': '28298597a141f78f',
    'context 0 1 0x9 13': 'e0d1e9eeb28f8763',
    'context 0 1 0x9 32': '4e219b1dfbbc1571',
    'context 0 1 0x11 1': '5af93f8dad65971b',
    'context 0 1 0x11 13': '52bbd249c8b60c18',
    'context 0 1 0x11 32': 'f2cd7a106dd2265c',
    'context 2 1 0x1 1': '65b9184be8bdf71f',
    'context 2 3 0x1 1': 'c88ef6f97c17c0ad',
    'context 2 1 0x1 13': '092b4e7d8867f460',
    'context 2 1 0x1 32': '7f5a1be38eccef82',
    'context 2 3 0x1 32': 'ae7674ffa1729c57',
    'context 2 1 0x9 1': '3f10d3786a5b9ee6',
    'context 2 1 0x9 13': 'bbdb7186d3eb97e5',
    'context 2 1 0x9 32': 'f353865656809873',
    'context 2 1 0x11 1': '01d54e5a7a634170',
    'context 2 1 0x11 13': 'f3f7179a191c1107',
    'context 2 1 0x11 32': '1e687dc78f7d8ec2',
    'context 1 1 0x1 32': 'c27552c23754eea7',
    'context 3 1 0x1 1': '8eab1af8df90498e',
    'context 3 1 0x1 32': '3d6de168ea5667da',
    'context 3 0 0x0 1': '3e0ed1a499bb3c0f',
    'pass loss_arguments': 'cce9b8771b7e8bfd',
    'pass conv_backward_arguments': 'a16ea092513d601d',
    'pass stem_backward_arguments': 'f680e656aebe47ef',
    'pass op_backward_arguments': '472486200c7e1f34',
    'pass batchnorm_arguments': '63e474dfa231c86b',
    'pass optimizer_arguments': '82b7de58c71f575d',
    'pass conv_envelope': '213341073940a95a',
    'pass conv_planner_arguments': '0af9347b816153b3',
    'pass conv_forward_arguments': '2c88547b28d13a56',
    'pass conv_chain_arguments': '2737d407926c80bb',
}


def run_sweep(path):
    # none of the library's own switches from the caller's shell (RON_IGEMM224, RON_SPLITK_NO_VETO, RON_PANEL_COLS, ... change plans)
    env = {k: v for k, v in os.environ.items() if not k.startswith('RON_')}
    env.update(RON_PLAN_ONLY='1', RON_PLAN_TRACE=path)
    p = subprocess.run([EXE, '--quick'], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=850)
    assert p.returncode == 0, p.stdout.decode(errors='replace')[-3000:]
    with open(path, 'rb') as f:
        return f.read()


def sections(trace):
    """{heading: digest of the heading and the lines up to the next heading}, in the order of the file"""
    out, name, h = {}, None, None
    for line in trace.splitlines(keepends=True):
        if line.startswith((b'context ', b'pass ')):
            if name is not None:
                out[name] = h.hexdigest()[:16]
            name, h = line.decode().strip(), hashlib.sha256()
            assert name not in out, 'two sections named %r' % name
        assert h is not None, 'the trace does not start with a heading: %r' % line[:80]
        h.update(line)
    if name is not None:
        out[name] = h.hexdigest()[:16]
    return out


@pytest.fixture(scope='module')
def traces():
    if os.path.exists(EXE) and os.path.exists('/opt/rocm/bin/hipcc'):
        # the sweep of THIS tree, not one left from another: make rebuilds what is older than its sources, and nothing otherwise
        subprocess.run(['make', '-C', os.path.dirname(os.path.dirname(EXE)), 'build_asan/plan_sweep'], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT, timeout=850)
    if not os.path.exists(EXE):
        pytest.skip('build_asan/plan_sweep not built (tests/test_asan_plan_sweep.py builds it)')
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(2) as pool:          # (the two runs side by side: half the wait)
        return list(pool.map(run_sweep, [os.path.join(d, 'trace%d.txt' % i) for i in range(2)]))


@pytest.mark.timeout(900)
def test_two_runs_write_the_same_trace(traces):
    assert len(traces[0]) > 1000000 and traces[0].count(b'\n') > 30000
    assert traces[0] == traces[1]


@pytest.mark.timeout(900)
def test_sections_are_the_recorded_ones(traces):
    got = sections(traces[0])
    assert list(got) == list(EXPECTED), 'the sweep\'s contexts / passes changed: %r' % sorted(set(got) ^ set(EXPECTED))


@pytest.mark.timeout(900)
@pytest.mark.parametrize('section', list(EXPECTED))
def test_section_digest(traces, section):
    assert sections(traces[0]).get(section) == EXPECTED[section]


if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as d:
        table = sections(run_sweep(os.path.join(d, 'trace.txt')))
    print('EXPECTED = {')
    for k, v in table.items():
        print('    %r: %r,' % (k, v))
    print('}')
    sys.exit(0)
