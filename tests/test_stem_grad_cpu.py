"""The stem-backward reference, its mutants and the argument checks of ron_conv2d_stem_backward_nhwc, without a GPU.

  * the float64 formulas of tests/stem_grad_ref.py against torch-CPU float64 autograd of conv2d + relu on the rounded operands, and
    the dense-pixel formulation (the kernel's walk) against them;
  * the lattice inputs meet the conditions that make them exact, for every case;
  * every mutant of stem_grad_ref.MUTANTS is caught by at least one case under the GPU test's grading;
  * ron_conv2d_stem_backward_workspace_bytes and every refusal of the entry point, through the C ABI in the library's dry-run mode."""
import ctypes as C  # noqa: F401
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_grad_ref as cgr
import stem_grad_cases as sc
import stem_grad_ref as ref

torch = pytest.importorskip('torch')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('case', sorted(sc.CASES))
def test_reference_is_torch_float64_autograd(case):
    """out = relu(conv2d(xs, w) + b) in float64 with the rounded dy as the upstream gradient: autograd's dw and db are the reference's
    with y = out (the mask is out > 0; rounding commutes with the mask)."""
    x, _, dy = sc.inputs('gauss', case)
    rs = np.random.RandomState(7)
    wt = rs.randn(3, 3, 3, 64) * 0.01
    bias = rs.randn(64) * 0.5
    xs = cgr.ROUND['bf16'](x)
    tx = torch.from_numpy(xs.astype(np.float64)).permute(0, 3, 1, 2)
    tw = torch.from_numpy(wt).permute(3, 2, 0, 1).requires_grad_(True)
    tb = torch.from_numpy(bias).requires_grad_(True)
    out = torch.relu(torch.nn.functional.conv2d(tx, tw, tb, padding=1))
    out.backward(torch.from_numpy(cgr.ROUND['bf16'](dy).astype(np.float64)).permute(0, 3, 1, 2))
    y = out.detach().permute(0, 2, 3, 1).numpy().astype(np.float32)
    assert ((out > 0).numpy() == (y > 0).transpose(0, 3, 1, 2)).all()          # the float32 copy of y keeps the mask
    xs2, dz = ref.seen(x, y, dy, 'bf16', True)
    g = ref.grads64(xs2, dz)
    # the same float64 products summed in another order: 2^-40 of each output's own largest magnitude (K <= 3200 additions of 2^-53)
    for name, got in (('dw', tw.grad.permute(2, 3, 1, 0).numpy()), ('db', tb.grad.numpy())):
        assert np.abs(got - g[name][0]).max() <= 2.0 ** -40 * max(np.abs(g[name][0]).max(), 1e-300), name
    dense = ref.dw_dense(xs2, dz)
    assert np.abs(dense - g['dw'][0]).max() <= 2.0 ** -40 * np.abs(g['dw'][0]).max()
    if case == 'A':          # only the centre tap sees a 1 x 1 map
        off_centre = np.ones((3, 3), bool)
        off_centre[1, 1] = False
        assert not g['dw'][0][off_centre].any() and g['dw'][0][1, 1].any()


@pytest.mark.parametrize('dtype', sc.DTYPES)
@pytest.mark.parametrize('case', sorted(sc.CASES))
def test_lattice_conditions_and_reference_inside_its_bounds(case, dtype):
    for kind in sc.KINDS:
        x, y, dy = sc.inputs(kind, case)
        for relu in (0, 1):
            xs, dz = ref.seen(x, y, dy, dtype, relu)
            g = ref.grads64(xs, dz)
            if kind == 'lattice':
                assert np.array_equal(xs, x)
                sc.assert_lattice(x, dz, list(cgr.ROUND.values()))
                assert np.array_equal(g['dw'][0], np.round(g['dw'][0])) and np.abs(g['dw'][0]).max() < 2 ** 24
                assert np.array_equal(ref.dw_dense(xs, dz), g['dw'][0])
                if relu and dz.size >= 640:
                    assert 0.3 < (y == 0).mean() < 0.5
            cgr.check('%s %s relu=%d reference' % (case, kind, relu), ref.deliver(g), g, dtype, kind)


@pytest.mark.parametrize('name', ref.MUTANTS)
def test_every_mutant_is_killed(name):
    """Under the GPU test's grading (lattice: equality, gauss: ratio <= 1) at least one (case, kind) rejects the mutant; the structural
    mutants must fall to the lattice, the rounding ones to the gauss inputs."""
    rounding = name in ref.ROUNDING_MUTANTS
    killed = []
    for case in sorted(sc.CASES):
        for kind in sc.KINDS:
            x, y, dy = sc.inputs(kind, case)
            out = ref.mutant(name, x, y, dy, 'bf16', 1)
            if out is None:
                continue
            g = ref.grads64(*ref.seen(x, y, dy, 'bf16', 1))
            tops = cgr.grade(case, out, g, 'bf16', kind, verbose=False)
            if max(tops.values()) > 1.0:
                killed.append((case, kind))
        if killed and (rounding or any(kd == 'lattice' for _, kd in killed)):
            break
    assert killed, 'mutant %s survives every case' % name
    if rounding:
        assert all(kd == 'gauss' for _, kd in killed), killed         # integers cannot show a missing rounding
    else:
        assert any(kd == 'lattice' for _, kd in killed), 'mutant %s: no lattice case catches it (%s)' % (name, killed)


def test_unmutated_operator_passes_the_grading():
    for case in sorted(sc.CASES):
        for kind in sc.KINDS:
            x, y, dy = sc.inputs(kind, case)
            out = ref.mutant(None, x, y, dy, 'bf16', 1)
            g = ref.grads64(*ref.seen(x, y, dy, 'bf16', 1))
            cgr.check(case, out, g, 'bf16', kind)


# ------------------------------------------------------------------------------------------------------------- the C ABI, dry run
_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from ron_tensorflow_amd import _lib
L = _lib.lib()
cases = json.loads(sys.argv[1])
fake = lambda i: C.c_void_p((i + 1) << 24)          # device "addresses" nobody dereferences in the dry run
def desc(n, h, w, cin=3, cout=64, k=3, rate=1, stride=1, relu=1, transpose=0, dtype='bf16', pool=0, splitk=-1, tile_cfg=-1):
    return _lib.ConvDesc(n, h, w, cin, cout, k, k, stride, rate, relu, transpose, _lib.DTYPES[dtype], tile_cfg, 0, 0, pool, splitk, 0)
size = lambda d: L.ron_conv2d_stem_backward_workspace_bytes(C.byref(d))
def call(d, ws_bytes, y=True, dy=None, dw=True, db=True, x=True):
    return L.ron_conv2d_stem_backward_nhwc(C.byref(d), fake(1) if x else None, fake(3) if y else None, fake(4) if dy is None else dy,
                                           fake(6) if dw else None, fake(7) if db else None, fake(8), ws_bytes, None)
out = {'bytes': {}, 'bytes2n': {}, 'ok': {}, 'refused': {}}
for name, c in cases.items():
    out['bytes'][name] = size(desc(*c))
    out['bytes2n'][name] = size(desc(2 * c[0], *c[1:]))
    for dt in ('bf16', 'fp16'):
        for sk in (-1, 1, 2, 7):
            d = desc(*c, dtype=dt, splitk=sk)
            out['ok']['%%s %%s %%d' %% (name, dt, sk)] = call(d, size(d))
out['layer'] = [size(desc(1, 320, 320)), size(desc(32, 320, 320))]
out['capped'] = size(desc(32, 320, 320, splitk=1000000000))
b = cases['B']
bad = {
    'cin 64': desc(*b, cin=64),
    'cout 24': desc(*b, cout=24),
    'k 1': desc(*b, k=1),
    'k 5': desc(*b, k=5),
    'dilation 2': desc(*b, rate=2),
    'stride 2': desc(2, 6, 8, stride=2),
    'transpose': desc(*b, transpose=1),
    'pool': desc(*b, pool=1),
    'fp32': desc(*b, dtype='fp32'),
    'f16x3': desc(*b, dtype='f16x3'),
    'tile_cfg 1': desc(*b, tile_cfg=1),
    'splitk 0': desc(*b, splitk=0),
    'pixel limit': desc(32768, 256, 256),                    # 2^31 pixels
    'pixel limit + 1': desc(1, 1, 2 ** 31 - 31),
}
for name, d in bad.items():
    nbytes = size(d)
    msg_b = L.ron_last_error().decode()
    rc = call(d, 1 << 40)
    out['refused'][name] = [nbytes, msg_b, rc, L.ron_last_error().decode()]
d = desc(*b)
need = size(d)
rc = call(d, need, y=False)
out['refused']['relu with NULL y'] = [-1, 'x', rc, L.ron_last_error().decode()]
rc = call(d, need - 1)
out['refused']['short workspace'] = [-1, 'x', rc, L.ron_last_error().decode()]
rc = call(d, need, dy=C.c_void_p((5 << 24) + 4))
out['refused']['misaligned dy'] = [-1, 'x', rc, L.ron_last_error().decode()]
rc = call(d, need, x=False)
out['refused']['dw without x'] = [-1, 'x', rc, L.ron_last_error().decode()]
out['ok']['no relu, NULL y'] = call(desc(*b, relu=0), need, y=False)
out['ok']['NULL dw, NULL x'] = call(d, need, dw=False, x=False)
out['ok']['NULL dbias'] = call(d, need, db=False)
out['ok']['both NULL'] = call(d, need, dw=False, db=False)
out['ok']['the last pixel count'] = 0 if size(desc(1, 1, 2 ** 31 - 32)) > 0 else 1
print('RESULT ' + json.dumps(out))
'''


@pytest.fixture(scope='module')
def dry_run():
    """One child process in the library's dry-run mode (RON_PLAN_ONLY=1: every host decision, no HIP call), so that neither this
    process's library state nor a GPU is involved."""
    import json
    lib_path = os.path.join(ROOT, 'ron_tensorflow_amd', 'libron_hip.so')
    if not os.path.exists(lib_path):
        pytest.fail('%s is not built' % lib_path)
    env = dict(os.environ, RON_PLAN_ONLY='1')
    p = subprocess.run([sys.executable, '-c', _CHILD % {'root': ROOT}, json.dumps(sc.CASES)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def test_workspace_bytes(dry_run):
    """Positive, multiples of 256, and growing with n.  The workspace holds one slab per pixel slice and nothing else, so it grows where
    the slices do: never smaller at twice the batch, larger where the by-shape split has steps to spread (case G, and the layer itself
    from batch 1 to batch 32); a map of a single K step has one slab at either batch."""
    for name in sc.CASES:
        b, b2 = dry_run['bytes'][name], dry_run['bytes2n'][name]
        assert b > 0 and b % 256 == 0 and b2 % 256 == 0, (name, b, b2)
        assert b2 >= b, 'case %s: the workspace shrinks with n (%d -> %d)' % (name, b, b2)
    assert dry_run['bytes2n']['G'] > dry_run['bytes']['G']
    assert dry_run['layer'][1] > dry_run['layer'][0] > 0


def test_forced_split_is_capped(dry_run):
    """conv1_1 at batch 32 with an absurd forced split: the slabs of the slices stay below 4 GiB."""
    assert 0 < dry_run['capped'] < 4 * 2 ** 30, dry_run['capped']


def test_accepted_descriptors_plan_in_the_dry_run(dry_run):
    assert dry_run['ok'] and all(rc == 0 for rc in dry_run['ok'].values()), {k: v for k, v in dry_run['ok'].items() if v}


REASONS = {
    'cin 64': 'cin 64', 'cout 24': 'cout 24', 'k 1': 'filter 1 x 1', 'k 5': 'filter 5 x 5', 'dilation 2': 'dilation 2',
    'stride 2': 'stride 2', 'transpose': 'transpose', 'pool': 'pool', 'fp32': 'dtype', 'f16x3': 'dtype', 'tile_cfg 1': 'tile_cfg',
    'splitk 0': 'pixel split 0', 'pixel limit': 'too many pixels', 'pixel limit + 1': 'too many pixels',
    'relu with NULL y': 'y is NULL', 'short workspace': 'workspace of', 'misaligned dy': '16-byte aligned', 'dw without x': 'dw needs x',
}


@pytest.mark.parametrize('name', sorted(REASONS))
def test_refusals(dry_run, name):
    nbytes, msg_b, rc, msg = dry_run['refused'][name]
    assert nbytes == -1 and msg_b, (name, nbytes, msg_b)
    assert rc == -1 and REASONS[name] in msg, '%s: status %d (%s), RON_ERR_INVALID (-1) naming "%s" expected' % (name, rc, msg, REASONS[name])
    if msg_b != 'x':
        assert REASONS[name] in msg_b, (name, msg_b)
