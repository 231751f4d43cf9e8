"""CPU test: the 256 x 224 form of the four-wave assembly K loop (csrc/kloop4w.inc, tools/gen_kloop4w.py) under the checks of
tests/test_isa_protocol.py.

Two levels.  The generated text itself (no compiler): the committed kloop4w.inc is what the generator writes, and the two 224-column
loops hold 15 LDS-DMA pieces per K step (8 of A, 7 of B), two tiles of them in the prologue behind `vmcnt(15)`, one `vmcnt(12)` in the
step with exactly 12 pieces in front of it, three barriers, 112 MFMAs into a[0:223] and never a piece directly behind an M0 write.
Then the ISA hipcc emits for conv_mfma4w.hip (tools/check_dma_counts.py, cross-compiled for gfx950): the same counts in the two new
kernels and in the two grouped kernels for launches with a 224-column member (template argument N224 = true), which hold the
256-column and the 224-column loop side by side - the other grouped kernels keep their one loop - and no compiler-generated
instruction that touches an accumulation register behind a loop."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import check_dma_counts as cdc  # noqa: E402

INC = os.path.join(ROOT, 'ron_tensorflow_amd', 'csrc', 'kloop4w.inc')


def _macro(name):
    """The instructions of `#define <name>` in kloop4w.inc, one per list entry."""
    text = open(INC).read()
    body = text.split('#define %s \\\n' % name)[1].split('\n\n')[0]
    return re.findall(r'"(.*?)\\n"', body)


def test_committed_include_is_what_the_generator_writes(tmp_path):
    out = tmp_path / 'kloop4w.inc'
    env = dict(os.environ, KLOOP_OUT=str(out))
    env.pop('KLOOP_OPTS', None)
    subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_kloop4w.py')], check=True, env=env, stdout=subprocess.DEVNULL)
    assert out.read_text() == open(INC).read(), 'kloop4w.inc is stale: run tools/gen_kloop4w.py'


@pytest.mark.parametrize('dtype, mfma', [('BF16', 'v_mfma_f32_16x16x32_bf16'), ('F16', 'v_mfma_f32_16x16x32_f16')])
def test_224_column_loop_text(dtype, mfma):
    ins = _macro('RON_KLOOP4W_N224_%s' % dtype)
    top = ins.index('.Lk4w_loop_%=:')
    end = ins.index('s_cbranch_scc0 .Lk4w_loop_%=')
    pro, body = ins[:top], ins[top:end]
    is_dma = lambda s: s.startswith('buffer_load_dwordx4') and s.endswith(' lds')
    # prologue: two tiles of 7 + 8 pieces, and the wait that leaves the second one in flight
    assert sum(map(is_dma, pro)) == 30
    assert 's_waitcnt vmcnt(15)' in pro
    # the step: 15 pieces (7 of B through s[52:55], 8 of A through s[48:51]), one counted wait with 12 of them in front of it
    dma = [s for s in body if is_dma(s)]
    assert len(dma) == 15
    assert sum('s[52:55]' in s for s in dma) == 7 and sum('s[48:51]' in s for s in dma) == 8
    waits = [i for i, s in enumerate(body) if 'vmcnt' in s]
    assert [body[i] for i in waits] == ['s_waitcnt vmcnt(12)']
    assert sum(map(is_dma, body[:waits[0]])) == 12
    assert body[waits[0] + 1].startswith(mfma) and body[waits[0] + 2] == 's_barrier'      # wait, then the barrier, then the reads
    assert body.count('s_barrier') == 3
    # 112 MFMAs: every block (i, j), i < 8, j < 7, once per k-half, accumulating in place in a[4 * (7 i + j) : +3]
    mm = [s for s in body if s.startswith(mfma)]
    assert len(mm) == 112
    accs = [int(re.match(r'\S+ a\[(\d+):', s).group(1)) for s in mm]
    assert accs[:56] == accs[56:] == [4 * b for b in range(56)]
    for s in mm:
        d, c = re.match(r'\S+ a\[(\d+):(\d+)\], .* a\[(\d+):(\d+)\]$', s).group(1, 3)
        assert d == c
    # fragment reads: 7 + 8 per k-half
    assert sum(s.startswith('ds_read_b128') for s in body) == 30
    # M0 is written by SALU instructions; the piece that uses it never follows directly
    for k, s in enumerate(body):
        if is_dma(s):
            assert 'm0' not in body[k - 1], (body[k - 1], s)
    # nothing of the 256-column tile's last block column: accumulators a224 .. a255 and the eighth B fragments stay untouched
    text = '\n'.join(ins)
    assert not re.search(r'\ba(22[4-9]|2[3-5]\d)\b', text) and not re.search(r'a\[(22[4-9]|2[3-5]\d):', text)
    assert 'v[188:191]' not in text and 'v[252:255]' not in text and ' v115,' not in text


def test_224_accumulator_reader_covers_its_register_map():
    text = open(INC).read()
    body = text.split('#define RON_ACC4W_N224_CASES \\\n')[1].split('\n\n')[0]
    cases = re.findall(r'case (\d+): asm volatile\("(.*?)" :', body)
    assert [int(c) for c, _ in cases] == list(range(32))
    seen = []
    for c, txt in cases:
        i, e = divmod(int(c), 4)
        regs = [int(r) for r in re.findall(r'v_accvgpr_read_b32 %\d+, a(\d+)', txt)]
        assert regs == [4 * (7 * i + j) + e for j in range(7)]
        seen += regs
    assert sorted(seen) == list(range(224))


@pytest.fixture(scope='module')
def checked():
    if not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('hipcc not available')
    return cdc.check_file('conv_mfma4w.hip')


def test_emitted_isa_of_the_224_kernels_and_the_two_loop_group_kernels(checked):
    assert len(checked) == cdc.EXPECTED['conv_mfma4w.hip']
    new = [(d, p) for d, p in checked if '<256, 224, 2, 2, 2' in d]
    assert sorted(d.split()[0] for d, _ in new) == ['BF16', 'F16']
    group = [(d, p) for d, p in checked if 'group_kernel' in d]
    assert len(group) == 5 and sorted(d.split()[0] for d, _ in group if '+224' in d) == ['BF16', 'F16']
    bad = ['%s: %s' % (d, '; '.join(p)) for d, p in new + group if p]
    assert not bad, '\n'.join(bad)


def test_the_checker_counts_both_loops_of_a_group_kernel():
    """The check itself: the grouped kernel for launches with a 224-column member (N224 = true) is expected to hold a 16-piece and a
    15-piece loop, every other grouped kernel and the stand-alone kernels a single loop."""
    g = '_ZN3ron6detail23conv_igemm_group_kernelINS0_%sELi256ELi256ELi2ELi2ELi2ELi1ELb1EEEvNS0_13ConvGroupArgsE'
    assert cdc.asm4w_pieces(g % '11TraitsBF16S') == [16, 15]
    assert cdc.asm4w_pieces(g % '10TraitsF16S') == [16, 15]
    assert cdc.asm4w_pieces((g % '11TraitsBF16S').replace('ELb1E', 'ELb0E')) == [16]
    assert cdc.asm4w_pieces((g % '12TraitsF16X3S').replace('ELb1E', 'ELb0E')) == [16]
    k = '_ZN3ron6detail17conv_igemm_kernelINS0_11TraitsBF16SELi256ELi%dELi2ELi2ELi2ELi1EEEvNS0_8ConvArgsE'
    assert [cdc.asm4w_pieces(k % bn) for bn in (256, 224, 128)] == [[16], [15], [12]]
    dma = '\tbuffer_load_dwordx4 v1, s[0:3], s4 offen lds'

    def loop(pieces, before, tag):
        return (['\t;;#ASMSTART'] + [dma] * (2 * pieces) + ['\ts_waitcnt vmcnt(%d)' % pieces, '.Lk4w_loop_%d:' % tag] + [dma] * before +
                ['\ts_waitcnt vmcnt(%d)' % before] + ['\ts_barrier'] * 3 + [dma] * (pieces - before) +
                ['\ts_cbranch_scc0 .Lk4w_loop_%d' % tag, '\t;;#ASMEND', '\t;;#ASMSTART', '\tv_accvgpr_read_b32 v1, a0', '\t;;#ASMEND'])
    name = g % '11TraitsBF16S'
    assert cdc.check_asm4w(name, loop(16, 13, 1) + loop(15, 12, 2)) == []
    assert any('expected 2' in p for p in cdc.check_asm4w(name, loop(16, 13, 1)))
    assert cdc.check_asm4w(name, loop(16, 13, 1) + loop(15, 11, 2) + [dma]) != []          # a piece short in front of the wait, one stray
    touched = loop(16, 13, 1) + loop(15, 12, 2) + ['\tv_accvgpr_write_b32 a3, v2']
    assert any('accumulation registers' in p for p in cdc.check_asm4w(name, touched))
