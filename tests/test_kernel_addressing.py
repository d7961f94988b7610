"""The memory-access form of the record-driven kernels, read from the generated code (no GPU: hipcc cross-compiles).

A kernel whose pointers arrive as kernel arguments is compiled to global_* accesses and counted `s_waitcnt vmcnt(N)`
waits.  A kernel that LOADS its pointers from a record in device memory (the grouped forward convs, the backward levels,
the exit path's table-driven launches, the co-training forms) gets flat_* accesses through every such pointer unless the
pointer is typed as global (gptr, csrc/common.h): a 64-bit vector address per access, a wait on lgkmcnt as well, and
only vmcnt(0) behind it -- which drains the prefetch the unit loops of csrc/conv_kernel.h keep in flight.  Nothing else
in the tree looks at the generated code, so this does:

  * the hot-path translation units are compiled device-only to assembly with the Makefile's own flags (in parallel);
  * the record-driven kernels are found from the SYMBOLS: every kernel with a pointer-to-struct parameter (Itanium
    `PK<len><name>`: a table of argument records) -- a new one is covered without a list to keep -- plus finish_opt_k,
    whose gradient operand comes from LDS or from global memory and must not be merged into one flat load;
  * each of them has no flat_load, flat_store or flat_atomic instruction;
  * the three pipelines the training step spends most of its time in also have at least one counted wait.

The evaluation kernels of exit_ev.hip, exit_gen.hip and the conv_gen family still carry plain pointers (they are
not on the training step) and are not compiled here."""
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'multipath-nn_amd', 'csrc')
UNITS = ('conv_fwd', 'conv_first', 'bwd_level', 'bwd_level_small', 'lin', 'exit_tail', 'route', 'wgrad')
EXTRA_KERNELS = ('_Z12finish_opt_k',)                 # by-value, but named by its LDS-or-global gradient operand
# kernel-name prefixes (mangled: fwd_group_k<false, false, false>, fwd_ks_k<2, 2>, bwd_level_k<5, 1, false>)
PIPELINES = ('_Z11fwd_group_kILb0ELb0ELb0EE', '_Z8fwd_ks_kILi2ELi2EE', '_Z11bwd_level_kILi5ELi1ELb0EE')
FLAT = ('flat_load', 'flat_store', 'flat_atomic')


def makefile_flags():
    """CXXFLAGS of csrc/Makefile with its variables filled in (EXTRA empty)."""
    text = open(os.path.join(CSRC, 'Makefile')).read().replace('\\\n', ' ')
    m = re.search(r'^CXXFLAGS\s*:=\s*(.*)$', text, re.M)
    assert m, 'no CXXFLAGS in csrc/Makefile'
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
    flags = m.group(1).replace('$(ARCH)', arch).replace('$(ROOT)', ROOT).replace('$(EXTRA)', '')
    return flags.split()


def parse_kernels(path):
    """{kernel symbol: [instruction lines]} of one assembly file."""
    lines = open(path).read().split('\n')
    kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', '\n'.join(lines), re.M))
    out, cur = {}, None
    for ln in lines:
        m = re.match(r'^(\w+):', ln)
        if m and m.group(1) in kernels:
            cur = out.setdefault(m.group(1), [])
            continue
        if re.match(r'^\.Lfunc_end\d+:', ln):
            cur = None
        elif cur is not None and ln.startswith('\t') and not ln.startswith('\t.') and not ln.startswith('\t;'):
            cur.append(ln.strip())
    return out


def record_driven(sym):
    return re.search(r'PK\d+[A-Za-z_]', sym) is not None or sym.startswith(EXTRA_KERNELS)


@pytest.fixture(scope='module')
def kernels():
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not available')
    flags = makefile_flags()
    tmp = tempfile.mkdtemp(prefix='mpnn_asm_')

    def compile_unit(u):
        out = os.path.join(tmp, u + '.s')
        r = subprocess.run(['hipcc'] + flags + ['--cuda-device-only', '-S', u + '.hip', '-o', out], cwd=CSRC,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, (u, r.stdout[-2000:])
        return parse_kernels(out)
    try:
        with ThreadPoolExecutor(max_workers=min(len(UNITS), os.cpu_count() or 1, 16)) as ex:
            found = {}
            for ks in ex.map(compile_unit, UNITS):
                found.update(ks)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return found


def test_record_driven_kernels_use_global_accesses(kernels):
    names = [k for k in kernels if record_driven(k)]
    # the families this is about are all there (a rename must not empty the test)
    for fam in ('fwd_group_k', 'fwd_ks_k', 'bwd_level_k', 'lin_fwd_k', 'lin_bwd_k', 'exit_tail_fwd_k', 'exit_tail_bwd_k',
                'exit_tail_fwd_big_k', 'exit_tail_bwd_big_k', 'fwd_first_k', 'route_multi_k', 'finish_opt_multi_k', 'finish_opt_k'):
        assert any(re.match(r'_Z%d%s' % (len(fam), fam), k) for k in names), fam + ': no such kernel found'
    bad = {}
    for k in names:
        n = {f: sum(1 for ins in kernels[k] if ins.startswith(f)) for f in FLAT}
        if any(n.values()):
            bad[k] = n
    assert not bad, 'flat accesses in record-driven kernels: %r' % bad


def test_by_value_kernels_have_none_either(kernels):
    """The kernels that take their pointers as arguments never had flat accesses; they share every helper with the
    record-driven ones and must stay that way."""
    bad = {k: n for k in kernels if not record_driven(k)
           for n in [sum(1 for ins in kernels[k] if ins.startswith(FLAT))] if n}
    assert not bad, bad


@pytest.mark.parametrize('prefix', PIPELINES)
def test_prefetch_pipelines_wait_with_counts(kernels, prefix):
    ks = [k for k in kernels if k.startswith(prefix)]
    assert len(ks) == 1, (prefix, ks)
    counted = [ins for ins in kernels[ks[0]] if ins.startswith('s_waitcnt') and re.search(r'vmcnt\(([1-9]\d*)\)', ins)]
    assert counted, ks[0] + ': every wait on memory is vmcnt(0)'
