"""CPU: the host-side checks of the label-free evaluation records (no device is touched: the entry points refuse before
they launch, and mpnn_exit_ev_check never launches)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

from lib import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000                       # a non-NULL pointer value; the checks never dereference device pointers


def _lib():
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _hip.load()


def _head_record(labels, cls, conf, p_cls=False, stride=10):
    e = _hip.ExitEvArgs()
    e.a.x, e.a.C, e.HW, e.n = FAKE, 16, 16, 37
    e.w_head, e.b_head, e.n_cls = FAKE, FAKE, 10
    if labels:
        e.y, e.c_err, e.d_cor = FAKE, FAKE, FAKE
    e.cls = FAKE if cls else None
    e.conf = FAKE if conf else None
    if p_cls:
        e.p_cls, e.p_stride = FAKE, stride
    return e


def test_exit_ev_check_of_label_free_heads():
    lib = _lib()
    chk = lambda e: lib.mpnn_exit_ev_check(C.byref(e))
    assert chk(_head_record(False, False, False)) == _hip.E_ARG          # no labels and nowhere to put a prediction
    assert chk(_head_record(False, True, True)) == 0
    assert chk(_head_record(False, True, False)) == _hip.E_ARG           # cls without conf
    assert chk(_head_record(False, False, True)) == _hip.E_ARG
    assert chk(_head_record(True, True, False)) == _hip.E_ARG
    assert chk(_head_record(True, False, False)) == 0                    # a fully labelled record, as before
    assert chk(_head_record(True, True, True)) == 0                      # ... and one that also stores its prediction
    assert chk(_head_record(False, True, True, p_cls=True)) == 0
    assert chk(_head_record(False, True, True, p_cls=True, stride=9)) == _hip.E_ARG      # rows shorter than n_cls
    e = _head_record(True, False, False, p_cls=True)
    assert chk(e) == _hip.E_ARG                                          # p_cls needs cls
    e = _head_record(True, False, False)
    e.c_err = None
    assert chk(e) == _hip.E_ARG                                          # the labelled rules hold unchanged
    e = _head_record(False, True, True)
    e.n_cls = 17
    assert chk(e) == _hip.E_SHAPE


def test_ev_select_refuses_bad_records_on_the_host():
    lib = _lib()
    assert lib.mpnn_ev_select(None, None) == _hip.E_ARG
    a = _hip.EvSelectArgs()
    a.n, a.n_nodes, a.n_leaves, a.n_cls = 70, _hip.MAX_NODES + 1, 4, 10
    for k in ('p_ev', 'node_ops', 'leaf_node', 'leaf_cls', 'leaf_conf', 'leaf', 'cls', 'conf', 'ops'):
        setattr(a, k, FAKE)
    a.leaf_stride = 70
    assert lib.mpnn_ev_select(C.byref(a), None) == _hip.E_SHAPE          # more nodes than mpnn_route takes
    a.n_nodes, a.n_leaves = 7, 8
    assert lib.mpnn_ev_select(C.byref(a), None) == _hip.E_SHAPE          # more leaves than nodes
    a.n_leaves, a.leaf_stride = 4, 69
    assert lib.mpnn_ev_select(C.byref(a), None) == _hip.E_ARG            # per-leaf rows shorter than the batch
    a.leaf_stride, a.ops = 70, None
    assert lib.mpnn_ev_select(C.byref(a), None) == _hip.E_ARG
    a.ops, a.probs = FAKE, FAKE
    assert lib.mpnn_ev_select(C.byref(a), None) == _hip.E_ARG            # probs without the leaves' rows
    a.n = 0
    assert lib.mpnn_ev_select(C.byref(a), None) == 0                     # nothing to do: no launch


def test_ev_select_record_matches_the_c_layout():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpnn_hip.h"', 'int main(void){',
             'printf("%zu", sizeof(mpnn_ev_select_args));']
    lines += ['printf(" %%zu", offsetof(mpnn_ev_select_args, %s));' % f for f, _ in _hip.EvSelectArgs._fields_]
    lines.append('return 0;}')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'a.c'), os.path.join(d, 'a.out')
        open(src, 'w').write('\n'.join(lines))
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe])
        nums = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert nums[0] == C.sizeof(_hip.EvSelectArgs)
    assert nums[1:] == [getattr(_hip.EvSelectArgs, f).offset for f, _ in _hip.EvSelectArgs._fields_]
    # the prediction fields sit at the END of mpnn_exit_ev_args: the offsets of the older fields did not move
    names = [f for f, _ in _hip.ExitEvArgs._fields_]
    assert names[-4:] == ['cls', 'conf', 'p_cls', 'p_stride'] and names[-5] == 'bn_eps2'
    body = re.search(r'typedef struct \{((?:(?!typedef).)*?)\} mpnn_exit_ev_args;', open(os.path.join(ROOT, 'include', 'mpnn_hip.h')).read(), re.S).group(1)
    assert body.index('bn_eps2;') < body.index('int *cls;')
