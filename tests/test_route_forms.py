"""GPU: the launch forms of mpnn_route (csrc/route.hip) that tests/test_exit_kernels.py::test_route_against_oracle does
not reach -- that test runs the 64-samples-per-workgroup kernel on at most two workgroups, with atomics, gradients on,
n_total == n and cleared accumulators.  Same oracle (oracle/route_ref.route), trees and tolerances (route_close):

  deterministic statistics   more than two workgroups with stat_part / stat_ticket: the last workgroup to arrive adds the
                             partial sums in workgroup order onto PRE-FILLED node_stat / loss, resets the ticket and
                             stays inside the exchange buffer; two launches from the same buffers give the same bits.
                             The same batches with stat_part = NULL (atomics).
  32 samples per workgroup   a tree whose tables do not fit 160 KB at 64 samples (the host formula, restated in
                             tests/step_end_ref.py, is asserted to pick 32), static and per-sample k_cpt
  evaluation form            node_stat = NULL, want_grad = 0: dr keeps its bits
  n_total = 4 n              gradients scale by n / n_total, the loss sums and the sample count do not
  mpnn_route_multi           three nets of one tree in one launch == three mpnn_route launches, bit for bit
(16 samples per workgroup: no tree within MPNN_MAX_NODES / MPNN_MAX_SINKS selects it --
tests/test_step_end_ref_cpu.py::test_no_tree_selects_sixteen_samples_per_workgroup.)
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lib import _hip
from hiputil import DEV, stream
import step_end_ref as R
from test_exit_kernels import OUTS, SENT32, RouteCase      # the builder test_route_against_oracle uses too


def bits(o):
    out = {k: o[k].buf.cpu().numpy() for k in OUTS}
    return {k: v.view(np.uint32 if v.dtype == np.float32 else np.uint64) for k, v in out.items()}


def same(a, b, what, skip=()):
    x, y = bits(a), bits(b)
    for k in OUTS:
        if k not in skip:
            assert np.array_equal(x[k], y[k]), '%s: %s differs' % (what, k)


# ---------------------------------------------------------------------------------------------------- the exchange
@pytest.mark.parametrize('kind,n', [('actor', 200), ('actor', 129), ('critic', 200), ('critic', 129), ('sr', 200)])
def test_route_deterministic_statistics(kind, n):
    cs = RouteCase(kind, 'chain8', n, seed=len(kind) * 1000 + n)
    assert cs.rb == 64 and cs.wgs == {200: 4, 129: 3}[n] and cs.wgs > 2 and n - (cs.wgs - 1) * 64 == {200: 8, 129: 1}[n]
    first = cs.launch(cs.outputs())
    cs.check(first)
    # the exchange buffer: workgroup b's [n_nodes][2] partial sums, then [workgroups][4] doubles; nothing beyond them
    part = first['part'].get()
    used = cs.wgs * (2 * cs.NN + 8)
    assert np.isfinite(part[:used]).all() and (part[used:] == SENT32).all()
    stat_parts = part[:cs.wgs * 2 * cs.NN].reshape(cs.wgs, cs.NN, 2).astype(np.float64)
    assert np.abs(stat_parts.sum(0) - cs.ref['node_stat']).max() <= 1e-5 * (1 + np.abs(cs.ref['node_stat']).max())
    again = cs.launch(cs.outputs())
    same(first, again, 'two launches from the same buffers')
    # the same batch through atomics
    atom = cs.launch(cs.outputs(), det=False)
    cs.check(atom)
    assert (atom['part'].get() == SENT32).all()
    same(first, atom, 'atomics against the exchange', skip=('stat', 'loss', 'part'))


# ---------------------------------------------------------------------------------------------------- 32 samples
@pytest.mark.parametrize('kind,dyn', [('actor', False), ('critic', False), ('actor', True)])
def test_route_32_samples_per_workgroup(kind, dyn):
    cs = RouteCase(kind, 'ternary', 70, seed=7 + dyn, dyn=dyn)
    assert (cs.NN, cs.ns, cs.nl, cs.MS) == (122, 40, 81, 3)
    per, fix = R.route_lds_floats(cs.NN, cs.ns, cs.nl, cs.MS)
    assert per == 930 and (per * 64 + fix) * 4 > 160 * 1024 >= (per * 32 + fix) * 4 and cs.rb == 32      # 238 KB / 119 KB
    assert cs.wgs == 3 and 70 - 2 * 32 == 6
    first = cs.launch(cs.outputs())
    cs.check(first)
    same(first, cs.launch(cs.outputs()), 'two launches from the same buffers')


# ---------------------------------------------------------------------------------------------------- evaluation, n_total
@pytest.mark.parametrize('kind', ['actor', 'critic'])
def test_route_evaluation_form(kind):
    cs = RouteCase(kind, 'mixed', 150, seed=len(kind))
    assert cs.wgs == 3
    o = cs.launch(cs.outputs(), det=False, want_grad=0, stat=False, w_cerr=False)
    cs.check(o, grads=False, stat=False, w_cerr=False)
    assert (o['dr'].get() == SENT32).all() and (o['part'].get() == SENT32).all()


@pytest.mark.parametrize('kind', ['actor', 'critic'])
def test_route_mean_over_n_total(kind):
    cs = RouteCase(kind, 'mixed', 150, seed=3 + len(kind))
    assert cs.wgs == 3                                 # (the exchange, not atomics)
    o = cs.launch(cs.outputs(), n_total=4 * cs.n)
    cs.check(o, scale=0.25)


# ---------------------------------------------------------------------------------------------------- several nets
@pytest.mark.parametrize('n', [128, 200])
@pytest.mark.parametrize('kind', ['actor', 'critic'])
def test_route_multi_is_three_launches(kind, n):
    lib = _hip.load()
    nets = [RouteCase(kind, 'chain8', n, seed=50 + k, vary=True) for k in range(3)]
    det = n == 200                                     # (two workgroups: atomics whatever stat_part says -- onto CLEARED sums)
    assert nets[0].wgs == (4 if det else 2)
    single = [cs.launch(cs.outputs(prefill=det), det=det) for cs in nets]
    outs = [cs.outputs(prefill=det) for cs in nets]
    recs = [cs.args(o, det=det) for cs, o in zip(nets, outs)]
    host = (_hip.RouteArgs * 3)(*recs)
    tab = _hip.to_device_table(recs, DEV)
    _hip.check(lib.mpnn_route_multi(host, tab.data_ptr(), 3, stream()), 'route_multi')
    for k, (cs, o) in enumerate(zip(nets, outs)):
        cs.done(o)
        cs.check(o, prefill=det)
        same(o, single[k], 'net %d of mpnn_route_multi against its own launch' % k)
