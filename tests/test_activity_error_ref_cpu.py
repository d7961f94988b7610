"""CPU: the float64 reference of ActivityError (tests/activity_error_ref.py) and the host side of the layer.

  * golden vectors: tests/golden/activity_error_ref_graph.npz, written by the reference's own ActivityError.link over the
    TensorFlow stand-in (tests/golden/activity_error_ref_graph.py --emit), alone (a row and a map, α of both signs) and
    inside a small SRNet, actor net and critic net built from the reference's own classes with the layer at all three
    positions of every exit -- per-sample costs, p_tr, and every variable after one training step -- reproduced at 1e-9 by
    the literal lines and by RefNetActivity; regenerated and compared where the reference tree is present;
  * head_bwd_extra and map_bwd_extra are the derivatives of the weighted cost (torch float64 autograd);
  * the limits of tests/test_activity_kernels.py can be met: the reference in numpy float32 stays below half of every limit
    on every kernel case;
  * no kernel that ignores α passes them: on every kernel case the float64 result with the term differs from the one without
    by more than 10 x the limit on at least half of the elements -- of the elements the layer can move at all, for the maps
    behind a ReLU: relu(bn(x)) is exactly zero on about half of a map (43 % to 52 % of these inputs are active), and a masked
    element has a zero term whatever α is; there the share is taken over the active elements and must exceed 0.99, and the
    active elements must be more than 0.4 of all;
  * the refusals: the layer anywhere but at its three positions, non-finite α, 'probs' on a head without Softmax, the
    single-scale Conv engine, and the flag parser; reg(..., activity=) / exit_activity build the chains; the new record
    fields lie where the header puts them.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import activity_error_ref as R
import exit_ref as X

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'activity_error_ref_graph.npz')
sys.path.insert(0, os.path.join(HERE, 'golden'))


# ------------------------------------------------------------------ the reference against the reference's own layer
def test_golden_vectors_of_the_reference_layer():
    import activity_error_ref_graph as G
    assert os.path.getsize(GOLDEN) < 200 * 1024
    with np.load(GOLDEN) as gold:
        for key, case in G.LAYER_CASES.items():
            x = G.layer_input(case)
            out, c_mod = R.layer(x, case['α'])
            g = gold['layer/%s/c_mod' % key]
            assert out.shape == x.shape and np.array_equal(out, x)
            assert c_mod.shape == g.shape == (case['shape'][0],), key              # per sample: every axis but the batch is summed
            assert np.abs(c_mod - g).max() <= 1e-9 * (1 + np.abs(g).max()), key
            assert (np.sign(c_mod) == np.sign(case['α'])).all()
    assert {len(c['shape']) for c in G.LAYER_CASES.values()} == {2, 4}


def _golden_net(key):
    import arch_and_hypers as A
    import lib.net_types as NT
    import activity_error_ref_graph as G
    import make_ref_graph_golden as M
    from test_ref_graph_golden import ordered
    spec = G.NETS[key]
    net = G.activity_chain(A, NT, spec)((32, 32, 3), (10,))
    params = ordered(net)
    rng = np.random.RandomState(spec['seed'])
    vals = {id(p): M.param_value(n, p.shape, rng) for n, p in params}
    return G, M, spec, net, params, vals


@pytest.mark.parametrize('key', ['sr', 'actor', 'critic'])
def test_refnet_activity_reproduces_the_reference_net(key):
    from lib._eng_common import _kind, head_activity
    G, M, spec, net, params, vals = _golden_net(key)
    leaves = [ℓ for ℓ in net.layers if not ℓ.sinks]
    assert all([type(c).__name__ for c in ℓ.comps] == ['Select', 'ActivityError', 'LinTrans', 'ActivityError', 'Softmax', 'ActivityError',
                                                       'CrossEntropyError'] and _kind(ℓ) == 'head' for ℓ in leaves)
    blocks = [2] if key == 'sr' else [0, 1, 2]
    assert [head_activity(ℓ) for ℓ in leaves] == [tuple(G.ACT[i][k] for k in ('map', 'logits', 'probs')) for i in blocks]
    ref = R.RefNetActivity(net)
    ref.load_params(vals)
    x0, y = G.net_inputs(spec)
    layers = list(net.layers)
    with np.load(GOLDEN) as gold:
        assert [n for n, _ in params] == list(gold['%s/names' % key])
        for mode in ('ev', 'tr'):
            res = ref.forward(x0, y, mode, τ=spec['tau'])
            Rr = lambda ℓ: res['out'][id(ℓ)]
            num = lambda v: v.detach().numpy() if hasattr(v, 'detach') else np.asarray(v, np.float64)
            vec = lambda v: np.broadcast_to(num(v), (len(x0),))

            def close(a, b, what):
                assert a.shape == b.shape and np.abs(a - b).max() <= 1e-9 * (1 + np.abs(b).max()), (mode, what)
            close(np.stack([vec(Rr(ℓ)['c_err']) for ℓ in leaves]), gold['%s/%s/c_err' % (key, mode)], 'c_err')
            c_mod = np.stack([vec(Rr(ℓ)['c_mod']) for ℓ in leaves])
            close(c_mod, gold['%s/%s/c_mod' % (key, mode)], 'c_mod')
            assert (c_mod.std(1) > 0).all()                                        # a per-sample vector, not the L2 scalar alone
            if key != 'sr':
                assert np.array_equal(np.stack([vec(Rr(ℓ)['p_ev']) for ℓ in layers]), gold['%s/%s/p_ev' % (key, mode)])
                close(np.stack([vec(Rr(ℓ)['p_tr']) for ℓ in layers]), gold['%s/%s/p_tr' % (key, mode)], 'p_tr')
        # one training step: every variable (parameters after the TALR-scaled momentum update, moving averages)
        ref.train_step(x0, y, M.LR, τ=spec['tau'])
        after = np.array([M.digest(ref.V(p).detach().numpy()) for _, p in params])
        g = gold['%s/after' % key]
        err = np.abs(after - g) / (1e-12 + np.abs(g).max(0, keepdims=True))
        assert err.max() <= 1e-9, ([params[i][0] for i in np.argwhere(err > 1e-9)[:, 0][:5]], err.max())


def test_golden_file_is_what_the_generator_writes(tmp_path):
    import activity_error_ref_graph as G
    if not os.path.isdir(G.REF):
        pytest.skip('the reference tree is not on this machine')
    path = str(tmp_path / 'again.npz')
    res = subprocess.run([sys.executable, os.path.join(HERE, 'golden', 'activity_error_ref_graph.py'), '--emit', path], capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    with np.load(GOLDEN) as a, np.load(path) as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            if a[k].dtype.kind in 'US':
                assert np.array_equal(a[k], b[k]), k
            else:
                assert np.abs(a[k] - b[k]).max() <= 1e-12 * (1 + np.abs(a[k]).max()), k


# ------------------------------------------------------------------ the two backward terms
def test_bwd_extras_are_the_gradients_of_the_weighted_cost():
    rng = np.random.default_rng(12)
    for n, nc in ((5, 1), (7, 3), (4, 40)):
        z, w = rng.standard_normal((n, nc)) * 2, rng.standard_normal(n)
        for α_z, α_p in ((0.3, 0.0), (0.0, -0.7), (-0.2, 1.1)):
            zt = torch.tensor(z, requires_grad=True)
            (R.cost_t(zt, torch.tensor(w), α_z) + R.cost_t(torch.softmax(zt, 1), torch.tensor(w), α_p)).backward()
            term, bound = R.head_bwd_extra(z, R.softmax(z), w, α_z, α_p)
            assert np.abs(term - zt.grad.numpy()).max() <= 1e-12 * (1 + np.abs(term).max())
            assert (np.abs(term) <= bound * (1 + 1e-12) + 1e-300).all()
        zt = torch.tensor(z, requires_grad=True)
        R.cost_t(zt, torch.tensor(w), 0.4).backward()                              # a head without Softmax
        assert np.abs(R.head_bwd_extra(z, None, w, 0.4, 0.0)[0] - zt.grad.numpy()).max() <= 1e-12
    for shape in ((3, 2, 2, 5), (6, 11)):
        x, w = np.maximum(rng.standard_normal(shape), 0), rng.standard_normal(shape[0])
        xt = torch.tensor(x, requires_grad=True)
        R.cost_t(xt, torch.tensor(w), -0.6).backward()
        term, bound = R.map_bwd_extra(x.reshape(shape[0], -1), w, -0.6)
        assert np.abs(term - xt.grad.numpy().reshape(shape[0], -1)).max() <= 1e-12
        assert np.array_equal(bound, np.abs(term)) and not term[x.reshape(shape[0], -1) == 0].any()


# ------------------------------------------------------------------ the kernel cases: limits reachable, α visible
LIN = [('tuned', k, α) for k, α in sorted(R.TUNED_LIN.items())] + [('gen', k, α) for k, α in sorted(R.GEN_LIN.items())] \
    + [('multi', X.TUNED_LIN_CASES.index(c), α) for c, α in zip(X.TUNED_LIN_MULTI, R.TUNED_LIN_MULTI_α) if α]


@pytest.mark.parametrize('family,k,α', LIN, ids=['%s-%d' % c[:2] for c in LIN])
def test_map_cases_meet_their_limits_in_float32_and_show_alpha(family, k, α):
    d = X.lin_inputs((X.LIN_CASES if family == 'gen' else X.TUNED_LIN_CASES)[k])
    w = R.act_w(d['n'], k)
    plain = X.lin_ref(d)
    ref, ref32 = R.lin_ref_with(d, plain, w, α), R.lin_ref_with(d, X.lin_ref(d, np.float32), w, α, np.float32)
    lim = R.grad_lim(ref['dx'][1])
    assert (np.abs(ref32['dx'][0] - ref['dx'][0]) <= 0.5 * lim).all()
    moved = np.abs(ref['dx'][0] - plain['dx'][0]) > 10 * lim
    active = R.lin_activated(d) != 0
    if d['mode'] == 'identity':
        assert moved.mean() >= 0.5 and active.all() and (R.lin_activated(d) < 0).any()        # raw activations, negative ones too
    else:
        assert active.mean() > 0.4 and moved[active].mean() > 0.99 and not moved[~active].any()
    if d['mode'] == 'batch':
        # the fused form: dz = masked dx and its reductions, for the reference's own mask
        fz, fz32 = X.lin_fused(d, ref), X.lin_fused(d, ref32, np.float32)
        same = fz['on'] == fz32['on']
        assert (np.abs(fz32['dz'][0] - fz['dz'][0])[same] <= 0.5 * R.grad_lim(fz['dz'][1])[same]).all() and (~same).mean() <= 1e-3
        red, bound = X.fused_red(fz, fz['on'], d['C'])
        red32, _ = X.fused_red(dict(fz32, dx=fz32['dx'].astype(np.float64), xh=fz32['xh'].astype(np.float64)), fz['on'], d['C'])
        plain_red, _ = X.fused_red(X.lin_fused(d, plain), fz['on'], d['C'])
        assert (np.abs(red32 - red) <= 0.5 * R.grad_lim(bound)).all()
        assert (np.abs(red - plain_red) > 10 * R.grad_lim(bound)).mean() >= 0.5


TAILS = [(t, name, form) for t, names in (('tuned', R.TUNED_TAIL), ('gen', R.GEN_TAIL)) for name in names for form in R.FORMS]


@pytest.mark.parametrize('family,name,form', TAILS, ids=['%s-%s-%s' % c for c in TAILS])
def test_tail_cases_meet_their_limits_in_float32_and_show_alpha(family, name, form):
    d = X.tail_inputs(name, table=R.tail_table(name))
    assert (R.tail_table(name) is X.TUNED_TAIL_CASES) == (family == 'tuned')
    plain = R.tail_dz(d, form, 0.0, 0.0)
    assert family == 'tuned' or d['nc'] > 16 and (d['nc'] >= 20 or d['n'] % 64)
    for α_z, α_p in R.ALPHAS[form]:
        assert (α_z or α_p) and not (form == 'lin' and α_p)
        dz, bound = R.tail_dz(d, form, α_z, α_p)
        dz32, _ = R.tail_dz(d, form, α_z, α_p, np.float32)
        assert (np.abs(dz32 - dz) <= 0.5 * R.dz_lim(bound)).all()
        assert (np.abs(dz - plain[0]) > 10 * R.dz_lim(bound)).mean() >= 0.5
    assert {(bool(a), bool(b)) for a, b in R.ALPHAS[form]} == ({(True, False)} if form == 'lin' else {(True, False), (False, True), (True, True)})


# ------------------------------------------------------------------ the layer on the host
def test_link_passes_x_through_and_validates_alpha():
    """Inside a Chain the layer passes x through and sets a symbolic per-sample c_mod; on its own -- a tree node, not a component --
    it stays refused, with the positions named (the position inside the chain is the engine's to judge)."""
    from lib.layer_types import ActivityError, Chain, Sym
    for x in (Sym((10,)), Sym((4, 4, 16))):
        ℓ = ActivityError(α=-0.5)
        Chain(comps=[ℓ]).link(x, Sym((10,)), 'tr')
        assert ℓ.x is x and isinstance(ℓ.c_mod, Sym) and ℓ.c_mod.producer is ℓ and ℓ.c_mod.shape == ()
        assert ℓ.c_err == 0.0 and ℓ.n_ops == 0 and vars(ℓ.params) == {} and ℓ.l2_terms == [] and ℓ.hypers.α == -0.5
    assert ActivityError().hypers.α == 0.0
    for α in (float('nan'), float('inf'), -float('inf'), np.float32('nan'), None, 'x', True):
        with pytest.raises(ValueError, match='ActivityError'):
            Chain(comps=[ActivityError(α=α)]).link(Sym((10,)), Sym((10,)), 'tr')
    ch = Chain(comps=[ActivityError(α=1), ActivityError(α=2)])
    ch.link(Sym((10,)), Sym((10,)), 'tr')
    assert ch.c_mod is ch.comps[1].c_mod and ch.c_err == 0.0
    with pytest.raises(NotImplementedError, match="behind\\s+Select.*LinTrans.*Softmax"):
        ActivityError(α=0.5).link(Sym((10,)), Sym((10,)), 'tr')


def test_reg_and_exit_activity_build_the_chains(monkeypatch):
    import arch_and_hypers as A
    from lib._eng_common import _kind, head_activity, head_parts
    from lib import _hip
    names = lambda ch: [type(c).__name__ for c in ch.comps]
    assert A.exit_activity is None and head_activity(A.reg(10)) == (0.0, 0.0, 0.0)
    ch = A.reg(10, activity={'map': 1e-4, 'logits': 0.01, 'probs': -0.5})
    assert names(ch) == ['Select', 'ActivityError', 'LinTrans', 'ActivityError', 'Softmax', 'ActivityError', 'CrossEntropyError']
    assert head_activity(ch) == (1e-4, 0.01, -0.5) and _kind(ch) == 'head' and head_parts(ch)[2] == _hip.LOSS_CE
    assert head_parts(ch)[0] is ch.comps[2] and head_parts(ch)[1] is ch.comps[-1]
    assert names(A.reg(10, activity={'logits': 2})) == ['Select', 'LinTrans', 'ActivityError', 'Softmax', 'CrossEntropyError']
    assert names(A.reg(10, activity={})) == ['Select', 'LinTrans', 'Softmax', 'CrossEntropyError']
    ch = A.reg(10, loss='squared-linear', activity={'map': 3, 'logits': -1})
    assert names(ch) == ['Select', 'ActivityError', 'LinTrans', 'ActivityError', 'SquaredError']
    assert head_activity(ch) == (3.0, -1.0, 0.0) and head_parts(ch)[2] == _hip.LOSS_SQ_LIN and _kind(ch) == 'head'
    ch = A.reg(10, loss='squared', activity={'probs': 1})
    assert names(ch)[-3:] == ['Softmax', 'ActivityError', 'SquaredError'] and head_parts(ch)[2] == _hip.LOSS_SQ
    ch = A.reg(10, np.ones((10, 2), np.float32), activity={'probs': 1})
    assert names(ch)[-2:] == ['ActivityError', 'SuperclassCrossEntropyError'] and ch.comps[1].hypers.n_chan == 2
    for bad in ({'probs': 1.0, 'z': 2}, {'map': float('nan')}, {'logits': float('inf')}, {'map': 'a'}, [('map', 1)], 0.5):
        with pytest.raises(ValueError):
            A.reg(10, activity=bad)
    with pytest.raises(ValueError, match='Softmax'):
        A.reg(10, loss='squared-linear', activity={'probs': 1.0})
    # several layers at one position add their α
    from lib.layer_types import ActivityError, Chain
    ch = A.reg(10, activity={'logits': 0.25})
    ch.comps.insert(3, ActivityError(α=0.5))
    ch.comps.insert(1, ActivityError(α=-2))
    ch.comps.insert(1, ActivityError(α=3))
    assert _kind(ch) == 'head' and head_activity(ch) == (1.0, 0.75, 0.0)
    # the knob: one dict for every exit, or {block index: dict}
    monkeypatch.setattr(A, 'arch', A.arch[:3])
    monkeypatch.setattr(A, 'exit_activity', {'logits': 0.01})
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert [head_activity(ℓ) for ℓ in net.leaves] == [(0.0, 0.01, 0.0)] * 3
    monkeypatch.setattr(A, 'exit_activity', {0: {'map': 1e-4}, 2: {'probs': 0.5, 'logits': -1}})
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert [head_activity(ℓ) for ℓ in net.leaves] == [(1e-4, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, -1.0, 0.5)]
    net = A.sr_chain(3)((32, 32, 3), (10,))
    assert [head_activity(ℓ) for ℓ in net.leaves] == [(0.0, -1.0, 0.5)]


def test_the_flag_parser():
    import arch_and_hypers as A
    assert A.parse_exit_activity('logits=0.01') == {'logits': 0.01}
    assert A.parse_exit_activity('logits=0.01,map=1e-4:2') == {0: {'logits': 0.01, 'map': 1e-4}, 1: {'logits': 0.01, 'map': 1e-4}}
    assert A.parse_exit_activity('probs=-0.5:0') == {}
    for bad in ('', 'logits', 'logits=', 'z=1', 'logits=nan', 'map=inf', 'map=1,map=2', 'map=1:', 'map=1:k', 'map=1;logits=2', 'map=1,'):
        with pytest.raises(ValueError, match='--exit-activity'):
            A.parse_exit_activity(bad)


POSITIONS = "behind Select.*behind the\\s+LinTrans.*behind the Softmax"


def test_every_other_position_is_refused(monkeypatch):
    import arch_and_hypers as A
    from lib._eng_common import _kind
    from lib.layer_types import ActivityError, Chain
    monkeypatch.setattr(A, 'arch', A.arch[:2])

    def at(k):
        def put(ch):
            ch.comps.insert(k, ActivityError(α=0.1))
            return ch
        return put
    for k in (0, 4):                                       # in front of Select; behind the error layer
        with pytest.raises(NotImplementedError, match=POSITIONS):
            _kind(at(k)(A.reg(10)))
    with pytest.raises(NotImplementedError, match=POSITIONS):
        _kind(at(3)(A.reg(10, loss='squared-linear')))     # behind SquaredError
    block = A.rcm(0)
    block.comps.append(ActivityError(α=0.1))               # a block chain: the layer on a multiscale list
    with pytest.raises(NotImplementedError, match=POSITIONS):
        _kind(block)
    pyr = A.pyr(A.rcm(0, A.reg(10)))
    pyr.comps.append(ActivityError(α=0.1))
    with pytest.raises(NotImplementedError, match=POSITIONS):
        _kind(pyr)


def test_probs_on_a_linear_head_is_refused_by_reg():
    import arch_and_hypers as A
    with pytest.raises(ValueError):
        A.reg(10, loss='squared-linear', activity={'probs': 0.1, 'map': 1.0})


def test_single_scale_conv_nets_refuse_the_layer():
    from lib._plan_conv import is_conv_net
    from lib.layer_types import ActivityError, Chain, Conv, CrossEntropyError, GlobalMaxPool, LinTrans, Rect, Softmax
    from lib.net_types import SRNet

    def net(head_extra, root_extra):
        head = Chain(name='LogReg', comps=[LinTrans(n_chan=10)] + head_extra + [Softmax(), CrossEntropyError()])
        root = Chain(name='Conv', sinks=[head], comps=[Conv(n_chan=16, supp=3), Rect()] + root_extra + [GlobalMaxPool()])
        return SRNet(x0_shape=(16, 16, 3), y_shape=(10,), root=root)
    assert is_conv_net(net([], []))
    for n in (net([ActivityError(α=0.1)], []), net([], [ActivityError(α=0.1)])):
        with pytest.raises(NotImplementedError, match=POSITIONS):
            is_conv_net(n)


def test_record_fields_match_the_c_layout():
    """act_alpha / act_w are the last members of mpnn_lin_bwd_args, act_z / act_p of mpnn_exit_tail_bwd_args, as gcc sees the
    header; mpnn_exit_tail_args still ends with `loss` and has the size it had (tests/test_squared_error_ref_cpu.py pins both), so
    no offset of the forward record or of the older backward fields moved; a fresh record reads zeros."""
    import ctypes
    import tempfile
    from lib import _hip
    root = os.path.dirname(HERE)
    q = [('mpnn_lin_bwd_args', f) for f in ('kcnt', 'act_alpha', 'act_w')] + [('mpnn_exit_tail_args', f) for f in ('loss',)] \
        + [('mpnn_exit_tail_bwd_args', f) for f in ('w_cerr', 'dh2', 'act_z', 'act_p')]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpnn_hip.h"', 'int main(void){']
    lines += ['printf("%%zu ", offsetof(%s, %s));' % c for c in q]
    lines += ['printf("%%zu ", sizeof(%s));' % r for r in ('mpnn_lin_bwd_args', 'mpnn_exit_tail_args', 'mpnn_exit_tail_bwd_args')] + ['return 0;}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'a.c'), os.path.join(d, 'a.out')
        open(src, 'w').write('\n'.join(lines))
        subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), src, '-o', exe])
        v = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    L, T, B = _hip.LinBwdArgs, _hip.ExitTailArgs, _hip.ExitTailBwdArgs
    mirror = {'mpnn_lin_bwd_args': L, 'mpnn_exit_tail_args': T, 'mpnn_exit_tail_bwd_args': B}
    assert v[:len(q)] == [getattr(mirror[r], f).offset for r, f in q]
    assert v[len(q):] == [ctypes.sizeof(L), ctypes.sizeof(T), ctypes.sizeof(B)]
    assert [f[0] for f in L._fields_[-2:]] == ['act_alpha', 'act_w'] and T._fields_[-1][0] == 'loss' and [f[0] for f in B._fields_[-3:]] == ['dh2', 'act_z', 'act_p']
    l, t = L(), B()
    assert l.act_alpha == 0 and not l.act_w and t.act_z == 0 and t.act_p == 0
    assert B.w_cerr.offset == ctypes.sizeof(T)                             # (the embedded forward record is the first member, unchanged)
