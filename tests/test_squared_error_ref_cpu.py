"""CPU: the float64 reference of SquaredError (tests/squared_error_ref.py) and the host side of the layer.

  * golden vectors: tests/golden/squared_error_ref_graph.npz, written by the reference's own SquaredError.link over the
    TensorFlow stand-in (tests/golden/squared_error_ref_graph.py --emit), alone (both forms, one-hot and real-valued
    targets, tied maxima, outputs below -1) and inside a small actor net and a small critic net (use_cls_err) built from
    the reference's own classes -- forward quantities, and every variable after one training step (each moved by its own
    gradient) -- reproduced at 1e-9 by the literal lines and by RefNetSquared; regenerated and compared where the
    reference tree is present;
  * head_bwd is the derivative of head_fwd (torch float64 autograd);
  * the limits of tests/test_squared_head_kernels.py can be met: the reference in numpy float32 stays below half of
    every limit on every kernel case, and every row without an exact tie has a top-two gap above 1e-4 in x and in y, so no
    row is exempt from the d_cor / cls comparison;
  * link and its refusals, reg(..., loss=) / exit_loss / --exit-loss, the kind of the head chains, the ConvEngine refusal.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import squared_error_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'squared_error_ref_graph.npz')
sys.path.insert(0, os.path.join(HERE, 'golden'))


def test_golden_vectors_of_the_reference_layer():
    import squared_error_ref_graph as G
    assert os.path.getsize(GOLDEN) < 200 * 1024
    both = 0
    with np.load(GOLDEN) as gold:
        for key, case in G.LAYER_CASES.items():
            x, y = G.layer_input(case)
            c_err, d_cor = R.layer(x, y)
            g = gold['layer/%s/c_err' % key]
            assert c_err.shape == g.shape == (case['n'],)
            assert np.abs(c_err - g).max() <= 1e-9 * (1 + np.abs(g).max()), key
            assert np.array_equal(d_cor, gold['layer/%s/d_cor' % key]), key
            both += 0 < d_cor.sum() < case['n']
            # head_fwd on the same rows: x itself in the linear form, the softmax of log x in the other
            f = R.head_fwd(np.log(x) if case['form'] == 'sq' else x, y, case['form'])
            assert np.abs(f['c_err'] - g).max() <= 1e-9 * (1 + np.abs(g).max()), key
            if not case.get('tie'):
                assert np.array_equal(f['d_cor'], d_cor), key
    assert both >= 4                                                       # (both answers occur)
    for key in ('sq_tie', 'lin_tie'):                                      # the two largest outputs are equal in every row
        x, _ = G.layer_input(G.LAYER_CASES[key])
        assert all(np.sort(r)[-1] == np.sort(r)[-2] for r in x)
    x, _ = G.layer_input(G.LAYER_CASES['lin_negative'])
    assert x.max() < -1                                                    # below the probability sentinel of the heads


def _golden_net(key):
    import arch_and_hypers as A
    import lib.net_types as NT
    import squared_error_ref_graph as G
    import make_ref_graph_golden as M
    from test_ref_graph_golden import ordered
    spec = G.NETS[key]
    net = G.squared_chain(A, NT, spec)((32, 32, 3), (10,))
    params = ordered(net)
    rng = np.random.RandomState(spec['seed'])
    vals = {id(p): M.param_value(n, p.shape, rng) for n, p in params}
    return G, M, spec, net, params, vals


@pytest.mark.parametrize('key', ['actor', 'critic'])
def test_refnet_squared_reproduces_the_reference_net(key):
    G, M, spec, net, params, vals = _golden_net(key)
    assert [type(ℓ.comps[-1]).__name__ for ℓ in net.leaves] == ['SquaredError', 'SquaredError', 'CrossEntropyError']
    assert [len(ℓ.comps) for ℓ in net.leaves] == [4, 3, 4]
    ref = R.RefNetSquared(net)
    ref.load_params(vals)
    x0, y = G.net_inputs(spec)
    layers = list(net.layers)
    leaves = [ℓ for ℓ in layers if not ℓ.sinks]
    with np.load(GOLDEN) as gold:
        assert [n for n, _ in params] == list(gold['%s/names' % key])
        for mode in ('ev', 'tr'):
            res = ref.forward(x0, y, mode, τ=spec['tau'])
            Rr = lambda ℓ: res['out'][id(ℓ)]
            num = lambda v: v.detach().numpy() if hasattr(v, 'detach') else np.asarray(v, np.float64)
            vec = lambda v: np.broadcast_to(num(v), (len(x0),))

            def close(a, b, what):
                assert a.shape == b.shape and np.abs(a - b).max() <= 1e-9 * (1 + np.abs(b).max()), (mode, what)
            assert np.array_equal(np.stack([vec(Rr(ℓ)['p_ev']) for ℓ in layers]), gold['%s/%s/p_ev' % (key, mode)])
            close(np.stack([vec(Rr(ℓ)['p_tr']) for ℓ in layers]), gold['%s/%s/p_tr' % (key, mode)], 'p_tr')
            close(np.stack([vec(Rr(ℓ)['c_err']) for ℓ in leaves]), gold['%s/%s/c_err' % (key, mode)], 'c_err')
            assert np.array_equal(np.stack([vec(Rr(ℓ)['δ_cor']) for ℓ in leaves]), gold['%s/%s/d_cor' % (key, mode)])
        # one training step: every variable (parameters after the TALR-scaled momentum update, moving averages)
        ref.train_step(x0, y, M.LR, τ=spec['tau'])
        after = np.array([M.digest(ref.V(p).detach().numpy()) for _, p in params])
        g = gold['%s/after' % key]
        err = np.abs(after - g) / (1e-12 + np.abs(g).max(0, keepdims=True))
        assert err.max() <= 1e-9, ([params[i][0] for i in np.argwhere(err > 1e-9)[:, 0][:5]], err.max())


def test_golden_file_is_what_the_generator_writes(tmp_path):
    import squared_error_ref_graph as G
    if not os.path.isdir(G.REF):
        pytest.skip('the reference tree is not on this machine')
    path = str(tmp_path / 'again.npz')
    res = subprocess.run([sys.executable, os.path.join(HERE, 'golden', 'squared_error_ref_graph.py'), '--emit', path], capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    with np.load(GOLDEN) as a, np.load(path) as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            if a[k].dtype.kind in 'US':
                assert np.array_equal(a[k], b[k]), k
            else:
                assert np.abs(a[k] - b[k]).max() <= 1e-12 * (1 + np.abs(a[k]).max()), k


# ------------------------------------------------------------------ the heads
@pytest.mark.parametrize('form', R.FORMS)
def test_head_bwd_is_the_gradient_of_head_fwd(form):
    rng = np.random.default_rng(11)
    for n, nc in ((5, 1), (7, 3), (4, 40)):
        z, y, w = rng.standard_normal((n, nc)) * 2, rng.standard_normal((n, nc)), rng.standard_normal(n)
        zt = torch.tensor(z, requires_grad=True)
        head = R.head_fwd_t(zt, torch.tensor(y), form)
        (head * torch.tensor(w)).sum().backward()
        dz, bound = R.head_bwd(z, y, w, form)
        assert np.abs(head.detach().numpy() - R.head_fwd(z, y, form)['c_err']).max() <= 1e-12
        assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12 * (1 + np.abs(dz).max())
        assert (np.abs(dz) <= bound * (1 + 1e-12) + 1e-300).all()


TAIL = R.tail_cases()


@pytest.mark.parametrize('case', TAIL, ids=[c[0] for c in TAIL])
def test_float32_reference_meets_the_tail_limits(case):
    cid, family, form, (z, y, w) = case
    f, f32 = R.head_fwd(z, y, form), R.head_fwd(z, y, form, np.float32)
    assert (np.abs(f32['c_err'] - f['c_err']) <= 0.5 * R.c_err_lim(f['c_err'])).all()
    dz, bound = R.head_bwd(z, y, w, form)
    dz32, _ = R.head_bwd(z, y, w, form, np.float32)
    assert (np.abs(dz32 - dz) <= 0.5 * R.dz_lim(dz, bound)).all()
    assert np.array_equal(f32['d_cor'], f['d_cor'])
    rows = R.no_tie_rows(cid, z)
    assert (f['gap_x'][rows] > 1e-4).all() and (f['gap_y'][rows] > 1e-4).all()
    if cid.endswith('ties'):
        top = lambda v: (v == v.max(1, keepdims=True)).sum(1)
        assert (top(z) >= 2).all() and (top(y) >= 2).all() and (top(f['x']) >= 2).all()
        assert 0 < f['d_cor'].sum() < len(z)
    if cid.endswith('sentinel'):
        assert z.max() <= -2 and z.min() >= -9 and (form == 'sq' or f['x'].max() < -1)


EV = R.ev_all_inputs()


@pytest.mark.parametrize('case', EV, ids=[c[0] for c in EV])
def test_float32_reference_meets_the_evaluation_limits(case):
    cid, form, d, ties = case
    z, z32 = R.ev_logits(d), R.ev_logits(d, np.float32)
    f, f32 = R.head_fwd(z, d['y'], form), R.head_fwd(z32, d['y'], form, np.float32)
    assert (np.abs(f32['c_err'] - f['c_err']) <= 0.5 * R.c_err_lim(f['c_err'])).all()
    assert np.abs(f32['x'] - f['x']).max() <= 0.5 * R.OUT_TOL * (1 + np.abs(f['x']).max())
    if ties:
        pz, py = R.TIES['tuned' if d['nc'] == R.TIE_CLS['tuned'] else 'gen'][0]
        assert (z[:, pz[0]] == z[:, pz[1]]).all() and (z.argmax(1) == pz[0]).all() and (d['y'].argmax(1) == py[0]).all()
    else:
        assert (f['gap_x'] > 1e-4).all() and (f['gap_y'] > 1e-4).all() and np.array_equal(f32['cls'], f['cls'])
    if 'sentinel' in cid:
        assert z.max() < -2 and z.min() > -9


# ------------------------------------------------------------------ the layer on the host
def _linked(n_in, y_shape=(10,)):
    from lib.layer_types import SquaredError, Sym
    ℓ = SquaredError()
    x = Sym(n_in if isinstance(n_in, tuple) else (n_in,))
    ℓ.link(x, Sym(y_shape), 'tr')
    return ℓ, x


def test_link_and_its_refusals():
    from lib.layer_types import Sym
    ℓ, x = _linked(10)
    assert ℓ.x is x and isinstance(ℓ.c_err, Sym) and isinstance(ℓ.δ_cor, Sym) and ℓ.c_err.producer is ℓ
    assert ℓ.n_ops == 0 and ℓ.c_mod == 0.0 and vars(ℓ.params) == {} and vars(ℓ.hypers) == {}
    for n_in, y_shape in [(9, (10,)), (11, (10,)), (10, (5, 2)), ((5, 2), (10,)), (10, (10, 1))]:
        with pytest.raises(ValueError, match='SquaredError'):
            _linked(n_in, y_shape)
    from lib.layer_types import ActivityError, Dropout
    for cls in (ActivityError, Dropout):                                   # (still outside)
        with pytest.raises(NotImplementedError):
            cls().link(Sym((10,)), Sym((10,)), 'tr')


def test_reg_and_exit_loss_build_the_chains(monkeypatch):
    import arch_and_hypers as A
    from lib import _hip
    from lib._eng_common import _kind, head_parts
    names = lambda ch: [type(c).__name__ for c in ch.comps]
    assert names(A.reg(10)) == ['Select', 'LinTrans', 'Softmax', 'CrossEntropyError']
    assert names(A.reg(10, loss='squared')) == ['Select', 'LinTrans', 'Softmax', 'SquaredError']
    assert names(A.reg(10, loss='squared-linear')) == ['Select', 'LinTrans', 'SquaredError']
    assert A.reg(7, loss='squared-linear').comps[1].hypers.n_chan == 7
    with pytest.raises(ValueError):
        A.reg(10, np.ones((10, 2), np.float32), 'squared')
    with pytest.raises(ValueError):
        A.reg(10, loss='brier')
    assert A.exit_loss is None
    kinds = lambda net: [head_parts(ℓ)[2] for ℓ in net.leaves]
    assert kinds(A.ac_chain()((32, 32, 3), (10,))) == [_hip.LOSS_CE] * 8
    monkeypatch.setattr(A, 'exit_loss', 'squared')
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))
    assert kinds(net) == [_hip.LOSS_SQ] * 8 and all(_kind(ℓ) == 'head' for ℓ in net.leaves)
    assert head_parts(next(iter(net.leaves)))[3] == 0.0 and head_parts(A.reg(10))[3] == 1e-6
    monkeypatch.setattr(A, 'exit_loss', {0: 'squared-linear', 2: 'squared', 99: 'squared'})
    monkeypatch.setattr(A, 'coarse_exits', {1: np.eye(10, 2, dtype=np.float32)})
    net = A.cr_chain()((32, 32, 3), (10,))
    assert kinds(net) == [_hip.LOSS_SQ_LIN, _hip.LOSS_CE, _hip.LOSS_SQ] + [_hip.LOSS_CE] * 5
    assert type(list(net.leaves)[1].comps[-1]).__name__ == 'SuperclassCrossEntropyError'
    assert net.leaf_n_cls == [10, 2] + [10] * 6
    assert len(set(kinds(A.ac_tree()((32, 32, 3), (10,))))) == 3
    assert kinds(A.sr_chain(3)((32, 32, 3), (10,))) == [_hip.LOSS_SQ]
    monkeypatch.setattr(A, 'exit_loss', {0: 'squared', 1: 'squared'})      # a block with both knobs: refused
    with pytest.raises(ValueError):
        A.ac_chain()((32, 32, 3), (10,))
    # the width must be the net's: a squared exit under a net with a two-dimensional label shape is refused at link
    monkeypatch.setattr(A, 'coarse_exits', None)
    with pytest.raises(ValueError, match='SquaredError'):
        A.sr_chain(2)((32, 32, 3), (5, 2))


def test_exit_loss_none_leaves_the_constructors_nets_as_they_are():
    import arch_and_hypers as A
    assert A.exit_loss is None
    for mk in (A.sr_chain(2), A.ac_chain(k_cpt=1.6e-8), A.cr_tree()):
        net = mk((32, 32, 3), (10,))
        assert all([type(c).__name__ for c in ℓ.comps] == ['Select', 'LinTrans', 'Softmax', 'CrossEntropyError'] for ℓ in net.leaves)


def test_exit_loss_argument():
    import arch_and_hypers as A
    assert A.parse_exit_loss('squared') == 'squared' and A.parse_exit_loss('squared-linear') == 'squared-linear'
    assert A.parse_exit_loss('squared:2') == {0: 'squared', 1: 'squared'}
    assert A.parse_exit_loss('squared-linear:3') == {i: 'squared-linear' for i in range(3)}
    assert A.parse_exit_loss('squared:0') == {}
    for bad in ('', 'brier', 'squared:', 'squared:x', 'squared:-1', 'linear:2', ':2'):
        with pytest.raises(ValueError, match='--exit-loss'):
            A.parse_exit_loss(bad)
    # train-nets refuses a bad value before it touches a device
    pkg = os.path.join(os.path.dirname(HERE), 'multipath-nn_amd')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--exit-loss', 'brier:2'],
                         capture_output=True)
    assert res.returncode == 2 and b'--exit-loss takes' in res.stderr


def test_checkpoint_record_round_trips_the_chains(monkeypatch):
    import io
    import arch_and_hypers as A
    from lib import serdes
    from lib.net_types import ActorNet
    monkeypatch.setattr(A, 'exit_loss', {0: 'squared', 1: 'squared-linear'})
    net = A.ac_chain(k_cpt=1.6e-8)((32, 32, 3), (10,))

    def strip(ℓ):
        """encode_layer without parameter values (they live on the device)."""
        if ℓ is None:
            return None
        return dict(type=type(ℓ).__name__, name=ℓ.name, hypers=dict(vars(ℓ.hypers)), params={}, router=strip(ℓ.router),
                    sinks=[strip(s) for s in ℓ.sinks], comps=[strip(c) for c in ℓ.comps])
    buf = io.BytesIO()
    np.save(buf, strip(net.root))
    buf.seek(0)
    monkeypatch.setattr(A, 'exit_loss', None)              # (the record alone says what the net is)
    back = ActorNet(x0_shape=(32, 32, 3), y_shape=(10,), root=serdes.decode_layer(np.load(buf, allow_pickle=True)[()]), k_cpt=1.6e-8)
    names = lambda n: [[type(c).__name__ for c in ℓ.comps] for ℓ in n.leaves]
    assert names(back) == names(net) and names(net)[1] == ['Select', 'LinTrans', 'SquaredError']


def test_single_scale_conv_nets_refuse_the_layer():
    from lib.layer_types import Chain, Conv, LinTrans, Rect, Softmax, SquaredError
    from lib.net_types import SRNet
    from lib._plan_conv import is_conv_net
    for comps in ([LinTrans(n_chan=10), Softmax(), SquaredError()], [LinTrans(n_chan=10), SquaredError()]):
        net = SRNet(x0_shape=(8, 8, 3), y_shape=(10,), root=Chain(comps=[Conv(n_chan=16, supp=3), Rect()], sinks=[Chain(comps=comps)]))
        with pytest.raises(NotImplementedError, match='single-scale Conv'):
            is_conv_net(net)


def test_loss_fields_match_the_c_layout():
    """`loss` is the last member of both records, as gcc sees the header.  mpnn_exit_tail_args: an entry of the ctypes
    mirror's _fields_.  mpnn_exit_ev_args: a property at the offset behind p_stride, in what was the record's tail padding --
    neither its size nor an older offset moved; a fresh record reads MPNN_LOSS_CE and copies carry the value."""
    import ctypes
    import re
    import tempfile
    from lib import _hip
    from lib._eng_common import copy_record
    root = os.path.dirname(HERE)
    recs = ('mpnn_exit_tail_args', 'mpnn_exit_ev_args')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mpnn_hip.h"', 'int main(void){']
    lines += ['printf("%%zu %%zu ", sizeof(%s), offsetof(%s, loss));' % (r, r) for r in recs]
    lines += ['printf("%zu %zu", offsetof(mpnn_exit_tail_args, bn_decay2), offsetof(mpnn_exit_ev_args, p_stride));', 'return 0;}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'a.c'), os.path.join(d, 'a.out')
        open(src, 'w').write('\n'.join(lines))
        subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), src, '-o', exe])
        tail_size, tail_loss, ev_size, ev_loss, tail_prev, ev_prev = (int(v) for v in subprocess.check_output([exe]).decode().split())
    T, E = _hip.ExitTailArgs, _hip.ExitEvArgs
    assert (tail_size, tail_loss) == (ctypes.sizeof(T), T.loss.offset) and T._fields_[-1][0] == 'loss'
    assert (ev_size, ev_loss) == (ctypes.sizeof(E), _hip.EXIT_EV_LOSS_OFFSET)
    # the last member of each: directly behind the member that used to be last, nothing behind it but padding
    assert tail_loss == tail_prev + 4 and tail_size - tail_loss <= 8 and ev_loss == ev_prev + 4 and ev_size - ev_loss == 4
    assert ev_loss > max(getattr(E, f).offset for f, _ in E._fields_)
    e = E()
    assert e.loss == 0 == _hip.LOSS_CE
    e.loss, e.p_stride = _hip.LOSS_SQ_LIN, 12345
    c = copy_record(e, n=7)
    assert (c.loss, c.p_stride, c.n, e.loss) == (2, 12345, 7, 2)
    raw = bytes(memoryview((E * 2)(e, c)))
    assert [int.from_bytes(raw[k * ev_size + ev_loss:k * ev_size + ev_loss + 4], sys.byteorder) for k in range(2)] == [2, 2]
    head = open(os.path.join(root, 'include', 'mpnn_hip.h')).read()
    defs = dict(re.findall(r'#define (MPNN_LOSS_\w+)\s+(\d+)', head))
    assert {k: int(v) for k, v in defs.items()} == {'MPNN_LOSS_CE': _hip.LOSS_CE, 'MPNN_LOSS_SQ': _hip.LOSS_SQ, 'MPNN_LOSS_SQ_LIN': _hip.LOSS_SQ_LIN}
