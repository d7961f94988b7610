"""GPU: routed evaluation of nets on the general conv kernels (csrc/conv_gen.hip) -- their blocks below the gather depth
run their convs on the sample lists the routers wrote (mpnn_conv_fwd_args.idx / cnt of mpnn_msconv_fwd_gen / _hw), like
the nets on the tuned kernels.

The nets: the conv_supp = 5 actor chain on 32x32 images, the critic chain with conv_supp = 1, the conv_supp = 5 actor
chain on 24x40 images (the any-map entry points), the stock 3x3 actor chain and the actor tree under MPNN_GENERIC_CONVS=1.
After two training steps (moving averages away from their initial values):

  * routed == dense exactly (tests/test_routed_eval.py: check_routed_equals_dense) with routed = True, 1 and 3;
  * with one eighth of the batch leaving at each exit, at 64 and at 1 000 samples, every block below the root carries a
    conv list under routed = 1 and its count lies strictly between 0 and n;
  * THE WORK IS SKIPPED: at initialisation every sample leaves at exit 0, and the NaN-poisoned maps of the blocks below
    the root are still NaN after net.eval(feed, routed=1); in the one-eighth state the rows of a block's maps are finite
    for the samples that reach it and still poisoned for those that left earlier;
  * the captured routed program, replayed on a batch that is routed differently, equals the dense pass again;
  * the conv_supp = 5 chain against the float64 oracle (TF SAME padding, as tests/test_conv_gen_nets.py sets it up)."""
import numpy as np
import pytest
import torch

from test_conv_gen_nets import _tf_same
from test_net_parity import perturb_routers
from test_routed_eval import calibrate_exit_fractions, check_routed_equals_dense, check_vs_oracle, randomise_routers, snapshot

pytestmark = pytest.mark.gpu

# name: (constructor, image, conv_supp, MPNN_GENERIC_CONVS=1)
NETS = {
    'ac-supp5': ('ac_chain', (32, 32, 3), 5, False),
    'cr-supp1': ('cr_chain', (32, 32, 3), 1, False),
    'ac-supp5-24x40': ('ac_chain', (24, 40, 3), 5, False),
    'ac-3x3-forced': ('ac_chain', (32, 32, 3), 3, True),
    'tree-3x3-forced': ('ac_tree', (32, 32, 3), 3, True),
}
CHAINS = [k for k in NETS if 'tree' not in k]


def _batch(shape, n, seed=0):
    rng = np.random.default_rng(seed)
    x0 = rng.random((n,) + tuple(shape)).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]
    return x0, y


@pytest.fixture
def build(monkeypatch):
    """build(name, trained=True) -> (net, image shape): the net on the general kernels, routers perturbed and two training
    steps done (trained) or as initialised (every sample leaves at exit 0)."""
    def make(name, trained=True):
        import arch_and_hypers as A
        from oracle import ref_net
        ctor, shape, supp, forced = NETS[name]
        monkeypatch.setattr(A, 'conv_supp', supp)
        monkeypatch.setattr(ref_net, 'conv_same', _tf_same)
        if forced:
            monkeypatch.setenv('MPNN_GENERIC_CONVS', '1')
        net = getattr(A, ctor)(k_cpt=1e-9, seed=7)(shape, (10,))
        eng = net.engine()
        assert eng.generic_convs and eng.anymap_convs == (shape[:2] != (32, 32))
        eng.init_params(1234)
        if trained:
            perturb_routers(net)
            x0, y = _batch(shape, 64, seed=3)
            for t in range(2):
                net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0})
        return net, shape
    return make


def _eval_routed_1(net, x0, y):
    """net.eval(routed=1) with its program built anew: the blocks' ev_list / ev_conv_list are those of the program built last."""
    eng = net.engine()
    eng._progs.clear(); eng._graphs.clear()
    net.eval({net.x0: x0, net.y: y}, routed=1)
    torch.cuda.synchronize()


def _below_root(eng):
    return [b for b in eng.blocks if b.parent is not None]


@pytest.mark.parametrize('name', list(NETS))
def test_routed_equals_dense(build, name):
    net, shape = build(name)
    eng = net.engine()
    x0, y = _batch(shape, 64, seed=3)
    if name not in CHAINS:                   # (the chains' spread over the exits is set by the one-eighth tests below)
        randomise_routers(net, seed=3, scale=1.0)
    dense = check_routed_equals_dense(net, x0, y, modes=(True, 1, 3))
    if name not in CHAINS:
        hist = np.stack([dense['p_ev'][nd.idx] for nd in eng.leaves]).mean(1)
        assert (hist > 0).sum() >= 2, hist
    _eval_routed_1(net, x0, y)
    with_list = [b.ev_conv_list is not None for b in _below_root(eng)]      # (a tree: the blocks below a static root share its "every sample")
    assert all(with_list) if name in CHAINS else sum(with_list) >= len(with_list) // 2
    assert {op.what for op in eng.program('ev', 64, routed=1)['fwd']} == {'fwd', 'exit_ev', 'route'}


@pytest.mark.parametrize('n', [64, 1000])
@pytest.mark.parametrize('name', CHAINS)
def test_one_eighth_per_exit_every_block_below_the_root_runs_on_its_list(build, name, n):
    net, shape = build(name)
    eng = net.engine()
    x0, y = _batch(shape, n, seed=5)
    calibrate_exit_fractions(net, x0, y, [1 / 8] * 7)
    dense = check_routed_equals_dense(net, x0, y, modes=(True, 1, 3))
    hist = np.stack([dense['p_ev'][nd.idx] for nd in eng.leaves]).mean(1)
    assert np.allclose(hist, 1 / 8, atol=0.5 / n), hist
    _eval_routed_1(net, x0, y)
    counts = []
    for b in _below_root(eng):
        assert b.ev_conv_list is not None and b.ev_conv_list is b.ev_list
        counts.append(int(b.ev_conv_list[1].cpu()[0]))
        assert 0 < counts[-1] < n, counts
    assert counts == sorted(counts, reverse=True) and len(set(counts)) == len(counts), counts      # (a chain: fewer at every depth)


@pytest.mark.parametrize('name', CHAINS)
def test_at_initialisation_no_block_below_the_root_runs(build, name):
    """The last router map starts at zero: every sample leaves at exit 0, and nothing below the root may run."""
    net, shape = build(name, trained=False)
    eng = net.engine()
    x0, y = _batch(shape, 64)
    eng._ensure_capacity(64)
    for b in eng.blocks[1:]:
        for t in b.s:
            t.fill_(float('nan'))
    net.eval({net.x0: x0, net.y: y}, routed=1)
    torch.cuda.synchronize()
    assert [float(nd.layer.p_ev.mean()) for nd in eng.leaves] == [1.0] + [0.0] * 7
    for b in eng.blocks[1:]:                 # not executed: the poison is still there
        for t in b.s:
            assert torch.isnan(t[:64]).all()
    assert torch.isfinite(eng.blocks[0].s[-1][:64]).all()


@pytest.mark.parametrize('name', CHAINS)
def test_a_block_runs_on_the_samples_that_reach_it_and_on_no_other(build, name):
    net, shape = build(name)
    eng = net.engine()
    n = 64
    x0, y = _batch(shape, n, seed=5)
    calibrate_exit_fractions(net, x0, y, [1 / 8] * 7)
    net.eval({net.x0: x0, net.y: y})
    torch.cuda.synchronize()
    dense = snapshot(net)
    for b in eng.blocks[1:]:
        for t in b.s:
            t.fill_(float('nan'))
    net.eval({net.x0: x0, net.y: y}, routed=1)
    torch.cuda.synchronize()
    for k, b in enumerate(eng.blocks[1:], 1):
        reach = torch.from_numpy(dense['p_ev'][b.node.idx] > 0).to(b.s[0].device)
        assert int(reach.sum()) == n - k * n // 8
        for t in b.s:
            assert torch.isfinite(t[:n][reach]).all(), 'block %d: a sample that reaches it has no result' % k
            assert torch.isnan(t[:n][~reach]).all(), 'block %d ran on a sample that left earlier' % k


@pytest.mark.parametrize('name', ['ac-supp5', 'ac-supp5-24x40'])
def test_the_captured_routed_program_replays_on_a_batch_routed_differently(build, name):
    net, shape = build(name)
    eng = net.engine()
    eng.use_graph = True
    feeds = [_batch(shape, 96, seed=s) for s in (11, 12, 13)]
    randomise_routers(net, seed=3, scale=1.0)
    calibrate_exit_fractions(net, *feeds[0], [1 / 8] * 7)      # (the first batch spreads over the eight exits; the others as they fall)
    seen = []
    for rep in range(2):
        for x0, y in feeds:                  # (first call: eager; second: captured; from the third on: replayed)
            dense = check_routed_equals_dense(net, x0, y, modes=(1,))
            seen.append(np.stack([dense['p_ev'][nd.idx] for nd in eng.leaves]))
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert any(k[0] == 'ev' and k[3] == 1 and not isinstance(g, str) for k, g in eng._graphs.items())


def test_supp5_chain_against_the_oracle(build):
    net, shape = build('ac-supp5')
    x0, y = _batch(shape, 64, seed=3)
    calibrate_exit_fractions(net, x0, y, [1 / 8] * 7)
    dense = check_routed_equals_dense(net, x0, y, modes=(True, 1, 3))
    hist = check_vs_oracle(net, x0, y, dense)
    assert np.allclose(hist, 1 / 8), hist
