"""CPU: oracle/ref_net.py against the reference's own graph code on RANDOMLY DRAWN nets and hyper-parameters
(tests/golden/fuzz_ref_graph.py; every key of ActorNet / CriticNet.default_hypers).  The reference side's results for draws
0 .. 119 are stored in tests/golden/fuzz_ref_graph_golden.npz (written by `fuzz_ref_graph.py --emit`); a longer hunt outside
that range (MPNN_FUZZ_DRAWS / MPNN_FUZZ_SEED0) runs the reference side as child processes and needs the reference tree."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import fuzz_ref_graph as Z
import make_ref_graph_golden as M

DRAWS = int(os.environ.get('MPNN_FUZZ_DRAWS', '120'))
SEED0 = int(os.environ.get('MPNN_FUZZ_SEED0', '0'))
WORKERS = 4


GOLDEN = os.path.join(HERE, 'golden', 'fuzz_ref_graph_golden.npz')


def reference_side(seed0, draws):
    """The reference graph code's results for draws seed0 .. seed0 + draws - 1: from the stored vectors where they cover
    the range, otherwise computed by child processes over the reference tree."""
    with np.load(GOLDEN) as z:
        gold = {k: z[k] for k in z.files}
    if all('%d/after' % s in gold for s in range(seed0, seed0 + draws)):
        return gold
    if not os.path.isdir(Z.REF):
        pytest.skip('draws %d .. %d are not in %s and the reference tree is absent' % (seed0, seed0 + draws - 1, GOLDEN))
    with tempfile.TemporaryDirectory() as d:
        per = -(-draws // WORKERS)
        procs = []
        for w in range(WORKERS):
            lo = seed0 + w * per
            cnt = min(per, seed0 + draws - lo)
            if cnt <= 0:
                continue
            env = dict(os.environ, OMP_NUM_THREADS='2', MKL_NUM_THREADS='2')
            path = os.path.join(d, 'w%d.npz' % w)
            procs.append((path, subprocess.Popen([sys.executable, os.path.join(HERE, 'golden', 'fuzz_ref_graph.py'), '--emit', path,
                                                  '--draws', str(cnt), '--seed0', str(lo)], env=env)))
        gold = {}
        for path, p in procs:
            assert p.wait() == 0
            with np.load(path) as z:
                gold.update({k: z[k] for k in z.files})
    return gold


def test_fuzzed_hypers_oracle_vs_reference_graph_code():
    import arch_and_hypers as A
    import lib.net_types as NT
    from oracle.ref_net import RefNet
    from test_ref_graph_golden import ordered
    gold = reference_side(SEED0, DRAWS)
    bad, seen = [], set()
    for seed in range(SEED0, SEED0 + DRAWS):
        case = Z.draw_case(seed)
        seen.add((case['kind'], case['shape'], case['hypers'].get('talr'), case['hypers'].get('α_rtr')))
        net = Z.build(A, NT, case)
        params = ordered(net)
        assert [n for n, _ in params] == list(gold['%d/names' % seed]), case
        rng = np.random.RandomState(seed)
        vals = {id(p): M.param_value(n, p.shape, rng) for n, p in params}
        ref = RefNet(net)
        ref.load_params(vals)
        x0, y, kc = Z.case_inputs(case)
        kw = {}
        if case['tau'] is not None:
            kw['τ'] = case['tau']
        if kc is not None:
            kw['k_cpt'] = kc
        if '%d/p_tr' % seed in gold:
            res = ref.forward(x0, y, 'tr', **kw)
            p_tr = np.stack([np.broadcast_to(res['out'][id(ℓ)]['p_tr'].detach().numpy(), (case['n'],)) for ℓ in net.layers])
            if np.abs(p_tr - gold['%d/p_tr' % seed]).max() > 1e-9:
                bad.append((seed, 'p_tr', case))
        ref.train_step(x0, y, case['lr'], **kw)
        after = np.array([M.digest(ref.V(p).detach().numpy()) for _, p in params])
        g = gold['%d/after' % seed]
        err = np.abs(after - g) / (1e-12 + np.abs(g).max(0, keepdims=True))
        if err.max() > 1e-9:
            bad.append((seed, [params[i][0] for i in np.argwhere(err > 1e-9)[:, 0][:4]], float(err.max()), case))
    assert not bad, '%d of %d draws disagree with the reference graph code: %r' % (len(bad), DRAWS, bad[:3])
    # the draws did cover the corner that rounds 1-4 got wrong: alpha_rtr != 1 without TALR, on both net types
    if DRAWS >= 50 and SEED0 == 0:
        assert any(k == 'ActorNet' and t is False and a != 1.0 for k, _, t, a in seen)
        assert any(k == 'CriticNet' and t is False and a != 1.0 for k, _, t, a in seen)
