"""CPU: the float64 reference of MultiscaleLLN (tests/lln_ref.py) and the host side of the layer.

  * known answer: a constant image c gives c / (c + ϵ) at every pixel -- borders and maps smaller than the filter included;
  * golden vectors: tests/golden/lln_ref_golden.npz, written by the reference's own MultiscaleLLN.link over the TensorFlow
    stand-in (tests/golden/lln_ref_graph.py --emit), reproduced to float64 rounding; RefNetLLN's torch lines agree too;
  * the GPU tests' tolerance can be met: an fp32 numpy model of the separable algorithm stays inside it on their inputs;
  * the signed inputs are well conditioned: min |m + ϵ| >= 0.25;
  * link behind ToPyramid (shapes, shifts, n_ops), the refusals, the checkpoint record, the default nets unchanged.
"""
import os

import numpy as np
import pytest

import lln_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'lln_ref_golden.npz')


@pytest.mark.parametrize('shape,S', [((4, 4), 1), ((8, 16), 4), ((24, 40), 4)])
@pytest.mark.parametrize('σ', [0.5, 3, 8])
def test_constant_image_known_answer(shape, S, σ):
    for c, ϵ in ((0.7, 1e-3), (-0.3, 1.0), (2.0, 0.5)):
        x = np.full((2,) + shape + (3,), c)
        want = c / (c * (0.2126 + 0.7152 + 0.0722) + ϵ)
        for o in R.lln(x, S, σ, ϵ):
            assert np.abs(o - want).max() <= 1e-14 * abs(want), (shape, σ, c)


def test_golden_vectors_of_the_reference_layer():
    import sys
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import lln_ref_graph as G
    assert os.path.getsize(GOLDEN) < 200 * 1024
    with np.load(GOLDEN) as gold:
        assert sorted(gold.files) == sorted('%s/%d' % (k, i) for k, c in G.CASES.items() for i in range(c['n_scales']))
        for key, case in G.CASES.items():
            x = G.case_input(case)
            hyp = {'σ': 3, 'ϵ': 1e-3, **case['hypers']}
            out = R.lln(x, case['n_scales'], hyp['σ'], hyp['ϵ'])
            for i, o in enumerate(out):
                g = gold['%s/%d' % (key, i)]
                assert o.shape == g.shape == (case['n'], case['shape'][0] >> i, case['shape'][1] >> i, 3)
                assert np.abs(o - g).max() <= 1e-13 * np.abs(g).max(), (key, i)


def _lln_net(A, monkeypatch, lln, ctor=None, shape=(32, 32, 3)):
    monkeypatch.setattr(A, 'lln', lln)
    return (ctor or A.sr_chain(2))(shape, (10,))


def test_refnet_lln_agrees_with_the_literal_lines(monkeypatch):
    import torch
    import arch_and_hypers as A
    net = _lln_net(A, monkeypatch, {'σ': 1.5, 'ϵ': 0.01}, shape=(24, 40, 3))
    ref = R.RefNetLLN(net)
    x = R.kernel_input((24, 40), False)[:2]
    out = {}
    xs = ref._link(net.root, torch.tensor(x, dtype=torch.float64), None, 'ev', out)
    want = R.lln(x, 4, 1.5, 0.01)
    assert len(xs) == 4
    for a, b in zip(xs, want):
        assert np.abs(a.numpy() - b).max() <= 1e-13 * np.abs(b).max()
    assert out[id(net.root)]['n_ops'] == 0


@pytest.mark.parametrize('shape,S,σ,eps,signed', R.kernel_cases())
def test_fp32_model_meets_the_gpu_tolerance(shape, S, σ, eps, signed):
    x = R.kernel_input(shape, signed)
    ref, bnd = R.bound(x, S, σ, eps, signed)
    got = R.model_fp32(x, S, σ, eps)
    worst = max(float((np.abs(g - r) / b).max()) for g, r, b in zip(got, ref, bnd))
    assert worst <= 1.0, worst


@pytest.mark.parametrize('shape,S', R.SHAPES)
@pytest.mark.parametrize('σ', R.SIGMAS)
def test_signed_inputs_are_well_conditioned(shape, S, σ):
    x = R.kernel_input(shape, True).astype(np.float64)
    for x_i in R.pyramid(x, S):
        assert np.abs(R.local_mean(x_i, σ) + 1.0).min() >= 0.25


# ------------------------------------------------------------------ the layer on the host
def test_link_behind_topyramid():
    from lib.layer_types import MultiscaleLLN, Sym, ToPyramid
    pyr = ToPyramid(n_scales=4)
    pyr.link(Sym((24, 40, 3)), None, None)
    ℓ = MultiscaleLLN()
    ℓ.link(pyr.x, None, 'tr')
    assert [s.shape for s in ℓ.x] == [(24, 40, 3), (12, 20, 3), (6, 10, 3), (3, 5, 3)]
    assert [s.shift for s in ℓ.x] == [0] * 4 and ℓ.in_shifts == [0, 1, 2, 3]
    assert all(s.producer is ℓ for s in ℓ.x)
    assert ℓ.n_ops == 0 and ℓ.c_err == 0.0 and ℓ.c_mod == 0.0 and vars(ℓ.params) == {}
    assert ℓ.radius == 6 and len(ℓ.taps()) == 13 and ℓ.taps()[6] == 1.0
    assert np.array_equal(ℓ.taps(), R.taps(3))
    ℓ = MultiscaleLLN(σ=8, shape0=(32, 32))          # (shape0: accepted and unused, as in the reference)
    ℓ.link(pyr.x, None, 'tr')
    assert ℓ.radius == 16


def test_refusals():
    from lib.layer_types import MultiscaleLLN, MultiscaleRect, Sym, ToPyramid
    pyr = ToPyramid(n_scales=2)
    pyr.link(Sym((8, 8, 3)), None, None)
    with pytest.raises(NotImplementedError):
        MultiscaleLLN().link([Sym((4, 4, 3))], None, 'tr')                    # a bare Sym
    rect = MultiscaleRect()
    rect.link(pyr.x, None, None)
    with pytest.raises(NotImplementedError):
        MultiscaleLLN().link(rect.x, None, 'tr')                              # behind another layer
    with pytest.raises(NotImplementedError):
        MultiscaleLLN().link(pyr.x[0], None, 'tr')                            # not a pyramid
    for c in (1, 4):
        p = ToPyramid(n_scales=2)
        p.link(Sym((8, 8, c)), None, None)
        with pytest.raises(ValueError):
            MultiscaleLLN().link(p.x, None, 'tr')
    for σ in (0, -1.0, 8.01, 100):
        with pytest.raises(NotImplementedError, match='16'):
            MultiscaleLLN(σ=σ).link(pyr.x, None, 'tr')


def test_kind_of_the_root_chain(monkeypatch):
    import arch_and_hypers as A
    from lib._eng_common import _kind
    assert _kind(_lln_net(A, monkeypatch, {}).root) == 'pyramid'
    assert _kind(_lln_net(A, monkeypatch, None).root) == 'pyramid'


def test_default_nets_are_unchanged_and_the_switch_is_read_at_call_time(monkeypatch):
    import arch_and_hypers as A
    assert A.lln is None
    make = A.ac_chain(k_cpt=1.6e-8)
    assert [type(c).__name__ for c in make((32, 32, 3), (10,)).root.comps] == ['ToPyramid']
    monkeypatch.setattr(A, 'lln', {'σ': 1.5})
    net = make((32, 32, 3), (10,))
    assert [type(c).__name__ for c in net.root.comps] == ['ToPyramid', 'MultiscaleLLN']
    assert net.root.comps[1].hypers.σ == 1.5 and net.root.comps[1].hypers.ϵ == 1e-3
    plain = A.ac_chain(k_cpt=1.6e-8)
    monkeypatch.setattr(A, 'lln', None)
    a, b = plain((32, 32, 3), (10,)), net
    assert [(p.name, p.shape) for p in a._all_params] == [(p.name, p.shape) for p in b._all_params]
    assert [ℓ.n_ops for ℓ in a.layers] == [ℓ.n_ops for ℓ in b.layers]


def test_checkpoint_record_round_trips_the_layer(monkeypatch):
    """encode_layer / decode_layer (lib/serdes.py; encode_net / decode_net wrap them around an engine, which needs a GPU:
    tests/test_lln_nets.py): the layer's type and hypers travel, and the rebuilt tree links."""
    import arch_and_hypers as A
    from lib import serdes
    from lib.layer_types import _Linker
    from lib.net_types import SRNet
    net = _lln_net(A, monkeypatch, {'σ': 1.5, 'ϵ': 0.25})
    rec = dict(type=type(net.root).__name__, name=net.root.name, hypers={}, params={}, sinks=[], router=None,
               comps=[serdes.encode_layer(c) for c in net.root.comps])
    root = serdes.decode_layer(rec)
    assert [type(c).__name__ for c in root.comps] == ['ToPyramid', 'MultiscaleLLN']
    assert vars(root.comps[1].hypers) == vars(net.root.comps[1].hypers)
    back = SRNet(x0_shape=(32, 32, 3), y_shape=(10,), root=root)
    assert [s.shape for s in back.root.x] == [s.shape for s in net.root.x] and back.root.comps[1].radius == 3
