"""GPU: 8-bit images through Net.predict(decode=) and whole arrays through Net.predict_all.  Every comparison is exact:

  * predict(x_u8, decode=t) == predict(t[x_u8]) in cls, leaf, conf, ops and probs -- dense and routed, host and device
    input, a named table and a table of one's own; the table is uploaded only when it changes;
  * predict_all == the concatenation of predict over the same chunks -- uint8 with decode, float32 without, host and
    device input, four full chunks (eager, capture, replay, replay: graph replay and the reuse of a pinned slot) and a
    partial last one, one chunk, many tiny chunks, chunks below and above Engine.routed_min_batch;
  * its tensors stay as they are under later runs; eval -> predict_all -> eval gives the first eval's bits again;
  * a net on the general any-map conv kernels, a dyn_k_cpt net with one k_cpt per image, staging buffers that grow, and
    the classify-images driver on a uint8 file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lib.decode import decode_table
from test_routed_eval import batch, calibrate_exit_fractions, make, randomise_routers, snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('cls', 'leaf', 'ops', 'conf', 'probs')


def host(res):
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy().copy() for k in KEYS if getattr(res, k) is not None}


def same(a, b, what=''):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert np.array_equal(a[k].view(np.int32) if a[k].dtype == np.float32 else a[k], b[k].view(np.int32) if b[k].dtype == np.float32 else b[k]), (what, k)


def pixels(n, shape=(32, 32, 3), seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n,) + tuple(shape), dtype=np.uint8)


def per_chunk(net, xf, size, **kw):
    """The reference of predict_all: predict over the chunks of the decoded float images, concatenated on the host."""
    k_cpt = kw.pop('k_cpt', None)
    parts = []
    for i in range(0, len(xf), size):
        kc = k_cpt[i:i + size] if isinstance(k_cpt, np.ndarray) and k_cpt.size > 1 else k_cpt
        parts.append(host(net.predict(xf[i:i + size], k_cpt=kc, **kw)))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.fixture(scope='module')
def chain():
    """(net, x_u8, table, table[x_u8]): the tuned actor chain, 300 8-bit images, exits calibrated on the decoded images."""
    net = make('ac', k_cpt=1e-9)
    randomise_routers(net)
    xu = pixels(300, seed=3)
    table = decode_table('gamma')
    xf = table[xu]
    y = batch(300, seed=3)[1]
    calibrate_exit_fractions(net, xf, y, [1 / 8] * 7)
    taken = np.bincount(host(net.predict(xf))['leaf'], minlength=8)
    assert (taken > 0).sum() >= 4, taken
    return net, xu, table, xf


# ---------------------------------------------------------------------------------- predict(decode=)
@pytest.mark.parametrize('routed', [False, True])
@pytest.mark.parametrize('probs', [False, True])
def test_predict_decodes_on_the_device(chain, routed, probs):
    net, xu, table, xf = chain
    want = host(net.predict(xf, routed=routed, probs=probs))
    assert (want.get('probs') is not None) == probs
    for x in (xu, torch.from_numpy(xu), torch.from_numpy(xu).to('cuda:0')):
        net.engine().x0.fill_(float('nan'))                       # (nothing of the result comes from what x0 held)
        same(host(net.predict(x, routed=routed, probs=probs, decode='gamma')), want, type(x).__name__)
    same(host(net.predict(xf, routed=routed, probs=probs)), want)          # (the float path behind it is as it was)


def test_table_of_ones_own_and_upload_only_on_change(chain):
    net, xu, _, _ = chain
    eng = net.engine()
    mine = np.linspace(-0.3, 1.2, 256).astype(np.float32) ** 2
    net.predict(xu[:50], decode='gamma')
    u0 = eng.decode_uploads
    net.predict(xu[:50], decode='gamma')
    net.predict(xu[50:90], decode=decode_table('gamma').copy())
    assert eng.decode_uploads == u0                               # the same table, by name or by value: no upload
    got = host(net.predict(xu[:50], decode=mine, probs=True))
    assert eng.decode_uploads == u0 + 1
    same(got, host(net.predict(mine[xu[:50]], probs=True)))
    same(host(net.predict(xu[:50], decode=mine.astype(np.float64), probs=True)), got)
    assert eng.decode_uploads == u0 + 1
    same(host(net.predict(xu[:50], decode='unit')), host(net.predict(decode_table('unit')[xu[:50]])))
    assert eng.decode_uploads == u0 + 2
    with pytest.raises(ValueError, match='uint8'):
        net.predict(mine[xu[:50]], decode='gamma')
    with pytest.raises(ValueError, match='input'):
        net.predict(xu[:50, :16], decode='gamma')


def test_table_rewritten_in_place_is_uploaded_again(chain):
    """A caller's own float32 table is taken as it is (decode_table hands the same object back): rewriting it in place
    between two calls must change the result -- the engine compares a writable table by value, never by identity."""
    net, xu, _, _ = chain
    eng = net.engine()
    mine = np.linspace(0.0, 1.0, 256).astype(np.float32)
    assert decode_table(mine) is mine
    before = host(net.predict(xu[:40], decode=mine, probs=True))
    same(before, host(net.predict(mine[xu[:40]], probs=True)))
    u0 = eng.decode_uploads
    mine[:] = mine[::-1].copy()
    after = host(net.predict(xu[:40], decode=mine, probs=True))
    assert eng.decode_uploads == u0 + 1
    same(after, host(net.predict(mine[xu[:40]], probs=True)))
    assert not np.array_equal(after['probs'], before['probs'])
    same(host(net.predict_all(xu[:40], batch=16, decode=mine, probs=True)), per_chunk(net, mine[xu[:40]], 16, probs=True))
    mine[3] = 0.5                                                 # (one entry)
    same(host(net.predict_all(xu[:40], batch=16, decode=mine, probs=True)), per_chunk(net, mine[xu[:40]], 16, probs=True))
    assert eng.decode_uploads == u0 + 2
    net.predict(xu[:40], decode='gamma')                          # the named tables still go by identity, without an upload
    u1 = eng.decode_uploads
    net.predict(xu[:40], decode='gamma')
    assert eng.decode_uploads == u1


# ---------------------------------------------------------------------------------- predict_all
@pytest.fixture(scope='module')
def chunked(chain):
    """size -> per-chunk predict of the decoded images with probs (computed once per size, shared, left unchanged)."""
    net, _, _, xf = chain
    cache = {}

    def get(size):
        if size not in cache:
            cache[size] = per_chunk(net, xf, size, probs=True)
        return cache[size]
    return get


def test_predict_all_uint8_five_chunks(chain, chunked):
    net, xu, _, _ = chain
    res = net.predict_all(xu, batch=64, decode='gamma', probs=True)
    assert res.cls.dtype == torch.int32 and res.leaf.dtype == torch.int32 and res.ops.dtype == torch.int64
    assert res.conf.dtype == torch.float32 and res.probs.shape == (300, 10) and res.cls.is_cuda
    same(host(res), chunked(64))
    assert any(k[0] == 'pr+p' and k[1] == 64 and not isinstance(g, str) for k, g in net.engine()._graphs.items())
    no_probs = net.predict_all(xu, batch=64, decode='gamma')
    assert no_probs.probs is None
    want = {k: v for k, v in chunked(64).items() if k != 'probs'}
    same(host(no_probs), want)


def test_predict_all_float32(chain, chunked):
    net, _, _, xf = chain
    same(host(net.predict_all(xf, batch=64, probs=True)), chunked(64))
    ro = xf.copy()
    ro.setflags(write=False)                                      # (a read-only array, as a memory-mapped file gives)
    same(host(net.predict_all(ro, batch=64, probs=True)), chunked(64))
    same(host(net.predict_all(torch.from_numpy(xf), batch=64, probs=True)), chunked(64))


def test_predict_all_device_tensors(chain, chunked):
    net, xu, _, xf = chain
    same(host(net.predict_all(torch.from_numpy(xu).to('cuda:0'), batch=64, decode='gamma', probs=True)), chunked(64))
    same(host(net.predict_all(torch.from_numpy(xf).to('cuda:0'), batch=64, probs=True)), chunked(64))


@pytest.mark.parametrize('size', [300, 7])
def test_predict_all_one_chunk_and_tiny_chunks(chain, chunked, size):
    net, xu, _, xf = chain
    same(host(net.predict_all(xu, batch=size, decode='gamma', probs=True)), chunked(size))
    same(host(net.predict_all(xf, batch=size, probs=True)), chunked(size))
    if size == 300:                                               # (a batch beyond the array is one chunk as well)
        same(host(net.predict_all(xu, batch=4096, decode='gamma', probs=True)), chunked(size))


def test_predict_all_across_the_routed_threshold(chain, monkeypatch):
    """routed='auto' with the threshold at 50: the full chunks of 64 run the routed program, the tail of 44 the dense one;
    and the explicit forms."""
    net, xu, _, xf = chain
    eng = net.engine()
    monkeypatch.setattr(eng, 'routed_min_batch', 50)
    want = per_chunk(net, xf, 64, routed='auto')
    assert any(k[0] == 'pr' and k[1] == 64 and k[4] for k in eng._progs) and any(k[0] == 'pr' and k[1] == 44 and not k[4] for k in eng._progs)
    same(host(net.predict_all(xu, batch=64, decode='gamma')), want)
    same(host(net.predict_all(xf, batch=64)), want)
    for routed in (True, False, 2):
        same(host(net.predict_all(xu, batch=64, decode='gamma', routed=routed)), per_chunk(net, xf, 64, routed=routed))


def test_empty_input(chain):
    net = chain[0]
    launches = len(net.engine()._graphs), len(net.engine()._progs)
    for x, decode in ((np.zeros((0, 32, 32, 3), np.float32), None), (np.zeros((0, 32, 32, 3), np.uint8), 'gamma')):
        res = net.predict_all(x, probs=True, decode=decode)
        assert res.cls.shape == (0,) and res.cls.dtype == torch.int32 and res.leaf.dtype == torch.int32
        assert res.conf.dtype == torch.float32 and res.ops.dtype == torch.int64 and res.probs.shape == (0, 10)
    assert (len(net.engine()._graphs), len(net.engine()._progs)) == launches


def test_results_outlive_later_runs(chain, chunked):
    net, xu, _, xf = chain
    y = batch(300, seed=3)[1]
    net.eval({net.x0: xf, net.y: y})
    torch.cuda.synchronize()
    first = snapshot(net)
    res = net.predict_all(xu, batch=64, decode='gamma', probs=True)
    net.eval({net.x0: xf, net.y: y})
    torch.cuda.synchronize()
    again = snapshot(net)
    for grp in ('p_ev', 'c_err', 'd_cor', 'r', 'state'):          # eval -> predict_all -> eval: the first eval's bits
        assert first[grp].keys() == again[grp].keys()
        for k in first[grp]:
            assert np.array_equal(first[grp][k], again[grp][k]), (grp, k)
    other = pixels(64, seed=9)
    net.predict(other, decode='gamma', probs=True)
    net.predict(decode_table('gamma')[other][:33], probs=True)
    net.predict_all(other, batch=20, decode='unit', probs=True)
    same(host(res), chunked(64))


# ---------------------------------------------------------------------------------- other nets
def test_24x40_chain_on_the_general_kernels(monkeypatch):
    import arch_and_hypers as A
    from test_rect_nets import SHAPE, _batch, _net5
    monkeypatch.setattr(A, 'conv_supp', 5)
    net = _net5(A)
    assert net.engine().anymap_convs
    xu = pixels(48, SHAPE, seed=4)
    table = decode_table('gamma')
    xf = table[xu]
    randomise_routers(net)
    calibrate_exit_fractions(net, xf, _batch(SHAPE, 48, seed=3)[1], [1 / 8] * 7)
    want = per_chunk(net, xf, 20, probs=True)
    assert len(set(want['leaf'].tolist())) >= 4
    same(host(net.predict_all(xu, batch=20, decode='gamma', probs=True)), want)
    same(host(net.predict_all(xf, batch=20, probs=True)), want)
    same(host(net.predict_all(xu, batch=20, decode='gamma', probs=True, routed=True)), per_chunk(net, xf, 20, probs=True, routed=True))


def test_dyn_k_cpt_per_image():
    import arch_and_hypers as A
    net = A.ac_chain(dyn_k_cpt=True)((32, 32, 3), (10,))
    net.engine().init_params(3)
    randomise_routers(net, seed=4, scale=1.0)
    rng = np.random.default_rng(6)
    for ℓ in net.switches:                                        # (the k_cpt column of the routers' first map starts at zero)
        w = ℓ.router.comps[1].params.w
        v = w.numpy().copy()
        v[-1] = rng.standard_normal(v.shape[1]) * 3.0
        w.assign(v)
    from test_predict_nets import _calibrate_with_feed
    xu = pixels(40, seed=6)
    xf = decode_table('gamma')[xu]
    _calibrate_with_feed(net, {net.x0: xf, net.y: batch(40, seed=6)[1], net.k_cpt: np.full(40, 1e-9, np.float32)}, [1 / 8] * 7)
    kc = np.where(np.arange(40) % 2 == 1, 1e-9, 6.4e-8).astype(np.float32)        # (calibrated at the first value)
    want = per_chunk(net, xf, 16, probs=True, k_cpt=kc)
    same(host(net.predict_all(xu, batch=16, decode='gamma', probs=True, k_cpt=kc)), want)
    same(host(net.predict_all(xf, batch=16, probs=True, k_cpt=torch.from_numpy(kc))), want)
    one = per_chunk(net, xf, 16, k_cpt=6.4e-8)
    same(host(net.predict_all(xu, batch=16, decode='gamma', k_cpt=6.4e-8)), one)
    assert not np.array_equal(one['leaf'], want['leaf'])          # (the per-image values are really read)
    assert np.array_equal(one['leaf'][kc > 1e-8], want['leaf'][kc > 1e-8])
    with pytest.raises(ValueError, match='k_cpt'):
        net.predict_all(xu, batch=16, decode='gamma')
    with pytest.raises(ValueError, match='k_cpt'):
        net.predict_all(xu, batch=16, decode='gamma', k_cpt=kc[:16])


def test_staging_buffers_grow():
    net = make('ac', seed=11, k_cpt=1e-9)
    randomise_routers(net)
    eng = net.engine()
    xu = pixels(150, seed=8)
    xf = decode_table('gamma')[xu]
    same(host(net.predict(xu[:16], decode='gamma')), host(net.predict(xf[:16])))
    small = eng._stage_buffer(torch.uint8)
    assert small.shape == (eng.n_max, 32, 32, 3) and small.dtype == torch.uint8
    same(host(net.predict_all(xu, batch=64, decode='gamma')), per_chunk(net, xf, 64))
    n_big = eng.n_max + 22                                        # (beyond whatever capacity the engine was built with)
    xu3, xf3 = np.concatenate([xu] * 3)[:2 * n_big + 5], np.concatenate([xf] * 3)[:2 * n_big + 5]
    want = per_chunk(make_like(net), xf3, n_big)
    got = net.predict_all(xu3, batch=n_big, decode='gamma')
    assert eng.n_max == n_big and eng._stage_buffer(torch.uint8).shape[0] == n_big
    same(host(got), want)
    same(host(net.predict_all(xf3, batch=n_big)), want)
    assert eng._stage_buffer(torch.float32).shape[0] == n_big


def make_like(net):
    """A second net with the parameters of `net` (its engine is sized by its own runs)."""
    twin = make('ac', seed=11, k_cpt=1e-9)
    randomise_routers(twin)
    return twin


def test_conv_engine_refuses():
    from test_conv_layer import conv_net
    net = conv_net()((16, 16, 3), (10,))
    with pytest.raises(NotImplementedError, match='predict'):
        net.predict_all(np.zeros((4, 16, 16, 3), np.float32))


# ---------------------------------------------------------------------------------- the driver
def test_classify_images_decodes_a_uint8_file(tmp_path):
    out = str(tmp_path / 'nets')
    pkg = os.path.join(ROOT, 'multipath-nn_amd')
    res = subprocess.run([sys.executable, os.path.join(pkg, 'train-nets'), 'cifar10-ac', '--synthetic', '--iters', '8', '--nets', '0',
                          '--out', out], cwd=str(tmp_path), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    ckpt = os.path.join(out, 'cifar10-ac', '0000.npy')
    xu = pixels(100, seed=5)
    xf = decode_table('gamma')[xu]
    np.savez(str(tmp_path / 'u8.npz'), x=xu)
    np.savez(str(tmp_path / 'f32.npz'), x=xf)
    outs, texts = {}, {}
    for name, decode in (('u8', 'gamma'), ('f32', 'none')):
        pred = str(tmp_path / (name + '_pred.npz'))
        res = subprocess.run([sys.executable, os.path.join(pkg, 'classify-images'), ckpt, str(tmp_path / (name + '.npz')), '--out', pred,
                              '--batch', '64', '--probs', '--decode', decode], cwd=str(tmp_path), capture_output=True)
        assert res.returncode == 0, res.stderr.decode()[-2000:]
        outs[name] = dict(np.load(pred))
        texts[name] = res.stdout.decode().replace(name + '_pred.npz', 'PRED')
    same(outs['u8'], outs['f32'])
    assert texts['u8'] == texts['f32']
    from lib.serdes import read_net
    want = per_chunk(read_net(ckpt), xf, 64, routed='auto', probs=True)        # (what classify() gave before predict_all)
    assert set(outs['f32']) == set(KEYS)
    same({k: outs['f32'][k] for k in want}, want)
    hist = [int(v) for v in texts['f32'].split('exit histogram:')[1].splitlines()[0].split()]
    assert np.array_equal(np.bincount(want['leaf'], minlength=8), hist) and sum(hist) == 100
    assert 'mean operations per image: %.1f' % want['ops'].mean() in texts['f32']
    assert '100 images -> ' in texts['f32']
