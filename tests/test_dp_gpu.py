"""GPU, world_size 2 on ONE device over gloo: the whole data-parallel training step through the real
engine (attach/broadcast, forward+backward graph, all-reduce of G with its TALR tail, optimizer graph
with 1/world scaling) against a single-process emulation that adds the other rank's gradients by hand.
RCCL refuses two ranks on one GPU, so the collective backend here is gloo; everything else is the code
path the multi-GPU bench runs."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64


def _batch(rank):
    g = np.random.default_rng(100 + rank)
    return g.random((N, 32, 32, 3)).astype(np.float32), np.eye(10, dtype=np.float32)[g.integers(0, 10, N)]


def _net(buckets=3):
    """(the bucketed form -- exits | deep blocks | rest -- unless asked otherwise: it exercises every piece of the
    data-parallel machinery; the shipped default is ONE bucket, test_default_is_one_bucket)"""
    for p in (ROOT, os.path.join(ROOT, 'multipath-nn_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import arch_and_hypers as A
    old = os.environ.get('MPNN_DP_BUCKETS')
    os.environ['MPNN_DP_BUCKETS'] = str(buckets)
    try:
        net = A.ac_chain(k_cpt=1.6e-8, seed=21)((32, 32, 3), (10,))
        net.engine()
    finally:
        if old is None:
            os.environ.pop('MPNN_DP_BUCKETS')
        else:
            os.environ['MPNN_DP_BUCKETS'] = old
    return net


def _feed(net, x0, y):
    return {net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0}


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    net = _net()
    from lib import _dp
    _dp.init('gloo')
    torch.cuda.set_device(0)
    _dp.attach(net)
    eng = net.engine()
    inner = eng.allreduce

    def via_host(flat):                      # gloo builds without device support: stage through the host
        try:
            return inner(flat)
        except RuntimeError:
            h = flat.cpu(); dist.all_reduce(h); flat.copy_(h); return flat
    eng.allreduce = via_host
    x0, y = _batch(rank)
    for _ in range(3):                       # eager step, graph capture, graph replay
        net.train.run(_feed(net, x0, y))
    torch.cuda.synchronize()
    np.save(os.path.join(out, 'P%d.npy' % rank), eng.P.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_two_ranks_match_hand_summed_gradients(tmp_path):
    world, port = 2, _free_port()
    # (results come back through files: a multiprocessing.Manager forked from a process that holds a HIP context was
    # seen to drop its connections in the middle of a long pytest run)
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    p0, p1 = (np.load(str(tmp_path / ('P%d.npy' % r))) for r in range(2))
    assert np.array_equal(p0, p1), 'replicas diverged'

    # single-process emulation of rank 0: the "collective" adds rank 1's gradients, which are
    # computed from the same parameters by a second engine stepping in lock-step
    net_a, net_b = _net(), _net()
    ea, eb = net_a.engine(), net_b.engine()
    ea.use_graph = eb.use_graph = False
    xa, ya = _batch(0)
    xb, yb = _batch(1)
    ea.world = eb.world = 2
    ea.dp_bucket_opt = False       # a: forward + backward only (its update is applied below, from b's reduced G); b applies each
    box = {}                       # bucket behind its "collective", the shipped form
    # the engine hands the collective one gradient BUCKET at a time (a view into G): b's "collective"
    # adds a's gradients of the same range
    def add_a(view):
        lo = (view.data_ptr() - eb.G.data_ptr()) // 4
        return view.add_(box['ga'][lo:lo + view.numel()])
    eb.allreduce = add_a
    ea.allreduce = lambda view: view
    assert list(eb.dp_buckets) == ['exit', 'mid', 'end']
    for _ in range(3):
        # rank a: forward+backward only; finish its step after b's G is known
        prog = ea.program('tr', N)
        assert [op.tag for op in prog['bwd'] if op.what == 'bucket'] == ['exit', 'mid', 'end']
        ea._stage(_feed(net_a, xa, ya)); ea._phase_a(prog, True); box['ga'] = ea.G.clone()
        net_b.train.run(_feed(net_b, xb, yb))          # b: G_b + G_a bucket by bucket, optimizer with 1/world
        ea.G.copy_(eb.G); ea._opt(N)
    torch.cuda.synchronize()
    pa, pb = ea.P.cpu().numpy(), eb.P.cpu().numpy()
    scale = np.abs(pa).max()
    assert np.abs(pa - pb).max() <= 1e-6 * scale
    # (three steps of a net that amplifies fp32 summation-order differences: 3e-5 observed)
    assert np.abs(p0 - pa).max() <= 3e-4 * scale, np.abs(p0 - pa).max()


def _conv_batch(rank, n=12):
    g = np.random.default_rng(300 + rank)
    return g.random((n, 16, 16, 3)).astype(np.float32), np.eye(10, dtype=np.float32)[g.integers(0, 10, n)]


def _conv_worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    for p in (ROOT, os.path.join(ROOT, 'multipath-nn_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    from test_conv_layer import conv_net
    from lib import _dp
    net = conv_net(res=True)((16, 16, 3), (10,))
    net.engine().init_params(4 + rank)               # (different on purpose: attach broadcasts rank 0's)
    _dp.init('gloo')
    torch.cuda.set_device(0)
    _dp.attach(net)
    x0, y = _conv_batch(rank)
    for t in range(3):
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.μ_lrn: 0.9})
    torch.cuda.synchronize()
    np.save(os.path.join(out, 'C%d.npy' % rank), net.engine().P.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_single_scale_conv_engine_is_data_parallel(tmp_path):
    """_dp.attach on the single-scale Conv engine (lib/_plan_conv.py; round 4 refused it): two ranks x 12 images take
    the steps one process takes on the 24 images (no BatchNorm in these nets: the global-batch step exactly, up to
    fp32 summation order), replicas bit-identical."""
    world, port = 2, _free_port()
    mp.spawn(_conv_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    p0, p1 = (np.load(str(tmp_path / ('C%d.npy' % r))) for r in range(2))
    assert np.array_equal(p0, p1), 'replicas diverged'
    for p in (os.path.join(ROOT, 'tests'),):
        if p not in sys.path:
            sys.path.insert(0, p)
    from test_conv_layer import conv_net
    net = conv_net(res=True)((16, 16, 3), (10,))
    net.engine().init_params(4)
    (xa, ya), (xb, yb) = _conv_batch(0), _conv_batch(1)
    x0, y = np.concatenate([xa, xb]), np.concatenate([ya, yb])
    for t in range(3):
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05, net.μ_lrn: 0.9})
    torch.cuda.synchronize()
    want = net.engine().P.cpu().numpy()
    assert np.abs(p0 - want).max() <= 2e-5 * np.abs(want).max(), np.abs(p0 - want).max()


def _rccl_one_rank(_idx, port, out, one_graph='1'):
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      MPNN_DP_ONE_GRAPH=one_graph)
    net = _net()
    from lib import _dp
    assert _dp.init('nccl', force=True) == (0, 1)
    _dp.attach(net, force=True)
    eng = net.engine()
    assert eng.allreduce is _dp.allreduce_async
    x0, y = _batch(0)
    for _ in range(4):                       # eager, capture (one graph per bucket section), two replays
        net.train.run(_feed(net, x0, y))
    _dp.sync_state(net)
    torch.cuda.synchronize()
    res = {'selftest': _dp.captured_collectives_work()}    # (what a run with more than one rank checks before it captures)
    key = [k for k in eng._graphs if k[0] == 'tr'][0]
    secs, gb = eng._graphs[key]
    res['sections'] = [b for _, b in secs]
    res['whole'] = gb == 'whole'
    res['buckets'] = list(eng.dp_buckets)
    np.save(os.path.join(out, 'P.npy'), eng.P.cpu().numpy())
    import json
    json.dump(res, open(os.path.join(out, 'res.json'), 'w'))
    dist.destroy_process_group()


def _run_rccl_one_rank(tmp_path, one_graph='1'):
    import json
    mp.spawn(_rccl_one_rank, args=(_free_port(), str(tmp_path), one_graph), nprocs=1, join=True)
    out = json.load(open(str(tmp_path / 'res.json')))
    out['P'] = np.load(str(tmp_path / 'P.npy'))
    return out


def test_rccl_path_on_one_gpu_matches_single_process(tmp_path):
    """The real collective backend (nccl = RCCL) with ONE rank: process-group init, asynchronous
    bucket all-reduces issued between the section graphs, stream-level waits, optimizer graph.  A
    one-rank sum is the identity, so the parameters must equal a plain single-process run."""
    out = _run_rccl_one_rank(tmp_path)
    # RCCL collectives capture: the whole step (bucket sections, async all-reduces, waits, optimizer) is ONE hipGraph
    assert out['buckets'] == ['exit', 'mid', 'end']
    assert out['whole'] and out['sections'] == [None]
    assert out['selftest'] is True
    net = _net()
    x0, y = _batch(0)
    for _ in range(4):
        net.train.run(_feed(net, x0, y))
    torch.cuda.synchronize()
    ref = net.engine().P.cpu().numpy()
    # (four steps of a net that amplifies fp32 summation-order differences -- the exit path's atomics
    # reorder between two processes; 1.6e-5 observed, as in the two-rank test below)
    assert np.abs(out['P'] - ref).max() <= 3e-4 * np.abs(ref).max()


def test_rccl_section_graphs_on_one_gpu(tmp_path):
    """The fallback form (MPNN_DP_ONE_GRAPH=0, or a stack whose collectives do not capture): one graph per bucket
    section, the all-reduces issued from the host between the replays, a graph for the optimizer."""
    out = _run_rccl_one_rank(tmp_path, '0')
    assert not out['whole'] and out['sections'] == ['exit', 'mid', 'end']
    net = _net()
    x0, y = _batch(0)
    for _ in range(4):
        net.train.run(_feed(net, x0, y))
    torch.cuda.synchronize()
    ref = net.engine().P.cpu().numpy()
    assert np.abs(out['P'] - ref).max() <= 3e-4 * np.abs(ref).max()


def _rccl_one_rank_k(_idx, port, out):
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    net = _net()
    from lib import _dp
    assert _dp.init('nccl', force=True) == (0, 1)
    _dp.attach(net, force=True)
    eng = net.engine()
    x0, y = _batch(0)
    eng._ensure_capacity(N)
    eng.x0[:N].copy_(torch.from_numpy(x0)); eng.y[:N].copy_(torch.from_numpy(y))
    feed = lambda t: {net.x0: eng.x0[:N], net.y: eng.y[:N], net.mode: 'tr', net.λ_lrn: 0.05 / (1 + t), net.τ: 1.0 - 0.05 * t}
    for rnd in range(3):                     # step by step (warm-up), capture + replay, replay
        net.train.run_steps([feed(4 * rnd + j) for j in range(4)])
    torch.cuda.synchronize()
    keys = [k for k in eng._graphs if k[0] == 'trK']
    res = {'captured': bool(keys) and not isinstance(eng._graphs[keys[0]], str), 'dp_key': bool(keys) and bool(keys[0][-1]),
           'buckets': list(eng.dp_buckets)}
    np.save(os.path.join(out, 'P.npy'), eng.P.cpu().numpy())
    import json
    json.dump(res, open(os.path.join(out, 'res.json'), 'w'))
    dist.destroy_process_group()


def test_k_step_graph_under_data_parallelism_rccl_one_rank(tmp_path):
    """Engine.run_steps with an all-reduce attached: K steps -- with their K x 3 captured RCCL all-reduces on the process
    group's stream and the optimizer behind each step's last one -- are ONE hipGraph (the step form of the single-process
    headline; round 5 ran one graph per step under data parallelism).  One rank: the sum is the identity, so twelve steps
    must equal twelve single-process steps with the same per-step schedule values."""
    import json
    mp.spawn(_rccl_one_rank_k, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    res = json.load(open(str(tmp_path / 'res.json')))
    assert res['captured'] and res['dp_key'] and res['buckets'] == ['exit', 'mid', 'end']
    net = _net()
    eng = net.engine()
    x0, y = _batch(0)
    for t in range(12):
        net.train.run({net.x0: x0, net.y: y, net.mode: 'tr', net.λ_lrn: 0.05 / (1 + t), net.τ: 1.0 - 0.05 * t})
    torch.cuda.synchronize()
    ref = eng.P.cpu().numpy()
    got = np.load(str(tmp_path / 'P.npy'))
    assert np.abs(got - ref).max() <= 3e-4 * np.abs(ref).max()


def _worker_k(rank, world, port, out):
    """As _worker, but the last two of the three steps through run_steps: over gloo the collectives do not capture, so the
    K-step call must fall back to one step per replay -- and still be the same three steps."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    net = _net()
    from lib import _dp
    _dp.init('gloo')
    torch.cuda.set_device(0)
    _dp.attach(net)
    eng = net.engine()
    inner = eng.allreduce

    def via_host(flat):
        try:
            return inner(flat)
        except RuntimeError:
            h = flat.cpu(); dist.all_reduce(h); flat.copy_(h); return flat
    eng.allreduce = via_host
    x0, y = _batch(rank)
    eng._ensure_capacity(N)
    eng.x0[:N].copy_(torch.from_numpy(x0)); eng.y[:N].copy_(torch.from_numpy(y))
    feed = {net.x0: eng.x0[:N], net.y: eng.y[:N], net.mode: 'tr', net.λ_lrn: 0.05, net.τ: 1.0}
    net.train.run(feed)
    net.train.run_steps([feed, feed])
    torch.cuda.synchronize()
    assert not any(k[0] == 'trK' and not isinstance(v, str) for k, v in eng._graphs.items())     # (nothing to capture over gloo)
    np.save(os.path.join(out, 'P%d.npy' % rank), eng.P.cpu().numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_run_steps_falls_back_over_gloo(tmp_path):
    mp.spawn(_worker_k, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    p0, p1 = np.load(str(tmp_path / 'P0.npy')), np.load(str(tmp_path / 'P1.npy'))
    assert np.array_equal(p0, p1), 'replicas diverged'
    ref_dir = tmp_path / 'ref'
    ref_dir.mkdir()
    mp.spawn(_worker, args=(2, _free_port(), str(ref_dir)), nprocs=2, join=True)
    want = np.load(str(ref_dir / 'P0.npy'))
    assert np.abs(p0 - want).max() <= 3e-5 * np.abs(want).max()


def test_default_is_one_bucket():
    """The shipped form: the whole of G (TALR statistics at its head) in ONE all-reduce after the backward pass."""
    for p in (ROOT, os.path.join(ROOT, 'multipath-nn_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import arch_and_hypers as A
    assert 'MPNN_DP_BUCKETS' not in os.environ
    net = A.ac_chain(k_cpt=1.6e-8, seed=21)((32, 32, 3), (10,))
    eng = net.engine()
    assert list(eng.dp_buckets) == ['end'] and eng.dp_buckets['end'] == (0, eng.G.numel())
    assert eng.node_stat.data_ptr() == eng.G.data_ptr() and eng.dp_reserve_cus == 0 and not eng._bucket_opt_on()
    P, res = _standin_run(0, False, net=net)
    ref = _net()
    x0, y = _batch(0)
    for _ in range(4):
        ref.train.run(_feed(ref, x0, y))
    torch.cuda.synchronize()
    r = ref.engine().P.cpu().numpy()
    assert np.abs(P - r).max() <= 3e-4 * np.abs(r).max()


def _standin_run(reserve, bucket_opt, k=8, T=10.0, steps=4, net=None):
    """The one-graph data-parallel step with the collective replaced by the co-runner stand-in of
    tools/dp_corunner_probe.py (k spinning workgroups on a side stream at every bucket point)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import dp_corunner_probe as probe
    net = _net() if net is None else net
    eng = net.engine()
    eng.dp_reserve_cus, eng.dp_bucket_opt = reserve, bucket_opt
    probe.install_corunner(eng, k, T)
    x0, y = _batch(0)
    for _ in range(steps):
        net.train.run(_feed(net, x0, y))
    torch.cuda.synchronize()
    key = [q for q in eng._graphs if q[0] == 'tr'][0]
    assert eng._graphs[key][1] == 'whole'
    prog = eng.program('tr', N)
    res = sorted({getattr(op, 'reserve', 0) for op in prog['bwd'] if op.what == 'bwd_scale'})
    return eng.P.cpu().numpy().copy(), res


def test_reserved_cus_and_per_bucket_updates_do_not_change_the_step():
    """Grids that leave compute units to a co-running collective (mpnn_set_reserved_cus) and updates applied bucket
    by bucket on a side stream are a SCHEDULE: four steps give the parameters of the plain single-process step."""
    net = _net()
    x0, y = _batch(0)
    for _ in range(4):
        net.train.run(_feed(net, x0, y))
    torch.cuda.synchronize()
    ref = net.engine().P.cpu().numpy()
    scale = np.abs(ref).max()
    for reserve, bucket_opt in ((0, False), (16, True), (32, True), (16, False)):
        P, res = _standin_run(reserve, bucket_opt)
        assert res == [reserve], res                  # every trunk-backward launch was built with the reservation
        assert np.abs(P - ref).max() <= 3e-4 * scale, (reserve, bucket_opt, np.abs(P - ref).max())
    lib = net.engine().lib
    assert lib.mpnn_set_reserved_cus(-1) == 0         # nothing leaks out of a step


def test_reserved_cus_shrink_the_slot_counts():
    for p in (ROOT, os.path.join(ROOT, 'multipath-nn_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    from lib import _hip
    lib = _hip.load()
    full = lib.mpnn_msconv_bwd_scale_slots(4, 4, 128, 1, 1, 4096)
    assert lib.mpnn_set_reserved_cus(32) == 0
    try:
        less = lib.mpnn_msconv_bwd_scale_slots(4, 4, 128, 1, 1, 4096)
    finally:
        lib.mpnn_set_reserved_cus(0)
    assert 0 < less < full and full - less == 32 * (full // 256), (full, less)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs of one node')
def test_two_gpus_over_rccl_torchrun(tmp_path):
    """torchrun, one process per GPU, RCCL over xGMI: replicas stay bit-identical, the bench runs."""
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    base = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
            '--master-addr', '127.0.0.1', '--master-port', '29561']
    subprocess.check_call(base + [os.path.join(ROOT, 'tests', 'dp_nccl_worker.py')], env=env, cwd=str(tmp_path))
    out = subprocess.check_output(base + [os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '20', '--warmup', '5',
                                          '--no-cpu-baseline'], env=env, cwd=str(tmp_path)).decode()
    import json
    line = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['config']['rccl_ranks'] == 2 and line['value'] > 0


def test_bench_two_ranks_functional_on_one_gpu(tmp_path):
    """bench.py launched exactly as the driver launches it (torch.distributed.run, --gpus 2), both ranks
    on GPU 0 over gloo (RCCL refuses two ranks per GPU): bucket sections, collectives issued in the same
    order on every rank, the rank-0-only measurements of --full after the timed region, the final barrier -- a
    deadlock or a rank-dependent collective shows up here, not on the 8-GPU node."""
    import json
    import subprocess
    env = dict(os.environ, MPNN_DP_BACKEND='gloo', MPNN_DP_ONE_GPU='1', MPNN_SINGLE_GPU_VALUE='250000')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '6', '--warmup', '3',
           '--full', '--no-cpu-baseline', '--eval-batch', '256']
    out = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['config']['global_batch'] == 256 and line['config']['rccl_ranks'] == 2
    assert set(line['config']['allreduce']) == {'end'}
    assert line['value'] > 0 and line['steady_state']['steps'] == 400
    # the run validates itself: both replicas hold the same parameters and accumulators after all 412 steps, and the
    # line says which form of the step ran (gloo: section graphs, no captured-collective self-test)
    cfg = line['config']
    assert cfg['replicas_identical'] is True and cfg['max_abs_param_divergence'] == 0.0 and cfg['max_abs_momentum_divergence'] == 0.0
    assert cfg['dp_form'] == 'sections' and cfg['backend'] == 'gloo' and cfg['captured_collective_selftest'] is None
    assert cfg['bn_moving_average_divergence'] > 0.0            # (per-replica state: the ranks see different images)
    assert abs(cfg['efficiency_vs_single'] - line['value'] / 500000) < 1e-9


def test_bench_spawns_its_own_ranks(tmp_path):
    """`python3 bench.py --gpus 2` with no torchrun environment (the shape of the driver's single-GPU command
    with a larger N): the parent process starts the two ranks itself, relays rank 0's line and the exit code."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    env.update(MPNN_DP_BACKEND='gloo', MPNN_DP_ONE_GPU='1')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '6', '--warmup', '3',
           '--no-cpu-baseline', '--eval-batch', '256']
    out = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, timeout=900)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['config']['rccl_ranks'] == 2 and line['config']['global_batch'] == 256


def test_bench_refuses_a_world_that_differs_from_gpus(tmp_path):
    """--gpus must be the number of ranks that actually run: a 1-rank process group under --gpus 2 is an error,
    not a silent single-GPU number."""
    import subprocess
    env = dict(os.environ, RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1'],
                         env=env, cwd=str(tmp_path), capture_output=True, timeout=600)
    assert out.returncode != 0 and b'--gpus 2' in out.stderr
