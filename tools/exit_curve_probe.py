#!/usr/bin/env python3
"""What the threshold curve of Net.exit_conf_curve costs (profiles/exit_curve_cost.txt).

    python tools/exit_curve_probe.py kernel
        mpnn_exit_curve alone on the tree of ac_chain (8 exits, 7 switches) with random confidences, hits and router
        outputs: 128 and 4 096 images x 1, 64 and 256 points, 200 launches per case in that order.  Run it under
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- and read the kernel's rows with `trace`.
    python tools/exit_curve_probe.py trace DIR
        the exit_curve_k rows of the kernel trace under DIR, split into the six cases by launch order: median and mean µs.
    python tools/exit_curve_probe.py curve [--images 65536] [--points 64] [--batch 4096] [--dump DIR]
        one Net.exit_conf_curve call of --points thresholds over --images images of ac_chain(k_cpt=1e-9) on 32x32x3 (random
        images, randomised routers): wall-clock seconds of the third call, for a host array (streamed) and for a tensor that
        is resident on the device.  --dump DIR: correct / ops / hist as DIR/curve_<name>.npy.
    python tools/exit_curve_probe.py sweep [--images 65536] [--points 64] [--batch 4096] [--dump DIR]
        the same curve the old way: --points calls of Net.predict_all(exit_conf=tau), each result downloaded and joined with
        the labels' hits on the host (one dense labelled eval per chunk supplies them).  Runs on any revision that has
        exit_conf.  --dump DIR: correct / ops / hist as DIR/sweep_<name>.npy.
    python tools/exit_curve_probe.py compare DIR_A DIR_B
        curve_<name>.npy of DIR_A against sweep_<name>.npy of DIR_B, element for element.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'multipath-nn_amd')]

CASES = [(n, T) for n in (128, 4096) for T in (1, 64, 256)]
LAUNCHES = 200


def chain_net():
    """The 8-exit actor chain with moving averages and routers away from their initial values."""
    import arch_and_hypers as A
    net = A.ac_chain(k_cpt=1e-9, seed=1234)((32, 32, 3), (10,))
    eng = net.to('cuda:0').engine()
    eng.init_params(7)
    rng = np.random.default_rng(8)
    for p in net._all_params:
        if not p.trainable:
            p.assign(rng.random(p.shape) * 0.5 + (0.75 if p.name == 'v_avg' else -0.25))
    rng = np.random.default_rng(5)
    for ℓ in net.switches:
        last = ℓ.router.comps[-1].params
        last.w.assign(rng.standard_normal(last.w.shape) * 0.5)
        last.b.assign(rng.standard_normal(last.b.shape) * 0.1)
    return net


def data(n):
    rng = np.random.default_rng(3)
    x = rng.random((n, 32, 32, 3), dtype=np.float32)
    y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]
    return x, y


def points(net, x, T):
    """T thresholds between the 2 % and 98 % quantiles of the first exit's confidences on the first 4 096 images."""
    c = np.sort(net.predict(x[:4096], routed=False, exit_conf=0.0).conf.cpu().numpy())
    return np.linspace(float(c[len(c) // 50]), float(c[-len(c) // 50]), T)


def kernel(args):
    import ctypes as C
    from lib import _hip
    net = chain_net()
    eng, lib = net.engine(), _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    nl, ns, MS = len(eng.leaves), len(eng.switches), eng.max_sinks
    for n, T in CASES:
        conf, d_cor = torch.rand(nl, n, generator=g).cuda(), (torch.rand(nl, n, generator=g) < 0.5).float().cuda()
        r = torch.randn(ns, n, MS, generator=g).cuda()
        taus = torch.rand(T, nl, generator=g).cuda()
        acc = torch.zeros(T * (2 + nl), dtype=torch.int64, device='cuda')
        a = _hip.ExitCurveArgs()
        a.n, a.n_nodes, a.n_leaves, a.n_switches, a.n_points, a.tau_per_leaf = n, len(eng.nodes), nl, ns, T, 1
        a.tree, a.node_ops = eng.curve_tree_dev.data_ptr(), eng.node_ops_i64.data_ptr()
        a.conf, a.conf_stride, a.d_cor, a.dcor_stride = conf.data_ptr(), n, d_cor.data_ptr(), n
        a.r, a.r_stride, a.r_switch_stride, a.taus = r.data_ptr(), MS, n * MS, taus.data_ptr()
        a.correct, a.ops, a.hist = acc.data_ptr(), acc[T:].data_ptr(), acc[2 * T:].data_ptr()
        _hip.check(lib.mpnn_exit_curve_check(C.byref(a), eng.curve_tree), 'record')
        for _ in range(LAUNCHES):
            _hip.check(lib.mpnn_exit_curve(C.byref(a), st), 'exit_curve')
        torch.cuda.synchronize()
        hist = acc[2 * T:].view(T, nl).cpu().numpy()
        assert (hist.sum(1) == LAUNCHES * n).all()
        read = 4 * n * (2 * nl + ns * MS) + 4 * T * nl
        print('exit_curve, %4d images x %3d points: grid %2d workgroups of 256 threads, %d launches; reads %d bytes, %d walks per launch; '
              'exits at point 0: %s' % (n, T, -(-n // 256), LAUNCHES, read, n * T, (hist[0] // LAUNCHES).tolist()))


def trace(args):
    import csv
    import glob
    f = sorted(glob.glob(args.dirs[0] + '/**/*kernel_trace.csv', recursive=True))[-1]
    rows = [r for r in csv.DictReader(open(f)) if 'exit_curve_k' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    assert len(rows) == LAUNCHES * len(CASES), len(rows)
    for k, (n, T) in enumerate(CASES):
        part = rows[k * LAUNCHES:(k + 1) * LAUNCHES]
        assert all(int(r['Grid_Size_X']) // int(r['Workgroup_Size_X']) == -(-n // 256) for r in part)
        us = np.array([(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in part][LAUNCHES // 10:])   # (the first tenth: cold)
        print('exit_curve_k %4d images x %3d points: %d launches, median %.2f us, mean %.2f us, %.1f ns per walk'
              % (n, T, len(us), np.median(us), us.mean(), 1e3 * np.median(us) / (n * T)))


def dump(d, prefix, correct, ops, hist):
    if d:
        os.makedirs(d, exist_ok=True)
        for name, v in (('correct', correct), ('ops', ops), ('hist', hist)):
            np.save(os.path.join(d, '%s_%s.npy' % (prefix, name)), np.asarray(v, np.int64))


def curve(args):
    net = chain_net()
    x, y = data(args.images)
    taus = points(net, x, args.points)
    for where, xs in (('host array', x), ('device tensor', torch.from_numpy(x).cuda())):
        secs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = net.exit_conf_curve(xs, y, taus, batch=args.batch)
            secs.append(time.perf_counter() - t0)
        print('exit_conf_curve, %d images x %d points, batch %d, %s: %s s per call (three calls); accuracy %.4f..%.4f, mean '
              'operations %.4g..%.4g' % (args.images, args.points, args.batch, where, ' '.join('%.3f' % s for s in secs),
                                         res.acc.min(), res.acc.max(), res.moc.min(), res.moc.max()))
    dump(args.dump, 'curve', res.correct, res.ops, res.hist)


def sweep(args):
    net = chain_net()
    x, y = data(args.images)
    taus = points(net, x, args.points)
    nl, N = len(list(net.leaves)), args.images
    for where, xs in (('host array', x), ('device tensor', torch.from_numpy(x).cuda())):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hits = np.zeros((nl, N), bool)                           # the labels' side: one dense labelled eval per chunk
        for i0 in range(0, N, args.batch):
            net.eval({net.x0: xs[i0:i0 + args.batch], net.y: y[i0:i0 + args.batch]})
            hits[:, i0:i0 + args.batch] = np.stack([ℓ.δ_cor.cpu().numpy() == 1 for ℓ in net.leaves])
        t_eval = time.perf_counter() - t0
        correct, ops, hist = np.zeros(args.points, np.int64), np.zeros(args.points, np.int64), np.zeros((args.points, nl), np.int64)
        for t, tau in enumerate(taus):
            res = net.predict_all(xs, batch=args.batch, exit_conf=float(tau))
            leaf = res.leaf.cpu().numpy()
            ops[t], hist[t] = int(res.ops.sum()), np.bincount(leaf, minlength=nl)
            correct[t] = int(hits[leaf, np.arange(N)].sum())
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        print('%d x predict_all(exit_conf=tau), %d images, batch %d, %s: %.3f s in all (%.3f s of it the labelled eval); accuracy '
              '%.4f..%.4f' % (args.points, N, args.batch, where, secs, t_eval, correct.min() / N, correct.max() / N))
    dump(args.dump, 'sweep', correct, ops, hist)


def compare(args):
    a, b = args.dirs
    bad = 0
    for name in ('correct', 'ops', 'hist'):
        u, v = np.load(os.path.join(a, 'curve_%s.npy' % name)), np.load(os.path.join(b, 'sweep_%s.npy' % name))
        ok = u.shape == v.shape and np.array_equal(u, v)
        bad += not ok
        print('curve against sweep, %-8s %6d elements  %s' % (name, u.size, 'equal' if ok else 'DIFFERENT'))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['kernel', 'trace', 'curve', 'sweep', 'compare'])
    ap.add_argument('dirs', nargs='*')
    ap.add_argument('--images', type=int, default=65536)
    ap.add_argument('--points', type=int, default=64)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--dump', metavar='DIR')
    a = ap.parse_args()
    dict(kernel=kernel, trace=trace, curve=curve, sweep=sweep, compare=compare)[a.what](a)
