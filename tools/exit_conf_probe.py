#!/usr/bin/env python3
"""What the confidence-threshold exits of Net.predict(exit_conf=) cost (profiles/exit_conf_cost.txt).

    python tools/exit_conf_probe.py kernel
        mpnn_conf_gate alone: one record of a two-way switch with one child list, 128, 512 and 4 096 rows, 200 launches
        each: run it under rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- and read the kernel's rows (the
        grid tells the cases apart: `trace`).
    python tools/exit_conf_probe.py trace DIR
        the conf_gate kernel's rows of the kernel trace under DIR, by grid size: launches, median and mean µs.
    python tools/exit_conf_probe.py predict [--batch 4096] [--reps 300] [--ungated] [--dump DIR]
        Net.predict of ac_chain(k_cpt=1e-9) on 32x32x3 with resident images, its routers calibrated to one eighth of the
        batch per exit, as hipGraph replays: median ms per call over HIP events, for routed='auto' and routed=1 -- under the
        learnt routers and under thresholds calibrated to the SAME exit fractions (each one a confidence that occurs at its
        exit).  --ungated: the learnt routers only (runs on any revision).  --dump DIR: the ungated answer as DIR/<name>.npy.
    python tools/exit_conf_probe.py compare DIR_A DIR_B
        every .npy of the two directories byte for byte.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'multipath-nn_amd')]

KEYS = ('cls', 'leaf', 'conf', 'ops', 'probs')


def time_replays(run, reps, chunk=10):
    st = torch.cuda.current_stream()
    k = max(1, reps // chunk)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(k + 1)]
    evs[0].record(st)
    for i in range(k):
        for _ in range(chunk):
            run()
        evs[i + 1].record(st)
    torch.cuda.synchronize()
    return float(np.median([evs[i].elapsed_time(evs[i + 1]) / chunk for i in range(k)]))


def host(res):
    torch.cuda.synchronize()
    return {k: getattr(res, k).cpu().numpy().copy() for k in KEYS if getattr(res, k) is not None}


def calibrated_chain(n):
    """The 8-exit actor chain with moving averages and routers away from their initial values, the routers' exit biases
    shifted so that one eighth of the n images leaves at each exit (the arrangement of tests/test_routed_eval.py)."""
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
    rng = np.random.default_rng(3)
    x0 = rng.random((n, 32, 32, 3)).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.integers(0, 10, n)]
    net.eval({net.x0: x0, net.y: y})
    alive = np.ones(n, bool)
    for ℓ in net.switches:
        r = ℓ.router.x.cpu().numpy().astype(np.float64)
        margin = r[:, 1] - r[:, 0]
        idx = np.flatnonzero(alive)
        order = idx[np.argsort(margin[idx], kind='stable')]
        b = ℓ.router.comps[-1].params.b
        v = b.numpy().copy()
        v[0] += 0.5 * (margin[order[n // 8 - 1]] + margin[order[n // 8]])
        b.assign(v)
        alive[order[:n // 8]] = False
    return net, x0


def predict(args):
    n = args.batch
    net, x0 = calibrated_chain(n)
    eng = net.engine()
    eng.x0[:n].copy_(torch.from_numpy(x0).cuda())
    x = eng.x0[:n]                                                # (resident: no upload in the timed calls)
    base = host(net.predict(x, routed=False, probs=True))
    print('batch %d, exits under the learnt routers: %s' % (n, np.bincount(base['leaf'], minlength=8).tolist()))
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for routed in (False, 'auto', 1):
            for k, v in host(net.predict(x, routed=routed, probs=True)).items():
                np.save(os.path.join(args.dump, 'predict_%s_%s.npy' % (routed, k)), v)
    taus = None
    if not args.ungated:
        # thresholds with the same exit fractions: per exit the confidence (of the images still on their way) with which one
        # eighth of the batch leaves; the confidences of exit k for every image come from the run that forces everybody out there
        inf = float('inf')
        alive, taus = np.ones(n, bool), []
        for k in range(7):
            c = host(net.predict(x, routed=False, exit_conf=[-inf if j == k else inf for j in range(8)]))['conf']
            idx = np.flatnonzero(alive)
            taus.append(float(np.sort(c[idx])[::-1][n // 8 - 1]))
            alive[idx[c[idx] >= np.float32(taus[k])]] = False
        taus.append(None)
        gated = host(net.predict(x, routed=False, probs=True, exit_conf=taus))
        print('batch %d, exits under the thresholds:      %s' % (n, np.bincount(gated['leaf'], minlength=8).tolist()))
    for routed in ('auto', 1):
        sides = [('learnt', {})] + ([('thresholds', dict(exit_conf=taus))] if taus is not None else [])
        for rnd in range(2):                                      # (two rounds, the sides alternating)
            for name, kw in sides:
                run = lambda: net.predict(x, routed=routed, **kw)
                for _ in range(20):
                    run()
                torch.cuda.synchronize()
                ms = [time_replays(run, args.reps) for _ in range(3)]
                gate = frozenset(range(7)) if kw else frozenset()
                whats = [op.what for op in eng.program('pr', n, routed, *([gate] if kw else []))['fwd']]
                print('predict batch %d routed=%r %-10s round %d: %s ms per call (3 medians of %d calls), %d launches, %d of them conf_gate'
                      % (n, routed, name, rnd + 1, ' '.join('%.4f' % m for m in ms), args.reps, len(whats), whats.count('conf_gate')))


def kernel(args):
    import ctypes as C
    from lib import _hip
    lib = _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    for n in (128, 512, 4096):
        conf = torch.rand(n, generator=g).cuda()
        tau = torch.tensor([0.5]).cuda()
        r0 = torch.randn(n, 4, generator=g).cuda()
        r = r0.clone()
        lst, cnt = torch.zeros(n, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
        rec = _hip.ConfGateArgs()
        rec.conf, rec.tau, rec.r, rec.r_stride, rec.n_sinks, rec.exit_sink, rec.n = conf.data_ptr(), tau.data_ptr(), r.data_ptr(), 4, 2, 0, n
        rec.child_idx[1], rec.child_cnt[1] = lst.data_ptr(), cnt.data_ptr()
        _hip.check(lib.mpnn_conf_gate_check(C.byref(rec)), 'record')
        tab = _hip.to_device_table([rec], 'cuda')
        for _ in range(200):
            r.copy_(r0)
            cnt.zero_()
            _hip.check(lib.mpnn_conf_gate(tab.data_ptr(), 1, n, st), 'conf_gate')
        torch.cuda.synchronize()
        stay = conf < 0.5
        assert int(cnt[0]) == int(stay.sum()) and torch.equal(torch.sort(lst[:int(cnt[0])].long()).values, torch.nonzero(stay)[:, 0])
        assert torch.equal(r[:, 0], (~stay).float()) and torch.equal(r[:, 1], stay.float()) and torch.equal(r[:, 2:], r0[:, 2:])
        print('conf_gate, %d rows: grid %d workgroups of 256 threads, 200 launches' % (n, -(-n // 256)))


def trace(args):
    import csv
    import glob
    f = sorted(glob.glob(args.dirs[0] + '/**/*kernel_trace.csv', recursive=True))[-1]
    by_grid = {}
    for r in csv.DictReader(open(f)):
        if 'conf_gate_k' in r['Kernel_Name']:
            grid = int(r['Grid_Size_X']) // int(r['Workgroup_Size_X'])
            by_grid.setdefault(grid, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    for grid, us in sorted(by_grid.items()):
        us = np.array(us[len(us) // 10:])                      # (the first tenth: cold launches)
        print('conf_gate_k grid %5d workgroups: %d launches, median %.2f us, mean %.2f us' % (grid, len(us), np.median(us), us.mean()))


def compare(args):
    a, b = args.dirs
    names = sorted(f for f in os.listdir(a) if f.endswith('.npy'))
    assert names and names == sorted(f for f in os.listdir(b) if f.endswith('.npy')), 'the two directories hold different files'
    bad = 0
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        ok = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        bad += not ok
        print('dump %-28s %8d elements %-8s %s' % (f, x.size, x.dtype, 'bit-identical' if ok else 'DIFFERENT'))
    print('all dumped arrays bit-identical' if not bad else '%d arrays differ' % bad)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['kernel', 'trace', 'predict', 'compare'])
    ap.add_argument('dirs', nargs='*')
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--ungated', action='store_true')
    ap.add_argument('--dump', metavar='DIR')
    a = ap.parse_args()
    dict(kernel=kernel, trace=trace, predict=predict, compare=compare)[a.what](a)
