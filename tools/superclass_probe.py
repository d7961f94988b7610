#!/usr/bin/env python3
"""What exits with a label space of their own cost (profiles/superclass_cost.txt).

    python tools/superclass_probe.py step [--coarse] [--batch 128] [--reps 400]
        the training step of ac_chain(k_cpt=1.6e-8) on 32x32x3, 10 classes, resident inputs, four steps per hipGraph replay
        (bench.py's loop): median ms per step over HIP events.  --coarse: the exits of blocks 0-2 on a 10>2 map, those of
        blocks 3-4 on a 10>5 map (net (a) of tests/test_superclass_nets.py).  Without --coarse it runs on any revision.
    python tools/superclass_probe.py kernel
        mpnn_label_map alone, 10>2 and 100>20 at 128 and 4 096 rows, 200 launches each: run it under
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- and read the kernel's rows (the grid tells the
        cases apart: `trace`).
    python tools/superclass_probe.py trace DIR
        the label_map kernel's rows of the kernel trace under DIR, by grid size: launches, median and mean µs.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'multipath-nn_amd')]


def hard_map(n_cls, n_sup):
    w = np.zeros((n_cls, n_sup), np.float32)
    w[np.arange(n_cls), np.arange(n_cls) * n_sup // n_cls] = 1
    return w


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


def step(args):
    import arch_and_hypers as A
    if args.coarse:
        A.coarse_exits = {**{i: hard_map(10, 2) for i in range(3)}, **{i: hard_map(10, 5) for i in (3, 4)}}
    net = A.ac_chain(k_cpt=1.6e-8, seed=1234)((32, 32, 3), (10,))
    eng = net.to('cuda:0').engine()
    n = args.batch
    eng.ensure_capacity(n, train=True)
    g = torch.Generator().manual_seed(0)
    eng.x0[:n].copy_(torch.rand((n, 32, 32, 3), generator=g).cuda())
    eng.y[:n].copy_(torch.nn.functional.one_hot(torch.randint(0, 10, (n,), generator=g), 10).float().cuda())
    feed = {net.x0: eng.x0[:n], net.y: eng.y[:n], net.mode: 'tr', net.λ_lrn: A.λ_lrn(0), net.τ: A.τ_ds(0)}
    run = lambda: net.train.run_steps([feed] * 4)
    for _ in range(30):
        run()
    torch.cuda.synchronize()
    ms = [time_replays(run, args.reps // 4, chunk=5) / 4 for _ in range(3)]
    launches = sum(1 for k in ('fwd', 'bwd') for op in eng.program('tr', n)[k] if op.what not in ('fork', 'join', 'bucket'))
    print('step %s batch %d: %s ms per step (3 medians of %d steps), %d launches per step'
          % ('coarse' if args.coarse else 'plain', n, ' '.join('%.4f' % m for m in ms), args.reps, launches))


def kernel(args):
    import ctypes as C
    from lib import _hip
    lib = _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    for n_cls, n_sup in ((10, 2), (100, 20)):
        for n in (128, 4096):
            y = torch.nn.functional.one_hot(torch.randint(0, n_cls, (n,)), n_cls).float().cuda()
            w = torch.from_numpy(hard_map(n_cls, n_sup)).cuda()
            out = torch.zeros(n, n_sup, device='cuda')
            rec = _hip.LabelMapArgs()
            rec.y, rec.w_cls, rec.y_sup, rec.n, rec.n_cls, rec.n_sup = y.data_ptr(), w.data_ptr(), out.data_ptr(), n, n_cls, n_sup
            _hip.check(lib.mpnn_label_map_check(C.byref(rec)), 'record')
            tab = _hip.to_device_table([rec], 'cuda')
            for _ in range(200):
                _hip.check(lib.mpnn_label_map(tab.data_ptr(), 1, n, n_sup, st), 'label_map')
            torch.cuda.synchronize()
            assert torch.equal(out, y @ w)
            print('label_map %d>%d, %d rows: grid %d workgroups of 256 threads, 200 launches'
                  % (n_cls, n_sup, n, -(-n // 16) * -(-n_sup // 16)))


def trace(args):
    import csv
    import glob
    f = sorted(glob.glob(args.dir + '/**/*kernel_trace.csv', recursive=True))[-1]
    by_grid = {}
    for r in csv.DictReader(open(f)):
        if 'label_map_k' in r['Kernel_Name']:
            grid = int(r['Grid_Size_X']) // int(r['Workgroup_Size_X'])
            by_grid.setdefault(grid, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    for grid, us in sorted(by_grid.items()):
        us = np.array(us[len(us) // 10:])                      # (the first tenth: cold launches)
        print('label_map_k grid %5d workgroups: %d launches, median %.2f us, mean %.2f us' % (grid, len(us), np.median(us), us.mean()))


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=['step', 'kernel', 'trace'])
    ap.add_argument('dir', nargs='?')
    ap.add_argument('--coarse', action='store_true')
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--reps', type=int, default=400)
    a = ap.parse_args()
    dict(step=step, kernel=kernel, trace=trace)[a.what](a)
