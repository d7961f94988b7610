#!/usr/bin/env python3
"""What ActivityError layers at the exits cost (profiles/activity_error_cost.txt).

    python tools/activity_probe.py [--exit-activity WHERE=ALPHA[,WHERE=ALPHA][:K]] [--batch 128] [--reps 400]
        the training step of ac_chain(k_cpt=0) on 32x32x3, 10 classes, resident inputs, four steps per hipGraph replay
        (bench.py's loop): median ms per step over HIP events (tools/superclass_probe.py's timing).  Without
        --exit-activity no exit carries the layer (on a revision without it: tools/squared_probe.py, the same loop).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'multipath-nn_amd'), os.path.join(ROOT, 'tools')]
from superclass_probe import time_replays


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--exit-activity', metavar='WHERE=ALPHA[,WHERE=ALPHA][:K]')
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--reps', type=int, default=400)
    args = ap.parse_args()
    import arch_and_hypers as A
    if args.exit_activity:
        A.exit_activity = A.parse_exit_activity(args.exit_activity)
    net = A.ac_chain(k_cpt=0.0, seed=1234)((32, 32, 3), (10,))
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
    print('step %s batch %d: %s ms per step (3 medians of %d steps), %d launches per step, parameters finite: %s'
          % (args.exit_activity or 'no activity layer', n, ' '.join('%.4f' % m for m in ms), args.reps, launches,
             bool(torch.isfinite(eng.P).all())))


if __name__ == '__main__':
    main()
