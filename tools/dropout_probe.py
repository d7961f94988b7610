#!/usr/bin/env python3
"""What Dropout in front of the exit classifiers costs (profiles/dropout_cost.txt).

    python tools/dropout_probe.py step [--exit-dropout LAMBDA[:K]] [--batch 128] [--reps 400]
        the training step of ac_chain(k_cpt=0) on 32x32x3, 10 classes, resident inputs, four steps per hipGraph replay
        (bench.py's loop): median ms per step over HIP events (tools/superclass_probe.py's timing).  Without
        --exit-dropout no exit carries the layer.
    python tools/dropout_probe.py launches [--reps 200]
        mpnn_dropout_fwd and mpnn_dropout_bwd alone through the C ABI: 128 and 512 rows, K = 256 and 2 048 (16 pixels of 16
        and of 128 channels, batch statistics), tables of 1 and of 8 records, λ = 0.5: median us per launch over HIP events
        round chunks of 20 back-to-back launches (the launch floor of the same loop with mpnn_debug_noop beside it).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'multipath-nn_amd'), os.path.join(ROOT, 'tools')]
from superclass_probe import time_replays


def step(args):
    import arch_and_hypers as A
    if args.exit_dropout:
        A.exit_dropout = A.parse_exit_dropout(args.exit_dropout)
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
    ops = [op for k in ('fwd', 'bwd') for op in eng.program('tr', n)[k] if op.what not in ('fork', 'join', 'bucket')]
    lin = [len(op.host) for op in ops if op.what == 'lin_fwd']
    print('step %s batch %d: %s ms per step (3 medians of %d steps), %d launches per step, %s lin records, parameters finite: %s'
          % ('--exit-dropout ' + args.exit_dropout if args.exit_dropout else 'no Dropout layer', n, ' '.join('%.4f' % m for m in ms),
             args.reps, len(ops), lin, bool(torch.isfinite(eng.P).all())))


def launches(args):
    from lib import _hip
    lib = _hip.load()
    dev = 'cuda:0'
    st = lambda: torch.cuda.current_stream().cuda_stream
    step_t = torch.zeros(1, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    noop = lambda: lib.mpnn_debug_noop(st())
    floor = time_replays(lambda: [noop() for _ in range(20)], args.reps, chunk=5) / 20 * 1e3
    print('launch floor (mpnn_debug_noop, 20 back to back): %.2f us per launch' % floor)
    for n in (128, 512):
        for HW, C_ in ((16, 16), (16, 128)):
            K = HW * C_
            for count in (1, 8):
                keep, recs = [], []
                for r in range(count):
                    x = torch.from_numpy(rng.standard_normal((n, HW, C_)).astype(np.float32)).to(dev)
                    x64 = x.double().reshape(-1, C_)
                    sums = torch.zeros(_hip.BN_SLOTS, 2 * C_, dtype=torch.float64, device=dev)
                    sums[0, :C_], sums[0, C_:] = x64.sum(0), (x64 ** 2).sum(0)
                    bn = dict(sum=sums, gamma=torch.ones(C_, device=dev), beta=torch.zeros(C_, device=dev),
                              m_avg=torch.zeros(C_, device=dev), v_avg=torch.ones(C_, device=dev), eps=1e-6, nslot=8)
                    xd, dxd, dx = (torch.zeros(n, K, device=dev) for _ in range(3))
                    d = _hip.DropoutArgs()
                    d.a, d.HW, d.n = _hip.act(x, C_, _hip.ACT_BN_BATCH, 0, bn, n * HW), HW, n
                    d.seed_lo, d.leaf, d.thresh, d.inv_keep = 1 + r, r, 1 << 31, 2.0
                    d.step, d.xd, d.dxd, d.dx, d.accumulate = step_t.data_ptr(), xd.data_ptr(), dxd.data_ptr(), dx.data_ptr(), 1
                    _hip.check(lib.mpnn_dropout_check(C.byref(d)), 'dropout record')
                    keep += [x, sums, bn, xd, dxd, dx]
                    recs.append(d)
                tab = _hip.to_device_table(recs, dev)
                out = []
                for fn in (lib.mpnn_dropout_fwd, lib.mpnn_dropout_bwd):
                    one = lambda: _hip.check(fn(tab.data_ptr(), count, n, K, st()), 'dropout launch')
                    for _ in range(50):
                        one()
                    torch.cuda.synchronize()
                    out.append(sorted(time_replays(lambda: [one() for _ in range(20)], args.reps, chunk=5) / 20 * 1e3 for _ in range(3))[1])
                mb = count * n * K * 4 / 1e6
                print('n %4d  K %5d  records %d: fwd %6.2f us  bwd %6.2f us per launch (%.2f MB of map per pass)' % (n, K, count, out[0], out[1], mb))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('what', choices=('step', 'launches'))
    ap.add_argument('--exit-dropout', metavar='LAMBDA[:K]')
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--reps', type=int, default=400)
    args = ap.parse_args()
    (step if args.what == 'step' else launches)(args)


if __name__ == '__main__':
    main()
