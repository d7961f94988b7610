"""What MultiscaleLLN costs (csrc/lln.hip: mpnn_lln_fwd, one launch in front of block 0).

  (a) the launch alone at n = 128 and n = 4 096, 32x32x3, 4 scales, σ = 3 (radius 6): HIP events around chunks of back-to-back
      launches on one stream, after a warm-up; median / min / max of the chunk means, and the bytes the algorithm needs
      (the image read once, the four scales written once) over that time;
  (b) ac_chain(k_cpt=0) with and without the layer: the training step at batch 128 (one hipGraph per step) and
      predict at 4 096 images (routed='auto'), the two variants alternating `reps` times in one process.

    python tools/lln_probe.py [steps] [reps]
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'multipath-nn_amd'))
import numpy as np
import torch
import arch_and_hypers as A


def chunks(fn, n_chunks, per):
    """Microseconds per call of fn: the means of n_chunks chunks of `per` calls (HIP events on the current stream)."""
    st = torch.cuda.current_stream()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_chunks + 1)]
    evs[0].record(st)
    for k in range(n_chunks):
        for _ in range(per):
            fn()
        evs[k + 1].record(st)
    torch.cuda.synchronize()
    return np.array([evs[k].elapsed_time(evs[k + 1]) / per for k in range(n_chunks)]) * 1e3


def build(lln, seed=1234):
    A.lln = lln
    try:
        net = A.ac_chain(k_cpt=0.0, seed=seed)((32, 32, 3), (10,))
    finally:
        A.lln = None
    net.engine()
    return net


def launch_alone(n):
    net = build({})
    eng = net.engine()
    eng.ensure_capacity(n, train=False)
    g = torch.Generator().manual_seed(0)
    eng.x0[:n].copy_(torch.rand((n, 32, 32, 3), generator=g))
    op, = [o for o in eng.program('ev', n)['fwd'] if o.what == 'lln']
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(200):                                    # warm clocks, code object loaded
        op(st)
    torch.cuda.synchronize()
    per = chunks(lambda: op(st), 40, 50)
    px = sum((32 >> i) ** 2 for i in range(4))
    byts = n * 3 * 4 * (32 * 32 + px)                       # x0 read once + four scales written
    print('lln launch  n %5d: us median %.2f min %.2f max %.2f (40 chunks of 50 launches); %.1f MB needed -> %.0f GB/s at the median'
          % (n, np.median(per), per.min(), per.max(), byts / 1e6, byts / np.median(per) / 1e3), flush=True)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for n in (128, 4096):
        launch_alone(n)
    nets = {'plain': build(None), 'lln': build({})}
    g = torch.Generator().manual_seed(0)
    n, n_ev = 128, 4096
    x_tr, x_ev = torch.rand((n, 32, 32, 3), generator=g).cuda(), torch.rand((n_ev, 32, 32, 3), generator=g).cuda()
    y = torch.zeros(n, 10).cuda(); y[:, 0] = 1
    step, rate = {k: [] for k in nets}, {k: [] for k in nets}
    for rep in range(reps):
        for k, net in nets.items():
            feed = {net.x0: x_tr, net.y: y, net.mode: 'tr', net.λ_lrn: 0.1, net.τ: 1.0}
            for _ in range(30):
                net.train.run(feed)
            torch.cuda.synchronize()
            per = chunks(lambda: net.train.run(feed), steps // 10, 10)
            step[k].append(float(np.median(per)))
            print('rep %d %-6s step_us   median %.1f min %.1f max %.1f' % (rep, k, np.median(per), per.min(), per.max()), flush=True)
        for k, net in nets.items():
            for _ in range(10):
                net.predict(x_ev)
            torch.cuda.synchronize()
            per = chunks(lambda: net.predict(x_ev), 20, 5)
            rate[k].append(float(n_ev / np.median(per)))
            print('rep %d %-6s predict_us median %.1f min %.1f max %.1f -> %.3f M img/s' % (rep, k, np.median(per), per.min(), per.max(),
                                                                                      n_ev / np.median(per)), flush=True)
    for k in nets:
        print('%-6s step medians %s us; predict rates %s M img/s' % (k, ' '.join('%.1f' % v for v in step[k]),
                                                                    ' '.join('%.3f' % v for v in rate[k])))
    print('lln - plain: step %+.1f us (%.2f %%); predict rate x %.3f' % (
        np.median(step['lln']) - np.median(step['plain']), 100 * (np.median(step['lln']) / np.median(step['plain']) - 1),
        np.median(rate['lln']) / np.median(rate['plain'])))


if __name__ == '__main__':
    main()
