"""Training-step time of nets on the any-channel conv entry points (csrc/conv_gen_ch.hip) against the any-map ones:

  (a) a NARROW table ([8]*4, [8]*4, [24]*3, [24]*3, [40]*2, [40]*2, [72], [72]) on mpnn_msconv_*_ch against the same net with
      every count rounded up to the next multiple of 16 on mpnn_msconv_*_hw (MPNN_ANYMAP_CONVS=1) -- what a user would
      have to run without the any-channel family; the padded table also with the any-width exit kernels
      (MPNN_GENERIC_EXITS=1), which the narrow table's exits need, to tell the convs' share from the exits';
  (b) the shipped table under MPNN_ANYCHAN_CONVS=1 against MPNN_ANYMAP_CONVS=1: what the fitted output tiles change.

ac_chain(k_cpt=0), batch 128, 32x32x3, one hipGraph per step.  Every variant is warmed up, then timed over `steps` steps
(HIP events around chunks of ten); the variants alternate `reps` times in one process.

    python tools/anychan_step.py [steps] [reps]        (only=<variant> in the environment: that variant alone, once)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'multipath-nn_amd'))
import numpy as np
import torch
import arch_and_hypers as A

NARROW = [[8] * 4, [8] * 4, [24] * 3, [24] * 3, [40] * 2, [40] * 2, [72], [72]]
PADDED = [[(c + 15) // 16 * 16 for c in row] for row in NARROW]
SHIPPED = A.arch
FLAGS = ('MPNN_ANYCHAN_CONVS', 'MPNN_ANYMAP_CONVS', 'MPNN_GENERIC_EXITS')
VARIANTS = {                                      # name: (table, environment)
    'narrow_ch': (NARROW, {}),
    'padded_hw': (PADDED, {'MPNN_ANYMAP_CONVS': '1'}),
    'padded_hw_genexits': (PADDED, {'MPNN_ANYMAP_CONVS': '1', 'MPNN_GENERIC_EXITS': '1'}),
    'shipped_ch': (SHIPPED, {'MPNN_ANYCHAN_CONVS': '1'}),
    'shipped_hw': (SHIPPED, {'MPNN_ANYMAP_CONVS': '1'}),
}
n = 128


def build(name):
    table, env = VARIANTS[name]
    for k in FLAGS:
        os.environ.pop(k, None)
    os.environ.update(env)
    A.arch = table
    try:
        net = A.ac_chain(k_cpt=0.0, seed=1234)((32, 32, 3), (10,))
        eng = net.engine()
    finally:
        A.arch = SHIPPED
        for k in FLAGS:
            os.environ.pop(k, None)
    eng._ensure_capacity(n)
    g = torch.Generator().manual_seed(0)
    eng.x0[:n].copy_(torch.rand((n, 32, 32, 3), generator=g)); eng.y[:n].zero_(); eng.y[:n, 0] = 1
    feed = {net.x0: eng.x0[:n], net.y: eng.y[:n], net.mode: 'tr', net.λ_lrn: 0.1, net.τ: 1.0}
    print('%-20s convs: generic %d anymap %d anychan %d; generic exits %d' % (
        name, eng.generic_convs, eng.anymap_convs, eng.anychan_convs, eng.generic_exits), flush=True)
    return net, feed


def timed(net, feed, steps):
    for _ in range(30):
        net.train.run(feed)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    K = steps // 10
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(K + 1)]
    evs[0].record(st)
    for k in range(K):
        for _ in range(10):
            net.train.run(feed)
        evs[k + 1].record(st)
    torch.cuda.synchronize()
    return np.array([evs[k].elapsed_time(evs[k + 1]) / 10 for k in range(K)]) * 1e3


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    only = os.environ.get('only')
    names = [only] if only else list(VARIANTS)
    nets = {k: build(k) for k in names}
    med = {k: [] for k in names}
    for rep in range(1 if only else reps):
        for k in names:
            per = timed(*nets[k], steps)
            med[k].append(float(np.median(per)))
            print('rep %d %-20s step_us median %.1f mean %.1f min %.1f max %.1f' % (rep, k, np.median(per), per.mean(), per.min(), per.max()),
                  flush=True)
    for k in names:
        print('%-20s medians %s  spread %.1f us' % (k, ' '.join('%.1f' % v for v in med[k]), max(med[k]) - min(med[k])))
    if not only:
        r = lambda a, b: np.median(med[a]) / np.median(med[b])
        print('narrow_ch / padded_hw %.3f   narrow_ch / padded_hw_genexits %.3f   shipped_ch / shipped_hw %.3f'
              % (r('narrow_ch', 'padded_hw'), r('narrow_ch', 'padded_hw_genexits'), r('shipped_ch', 'shipped_hw')))


if __name__ == '__main__':
    main()
