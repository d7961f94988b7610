"""Dense vs routed evaluation throughput over batch sizes (exit fractions 1/8 each).

    eval_sweep.py [batch ...]                          the stock 3x3 actor chain on 32x32 images (the tuned kernels)
    eval_sweep.py --supp 5 [batch ...]                 conv_supp = 5: a net on the general conv kernels (csrc/conv_gen.hip)
    eval_sweep.py --supp 5 --shape 24 40 [batch ...]   ... on 24x40 images (the any-map entry points)
    --prefix-sweep (or PREFIX_SWEEP=1): every gather depth d0 of the routed program instead of True / 'auto'
    --reps R: R timed repetitions per figure; the median and the (min .. max) spread are printed"""
import sys, os, time, argparse
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'multipath-nn_amd'))
import torch, numpy as np, arch_and_hypers as A
import bench
ap = argparse.ArgumentParser()
ap.add_argument('batches', nargs='*', type=int)
ap.add_argument('--supp', type=int, default=A.conv_supp, help='conv_supp of the spec file (3: the tuned kernels)')
ap.add_argument('--shape', nargs=2, type=int, default=[32, 32], metavar=('H', 'W'))
ap.add_argument('--prefix-sweep', action='store_true', default=bool(os.environ.get('PREFIX_SWEEP')))
ap.add_argument('--reps', type=int, default=1)
ap.add_argument('--iters', type=int, default=20)
args = ap.parse_args()
A.conv_supp = args.supp
H, W = args.shape
net = A.ac_chain(k_cpt=0.0, seed=1234)((H, W, 3), (10,))
eng = net.engine()
print('ac_chain conv_supp %d on %dx%d images: %s' % (args.supp, H, W, 'general conv kernels (%s)' % ('_hw' if eng.anymap_convs else '_gen')
                                                       if eng.generic_convs else 'tuned conv kernels'), flush=True)
rng = np.random.default_rng(5)
for l in net.layers:                      # the last router map starts at zero: give the routers something to decide on
    if l.router is not None:
        w = l.router.comps[-1].params.w
        w.assign(rng.standard_normal(w.shape) * 0.5)


def timed(routed):
    """Median and spread (ms per evaluation) of args.reps repetitions of args.iters evaluations."""
    for _ in range(3): net.eval(feed, routed=routed)
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(args.iters): net.eval(feed, routed=routed)
        torch.cuda.synchronize(); ts.append((time.perf_counter() - t) / args.iters * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


fmt = lambda r: '%.3f' % r[0] if args.reps == 1 else '%.3f (%.3f..%.3f)' % r
for nb in args.batches or [1024, 4096, 8192]:
    if (H, W) == (32, 32):
        x, y = bench.synthetic(nb, 1, 'cuda:0')
    else:
        g = torch.Generator().manual_seed(1)
        x = torch.rand((nb, H, W, 3), generator=g).to('cuda:0')
        y = torch.nn.functional.one_hot(torch.randint(0, 10, (nb,), generator=g), 10).float().to('cuda:0')
    eng._ensure_capacity(nb, train=False)
    eng.x0[:nb].copy_(x); eng.y[:nb].copy_(y)
    feed = {net.x0: eng.x0[:nb], net.y: eng.y[:nb]}
    bench.set_exit_fractions(net, feed, nb, [1 / 8] * 7)
    res = {}
    if args.prefix_sweep:
        # routed evaluation with the convs of the blocks above depth d0 run on every sample (lib/_eng_eval.py:_program_ev);
        # d0 = 8 is beyond the deepest block of the chain: every conv on every sample, the exits made routed by the prefix walk
        line = [(d0, timed(d0)) for d0 in (False, 1, 2, 3, 4, 5, 6, 7, 8)]
        line.append(('auto', timed('auto')))
        print('batch %6d: ' % nb + '  '.join('%s %s' % ('dense' if d0 is False else d0 if d0 == 'auto' else 'd0=%d' % d0, fmt(t))
                                              for d0, t in line) + '  (ms)', flush=True)
        continue
    for routed in (False, True, 'auto'):
        res[routed] = timed(routed)
    print('batch %6d: dense %s ms (%.2f M img/s)  routed %s ms (%.2f M img/s)  x%.2f   routed=auto %s ms (x%.2f)' % (
        nb, fmt(res[False]), nb / res[False][0] / 1e3, fmt(res[True]), nb / res[True][0] / 1e3, res[False][0] / res[True][0],
        fmt(res['auto']), res[False][0] / res['auto'][0]), flush=True)
    if nb == 4096:
        print('   exit histogram', [round(float(nd.layer.p_ev.mean()), 3) for nd in eng.leaves])
        prog = eng.program('ev', nb, routed=True)
        st = torch.cuda.current_stream()
        tot = [0.0] * len(prog['fwd'])
        for rep in range(6):
            eng._begin(False)                      # (clears the sample counts: the lists are appended to)
            evs = []
            for op in prog['fwd']:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st); op(st.cuda_stream); e1.record(st)
                evs.append((e0, e1))
            torch.cuda.synchronize()
            if rep:
                for k, (e0, e1) in enumerate(evs): tot[k] += e0.elapsed_time(e1) / 5
        for op, t in zip(prog['fwd'], tot):
            print('   routed %-12s %-30s %8.1f us' % (op.what, op.tag[:30], t * 1e3))
