"""End-to-end rate of classifying images that start in pageable host memory (profiles/predict_stream.txt).

    predict_stream_sweep.py --parent DIR [--batch 4096 512] [--images 65536] [--reps 7]

The stock ac_chain on 32x32x3 images, one eighth leaving at each exit (calibrated on the first 4 096 decoded images).
DIR is a built checkout of the commit to compare against.  Two worker processes are kept alive on one GPU -- one on DIR's
tree, one on this tree -- and asked in turn, so that the two versions alternate inside one run; every figure is the median of
--reps repeats after a warm-up of the same call, and every repeat of (a)-(d) ends with the results on the host.

  (a) classify() of DIR's classify-images on float32 images        (the parent's chunk loop: convert, upload, run, .cpu())
  (b) classify() of this tree's classify-images on the same images
  (c) Net.predict_all on float32 images, results copied to the host
  (d) Net.predict_all on uint8 images with decode='gamma', results copied to the host
  (e) Net.predict with the inputs resident in the engine's buffers (the protocol of profiles/predict_eval_sweep.txt: a
      host-clock window of 400 / 1 500 calls ending in a device synchronise), on both trees: the ceiling of (a)-(d)
  (f) mpnn_decode_u8 alone on 4 096 images (device events around 200 launches), and the stages of one chunk of (d)
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12                 # bytes/s: the HBM3E specification of the MI355X
WORKER_LIMIT = 300.0              # seconds a worker may take to answer one request


# ------------------------------------------------------------------------------------------------ worker
def worker(root, n_images):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'multipath-nn_amd'))
    import runpy
    import numpy as np
    import torch
    import arch_and_hypers as A
    import bench
    classify = runpy.run_path(os.path.join(root, 'multipath-nn_amd', 'classify-images'), run_name='not_main')['classify']
    net = A.ac_chain(k_cpt=0.0, seed=1234)((32, 32, 3), (10,))
    eng = net.engine()
    rng = np.random.default_rng(5)
    for l in net.layers:                      # the last router map starts at zero: give the routers something to decide on
        if l.router is not None:
            w = l.router.comps[-1].params.w
            w.assign(rng.standard_normal(w.shape) * 0.5)
    xu = np.random.default_rng(1).integers(0, 256, (n_images, 32, 32, 3), dtype=np.uint8)
    gamma = np.float32(np.arange(256, dtype=np.uint8) ** 2.2 / 255 ** 2.2)
    xf = gamma[xu]                            # pageable host memory, as np.load gives it
    cal = min(4096, n_images)
    y = np.eye(10, dtype=np.float32)[np.random.default_rng(2).integers(0, 10, cal)]
    bench.set_exit_fractions(net, {net.x0: xf[:cal], net.y: y}, cal, [1 / 8] * 7)
    has_all = hasattr(net, 'predict_all')
    keep = {}

    def to_host(res):
        return [t.cpu() for t in (res.cls, res.leaf, res.conf, res.ops)]

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def op_classify(b):
        t, out = wall(lambda: classify(net, xf, b))
        keep['classify'] = out
        return dict(s=t, hist=np.bincount(out['leaf'], minlength=8).tolist(), crc=int(out['cls'].astype(np.int64).sum() * 31 + out['ops'].sum() % 1000003))

    def op_all(b, kind):
        x, dec = (xu, 'gamma') if kind == 'u8' else (xf, None)
        t, out = wall(lambda: to_host(net.predict_all(x, batch=b, decode=dec)))
        same = all(np.array_equal(keep['classify'][k], v.numpy()) for k, v in zip(('cls', 'leaf', 'conf', 'ops'), out)) if 'classify' in keep else None
        return dict(s=t, same_as_classify=same)

    def op_resident(b):
        eng.ensure_capacity(b, train=False)
        eng.x0[:b].copy_(torch.from_numpy(xf[:b]))
        calls = 400 if b >= 2048 else 1500
        for _ in range(5):
            net.predict(eng.x0[:b])
        t, _ = wall(lambda: [net.predict(eng.x0[:b]) for _ in range(calls)])
        return dict(s=t / calls)

    def op_stages(b):
        """One chunk of (d) and of (c), stage by stage: the host copy into a pinned buffer, the upload, the decode (or the
        device copy into x0) -- the program is the resident figure."""
        out = {}
        eng.ensure_capacity(b, train=False)
        for kind, x, dt in (('u8', xu, torch.uint8), ('f32', xf, torch.float32)):
            pin = torch.empty((b, 32, 32, 3), dtype=dt, pin_memory=True)
            dev = torch.empty((b, 32, 32, 3), dtype=dt, device=eng.dev)
            ts = []
            for r in range(9):
                src = torch.from_numpy(x[(r * b) % (n_images - b + 1):][:b])
                t = time.perf_counter()
                pin.copy_(src)
                ts.append(time.perf_counter() - t)
            out[kind + '_host_copy_s'] = float(np.median(ts[2:]))
            ups = []
            for r in range(9):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dev.copy_(pin, non_blocking=True)
                e1.record()
                torch.cuda.synchronize()
                ups.append(e0.elapsed_time(e1) * 1e-3)
            out[kind + '_upload_s'] = float(np.median(ups[2:]))
            if kind == 'u8':
                lut = eng._decode_lut(gamma)
                run = lambda: eng._decode_launch(dev, b, lut)
            else:
                run = lambda: eng.x0[:b].copy_(dev)
            for _ in range(10):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                run()
            e1.record()
            torch.cuda.synchronize()
            out[kind + '_to_x0_s'] = e0.elapsed_time(e1) * 1e-3 / 200
        # a plain float copy of the decode's output size on the same device, same loop: what a streaming kernel reaches here
        a, c = torch.empty((b, 32, 32, 3), device=eng.dev), torch.empty((b, 32, 32, 3), device=eng.dev)
        for _ in range(10):
            c.copy_(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            c.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        out['float_copy_s'] = e0.elapsed_time(e1) * 1e-3 / 200
        return out

    print(json.dumps(dict(ready=True, has_all=has_all)), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == 'quit':
            break
        b = int(cmd[1])
        res = (op_classify(b) if cmd[0] == 'classify' else op_all(b, cmd[2]) if cmd[0] == 'all' else
               op_resident(b) if cmd[0] == 'resident' else op_stages(b))
        print(json.dumps(res), flush=True)


# ------------------------------------------------------------------------------------------------ driver
class Proc:
    def __init__(self, root, n_images):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--worker', root, '--images', str(n_images)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        # (a thread hands the worker's lines over, so that waiting for an answer has a time limit)
        import queue
        import threading
        self.lines = queue.Queue()
        threading.Thread(target=self._pump, daemon=True).start()
        self.info = self._read()

    def _pump(self):
        for line in self.p.stdout:
            self.lines.put(line)
        self.lines.put('')                                    # (end of the worker's output)

    def _read(self):
        import queue
        while True:
            try:
                line = self.lines.get(timeout=WORKER_LIMIT)
            except queue.Empty:
                self.p.kill()
                raise RuntimeError('worker gave no answer within %.0f s' % WORKER_LIMIT)
            if not line:
                raise RuntimeError('worker ended (exit status %r)' % self.p.poll())
            if line.startswith('{'):
                return json.loads(line)

    def ask(self, *cmd):
        self.p.stdin.write(' '.join(str(c) for c in cmd) + '\n')
        self.p.stdin.flush()
        return self._read()

    def close(self):
        try:
            self.p.stdin.write('quit\n')
            self.p.stdin.flush()
        except Exception:
            pass
        self.p.wait(timeout=60)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--worker', metavar='ROOT')
    ap.add_argument('--parent', metavar='DIR')
    ap.add_argument('--batch', nargs='*', type=int, default=[4096, 512])
    ap.add_argument('--images', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.images)
    if not args.parent:
        ap.error('--parent DIR: a built checkout of the commit to compare against')
    N, R = args.images, args.reps
    old, new = Proc(os.path.abspath(args.parent), N), Proc(HERE, N)
    assert not old.info['has_all'] and new.info['has_all']
    print('Classifying %d images 32x32x3 that start in pageable host memory: the stock ac_chain, one eighth leaving at each exit\n'
          '(calibrated on the first 4 096 decoded images), hipGraph replay.  Two processes kept alive on one MI355X -- the parent\n'
          'commit and this one -- asked in turn; %d repeats per figure after one warm-up call of the same kind; (a)-(d) are host-clock\n'
          'times of one pass over all images that end with cls, leaf, conf and ops on the host; spread = max - min of the repeats.\n' % (N, R))
    try:
        for b in args.batch:
            rows = [('(a) parent classify f32', old, ('classify', b)), ('(b) this classify f32', new, ('classify', b)),
                    ('(c) predict_all f32', new, ('all', b, 'f32')), ('(d) predict_all u8 gamma', new, ('all', b, 'u8'))]
            ts = {name: [] for name, _, _ in rows}
            extra = {}
            for name, proc, cmd in rows:                       # warm-up: every shape, the graphs, the pinned buffers
                extra[name] = proc.ask(*cmd)
            for _ in range(R):
                for name, proc, cmd in rows:
                    r = proc.ask(*cmd)
                    ts[name].append(r['s'])
                    extra[name] = r
            res = {}
            for name, _, _ in rows:
                med, lo, hi = res[name] = stats(ts[name])
                print('batch %5d  %-26s median %8.2f ms  min %8.2f  max %8.2f  spread %6.2f  %6.3f M img/s   repeats %s' % (
                    b, name, med * 1e3, lo * 1e3, hi * 1e3, (hi - lo) * 1e3, N / med / 1e6, ' '.join('%.2f' % (t * 1e3) for t in ts[name])))
            hist_a, hist_b = extra[rows[0][0]]['hist'], extra[rows[1][0]]['hist']
            print('batch %5d  exit histogram %s; (b) == (a): %s; (c), (d) == (b): %s %s' % (
                b, hist_a, hist_a == hist_b and extra[rows[0][0]]['crc'] == extra[rows[1][0]]['crc'],
                extra[rows[2][0]]['same_as_classify'], extra[rows[3][0]]['same_as_classify']))
            # (e) resident inputs, both trees in turn
            rs = {'parent': [], 'this': []}
            for _ in range(R):
                rs['parent'].append(old.ask('resident', b)['s'])
                rs['this'].append(new.ask('resident', b)['s'])
            for who in ('parent', 'this'):
                med, lo, hi = res['e ' + who] = stats(rs[who])
                print('batch %5d  (e) %-6s predict resident median %.4f ms  min %.4f  max %.4f  spread %.4f  %6.3f M img/s   repeats %s' % (
                    b, who, med * 1e3, lo * 1e3, hi * 1e3, (hi - lo) * 1e3, b / med / 1e6, ' '.join('%.4f' % (t * 1e3) for t in rs[who])))
            st = new.ask('stages', b)
            elems = b * 32 * 32 * 3
            dec = st['u8_to_x0_s']
            cp = st['float_copy_s']
            print('batch %5d  (f) mpnn_decode_u8 on %d images: %.1f us, %.2f TB/s = %.0f %% of the 8.0 TB/s HBM peak; a float copy of its output size '
                  '(torch, same loop): %.1f us, %.2f TB/s, so the decode moves bytes at %.0f %% of that copy\'s rate' % (
                      b, b, dec * 1e6, 5 * elems / dec / 1e12, 100 * 5 * elems / dec / HBM_PEAK, cp * 1e6, 8 * elems / cp / 1e12,
                      100 * (5 * elems / dec) / (8 * elems / cp)))
            prog = res['e this'][0]
            for kind, label in (('u8', '(d)'), ('f32', '(c)')):
                print('batch %5d  stages of one chunk of %s: host copy into pinned %.3f ms, upload %.3f ms (%.1f GB/s), %s %.3f ms, program %.3f ms' % (
                    b, label, st[kind + '_host_copy_s'] * 1e3, st[kind + '_upload_s'] * 1e3,
                    elems * (1 if kind == 'u8' else 4) / st[kind + '_upload_s'] / 1e9, 'decode' if kind == 'u8' else 'copy into x0',
                    st[kind + '_to_x0_s'] * 1e3, prog * 1e3))
            chunks = (N + b - 1) // b
            for kind, label, row in (('u8', '(d)', rows[3][0]), ('f32', '(c)', rows[2][0])):
                per = res[row][0] / chunks
                stage = {'the host copy into pinned memory': st[kind + '_host_copy_s'], 'the upload': st[kind + '_upload_s'],
                         'the program': prog + st[kind + '_to_x0_s']}
                bound = max(stage, key=stage.get)
                print('batch %5d  %s takes %.3f ms per chunk; its longest stage is %s (%.3f ms), the stages beside it are hidden behind it; '
                      'the other %.3f ms are the four result copies, the gaps between eager launches and the graph, the first upload and the '
                      'last download' % (b, label, per * 1e3, bound, stage[bound] * 1e3, (per - stage[bound]) * 1e3))
            a, sp = res[rows[0][0]][0], res[rows[0][0]][2] - res[rows[0][0]][1]
            bm, dm = res[rows[1][0]][0], res[rows[3][0]][0]
            print('batch %5d  (b) - (a) = %+.2f ms, spread of (a) %.2f ms: %s;  (a) - (d) = %+.2f ms: %s;  (d) reaches %.0f %% of (e)' % (
                b, (bm - a) * 1e3, sp * 1e3, 'not slower by more than that spread' if bm - a <= sp else 'SLOWER by more than that spread',
                (a - dm) * 1e3, 'faster by more than that spread' if a - dm > sp else 'NOT faster by more than that spread',
                100 * (N / dm) / (b / prog)))
            ep, et = res['e parent'], res['e this']
            print('batch %5d  (e) this - parent = %+.4f ms, spread of the parent %.4f ms: %s\n' % (
                b, (et[0] - ep[0]) * 1e3, (ep[2] - ep[1]) * 1e3,
                'within that spread' if et[0] - ep[0] <= ep[2] - ep[1] else 'SLOWER by more than that spread'), flush=True)
    finally:
        old.close()
        new.close()


if __name__ == '__main__':
    main()
