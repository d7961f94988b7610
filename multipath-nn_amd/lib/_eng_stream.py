"""8-bit inputs and whole datasets for the label-free evaluation: the on-device decode in front of a 'pr' program
(mpnn_decode_u8, csrc/decode.hip) and Net.predict_all -- chunks of a host array go through a ring of pinned buffers and a
copy stream into a device staging buffer while the previous chunk's program runs ("Label-free
evaluation")."""
from types import SimpleNamespace as Ns

import numpy as np
import torch

from lib import _hip
from lib._upload import UploadRing

RING = 2                           # pinned host buffers of predict_all: one being uploaded, one being filled (uploads are serial
                                   # on the one device staging buffer, so a third slot would never be in flight)


class StreamedPredict:

    # ------------------------------------------------------------------ decode
    def _init_stream_state(self):
        """Engine.__init__: nothing is allocated before the first decode / predict_all."""
        self._dec_lut = None             # device copy of the decode table last used, the table's bytes, and -- for the
        self._dec_raw = None             # READ-ONLY named tables only -- the host object (spares the comparison)
        self._dec_named = None
        self.decode_uploads = 0          # uploads of a decode table so far (only when the table changes)
        self._stage_bufs = {}            # dtype -> device staging buffer [capacity, H, W, C]
        self._pinned = {}                # dtype -> UploadRing of RING pinned host buffers [rows, H, W, C]
        self._copy_stream = None

    def _decode_lut(self, table):
        """The device copy of a decode table (np.float32[256]); uploaded only when the table's VALUES change: a caller's
        own array may have been rewritten in place since the last call, so it is compared byte for byte (1 KB); only
        the read-only named tables of lib/decode.py are recognised by identity."""
        if self._dec_named is table and not table.flags.writeable:
            return self._dec_lut
        raw = table.tobytes()
        if self._dec_raw != raw:
            if self._dec_lut is None:
                self._dec_lut = torch.zeros(256, device=self.dev)
            self._dec_lut.copy_(torch.from_numpy(np.array(table, dtype=np.float32)))       # (stream-ordered behind earlier decodes)
            self._dec_raw = raw
            self.decode_uploads += 1
        self._dec_named = None if table.flags.writeable else table
        return self._dec_lut

    def _stage_buffer(self, dtype):
        """The device staging buffer [capacity, H, W, C] of a dtype (uint8 bytes in front of the decode, float32 images in
        front of the copy into x0): allocated on first use, grows with the capacity."""
        bufs = self._stage_bufs
        t = bufs.get(dtype)
        if t is None or t.shape[0] < self.n_max:
            if t is not None and self._copy_stream is not None:
                self._copy_stream.synchronize()                  # (an upload into the old buffer may still be running)
            t = bufs[dtype] = torch.empty((self.n_max,) + tuple(self.x0_shape), dtype=dtype, device=self.dev)
        return t

    def _image_count(self, x):
        n = int(x.shape[0])
        per = int(np.prod(self.x0_shape))
        numel = x.numel() if isinstance(x, torch.Tensor) else x.size
        if numel != n * per:
            raise ValueError('images of shape %r do not fit the net\'s input %r' % (tuple(x.shape[1:]), tuple(self.x0_shape)))
        return n

    def _decode_launch(self, src, n, lut):
        """x0[:n] = lut[src]: one eager launch on the current stream (src: n images of bytes in device memory)."""
        _hip.check(self.lib.mpnn_decode_u8(src.data_ptr(), self.x0.data_ptr(), lut.data_ptr(), n * int(np.prod(self.x0_shape)),
                                           torch.cuda.current_stream().cuda_stream), 'decode_u8')

    def _decode_into_x0(self, x0, table):
        """predict(decode=): the bytes of a host array go to the uint8 staging buffer (a device tensor is read where it
        lies), mpnn_decode_u8 writes the engine's x0; returns x0[:n], which the staging of the 'pr' program then finds in
        place."""
        n = self._image_count(x0)
        self._ensure_capacity(n, False)
        lut = self._decode_lut(table)
        if isinstance(x0, torch.Tensor) and x0.is_cuda:
            src = x0.contiguous()
        else:
            src = self._stage_buffer(torch.uint8)[:n]
            if not isinstance(x0, torch.Tensor):
                x0 = np.ascontiguousarray(x0)
                x0 = torch.from_numpy(x0 if x0.flags.writeable else x0.copy())
            src.copy_(x0.reshape(src.shape), non_blocking=True)
        self._decode_launch(src, n, lut)
        return self.x0[:n]

    # ------------------------------------------------------------------ predict_all
    def _pinned_ring(self, dtype, rows):
        """The upload ring of a dtype: RING pinned host buffers [rows, H, W, C]; grows with the chunk size."""
        ring = self._pinned.get(dtype)
        if ring is None or ring.rows < rows:
            if ring is not None:
                ring.drain()
            ring = self._pinned[dtype] = UploadRing(RING, (rows,) + tuple(self.x0_shape), dtype)
        return ring

    def predict_all(self, x, batch=4096, routed='auto', probs=False, k_cpt=None, table=None, exit_conf=None):
        """Net.predict_all: predict() over x in chunks of `batch`, the results gathered in full-length device tensors of
        their own.  A host array is streamed: chunk i + 1 is copied into a pinned buffer and uploaded on a copy stream
        while chunk i's program runs; the upload waits only for the launch that consumed the staging buffer (the decode,
        or the copy into x0), and a pinned buffer is reused only after the event behind its last upload has completed (the
        rule of lib/_upload.py) -- the only place where the host waits for the device.  exit_conf: as in predict, the same
        thresholds for every chunk."""
        N = self._image_count(x)
        dev = self.dev
        out = Ns(cls=torch.empty(N, dtype=torch.int32, device=dev), leaf=torch.empty(N, dtype=torch.int32, device=dev),
                 conf=torch.empty(N, device=dev), ops=torch.empty(N, dtype=torch.int64, device=dev),
                 probs=torch.empty((N, self.n_cls_max), device=dev) if probs else None)
        if N == 0:
            return out
        cap = min(batch, N)
        self._ensure_capacity(cap, False)
        kc = None
        if k_cpt is not None and getattr(self.net.hypers, 'dyn_k_cpt', False):
            kc = torch.as_tensor(k_cpt, dtype=torch.float32).reshape(-1).to(dev)          # (on the device once: a chunk's values are a slice)
            if kc.numel() not in (1, N):
                raise ValueError('predict_all: k_cpt is one value or one per image (%d given for %d images)' % (kc.numel(), N))
        lut = self._decode_lut(table) if table is not None else None

        def run(i0, n, x0):
            res = self.predict(x0, routed, probs, k_cpt if kc is None else kc if kc.numel() == 1 else kc[i0:i0 + n],       # (its refusals are predict's)
                               exit_conf=exit_conf)
            out.cls[i0:i0 + n].copy_(res.cls)                     # (on the compute stream, before the next program rewrites them)
            out.leaf[i0:i0 + n].copy_(res.leaf)
            out.conf[i0:i0 + n].copy_(res.conf)
            out.ops[i0:i0 + n].copy_(res.ops)
            if probs:
                out.probs[i0:i0 + n].copy_(res.probs)

        self._for_each_chunk(x, N, batch, lut, run)
        return out

    def _for_each_chunk(self, x, N, batch, lut, run):
        """run(i0, n, x0) for every chunk of `batch` images of x, with the chunk's images in place (x0 = self.x0[:n], or a
        slice of a float device tensor): the streaming of predict_all, shared with exit_conf_curve.  lut: the device decode
        table of 8-bit images, or None.  The capacity is the caller's (_ensure_capacity(min(batch, N)))."""
        dev, cur, cap = self.dev, torch.cuda.current_stream(), min(batch, N)
        if isinstance(x, torch.Tensor) and x.is_cuda:             # already on the device: no ring, no staging buffer
            x = x.reshape((N,) + tuple(self.x0_shape))
            for i0 in range(0, N, batch):
                n = min(batch, N - i0)
                if lut is not None:
                    self._decode_launch(x[i0:i0 + n].contiguous(), n, lut)
                    run(i0, n, self.x0[:n])
                else:
                    run(i0, n, x[i0:i0 + n])
            return

        if isinstance(x, torch.Tensor):
            x = x.numpy()
        x = x.reshape((N,) + tuple(self.x0_shape))
        dtype = torch.uint8 if lut is not None else torch.float32
        stage = self._stage_buffer(dtype)
        ring = self._pinned_ring(dtype, cap)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=dev)
        cs = self._copy_stream
        ev = torch.cuda.Event()
        ev.record(cur)
        cs.wait_event(ev)                                         # (earlier work on the compute stream may read the staging buffer)
        state = Ns(consumed=None)

        def upload(i0):
            n = min(batch, N - i0)
            buf = ring.acquire()
            chunk = x[i0:i0 + n]
            if chunk.flags.writeable:
                buf[:n].copy_(torch.from_numpy(chunk))
            else:
                np.copyto(buf[:n].numpy(), chunk, casting='unsafe')
            if state.consumed is not None:
                cs.wait_event(state.consumed)
            with torch.cuda.stream(cs):
                stage[:n].copy_(buf[:n], non_blocking=True)
            return n, ring.release(cs)

        nxt = upload(0)
        for i0 in range(0, N, batch):
            n, up = nxt
            cur.wait_event(up)
            if lut is not None:
                self._decode_launch(stage[:n], n, lut)
            else:
                self.x0[:n].copy_(stage[:n])
            state.consumed = torch.cuda.Event()
            state.consumed.record(cur)
            run(i0, n, self.x0[:n])
            if i0 + batch < N:
                nxt = upload(i0 + batch)                          # (host copy and upload of chunk i + 1 beside chunk i's program)

    # ------------------------------------------------------------------ exit_conf_curve
    def exit_conf_curve(self, x, y, taus, batch=4096, k_cpt=None, table=None):
        """Net.exit_conf_curve: the threshold curve of a labelled data set in ONE dense pass.  taus: float32 [T, leaves] on
        the host (NaN: that exit is not gated), uploaded once; the accumulators are zeroed once; every chunk of `batch`
        images goes through the streaming of predict_all into the 'ev+c' program (lib/_eng_eval.py: the dense labelled
        evaluation whose exits also store their confidences, then mpnn_exit_curve, which adds the chunk's images to the
        T x (correct, ops, hist) integer sums -- one hipGraph per chunk size from the third chunk of that size on); the
        three arrays are downloaded once at the end.  Returns (correct [T], ops [T], hist [T, leaves]) as int64 numpy
        arrays."""
        net = self.net
        N, T, nl = self._image_count(x), int(taus.shape[0]), len(self.leaves)
        dyn = bool(getattr(net.hypers, 'dyn_k_cpt', False))
        if any(nd.kind != 'head' for nd in self.leaves):
            raise NotImplementedError('exit_conf_curve: a leaf without a classifier has no confidence')
        zeros = (np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros((T, nl), np.int64))
        if N == 0:
            return zeros
        dev = self.dev
        self._ensure_capacity(min(batch, N), False)
        d_taus, ring, acc = self._curve_buffers(T)
        ring.upload(d_taus, torch.from_numpy(np.ascontiguousarray(taus, np.float32)))
        acc.zero_()
        y = (y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y, np.float32))).to(dev, torch.float32)
        kc = None
        if dyn:
            kc = torch.as_tensor(k_cpt, dtype=torch.float32).reshape(-1).to(dev)
            if kc.numel() not in (1, N):
                raise ValueError('exit_conf_curve: k_cpt is one value or one per image (%d given for %d images)' % (kc.numel(), N))
        lut = self._decode_lut(table) if table is not None else None

        def run(i0, n, x0):
            feed = {net.x0: x0, net.y: y[i0:i0 + n]}
            if dyn:
                feed[net.k_cpt] = kc if kc.numel() == 1 else kc[i0:i0 + n]
            n_, _ = self._enter(feed)
            self._dispatch(self.program('ev+c', n_, False, points=T), False, n_)
            self.last_n, self.last_mode = n_, 'cv'            # (no p_ev, no statistics: state() refuses)

        self._for_each_chunk(x, N, batch, lut, run)
        out = acc.cpu().numpy()                                # (the one download: waits for the last chunk)
        return out[:T].copy(), out[T:2 * T].copy(), out[2 * T:].reshape(T, nl).copy()
