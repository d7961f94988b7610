"""The flat HBM buffers of a net, allocated from the layout of lib/_eng_structure.py: parameters / momentum / gradients,
BatchNorm state, the fp64 statistic arenas, the layout's tables on the device, per-block activation and gradient maps
sized for a batch capacity."""
import ctypes as C

import numpy as np
import torch

from lib import _hip
from lib._upload import ValueRing
from lib._eng_common import Launch, _attr


class Allocation:

    # ------------------------------------------------------------------ parameters
    def _alloc_params(self):
        """The flat buffers of the layout (Structure._layout, which has every size and offset), and its tables on the device."""
        dev = self.dev
        up = lambda a: torch.from_numpy(a).to(dev)
        self.P = torch.zeros(self.n_params, device=dev)
        self.A = torch.zeros(self.n_params, device=dev)
        self.S = torch.zeros(max(self.n_state, 1), device=dev)
        self.packs = torch.zeros(max(self.pack_size, 1), device=dev)
        self.pack_desc = up(self.pack_desc_host)
        self.w_eq = up(self.w_eq_host) if self.w_eq_host is not None else None
        self._packs_fresh = False
        self.seg = up(self.seg_host)
        # dsum | dred | loss live in ONE byte arena so a step zeroes them with a single memset
        nd = self.n_dsum
        # ... together with the gradient tensor (and its node-statistics tail): mpnn_step_begin clears
        # the whole arena in the launch that packs the weights.
        zb = (2 * nd + 4) * 8
        gb = (self.n_params * 4 + 15) // 16 * 16
        self._zarena = torch.zeros(zb + gb, dtype=torch.uint8, device=dev)
        z64 = self._zarena[:zb].view(torch.float64)
        self.dsum, self.dred, self.loss = z64[:nd], z64[nd:2 * nd], z64[2 * nd:2 * nd + 4]
        # the forward sums of the LAST completed training step (the live ones are cleared by their last reader)
        self.dsum_last = torch.zeros(nd, dtype=torch.float64, device=dev)
        self.G = self._zarena[zb:zb + self.n_params * 4].view(torch.float32)
        self.node_stat = self.G[:self.n_stat]
        for p in self.trainable:
            p.data = self.P[p.offset:p.offset + p.size]
            p.grad = self.G[p.offset:p.offset + p.size]
            p.accum = self.A[p.offset:p.offset + p.size]
            p._on_assign = self.invalidate_packs
        for p in self.state_params:
            p.data = self.S[p.offset:p.offset + p.size]
        self.bn_table = up(self.bn_table_host)
        self.node_tab, self.kid_tab, self.leaf_node_tab = up(self.node_tab_host), up(self.kid_tab_host), up(self.leaf_node_tab_host)
        self.node_ops = torch.tensor(self.node_ops_host, dtype=torch.float32, device=dev)
        self.node_ops_i64 = up(self.node_ops_i64_host)
        self.hyp = torch.zeros(_hip.HYP_N, device=dev)
        self._hyp_stage = torch.zeros(_hip.HYP_N)
        self._hyp_ring = ValueRing(8, (_hip.HYP_N,))
        # gate_tau: one threshold per leaf in device memory (the confidence-threshold exits of Structure.gateable) -- a
        # program bakes in the ADDRESSES of its gated leaves' entries, each call uploads the values in front of it.
        self.gate_tau = torch.zeros(max(len(self.leaves), 1), device=dev)
        self._tau_stage = torch.zeros(max(len(self.leaves), 1))
        self._tau_ring = ValueRing(8, (max(len(self.leaves), 1),))
        # drop_steps: the step counters the Dropout launches draw with, in device memory -- slot 0 for the one-step program,
        # slot j for step j of a K-step graph (lib/_eng_ksteps.py); the host fills them in front of every launch or replay
        self.has_dropout = any(b.drop is not None for b in self.blocks)
        self.drop_steps = torch.zeros(self.STEPS_MAX, dtype=torch.int32, device=dev)
        self._drop_stage = torch.zeros(self.STEPS_MAX, dtype=torch.int32)
        self._drop_ring = ValueRing(8, (self.STEPS_MAX,), dtype=torch.int32)
        self.curve_tree_dev = _hip.to_device_table(list(self.curve_tree), dev)
        self._curve_bufs = {}              # points T -> (taus [T, leaves] on the device, its upload ring, accumulators int64 [T, 2 + leaves])
        self.w_cls_dev = [torch.from_numpy(w).to(dev) for w in self.label_maps]


    def init_params(self, seed=None):
        """Draw every parameter from the reference's initialisation law
        (layer_types.py:48-50, 64-71, 156-173, 227-230)."""
        rng = np.random.default_rng(seed)
        P = np.zeros(self.n_params, np.float32)
        S = np.zeros(self.S.numel(), np.float32)
        for p in self.net._all_params:
            kind, scale = p.init
            if kind == 'normal':
                v = (scale * rng.standard_normal(p.size)).astype(np.float32)
                if p.eq is not None:
                    v = v + p.eq.reshape(-1)
            elif kind == 'ones':
                v = np.ones(p.size, np.float32)
            else:
                v = np.zeros(p.size, np.float32)
            (P if p.trainable else S)[p.offset:p.offset + p.size] = v
        self.P.copy_(torch.from_numpy(P))
        self.S.copy_(torch.from_numpy(S))
        self.A.zero_()
        self.invalidate_packs()


    # ------------------------------------------------------------------ buffers
    def _ensure_capacity(self, n, train=True):
        """Device buffers for batches of up to n samples.  The evaluation path ('ev': forward only, any
        batch size -- the statistics pass of scripts/lib/desc.py:10-22 feeds thousands of images per
        launch) allocates only what a forward pass touches; the gradient buffers follow the largest
        TRAINING batch seen."""
        dev = self.dev
        z = lambda *shape: torch.zeros(shape, device=dev)
        if n > self.n_max:
            biggest = max([b.H[i] * b.W[i] * b.C[i] for b in self.blocks for i in range(b.L)] + [int(np.prod(self.x0_shape))])
            if n * biggest >= 2 ** 30:
                raise ValueError('batch of %d samples: the kernels address an activation tensor with 32-bit byte offsets' % n)
            self.n_max = n
            self._progs.clear()
            self._graphs.clear()
            self._gen += 1                                 # (buffer generation: lib/_co.py rebuilds its merged program)
            self.n_max_bwd = 0
            h, w, c0 = self.x0_shape
            self.x0 = z(n, h, w, c0)
            if self.lln is not None:
                self.lln_out = [z(n, h >> i, w >> i, c0) for i in range(len(self.lln.x))]
            self.y = z(n, self.n_cls)
            self.y_sup = [z(n, w.shape[1]) for w in self.label_maps]       # (written by the 'label_map' launch of a program)
            self.k_cpt = z(n)
            for b in self.blocks:
                b.s = [z(n, b.H[i], b.W[i], b.C[i]) for i in range(b.L)]
                b.sp = [z(n, b.H[i] // 2, b.W[i] // 2, b.C[i]) for i in range(b.L - 1)]     # 2x2-max-pooled s
                if b.has_exit:
                    b.z = z(n, b.n_out) if b.head is not None else None
                    if b.router is not None:
                        R, R2 = (b.router.comps[k].hypers.n_chan for k in (1, 4))
                        b.R, b.R2 = R, R2
                        b.h1, b.h2 = z(n, R), z(n, R2)
                        b.bn_save = z(2 * R + 2 * R2)
            nn, nl, ns = len(self.nodes), len(self.leaves), max(len(self.switches), 1)
            self.p_tr, self.p_ev = z(nn * n), z(nn * n)
            self.w_cerr = z(nl * n)
            self.dr = z(ns * n * self.max_sinks)
            # One allocation that the evaluation path clears with the launch that packs the weights:
            # loss sums | per-block sample counts of the routed evaluation | r | c_err | d_cor
            # (routed evaluation only writes the entries of samples that REACH a node).
            nb = (len(self.blocks) + 3) // 4 * 4
            n_r, n_l = ns * n * self.max_sinks, nl * n
            self._ev_arena = torch.zeros(32 + 4 * nb + 4 * ((n_r + 2 * n_l + 3) // 4 * 4), dtype=torch.uint8, device=dev)
            self.loss_ev = self._ev_arena[:32].view(torch.float64)
            self.ev_cnt = self._ev_arena[32:32 + 4 * nb].view(torch.int32)
            fl = self._ev_arena[32 + 4 * nb:].view(torch.float32)
            self.r, self.c_err, self.d_cor = fl[:n_r], fl[n_r:n_r + n_l], fl[n_r + n_l:n_r + 2 * n_l]
            for k, b in enumerate(self.blocks):
                b.ev_idx = torch.zeros(n, dtype=torch.int32, device=dev)     # samples routed to this block ('ev')
                b.ev_cnt = self.ev_cnt[k:k + 1]
            # label-free evaluation (Net.predict): every head's prediction by image [leaves][n], and the answer by sample;
            # the softmax rows [leaves][n][n_cls] only once a call asks for them (EvalPrograms._pr_rows)
            self.pr_cls = torch.zeros(nl * n, dtype=torch.int32, device=dev)
            self.pr_conf = z(nl * n)
            self.pr_p = self.pr_probs = None
            self.res_leaf = torch.zeros(n, dtype=torch.int32, device=dev)
            self.res_cls = torch.zeros(n, dtype=torch.int32, device=dev)
            self.res_conf = z(n)
            self.res_ops = torch.zeros(n, dtype=torch.int64, device=dev)
        if train and n > self.n_max_bwd:
            self.n_max_bwd = n
            self._gen += 1
            self._progs = {k: v for k, v in self._progs.items() if k[0] != 'tr'}
            self._graphs = {k: v for k, v in self._graphs.items() if k[0] not in ('tr', 'trK')}
            for b in self.blocks:
                b.dzg = [z(n, b.H[i], b.W[i], b.C[i]) for i in range(b.L)]
                if b.has_exit:
                    b.dx = z(n, b.H[-1] * b.W[-1] * b.C[-1])
                    b.dzh = z(n, b.n_out) if b.head is not None else None
                    if b.drop is not None:             # Dropout in front of the head: the dropped map and the head's dX
                        b.xd, b.dxd = z(n, b.H[-1] * b.W[-1] * b.C[-1]), z(n, b.H[-1] * b.W[-1] * b.C[-1])
                    if b.router is not None:
                        b.dh1 = z(n, b.R)
                        b.dh2 = z(n, b.R2) if (self.generic_exits or n > 128) else None     # (scratch of mpnn_exit_tail_bwd_gen)


    # ------------------------------------------------------------------ programs
    def _bn(self, b, i, with_sum=True):
        bn = b.bns[i].params
        return dict(sum=self.dsum[b.sum_off[i]:] if with_sum else None, gamma=bn.γ.data, beta=bn.β.data,
                    m_avg=bn.m_avg.data, v_avg=bn.v_avg.data, eps=float(b.bns[i].hypers.ϵ),
                    nslot=self._nslot(b, i))


    def _act_of_input(self, b, i, n, mode, fwd=False):
        """mpnn_act of the block's input at scale i."""
        if b.in_map is None:
            if fwd and getattr(self, 'rgbx_probe', False) and b.in_shift[i] > 0:
                # TIMING PROBE (tools/rgbx_probe.py; results are only right while x4 holds the strided picks of x0): the
                # pyramid scale as a dense 4-channel map (RGBX, X = 0) -- aligned float4 pixels, no address shift
                return _hip.act(self.x4[b.in_shift[i]], 4, _hip.ACT_IDENTITY, 0)
            if self.lln is not None:
                return _hip.act(self.lln_out[b.in_shift[i]], self.x0_shape[2], _hip.ACT_IDENTITY, 0)
            return _hip.act(self.x0, self.x0_shape[2], _hip.ACT_IDENTITY, b.in_shift[i])
        pb, j = b.parent, b.in_map[i]
        return _hip.act(pb.s[j], pb.C[j], mode, 0, self._bn(pb, j), n * pb.H[j] * pb.W[j])


    def _lln_launches(self, n):
        """The launch in front of the first conv of every program of a net with MultiscaleLLN: [mpnn_lln_fwd] -- x0 to the
        normalised scales lln_out (always dense: root blocks never carry a sample list) -- or [] without the layer.  host:
        the net's record (the co-trainer concatenates the records of its nets; the geometry is the architecture's)."""
        if self.lln is None:
            return []
        ℓ = self.lln
        rec = _hip.LlnArgs()
        rec.x, rec.n, rec.eps = self.x0.data_ptr(), n, float(_attr(ℓ.hypers, 'ϵ'))
        for i, t in enumerate(self.lln_out):
            rec.out[i] = t.data_ptr()
        geom = _hip.LlnGeom()
        geom.n_max, geom.H, geom.W, geom.n_scales, geom.radius = n, self.x0_shape[0], self.x0_shape[1], len(self.lln_out), ℓ.radius
        for k, g in enumerate(ℓ.taps()):
            geom.tap[k] = g                        # (float64 on the host, rounded to fp32 here)
        tab = _hip.to_device_table([rec], self.dev)
        self._keep += [rec, geom, tab]
        px = sum(t[0].numel() for t in self.lln_out) // 3
        return [Launch(self.lib.mpnn_lln_fwd, 'lln', tab.data_ptr(), 1, C.byref(geom), host=[rec],
                       flops=float(n * px * (4 * (2 * ℓ.radius + 1) + 12)), tag='%dx%d s%d' % (*self.x0_shape[:2], ℓ.radius))]


    def _labels_of(self, b):
        """The labels the head of block b is scored against: y, or y_sup of its map."""
        return self.y if b.lmap is None else self.y_sup[b.lmap]


    def _label_map_launches(self, n):
        """The launch at the head of every program WITH LABELS of a net with superclass heads: [mpnn_label_map] -- y to y_sup of
        every distinct map -- or [] without such a head.  By then the step's prologue has written y.  host: one record per
        map (the co-trainer concatenates the records of its nets)."""
        if not self.label_maps:
            return []
        recs = []
        for w, y_sup in zip(self.w_cls_dev, self.y_sup):
            rec = _hip.LabelMapArgs()
            rec.y, rec.w_cls, rec.y_sup = self.y.data_ptr(), w.data_ptr(), y_sup.data_ptr()
            rec.n, rec.n_cls, rec.n_sup = n, w.shape[0], w.shape[1]
            _hip.check(self.lib.mpnn_label_map_check(C.byref(rec)), 'label_map record')
            recs.append(rec)
        tab = _hip.to_device_table(recs, self.dev)
        self._keep += [recs, tab]
        return [Launch(self.lib.mpnn_label_map, 'label_map', tab.data_ptr(), len(recs), n, max(w.shape[1] for w in self.w_cls_dev), host=recs,
                       flops=float(2 * n * sum(w.numel() for w in self.w_cls_dev)),
                       tag=' '.join('%d>%d' % tuple(w.shape) for w in self.w_cls_dev))]


    def _bn_ctx(self, b, i, n, with_red=True):
        ctx = _hip.BnCtx()
        ctx.s = b.s[i].data_ptr()
        ctx.bn = _hip.act(None, b.C[i], _hip.ACT_BN_BATCH, 0, self._bn(b, i), n * b.H[i] * b.W[i])
        ctx.red = self.dred[b.sum_off[i]:].data_ptr() if with_red else None
        ctx.red_nslot = self._nslot(b, i)
        self._keep.append(ctx)
        return ctx
