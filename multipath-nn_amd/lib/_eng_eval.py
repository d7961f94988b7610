"""The evaluation programs: dense ('ev': every block on every sample, the reference's schedule) and routed (a block runs on
the samples its ancestors' routers sent to it: sample lists written on the device, a dense prefix made routed after the
fact) -- DESIGN.md section 3, "Routed evaluation" -- their label-free form ('pr': Net.predict), and the dense labelled pass in
front of the threshold curve ('ev+c': Net.exit_conf_curve)."""
import ctypes as C
import os

import torch

from lib import _hip
from lib._eng_common import Launch, _attr, head_parts


class EvalPrograms:

    def _program_ev(self, n, routed):
        """The labelled evaluation (Net.eval): see _program_fwd."""
        return self._program_fwd(n, routed, 'ev')

    def _program_pr(self, n, routed, probs=False, gate=frozenset()):
        """The LABEL-FREE evaluation (Net.predict): the launches of _program_ev -- same convs, sample lists, prefix walk
        and gather depth -- with exit records that store each head's prediction (cls / conf, the softmax row with
        `probs`) instead of reading labels, and mpnn_ev_select behind mpnn_route: by p_ev, each sample's exit, class,
        confidence and operation count (csrc/ev_select.hip).  gate: the leaf ids whose switches leave by a confidence
        threshold (see _program_fwd)."""
        return self._program_fwd(n, routed, 'pr+p' if probs else 'pr', gate)

    def _program_cv(self, n, points):
        """The DENSE LABELLED evaluation in front of the threshold curve (Engine.exit_conf_curve): the launches of the dense
        'ev' program with exit records that carry labels AND predictions (c_err / d_cor and cls / conf), then ONE
        mpnn_exit_curve launch over `points` threshold rows instead of mpnn_route and the statistics (see _program_fwd)."""
        return self._program_fwd(n, False, 'ev+c', points=points)

    def _program_fwd(self, n, routed, mode, gate=frozenset(), points=0):
        """Forward-only program in evaluation mode (BatchNorm moving averages, layer_types.py:237-238;
        hard routing pi_ev, net_types.py:127-131).

        dense : the reference's schedule -- every block on every sample (11 wavefront launches), then
                ONE mpnn_exit_ev launch for all exits and mpnn_route for p_ev / p_tr.
        routed: the reference multiplies 0/1 masks p_ev into the statistics and still evaluates every
                block densely; here a block only runs on the samples its ancestors' routers sent to it.
                Per tree depth: the block's convs gather their inputs through the block's sample list
                (mpnn_conv_fwd_args.idx/cnt: indirection in the tile loader, results land at the
                samples' own rows), then mpnn_exit_ev evaluates head + router on that list and appends
                each sample to the list of the child it is routed to (wave ballot + prefix sum, count
                on the device).  No host sync anywhere; mpnn_route at the end reads the (cleared,
                then sparsely written) r / c_err / d_cor and produces the same p_ev as the dense pass.

        gate (label-free modes): leaf ids of gateable blocks (a head AND a router: Allocation.gateable) whose switch
        leaves by a CONFIDENCE THRESHOLD instead of by its router (Net.predict(exit_conf=)).  Such a switch's exit record
        gets no child lists; behind each exit launch stands one mpnn_conf_gate launch (csrc/conf_gate.hip) with a record
        per gated switch of that launch: on the same sample list it compares the confidence the head just stored with
        gate_tau[leaf] (device memory: the values are no part of the program), rewrites the switch's router row to the
        one-hot row of the decision -- the exit, or the router's arg-max among the child blocks -- and writes the child
        lists the exit record would have written (none in the dense program or in the prefix).  The prefix walk, the
        next depth's convs, mpnn_route and mpnn_ev_select follow it unchanged: they read the decision from r by their
        own arg-max.  Ungated switches keep their records; an empty gate is the program of before, launch for launch.
        """
        lib, keep = self.lib, self._keep
        ϕ = self.net.hypers
        act_mode = _hip.ACT_BN_MOVING
        labelled, stores = mode in ('ev', 'ev+c'), mode != 'ev'       # (the exits read labels / store their predictions)
        fwd = (self._label_map_launches(n) if labelled else []) + self._lln_launches(n)
        depth = self._depths()
        # A geometry the group launch has no body for (64+ channels on 16x16 / 32x32 maps: no shipped spec has one): every
        # conv as its own mpnn_msconv_fwd launch.  That entry point takes no sample lists, so a ROUTED pass of such a net
        # runs every conv densely (d0 beyond the deepest block) and is made routed by mpnn_ev_prefix_walk alone.  A net on
        # the general kernels is not meant: mpnn_msconv_fwd_gen / _hw take the lists.
        if routed and not self._groupable() and not self.generic_convs:
            routed = 1 + max(depth.values())
        # routed = d0 >= 1: the CONVS of blocks with depth < d0 run on every sample (wavefront groups, like the dense
        # program); from depth d0 on a block's convs gather through its sample list.  Every EXIT runs on its block's list
        # (so that r / c_err / d_cor are only written where a sample reaches the node), whatever the depth.
        d0 = int(routed)
        # The dense prefix's EXITS in one launch as well (d0 >= 2): a routed pass is a chain of (conv, exit) launches per
        # depth, each exit gated by the router above it -- d0 serial exit launches for blocks whose convs run on every
        # sample anyway.  Their exits run densely in ONE launch instead; mpnn_ev_prefix_walk then clears the entries of the
        # samples that do not reach a node and writes the lists of the blocks at depth d0 (csrc/exit_ev.hip).  Same results.
        def src_of(b):
            # the nearest switch above block b and the sink of it that leads to b (None: every sample reaches b)
            child, p = b, b.parent
            while p is not None and p.router is None:
                child, p = p, p.parent
            return None if p is None else (p, p.sink_blocks.index(child))
        prefix = [b for b in self.blocks if routed and depth[id(b)] < d0]
        walk = bool(routed) and d0 >= 2 and os.environ.get('MPNN_EV_PREFIX_WALK', '1') != '0' and \
            sum(1 for b in prefix if b.has_exit) <= _hip.PREFIX_MAX and \
            sum(1 for b in self.blocks if depth[id(b)] == d0) <= _hip.PREFIX_MAX
        in_prefix = {id(b) for b in prefix} if walk else set()
        # sample lists: a block below a dynamic switch owns one; below a static node it shares its parent's
        for b in self.blocks:
            par = b.parent
            if not routed or par is None or id(b) in in_prefix:
                b.ev_list = None
            elif walk and depth[id(b)] == d0:          # (frontier: its list comes from the prefix walk)
                b.ev_list = (b.ev_idx, b.ev_cnt) if src_of(b) is not None else None
            elif par.router is not None:
                b.ev_list = (b.ev_idx, b.ev_cnt)
            else:
                b.ev_list = par.ev_list
            b.ev_conv_list = b.ev_list if (routed and depth[id(b)] >= d0) else None
        rows = lambda b: b.ev_conv_list

        # ---- exit records ----
        dyn = bool(getattr(ϕ, 'dyn_k_cpt', False))
        MS = self.max_sinks
        recs = {}
        gated = {id(b): leaf for leaf, b in self.gateable.items() if leaf in gate} if not labelled else {}
        gates = {}
        for b in self.blocks:
            if not b.has_exit:
                continue
            L1 = b.L - 1
            e = _hip.ExitEvArgs()
            e.a = _hip.act(b.s[L1], b.C[L1], act_mode, 0, self._bn(b, L1, with_sum=False), n * b.H[L1] * b.W[L1])
            e.HW, e.n = b.H[L1] * b.W[L1], n
            if b.head is not None:
                lt, _, e.loss, e.eps_ce = head_parts(b.head.layer)
                leaf = b.head.leaf_id
                e.w_head, e.b_head, e.n_cls = lt.params.w.data.data_ptr(), lt.params.b.data.data_ptr(), b.n_out
                if labelled:
                    e.y = self._labels_of(b).data_ptr()
                    e.c_err, e.d_cor = self.c_err[leaf * n:].data_ptr(), self.d_cor[leaf * n:].data_ptr()
                if stores:                               # (rows of the per-leaf prediction buffers, by capacity)
                    cap = self.n_max
                    e.cls, e.conf = self.pr_cls[leaf * cap:].data_ptr(), self.pr_conf[leaf * cap:].data_ptr()
                    if mode == 'pr+p':
                        e.p_cls, e.p_stride = self._pr_rows()[leaf * cap * self.n_cls_max:].data_ptr(), self.n_cls_max
            if b.router is not None:
                rc = b.router.comps
                l1, bn1, l2, bn2, l3 = rc[1], rc[2], rc[4], rc[5], rc[7]
                sw = b.node.switch_id
                D = lambda prm: prm.data.data_ptr()
                e.w1, e.b1, e.R, e.n_sinks, e.R2 = D(l1.params.w), D(l1.params.b), b.R, len(b.node.layer.sinks), b.R2
                e.extra_col, e.k_cpt, e.alpha_cpt = (1 if dyn else 0), self.k_cpt.data_ptr(), float(_attr(ϕ, 'α_cpt', 0.0))
                e.g1, e.be1, e.m1, e.v1 = D(bn1.params.γ), D(bn1.params.β), D(bn1.params.m_avg), D(bn1.params.v_avg)
                e.w2, e.bias2 = D(l2.params.w), D(l2.params.b)
                e.g2, e.be2, e.m2, e.v2 = D(bn2.params.γ), D(bn2.params.β), D(bn2.params.m_avg), D(bn2.params.v_avg)
                e.w3, e.bias3 = D(l3.params.w), D(l3.params.b)
                e.bn_eps, e.bn_eps2 = float(bn1.hypers.ϵ), float(bn2.hypers.ϵ)
                e.r, e.r_stride = self.r[sw * n * MS:].data_ptr(), MS
                lists = e
                if id(b) in gated:                          # (the threshold decides: the gate record carries the child lists)
                    lists = q = gates[id(b)] = _hip.ConfGateArgs()
                    leaf = gated[id(b)]
                    q.conf, q.tau = self.pr_conf[leaf * self.n_max:].data_ptr(), self.gate_tau[leaf:].data_ptr()
                    q.r, q.r_stride, q.n_sinks, q.n = e.r, e.r_stride, e.n_sinks, n
                    q.exit_sink = b.node.layer.sinks.index(b.head.layer)
                if routed and id(b) not in in_prefix:       # (a prefix exit runs on every sample: the walk writes the lists)
                    for i, sb in enumerate(b.sink_blocks):
                        if sb is not None:
                            lists.child_idx[i], lists.child_cnt[i] = sb.ev_idx.data_ptr(), sb.ev_cnt.data_ptr()
            if b.ev_list is not None:
                e.idx, e.cnt = b.ev_list[0].data_ptr(), b.ev_list[1].data_ptr()
                if id(b) in gates:
                    gates[id(b)].idx, gates[id(b)].cnt = e.idx, e.cnt
            if id(b) in gates:
                _hip.check(lib.mpnn_conf_gate_check(C.byref(gates[id(b)])), 'conf_gate record')
            if self.generic_exits:                       # (scratch maps of mpnn_exit_ev_gen)
                e.z = b.z.data_ptr() if b.head is not None else None
                e.h1 = b.h1.data_ptr() if b.router is not None else None
            if not self.generic_exits:
                _hip.check(lib.mpnn_exit_ev_check(C.byref(e)), 'exit_ev record')
            recs[id(b)] = e

        def wavefront(blocks):
            for members in self._wavefront(blocks):
                fwd.extend(self._conv_fwd_launches(members, n, 'ev', rows))

        def exits_of(blocks):
            order = [recs[id(b)] for b in blocks if id(b) in recs]
            if order:
                tab = _hip.to_device_table(order, self.dev)
                keep.append(tab)
                fwd.append(Launch(lib.mpnn_exit_ev_gen if self.generic_exits else lib.mpnn_exit_ev, 'exit_ev', tab.data_ptr(), len(order), n,
                                  host=order))
            order = [gates[id(b)] for b in blocks if id(b) in gates]
            if order:                      # (behind the exits whose conf they read, in front of every reader of r)
                tab = _hip.to_device_table(order, self.dev)
                keep.append(tab)
                fwd.append(Launch(lib.mpnn_conf_gate, 'conf_gate', tab.data_ptr(), len(order), n, host=order))

        if not routed:
            wavefront(self.blocks)
            exits_of(self.blocks)
        else:
            by_depth = {}
            for b in self.blocks:
                by_depth.setdefault(depth[id(b)], []).append(b)
            wavefront([b for b in self.blocks if depth[id(b)] < d0])
            if walk:
                exits_of(prefix)
                pa, rec_of = _hip.EvPrefixArgs(), {}
                pa.n = n
                for b in prefix:
                    if not b.has_exit:
                        continue
                    j = rec_of[id(b)] = len(rec_of)
                    src = src_of(b)
                    pa.parent[j], pa.parent_sink[j] = (-1, 0) if src is None else (rec_of[id(src[0])], src[1])
                    e = recs[id(b)]
                    if b.router is not None:
                        pa.n_sinks[j], pa.r_stride[j], pa.r[j] = e.n_sinks, e.r_stride, e.r
                    if b.head is not None and labelled:          # (label-free: nothing to clear, the answer goes by p_ev)
                        pa.c_err[j], pa.d_cor[j] = e.c_err, e.d_cor
                pa.count = len(rec_of)
                for b in self.blocks:
                    if depth[id(b)] == d0 and b.ev_list is not None:
                        f = pa.n_front
                        src = src_of(b)
                        pa.front_parent[f], pa.front_sink[f] = rec_of[id(src[0])], src[1]
                        pa.front_idx[f], pa.front_cnt[f] = b.ev_idx.data_ptr(), b.ev_cnt.data_ptr()
                        pa.n_front = f + 1
                if pa.count > 0:                   # (a prefix of static blocks only has no exit to make routed)
                    dev_pa = _hip.to_device_table([pa], self.dev)
                    keep.extend([pa, dev_pa])
                    fwd.append(Launch(lib.mpnn_ev_prefix_walk, 'ev_prefix_walk', C.byref(pa), dev_pa.data_ptr()))
            for d in sorted(by_depth):
                bs = by_depth[d]
                if walk and d < d0:
                    continue
                if d >= d0:
                    for i in range(max(b.L for b in bs)):
                        members = [(b, i) for b in bs if i < b.L]
                        # a launch holds members that all carry a list, or none (the root block: every sample)
                        for with_list in (False, True):
                            part = [(b, i) for b, i in members if (b.ev_conv_list is not None) == with_list]
                            if part:
                                fwd.extend(self._conv_fwd_launches(part, n, 'ev', rows))
                exits_of(bs)            # (the exits of one depth: their lists come from the depth above)

        if mode == 'ev+c':                  # (the curve needs neither p_ev nor the statistics: the walk reads conf, d_cor and r)
            fwd.append(self._curve_launch(n, points))
            return dict(fwd=fwd, bwd=[], n=n, mode=mode, routed=routed, gate=frozenset(), points=points)
        fwd.append(self._route_launch(n, 'ev', self.loss_ev))
        if mode != 'ev':
            fwd.append(self._select_launch(n, mode == 'pr+p'))
        return dict(fwd=fwd, bwd=[], n=n, mode=mode, routed=routed, gate=frozenset(gated.values()))

    def _curve_buffers(self, points):
        """The device side of one curve of `points` threshold rows: the thresholds [points, leaves], the pinned ring they are
        uploaded through, and the accumulators int64 [points, 2 + leaves] (correct | ops | hist) -- kept per number of
        points, so that a program (and its graph) for that many points holds their addresses for good."""
        bufs = self._curve_bufs.get(points)
        if bufs is None:
            from lib._upload import UploadRing
            nl = len(self.leaves)
            bufs = self._curve_bufs[points] = (torch.zeros(points, nl, device=self.dev), UploadRing(2, (points, nl)),
                                               torch.zeros(points * (2 + nl), dtype=torch.int64, device=self.dev))
        return bufs

    def _curve_launch(self, n, points):
        taus, _, acc = self._curve_buffers(points)
        nl, MS = len(self.leaves), self.max_sinks
        ca = _hip.ExitCurveArgs()
        ca.n, ca.n_nodes, ca.n_leaves, ca.n_switches, ca.n_points, ca.tau_per_leaf = n, len(self.nodes), nl, len(self.switches), points, 1
        ca.tree, ca.node_ops = self.curve_tree_dev.data_ptr(), self.node_ops_i64.data_ptr()
        ca.conf, ca.conf_stride = self.pr_conf.data_ptr(), self.n_max
        ca.d_cor, ca.dcor_stride = self.d_cor.data_ptr(), n
        ca.r, ca.r_stride, ca.r_switch_stride = self.r.data_ptr(), MS, n * MS
        ca.taus = taus.data_ptr()
        ca.correct, ca.ops, ca.hist = acc.data_ptr(), acc[points:].data_ptr(), acc[2 * points:].data_ptr()
        _hip.check(self.lib.mpnn_exit_curve_check(C.byref(ca), self.curve_tree), 'exit_curve record')
        self._keep.append(ca)
        return Launch(self.lib.mpnn_exit_curve, 'exit_curve', C.byref(ca), host=ca)

    def _pr_rows(self):
        """The per-leaf softmax rows of predict(probs=True): [leaves][capacity][n_cls] floats (4 x leaves x capacity x n_cls
        bytes: 1.3 MB for the 8-exit chain at 4 096 samples and 10 classes), allocated on the first call that asks.  n_cls:
        the widest head's.  An exit writes the first entries of its rows, as many as its own label space has; the rest
        stay at the zero they are allocated with (here and again when _ensure_capacity dropped the buffers)."""
        if self.pr_p is None:
            self.pr_p = torch.zeros(len(self.leaves) * self.n_max * self.n_cls_max, device=self.dev)
            self.pr_probs = torch.zeros(self.n_max, self.n_cls_max, device=self.dev)
        return self.pr_p

    def _select_launch(self, n, probs):
        sa = _hip.EvSelectArgs()
        sa.n, sa.n_nodes, sa.n_leaves, sa.n_cls = n, len(self.nodes), len(self.leaves), self.n_cls_max
        sa.p_ev, sa.node_ops, sa.leaf_node = self.p_ev.data_ptr(), self.node_ops_i64.data_ptr(), self.leaf_node_tab.data_ptr()
        sa.leaf_cls, sa.leaf_conf, sa.leaf_stride = self.pr_cls.data_ptr(), self.pr_conf.data_ptr(), self.n_max
        if probs:
            sa.leaf_p, sa.p_stride, sa.probs = self._pr_rows().data_ptr(), self.n_cls_max, self.pr_probs.data_ptr()
        sa.leaf, sa.cls, sa.conf, sa.ops = (t.data_ptr() for t in (self.res_leaf, self.res_cls, self.res_conf, self.res_ops))
        self._keep.append(sa)
        return Launch(self.lib.mpnn_ev_select, 'ev_select', C.byref(sa), host=sa)
