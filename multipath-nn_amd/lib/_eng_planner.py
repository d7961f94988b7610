"""The training program of a net: the launch lists of one step ('tr') -- forward wavefront groups, exit path, backward
dependency levels with their workgroup budgets, the finishing launch -- built once per (batch, planner settings) and
cached.  The backward pass is decided first, as host data (`_bwd_plan`: groups and budgets, splits,
slab layout, who writes a shared map, the data-parallel cut), and its records are then built from that plan with their final
pointers (`_bwd_launches`); the plan stays in the program under 'bwd_plan'.  `program(mode, n, routed, gate, points)` is the
entry point; evaluation programs: lib/_eng_eval.py."""
import ctypes as C
import functools
import os

import numpy as np
import torch

from lib import _hip
from lib._eng_common import Launch, _attr, dropout_seed, dropout_thresh, head_activity, head_parts


class Planner:

    def _wsplit(self, b, i, n, fused=False):
        """Workgroups the pixel range of a wgrad launch is divided over."""
        H = b.H[i]
        tiles = n * (H // 16) * (H // 4) if H >= 16 else (n if H == 8 else (n + 3) // 4)
        nch = (b.Cin[i] + 15) // 16 + ((b.C[i - 1] + 15) // 16 if i > 0 else 0)
        groups = max(1, b.C[i] // 64) if b.C[i] % 64 == 0 else (b.C[i] // 32 if b.C[i] % 32 == 0 else b.C[i] // 16)
        if fused:
            groups = b.C[i] // 64 if b.C[i] % 64 == 0 else b.C[i] // 16    # as mpnn_msconv_bwd_scale
        budget = 512
        if fused:
            # about half of the workgroups that are resident at once: the dgrad bodies of the same
            # launch take the rest, and everything starts together
            has_dgrad = 1 if (b.in_map is not None or i > 0) else 0
            dg_items = tiles * ((b.parent.C[b.in_map[i]] // 16 if b.parent is not None else 0) + (b.C[i - 1] // 16 if i > 0 else 0))
            slots = self.lib.mpnn_msconv_bwd_scale_slots(b.H[i], b.W[i], b.C[i], has_dgrad, 1 if i > 0 else 0, dg_items)
            if slots > 0:
                budget = min(budget, slots // 2 if has_dgrad else slots)      # (a third / a quarter: measured slower)
                if has_dgrad and b.C[i] % 64 == 0 and dg_items > slots // 3:
                    # a 64-channel layer with three workgroups per CU: the input-gradient bodies get one workgroup
                    # per (tile, row) if that fits, the weight gradients the rest
                    budget = min(budget, max(slots - dg_items, slots // 4))
        want = max(1, budget // (nch * groups))
        want = min(want, max(1, (12 << 20) // self._w_bytes(b, i)))       # keep a layer's slab under ~12 MB
        want = max(1, min(tiles, want))
        return self._xcd_round(want)


    @staticmethod
    def _w_bytes(b, i):
        """Bytes of the weights of conv (b, i): w_horz_i and w_vert_{i-1}."""
        (kh, kw), (kvh, kvw) = b.kh[i], b.kv[i] or (0, 0)
        return 4 * b.C[i] * (kh * kw * b.Cin[i] + (kvh * kvw * b.C[i - 1] if i > 0 else 0))


    def _wsplit_gen(self, b, i, n):
        """Pixel split of a general weight-gradient launch (csrc/conv_gen.hip: one workgroup per split, operand chunk -- 16
        channels, the last one partly filled where C % 16 != 0 --, tap row and 64 output channels): about 512 workgroups, at least two splits (the gradients then come out of a slab, and
        the fused finishing launch exists for every net), the slab under ~12 MB."""
        (kh, _), (kvh, _) = b.kh[i], b.kv[i] or (0, 0)
        items = (b.Cin[i] + 15) // 16 * kh + ((b.C[i - 1] + 15) // 16 * kvh if i > 0 else 0)
        want = max(1, 512 // (items * ((b.C[i] + 63) // 64)))
        tiles = self.lib.mpnn_msconv_hw_tiles if self.anymap_convs else self.lib.mpnn_msconv_gen_tiles
        want = min(want, tiles(n, b.H[i], b.W[i]), max(1, (12 << 20) // self._w_bytes(b, i)))
        return max(2, want)


    def _gen_fn(self, name):
        """Entry point `name` of a net on the general kernels: the _gen form, the any-map _hw form or the any-channel _ch
        form (same records)."""
        return getattr(self.lib, 'mpnn_msconv_%s_%s' % (name, 'ch' if self.anychan_convs else 'hw' if self.anymap_convs else 'gen'))


    @staticmethod
    def _xcd_round(g):
        """Workgroups per row of an XCD-aware launch (conv_kernel.h, ConvP::xcd): a multiple of 8 from 16 on."""
        return (g // 8) * 8 if g >= 16 else g


    # ------------------------------------------------------------------ backward schedule
    def _bwd_deps(self, b, i):
        """(block, scale) triples B(.) that must have run before B(b, i) = {dgrad-horz, dgrad-vert, weight gradients
        of g(b, i)}: the coarser scale of the block (its dgrad-vert turns dz(b, i) into g(b, i)), the child blocks'
        launches at this scale (their dgrad-horz writes dz(b, i)), and -- because the dgrad-vert of B(b, i) converts
        dz(b, i-1) into g(b, i-1) IN PLACE -- the child blocks' launches at the finer scale as well."""
        deps = []
        if i < b.L - 1:
            deps.append((b, i + 1))
        for c in b.children:
            for j, src in enumerate(c.in_map):
                if src == i or (src == i - 1 and i > 0 and b.has_dz[i - 1]):
                    deps.append((c, j))
        return deps


    def _bwd_schedule(self, order, n):
        """Launch groups of the backward pass: [[((kb, b, i), budget), ...], ...] in execution order.  Triples of one
        dependency level run as ONE launch (mpnn_msconv_bwd_level) when a kernel variant covers their shapes, they
        write different maps (tree nets: siblings accumulate into one parent map -> consecutive launches) and there
        are at most MPNN_BWD_LEVEL_MAX of them; budget = workgroups of each body (None: a plain mpnn_msconv_bwd_scale
        launch, which sizes itself)."""
        level = {}
        for kb, b, i in order:                               # (a topological order)
            level[(id(b), i)] = 1 + max([level[(id(d), j)] for d, j in self._bwd_deps(b, i)], default=-1)
        by_level = {}
        for m in order:
            by_level.setdefault(level[(id(m[1]), m[2])], []).append(m)
        groups = []
        for d in sorted(by_level):
            pend = list(by_level[d])
            while pend:
                grp, targets, rest = [], set(), []
                for m in pend:
                    kb, b, i = m
                    tgt = (id(b.parent), b.in_map[i]) if b.parent is not None else None
                    if len(grp) < _hip.BWD_LEVEL_MAX and (tgt is None or tgt not in targets):
                        grp.append(m)
                        targets.add(tgt)
                    else:
                        rest.append(m)
                pend = rest
                bud = self._level_budget(grp, n) if (len(grp) > 1 or self.co_share > 1) else None
                if bud is None and self.co_share > 1 and len(grp) > 1:
                    # (the members do not fit slots / co_share together: one table-driven launch each)
                    buds = [self._level_budget([m], n) for m in grp]
                    if any(b is None for b in buds):
                        raise NotImplementedError('co-training %d nets: a backward launch does not fit the resident slots' % self.co_share)
                    groups += [[(m, b[0])] for m, b in zip(grp, buds)]
                elif bud is None and self.co_share > 1:
                    raise NotImplementedError('co-training %d nets: a backward launch does not fit the resident slots' % self.co_share)
                elif bud is None:
                    groups += [[(m, None)] for m in grp]
                else:
                    groups.append(list(zip(grp, bud)))
        return groups


    # Budget model of a level launch: relative latency of one work item of a body (a dgrad unit = a 16-channel chunk
    # of g for one 64-pixel tile and one 16-channel output row; a weight-gradient tile), from the phase traces
    # (profiles/) and a sweep of the step time (profiles/r03_knob_sweep.txt): dgrad-vert units carry the max-pool /
    # BatchNorm-backward epilogue, a 16-channel weight-gradient tile is cheaper than a dgrad unit (nine-tap
    # accumulation, lean staging), 64-channel groups have four times its MFMAs.
    _LAT = dict(h=1.0, v=1.4, w1=0.75, w4=2.6)

    # co-trained groups (throughput-bound launches; swept at K = 8: w4 2.6 -> 2 086 us per joint step, 3.4 -> 2 067, 4.5 -> 2 090)
    _LAT_CO = dict(h=1.0, v=1.4, w1=0.75, w4=3.4)


    def _level_budget(self, grp, n):
        """Workgroups of every body of a level launch: the assignment that minimises the longest serial chain
        (items per workgroup x item latency) over all bodies with everything resident at once -- small members get
        (nearly) one item per workgroup, the large member the rest.  None: no kernel variant covers the shapes."""
        lib = self.lib
        LAT = self._LAT if self.co_share == 1 else self._LAT_CO
        H = (C.c_int * len(grp))(*[b.H[i] for _, b, i in grp])
        W = (C.c_int * len(grp))(*[b.W[i] for _, b, i in grp])
        Co = (C.c_int * len(grp))(*[b.C[i] for _, b, i in grp])
        slots = lib.mpnn_msconv_bwd_level_slots(H, W, Co, len(grp))
        if slots <= 0:
            return None
        slots //= self.co_share
        bodies = []                                          # (member, kind, rows, tiles, latency per item)
        for k, (kb, b, i) in enumerate(grp):
            tiles = lib.mpnn_wgrad_tiles(n, b.H[i], b.W[i])
            units = b.C[i] // 16
            if b.parent is not None:
                bodies.append((k, 'h', b.parent.C[b.in_map[i]] // 16, tiles, LAT['h'] * units))
            if i > 0:
                bodies.append((k, 'v', b.C[i - 1] // 16, tiles, LAT['v'] * units))
            ot = 4 if b.C[i] % 64 == 0 else 1
            nch = (b.Cin[i] + 15) // 16 + ((b.C[i - 1] + 15) // 16 if i > 0 else 0)
            bodies.append((k, 'w', nch * (b.C[i] // (16 * ot)), tiles, LAT['w%d' % ot]))
        if sum(rows for _, _, rows, _, _ in bodies) > slots:
            return None

        def fit(T):                                          # workgroups per row of each body for a chain of at most T
            gx = []
            for _, _, rows, tiles, lat in bodies:
                per = int(T / lat + 1e-9)
                if per < 1:
                    return None
                gx.append(-(-tiles // per))
            return gx if sum(g * body[2] for g, body in zip(gx, bodies)) <= slots else None
        cands = sorted({lat * j for _, _, _, tiles, lat in bodies for j in range(1, tiles + 1)})
        lo, hi = 0, len(cands) - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if fit(cands[mid]) is not None:
                hi = mid
            else:
                lo = mid + 1
        gx = fit(cands[lo])
        if gx is None:
            return None
        # left-over slots: to the bodies with the longest chain
        used = sum(g * body[2] for g, body in zip(gx, bodies))
        while True:
            cand = [q for q in range(len(gx)) if gx[q] < bodies[q][3] and used + bodies[q][2] <= slots]
            if not cand:
                break
            q = max(cand, key=lambda q: -(-bodies[q][3] // gx[q]) * bodies[q][4])
            gx[q] += 1
            used += bodies[q][2]
        if os.environ.get('MPNN_PLAN_DEBUG'):
            print('level budget: %d slots, chain %.1f; ' % (slots, cands[lo]) + '; '.join(
                'm%d %s rows %d tiles %d -> gx %d (%d wgs, %d items/wg)' % (k, kind, rows, tiles, g, g * rows, -(-tiles // g))
                for (k, kind, rows, tiles, lat), g in zip(bodies, gx)))
        out = [dict(gxh=0, gxv=0, split=1) for _ in grp]
        for (k, kind, rows, tiles, lat), g in zip(bodies, gx):
            if self.co_share == 1:              # (co-trained groups: no XCD-aware order, no rounding of slots / K: see conv_fwd.hip)
                g = self._xcd_round(g)
            if kind == 'w':
                kb, b, i = grp[k]
                g = max(1, min(g, max(1, (12 << 20) // self._w_bytes(b, i))))      # keep a layer's slab under ~12 MB
            out[k]['gxh' if kind == 'h' else 'gxv' if kind == 'v' else 'split'] = int(g)
        return out


    def program(self, mode, n, routed=False, gate=frozenset(), points=0):
        """Launch lists of one (mode, batch size).  routed ('ev' only): the routed evaluation -- every
        block runs on the sample list its parent's router produced on the device (see _program_ev).  gate ('pr' / 'pr+p'
        only): the leaf ids whose switches leave by a confidence threshold (_program_fwd); the thresholds' VALUES are no
        part of a program.  points ('ev+c' only: the dense labelled pass in front of mpnn_exit_curve, _program_cv): the
        number of threshold rows of the curve."""
        try:
            return self._program(mode, n, routed, frozenset(gate), int(points))
        finally:
            self.lib.mpnn_set_reserved_cus(0)      # (a data-parallel training program is built with a reservation in place)


    def routed_prefix(self, n):
        """Depth from which the routed evaluation gathers (>= 1; see _program_ev).  The blocks above it run on every
        sample in wavefront-grouped launches: early blocks lose few samples, so routing them saves little work and
        costs the block-serial schedule (one launch per scale, then the exit, per block) -- which is what made the
        fully routed program slower than the dense one below ~2 000 samples (profiles/r04_eval_sweep.txt).  Nets on the
        general conv kernels have a table of their own (_ROUTED_PREFIX_GEN)."""
        table = self._ROUTED_PREFIX_GEN if self.generic_convs else self._ROUTED_PREFIX
        for lim, d0 in table:
            if n >= lim:
                return d0
        return table[-1][1]

    _ROUTED_PREFIX = ((6144, 1), (3072, 2), (1536, 3), (640, 4), (0, 6))     # (re-swept with the prefix walk: profiles/r05_eval_prefix_sweep.txt)
    # A net on the general conv kernels (one tile per workgroup, a launch per conv in the dense program as well): gathering
    # from depth 1 is the fastest routed program at every batch from 256 to 8 192 (profiles/gen_routed_eval_sweep.txt)
    _ROUTED_PREFIX_GEN = ((0, 1),)


    def _program(self, mode, n, routed, gate=frozenset(), points=0):
        # routed='auto': routed above ROUTED_MIN_BATCH samples, dense below (the routed schedule is block-serial --
        # 28 launches against 13 -- and only pays once the launches are throughput-bound; profiles/r03_eval_sweep.txt).
        # A net on the general conv kernels has a threshold of its own (at 256 samples the routed program of the
        # conv_supp = 5 chain is 1.2 % slower than the dense one, from 512 on it is faster: profiles/gen_routed_eval_sweep.txt)
        if routed == 'auto':
            routed = n >= (self.routed_min_batch_gen if self.generic_convs else self.routed_min_batch)
        explicit = routed if (isinstance(routed, int) and not isinstance(routed, bool) and routed >= 1) else None
        routed = bool(routed) and mode != 'tr' and bool(self.switches) and self.net._net_kind != 'sr'
        if routed:                                   # (an int >= 1: blocks of a smaller depth run on every sample)
            routed = explicit if explicit is not None else self.routed_prefix(n)
        if mode == 'tr' and self.allreduce is not None and self.multi_stream:
            # one section would fork and re-join the same side streams twice inside one capture (ROCm 7.2 crashes in
            # hipStreamEndCapture), and the DAG schedule has no bucket boundaries to overlap the collectives with
            raise NotImplementedError('data-parallel training runs on the single-stream schedule (MPNN_STREAMS=0)')
        dp = mode == 'tr' and self.allreduce is not None
        reserve = self.dp_reserve_cus if (dp and len(self.dp_buckets) > 1) else 0
        key = (mode, n, self.multi_stream, self.group_fwd, routed, dp, self.bwd_levels, self.fold_clear, reserve, self.fuse_opt, self.co_share, gate) + \
            ((points,) if mode == 'ev+c' else ())
        if key in self._progs:
            return self._progs[key]
        self._ensure_capacity(n, mode == 'tr')
        if mode != 'tr':
            prog = self._progs[key] = self._program_ev(n, routed) if mode == 'ev' else self._program_cv(n, points) if mode == 'ev+c' else \
                self._program_pr(n, routed, mode == 'pr+p', gate)
            return prog
        if self.multi_stream and self.generic_convs:
            raise NotImplementedError('the multi-stream schedule has no launches for the general conv kernels (filters other '
                                      'than 3x3, maps other than the tuned squares): such nets run on the single-stream '
                                      'schedule (MPNN_STREAMS=0)')
        if self.multi_stream and any(b.drop is not None for b in self.blocks):
            raise NotImplementedError('the multi-stream schedule has no place for the Dropout launches of an exit: nets with '
                                      'Dropout (λ < 1) train on the single-stream schedule (MPNN_STREAMS=0)')
        if self.multi_stream and any(len(b.children) > 1 for b in self.blocks):
            raise NotImplementedError('the multi-stream schedule serialises nothing between sibling blocks that '
                                      'accumulate into one gradient map: tree nets run on the single-stream schedule')
        prog = self._progs[key] = self._program_tr(n, dp, reserve)
        return prog


    def _program_tr(self, n, dp, reserve):
        """The training step: forward convs, exit path and mpnn_route ('fwd'); the exits' backward, the backward conv
        launches and the launch that ends the backward pass ('bwd'), data parallel with the gradient-bucket markers."""
        # Streams: 0 = main (the 4x4 maps: the critical path through every block); 1.. = one per
        # larger map size; the last two = weight-gradient side streams (leaves of the DAG).
        sizes = sorted({h for b in self.blocks for h in b.H}, reverse=True)
        sid = {h: (0 if h == sizes[-1] else 1 + k) for k, h in enumerate(sizes)}
        self.n_streams = len(sizes) + 2
        fwd = self._label_map_launches(n) + self._lln_launches(n) + [Launch(None, 'fork')]
        # (the wavefront form also needs every root block to read the input pyramid)
        if self.group_fwd and not self.multi_stream and self._groupable() and \
                all(b.parent is not None or b.in_map is None for b in self.blocks):
            for members in self._wavefront(self.blocks):
                fwd += self._conv_fwd_launches(members, n, 'tr')
        else:
            F = lambda b, i: 'F%d_%d' % (self.blocks.index(b), i)
            for b in self.blocks:
                for i in range(b.L):
                    fwd.append(self._conv_fwd_single(b, i, n, 'tr', None, 'msconv_fwd', stream=sid[b.H[i]],
                                                     waits=[F(b, i - 1)] if i > 0 else [], records=F(b, i)))
        fwd.append(Launch(None, 'join'))
        exit_fwd, bwd, fold = self._exit_launches(n)
        fwd += exit_fwd + [self._route_launch(n, 'tr', self.loss)]
        if dp and 'exit' in self.dp_buckets:
            bwd.append(Launch(None, 'bucket', tag='exit'))      # head + router gradients are final: their all-reduce starts here
        # From here to the end of the backward pass a bucket's all-reduce runs beside the launches: their persistent
        # grids (and the workgroup budgets computed below) leave `reserve` compute units to the collective's kernels.
        self.lib.mpnn_set_reserved_cus(reserve)           # (program() resets it)
        convs, plan = self._bwd_launches(n, sid, dp, reserve, fold)
        bwd += convs
        if dp:
            bwd.append(Launch(None, 'bucket', tag='end'))
        return dict(fwd=fwd, bwd=bwd, n=n, mode='tr', fold=fold, fused_opt=plan['fused_opt'], bwd_plan=plan)


    # ------------------------------------------------------------------ forward convs (training and evaluation)
    def _conv_fwd_args(self, b, i, n, mode, rows=None):
        """The record of conv (b, i) of a step on n samples.  Training: the input's BatchNorm with batch statistics, the
        output's slot sums accumulated; evaluation: moving averages.  rows: the (index, count) sample list of a routed
        evaluation."""
        train = mode == 'tr'
        a = _hip.ConvFwdArgs()
        a.a = self._act_of_input(b, i, n, _hip.ACT_BN_BATCH if train else _hip.ACT_BN_MOVING, fwd=train)
        cp = b.conv.params
        if i > 0:
            a.v, a.Cv = b.sp[i - 1].data_ptr(), b.C[i - 1]
            a.wv_pack = getattr(cp, 'w_vert_%i' % (i - 1)).data.data_ptr() if self.generic_convs else \
                self.packs[b.pack['w_vert_%i' % (i - 1)][0]:].data_ptr()
        if i < b.L - 1:
            a.pool_out = b.sp[i].data_ptr()
        a.wa_pack = getattr(cp, 'w_horz_%i' % i).data.data_ptr() if self.generic_convs else \
            self.packs[b.pack['w_horz_%i' % i][0]:].data_ptr()
        a.bias = getattr(b.conv.params, 'b_%i' % i).data.data_ptr()
        a.out = b.s[i].data_ptr()
        a.out_sum = self.dsum[b.sum_off[i]:].data_ptr() if train else None
        a.out_nslot = self._nslot(b, i)
        a.n, a.H, a.W, a.Cout = n, b.H[i], b.W[i], b.C[i]
        if rows is not None:
            a.idx, a.cnt = rows[0].data_ptr(), rows[1].data_ptr()
        return a


    @staticmethod
    def _conv_flops(b, i, n):
        (kh, kw), (kvh, kvw) = b.kh[i], b.kv[i] or (0, 0)
        return 2.0 * n * b.H[i] * b.W[i] * b.C[i] * (kh * kw * b.Cin[i] + (kvh * kvw * b.C[i - 1] if i > 0 else 0))


    def _conv_fwd_single(self, b, i, n, mode, rows, what, **kw):
        """Conv (b, i) as a launch of its own: mpnn_msconv_fwd, or for a net on the general kernels mpnn_msconv_fwd_gen /
        mpnn_msconv_fwd_hw / mpnn_msconv_fwd_ch (the same record, sample list included)."""
        a = self._conv_fwd_args(b, i, n, mode, rows)
        self._keep.append(a)
        fl, tag = self._conv_flops(b, i, n), self._conv_tag(b, i)
        if self.generic_convs:
            return Launch(self._gen_fn('fwd'), what, C.byref(a), *b.kh[i], *(b.kv[i] or (0, 0)), flops=fl, tag=tag, **kw)
        return Launch(self.lib.mpnn_msconv_fwd, what, C.byref(a), flops=fl, tag=tag, **kw)


    @staticmethod
    def _conv_tag(b, i):
        hw = 'h%d' % b.H[i] if b.H[i] == b.W[i] else 'h%dx%d' % (b.H[i], b.W[i])
        return '%s %d+%d->%d' % (hw, b.Cin[i], b.C[i - 1] if i > 0 else 0, b.C[i])


    def _wavefront(self, blocks):
        """The forward convs of `blocks` by level of the block x scale grid: F(b, k) needs only F(b-1, k) and F(b, k-1),
        so the convs of level depth(b) + k are mutually independent.  [[(b, i), ...], ...] in level order."""
        depth = self._depths()
        kidx = {h: k for k, h in enumerate(sorted({h for b in self.blocks for h in b.H}, reverse=True))}
        levels = {}
        for b in blocks:
            for i in range(b.L):
                levels.setdefault(depth[id(b)] + kidx[b.H[i]], []).append((b, i))
        return [levels[d] for d in sorted(levels)]


    def _conv_fwd_launches(self, members, n, mode, rows=lambda b: None):
        """The launches of the mutually independent forward convs `members` [(b, i), ...]: tables of at most four records
        (mpnn_msconv_fwd_group; one net of a co-trained group: the grids it has inside the joint launches) -- or, for a
        geometry the group launch has no body for, one mpnn_msconv_fwd each.  rows(b): block b's sample list or None."""
        lib, out = self.lib, []
        if not self._groupable():
            return [self._conv_fwd_single(b, i, n, mode, rows(b), 'fwd') for b, i in members]
        for c0 in range(0, len(members), 4):
            grp = members[c0:c0 + 4]
            arr = (_hip.ConvFwdArgs * len(grp))(*[self._conv_fwd_args(b, i, n, mode, rows(b)) for b, i in grp])
            dev_arr = _hip.to_device_table(list(arr), self.dev)
            self._keep += [arr, dev_arr]
            fl, tag = sum(self._conv_flops(b, i, n) for b, i in grp), ' | '.join(self._conv_tag(b, i) for b, i in grp)
            if self.co_share > 1:
                out.append(Launch(lib.mpnn_msconv_fwd_group_rep, 'fwd_group', arr, dev_arr.data_ptr(), len(grp), 1, self.co_share,
                                  flops=fl, tag=tag, host=arr))
            else:
                out.append(Launch(lib.mpnn_msconv_fwd_group, 'fwd_group', arr, dev_arr.data_ptr(), len(grp), flops=fl, tag=tag, host=arr))
        return out


    def _depths(self):
        depth = {}
        for b in self.blocks:
            depth[id(b)] = 0 if b.parent is None else depth[id(b.parent)] + 1
        return depth


    def _groupable(self):
        """The forward convs of this architecture all have the wavefront-grouped (table-driven) launch form -- no 64+
        channel conv on a 16x16 or larger map -- so its nets can share launches in a co-trained group (lib/_co.py)."""
        return not self.generic_convs and \
            all(c % 16 == 0 and not (c % 64 == 0 and h >= 16) for b in self.blocks for c, h in zip(b.C, b.H))


    # ------------------------------------------------------------------ exits and route
    def _exit_launches(self, n):
        """The exit path of a training step: one record per block with a head or a router for each of mpnn_lin_fwd and
        mpnn_exit_tail_fwd (forward), mpnn_exit_tail_bwd and mpnn_lin_bwd (the first launches of the backward pass).
        A block whose head carries Dropout (b.drop): mpnn_dropout_fwd in front of mpnn_lin_fwd writes the dropped map xd,
        the block's lin record keeps the router alone (no router: no such record) and a second lin record runs the head on
        xd as it is; the head's dX goes to dxd, and mpnn_dropout_bwd behind mpnn_lin_bwd folds it into b.dx.
        Returns (forward launches, backward launches, fold)."""
        lib, keep = self.lib, self._keep
        act_mode = _hip.ACT_BN_BATCH
        ϕ = self.net.hypers
        dyn = bool(getattr(ϕ, 'dyn_k_cpt', False))
        lin_f, lin_b, tail_f, tail_b, drops = [], [], [], [], []
        MS = self.max_sinks
        kmax = kmax_drop = 0

        def lin_pair(a_in, HW, K):
            """The mpnn_lin_fwd / mpnn_lin_bwd records of one input map, with their split scratch; no weight set yet."""
            lf, lb = _hip.LinFwdArgs(), _hip.LinBwdArgs()
            lf.a, lb.a = a_in, a_in
            lf.HW = lb.HW = HW
            lf.n = lb.n = n
            lf.k_cpt = lb.k_cpt = self.k_cpt.data_ptr()
            lf.alpha_cpt = lb.alpha_cpt = float(_attr(ϕ, 'α_cpt', 0.0))
            if K >= 512 and n <= 512:
                # K-slices for mpnn_lin_fwd (one workgroup per 16 rows pulled all of W through one compute
                # unit); small batches only -- with thousands of rows the launch has workgroups enough
                rg = (n + 15) // 16
                kpart = torch.empty(rg * _hip.LIN_KSLICES * 512, device=self.dev)
                kcnt = torch.zeros(rg, dtype=torch.int32, device=self.dev)
                keep.extend([kpart, kcnt])
                lf.kpart, lf.kcnt = kpart.data_ptr(), kcnt.data_ptr()
            if n <= 512:
                # row split for mpnn_lin_bwd_rs: partial dW / db tiles of the row groups of a feature block
                nblk = (K + 1 + 63) // 64
                bpart = torch.empty(nblk * _hip.LIN_RSPLIT * _hip.LIN_RS_TILE, device=self.dev)
                bcnt = torch.zeros(nblk, dtype=torch.int32, device=self.dev)
                keep.extend([bpart, bcnt])
                lb.kpart, lb.kcnt = bpart.data_ptr(), bcnt.data_ptr()
            return lf, lb

        for b in self.blocks:
            if not b.has_exit:
                continue
            L1 = b.L - 1
            K = b.H[L1] * b.W[L1] * b.C[L1]
            kmax = max(kmax, K)
            tf, tb = _hip.ExitTailArgs(), _hip.ExitTailBwdArgs()
            tf.n = n
            a_in = _hip.act(b.s[L1], b.C[L1], act_mode, 0, self._bn(b, L1), n * b.H[L1] * b.W[L1])
            lf, lb = lin_pair(a_in, b.H[L1] * b.W[L1], K)
            hf, hb = lf, lb                          # the records that carry the head's weight set
            if b.drop is not None:
                # Dropout in front of the head's LinTrans: the head reads the dropped map xd, as it is, through records of
                # its own; the router keeps reading the block's map
                hf, hb = lin_pair(_hip.act(b.xd, b.C[L1], _hip.ACT_IDENTITY, 0), b.H[L1] * b.W[L1], K)
                hb.dx = b.dxd.data_ptr()
                λ = float(b.drop.hypers.λ)
                seed = dropout_seed(b.drop.hypers.seed, self.dropout_rank)
                dr = _hip.DropoutArgs()
                dr.a, dr.HW, dr.n = a_in, b.H[L1] * b.W[L1], n
                dr.seed_lo, dr.seed_hi, dr.leaf = seed & 0xFFFFFFFF, seed >> 32, b.head.leaf_id
                dr.thresh, dr.inv_keep = dropout_thresh(λ), float(np.float32(1.0 / λ))
                dr.step = self.drop_steps.data_ptr()                 # (slot 0: the one-step program; run_steps: slot j)
                dr.xd, dr.dxd, dr.dx = b.xd.data_ptr(), b.dxd.data_ptr(), b.dx.data_ptr()
                dr.accumulate = 1 if b.router is not None else 0      # (the router's record writes b.dx first)
                _hip.check(lib.mpnn_dropout_check(C.byref(dr)), 'dropout record')
                drops.append(dr)
                kmax_drop = max(kmax_drop, K)
            lb.dx = b.dx.data_ptr()
            if not b.children and not self.multi_stream and not self.generic_exits and b.drop is None:
                # the exit's dX is the only gradient of this map: lin_bwd masks it and accumulates the
                # BatchNorm-backward reductions itself (no mpnn_bn_bwd_reduce launch)
                lb.dx = None
                lb.dz_out = b.dzg[L1].data_ptr()
                lb.red_out = self.dred[b.sum_off[L1]:].data_ptr()
                lb.red_nslot = self._nslot(b, L1)
            tf.mode = act_mode
            if b.head is not None:
                lt, _, tf.loss, tf.eps_ce = head_parts(b.head.layer)
                hf.w[0], hf.b[0], hf.y[0], hf.M[0] = lt.params.w.data.data_ptr(), lt.params.b.data.data_ptr(), b.z.data_ptr(), b.n_out
                hb.w[0], hb.dy[0], hb.M[0] = hf.w[0], b.dzh.data_ptr(), b.n_out
                hb.dw[0], hb.db[0] = lt.params.w.grad.data_ptr(), lt.params.b.grad.data_ptr()
                leaf = b.head.leaf_id
                tf.z, tf.y, tf.n_cls = b.z.data_ptr(), self._labels_of(b).data_ptr(), b.n_out
                tf.c_err = self.c_err[leaf * n:].data_ptr()
                tf.d_cor = self.d_cor[leaf * n:].data_ptr()
                tb.w_cerr = self.w_cerr[leaf * n:].data_ptr()
                tb.dz = b.dzh.data_ptr()
                # ActivityError in the head chain: backward only -- the map's term in lin_bwd's dX, the logits' and the
                # probabilities' in the tail's dz, each weighted with the leaf's w_cerr (no launch of its own)
                hb.act_alpha, tb.act_z, tb.act_p = head_activity(b.head.layer)
                if hb.act_alpha:
                    hb.act_w = tb.w_cerr
            if b.router is not None:
                rc = b.router.comps
                l1, bn1, l2, bn2, l3 = rc[1], rc[2], rc[4], rc[5], rc[7]
                R, S = b.R, len(b.node.layer.sinks)
                sw = b.node.switch_id
                lf.w[1], lf.b[1], lf.y[1], lf.M[1] = l1.params.w.data.data_ptr(), l1.params.b.data.data_ptr(), b.h1.data_ptr(), R
                lb.w[1], lb.dy[1], lb.M[1] = lf.w[1], b.dh1.data_ptr(), R
                lb.dw[1], lb.db[1] = l1.params.w.grad.data_ptr(), l1.params.b.grad.data_ptr()
                lf.extra_col[1] = lb.extra_col[1] = 1 if dyn else 0
                tf.h1, tf.R, tf.n_sinks, tf.R2 = b.h1.data_ptr(), R, S, b.R2
                tf.g1, tf.b1 = bn1.params.γ.data.data_ptr(), bn1.params.β.data.data_ptr()
                tf.m1, tf.v1 = bn1.params.m_avg.data.data_ptr(), bn1.params.v_avg.data.data_ptr()
                tf.w2, tf.bias2 = l2.params.w.data.data_ptr(), l2.params.b.data.data_ptr()
                tf.g2, tf.b2 = bn2.params.γ.data.data_ptr(), bn2.params.β.data.data_ptr()
                tf.m2, tf.v2 = bn2.params.m_avg.data.data_ptr(), bn2.params.v_avg.data.data_ptr()
                tf.w3, tf.bias3 = l3.params.w.data.data_ptr(), l3.params.b.data.data_ptr()
                tf.h2 = b.h2.data_ptr()
                tf.r, tf.r_stride = self.r[sw * n * MS:].data_ptr(), MS
                tf.bn_save = b.bn_save.data_ptr()
                tf.bn_eps, tf.bn_decay = float(bn1.hypers.ϵ), float(bn1.hypers.d)
                tf.bn_eps2, tf.bn_decay2 = float(bn2.hypers.ϵ), float(bn2.hypers.d)
                tb.dr = self.dr[sw * n * MS:].data_ptr()
                tb.dh1 = b.dh1.data_ptr()
                if getattr(b, 'dh2', None) is not None:
                    tb.dh2 = b.dh2.data_ptr()
                tb.dg1, tb.db1 = bn1.params.γ.grad.data_ptr(), bn1.params.β.grad.data_ptr()
                tb.dw2, tb.dbias2 = l2.params.w.grad.data_ptr(), l2.params.b.grad.data_ptr()
                tb.dg2, tb.db2 = bn2.params.γ.grad.data_ptr(), bn2.params.β.grad.data_ptr()
                tb.dw3, tb.dbias3 = l3.params.w.grad.data_ptr(), l3.params.b.grad.data_ptr()
            tb.f = tf
            tail_f.append(tf); tail_b.append(tb)
            if b.drop is None or b.router is not None:
                lin_f.append(lf); lin_b.append(lb)
            if b.drop is not None:
                lin_f.append(hf); lin_b.append(hb)
        n_exit, n_lin = len(tail_f), len(lin_f)
        # A training step without a clearing launch: the slot sums are cleared by their last reader (the launch that
        # ends the backward pass), the accumulators of mpnn_route by the launch before it (see run()).
        fold = n_exit > 0 and self.fold_clear
        if not n_exit:
            return [], [], fold
        if fold:
            tail_f[0].clear_f, tail_f[0].n_clear_f = self.node_stat.data_ptr(), self.node_stat.numel()
            tail_f[0].clear_d, tail_f[0].n_clear_d = self.loss.data_ptr(), self.loss.numel()
        t_lf, t_lb = _hip.to_device_table(lin_f, self.dev), _hip.to_device_table(lin_b, self.dev)
        t_tf, t_tb = _hip.to_device_table(tail_f, self.dev), _hip.to_device_table(tail_b, self.dev)
        keep += [t_lf, t_lb, t_tf, t_tb]
        if self.generic_exits:
            lin_fwd = Launch(lib.mpnn_lin_fwd_gen, 'lin_fwd', t_lf.data_ptr(), n_lin, n, host=lin_f)
        elif n <= 512:
            lin_fwd = Launch(lib.mpnn_lin_fwd_ks, 'lin_fwd', t_lf.data_ptr(), n_lin, n, kmax, host=lin_f)
        else:
            lin_fwd = Launch(lib.mpnn_lin_fwd, 'lin_fwd', t_lf.data_ptr(), n_lin, n, host=lin_f)
        # batches beyond the 128 samples the LDS-resident tails hold: the any-width tails (csrc/exit_gen.hip: every pass on
        # 1 024 threads) instead of the tuned kernels' any-size forms -- same records; measured at 256 / 512 / 1 024
        # samples: profiles/r05_train_sweep.txt
        gen_tails = self.generic_exits or n > 128
        lin_bwd = lib.mpnn_lin_bwd_gen if self.generic_exits else lib.mpnn_lin_bwd_rs if n <= 512 else lib.mpnn_lin_bwd
        fwd = [lin_fwd, Launch(lib.mpnn_exit_tail_fwd_gen if gen_tails else lib.mpnn_exit_tail_fwd, 'exit_tail_fwd',
                               t_tf.data_ptr(), n_exit, n, host=tail_f)]
        bwd = [Launch(lib.mpnn_exit_tail_bwd_gen if gen_tails else lib.mpnn_exit_tail_bwd, 'exit_tail_bwd', t_tb.data_ptr(), n_exit, n,
                      host=tail_b),
               Launch(lin_bwd, 'lin_bwd', t_lb.data_ptr(), n_lin, n, kmax, host=lin_b)]
        if drops:
            # one table for both launches: a record holds the forward and the backward half of its exit
            t_dr = _hip.to_device_table(drops, self.dev)
            keep += [drops, t_dr]
            tag = ' '.join('leaf%d' % d.leaf for d in drops)
            fwd.insert(0, Launch(lib.mpnn_dropout_fwd, 'dropout_fwd', t_dr.data_ptr(), len(drops), n, kmax_drop, host=drops, tag=tag))
            bwd.append(Launch(lib.mpnn_dropout_bwd, 'dropout_bwd', t_dr.data_ptr(), len(drops), n, kmax_drop, host=drops, tag=tag))
        return fwd, bwd, fold


    def _route_launch(self, n, mode, loss):
        """mpnn_route: routing probabilities, per-sample costs and the loss sums (training: the routers' gradients too)."""
        ϕ, kind = self.net.hypers, self.net._net_kind
        ra = _hip.RouteArgs()
        ra.net_type = {'sr': _hip.NET_SR, 'actor': _hip.NET_ACTOR, 'critic': _hip.NET_CRITIC}[kind]
        ra.n_nodes, ra.n_leaves, ra.n_switches, ra.max_sinks = len(self.nodes), len(self.leaves), len(self.switches), self.max_sinks
        ra.optimistic = int(bool(getattr(ϕ, 'optimistic', False)))
        ra.use_cls_err = int(bool(getattr(ϕ, 'use_cls_err', False)))
        ra.want_grad = 1 if mode == 'tr' else 0
        ra.nodes, ra.sw_children, ra.node_ops = self.node_tab.data_ptr(), self.kid_tab.data_ptr(), self.node_ops.data_ptr()
        ra.hyp = self.hyp.data_ptr()
        ra.k_cpt_vec = self.k_cpt.data_ptr() if bool(getattr(ϕ, 'dyn_k_cpt', False)) else None
        ra.r, ra.c_err, ra.d_cor = self.r.data_ptr(), self.c_err.data_ptr(), self.d_cor.data_ptr()
        ra.p_tr, ra.p_ev, ra.w_cerr, ra.dr = self.p_tr.data_ptr(), self.p_ev.data_ptr(), self.w_cerr.data_ptr(), self.dr.data_ptr()
        ra.node_stat = self.node_stat.data_ptr() if mode == 'tr' else None
        if mode == 'tr':
            # more than two workgroups (trees at 128 samples, chains beyond): per-workgroup partial sums + a last-arriver sum in
            # workgroup order instead of fp32 atomics -- the TALR statistics are the same bits from run to run
            need = (n + 15) // 16 * (len(self.nodes) * 2 + 8)          # (+ 4 doubles per workgroup: the loss sums)
            if self._stat_part is None or self._stat_part.numel() < need:
                self._stat_part = torch.zeros(need, device=self.dev)
                self._stat_ticket = torch.zeros(4, dtype=torch.int32, device=self.dev)
            ra.stat_part, ra.stat_ticket = self._stat_part.data_ptr(), self._stat_ticket.data_ptr()
            self._keep += [self._stat_part, self._stat_ticket]
        ra.loss = loss.data_ptr()
        ra.n, ra.n_total = n, n
        self._keep.append(ra)
        return Launch(self.lib.mpnn_route, 'route', C.byref(ra), host=ra)


    # ------------------------------------------------------------------ backward pass
    def _bwd_plan(self, n, dp):
        """Everything the backward pass of a step on n samples decides, as plain data (no torch, no device pointer; of the
        device only the resident-slot counts of the two *_slots entry points, under the reservation in force).  Triples are
        named (kb, i): block kb of reversed(self.blocks), scale i.
          groups        single-stream: the launch groups in execution order, [[(kb, i, budget), ...], ...] -- budget: the
                        workgroups of a level launch's bodies (_level_budget) or None (a launch that sizes itself);
          launches      multi-stream: [(kind, kb, i), ...], kind 'vert' / 'horz' / 'wgrad', in launch order;
          triples       (kb, i) -> split, split_stride (of the weight-gradient launch), slab ({'dwa' / 'dwv' / 'db': offset in
                        the slab buffer} or None: straight into G), accumulate and dy_extra (of the dgrad-horz record; None
                        without a parent block) -- in the order the slabs are laid out;
          slab_size     floats of the slab buffer;
          items         the table of mpnn_slab_reduce [items][6], the data-parallel cut blocks' items first: n_cut of them;
          item_seg      the optimizer row of every item [items][SEG_INTS];
          slab_params   p.offset of the parameters whose gradient leaves a slab;
          mid_after     the group behind which the 'mid' bucket marker goes (None: no marker), mid_reduce: with an
                        mpnn_slab_reduce of the first n_cut items in front of it;
          fused_opt     the launch that ends the backward pass applies the update as well."""
        rev = list(reversed(self.blocks))
        cut_kb = self.dp_cut_block if dp else None
        plan = dict(groups=None, launches=None, mid_after=None)
        if not self.multi_stream:
            # One launch per (block, scale) -- dgrad-horz, dgrad-vert (which produces g(b,i-1)) and the weight
            # gradients of g(b,i) -- or, with bwd_levels, one launch per DEPENDENCY LEVEL of those triples
            # (_bwd_schedule): the reversed block order with scales coarsest first is a topological order.
            order = [(kb, b, i) for kb, b in enumerate(rev) for i in range(b.L - 1, -1, -1)]
            # (nets on the general kernels: one set of launches per triple, in this order -- no level tables)
            groups = self._bwd_schedule(order, n) if (self.bwd_levels and not self.generic_convs) else [[(m, None)] for m in order]
            plan['groups'] = [[(kb, i, bud) for (kb, b, i), bud in grp] for grp in groups]
            walk = [(kb, i, None if bud is None else bud['split']) for grp in plan['groups'] for kb, i, bud in grp]
            if cut_kb is not None:
                plan['mid_after'] = max(g for g, grp in enumerate(plan['groups']) for kb, i, _ in grp if kb <= cut_kb)
        else:
            plan['launches'] = [(kind, kb, i) for kb, b in enumerate(rev) for kind, scales in
                                (('vert', range(b.L - 1, 0, -1)), ('horz', range(b.L if b.parent is not None else 0)), ('wgrad', range(b.L)))
                                for i in scales]
            walk = [(kb, i, None) for kb, b in enumerate(rev) for i in range(b.L)]
        triples, members, written, slab_size = {}, [], set(), 0     # members: (is_cut_block, table rows, optimizer rows, parameters)
        for kb, i, split in walk:
            b = rev[kb]
            t = triples[(kb, i)] = dict(accumulate=None, dy_extra=None, slab=None, split_stride=0)
            if b.parent is not None:
                # a map that feeds several child blocks (tree nets): the first child to run writes it
                # (with the exit's dX), the others add their masked share
                pb, j = b.parent, b.in_map[i]
                first = (id(pb), j) not in written
                written.add((id(pb), j))
                t['accumulate'] = 0 if first else 1
                t['dy_extra'] = bool(first and pb.has_exit and j == pb.L - 1)
            if split is None:
                split = self._wsplit_gen(b, i, n) if self.generic_convs else self._wsplit(b, i, n, fused=not self.multi_stream)
            t['split'] = split
            if split == 1:
                continue
            cp = b.conv.params
            prms = [('dwa', getattr(cp, 'w_horz_%i' % i))] + ([('dwv', getattr(cp, 'w_vert_%i' % (i - 1)))] if i > 0 else []) + \
                [('db', getattr(cp, 'b_%i' % i))]
            prms = [(field, prm, prm.size) for field, prm in prms]
            stride = t['split_stride'] = (sum(sz for _, _, sz in prms) + 3) // 4 * 4
            t['slab'], off, rows, srows = {}, slab_size, [], []
            slab_size += split * stride
            for field, prm, sz in prms:
                t['slab'][field] = off
                item = _hip.slab_item_size(split)
                l2b, eqo, pk = self._opt_info[id(prm)]
                if pk[1] and pk[1] % 4 == 0:
                    # a weight tensor [9 * Cin][Cout]: items of whole 4-row groups, so that the update applied by
                    # the item's workgroup (mpnn_backward_finish_opt) can write the weight packs as contiguous runs
                    item = min(_hip.SLAB_ITEM, max(item, 4 * pk[2]))
                for k in range(0, sz, item):
                    cnt = min(item, sz - k)
                    rows += [off + k, prm.offset + k, cnt, split, stride, 0]
                    srows += [prm.offset + k, cnt, prm.node, prm.is_router, l2b, eqo + k if eqo >= 0 else -1,
                              pk[0], pk[1], pk[2], pk[3], pk[4], 0]
                off += sz
            members.append((cut_kb is not None and kb <= cut_kb, rows, srows, [prm.offset for _, prm, _ in prms]))
        members.sort(key=lambda m: not m[0])                # the cut blocks' items first: the 'mid' reduction takes a prefix
        plan.update(triples=triples, slab_size=slab_size,
                    items=np.array([r for m in members for r in m[1]], np.int32).reshape(-1, 6),
                    item_seg=np.array([r for m in members for r in m[2]], np.int32).reshape(-1, _hip.SEG_INTS),
                    n_cut=sum(len(m[1]) for m in members if m[0]) // 6,
                    slab_params=sorted(o for m in members for o in m[3]))
        plan['mid_reduce'] = plan['mid_after'] is not None and plan['n_cut'] > 0
        plan['fused_opt'] = bool(slab_size) and not dp and self.fuse_opt and not self.multi_stream
        return plan


    def _bwd_launches(self, n, sid, dp, reserve, fold):
        """The backward conv launches between a fork and a join of the side streams, as _bwd_plan lays them out -- one per
        dependency level of the (block, scale) triples, or per triple; multi-stream: one per triple and kind -- then the
        launch that ends the backward pass.  Each leaves `reserve` compute units free.  Returns (launches, plan)."""
        lib, keep = self.lib, self._keep
        call = functools.partial(Launch, reserve=reserve)
        Gn = lambda b, i: 'G%d_%d' % (self.blocks.index(b), i)
        plan = self._bwd_plan(n, dp)
        triples = plan['triples']
        slab = tab = None
        if plan['slab_size']:
            slab = torch.empty(plan['slab_size'], device=self.dev)
            tab = torch.from_numpy(plan['items'].reshape(-1)).to(self.dev)
            keep += [slab, tab]
        bwd = [Launch(None, 'fork')]

        def make_block(kb, b):
            """Argument builders of one block's backward launches (bound to THIS block)."""
            cp = b.conv.params
            L1 = b.L - 1
            pre = []
            # coarsest scale without a child block: its dy is the exit's dX alone
            if not b.children and (self.multi_stream or not b.has_exit or self.generic_exits or b.drop is not None):
                ctx = self._bn_ctx(b, L1, n, with_red=False)
                pre.append(call(lib.mpnn_bn_bwd_reduce, 'bn_bwd_reduce', b.dx.data_ptr(), C.byref(ctx),
                                b.dzg[L1].data_ptr(), self.dred[b.sum_off[L1]:].data_ptr(),
                                n * b.H[L1] * b.W[L1], stream=sid[b.H[L1]]))
            # g of the coarsest scale = BatchNorm backward of dz: its own launch in the multi-stream
            # schedule, applied while loading by the three consumers in the fused schedule.
            # (the general kernels have no g_ctx either: the same launch of its own)
            g_ctx = None
            if self.multi_stream or self.generic_convs:
                ctx = self._bn_ctx(b, L1, n)
                pre.append(call(lib.mpnn_bn_bwd_apply, 'bn_bwd_apply', b.dzg[L1].data_ptr(), C.byref(ctx),
                                n * b.H[L1] * b.W[L1], stream=sid[b.H[L1]], records=Gn(b, L1)))
            else:
                g_ctx = C.pointer(self._bn_ctx(b, L1, n))

            def vert_args(i):
                a = _hip.DgradVertArgs()
                fine = self._bn_ctx(b, i - 1, n)
                a.g, a.Cg = b.dzg[i].data_ptr(), b.C[i]
                if i == L1 and g_ctx is not None:
                    a.g_ctx = g_ctx
                a.w_pack = getattr(cp, 'w_vert_%i' % (i - 1)).data.data_ptr() if self.generic_convs else \
                    self.packs[b.pack['w_vert_%i' % (i - 1)][1]:].data_ptr()
                a.fine = C.pointer(fine)
                a.fine_has_dz = 1 if b.has_dz[i - 1] else 0
                a.dz_g_fine = b.dzg[i - 1].data_ptr()
                a.n, a.H, a.W, a.Cout = n, b.H[i], b.W[i], b.C[i - 1]
                keep.append(a)
                return a

            def horz_args(i):
                pb, j = b.parent, b.in_map[i]
                a = _hip.DgradHorzArgs()
                a.g, a.Cg = b.dzg[i].data_ptr(), b.C[i]
                if i == L1 and g_ctx is not None:
                    a.g_ctx = g_ctx
                a.w_pack = getattr(cp, 'w_horz_%i' % i).data.data_ptr() if self.generic_convs else \
                    self.packs[b.pack['w_horz_%i' % i][1]:].data_ptr()
                a.accumulate = triples[(kb, i)]['accumulate']
                a.dy_extra = pb.dx.data_ptr() if triples[(kb, i)]['dy_extra'] else None
                prev = self._bn_ctx(pb, j, n, with_red=False)
                a.prev = C.pointer(prev)
                a.out = pb.dzg[j].data_ptr()
                a.red_out = self.dred[pb.sum_off[j]:].data_ptr()
                a.n, a.H, a.W, a.Cout = n, b.H[i], b.W[i], pb.C[j]
                keep.append(a)
                return a

            def wgrad_args(i):
                t = triples[(kb, i)]
                a = _hip.WgradArgs()
                a.a = self._act_of_input(b, i, n, _hip.ACT_BN_BATCH)
                pa = getattr(cp, 'w_horz_%i' % i)
                pv = getattr(cp, 'w_vert_%i' % (i - 1)) if i > 0 else None
                pb = getattr(cp, 'b_%i' % i)
                if i > 0:
                    a.v, a.Cv = b.sp[i - 1].data_ptr(), b.C[i - 1]
                a.g = b.dzg[i].data_ptr()
                if i == L1 and g_ctx is not None:
                    a.g_ctx = g_ctx
                a.n, a.H, a.W, a.Cout = n, b.H[i], b.W[i], b.C[i]
                a.n_split, a.split_stride = t['split'], t['split_stride']
                # the partial gradients of a split launch go to its slabs, those of an unsplit one straight into G
                dst = lambda f, prm: prm.grad.data_ptr() if t['slab'] is None else slab.data_ptr() + 4 * t['slab'][f]
                a.dwa, a.db = dst('dwa', pa), dst('db', pb)
                a.dwv = dst('dwv', pv) if pv is not None else None
                keep.append(a)
                return a

            return pre, vert_args, horz_args, wgrad_args

        fl_v = lambda b, i: 2.0 * n * b.H[i] * b.W[i] * b.kv[i][0] * b.kv[i][1] * b.C[i] * b.C[i - 1]
        fl_h = lambda b, i: 2.0 * n * b.H[i] * b.W[i] * b.kh[i][0] * b.kh[i][1] * b.C[i] * b.parent.C[b.in_map[i]]
        rev = list(reversed(self.blocks))
        if not self.multi_stream:
            fns = {kb: make_block(kb, b) for kb, b in enumerate(rev)}
            started = set()
            for g, grp in enumerate(plan['groups']):
                for kb, i, _ in grp:
                    if kb not in started:
                        started.add(kb)
                        bwd += fns[kb][0]
                built = []                                  # (horz, vert, wgrad records, budget, flops, tag) per member
                for kb, i, bud in grp:
                    b, (_, vert_args, horz_args, wgrad_args) = rev[kb], fns[kb]
                    h = horz_args(i) if b.parent is not None else None
                    v = vert_args(i) if i > 0 else None
                    w = wgrad_args(i)
                    fl = self._conv_flops(b, i, n) + (fl_h(b, i) if h is not None else 0) + (fl_v(b, i) if v is not None else 0)
                    built.append((h, v, w, bud, fl, self._conv_tag(b, i)))
                fl, tag = sum(x[4] for x in built), ' | '.join(x[5] for x in built)
                if self.generic_convs:
                    (kb, i, _), (h, v, w) = grp[0], built[0][:3]
                    b = rev[kb]
                    kv = b.kv[i] or (0, 0)
                    if h is not None:
                        bwd.append(call(self._gen_fn('dgrad_horz'), 'dgrad_horz', C.byref(h), *b.kh[i], flops=fl_h(b, i), tag=tag))
                    if v is not None:
                        bwd.append(call(self._gen_fn('dgrad_vert'), 'dgrad_vert', C.byref(v), *kv, flops=fl_v(b, i), tag=tag))
                    bwd.append(call(self._gen_fn('wgrad'), 'wgrad', C.byref(w), *b.kh[i], *kv, flops=self._conv_flops(b, i, n),
                                    tag=tag))
                elif len(built) == 1 and built[0][3] is None:
                    h, v, w = built[0][:3]
                    bwd.append(call(lib.mpnn_msconv_bwd_scale, 'bwd_scale', C.byref(h) if h is not None else None,
                                    C.byref(v) if v is not None else None, C.byref(w), flops=fl, tag=tag))
                else:
                    mem = (_hip.BwdMember * len(built))()
                    for m, (h, v, w, bud, _, _) in zip(mem, built):
                        m.horz = C.pointer(h) if h is not None else None
                        m.vert = C.pointer(v) if v is not None else None
                        m.wgrad = C.pointer(w)
                        m.wg_horz, m.wg_vert = bud['gxh'], bud['gxv']
                    dev_rec = self._level_records(mem)
                    keep += [mem, dev_rec]
                    if self.co_share > 1:      # (one net of a co-trained group by itself: the group's launch form, one copy)
                        bwd.append(call(lib.mpnn_msconv_bwd_level_rep, 'bwd_scale', mem, len(built), 1, dev_rec.data_ptr(),
                                        flops=fl, tag=tag, host=mem))
                    else:
                        bwd.append(call(lib.mpnn_msconv_bwd_level, 'bwd_scale', mem, len(built), dev_rec.data_ptr(),
                                        flops=fl, tag=tag, host=mem))
                if g == plan['mid_after']:
                    if plan['mid_reduce']:
                        # data parallel: the conv gradients of the blocks the backward finished first are reduced
                        # from their slabs at the bucket boundary (their all-reduce then overlaps the rest of the
                        # backward pass); the launch that ends the backward takes the remaining items
                        bwd.append(call(lib.mpnn_slab_reduce, 'slab_reduce', slab.data_ptr(), self.G.data_ptr(), tab.data_ptr(),
                                        plan['n_cut']))
                    bwd.append(Launch(None, 'bucket', tag='mid'))
        else:
            wg_streams = (len(sid), len(sid) + 1)
            fns, started = {}, set()
            for kind, kb, i in plan['launches']:
                b = rev[kb]
                if kb not in started:
                    started.add(kb)
                    fns[kb] = make_block(kb, b)
                    bwd += fns[kb][0]
                _, vert_args, horz_args, wgrad_args = fns[kb]
                if kind == 'vert':
                    bwd.append(call(lib.mpnn_msconv_dgrad_vert, 'dgrad_vert', C.byref(vert_args(i)), flops=fl_v(b, i),
                                    tag='h%d %d->%d' % (b.H[i], b.C[i], b.C[i - 1]),
                                    stream=sid[b.H[i - 1]], waits=[Gn(b, i)], records=Gn(b, i - 1)))
                elif kind == 'horz':
                    bwd.append(call(lib.mpnn_msconv_dgrad_horz, 'dgrad_horz', C.byref(horz_args(i)), flops=fl_h(b, i),
                                    tag='h%d %d->%d' % (b.H[i], b.C[i], b.parent.C[b.in_map[i]]),
                                    stream=sid[b.H[i]]))
                else:
                    bwd.append(call(lib.mpnn_msconv_wgrad, 'wgrad', C.byref(wgrad_args(i)), flops=self._conv_flops(b, i, n),
                                    tag=self._conv_tag(b, i), stream=wg_streams[i % 2], waits=[Gn(b, i)]))
        bwd.append(Launch(None, 'join'))

        # ---- the launch that ends the backward pass ----
        keep_ptr = self.dsum_last.data_ptr() if fold else None
        if plan['fused_opt']:
            bwd.append(self._finish_opt_launch(n, slab, tab, plan, keep_ptr))
        elif slab is not None:
            # slab reduction + BatchNorm finalisation (moving averages, dgamma/dbeta): one launch
            bwd.append(call(lib.mpnn_backward_finish, 'backward_finish', slab.data_ptr(), self.G.data_ptr(),
                            tab[6 * plan['n_cut']:].data_ptr(), len(plan['items']) - plan['n_cut'], self.dsum.data_ptr(),
                            self.dred.data_ptr(), self.S.data_ptr(), self.bn_table.data_ptr(), self.n_bn, self.bn_decay, n, keep_ptr))
        else:
            bwd.append(call(lib.mpnn_bn_finalize, 'bn_finalize', self.dsum.data_ptr(), self.dred.data_ptr(),
                            self.S.data_ptr(), self.G.data_ptr(), self.bn_table.data_ptr(), self.n_bn,
                            self.bn_decay, n, keep_ptr))
        return bwd, plan


    def _finish_opt_launch(self, n, slab, tab, plan, keep_ptr):
        """Single process: slab reduction + BatchNorm finalisation + the TALR / momentum update of EVERY parameter as one
        launch (mpnn_backward_finish_opt) -- each workgroup updates the elements whose gradient it has just produced; the
        parameters whose gradients were final before (exits; tensors written without slabs) get workgroups of their own.
        Its arguments are the fields of one FinishNet record, with the BatchNorms' decay after bn_opt; the record is the
        launch's host (lib/_co.py: one record per net)."""
        bn_opt, fused = [], set(plan['slab_params'])       # fused: offsets of the parameters updated by slab items or BatchNorm rows
        for b in self.blocks:
            for i in range(b.L):
                bn = b.bns[i].params
                bn_opt += [b.node.idx, int(np.float32(bn.γ.l2).view(np.int32)), int(np.float32(bn.β.l2).view(np.int32)), 0]
                fused |= {bn.γ.offset, bn.β.offset}
        segs = self.seg_host.reshape(-1, _hip.SEG_INTS)
        plain = [segs[k] for k, off in enumerate(self._seg_owner) if off not in fused]
        t_seg = torch.from_numpy(plan['item_seg'].reshape(-1)).to(self.dev)
        t_bno = torch.tensor(bn_opt, dtype=torch.int32, device=self.dev)
        t_plain = torch.from_numpy(np.concatenate(plain) if plain else np.zeros(_hip.SEG_INTS, np.int32)).to(self.dev)
        self._keep += [t_seg, t_bno, t_plain]
        talr = 1 if (self.net._net_kind != 'sr' and getattr(self.net.hypers, 'talr', False)) else 0
        fin = _hip.FinishNet()
        fin.slabs, fin.slab_table, fin.n_items, fin.item_seg = slab.data_ptr(), tab.data_ptr(), len(plan['items']), t_seg.data_ptr()
        fin.sums, fin.reds, fin.state = self.dsum.data_ptr(), self.dred.data_ptr(), self.S.data_ptr()
        fin.bn_table, fin.n_bn, fin.bn_opt, fin.n_img, fin.sums_keep = self.bn_table.data_ptr(), self.n_bn, t_bno.data_ptr(), n, keep_ptr
        fin.params, fin.accum, fin.grads = self.P.data_ptr(), self.A.data_ptr(), self.G.data_ptr()
        fin.node_stat, fin.hyp, fin.talr, fin.inv_n, fin.grad_scale = self.node_stat.data_ptr(), self.hyp.data_ptr(), talr, 1.0 / n, 1.0
        fin.w_eq, fin.packs = (self.w_eq.data_ptr() if self.w_eq is not None else None), self.packs.data_ptr()
        fin.plain_seg, fin.n_plain = t_plain.data_ptr(), len(plain)
        f = [getattr(fin, name) for name, _ in fin._fields_]       # (f[:10]: slabs ... bn_opt)
        return Launch(self.lib.mpnn_backward_finish_opt, 'backward_finish', *f[:10], self.bn_decay, *f[10:], host=fin)


    def _level_records(self, mem):
        """The device records of a level launch, prepared from its member records `mem` (every pointer in them final)."""
        host = (C.c_char * (self.lib.mpnn_msconv_bwd_level_record_size() * len(mem)))()
        if self.co_share > 1:
            _hip.check(self.lib.mpnn_msconv_bwd_level_prepare_rep(mem, len(mem), 1, C.cast(host, C.c_void_p)), 'bwd_level records')
        else:
            _hip.check(self.lib.mpnn_msconv_bwd_level_prepare(mem, len(mem), C.cast(host, C.c_void_p)), 'bwd_level records')
        return torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(self.dev)
