"""What the engine decides about a net before anything is allocated, as host arithmetic: the tree classification with its
refusals, the conv and exit kernel families, and the layout of the flat buffers -- parameters / momentum / gradients in the
order the backward pass finishes them, gradient buckets, weight packs, optimizer work items, the fp64 statistic arenas, the
routing tables.  Structure(net) stands on its own, on a machine without a GPU: it loads the kernel
library for its host-only *_check / *_tiles entry points and keeps every table as numpy arrays, lists or ctypes records;
Allocation (lib/_eng_alloc.py) uploads them."""
import os

import numpy as np

from lib import _hip
from lib.layer_types import Chain
from lib.net_types import n_leaves, params_list_rec
from lib._eng_common import OPT_CHUNK, ROUTER_COMPS, _Block, _kind, _Node, head_dropout, head_parts, refuse_activity, refuse_dropout


class Structure:
    def __init__(self, net):
        self.net = net
        self.lib = _hip.load()
        self._classify()
        self._layout()

    # ------------------------------------------------------------------ structure
    def _classify(self):
        net = self.net
        self.nodes = []
        index = {}
        for ℓ in net.layers:
            nd = _Node()
            nd.idx, nd.layer, nd.kind = len(self.nodes), ℓ, _kind(ℓ)
            nd.parent, nd.sink_index = -1, 0
            index[id(ℓ)] = nd
            self.nodes.append(nd)
        for nd in self.nodes:
            for i, s in enumerate(nd.layer.sinks):
                index[id(s)].parent, index[id(s)].sink_index = nd.idx, i
        self.leaves = [nd for nd in self.nodes if len(nd.layer.sinks) == 0]
        self.switches = [nd for nd in self.nodes if len(nd.layer.sinks) > 1]
        for i, nd in enumerate(self.leaves):
            nd.leaf_id = i
        for i, nd in enumerate(self.switches):
            nd.switch_id = i
        self.max_sinks = max([len(nd.layer.sinks) for nd in self.switches] + [2])
        if len(self.nodes) > _hip.MAX_NODES or self.max_sinks > _hip.MAX_SINKS:
            raise NotImplementedError('routing tree too large for mpnn_route')
        kind = self.net._net_kind
        for nd in self.nodes:
            r = nd.layer.router
            if r is not None:
                if kind == 'sr' or len(nd.layer.sinks) < 2:
                    raise NotImplementedError('router on a node with < 2 sinks / in an SRNet')
                refuse_activity(getattr(r, 'comps', ()), 'the router of layer %r' % (nd.layer.name,))
                refuse_dropout(getattr(r, 'comps', ()), 'the router of layer %r' % (nd.layer.name,))
                if not isinstance(r, Chain) or [type(c).__name__ for c in r.comps] != ROUTER_COMPS:
                    raise NotImplementedError('router chain outside the MI355X hot path')
                if nd.kind != 'block':
                    raise NotImplementedError('router on a %s node' % nd.kind)
            elif len(nd.layer.sinks) > 1 and kind != 'sr':
                raise NotImplementedError('switch without router')
            if nd.kind == 'head' and nd.layer.sinks:
                raise NotImplementedError('LogReg with sinks')
        root = self.nodes[0]
        if root.kind != 'pyramid':
            raise NotImplementedError('root must be the ToPyramid chain')
        self.x0_shape = tuple(self.net.hypers.x0_shape)
        self.n_cls = int(self.net.hypers.y_shape[0])
        # blocks
        self.blocks = []
        self.label_maps = []           # the distinct w_cls [n_cls, n_sup] of the net's superclass heads, in tree order
        self.generic_exits = bool(int(os.environ.get('MPNN_GENERIC_EXITS', '0')))      # (1: the any-width exit kernels for every net)
        # The tuned conv bodies are 3x3 only: a net with any other filter runs ALL its multiscale convs on the general
        # kernels (csrc/conv_gen.hip: HWIO weights, no packs); 1 forces them on every net (cross-checks at 3x3).
        self.generic_convs = bool(int(os.environ.get('MPNN_GENERIC_CONVS', '0')))
        # Neither family takes every map (the tuned bodies: squares of 4, 8 or a multiple of 16; the general entry points:
        # squares of 4 or a multiple of 8): a net with any other map runs ALL its multiscale convs on the any-map entry
        # points (mpnn_msconv_*_hw: the general kernels with masked tiles, 1..256 per axis); 1 forces them on every net.
        self.anymap_convs = bool(int(os.environ.get('MPNN_ANYMAP_CONVS', '0')))
        # Both general families take Cin 1, 3 or a multiple of 16 and Cv / Cout in multiples of 16: a net with any other
        # channel count (the image's included) runs ALL its multiscale convs on the any-channel entry points
        # (mpnn_msconv_*_ch: the same records, output tiles fitted to the layer, 1..512 channels); 1 forces them on every net.
        self.anychan_convs = bool(int(os.environ.get('MPNN_ANYCHAN_CONVS', '0')))
        self._check_pyramid(root)
        # MultiscaleLLN behind ToPyramid: one launch in front of every program writes the normalised scales (lln_out, allocated
        # with x0), and the root blocks read those -- materialised maps, no strided pick -- instead of the image
        self.lln = root.layer.comps[1] if len(root.layer.comps) > 1 else None
        if self.lln is not None and (self.x0_shape[2] != 3 or self.lln.in_shifts != list(range(len(self.lln.in_shifts)))):
            raise NotImplementedError('MultiscaleLLN on other than the scales of a 3-channel ToPyramid')
        for nd in self.nodes:
            if nd.kind != 'block':
                continue
            b = _Block()
            b.node = nd
            conv, mbn, _ = nd.layer.comps
            b.conv, b.bns = conv, mbn.comps
            b.L = len(conv.hypers.n_chan)
            b.H = [s.shape[0] for s in conv.x]
            b.W = [s.shape[1] for s in conv.x]
            b.C = [s.shape[2] for s in conv.x]
            # filter geometry (layer_types.py:156-173): w_horz_i clipped to the map, w_vert_i supp x supp
            b.kh = [tuple(getattr(conv.params, 'w_horz_%i' % i).shape[:2]) for i in range(b.L)]
            b.kv = [None] + [tuple(getattr(conv.params, 'w_vert_%i' % (i - 1)).shape[:2]) for i in range(1, b.L)]
            if any(k != (3, 3) for k in b.kh + b.kv[1:]) or not all(self._tuned_map(h, w) for h, w in zip(b.H, b.W)):
                self.generic_convs = True
            par = self.nodes[nd.parent]
            b.parent = getattr(par, 'block', None)
            if par.kind == 'pyramid':
                n_pyr = par.layer.comps[0].hypers.n_scales
                b.in_shift = [n_pyr - b.L + i for i in range(b.L)]
                b.in_map = None
                b.Cin = [self.x0_shape[2]] * b.L
            elif par.kind == 'block':
                b.in_map = [b.parent.L - b.L + i for i in range(b.L)]
                b.in_shift = [0] * b.L
                b.Cin = [b.parent.C[j] for j in b.in_map]
            else:
                raise NotImplementedError('block below a %s node' % par.kind)
            b.children = []
            nd.block = b
            self.blocks.append(b)
        for b in self.blocks:
            kids = [self.nodes_by_layer(s) for s in b.node.layer.sinks]
            b.children = [k.block for k in kids if k.kind == 'block']       # tree nets: several (arch_and_hypers.py:99-127)
            b.sink_blocks = [k.block if k.kind == 'block' else None for k in kids]
            hs = [k for k in kids if k.kind == 'head']
            if len(hs) > 1:
                raise NotImplementedError('more than one LogReg under a block')
            b.head = hs[0] if hs else None
            # the width of the head's label space: the net's classes, or the columns of the map of a head that classifies
            # superclasses (SuperclassCrossEntropyError); b.lmap: which of the net's distinct maps it reads its labels through
            # b.loss: the head's error layer as the exit records carry it (MPNN_LOSS_*: cross-entropy, or SquaredError on the
            # softmax / on the LinTrans output)
            b.n_out, b.lmap, b.loss = self.n_cls if b.head is not None else 0, None, _hip.LOSS_CE
            err = None
            if b.head is not None:
                _, err, b.loss, _ = head_parts(b.head.layer)
            if type(err).__name__ == 'SuperclassCrossEntropyError':
                w = err.hypers.w_cls
                b.n_out = int(w.shape[1])
                b.lmap = next((k for k, m in enumerate(self.label_maps) if np.array_equal(m, w)), len(self.label_maps))
                if b.lmap == len(self.label_maps):
                    self.label_maps.append(w)
            b.router = b.node.layer.router
            b.has_exit = b.head is not None or b.router is not None
            # b.drop: the head's Dropout layer where the training program has to run one (λ < 1), else None
            b.drop = head_dropout(b.head.layer) if b.head is not None else None
            # which scales' BN outputs are consumed (by child blocks or the exit)
            b.has_dz = [False] * b.L
            for cb in b.children:
                for j in cb.in_map:
                    b.has_dz[j] = True
            if b.has_exit:
                b.has_dz[b.L - 1] = True
            # compile-time limits of the TUNED exit kernels (exit_tail.hip, exit_ev.hip, lin.hip): <= 16 classes, two
            # equal router layers of <= 16 units, C <= 128 in multiples of 16 (H*W*C % 16 == 0 alone does not say so: a
            # 4x4x10 map has K = 160).  A net with an exit beyond them runs ALL
            # its exits on the any-width forms (csrc/exit_gen.hip: plain kernels, same records), whose own limits are
            # checked here; beyond those the engine refuses instead of truncating.
            if b.has_exit:
                K = b.H[-1] * b.W[-1] * b.C[-1]
                R = R2 = 0
                if b.router is not None:
                    R, R2 = (b.router.comps[k].hypers.n_chan for k in (1, 4))
                    if len(b.node.layer.sinks) > _hip.MAX_SINKS:
                        raise NotImplementedError('more than %d sinks under one switch' % _hip.MAX_SINKS)
                tuned = b.C[-1] <= 128 and b.C[-1] % 16 == 0 and K % 16 == 0 and (b.head is None or b.n_out <= 16) and R == R2 and R <= 16
                if not tuned:
                    self.generic_exits = True
                    if self.lib.mpnn_exit_gen_check(b.C[-1], K, b.n_out, R, R2,
                                                    len(b.node.layer.sinks) if b.router is not None else 0):
                        raise NotImplementedError('exit on a %dx%dx%d map with %d classes and a %d-%d router: outside the any-width '
                                                  'exit kernels too (C <= 256, H*W*C <= 65536, <= 1024 classes, <= 256 units)'
                                                  % (b.H[-1], b.W[-1], b.C[-1], b.n_out, R, R2))
        for nd in self.nodes:
            if nd.kind == 'head' and self.nodes[nd.parent].kind != 'block':
                raise NotImplementedError('LogReg must hang off a ReConvMax block')
        # per leaf, in net.leaves order: the width of its label space; prediction rows are as wide as the widest
        self.leaf_n_cls = [self.nodes[nd.parent].block.n_out if nd.kind == 'head' else 0 for nd in self.leaves]
        self.n_cls_max = max(self.leaf_n_cls + [1])
        # Dispatch, once per net: (1) tuned launches where every map, filter and channel count is theirs; (2) else the
        # general entry points where every map is theirs; (3) else the any-map entry points; (4) the any-channel entry
        # points where a channel count is outside (2) and (3).  (2) to (4) share everything on the host (HWIO weights,
        # single-stream schedule, one set of launches per (block, scale)): generic_convs is set for all three.
        convs = [(b.H[i], b.W[i], b.Cin[i], b.C[i - 1] if i > 0 else 0, b.C[i], *b.kh[i], *(b.kv[i] or (0, 0)))
                 for b in self.blocks for i in range(b.L)]
        if not all(self.lib.mpnn_msconv_hw_check(8, 8, cin, cv, cout, 1, 1, 1 if cv else 0, 1 if cv else 0) == 0
                   for _, _, cin, cv, cout, *_ in convs):
            self.anychan_convs = True
        if self.anychan_convs:
            self.anymap_convs = True
        if self.generic_convs and not all(self.lib.mpnn_msconv_gen_check(h, w, 16, 0, 16, 1, 1, 0, 0) == 0 for h, w, *_ in convs):
            self.anymap_convs = True
        if self.anymap_convs:
            self.generic_convs = True
        if self.generic_convs:
            check = self.lib.mpnn_msconv_ch_check if self.anychan_convs else \
                self.lib.mpnn_msconv_hw_check if self.anymap_convs else self.lib.mpnn_msconv_gen_check
            for c in convs:
                if check(*c):
                    raise NotImplementedError(
                        'multiscale conv on a %dx%d map, %d+%d -> %d channels, %dx%d / %dx%d filters: outside the general '
                        'conv kernels (filters 1..7 per side, maps of 1..256 per side, 1..512 channels on every operand)' % c)


    def _tuned_map(self, h, w):
        """A map the tuned 3x3 bodies run in this engine: a square of side 4, 8 or a multiple of 16 (the geometries of
        mpnn_wgrad_tiles / mpnn_msconv_bwd_level_slots, of which the engine has only ever used the square ones)."""
        return h == w and self.lib.mpnn_wgrad_tiles(1, h, w) > 0


    def _check_pyramid(self, root):
        """The image sizes a pyramid of S scales is exact on: H0 and W0 multiples of 2**(S-1).  Only then is the reference's
        legacy bilinear resize at every scale a strided pick (oracle/np_ops.py: pyramid), every scale but the coarsest is
        even on both axes (the 2x2 / 2 SAME max-pool never pads, and pool(out[i-1]) has the size of scale i)."""
        S = int(root.layer.comps[0].hypers.n_scales)
        h, w = self.x0_shape[:2]
        q = 2 ** (S - 1)
        if h % q or w % q or not (1 <= h <= 256 and 1 <= w <= 256):
            raise NotImplementedError('a pyramid of %d scales needs image sides that are multiples of %d (at most 256): a %dx%d '
                                      'image is outside the MI355X hot path (its coarser scales would not be strided picks)'
                                      % (S, q, h, w))


    def nodes_by_layer(self, ℓ):
        for nd in self.nodes:
            if nd.layer is ℓ:
                return nd
        raise KeyError(ℓ)


    @staticmethod
    def _nslot(b, i):
        """Statistics slots of scale i: many workgroups -> many slots; few -> few (every consumer
        workgroup re-adds the slots in its prologue)."""
        return 8          # measured: 8 everywhere beats 16/16/8/4 by 1.6 % (one slot-sum round trip in every consumer)


    # ------------------------------------------------------------------ layout
    def _layout(self):
        """Every offset and table of the net's flat buffers, as host data; a table that Allocation uploads under the name
        `x` is kept here as `x_host`."""
        owner = {}
        for nd in self.nodes:
            for p in params_list_rec(nd.layer):
                owner[id(p)] = (nd.idx, 0)
            for p in params_list_rec(nd.layer.router):
                owner[id(p)] = (nd.idx, 1)
        # Flat layout in the order the BACKWARD pass finishes the gradients, so that data-parallel
        # training can all-reduce contiguous buckets while later gradients are still being computed:
        #   class 0: exit parameters (heads + routers): final after mpnn_lin_bwd, before the trunk backward
        #   class 1: conv weights / biases, deepest block first (the order the trunk backward runs)
        #   class 2: BatchNorm gamma / beta of the blocks (written by the launch that ends the backward)
        rev = {id(b): k for k, b in enumerate(reversed(self.blocks))}

        def ready_class(p):
            nd = self.nodes[owner[id(p)][0]]
            if owner[id(p)][1] or nd.kind != 'block':
                return (0, 0)
            if type(p.owner).__name__ == 'MultiscaleConvMax':
                return (1, rev[id(nd.block)])
            return (2, 0)
        self.trainable = sorted((p for p in self.net._all_params if p.trainable), key=ready_class)
        self.state_params = [p for p in self.net._all_params if not p.trainable]
        # The per-node TALR statistics (sum p_tr, sum p_tr^2; net_types.py:25-27) sit at the HEAD of G: they are final
        # right after mpnn_route -- before any gradient -- and every segment's learning-rate scale needs them, so under
        # data parallelism they ride in the FIRST bucket and each bucket can be applied as soon as it is reduced.
        # P and A keep the same (unused) prefix: one offset addresses a parameter in all three buffers.
        self.n_stat = 2 * len(self.nodes)
        off = self.stat_pad = (self.n_stat + 3) // 4 * 4
        cls_end, blk_end = {0: off, 1: off, 2: off}, {}
        for p in self.trainable:
            # every tensor starts on a 16-byte boundary: the kernels that stream gradients (slab reduction:
            # float4 loads and stores) take a 4x slower scalar path for a misaligned destination, and one
            # 10-float head bias would misalign everything behind it
            off = (off + 3) // 4 * 4
            p.offset, p.node, p.is_router = off, *owner[id(p)]
            off += p.size
            c = ready_class(p)
            for k in range(c[0], 3):
                cls_end[k] = off
            if c[0] == 1:
                blk_end[c[1]] = off
        off = (off + 3) // 4 * 4
        self.n_params = off
        # gradient buckets [lo, hi) in floats of G (the TALR node statistics ride at the head of the first one):
        # exits | conv of the blocks the backward finishes first (>= 40 % of the conv floats) | the rest
        conv_lo, conv_hi = cls_end[0], cls_end[1]
        cut, self.dp_cut_block = conv_hi, None
        for k in sorted(blk_end):
            if blk_end[k] - conv_lo >= 0.4 * (conv_hi - conv_lo) and blk_end[k] < conv_hi:
                cut, self.dp_cut_block = blk_end[k], k          # k: index in reversed(self.blocks)
                break
        end = off
        self.dp_buckets = {}                                   # name -> (lo, hi); markers of the same names in the program
        # ONE bucket by default: the whole of G is all-reduced after the launch that ends the backward pass.  The
        # bucketed form (3: exits | deep blocks | rest, each all-reduce issued where its bucket becomes final, beside the
        # rest of the backward pass) hides two of three collectives, but inside the step's hipGraph every parallel
        # branch that starts in the MIDDLE of the main branch stalls the main branch by ~30 us on this runtime
        # (profiles/r04_dp_corunner.txt: 498 -> 573 us with two 40-us stand-in kernels that overlap perfectly in the
        # kernel trace; no runtime knob changes it, profiles/r04_dp_env_sweep.txt), which is more than a 0.7-0.9 MB
        # all-reduce over xGMI takes.  A branch at the END of the graph (the one-bucket form) costs ~2 us.
        n_buckets = int(os.environ.get('MPNN_DP_BUCKETS', '1'))
        if os.environ.get('MPNN_DP_OVERLAP', '1') == '0':      # no overlap at all: the comparison point of the bucketed form
            n_buckets = 1
        if n_buckets <= 1:                                     # ONE all-reduce of the whole of G after the backward pass
            conv_lo, self.dp_cut_block = 0, None
        elif n_buckets == 2:                                   # exits | everything else
            self.dp_cut_block = None
        if conv_lo > self.stat_pad:
            self.dp_buckets['exit'] = (0, conv_lo)             # (with the node statistics at its head)
        else:
            conv_lo = 0
        if self.dp_cut_block is not None:
            self.dp_buckets['mid'] = (conv_lo, cut)
            self.dp_buckets['end'] = (cut, end)
        else:
            self.dp_buckets['end'] = (conv_lo, end)
        soff = 0
        for p in self.state_params:
            p.offset = soff
            soff += p.size
        self.n_state = soff
        # optimizer work items
        # weight packs
        desc, poff, pack_of = [], 0, {}
        for b in self.blocks:
            b.pack = {}
            for i in range(b.L if not self.generic_convs else 0):      # (the general kernels read the HWIO tensors)
                names = ['w_horz_%i' % i] + (['w_vert_%i' % (i - 1)] if i > 0 else [])
                for name in names:
                    p = getattr(b.conv.params, name)
                    ci, co = p.shape[2], p.shape[3]
                    fs = 9 * ((ci + 15) // 16) * 16 * co
                    bs = 9 * ((co + 15) // 16) * 16 * ci if ci % 16 == 0 else 0
                    desc += [p.offset, poff, poff + fs if bs else -1, ci, co, 0]
                    pack_of[id(p)] = (p.offset, ci, co, poff, poff + fs if bs else -1)
                    b.pack[name] = (poff, poff + fs if bs else None)
                    poff += fs + bs
        self.n_pack = len(desc) // 6
        self.pack_size = poff
        self.pack_desc_host = np.array(desc, np.int32)
        # `res` layers (layer_types.py:46,52,65-72): L2 pulls towards w_eq, the identity part of the init
        seg, eqs, eq_off = [], [], 0
        self._seg_owner = []                                # parameter (its offset) of every optimizer work item
        self._opt_info = {}                                 # id(p) -> (l2 bits, w_eq offset | -1, pack fields)

        for p in self.trainable:
            l2 = np.float32(p.l2).view(np.int32)
            has_eq = bool(p.l2) and p.eq is not None
            pk = pack_of.get(id(p), (0, 0, 0, -1, -1))     # conv weights: the optimizer also refreshes their packs
            self._opt_info[id(p)] = (int(l2), eq_off if has_eq else -1, pk)
            for s in range(0, p.size, OPT_CHUNK):
                seg += [p.offset + s, min(OPT_CHUNK, p.size - s), p.node, p.is_router, int(l2), eq_off + s if has_eq else -1,
                        pk[0], pk[1], pk[2], pk[3], pk[4], 0]
                self._seg_owner.append(p.offset)
            if has_eq:
                eqs.append(np.asarray(p.eq, np.float32).reshape(-1))
                eq_off += p.size
        self.w_eq_host = np.concatenate(eqs) if eqs else None
        self.n_seg = len(seg) // _hip.SEG_INTS
        # optimizer work items of each gradient bucket (the items are in layout order): [first, count)
        seg_off = seg[0::_hip.SEG_INTS]
        self.seg_range = {}
        for name, (lo, hi) in self.dp_buckets.items():
            ks = [k for k, o in enumerate(seg_off) if lo <= o < hi]
            self.seg_range[name] = (ks[0], len(ks)) if ks else (0, 0)
            assert not ks or ks == list(range(ks[0], ks[0] + len(ks)))
        self.seg_host = np.array(seg, np.int32)
        # fp64 BatchNorm arenas + finalize table
        doff, tab = 0, []
        for b in self.blocks:
            b.sum_off = []
            for i in range(b.L):
                bn = b.bns[i].params
                b.sum_off.append(doff)
                tab += [doff, bn.m_avg.offset, bn.v_avg.offset, b.C[i], b.H[i] * b.W[i],
                        bn.γ.offset if b.has_dz[i] else -1, bn.β.offset, self._nslot(b, i)]
                doff += 2 * b.C[i] * _hip.BN_SLOTS
        self.n_dsum = max(doff, 1)                              # doubles of each of the arenas dsum, dred and dsum_last
        self.n_bn = len(tab) // 8
        self.bn_table_host = np.array(tab, np.int32)
        # ONE moving-average decay for the conv BatchNorms of a net (a kernel argument of the finishing launch).  Trees
        # built through the layer classes always satisfy this: MultiscaleBatchNorm gives every scale a default
        # BatchNorm() whatever it was handed (reference layer_types.py:246).  A tree whose comps were edited by hand
        # is refused instead of trained with block 0's number.
        decays = sorted({float(bn.hypers.d) for b in self.blocks for bn in b.bns})
        if len(decays) > 1:
            raise NotImplementedError('conv BatchNorms with different moving-average decays %r are outside the MI355X '
                                      'hot path (one decay per net)' % (decays,))
        self.bn_decay = decays[0] if decays else 0.9
        # routing tables
        nodes, ops = [], []
        for nd in self.nodes:                                   # (DFS preorder: a parent comes before its children)
            nd.depth = 0 if nd.parent < 0 else self.nodes[nd.parent].depth + 1
        order = sorted(range(len(self.nodes)), key=lambda j: (self.nodes[j].depth, j))
        rank = {j: k for k, j in enumerate(order)}
        for nd in self.nodes:
            ℓ = nd.layer
            nodes += [nd.parent, nd.sink_index, len(ℓ.sinks), getattr(nd, 'switch_id', -1),
                      getattr(nd, 'leaf_id', -1), n_leaves(ℓ), nd.depth, rank[nd.idx]]
            ops.append(float(ℓ.n_ops + (ℓ.router.n_ops if ℓ.router is not None else 0)))
        kids = []
        for nd in self.switches:
            row = [self.nodes_by_layer(s).idx for s in nd.layer.sinks]
            kids += row + [0] * (self.max_sinks - len(row))
        self.node_tab_host = np.array(nodes, np.int32)
        self.kid_tab_host = np.array(kids if kids else [0], np.int32)
        self.node_ops_host = ops
        # (mpnn_ev_select: exact integer operation counts, and the node of every leaf in net.leaves order)
        self.node_ops_i64_host = np.array([int(round(o)) for o in ops], np.int64)
        self.leaf_node_tab_host = np.array([nd.idx for nd in self.leaves], np.int32)
        # Confidence-threshold exits (Net.predict(exit_conf=); csrc/conf_gate.hip).  A block is GATEABLE when it has both a
        # head and a router: gateable[leaf id of its head] = the block.
        self.gateable = {b.head.leaf_id: b for b in self.blocks if b.head is not None and b.router is not None}
        # The tree as mpnn_exit_curve walks it (csrc/exit_curve.hip; Net.exit_conf_curve), built once: per node its sinks, the
        # row of r of its ROUTER (-1: a static node, whatever its switch id), its leaf id and the sink that is a classifier
        # leaf directly below it.  curve_tree is the host copy that mpnn_exit_curve_check reads with every record.
        self.curve_tree = (_hip.CurveNode * len(self.nodes))()
        for nd, q in zip(self.nodes, self.curve_tree):
            sinks = [self.nodes_by_layer(s) for s in nd.layer.sinks]
            q.n_sinks = len(sinks)
            for i, s in enumerate(sinks):
                q.sink[i] = s.idx
            q.switch_id = nd.switch_id if nd.layer.router is not None else -1
            q.leaf_id = getattr(nd, 'leaf_id', -1)
            heads = [i for i, s in enumerate(sinks) if s.kind == 'head' and not s.layer.sinks] if len(sinks) > 1 else []
            q.exit_sink = heads[0] if heads else -1
