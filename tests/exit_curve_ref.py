"""mpnn_exit_curve (csrc/exit_curve.hip) restated in plain numpy: one image and one threshold point at a time.

A tree is a list of nodes, each a dict(sinks=[node ids], switch=<row of r, or -1>, leaf=<leaf id, or -1>, exit=<index into
sinks of the classifier leaf directly below, or -1>); node 0 is the root.  conf, d_cor: [n_leaves, >= n]; r: [n_switches,
>= n, >= max sinks]; taus: [T, n_leaves] or, the broadcast form, [T]; node_ops: one integer per node."""
import numpy as np


def node(sinks=(), switch=-1, leaf=-1, exit=-1):
    return dict(sinks=list(sinks), switch=switch, leaf=leaf, exit=exit)


def argmax_first(v, skip=-1):
    """The arg-max of conf_gate_k: candidates in order, a later one wins only if it is GREATER (a NaN first stays)."""
    best, d = None, 0
    for i, x in enumerate(v):
        if i == skip:
            continue
        if best is None or np.float32(x) > best:
            best, d = np.float32(x), i
    return d


def walk(tree, node_ops, conf, r, tau_row, img):
    """(exit leaf, operations) of one image under one threshold row [n_leaves]."""
    cur, ops = 0, 0
    while True:
        nd = tree[cur]
        ops += int(node_ops[cur])
        S = len(nd['sinks'])
        if S == 0:
            return nd['leaf'], ops
        if S == 1:
            cur = nd['sinks'][0]
            continue
        e = nd['exit']
        tau = np.float32(np.nan)
        if e >= 0:
            le = tree[nd['sinks'][e]]['leaf']
            tau = np.float32(tau_row[le])
        gated = e >= 0 and not np.isnan(tau)
        if gated and np.float32(conf[le, img]) >= tau:             # (a NaN confidence compares false)
            d = e
        elif nd['switch'] >= 0:
            d = argmax_first(r[nd['switch'], img, :S], skip=e if gated else -1)
        else:                                                       # a static fork: one leaf + one other
            assert S == 2 and e >= 0
            d = 1 - e
        cur = nd['sinks'][d]


def curve(tree, node_ops, conf, d_cor, r, taus, n, n_leaves=None):
    """correct [T], ops [T], hist [T, n_leaves] (int64) over the images 0 .. n - 1."""
    n_leaves = sum(1 for nd in tree if not nd['sinks']) if n_leaves is None else n_leaves
    taus = np.asarray(taus, np.float32)
    if taus.ndim == 1:
        taus = np.repeat(taus[:, None], n_leaves, 1)
    T = taus.shape[0]
    correct, ops, hist = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros((T, n_leaves), np.int64)
    for t in range(T):
        for img in range(n):
            leaf, o = walk(tree, node_ops, conf, r, taus[t], img)
            ops[t] += o
            hist[t, leaf] += 1
            correct[t] += int(d_cor[leaf, img] == 1)
    return correct, ops, hist


def tree_of_net(net):
    """The tree of a net as Engine builds it (lib/_eng_alloc.py: nodes in net.layers order, a switch id per layer with two or
    more sinks, a leaf id per layer without), and node_ops."""
    layers = list(net.layers)
    index = {id(ℓ): k for k, ℓ in enumerate(layers)}
    leaf = {id(ℓ): k for k, ℓ in enumerate(ℓ for ℓ in layers if not ℓ.sinks)}
    sw = {id(ℓ): k for k, ℓ in enumerate(ℓ for ℓ in layers if len(ℓ.sinks) > 1)}
    tree, ops = [], []
    for ℓ in layers:
        ex = [i for i, s in enumerate(ℓ.sinks) if not s.sinks] if len(ℓ.sinks) > 1 else []
        tree.append(node([index[id(s)] for s in ℓ.sinks], sw[id(ℓ)] if ℓ.router is not None else -1,
                         leaf.get(id(ℓ), -1), ex[0] if ex else -1))
        ops.append(int(round(ℓ.n_ops + (ℓ.router.n_ops if ℓ.router is not None else 0))))
    return tree, ops


def ds_chain(n_blocks, x0_shape=(32, 32, 3), n_cls=10):
    """A deeply supervised SRNet chain, built by hand: an exit under EVERY block, no router anywhere (static forks)."""
    import arch_and_hypers as A
    from lib.layer_types import Chain, MultiscaleBatchNorm, MultiscaleConvMax, MultiscaleRect
    from lib.net_types import SRNet

    def block(i, *sinks):
        body = [MultiscaleConvMax(n_chan=A.arch[i], supp=A.conv_supp, k_l2=A.k_l2, σ_w=A.σ_w), MultiscaleBatchNorm(), MultiscaleRect()]
        return Chain(name='ReConvMax', sinks=sinks, comps=body)
    node = block(n_blocks - 1, A.reg(n_cls))
    for i in range(n_blocks - 2, -1, -1):
        node = block(i, A.reg(n_cls), node)
    return SRNet(x0_shape=x0_shape, y_shape=(n_cls,), root=A.pyr(node))
