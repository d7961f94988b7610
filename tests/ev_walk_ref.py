"""mpnn_ev_prefix_walk's contract (include/mpnn_hip.h) restated in plain numpy, and a builder of its record tables.

The launch gets the exits of a routed evaluation's dense prefix -- `count` records in topological order, each with a
router (n_sinks[j] > 0, outputs r[j]: [n, r_stride[j]]) and / or a head (c_err[j], d_cor[j]: [n]) -- evaluated on EVERY
sample, and makes them routed after the fact:

  * a switch sends sample s to sink arg-max r[j][s, :n_sinks[j]], FIRST index on ties (net_types.py:127-129);
  * record j is reached by s when parent[j] < 0, or when s reaches record parent[j] and that switch sends it to
    parent_sink[j];
  * r[j][s, :n_sinks[j]], c_err[j][s] and d_cor[j][s] of a record s does not reach become 0; everything else -- reached
    entries, the padding columns r[j][s, n_sinks[j]:] -- keeps its bits;
  * frontier list f receives every sample that reaches front_parent[f] and is sent to front_sink[f] there (appended, in
    any order).

TEST INFRASTRUCTURE: tests/test_ev_walk_ref_cpu.py checks it against oracle/route_ref.py's p_ev on random trees,
tests/test_ev_prefix_walk.py checks the kernel against it."""
import numpy as np


class Table:
    """parent, parent_sink, n_sinks, r_stride, has_head: one entry per record; front_parent, front_sink: per list;
    node / front_node: the tree node behind each record / list (None for a table given directly)."""

    def __init__(self, parent, parent_sink, n_sinks, has_head, front_parent, front_sink, r_stride=None, node=None,
                 front_node=None):
        self.parent, self.parent_sink, self.n_sinks = list(parent), list(parent_sink), list(n_sinks)
        self.has_head = [bool(h) for h in has_head]
        self.front_parent, self.front_sink = list(front_parent), list(front_sink)
        self.r_stride = list(r_stride) if r_stride is not None else list(self.n_sinks)
        self.node, self.front_node = node, front_node
        self.count, self.n_front = len(self.parent), len(self.front_parent)
        for j in range(self.count):                            # (what the host refuses)
            p = self.parent[j]
            assert p < j and (p < 0 or 0 <= self.parent_sink[j] < self.n_sinks[p])
            assert self.n_sinks[j] == 0 or self.r_stride[j] >= self.n_sinks[j]
        for p, k in zip(self.front_parent, self.front_sink):
            assert 0 <= p < self.count and 0 <= k < self.n_sinks[p]


def build(tree, records, heads, fronts, r_stride=None):
    """The table of a prefix of `tree` (oracle.route_ref.Tree: nodes in DFS preorder, a node with two or more sinks is a
    switch).  records: the nodes that get a record (ascending = topological); heads: those of them with a head; fronts:
    the nodes OUTSIDE the prefix that get a sample list.  Every switch above a record or a list must be a record.
    r_stride: {node: row stride of its router outputs} (default: its number of sinks)."""
    up = {0: (-1, 0)}
    for i, nd in enumerate(tree.nodes):
        for k, c in enumerate(nd['sinks']):
            up[c] = (i, k)

    def switch_above(x):
        """(nearest switch above node x, its sink that leads to x) or (-1, 0)."""
        p, k = up[x]
        while p >= 0 and len(tree.nodes[p]['sinks']) < 2:
            p, k = up[p]
        return (p, k) if p >= 0 else (-1, 0)

    records = sorted(records)
    rec_of = {x: j for j, x in enumerate(records)}
    parent, parent_sink, n_sinks = [], [], []
    for x in records:
        p, k = switch_above(x)
        parent.append(rec_of[p] if p >= 0 else -1)
        parent_sink.append(k)
        s = len(tree.nodes[x]['sinks'])
        n_sinks.append(s if s > 1 else 0)
    fp, fs = [], []
    for x in fronts:
        assert x not in rec_of
        p, k = switch_above(x)
        fp.append(rec_of[p])
        fs.append(k)
    stride = [max((r_stride or {}).get(x, 0), s) for x, s in zip(records, n_sinks)]
    return Table(parent, parent_sink, n_sinks, [x in heads for x in records], fp, fs, stride, records, list(fronts))


def walk(tab, r, c_err=None, d_cor=None):
    """r[j]: [n, r_stride[j]] (None for a record without a router); c_err[j], d_cor[j]: [n] (None without a head).
    Returns dict(arg [count][n] (-1: no router), reach [count][n] bool, r / c_err / d_cor as the launch leaves them
    (copies), fronts: one sorted int array of samples per list)."""
    n = next(x.shape[0] for x in r if x is not None)
    arg = np.full((tab.count, n), -1)
    reach = np.zeros((tab.count, n), bool)
    for j in range(tab.count):
        if tab.n_sinks[j] > 0:
            arg[j] = np.argmax(r[j][:, :tab.n_sinks[j]], axis=1)           # (np.argmax: the first maximum)
        p = tab.parent[j]
        reach[j] = True if p < 0 else reach[p] & (arg[p] == tab.parent_sink[j])
    out = dict(arg=arg, reach=reach, r=[], c_err=[], d_cor=[])
    for j in range(tab.count):
        x = None
        if r[j] is not None:
            x = np.array(r[j])
            x[~reach[j], :tab.n_sinks[j]] = 0.0
        out['r'].append(x)
        for name, src in (('c_err', c_err), ('d_cor', d_cor)):
            y = None
            if src is not None and src[j] is not None:
                y = np.array(src[j])
                y[~reach[j]] = 0.0
            out[name].append(y)
    out['fronts'] = [np.flatnonzero(reach[p] & (arg[p] == k)) for p, k in zip(tab.front_parent, tab.front_sink)]
    return out
