"""CPU: tests/ev_walk_ref.py (the numpy statement of mpnn_ev_prefix_walk that tests/test_ev_prefix_walk.py holds the
kernel to) against the routing oracle on random trees: a record's reach bits are the 0/1 p_ev that oracle/route_ref.py
gives its node for the same router outputs (ties included: quantised outputs, +0.0 against -0.0), every sample lands in
at most one frontier list, and in exactly one when no leaf of the prefix takes it."""
import numpy as np
import pytest

import ev_walk_ref as W


def random_tree(rng, max_depth):
    """A static root over a switch (every deeper node then has a switch above it); below: leaves, static nodes and 2-,
    3- and 4-way switches at random, DFS preorder.  Returns (Tree, depth of every node)."""
    from oracle.route_ref import Tree
    nodes, depth = [], []

    def add(d, force=None):
        i = len(nodes)
        nodes.append(dict(sinks=[]))
        depth.append(d)
        k = force if force is not None else (0 if d >= max_depth else int(rng.choice([0, 0, 1, 2, 2, 3, 4])))
        for _ in range(k):
            nodes[i]['sinks'].append(add(d + 1))
        return i

    root = add(0, force=1)
    assert root == 0
    return Tree(nodes), depth


def _grow(rng, max_depth):
    while True:
        tree, depth = random_tree(rng, max_depth)
        if len(tree.nodes[1]['sinks']) >= 2 and len(tree.nodes) <= 60:
            return tree, depth


@pytest.mark.parametrize('seed', range(12))
def test_reach_bits_are_the_oracles_p_ev(seed):
    from oracle.route_ref import route
    rng = np.random.default_rng(seed)
    tree, depth = _grow(rng, max_depth=2 + seed % 4)
    n, N = 97, tree.nodes
    # router outputs: half of the switches quantised to {-1, -0.0, +0.0, 1} -- ties in most rows
    r_sw = []
    for i in tree.switches:
        S = len(N[i]['sinks'])
        x = rng.standard_normal((n, S))
        if rng.random() < 0.5:
            x = rng.choice([-1.0, -0.0, 0.0, 1.0], size=(n, S))
        r_sw.append(x)
    nl = len(tree.leaves)
    ref = route('actor', tree, r_sw, rng.random((nl, n)), np.ones((nl, n)), np.ones(len(N)))
    p_ev = ref['p_ev']
    assert np.isin(p_ev, (0.0, 1.0)).all()
    for d0 in range(2, max(depth) + 2):
        prefix = [i for i in range(len(N)) if depth[i] < d0]
        # records: every switch of the prefix (with or without a head), and some of its other nodes (head only)
        records = [i for i in prefix if len(N[i]['sinks']) > 1 or rng.random() < 0.5]
        heads = {i for i in records if len(N[i]['sinks']) < 2 or rng.random() < 0.5}
        fronts = [i for i in range(len(N)) if depth[i] == d0]
        stride = {i: len(N[i]['sinks']) + int(rng.integers(0, 3)) for i in records}
        tab = W.build(tree, records, heads, fronts, stride)
        r = []
        for i in tab.node:
            if len(N[i]['sinks']) > 1:
                x = np.full((n, stride[i]), np.nan)
                x[:, :len(N[i]['sinks'])] = r_sw[N[i]['switch_id']]
                r.append(x)
            else:
                r.append(None)
        ce = [rng.random(n) + 1.0 if h else None for h in tab.has_head]
        dc = [np.ones(n) if h else None for h in tab.has_head]
        got = W.walk(tab, r, ce, dc)
        for j, i in enumerate(tab.node):
            assert np.array_equal(got['reach'][j], p_ev[i] == 1.0), (d0, i)
            if tab.has_head[j]:
                assert np.array_equal(got['c_err'][j], ce[j] * p_ev[i]) and np.array_equal(got['d_cor'][j], p_ev[i])
            if r[j] is not None:
                S = tab.n_sinks[j]
                assert np.isnan(got['r'][j][:, S:]).all()
                assert np.array_equal(got['r'][j][:, :S], np.where(p_ev[i][:, None] == 1.0, r[j][:, :S], 0.0))
        member = np.zeros((len(fronts), n), int)
        for f, i in enumerate(fronts):
            member[f, got['fronts'][f]] = 1
            assert np.array_equal(member[f], p_ev[i].astype(int)), (d0, i)
        assert (member.sum(0) <= 1).all()
        taken = np.zeros(n, bool)                              # by a leaf of the prefix
        for i in prefix:
            if not N[i]['sinks']:
                taken |= p_ev[i] == 1.0
        assert np.array_equal(member.sum(0) == 1, ~taken)


def test_builder_on_a_known_tree():
    """static root -> 3-way A {leaf, B, C}; B 2-way {leaf, static D -> leaf}: tables by hand."""
    from oracle.route_ref import Tree
    tree = Tree([dict(sinks=[1]), dict(sinks=[2, 3, 6]), dict(), dict(sinks=[4, 5]), dict(), dict(sinks=[7]), dict(), dict()])
    tab = W.build(tree, [0, 1, 3, 5], {0, 3, 5}, [7, 6, 4], {1: 4})
    assert tab.parent == [-1, -1, 1, 2] and tab.parent_sink == [0, 0, 1, 1]
    assert tab.n_sinks == [0, 3, 2, 0] and tab.r_stride == [0, 4, 2, 0] and tab.has_head == [True, False, True, True]
    assert tab.front_parent == [2, 1, 2] and tab.front_sink == [1, 2, 0]
    r = [None, np.array([[0., 0., 0., np.nan], [0., 2., 2., np.nan], [-0., 0., 1., np.nan]]), np.array([[1., 1.], [0., 1.], [5., 4.]]), None]
    got = W.walk(tab, r, [np.ones(3), None, np.ones(3), np.ones(3)], [np.ones(3), None, np.ones(3), np.ones(3)])
    assert got['arg'][1].tolist() == [0, 1, 2] and got['arg'][2].tolist() == [0, 1, 0]
    assert got['reach'].tolist() == [[True] * 3, [True] * 3, [False, True, False], [False, True, False]]
    assert [f.tolist() for f in got['fronts']] == [[1], [2], []]
    assert got['r'][2].tolist() == [[0., 0.], [0., 1.], [0., 0.]] and got['c_err'][3].tolist() == [0., 1., 0.]
