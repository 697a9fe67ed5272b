"""Synthetic forests for the irradiance tests (include/pgsd_irradiance.h), built with the oracle's forced splits and
tests/synth.py's streams: unbalanced quadtrees of chosen depths whose corner cells reach the deepest level (cells at both poles
and at phi = 0 / 2 pi), with consistent energies (leaves uniform in (0, 1], inner nodes the fp32 sum of their children).

Test infrastructure; the product never imports it.
"""
from __future__ import annotations

import numpy as np

import synth
from oracle import pg_oracle as po

BB0, BB1 = [0.0] * 3, [100.0] * 3


def node_cells(cols):
    """Per quadtree node of an export(): (tree, ix, iy, depth) of its cell; child k + 1 of the export is child k of
    pgsd_radiance.h (0: x high, y high; 1: x low, y high; 2: x low, y low; 3: x high, y low)."""
    root = np.asarray(cols["quadtree_rootNodeIndex"], np.int64)
    is_leaf = np.asarray(cols["quadtree_isLeaf"], bool)
    ch = [np.asarray(cols["quadtree_child_%d_index" % k], np.int64) for k in (1, 2, 3, 4)]
    n = is_leaf.shape[0]
    tree, ix, iy, d = (np.full(n, -1, np.int64) for _ in range(4))
    node = root.copy()
    tree[node], ix[node], iy[node], d[node] = np.arange(root.shape[0]), 0, 0, 0
    while node.size:
        node = node[~is_leaf[node]]
        for k in range(4):
            c = ch[k][node]
            tree[c], d[c] = tree[node], d[node] + 1
            ix[c] = 2 * ix[node] + (1 if k in (0, 3) else 0)
            iy[c] = 2 * iy[node] + (1 if k in (0, 1) else 0)
        node = np.concatenate([ch[k][node] for k in range(4)])
    return tree, ix, iy, d


def set_energies(cols, seed, leaf_energy=None):
    """Writes quadtree_irradiance: leaves 1 - u (or leaf_energy(tree, ix, iy, d, u) -> fp32), inner nodes c1 + c2 + c3 + c4 in
    fp32, that order, bottom-up."""
    is_leaf = np.asarray(cols["quadtree_isLeaf"], bool)
    n = is_leaf.shape[0]
    tree, ix, iy, d = node_cells(cols)
    u = synth.uniform(n, seed)[0]
    irr = np.zeros(n, np.float32)
    e = (np.float32(1) - u).astype(np.float32) if leaf_energy is None else np.asarray(leaf_energy(tree, ix, iy, d, u), np.float32)
    irr[is_leaf] = e[is_leaf]
    ch = [np.asarray(cols["quadtree_child_%d_index" % k], np.int64) for k in (1, 2, 3, 4)]
    for lv in range(int(d.max()) - 1, -1, -1):
        sel = np.nonzero((d == lv) & ~is_leaf)[0]
        s = irr[ch[0][sel]]
        for j in (1, 2, 3):
            s = (s + irr[ch[j][sel]]).astype(np.float32)
        irr[sel] = s
    cols["quadtree_irradiance"] = irr
    return cols


def ragged_forest(kd_rounds, extra_leaves, depths, seed=5):
    """export() columns of a forest of 2^kd_rounds + extra_leaves KD leaves; quadtree t is depths[t % len(depths)] levels deep.
    Below the first two levels a leaf splits when it is a corner cell of the square or one in three by position: ragged trees
    whose deepest cells touch both poles and the seam phi = 0 / 2 pi.  Energies: set_energies(seed)."""
    t = po.OracleTree()
    t.setup(BB0, BB1, 20, 20, True)
    for _ in range(kd_rounds):
        t.kd_split(t.kd_all_leaves())
    if extra_leaves:
        t.kd_split(t.kd_all_leaves()[:extra_leaves])
    depths = np.asarray(depths, np.int64)
    for lv in range(int(depths.max())):
        c = t.export()
        tree, ix, iy, d = node_cells(c)
        leaves = t.quad_all_leaves().astype(np.int64)
        top = (1 << d[leaves]) - 1
        corner = ((ix[leaves] == 0) | (ix[leaves] == top)) & ((iy[leaves] == 0) | (iy[leaves] == top))
        third = (tree[leaves] + 3 * ix[leaves] + 5 * iy[leaves]) % 3 == 0
        pick = (d[leaves] == lv) & (depths[tree[leaves] % depths.shape[0]] > lv) & ((lv < 2) | corner | third)
        t.quad_split(leaves[pick].astype(np.uint32))
    t.clean_unused_quadtree()
    return set_energies(t.export(), seed)
