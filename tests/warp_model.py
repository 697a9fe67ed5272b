"""A numpy model of the sample warp and its inverse, written from include/pgsd_warp.h (not from the kernels).

Test infrastructure.  One numpy operation per operation the header writes, on arrays of the model's float type, vectorised over
lanes, at most 32 passes over the levels.  It runs on the columns of OracleTree.export(); the parts the oracle already defines
come from it (canonical_to_dir, dir_to_canonical, get_leaf_node_index, pdf).

`WarpModel(tree)` is the float32 model the kernels must equal bit for bit.  `WarpModel(tree, np.float64)` is the same code in
float64 -- the probabilities, the rectangles and the canonical mappings (numpy's own sin / cos / arctan2 there) -- and serves as
the reference of the tolerances in tests/test_warp_model.py.

The warp (`_forward`) walks by node index and picks a child from u; the inverse (`_inverse`) walks by geometry and picks the
child that contains the position.  They share no code but the node's row and column sums, which the header defines once.
"""
from __future__ import annotations

import numpy as np

from oracle import pg_oracle as po

MAX_LEVELS = 32
# geometry of quad_child[k] (quadtree.py:153-175), k = 0..3: TR, TL, BL, BR
TOP = np.array([True, True, False, False])
LEFT = np.array([False, True, True, False])


class WarpModel:
    def __init__(self, tree, dtype=np.float32):
        self.tree = tree
        self.F = F = np.dtype(dtype).type
        c = tree.export()
        self.kd_tree = c["kdtree_quadTreeRootIndex"].astype(np.int64)
        self.roots = c["quadtree_rootNodeIndex"].astype(np.int64)
        self.leaf = c["quadtree_isLeaf"].astype(bool)
        self.child = np.stack([c["quadtree_child_%d_index" % k].astype(np.int64) for k in (1, 2, 3, 4)])
        self.irr = c["quadtree_irradiance"].astype(F)  # (float32 values; exact in float64)
        self.bbox_min, self.bbox_max = c["quadtree_bbox_min"], c["quadtree_bbox_max"]
        self.ONE_M = F(1) - F(2.0 ** -24)

    # ---- the parts pgsd_warp.h defines once -------------------------------------------------------------------------------
    def clamp_unit(self, v):
        F = self.F
        with np.errstate(invalid="ignore"):
            return np.where(v > 0, np.where(v < self.ONE_M, v, self.ONE_M), F(0)).astype(F)

    def node_sums(self, node):
        """(eTL, eBL, t, b, tot) of inner nodes, the uniform fallback applied."""
        F = self.F
        e = [self.irr[self.child[k][node]] for k in range(4)]
        with np.errstate(invalid="ignore", over="ignore"):
            t = (e[0] + e[1]).astype(F)
            b = (e[2] + e[3]).astype(F)
            tot = (t + b).astype(F)
            bad = ~(tot > 0) | ~np.isfinite(tot)
        return (np.where(bad, F(1), e[1]).astype(F), np.where(bad, F(1), e[2]).astype(F), np.where(bad, F(2), t).astype(F),
                np.where(bad, F(2), b).astype(F), np.where(bad, F(4), tot).astype(F))

    def root_of(self, p):
        """The root node of the quadtree of the KD leaf that holds each position (outside the box, NaN: node 0's tree)."""
        return self.roots[self.kd_tree[self.tree.get_leaf_node_index(p).astype(np.int64)]]

    # ---- WARP -------------------------------------------------------------------------------------------------------------
    def _forward(self, root, u):
        """u (2, n) -> canonical position (2, n), the leaf node reached, levels walked."""
        F = self.F
        ux, uy = self.clamp_unit(np.asarray(u[0], F)), self.clamp_unit(np.asarray(u[1], F))
        n = ux.shape[0]
        node = np.array(root, np.int64, copy=True)
        x0, y0, s = np.zeros(n, F), np.zeros(n, F), np.ones(n, F)
        levels = np.zeros(n, np.int64)
        for _ in range(MAX_LEVELS):
            w = np.nonzero(~self.leaf[node])[0]
            if w.size == 0:
                break
            eTL, eBL, t, b, tot = self.node_sums(node[w])
            x, y = ux[w], uy[w]
            with np.errstate(invalid="ignore", divide="ignore"):
                Py = (t / tot).astype(F)
                top = y < Py
                vy = np.where(top, (y / Py).astype(F), ((y - Py).astype(F) / (F(1) - Py).astype(F)).astype(F))
                rs, eL = np.where(top, t, b), np.where(top, eTL, eBL)
                Pl = (eL / rs).astype(F)
                left = x < Pl
                vx = np.where(left, (x / Pl).astype(F), ((x - Pl).astype(F) / (F(1) - Pl).astype(F)).astype(F))
                vx = np.where(vx < self.ONE_M, vx, self.ONE_M).astype(F)
                vy = np.where(vy < self.ONE_M, vy, self.ONE_M).astype(F)
            h = (s[w] * F(0.5)).astype(F)
            x0[w] = np.where(~left, (x0[w] + h).astype(F), x0[w])
            y0[w] = np.where(top, (y0[w] + h).astype(F), y0[w])
            s[w] = h
            k = np.where(top, np.where(left, 1, 0), np.where(left, 2, 3))
            node[w] = self.child[k, node[w]]
            ux[w], uy[w] = vx, vy
            levels[w] += 1
        px = (x0 + (ux * s).astype(F)).astype(F)
        py = (y0 + (uy * s).astype(F)).astype(F)
        return np.stack([px, py]), node, levels

    def canonical_to_dir(self, c):
        if self.F is np.float32:
            return po.canonical_to_dir(c)
        cos_t = 2.0 * c[1] - 1.0
        sin_t = np.sqrt(1.0 - cos_t * cos_t)
        phi = 2.0 * np.pi * c[0]
        return np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t])

    def dir_to_canonical(self, d):
        if self.F is np.float32:
            return po.dir_to_canonical(d)
        phi = np.arctan2(d[1], d[0])
        phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
        return np.stack([phi / (2.0 * np.pi), (np.clip(d[2], -1.0, 1.0) + 1.0) / 2.0])

    def sample_warp(self, p, u, active=None):
        """pg_sample_warp: (dir (3, n), pdf (n,)).  (float64: the pdf is not modelled, None.)"""
        c, _, _ = self._forward(self.root_of(p), u)
        d = self.canonical_to_dir(c)
        if self.F is not np.float32:
            return d, None
        pdf = self.tree.pdf(p, d)
        if active is not None:
            off = np.asarray(active) == 0
            d[:, off] = np.array([[0.0], [0.0], [-1.0]], np.float32)
            pdf[off] = 1.0
        return d, pdf

    # ---- INVERSE ----------------------------------------------------------------------------------------------------------
    def _inverse(self, root, c):
        """canonical position (2, n) -> dict of ax, ay, bx, by (the leaf's preimage), x0, y0, s (its cell), levels, node."""
        F = self.F
        cx, cy = np.asarray(c[0], F), np.asarray(c[1], F)
        n = cx.shape[0]
        node = np.array(root, np.int64, copy=True)
        ax, ay, bx, by = np.zeros(n, F), np.zeros(n, F), np.ones(n, F), np.ones(n, F)
        x0, y0, s = np.zeros(n, F), np.zeros(n, F), np.ones(n, F)
        levels = np.zeros(n, np.int64)
        stopped = np.zeros(n, bool)
        for _ in range(MAX_LEVELS):
            w = np.nonzero(~self.leaf[node] & ~stopped)[0]
            if w.size == 0:
                break
            h = (s[w] * F(0.5)).astype(F)
            mx, my = (x0[w] + h).astype(F), (y0[w] + h).astype(F)
            xge, xle, yge, yle = cx[w] >= mx, cx[w] <= mx, cy[w] >= my, cy[w] <= my
            last = np.where(xge & yle, 3, np.where(xle & yle, 2, np.where(xle & yge, 1, np.where(xge & yge, 0, -1))))
            stopped[w[last < 0]] = True          # outside every child: a canonical position never is
            keep = last >= 0
            w, h, mx, my, last = w[keep], h[keep], mx[keep], my[keep], last[keep]
            top, left = TOP[last], LEFT[last]
            eTL, eBL, t, b, tot = self.node_sums(node[w])
            Py = (t / tot).astype(F)
            yp = (by[w] * Py).astype(F)
            ay[w] = np.where(top, ay[w], (ay[w] + yp).astype(F))
            by[w] = np.where(top, yp, (by[w] * (F(1) - Py).astype(F)).astype(F))
            rs, eL = np.where(top, t, b), np.where(top, eTL, eBL)
            with np.errstate(invalid="ignore", divide="ignore"):
                Pl = np.where(rs > 0, (eL / rs).astype(F), F(0.5)).astype(F)
            xp = (bx[w] * Pl).astype(F)
            ax[w] = np.where(left, ax[w], (ax[w] + xp).astype(F))
            bx[w] = np.where(left, xp, (bx[w] * (F(1) - Pl).astype(F)).astype(F))
            x0[w] = np.where(~left, mx, x0[w])
            y0[w] = np.where(top, my, y0[w])
            s[w] = h
            node[w] = self.child[last, node[w]]
            levels[w] += 1
        return {"ax": ax, "ay": ay, "bx": bx, "by": by, "x0": x0, "y0": y0, "s": s, "levels": levels, "node": node}

    def invert_canonical(self, root, c):
        """u (2, n) of canonical positions, and the walk's dict."""
        F = self.F
        r = self._inverse(root, c)
        vx = ((np.asarray(c[0], F) - r["x0"]).astype(F) / r["s"]).astype(F)
        vy = ((np.asarray(c[1], F) - r["y0"]).astype(F) / r["s"]).astype(F)
        ux = self.clamp_unit((r["ax"] + (r["bx"] * vx).astype(F)).astype(F))
        uy = self.clamp_unit((r["ay"] + (r["by"] * vy).astype(F)).astype(F))
        return np.stack([ux, uy]), r

    def invert_warp(self, p, d, active=None):
        """pg_invert_warp: (u (2, n), pdf (n,)).  (float64: the pdf is not modelled, None.)"""
        u, _ = self.invert_canonical(self.root_of(p), self.dir_to_canonical(d))
        if self.F is not np.float32:
            return u, None
        pdf = self.tree.pdf(p, d)
        if active is not None:
            off = np.asarray(active) == 0
            u[:, off] = 0.0
            pdf[off] = 1.0
        return u, pdf

    # ---- helpers of the tests ---------------------------------------------------------------------------------------------
    def leaves_of(self, root):
        """Node indices of the leaves below `root` (one quadtree)."""
        out, todo = [], np.array([root], np.int64)
        while todo.size:
            out.append(todo[self.leaf[todo]])
            todo = self.child[:, todo[~self.leaf[todo]]].reshape(-1)
        return np.concatenate(out)

    def leaf_centres(self, nodes):
        """(2, n) canonical centres of quadtree nodes, from the exported boxes (exact: dyadic numbers)."""
        return ((self.bbox_min[nodes].astype(np.float64) + self.bbox_max[nodes].astype(np.float64)) * 0.5).T.astype(self.F)

    def root_thresholds(self, root):
        """(Py, Pl of the top row, Pl of the bottom row) of one inner root node, as the model's floats."""
        F = self.F
        eTL, eBL, t, b, tot = self.node_sums(np.array([root], np.int64))
        return F(t[0] / tot[0]), F(eTL[0] / t[0]), F(eBL[0] / b[0])


def with_dead_quadtree(tree, which: int = 0):
    """A copy of `tree` (through export() / load()) in which every node of quadtree `which` has energy 0: the warp falls back to
    uniform at every level there, and every direction has pdf 0."""
    c = tree.export()
    m = WarpModel(tree)
    todo, nodes = np.array([m.roots[which]], np.int64), []
    while todo.size:
        nodes.append(todo)
        todo = m.child[:, todo[~m.leaf[todo]]].reshape(-1)
    irr = c["quadtree_irradiance"].copy()
    irr[np.concatenate(nodes)] = 0
    c["quadtree_irradiance"] = irr
    out = po.OracleTree()
    out.load(c)
    return out
