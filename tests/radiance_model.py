"""Model of include/pgsd_radiance.h in numpy, written from the header, one operation per header operation: the estimate
(pg_radiance_query), the decision (pg_radiance_rr), and the weights a refine carries.  It runs on the columns of an export()
(the oracle's or the device's: the same schema) plus a weight array, and uses of the oracle only its scalar helpers
(dirToCanonical, the PCG32 stream).

The float type is a parameter: float32 is the model the device must equal bit for bit, float64 the reference the tolerances
of tests/test_radiance_model.py come from.  (The canonical coordinates are dirToCanonical's fp32 values in both: they decide
WHICH leaf is read, which is not a matter of precision.)

Test infrastructure; the product never imports it.
"""
from __future__ import annotations

import numpy as np

from oracle import pg_oracle as po

INV_FOUR_PI = 0.07957747154594766788


def rr_window(window, ftype=np.float32):
    """lo = 2 / (1 + s), hi = s * lo, each operation rounded on its own."""
    T = ftype
    s = T(window)
    lo = T(T(2) / T(T(1) + s))
    return lo, T(s * lo)


class RadianceModel:
    def __init__(self, cols, weights, ftype=np.float32):
        self.T = ftype
        self.c = cols
        self.w = np.asarray(weights, np.uint64)
        self.kd_leaf = np.asarray(cols["kdtree_isLeaf"], bool)
        self.kd_l = np.asarray(cols["kdtree_child_left_index"], np.int64)
        self.kd_r = np.asarray(cols["kdtree_child_right_index"], np.int64)
        self.kd_depth = np.asarray(cols["kdtree_depth"], np.int64)
        self.kd_min = np.asarray(cols["kdtree_bbox_min"], np.float32).reshape(-1, 3)
        self.kd_max = np.asarray(cols["kdtree_bbox_max"], np.float32).reshape(-1, 3)
        self.kd_tree = np.asarray(cols["kdtree_quadTreeRootIndex"], np.int64)
        self.root = np.asarray(cols["quadtree_rootNodeIndex"], np.int64)
        self.q_leaf = np.asarray(cols["quadtree_isLeaf"], bool)
        self.q_irr = np.asarray(cols["quadtree_irradiance"], np.float32)
        self.q_ch = np.stack([np.asarray(cols["quadtree_child_%d_index" % k], np.int64) for k in (1, 2, 3, 4)])
        assert self.w.shape == self.root.shape

    # ---- the KD leaf: KDTree.getLeafNodeIndex --------------------------------------------------------------------------------
    def kd_node(self, p, active=None):
        """The node pg_pdf finds: a position outside the root box (inclusive) or NaN gets the root node; inside a node the
        right child takes p[axis] >= its lower plane (the children meet at the split), axis = depth % 3."""
        p = np.asarray(p, np.float32)
        n = p.shape[1]
        with np.errstate(invalid="ignore"):
            search = ((p >= self.kd_min[0][:, None]) & (p <= self.kd_max[0][:, None])).all(axis=0)
        if active is not None:
            search &= np.asarray(active) != 0
        node = np.zeros(n, np.int64)
        lanes = np.arange(n)
        for _ in range(64):
            go = search & ~self.kd_leaf[node]
            if not go.any():
                break
            axis = self.kd_depth[node] % 3
            right = self.kd_r[node]
            split = self.kd_min[right, axis]
            node = np.where(go, np.where(p[axis, lanes] >= split, right, self.kd_l[node]), node)
        return node

    def tree_of(self, p, active=None):
        return self.kd_tree[self.kd_node(p, active)]

    # ---- the directional leaf: the descent of pdfQuadTree / addIrradiancePropagate ----------------------------------------
    def leaf(self, tree, cx, cy):
        """(e, d, node) of the leaf the descent reaches from the root of `tree`: level by level the HIGHEST-numbered child
        whose test holds, edges included."""
        cx, cy = np.asarray(cx, np.float32), np.asarray(cy, np.float32)
        node = self.root[tree].copy()
        n = node.shape[0]
        lox, loy = np.zeros(n, np.float32), np.zeros(n, np.float32)
        h = np.full(n, 0.5, np.float32)
        d = np.zeros(n, np.int64)
        walking = np.ones(n, bool)
        for _ in range(64):
            go = walking & ~self.q_leaf[node]
            if not go.any():
                break
            mx, my = lox + h, loy + h
            xge, xle, yge, yle = cx >= mx, cx <= mx, cy >= my, cy <= my
            t0, t1, t2, t3 = xge & yge, xle & yge, xle & yle, xge & yle
            last = np.where(t3, 3, np.where(t2, 2, np.where(t1, 1, np.where(t0, 0, -1))))
            walking &= ~(go & (last < 0))          # no test holds: the walk ends at the node it stands on
            go &= last >= 0
            node = np.where(go, self.q_ch[np.maximum(last, 0), node], node)
            lox = np.where(go & ((last == 0) | (last == 3)), mx, lox)
            loy = np.where(go & ((last == 0) | (last == 1)), my, loy)
            h = np.where(go, h * np.float32(0.5), h)
            d += go
        return self.q_irr[node], d, node

    # ---- the estimate ----------------------------------------------------------------------------------------------------------
    def estimate(self, p, direction=None, active=None):
        """(L_dir, L_mean); L_dir is None without a direction."""
        T = self.T
        n = np.asarray(p).shape[1]
        act = np.ones(n, bool) if active is None else np.asarray(active) != 0
        t = self.tree_of(p, None)             # (the KD leaf is pg_pdf's for every lane that is computed: active lanes search)
        N = self.w[t]
        Nf = N.astype(np.float32).astype(T) if T is np.float32 else N.astype(np.float64)
        zero = N == 0
        Nf = np.where(zero, T(1), Nf)
        k = T(np.float32(INV_FOUR_PI))
        with np.errstate(all="ignore"):
            L_mean = ((self.q_irr[self.root[t]].astype(T) * k).astype(T) / Nf).astype(T)
            L_mean = np.where(zero | ~act, T(0), L_mean).astype(T)
            L_dir = None
            if direction is not None:
                c = po.dir_to_canonical(np.asarray(direction, np.float32))
                e, d, _ = self.leaf(t, c[0], c[1])
                area_inv = np.ldexp(T(1), (2 * d).astype(np.int32)).astype(T)     # 4^d, exact
                L_dir = ((((e.astype(T) * area_inv).astype(T)) * k).astype(T) / Nf).astype(T)
                L_dir = np.where(zero | ~act, T(0), L_dir).astype(T)
        return L_dir, L_mean

    # ---- the decision ----------------------------------------------------------------------------------------------------------
    def roulette(self, p, direction, weight, reference, state, inc, window, max_split, active=None, L_dir=None):
        """(count uint32, scale, L_dir); `state` advances in place by ONE draw per active lane.  L_dir: estimate()'s, where the
        caller has it already."""
        n = np.asarray(p).shape[1]
        act = np.ones(n, bool) if active is None else np.asarray(active) != 0
        if L_dir is None:
            L_dir, _ = self.estimate(p, direction, active)
        st = np.ascontiguousarray(state[act])
        xi_act = po.rng_next_f32(st, np.ascontiguousarray(inc[act]))
        state[act] = st
        xi = np.zeros(n, np.float32)
        xi[act] = xi_act
        count, scale = decide(L_dir, weight, reference, xi, window, max_split, self.T)
        count = np.where(act, count, 1).astype(np.uint32)
        scale = np.where(act, scale, self.T(1)).astype(self.T)
        return count, scale, L_dir


def decide(L, w, I, xi, window, max_split, ftype=np.float32):
    """count, scale of the lanes (all taken as active), branch by branch as pgsd_radiance.h lists them."""
    T = ftype
    L, w, I, xi = (np.asarray(a).astype(T) for a in (L, w, I, xi))
    lo, hi = rr_window(window, T)
    n = L.shape[0]
    count = np.ones(n, np.uint32)
    scale = np.ones(n, T)
    with np.errstate(all="ignore"):
        opinion = (L > 0) & (w > 0) & (I > 0) & np.isfinite(L) & np.isfinite(w) & np.isfinite(I)
        q = ((w * L).astype(T) / I).astype(T)
        opinion &= np.isfinite(q)
        rou = opinion & (q < lo)
        P = (q / lo).astype(T)
        survive = xi < P
        count = np.where(rou, np.where(survive, 1, 0), count).astype(np.uint32)
        scale = np.where(rou, np.where(survive, (lo / q).astype(T), T(0)), scale).astype(T)
        spl = opinion & ~rou & (q > hi) & (int(max_split) > 1)
        r = np.minimum((q / hi).astype(T), T(max_split)).astype(T)
        r = np.where(spl, r, T(1)).astype(T)
        k = np.floor(r).astype(T)
        extra = xi < (r - k).astype(T)
        count = np.where(spl, k.astype(np.uint32) + extra.astype(np.uint32), count).astype(np.uint32)
        scale = np.where(spl, (T(1) / r).astype(T), scale).astype(T)
    return count, scale


def grid_directions(k=7):
    """Directions (3, M), not normalised, whose canonical coordinates are exact multiples of 2^-k: the edges and corners of the
    quadtrees' cells, where the tie rule decides and the jump tables are missed.  cy = (z + 1) / 2 is exact for z = 2 cy - 1.
    cx = atan2(y, x) / 2 pi is exact on the axes; for the other multiples (x, y) = (cos, sin) of the angle is searched a few
    ulps of y around for a pair that dirToCanonical maps onto the multiple exactly (the targets without one are left out)."""
    G = 1 << k
    xs = [(1.0, 0.0)]
    for j in range(1, G):
        a = 2.0 * np.pi * j / G
        dx = np.float32(np.cos(a))
        cand = [np.float32(np.sin(a))]
        for _ in range(8):
            cand = [np.nextafter(cand[0], np.float32(-2))] + cand + [np.nextafter(cand[-1], np.float32(2))]
        d = np.array([[dx] * len(cand), cand, [0.0] * len(cand)], np.float32)
        hit = np.nonzero(po.dir_to_canonical(d)[0] == np.float32(j / G))[0]
        if hit.size:
            xs.append((float(dx), float(cand[hit[0]])))
    xs = np.array(xs, np.float32)
    z = (2.0 * np.arange(G + 1) / G - 1.0).astype(np.float32)
    out = np.empty((3, xs.shape[0] * z.shape[0]), np.float32)
    out[0] = np.repeat(xs[:, 0], z.shape[0])
    out[1] = np.repeat(xs[:, 1], z.shape[0])
    out[2] = np.tile(z, xs.shape[0])
    return out


def corner_records(m, seed, bbox_min, bbox_max, radiance=None):
    """synth.records with the positions drawn towards the bbox_min corner (the product of two uniforms per axis: 61 % of them
    fall into the corner's octant, 0.3 % into the opposite one), so that a refine splits some KD leaves several times and
    others not at all.  radiance: a constant field seen through uniformly drawn directions (wo_pdf = 1 / (4 pi), no emitter
    deposit) instead of synth.records' values."""
    import synth
    rec = synth.records(m, seed, bbox_min, bbox_max)
    u = synth.uniform(m, seed + 7, 6)
    lo = np.asarray(bbox_min, np.float32)[:, None]
    hi = np.asarray(bbox_max, np.float32)[:, None]
    rec["position"] = (lo + (u[0:3] * u[3:6]).astype(np.float32) * (hi - lo)).astype(np.float32)
    if radiance is not None:
        rec["direction"] = synth.canonical_uniform(m, seed + 8)
        rec["radiance"] = np.full(m, radiance, np.float32)
        rec["woPdf"] = np.full(m, INV_FOUR_PI, np.float32)
        rec["radiance_nee_lum"] = np.zeros(m, np.float32)
    return rec


# ---- the weights a refine carries, derived without the library -------------------------------------------------------------
def source_leaves(old_cols, new_cols):
    """(leaf, tree, source): the KD leaves of the refined tree, their quadtrees, and for each the leaf of the tree BEFORE the
    refine whose box contains its box (found through the box's centre, the matching of tests/test_gpu_fraction.py)."""
    def leaves(c):
        i = np.nonzero(np.asarray(c["kdtree_isLeaf"], bool))[0]
        return (i, np.asarray(c["kdtree_bbox_min"], np.float64).reshape(-1, 3)[i], np.asarray(c["kdtree_bbox_max"], np.float64).reshape(-1, 3)[i])
    oi, omin, omax = leaves(old_cols)
    ni, nmin, nmax = leaves(new_cols)
    centre = (nmin + nmax) / 2
    src = np.empty(ni.shape[0], np.int64)
    for a in range(0, ni.shape[0], 512):            # (in slices: leaves x leaves booleans)
        c = centre[a:a + 512]
        inside = ((c[:, None, :] >= omin[None]) & (c[:, None, :] <= omax[None])).all(axis=2)
        assert (inside.sum(axis=1) == 1).all()
        k = inside.argmax(axis=1)
        assert (nmin[a:a + 512] >= omin[k]).all() and (nmax[a:a + 512] <= omax[k]).all()
        src[a:a + 512] = oi[k]
    tree = np.asarray(new_cols["kdtree_quadTreeRootIndex"], np.int64)[ni]
    assert np.array_equal(np.sort(tree), np.arange(np.asarray(new_cols["quadtree_rootNodeIndex"]).shape[0]))   # one leaf per quadtree
    return ni, tree, src


def carried_weights(old_cols, old_kd_count, new_cols):
    """weight of every quadtree of the refined tree: a new KD leaf takes the integer record count (kd_column("count") of the
    tree BEFORE the refine, per KD node) of the old leaf it comes from."""
    _, tree, src = source_leaves(old_cols, new_cols)
    w = np.zeros(tree.shape[0], np.uint64)
    w[tree] = np.asarray(old_kd_count, np.uint64)[src]
    return w


def splits_between(old_cols, new_cols):
    """Per quadtree of the refined tree: how many KD splits lie between its leaf and the old leaf it comes from."""
    leaf, tree, src = source_leaves(old_cols, new_cols)
    out = np.zeros(tree.shape[0], np.int64)
    out[tree] = np.asarray(new_cols["kdtree_depth"], np.int64)[leaf] - np.asarray(old_cols["kdtree_depth"], np.int64)[src]
    return out
