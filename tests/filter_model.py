"""A numpy model of the training filters of pg_set_splat_filter, written from include/pgsd.h (the section "training
filters of the record boundary"), over the exported columns of an SD-tree (SDTree.export() / OracleTree.export()).

Test infrastructure.  Every fp32 operation the header names is one float32 numpy operation here, in the header's order;
sums are exact integers.  The result names, per canonical quadtree node, the exact sum of the deposits in units of
2^-40 (inner nodes: the sum of their leaves) and, per KD node, the number of counted records -- what
SDTree.exportAccumulators() returns.
"""
from __future__ import annotations

import numpy as np

from oracle import pg_oracle as po

F = np.float32


def _kd_leaf(c, p, search):
    """KDTree.getLeafNodeIndex over the columns: node of every p (3, n) with search[i]; 0 elsewhere."""
    n = p.shape[1]
    leaf = np.asarray(c["kdtree_isLeaf"], bool)
    L, R = c["kdtree_child_left_index"].astype(np.int64), c["kdtree_child_right_index"].astype(np.int64)
    depth, bmin = c["kdtree_depth"].astype(np.int64), c["kdtree_bbox_min"]
    node = np.zeros(n, np.int64)
    idx = np.nonzero(search & ~leaf[0])[0]
    while idx.size:
        nd = node[idx]
        axis = depth[nd] % 3
        split = bmin[R[nd], axis]          # the children meet at the parent's midpoint
        node[idx] = np.where(p[axis, idx] >= split, R[nd], L[nd])
        idx = idx[~leaf[node[idx]]]
    return node


def _children(c):
    return np.stack([c["quadtree_child_%d_index" % k].astype(np.int64) for k in (1, 2, 3, 4)])


def _quad_leaf(c, ch, root, cx, cy):
    """addIrradiancePropagate's descent: the highest-numbered child whose closed cell holds the point."""
    leaf = np.asarray(c["quadtree_isLeaf"], bool)
    qmin = c["quadtree_bbox_min"]
    node = root.copy()
    idx = np.nonzero(~leaf[node])[0]
    while idx.size:
        nd = node[idx]
        mid = qmin[ch[0][nd]]               # child 1 is the (+x, +y) quadrant: its lower corner is the midpoint
        x, y = cx[idx], cy[idx]
        xge, xle, yge, yle = x >= mid[:, 0], x <= mid[:, 0], y >= mid[:, 1], y <= mid[:, 1]
        j = np.where(xge & yle, 3, np.where(xle & yle, 2, np.where(xle & yge, 1, 0)))
        node[idx] = ch[j, nd]
        idx = idx[~leaf[node[idx]]]
    return node


class _Sums:
    """Exact sums of signed 128-bit deposits per node: limbs lo & 2^32-1, lo >> 32 (unsigned) and hi (signed)."""

    def __init__(self, n):
        self.l = np.zeros((4, n), np.int64)    # (row 3: the number of deposits)
        self.deposits = 0

    def add(self, node, w):
        if node.size == 0:
            return
        lo, hi = po.quantize(np.ascontiguousarray(w, F))
        self.deposits += int(node.size)
        order = np.argsort(node, kind="stable")
        ns = node[order]
        first = np.nonzero(np.r_[True, ns[1:] != ns[:-1]])[0]
        for k, v in enumerate(((lo & np.uint64(0xFFFFFFFF)).astype(np.int64), (lo >> np.uint64(32)).astype(np.int64), hi,
                               np.ones(node.size, np.int64))):
            self.l[k, ns[first]] += np.add.reduceat(v[order], first)


def _box_pairs(c, ch, S, root, N, cx, cy, w):
    """PG_DIRECTIONAL_BOX for pairs whose nearest leaf N lies below the root (d >= 1) and whose quantize(w) is not zero."""
    leaf = np.asarray(c["quadtree_isLeaf"], bool)
    qdepth = c["quadtree_depth"].astype(np.int64)
    d = qdepth[N] - qdepth[root]
    G = np.ldexp(F(1), d.astype(np.int32)).astype(F)
    Gi = np.int64(1) << d
    vx = (cx * G).astype(F) - F(0.5)
    fjx = np.floor(vx)
    tx = (vx - fjx).astype(F)
    X0 = fjx.astype(np.int64) & (Gi - 1)
    vy = np.maximum((cy * G).astype(F) - F(0.5), F(0))
    fjy = np.floor(vy)
    ty = (vy - fjy).astype(F)
    jy = fjy.astype(np.int64)
    top = jy >= Gi - 1
    jy = np.where(top, Gi - 1, jy)
    ty = np.where(top, F(0), ty).astype(F)
    X1, Y0, Y1 = (X0 + 1) & (Gi - 1), jy, jy + 1
    wid = [[(F(1) - tx).astype(F), tx], [(F(1) - ty).astype(F), ty]]    # hx - lx of column 0 / 1, hy - ly of row 0 / 1
    for qb in (0, 1):
        for qa in (0, 1):
            fa, fb = wid[0][qa], wid[1][qb]
            it = np.nonzero((fa > 0) & (fb > 0))[0]
            if it.size == 0:
                continue
            X, Y = (X1 if qa else X0)[it], (Y1 if qb else Y0)[it]
            di = d[it]
            node = root[it].copy()
            for lv in range(int(di.max())):                            # the node of cell (X, Y) at depth d, or the leaf above it
                go = np.nonzero((lv < di) & ~leaf[node])[0]
                if go.size == 0:
                    break
                bit = di[go] - 1 - lv
                xh, yh = (X[go] >> bit) & 1, (Y[go] >> bit) & 1
                j = np.where(yh == 1, np.where(xh == 1, 0, 1), np.where(xh == 1, 3, 2))
                node[go] = ch[j, node[go]]
            is_leaf = leaf[node]
            # a leaf at depth <= d: one deposit, made when its first cell of the block is opened
            k = np.nonzero(is_leaf)[0]
            ik = it[k]
            sh = di[k] - (qdepth[node[k]] - qdepth[root[ik]])
            col_merge = (wid[0][1 - qa][ik] > 0) & ((X0[ik] >> sh) == (X1[ik] >> sh))
            row_merge = (wid[1][1 - qb][ik] > 0) & ((Y0[ik] >> sh) == (Y1[ik] >> sh))
            keep = ~((col_merge & bool(qa)) | (row_merge & bool(qb)))
            ox = np.where(col_merge, F(1), fa[ik]).astype(F)
            oy = np.where(row_merge, F(1), fb[ik]).astype(F)
            S.add(node[k][keep], (w[ik] * (ox * oy).astype(F)).astype(F)[keep])
            # a subdivided cell: every leaf below it that meets the footprint, in the cell's own frame
            k = np.nonzero(~is_leaf)[0]
            ik = it[k]
            fr_item, fr_node = ik, node[k]
            fr_u = np.zeros(k.size, F)
            fr_v = np.zeros(k.size, F)
            h = F(1)
            lx, hx = (np.zeros_like(tx), tx) if qa else (tx, np.ones_like(tx))
            ly, hy = (np.zeros_like(ty), ty) if qb else (ty, np.ones_like(ty))
            while fr_item.size:
                h = F(h * F(0.5))
                nxt = [[], [], [], []]
                for j in range(4):
                    u0 = (fr_u + h).astype(F) if j in (0, 3) else fr_u
                    v0 = (fr_v + h).astype(F) if j in (0, 1) else fr_v
                    ox = (np.minimum((u0 + h).astype(F), hx[fr_item]) - np.maximum(u0, lx[fr_item])).astype(F)
                    oy = (np.minimum((v0 + h).astype(F), hy[fr_item]) - np.maximum(v0, ly[fr_item])).astype(F)
                    hit = (ox > 0) & (oy > 0)
                    cn = ch[j, fr_node]
                    lf = hit & leaf[cn]
                    S.add(cn[lf], (w[fr_item[lf]] * (ox[lf] * oy[lf]).astype(F)).astype(F))
                    inner = hit & ~leaf[cn]
                    for a, v in zip(nxt, (fr_item[inner], cn[inner], u0[inner], v0[inner])):
                        a.append(v)
                fr_item, fr_node, fr_u, fr_v = (np.concatenate(a) for a in nxt)


def splat(cols, rec, spatial="nearest", directional="nearest", seed=0, store_nee=True, index=None):
    """The accumulators one pg_splat of `rec` (synth.records' keys, planar) leaves on a reset tree with columns `cols`.
    index: the record numbers of the jitter's streams (default: 0 .. m-1, pg_splat's; the dense slots for pg_process_and_splat).
    Returns a dict: kd_count (n_kd,) uint64, units (n_quad,) Python ints (object array), lo / hi (the same as 128-bit
    two's complement halves), deposits_below (n_quad,) deposits made at or below each node, count_leaf (n_kd,) counted records per KD leaf, deposits (number of quantised deposits made),
    kd_leaf (m,) the KD leaf every record went to, inside (m,)."""
    assert spatial in ("nearest", "stochastic") and directional in ("nearest", "box")
    c = cols
    p = np.ascontiguousarray(rec["position"], F).copy()
    m = p.shape[1]
    rmin, rmax = c["kdtree_bbox_min"][0].astype(F), c["kdtree_bbox_max"][0].astype(F)
    inside = np.ones(m, bool)
    for a in range(3):
        inside &= (p[a] >= rmin[a]) & (p[a] <= rmax[a])
    if spatial == "stochastic":
        L = _kd_leaf(c, p, inside)
        e = (c["kdtree_bbox_max"][L] - c["kdtree_bbox_min"][L]).astype(F)       # (m, 3)
        idx = np.arange(m, dtype=np.int64) if index is None else np.asarray(index, np.int64) & 0xFFFFFFFF
        st, inc = po.rng_seed(int(idx.max()) + 1 if m else 0, seed & 0xFFFFFFFF, 0)
        for a in range(3):
            u = po.rng_next_f32(st, inc)[idx]
            v = (p[a] + ((u - F(0.5)).astype(F) * e[:, a]).astype(F)).astype(F)
            v = np.minimum(np.maximum(v, rmin[a]), rmax[a]).astype(F)
            p[a] = np.where(inside, v, p[a])
    kd = _kd_leaf(c, p, inside)
    n_kd, n_q = c["kdtree_depth"].shape[0], c["quadtree_depth"].shape[0]
    count_leaf = np.bincount(kd[inside], minlength=n_kd).astype(np.uint64)
    tree = c["kdtree_quadTreeRootIndex"].astype(np.int64)[kd]    # outside the box: node 0's (stale) tree
    root = c["quadtree_rootNodeIndex"].astype(np.int64)[tree]
    ch = _children(c)
    qdepth = c["quadtree_depth"].astype(np.int64)
    S = _Sums(n_q)
    wp = np.asarray(rec["woPdf"], F)
    pairs = [(rec["direction"], rec["radiance"])]
    if store_nee:
        pairs.append((rec["direction_nee"], rec["radiance_nee_lum"]))
    with np.errstate(all="ignore"):
        for dirs, val in pairs:
            cx, cy = np.asarray(dirs[0], F), np.asarray(dirs[1], F)
            w = np.where(wp > 0, (np.asarray(val, F) / wp).astype(F), F(0)).astype(F)
            ok = (cx >= 0) & (cx <= 1) & (cy >= 0) & (cy <= 1)
            i = np.nonzero(ok)[0]
            N = _quad_leaf(c, ch, root[i], cx[i], cy[i])
            if directional == "box":
                lo, hi = po.quantize(w[i])
                box = (qdepth[N] > qdepth[root[i]]) & ((lo != 0) | (hi != 0))
            else:
                box = np.zeros(i.size, bool)
            S.add(N[~box], w[i][~box])
            b = i[box]
            if b.size:
                _box_pairs(c, ch, S, root[b], N[box], cx[b], cy[b], w[b])
    # inner nodes: the sums of their children, bottom-up
    leaf = np.asarray(c["quadtree_isLeaf"], bool)
    for lv in range(int(qdepth.max()) - 1, -1, -1):
        sel = np.nonzero((qdepth == lv) & ~leaf)[0]
        S.l[:, sel] = S.l[:, ch[0][sel]] + S.l[:, ch[1][sel]] + S.l[:, ch[2][sel]] + S.l[:, ch[3][sel]]
    units = S.l[0].astype(object) + (S.l[1].astype(object) << 32) + (S.l[2].astype(object) << 64)
    lo = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in units], np.uint64)
    hi = np.array([int(v) >> 64 for v in units], np.int64)
    kd_count = count_leaf.copy()
    kleaf = np.asarray(c["kdtree_isLeaf"], bool)
    kdep = c["kdtree_depth"].astype(np.int64)
    KL, KR = c["kdtree_child_left_index"].astype(np.int64), c["kdtree_child_right_index"].astype(np.int64)
    for lv in range(int(kdep.max()) - 1, -1, -1):
        sel = np.nonzero((kdep == lv) & ~kleaf)[0]
        kd_count[sel] = kd_count[KL[sel]] + kd_count[KR[sel]]
    return {"kd_count": kd_count, "units": units, "lo": lo, "hi": hi, "count_leaf": count_leaf, "deposits": S.deposits,
            "deposits_below": S.l[3].copy(),
            "kd_leaf": kd, "inside": inside, "position": p}
