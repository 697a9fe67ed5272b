"""A numpy model of PG_SPATIAL_OVERLAP_BOX, the deterministic spatial box filter of pg_set_splat_filter, written from
include/pgsd.h (the section "training filters of the record boundary"), over the exported columns of an SD-tree.

Test infrastructure, beside tests/filter_model.py (whose helpers it uses, and whose splat() it matches in what it returns).
Every fp32 operation the header names is one float32 numpy operation here, in the header's order; sums are exact integers.
The KD leaves under a record's box are found by a descent that enters a node only if the node's own box passes the header's
test (len[a] > 0 on the three axes): the box of a leaf lies inside the boxes of the nodes above it, so no leaf that takes part
is missed, and the test that admits a leaf is the header's, made on the leaf's own columns.
"""
from __future__ import annotations

import numpy as np

import filter_model as fm
from oracle import pg_oracle as po

F = np.float32


def record_boxes(cols, p, inside):
    """L, e, lo, hi and the records the filter applies to (the others are handled as PG_SPATIAL_NEAREST); p is (3, m)."""
    bmin, bmax = cols["kdtree_bbox_min"].astype(F), cols["kdtree_bbox_max"].astype(F)
    rmin, rmax = bmin[0], bmax[0]
    L = fm._kd_leaf(cols, p, inside)
    with np.errstate(all="ignore"):
        e = (bmax[L] - bmin[L]).astype(F)                                   # (m, 3)
        filt = inside & (L != 0) & np.isfinite(e).all(axis=1) & (e > 0).all(axis=1)
        pt = np.ascontiguousarray(p.T, F)
        lo = np.maximum((pt - (F(0.5) * e).astype(F)).astype(F), rmin)
        hi = (lo + e).astype(F)
        over = hi > rmax
        hi = np.where(over, rmax, hi).astype(F)
        lo = np.where(over, np.maximum((hi - e).astype(F), rmin), lo).astype(F)
    return L, e, lo, hi, filt


def _lens(bmin, bmax, node, lo, hi):
    return (np.minimum(bmax[node], hi) - np.maximum(bmin[node], lo)).astype(F)


def leaves_under(cols, item, e, lo, hi):
    """Every (record, KD leaf M) pair that takes part, with its share s: arrays (item, M, s) over the records `item`."""
    bmin, bmax = cols["kdtree_bbox_min"].astype(F), cols["kdtree_bbox_max"].astype(F)
    leaf = np.asarray(cols["kdtree_isLeaf"], bool)
    kids = (cols["kdtree_child_left_index"].astype(np.int64), cols["kdtree_child_right_index"].astype(np.int64))
    out_i, out_m, out_s = [], [], []
    fr_i, fr_n = item.astype(np.int64), np.zeros(item.size, np.int64)
    while fr_i.size:
        at = leaf[fr_n]
        k = np.nonzero(at)[0]
        if k.size:
            i, m = fr_i[k], fr_n[k]
            ln = _lens(bmin, bmax, m, lo[i], hi[i])
            take = (ln > 0).all(axis=1)                                       # (a node passed the test to be entered)
            i, m, ln = i[take], m[take], ln[take]
            q = (ln / e[i]).astype(F)
            out_i.append(i)
            out_m.append(m)
            out_s.append(((q[:, 0] * q[:, 1]).astype(F) * q[:, 2]).astype(F))
        k = np.nonzero(~at)[0]
        nxt_i, nxt_n = [], []
        for side in kids:
            i, c = fr_i[k], side[fr_n[k]]
            go = (_lens(bmin, bmax, c, lo[i], hi[i]) > 0).all(axis=1)
            nxt_i.append(i[go])
            nxt_n.append(c[go])
        fr_i, fr_n = np.concatenate(nxt_i), np.concatenate(nxt_n)
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F)
    return np.concatenate(out_i), np.concatenate(out_m), np.concatenate(out_s)


def splat(cols, rec, directional="nearest", store_nee=True):
    """The accumulators one pg_splat of `rec` leaves on a reset tree with columns `cols` under ("overlap", directional).
    Returns filter_model.splat's dict (kd_leaf: the leaf L of every record) and, beside it, filtered (m,) the records the
    filter applied to, and item / leaf / share: the (record, KD leaf, s) triples of those records."""
    assert directional in ("nearest", "box")
    c = cols
    p = np.ascontiguousarray(rec["position"], F)
    m = p.shape[1]
    rmin, rmax = c["kdtree_bbox_min"][0].astype(F), c["kdtree_bbox_max"][0].astype(F)
    inside = np.ones(m, bool)
    for a in range(3):
        inside &= (p[a] >= rmin[a]) & (p[a] <= rmax[a])
    L, e, lo, hi, filt = record_boxes(c, p, inside)
    f_item, f_leaf, f_share = leaves_under(c, np.nonzero(filt)[0], e, lo, hi)
    rest = np.nonzero(~filt)[0]
    # one entry per (record, KD leaf) that receives the record's pairs; share None = the weight itself (nearest)
    item = np.concatenate([rest, f_item])
    kd = np.concatenate([L[rest], f_leaf])
    scaled = np.concatenate([np.zeros(rest.size, bool), np.ones(f_item.size, bool)])
    share = np.concatenate([np.ones(rest.size, F), f_share]).astype(F)
    n_kd, n_q = c["kdtree_depth"].shape[0], c["quadtree_depth"].shape[0]
    count_leaf = np.bincount(L[inside], minlength=n_kd).astype(np.uint64)      # the count: L alone
    tree = c["kdtree_quadTreeRootIndex"].astype(np.int64)[kd]
    root = c["quadtree_rootNodeIndex"].astype(np.int64)[tree]
    ch = fm._children(c)
    qdepth = c["quadtree_depth"].astype(np.int64)
    S = fm._Sums(n_q)
    wp = np.asarray(rec["woPdf"], F)
    pairs = [(rec["direction"], rec["radiance"])]
    if store_nee:
        pairs.append((rec["direction_nee"], rec["radiance_nee_lum"]))
    with np.errstate(all="ignore"):
        for dirs, val in pairs:
            cx, cy = np.asarray(dirs[0], F)[item], np.asarray(dirs[1], F)[item]
            w0 = np.where(wp > 0, (np.asarray(val, F) / wp).astype(F), F(0)).astype(F)[item]
            w = np.where(scaled, (w0 * share).astype(F), w0).astype(F)         # one product w * s
            ok = (cx >= 0) & (cx <= 1) & (cy >= 0) & (cy <= 1)
            i = np.nonzero(ok)[0]
            N = fm._quad_leaf(c, ch, root[i], cx[i], cy[i])
            if directional == "box":
                qlo, qhi = po.quantize(w[i])
                box = (qdepth[N] > qdepth[root[i]]) & ((qlo != 0) | (qhi != 0))
            else:
                box = np.zeros(i.size, bool)
            S.add(N[~box], w[i][~box])
            b = i[box]
            if b.size:
                fm._box_pairs(c, ch, S, root[b], N[box], cx[b], cy[b], w[b])
    leaf = np.asarray(c["quadtree_isLeaf"], bool)
    for lv in range(int(qdepth.max()) - 1, -1, -1):
        sel = np.nonzero((qdepth == lv) & ~leaf)[0]
        S.l[:, sel] = S.l[:, ch[0][sel]] + S.l[:, ch[1][sel]] + S.l[:, ch[2][sel]] + S.l[:, ch[3][sel]]
    units = S.l[0].astype(object) + (S.l[1].astype(object) << 32) + (S.l[2].astype(object) << 64)
    lo64 = np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in units], np.uint64)
    hi64 = np.array([int(v) >> 64 for v in units], np.int64)
    kd_count = count_leaf.copy()
    kleaf = np.asarray(c["kdtree_isLeaf"], bool)
    kdep = c["kdtree_depth"].astype(np.int64)
    KL, KR = c["kdtree_child_left_index"].astype(np.int64), c["kdtree_child_right_index"].astype(np.int64)
    for lv in range(int(kdep.max()) - 1, -1, -1):
        sel = np.nonzero((kdep == lv) & ~kleaf)[0]
        kd_count[sel] = kd_count[KL[sel]] + kd_count[KR[sel]]
    return {"kd_count": kd_count, "units": units, "lo": lo64, "hi": hi64, "count_leaf": count_leaf, "deposits": S.deposits,
            "deposits_below": S.l[3].copy(), "kd_leaf": L, "inside": inside, "position": p,
            "filtered": filt, "item": f_item, "leaf": f_leaf, "share": f_share}


def leaf_energy(cols, units):
    """The energy (units of 2^-40, Python ints) every KD node's quadtree received; 0 for inner KD nodes."""
    root = cols["quadtree_rootNodeIndex"].astype(np.int64)[cols["kdtree_quadTreeRootIndex"].astype(np.int64)]
    out = np.array([int(v) for v in units[root]], object)
    out[~np.asarray(cols["kdtree_isLeaf"], bool)] = 0
    return out
