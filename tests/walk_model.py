"""A numpy restatement of the walk through the four-wide BVH (csrc/pg_render_dev.hpp: bvh_node_step, bvh_leaf_step, bvh_pop),
all rays at once, in float32 with the device's operations: the padded slab test, Moeller-Trumbore, the five-comparator
network.  It walks the BVH only (no quads, spheres or boxes) and exists to state what the any-hit walk rests on; the device
is compared with the CPU oracle, not with this.

Two forms of the node step:
  ordered    the children the ray reaches sorted by entry distance, the nearest next, the others pushed with their distance,
             farthest first; a popped entry is dropped when the ray has become shorter than its distance
  unordered  the first child the ray reaches next, the later ones pushed as references alone, last first; nothing is dropped
             when popped
and two kinds of walk: closest hit (all of it) or any hit (over at the first leaf that holds a hit).
"""
import numpy as np

F = np.float32
NONE, LEAF = 0xffffffff, 0x80000000
PAD = F(1.0000004)


def _box_step(T, node, o, inv, neg, bt):
    """-> refs (k,4) with NONE where absent or missed, entry distances (k,4) with inf there"""
    planes = T.bvh[node, :24].view(np.float32).reshape(-1, 2, 3, 4)      # [lane][lo/hi][axis][child]
    refs = T.bvh[node, 24:28].astype(np.int64)
    k = node.shape[0]
    ax = np.arange(3)[None, :]
    near = planes[np.arange(k)[:, None], neg.astype(np.int64), ax]       # (k,3,4)
    far = planes[np.arange(k)[:, None], 1 - neg.astype(np.int64), ax]
    with np.errstate(invalid="ignore", over="ignore"):
        tn = (near - o[:, :, None]) * inv[:, :, None]
        tf = (far - o[:, :, None]) * inv[:, :, None]
        tmin = np.fmax(np.fmax(np.fmax(tn[:, 0], tn[:, 1]), tn[:, 2]), F(0))
        tmax = np.fmin(np.fmin(np.fmin(tf[:, 0], tf[:, 1]), tf[:, 2]), bt[:, None])
        hit = (tmin <= tmax * PAD) & (refs != NONE)
    return np.where(hit, refs, NONE), np.where(hit, tmin, F(np.inf)).astype(F)


def _tri_step(T, i, o, d, bt):
    """Moeller-Trumbore of triangle i for each lane -> accepted, t"""
    tr = T.tris[i].astype(F)
    v0, e1, e2 = tr[:, 0:3], tr[:, 3:6], tr[:, 6:9]
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    cross = lambda a, b: np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                   a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    with np.errstate(all="ignore"):
        p = cross(d, e2)
        det = dot(e1, p)
        inv_det = F(1) / det
        s = o - v0
        u = dot(s, p) * inv_det
        q = cross(s, e1)
        v = dot(d, q) * inv_det
        t = dot(e2, q) * inv_det
        ok = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > 0) & (t < bt)
    return ok, t.astype(F)


def walk(T, o, d, tmax, any_hit, ordered, depth=64):
    """-> best (n) triangle index or -1, bt (n), opened (n, nodes) bool: the nodes whose children were tested,
    leaves (n): how many leaf references the walk met"""
    o, d = np.asarray(o, F), np.asarray(d, F)
    n, nn = o.shape[0], T.bvh.shape[0]
    with np.errstate(divide="ignore"):
        inv = (F(1) / d).astype(F)
    neg = np.signbit(d)
    bt = np.asarray(tmax, F).copy()
    best = np.full(n, -1, np.int64)
    nxt = np.zeros(n, np.int64)                       # the root
    sp = np.zeros(n, np.int64)
    s_ref = np.full((n, depth), NONE, np.int64)
    s_t = np.zeros((n, depth), F)
    opened = np.zeros((n, nn), bool)
    leaves = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    for _ in range(16 * nn + 16):
        if not live.any():
            break
        at_node = live & (nxt != NONE) & ((nxt & LEAF) == 0)
        at_leaf = live & (nxt != NONE) & ((nxt & LEAF) != 0)
        popping = live & (nxt == NONE)
        k = np.nonzero(at_node)[0]
        if k.size:
            opened[k, nxt[k]] = True
            r, t = _box_step(T, nxt[k], o[k], inv[k], neg[k], bt[k])
            if ordered:
                def cswap(a, b):
                    sw = t[:, a] > t[:, b]
                    t[sw, a], t[sw, b] = t[sw, b], t[sw, a]
                    r[sw, a], r[sw, b] = r[sw, b], r[sw, a]
                for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
                    cswap(a, b)
                order = (3, 2, 1)
            else:
                first = (r != NONE).argmax(1)         # the first child the ray reaches (child 0, a NONE, where it reaches none)
                nxt_k = r[np.arange(k.size), first].copy()
                r[np.arange(k.size), first] = NONE
                r = np.concatenate([nxt_k[:, None], r[:, 1:]], 1)
                order = (3, 2, 1)
            for c in order:
                push = r[:, c] != NONE
                kk = k[push]
                s_ref[kk, sp[kk]] = r[push, c]
                s_t[kk, sp[kk]] = t[push, c]
                sp[kk] += 1
            nxt[k] = r[:, 0]
        k = np.nonzero(at_leaf)[0]
        if k.size:
            leaves[k] += 1
            first, count = nxt[k] & 0x0fffffff, ((nxt[k] >> 28) & 7) + 1
            for j in range(int(count.max())):
                m = j < count
                ok, t = _tri_step(T, (first + j)[m], o[k[m]], d[k[m]], bt[k[m]])
                kk = k[m][ok]
                bt[kk] = t[ok]
                best[kk] = (first + j)[m][ok]
            nxt[k] = NONE
            if any_hit:
                live[k[best[k] >= 0]] = False
        k = np.nonzero(popping)[0]
        if k.size:
            done = sp[k] == 0
            live[k[done]] = False
            k = k[~done]
            sp[k] -= 1
            ref = s_ref[k, sp[k]]
            if ordered:
                with np.errstate(invalid="ignore"):
                    keep = s_t[k, sp[k]] <= bt[k] * PAD
                ref = np.where(keep, ref, NONE)
            nxt[k] = ref
    assert not live.any(), "a walk did not end"
    return best, bt, opened, leaves
