"""A numpy model of the learned light selection, written from include/ext/pg_lights.h (not from the kernels).

Test infrastructure.  One float32 numpy operation per operation the header writes, vectorised over lanes, records or lights; the
sums are Python ints.  The parts the oracle already defines come from it: quantize and acc_to_float as they are, the PCG32
stream, and the KD leaf of a position (get_leaf_node_index on the tree whose exported columns the model reads, as
tests/fraction_model.py does).  SELECT and PMF are module functions on a table of rows, so that the CPU tests can walk a single
row without a tree.
"""
from __future__ import annotations

import numpy as np

from oracle import pg_oracle as po

F = np.float32
NONE = 0xFFFFFFFF
WEIGHT_ONE = 65536
MAX_LIGHTS = 4096


# ---- SELECT and PMF of the header, on rows[n_leaves, L]; leaf[i] = -1: no leaf (outside the root box) ---------------------------
def sanitize(u):
    u = np.asarray(u, F)
    with np.errstate(invalid="ignore"):
        ok = (u >= F(0)) & (u < F(1))
    return np.where(ok, u, F(0)).astype(F)


def _K(rows, leaf):
    L = rows.shape[1]
    return np.where(leaf >= 0, rows[np.maximum(leaf, 0), L - 1], 0).astype(np.uint32)


def select(rows, leaf, u, delta):
    """(j uint32, took the tree branch) of SELECT for every lane; u as given (it is sanitised here)."""
    rows = np.asarray(rows, np.uint32)
    leaf = np.asarray(leaf, np.int64)
    L = rows.shape[1]
    Lf, delta = F(L), F(delta)
    u = sanitize(u)
    K = _K(rows, leaf)
    j = np.zeros(u.shape[0], np.uint32)
    un = K == 0
    j[un] = np.minimum((u[un] * Lf).astype(F).astype(np.uint32), L - 1)
    ub = ~un & (u < delta)
    j[ub] = np.minimum(((u[ub] / delta).astype(F) * Lf).astype(F).astype(np.uint32), L - 1)
    tb = ~un & ~ub
    if tb.any():
        v = ((u[tb] - delta).astype(F) / (F(1) - delta)).astype(F)
        t = np.minimum((v * F(16777216)).astype(F).astype(np.uint64), np.uint64(16777215))
        x = (t * K[tb].astype(np.uint64)) >> np.uint64(24)
        lf = leaf[tb]
        jt = np.zeros(x.shape[0], np.uint32)
        for l in np.unique(lf):
            sel = lf == l
            jt[sel] = np.searchsorted(rows[l].astype(np.uint64), x[sel], side="right")     # the smallest index with C[j] > x
        j[tb] = jt
    return j, tb


def pmf(rows, leaf, j, delta):
    rows = np.asarray(rows, np.uint32)
    leaf = np.asarray(leaf, np.int64)
    j = np.asarray(j, np.uint32).astype(np.int64)
    L = rows.shape[1]
    delta, invL = F(delta), F(1) / F(L)
    K = _K(rows, leaf)
    valid = j < L
    jj, ll = np.where(valid, j, 0), np.maximum(leaf, 0)
    k = (rows[ll, jj].astype(np.int64) - np.where(jj > 0, rows[ll, np.maximum(jj - 1, 0)], 0).astype(np.int64)).astype(np.uint32)
    with np.errstate(all="ignore"):
        share = (k.astype(F) / K.astype(F)).astype(F)
        learned = ((delta * invL).astype(F) + ((F(1) - delta) * share).astype(F)).astype(F)
    out = np.where(K == 0, invL, learned).astype(F)
    return np.where(valid, out, F(0)).astype(F)


def weights(row):
    row = np.asarray(row, np.uint32).astype(np.int64)
    return np.diff(row, prepend=0)


def build_row(T, count, root):
    """BUILD of the header for one leaf: T and count are lists of Python ints (one per light).  None: the leaf keeps its row."""
    L = len(T)
    has = np.array([c > 0 for c in count], bool)
    m = np.zeros(L, F)
    if has.any():
        idx = np.nonzero(has)[0]
        lo = np.array([T[i] & 0xffffffffffffffff for i in idx], np.uint64)
        hi = np.array([T[i] >> 64 for i in idx], np.int64)
        cnt = np.array([F(count[i]) for i in idx], F)
        with np.errstate(all="ignore"):
            m[idx] = (po.acc_to_float(lo, hi) / cnt).astype(F)
    with np.errstate(all="ignore"):
        if root:
            m = np.sqrt(m).astype(F)
        m = np.where(np.isfinite(m) & (m > 0), m, F(0)).astype(F)
    M = m.max()
    if not M > 0:
        return None
    k = ((m / M).astype(F) * F(65536)).astype(F).astype(np.uint32)
    return np.cumsum(k.astype(np.uint64)).astype(np.uint32)


def limb_words(value):
    """quantize(value) of non-negative values as the three words the header adds: (q >> 32 k) mod 2^32, word 2 unmasked (int64)."""
    lo, hi = po.quantize(np.ascontiguousarray(value, F))
    return (lo & np.uint64(0xffffffff)).astype(np.int64), (lo >> np.uint64(32)).astype(np.int64), hi.astype(np.int64)


class LightsModel:
    def __init__(self, tree, n_lights, delta=0.1, root=False):
        assert 1 <= n_lights <= MAX_LIGHTS
        self.tree = tree
        c = tree.export()
        self.kd_tree = c["kdtree_quadTreeRootIndex"].astype(np.int64)
        self.bmin, self.bmax = c["kdtree_bbox_min"][0].astype(F), c["kdtree_bbox_max"][0].astype(F)
        self.n = int(c["quadtree_rootNodeIndex"].shape[0])
        self.L, self.delta, self.root = int(n_lights), F(delta), bool(root)
        self.rows = np.zeros((self.n, self.L), np.uint32)
        self._zero_acc()

    def _zero_acc(self):
        self.acc = np.zeros((self.n * self.L, 4), dtype=object)    # Python ints
        self.acc[:] = 0

    # ---- state ------------------------------------------------------------------------------------------------------------
    def state(self):
        return {"rows": self.rows.copy(), "acc": self.acc_words()}

    def load_state(self, st):
        rows = np.array(st["rows"], np.uint32)
        assert rows.shape == (self.n, self.L)
        self.rows = rows
        self._zero_acc()

    def acc_words(self):
        return self.acc.astype(np.int64).reshape(self.n, self.L, 4)

    def add_words(self, words):
        """Element-wise sum of another rank's buffer into this one (what ranks do before the build)."""
        w = np.asarray(words, np.int64).reshape(self.n * self.L, 4)
        nz = np.nonzero(w.any(axis=1))[0]
        for e in nz:
            for k in range(4):
                self.acc[e, k] += int(w[e, k])

    def learned_leaves(self):
        return int((self.rows[:, -1] != 0).sum())

    # ---- the KD leaf ------------------------------------------------------------------------------------------------------
    def inside(self, p):
        with np.errstate(invalid="ignore"):
            return ((p >= self.bmin[:, None]) & (p <= self.bmax[:, None])).all(axis=0)

    def leaf_of(self, p, inside):
        """the leaf of every position, -1 where it is not inside"""
        q = np.where(inside[None, :], p, self.bmin[:, None]).astype(F)   # (lanes outside are not looked up: any inside point)
        leaf = self.kd_tree[self.tree.get_leaf_node_index(np.ascontiguousarray(q)).astype(np.int64)]
        return np.where(inside, leaf, -1)

    # ---- SAMPLE and PMF ---------------------------------------------------------------------------------------------------
    def sample(self, p, u=None, rng_state=None, rng_inc=None, active=None):
        """(light uint32, pmf float32); with u None the streams (numpy uint64 arrays) are advanced in place on active lanes."""
        p = np.asarray(p, F)
        n = p.shape[1]
        act = np.ones(n, bool) if active is None else np.asarray(active) != 0
        if u is None:
            idx = np.nonzero(act)[0]
            st, inc = np.ascontiguousarray(rng_state[idx]), np.ascontiguousarray(rng_inc[idx])
            drawn = po.rng_next_f32(st, inc)
            rng_state[idx] = st
            u = np.zeros(n, F)
            u[idx] = drawn
        leaf = self.leaf_of(p, self.inside(p))
        j, _ = select(self.rows, leaf, u, self.delta)
        pm = pmf(self.rows, leaf, j, self.delta)
        return np.where(act, j, np.uint32(NONE)).astype(np.uint32), np.where(act, pm, F(0)).astype(F)

    def pmf(self, p, light, active=None):
        p = np.asarray(p, F)
        act = np.ones(p.shape[1], bool) if active is None else np.asarray(active) != 0
        pm = pmf(self.rows, self.leaf_of(p, self.inside(p)), light, self.delta)
        return np.where(act, pm, F(0)).astype(F)

    # ---- RECORD -----------------------------------------------------------------------------------------------------------
    def kept(self, rec, count=None):
        p = np.asarray(rec["position"], F)
        light = np.asarray(rec["light"]).astype(np.uint32)
        value = np.asarray(rec["value"], F)
        ins = self.inside(p)
        with np.errstate(invalid="ignore"):
            keep = ins & (light < self.L) & np.isfinite(value) & (value >= 0)
        if count is not None:
            keep &= np.arange(p.shape[1]) < int(count)
        return keep, self.leaf_of(p, ins), light, value

    def record(self, rec, count=None):
        keep, leaf, light, value = self.kept(rec, count)
        idx = np.nonzero(keep)[0]
        key = leaf[idx] * self.L + light[idx].astype(np.int64)
        w0, w1, w2 = limb_words(value[idx])
        # (a batch's words in int64: fewer than 2^31 records of less than 2^32 each; what they are added to are Python ints)
        assert idx.size < (1 << 31) and (w2 < (1 << 32)).all()
        batch = np.zeros((self.n * self.L, 4), np.int64)
        for k, w in enumerate((w0, w1, w2, np.ones(idx.size, np.int64))):
            np.add.at(batch[:, k], key, w)
        for e in np.unique(key):
            for k in range(4):
                self.acc[e, k] += int(batch[e, k])
        return keep

    # ---- BUILD ------------------------------------------------------------------------------------------------------------
    def build(self):
        """returns the number of leaves whose row was written"""
        built = 0
        acc = self.acc.reshape(self.n, self.L, 4)
        for t in range(self.n):
            a = acc[t]
            count = [int(c) for c in a[:, 3]]
            if not any(c > 0 for c in count):
                continue
            T = [int(a[j, 0]) + (int(a[j, 1]) << 32) + (int(a[j, 2]) << 64) for j in range(self.L)]
            row = build_row(T, count, self.root)
            if row is not None:
                self.rows[t] = row
                built += 1
        return built


# ---- record sets shared by the CPU and the GPU tests ------------------------------------------------------------------------
def synthetic_records(m, seed, bbox_min, bbox_max, n_lights, position=None, light=None):
    """m records with uniform positions (or all at `position`) and lights (or all `light`); a light's values are scaled by a
    factor that falls off with its index, a third of them are zero (occluded)."""
    import synth
    p = synth.positions_uniform(m, seed, bbox_min, bbox_max)
    if position is not None:
        p[:] = np.asarray(position, F)[:, None]
    u = synth.uniform(m, seed + 1, 3)
    lt = np.minimum((u[0] * F(n_lights)).astype(np.uint32), n_lights - 1)
    if light is not None:
        lt[:] = light
    scale = np.ldexp(F(1), -(lt % 12).astype(np.int32)).astype(F)
    value = np.where(u[2] < F(1 / 3), F(0), (F(0.01) + F(4) * u[1]) * scale).astype(F)
    return {"position": p, "light": lt.astype(np.uint32), "value": value}


EDGE_KINDS = ("light == n_lights", "light huge", "negative", "nan value", "inf value", "negative inf", "outside", "nan position",
              "above the clamp", "zero", "negative zero", "denormal", "on the box face", "last light")
EDGE_DROPPED = EDGE_KINDS[:8]


def salt_with_edges(rec, bbox_min, bbox_max, n_lights, stride=5):
    """Every `stride`-th record becomes one of EDGE_KINDS in turn; returns the kind of every record ('' = untouched)."""
    m = rec["value"].shape[0]
    kinds = np.array([""] * m, dtype=object)
    lo, hi = F(bbox_min[0]), F(bbox_max[0])
    for j, i in enumerate(range(3, m, stride)):
        k = EDGE_KINDS[j % len(EDGE_KINDS)]
        kinds[i] = k
        if k == "light == n_lights": rec["light"][i] = n_lights
        elif k == "light huge": rec["light"][i] = 0xFFFFFFFF if j % 2 else 0x80000000
        elif k == "negative": rec["value"][i] = -1e-3
        elif k == "nan value": rec["value"][i] = np.nan
        elif k == "inf value": rec["value"][i] = np.inf
        elif k == "negative inf": rec["value"][i] = -np.inf
        elif k == "outside": rec["position"][j % 3, i] = np.nextafter(hi, F(np.inf)) if j % 2 else F(lo - F(1e-3))
        elif k == "nan position": rec["position"][j % 3, i] = np.nan
        elif k == "above the clamp": rec["value"][i] = 3e38
        elif k == "zero": rec["value"][i] = 0.0
        elif k == "negative zero": rec["value"][i] = -0.0
        elif k == "denormal": rec["value"][i] = 1e-40
        elif k == "on the box face": rec["position"][j % 3, i] = hi if j % 2 else lo
        elif k == "last light": rec["light"][i] = n_lights - 1
    return kinds
