"""A numpy model of the learned BSDF sampling fraction, written from include/pgsd_fraction.h (not from the kernels).

Test infrastructure.  One float32 numpy operation per operation the header writes, vectorised over records or leaves; the sums
are Python ints.  The parts the oracle already defines come from it: the library's exp (math1("exp", .)), quantize and
acc_to_float as they are, and the KD leaf of a position (get_leaf_node_index on the tree whose exported columns the model reads,
as tests/warp_model.py does).
"""
from __future__ import annotations

import numpy as np

from oracle import pg_oracle as po

F = np.float32
THETA_MAX = F(20)
LOSS_KL, LOSS_VARIANCE = 0, 1
DEFAULTS = dict(theta0=0.0, learning_rate=0.01, beta1=0.9, beta2=0.999, epsilon=1e-8, l2=0.01, loss=LOSS_KL)


def logistic(theta):
    theta = np.atleast_1d(np.asarray(theta, F))
    e = po.math1("exp", (F(0) - theta).astype(F))
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + e).astype(F)).astype(F)


def limbs(g):
    """quantize(g) of every gradient as the three words the header adds: sign(q) * ((|q| >> 32 k) mod 2^32), word 2 unmasked."""
    lo, hi = po.quantize(np.ascontiguousarray(g, F))
    out = []
    for l, h in zip(lo.tolist(), hi.tolist()):
        q = (h << 64) | l            # (hi is signed, lo unsigned: the two's complement value)
        s, a = (-1 if q < 0 else 1), abs(q)
        out.append((s * (a & 0xffffffff), s * ((a >> 32) & 0xffffffff), s * (a >> 64)))
    return out


class FractionModel:
    def __init__(self, tree, **params):
        prm = dict(DEFAULTS, **params)
        self.tree = tree
        c = tree.export()
        self.kd_tree = c["kdtree_quadTreeRootIndex"].astype(np.int64)
        self.bmin, self.bmax = c["kdtree_bbox_min"][0].astype(F), c["kdtree_bbox_max"][0].astype(F)
        self.n = n = int(c["quadtree_rootNodeIndex"].shape[0])
        self.loss = int(prm["loss"])
        self.theta0, self.lr, self.beta1, self.beta2, self.eps, self.l2 = (F(prm[k]) for k in (
            "theta0", "learning_rate", "beta1", "beta2", "epsilon", "l2"))
        self.theta = np.full(n, self.theta0, F)
        self.m, self.v = np.zeros(n, F), np.zeros(n, F)
        self.p1, self.p2 = np.ones(n, F), np.ones(n, F)
        self.steps = np.zeros(n, np.uint32)
        self.acc = [[0, 0, 0, 0] for _ in range(n)]     # Python ints

    # ---- state ------------------------------------------------------------------------------------------------------------
    def state(self):
        return {"theta": self.theta.copy(), "m": self.m.copy(), "v": self.v.copy(), "p1": self.p1.copy(), "p2": self.p2.copy(),
                "steps": self.steps.copy(), "acc": self.acc_words()}

    def load_state(self, st):
        for k in ("theta", "m", "v", "p1", "p2"):
            setattr(self, k, np.array(st[k], F))
        self.steps = np.array(st["steps"], np.uint32)
        self.acc = [[0, 0, 0, 0] for _ in range(self.n)]

    def acc_words(self):
        return np.array(self.acc, dtype=object).astype(np.int64).reshape(self.n, 4)

    def add_words(self, words):
        """Element-wise sum of another rank's buffer into this one (what ranks do before the step)."""
        w = np.asarray(words).reshape(self.n, 4)
        for t in range(self.n):
            for k in range(4):
                self.acc[t][k] += int(w[t, k])

    # ---- the KD leaf ------------------------------------------------------------------------------------------------------
    def inside(self, p):
        with np.errstate(invalid="ignore"):
            return ((p >= self.bmin[:, None]) & (p <= self.bmax[:, None])).all(axis=0)

    def leaf_of(self, p, inside):
        q = np.where(inside[None, :], p, self.bmin[:, None]).astype(F)   # (lanes outside are not looked up: any inside point)
        return self.kd_tree[self.tree.get_leaf_node_index(np.ascontiguousarray(q)).astype(np.int64)]

    # ---- QUERY ------------------------------------------------------------------------------------------------------------
    def query(self, p, active=None):
        p = np.asarray(p, F)
        ins = self.inside(p)
        if active is not None:
            ins = ins & (np.asarray(active) != 0)
        theta = np.where(ins, self.theta[self.leaf_of(p, ins)], self.theta0).astype(F)
        return logistic(theta)

    # ---- RECORD -----------------------------------------------------------------------------------------------------------
    def gradients(self, rec, count=None):
        """(kept mask, leaf of every record, g of every record) -- g is meaningful on kept records."""
        p = np.asarray(rec["position"], F)
        m = p.shape[1]
        b, gp, pr, wo = (np.asarray(rec[k], F) for k in ("bsdf_pdf", "guide_pdf", "product", "wo_pdf"))
        delta = np.zeros(m, bool) if rec.get("is_delta") is None else np.asarray(rec["is_delta"]) != 0
        ins = self.inside(p)
        leaf = self.leaf_of(p, ins)
        fin = np.isfinite(b) & np.isfinite(gp) & np.isfinite(pr) & np.isfinite(wo)
        with np.errstate(all="ignore"):
            f = logistic(self.theta[leaf])
            omf = (F(1) - f).astype(F)
            mix = ((f * b).astype(F) + (omf * gp).astype(F)).astype(F)
            kept = ~delta & ins & fin & (wo > 0) & (mix > 0)
            if count is not None:
                kept &= np.arange(m) < int(count)
            r = (pr / mix).astype(F)
            if self.loss == LOSS_VARIANCE:
                r = (r * r).astype(F)
            dLdf = (((F(0) - r).astype(F) / wo).astype(F) * (b - gp).astype(F)).astype(F)
            g = (dLdf * (f * omf).astype(F)).astype(F)
        return kept, leaf, g

    def record(self, rec, count=None):
        kept, leaf, g = self.gradients(rec, count)
        idx = np.nonzero(kept)[0]
        for t, (w0, w1, w2) in zip(leaf[idx].tolist(), limbs(g[idx])):
            a = self.acc[t]
            a[0] += w0
            a[1] += w1
            a[2] += w2
            a[3] += 1
        return kept

    # ---- STEP -------------------------------------------------------------------------------------------------------------
    def step(self):
        sel = np.array([t for t in range(self.n) if self.acc[t][3] > 0], np.int64)
        if sel.size == 0:
            return
        tot = [self.acc[t][0] + (self.acc[t][1] << 32) + (self.acc[t][2] << 64) for t in sel]
        lo = np.array([v & 0xffffffffffffffff for v in tot], np.uint64)
        hi = np.array([v >> 64 for v in tot], np.int64)
        cnt = np.array([F(self.acc[t][3]) for t in sel], F)
        th, m, v, p1, p2 = self.theta[sel], self.m[sel], self.v[sel], self.p1[sel], self.p2[sel]
        with np.errstate(all="ignore"):
            g = (po.acc_to_float(lo, hi) / cnt).astype(F)
            g = (g + (self.l2 * th).astype(F)).astype(F)
            m = ((self.beta1 * m).astype(F) + ((F(1) - self.beta1) * g).astype(F)).astype(F)
            v = ((self.beta2 * v).astype(F) + ((F(1) - self.beta2) * (g * g).astype(F)).astype(F)).astype(F)
            p1 = (p1 * self.beta1).astype(F)
            p2 = (p2 * self.beta2).astype(F)
            a = (self.lr * (np.sqrt((F(1) - p2).astype(F)).astype(F) / (F(1) - p1).astype(F)).astype(F)).astype(F)
            th = (th - (a * (m / (np.sqrt(v).astype(F) + self.eps).astype(F)).astype(F)).astype(F)).astype(F)
            th = np.where(th < -THETA_MAX, -THETA_MAX, np.where(th > THETA_MAX, THETA_MAX, th)).astype(F)
        self.theta[sel], self.m[sel], self.v[sel], self.p1[sel], self.p2[sel] = th, m, v, p1, p2
        self.steps[sel] += np.uint32(1)
        for t in sel:
            self.acc[t] = [0, 0, 0, 0]


# ---- record sets shared by the CPU and the GPU tests ------------------------------------------------------------------------
def synthetic_records(m, seed, bbox_min, bbox_max, position=None):
    """m records with uniform positions (or all at `position`): pdfs and product positive and finite, wo_pdf the 0.5 mixture."""
    import synth
    p = synth.positions_uniform(m, seed, bbox_min, bbox_max)
    if position is not None:
        p[:] = np.asarray(position, F)[:, None]
    u = synth.uniform(m, seed + 1, 4)
    b = (F(0.05) + F(2) * u[0]).astype(F)
    g = np.ldexp(F(0.01) + u[1], np.floor(u[2] * F(8)).astype(np.int32) - 4).astype(F)
    pr = (F(4) * u[3]).astype(F)
    wo = ((F(0.5) * b).astype(F) + (F(0.5) * g).astype(F)).astype(F)
    return {"position": p, "bsdf_pdf": b, "guide_pdf": g, "product": pr, "wo_pdf": wo, "is_delta": np.zeros(m, np.uint8)}


EDGE_KINDS = ("delta", "nan product", "inf guide", "nan bsdf", "zero wo", "negative wo", "inf wo", "zero mix", "outside", "nan position",
              "zero product", "tiny gradient", "huge gradient", "on the box face")
EDGE_DROPPED = EDGE_KINDS[:10]


def salt_with_edges(rec, bbox_min, bbox_max, stride=5):
    """Every `stride`-th record becomes one of EDGE_KINDS in turn; returns the kind of every record ('' = untouched)."""
    m = rec["wo_pdf"].shape[0]
    kinds = np.array([""] * m, dtype=object)
    lo, hi = F(bbox_min[0]), F(bbox_max[0])
    for j, i in enumerate(range(3, m, stride)):
        k = EDGE_KINDS[j % len(EDGE_KINDS)]
        kinds[i] = k
        if k == "delta": rec["is_delta"][i] = 1
        elif k == "nan product": rec["product"][i] = np.nan
        elif k == "inf guide": rec["guide_pdf"][i] = np.inf
        elif k == "nan bsdf": rec["bsdf_pdf"][i] = np.nan
        elif k == "zero wo": rec["wo_pdf"][i] = 0.0
        elif k == "negative wo": rec["wo_pdf"][i] = -1.0
        elif k == "inf wo": rec["wo_pdf"][i] = np.inf
        elif k == "zero mix": rec["bsdf_pdf"][i] = 0.0; rec["guide_pdf"][i] = 0.0
        elif k == "outside": rec["position"][j % 3, i] = np.nextafter(hi, F(np.inf)) if j % 2 else F(lo - F(1e-3))
        elif k == "nan position": rec["position"][j % 3, i] = np.nan
        elif k == "zero product": rec["product"][i] = 0.0
        elif k == "tiny gradient": rec["product"][i] = 1e-30
        elif k == "huge gradient": rec["product"][i] = 3e38; rec["wo_pdf"][i] = 1e-30
        elif k == "on the box face": rec["position"][j % 3, i] = hi if j % 2 else lo
    return kinds
