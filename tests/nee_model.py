"""pg_nee_set_lights and pg_nee_resample (include/ext/lights/pg_nee.h) restated in numpy float32: vectorised over the lanes (or the
lights), a Python loop over the candidates.  Built on tests/lights_model.py for SELECT, PMF, the rows and the KD leaf of a
position, and on the oracle's rng_next_f32 for the stream.  It takes nothing from the device.

Every array operation below is ONE fp32 operation per element (numpy rounds each on its own; there is no contraction), in the
order the header states them.

Test infrastructure; the product never imports it.
"""
from __future__ import annotations

import numpy as np

import lights_model as lm
from oracle import pg_oracle as po
from resample_model import weight_of_the_header, weight_one_over_source, weight_without_one_over_m  # noqa: F401  (the three weights)

F = np.float32
NONE = 0xFFFFFFFF                                     # PG_LIGHTS_NONE and PG_RESAMPLE_NONE
TABLE_WORDS = 12
OUT_FIELDS = ("point", "weight", "dir", "dist", "target", "source")     # fp32 columns of a result
OUT_FLAGS = ("light", "index")                                            # uint32 columns
CAND_FIELDS = ("cand_point", "cand_target", "cand_source")
CAND_FLAGS = ("cand_light",)


def table(origin, edge_a, edge_b, radiance, triangle, two_sided):
    """the dict SDTree.lightsSetGeometry takes"""
    L = len(radiance)
    t = {"origin": np.array(origin, F).reshape(L, 3), "edge_a": np.array(edge_a, F).reshape(L, 3),
         "edge_b": np.array(edge_b, F).reshape(L, 3), "radiance": np.array(radiance, F).reshape(L),
         "triangle": np.array(triangle, bool).reshape(L), "two_sided": np.array(two_sided, bool).reshape(L)}
    return t


def accepted(t):
    """what pg_nee_set_lights does not refuse"""
    L = len(t["radiance"])
    coords = np.concatenate([np.asarray(t[k], F).reshape(L, 3) for k in ("origin", "edge_a", "edge_b")], axis=1)
    r = np.asarray(t["radiance"], F)
    return 1 <= L <= lm.MAX_LIGHTS and bool(np.isfinite(coords).all() and np.isfinite(r).all() and (r >= 0).all())


def prepare(t):
    """the prepare step: the records of the lights, columns of length L"""
    assert accepted(t)
    o, a, b = (np.asarray(t[k], F) for k in ("origin", "edge_a", "edge_b"))
    kind = np.asarray(t["triangle"], bool)
    with np.errstate(all="ignore"):
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        len2 = (cx * cx + cy * cy) + cz * cz
        ln = np.sqrt(len2)
        N = np.stack([cx / ln, cy / ln, cz / ln], axis=1)
        area = np.where(kind, F(0.5) * ln, ln).astype(F)
        invA = np.where((ln > 0) & np.isfinite(ln), F(1) / area, F(0)).astype(F)
    out = {"o": o, "a": a, "b": b, "N": N.astype(F), "invA": invA, "radiance": np.asarray(t["radiance"], F), "kind": kind,
           "two_sided": np.asarray(t["two_sided"], bool)}
    assert all(v.dtype in (F, np.bool_) for v in out.values())
    return out


def resample(rows, leaf, delta, lights, p, normal, st, inc, M, active=None, weight=weight_of_the_header, candidates=False):
    """rows uint32 (n_leaves, L) and leaf int (n,) (-1: no leaf) as lights_model.select takes them; lights: prepare()'s.
    -> {"light", "index" uint32 (n,), "point", "dir" (3, n), "weight", "dist", "target", "source" fp32 (n,)} (+ "cand_light"
    uint32 (M, n), "cand_point" (M, 3, n), "cand_target", "cand_source" (M, n)).  st (uint64 (n,)) is advanced in place."""
    rows = np.asarray(rows, np.uint32)
    p = np.ascontiguousarray(p, F)
    normal = np.ascontiguousarray(normal, F)
    n = p.shape[1]
    assert p.shape == normal.shape == (3, n) and st.shape == inc.shape == (n,) and st.dtype == inc.dtype == np.uint64
    assert 1 <= M <= 64 and rows.shape[1] == lights["invA"].shape[0]
    live = np.isfinite(normal).all(axis=0)
    if active is not None:
        live &= np.asarray(active) != 0
    idx = np.nonzero(live)[0]
    m = idx.shape[0]
    P, Nn, lf = p[:, idx], normal[:, idx], np.asarray(leaf, np.int64)[idx]
    S, I = st[idx].copy(), inc[idx].copy()
    wsum = np.zeros(m, F)
    ky, kw = np.zeros((3, m), F), np.zeros((3, m), F)
    kd, kt, ks = np.zeros(m, F), np.zeros(m, F), np.zeros(m, F)
    kk, kj = np.full(m, NONE, np.uint32), np.full(m, NONE, np.uint32)
    cl_, cp, ct, cs_ = np.zeros((M, n), np.uint32), np.zeros((M, 3, n), F), np.zeros((M, n), F), np.zeros((M, n), F)
    with np.errstate(all="ignore"):
        for k in range(M):
            u = po.rng_next_f32(S, I)
            j, _ = lm.select(rows, lf, u, delta)
            pm = lm.pmf(rows, lf, j, delta)
            e1 = po.rng_next_f32(S, I)
            e2 = po.rng_next_f32(S, I)
            fold = lights["kind"][j] & (e1 + e2 > F(1))
            e1 = np.where(fold, F(1) - e1, e1).astype(F)
            e2 = np.where(fold, F(1) - e2, e2).astype(F)
            o, a, b, N = lights["o"][j].T, lights["a"][j].T, lights["b"][j].T, lights["N"][j].T
            y = ((o + e1 * a) + e2 * b).astype(F)
            v = y - P
            d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
            dist = np.sqrt(d2)
            w = v / dist
            cs = (Nn[0] * w[0] + Nn[1] * w[1]) + Nn[2] * w[2]
            cl = -((N[0] * w[0] + N[1] * w[1]) + N[2] * w[2])
            cl = np.where(lights["two_sided"][j], np.abs(cl), cl).astype(F)
            g = np.where((d2 > 0) & (cs > 0) & (cl > 0), (cs * cl) / d2, F(0)).astype(F)
            t = lights["radiance"][j] * g
            s = pm * lights["invA"][j]
            r = t / s
            wk = np.where((s > 0) & (t > 0) & np.isfinite(r), r, F(0)).astype(F)
            zeta = po.rng_next_f32(S, I)
            wsum = wsum + wk
            keep = (wk > 0) & (zeta * wsum < wk)
            kk[keep], kj[keep] = k, j[keep]
            ky[:, keep], kw[:, keep], kd[keep], kt[keep], ks[keep] = y[:, keep], w[:, keep], dist[keep], t[keep], s[keep]
            cl_[k, idx], ct[k, idx], cs_[k, idx] = j, t, s
            cp[k][:, idx] = y
            assert y.dtype == w.dtype == t.dtype == s.dtype == wk.dtype == wsum.dtype == F
        kept = kk != NONE
        W = np.zeros(m, F)
        W[kept] = weight(wsum[kept], M, kt[kept], ks[kept])
    st[idx] = S
    out = {"light": np.full(n, NONE, np.uint32), "index": np.full(n, NONE, np.uint32), "point": np.zeros((3, n), F),
           "dir": np.zeros((3, n), F), "weight": np.zeros(n, F), "dist": np.zeros(n, F), "target": np.zeros(n, F),
           "source": np.zeros(n, F)}
    out["light"][idx], out["index"][idx], out["point"][:, idx], out["dir"][:, idx] = kj, kk, ky, kw
    out["weight"][idx], out["dist"][idx], out["target"][idx], out["source"][idx] = W, kd, kt, ks
    for v in out.values():
        assert v.dtype in (F, np.uint32)
    if candidates:
        out.update(cand_light=cl_, cand_point=cp, cand_target=ct, cand_source=cs_)
    return out


def resample_in_tree(model, lights, p, normal, st, inc, M, **kw):
    """resample() with the rows, the delta and the KD leaves of a lights_model.LightsModel"""
    p = np.ascontiguousarray(p, F)
    return resample(model.rows, model.leaf_of(p, model.inside(p)), model.delta, lights, p, normal, st, inc, M, **kw)
