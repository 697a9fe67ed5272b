"""pg_resample_lobe (include/ext/guiding/pg_resample_lobe.h) restated in numpy float32: vectorised over the lanes, a Python loop
over the candidates.  Built from the unchanged oracle -- OracleTree.sample, OracleTree.pdf and rng_next_f32 of
oracle/pg_oracle.py -- from resample_model's duff_frame, to_world and cosine_local, and, for the GGX lobe, from the oracle's own
rough conductor: bsdf_probe of one ONE-SIDED ROUGH_CONDUCTOR row per lane with alpha = -roughness (GGX).  The pdf of its eval
is the header's g; with u = (., u1, u2) its sampled wo is the header's o, and a sample that failed comes back as wo = (0, 0, 0)
(a sample that did not has o.z > 0).  It takes nothing from the device.

Every array operation below is ONE fp32 operation per element (numpy rounds each on its own; there is no contraction), in the
order the header states them.

Test infrastructure; the product never imports it.  Run as a program it writes profiles/resample_lobe/variance.txt.
"""
from __future__ import annotations

import os

import numpy as np

import bsdf_model as BM
import resample_model as rs
from oracle import pg_oracle as po
from resample_model import (CAND_FIELDS, INV_4PI, INV_PI, NONE, OUT_FIELDS, weight_of_the_header,  # noqa: F401
                            weight_one_over_source, weight_without_one_over_m)

F = np.float32
MIN_ROUGHNESS = F(1e-3)                                      # PG_RESAMPLE_LOBE_MIN_ROUGHNESS
TREE, COSINE, GGX, GGX_FAILED = 0, 1, 2, 3                   # "kind" of a candidate (kinds=True; 255: the lane was not served)


def to_local(s, t, n, v):
    """(dot3(v, s), dot3(v, t), dot3(v, n)), dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z"""
    return np.stack([(v[0] * b[0] + v[1] * b[1]) + v[2] * b[2] for b in (s, t, n)]).astype(F)


def rows_of(roughness):
    """one ONE-SIDED GGX rough-conductor row per lane (tests/bsdf_sets._row's columns), (m, 16)"""
    r = np.zeros((roughness.shape[0], BM.STRIDE), F)
    r[:, 0], r[:, 1:4], r[:, 4], r[:, 11] = BM.ROUGH_CONDUCTOR, 1, -roughness, 1
    return r


def ggx_density(roughness, wil, wl):
    """g(wl) per lane: wil, wl (3, m) -> (m,), the pdf of the oracle's eval"""
    m = roughness.shape[0]
    if m == 0:
        return np.zeros(0, F)
    return po.bsdf_probe(rows_of(roughness), np.arange(m, dtype=np.int32), wil.T, wl.T, np.zeros((m, 3), F), level=3)[1]


def ggx_sample(roughness, wil, u1, u2):
    """-> o (3, m), ok (m,): the oracle's sampled wo, and whether the sample did not fail"""
    m = roughness.shape[0]
    if m == 0:
        return np.zeros((3, 0), F), np.zeros(0, bool)
    u = np.stack([np.full(m, 0.5, F), u1, u2], axis=1).astype(F)
    swo = po.bsdf_probe(rows_of(roughness), np.arange(m, dtype=np.int32), wil.T, wil.T, u, level=3)[2]
    return np.ascontiguousarray(swo.T), swo[:, 2] > 0


def valid_lanes(normal, wi, roughness, specular, active=None):
    with np.errstate(invalid="ignore"):
        live = np.isfinite(normal).all(axis=0) & np.isfinite(wi).all(axis=0)
        live &= (roughness >= MIN_ROUGHNESS) & (roughness <= F(1)) & (specular >= F(0)) & (specular <= F(1))
    if active is not None:
        live &= np.asarray(active) != 0
    return live


def resample(tree, p, normal, wi, roughness, specular, st, inc, M, alpha, delta, active=None, weight=weight_of_the_header,
             candidates=False, kinds=False):
    """-> {"dir" (3, n), "weight", "target", "source" fp32 (n,), "index" uint32 (n,)} (+ "cand_dir" (M, 3, n), "cand_target",
    "cand_source" (M, n); + "kind" uint8 (M, n), the model's own note of where a candidate came from).  st (uint64 (n,)) is
    advanced in place, as the oracle's own calls do."""
    p, normal, wi = (np.ascontiguousarray(x, F) for x in (p, normal, wi))
    roughness, specular = np.ascontiguousarray(roughness, F), np.ascontiguousarray(specular, F)
    n = p.shape[1]
    assert p.shape == normal.shape == wi.shape == (3, n) and roughness.shape == specular.shape == (n,)
    assert st.shape == inc.shape == (n,) and st.dtype == inc.dtype == np.uint64
    assert 1 <= M <= 64
    alpha, delta = F(alpha), F(delta)
    assert 0 <= alpha <= 1 and 0 <= delta <= 1
    om, d4, omd = F(1) - alpha, delta * INV_4PI, F(1) - delta
    idx = np.nonzero(valid_lanes(normal, wi, roughness, specular, active))[0]
    m = idx.shape[0]
    P, Nn, Wi = (np.ascontiguousarray(x[:, idx]) for x in (p, normal, wi))
    R, Sp = roughness[idx], specular[idx]
    S, I = st[idx].copy(), inc[idx].copy()
    wsum = np.zeros(m, F)
    kdir = np.tile(np.array([[0], [0], [-1]], F), (1, m))
    kt, ks, kk = np.zeros(m, F), np.zeros(m, F), np.full(m, NONE, np.uint32)
    cd, ct, cs = np.zeros((M, 3, n), F), np.zeros((M, n), F), np.zeros((M, n), F)
    kind = np.full((M, n), 255, np.uint8)
    with np.errstate(all="ignore"):
        fs, ft = rs.duff_frame(Nn)
        wil = to_local(fs, ft, Nn, Wi)
        sg = np.where(wil[2] > 0, Sp, F(0)).astype(F)
        oms = F(1) - sg
        for k in range(M):
            xi = po.rng_next_f32(S, I)
            from_tree = xi > alpha
            w, q = np.zeros((3, m), F), np.zeros(m, F)
            ok = np.ones(m, bool)
            kd = np.zeros(m, np.uint8)
            j = np.nonzero(from_tree)[0]
            if j.size:
                sj, ij = S[j].copy(), I[j].copy()
                w[:, j], q[j] = tree.sample(np.ascontiguousarray(P[:, j]), sj, ij)
                S[j] = sj
            j = np.nonzero(~from_tree)[0]
            if j.size:
                sj, ij = S[j].copy(), I[j].copy()
                xi2 = po.rng_next_f32(sj, ij)
                u1 = po.rng_next_f32(sj, ij)
                u2 = po.rng_next_f32(sj, ij)
                S[j] = sj
                gg = xi2 < sg[j]
                o, okj = np.empty((3, j.size), F), np.ones(j.size, bool)
                o[:, gg], okj[gg] = ggx_sample(R[j][gg], np.ascontiguousarray(wil[:, j][:, gg]), u1[gg], u2[gg])
                o[:, ~gg] = rs.cosine_local(u1[~gg], u2[~gg])
                wj = rs.to_world(fs[:, j], ft[:, j], Nn[:, j], o)
                jo = j[okj]
                w[:, jo] = wj[:, okj]
                if jo.size:
                    q[jo] = tree.pdf(np.ascontiguousarray(P[:, jo]), np.ascontiguousarray(wj[:, okj]))
                ok[j] = okj
                kd[j] = np.where(gg, np.where(okj, GGX, GGX_FAILED), COSINE)
            wl = to_local(fs, ft, Nn, w)
            c = np.where(wl[2] > 0, wl[2] * INV_PI, F(0)).astype(F)
            g = np.zeros(m, F)
            e = np.nonzero(ok & (sg != 0))[0]                   # with sg == 0, g is not evaluated
            g[e] = ggx_density(R[e], np.ascontiguousarray(wil[:, e]), np.ascontiguousarray(wl[:, e]))
            b = np.where(sg == 0, c, (sg * g) + (oms * c)).astype(F)
            b = np.where(np.isfinite(b), b, F(0)).astype(F)
            s = alpha * b + om * q
            t = b * (d4 + omd * q)
            r = t / s
            wk = np.where(ok & (s > 0) & (t > 0) & np.isfinite(r), r, F(0)).astype(F)
            s, t = np.where(ok, s, F(0)).astype(F), np.where(ok, t, F(0)).astype(F)      # a failed candidate: t = s = 0
            zeta = po.rng_next_f32(S, I)
            wsum = wsum + wk
            keep = (wk > 0) & (zeta * wsum < wk)
            kk[keep] = k
            kdir[:, keep], kt[keep], ks[keep] = w[:, keep], t[keep], s[keep]
            cd[k][:, idx], ct[k, idx], cs[k, idx], kind[k, idx] = w, t, s, kd
        kept = kk != NONE
        W = np.zeros(m, F)
        W[kept] = weight(wsum[kept], M, kt[kept], ks[kept])
    st[idx] = S
    out = {"dir": np.tile(np.array([[0], [0], [-1]], F), (1, n)), "weight": np.zeros(n, F), "target": np.zeros(n, F),
           "source": np.zeros(n, F), "index": np.full(n, NONE, np.uint32)}
    out["dir"][:, idx], out["weight"][idx], out["target"][idx], out["source"][idx], out["index"][idx] = kdir, W, kt, ks, kk
    for v in out.values():
        assert v.dtype in (F, np.uint32)
    if candidates:
        out.update(cand_dir=cd, cand_target=ct, cand_source=cs)
    if kinds:
        out["kind"] = kind
    return out


# ---- the product the estimator is measured on (tests/test_resample_lobe_model.py; the issue's settings) ------------------------
SETTINGS = ((0.1, 0.7), (0.02, 1.0), (0.5, 0.3))             # (roughness, specular)
WI = (0.6, 0.0, 0.8)
N_LANES, SEED, ALPHA, DELTA = 1 << 16, 1234, 0.5, 0.1


def fixed_vertex(n, roughness, specular):
    """n lanes at the centre of the box with the normal +z, the viewer at WI"""
    p, nrm = rs.fixed_vertex(n)
    return p, nrm, np.tile(np.array(WI, F)[:, None], (1, n)), np.full(n, roughness, F), np.full(n, specular, F)


def lobe_f64(wl, wil, roughness, specular):
    """b in float64, written out from the header's formulas and from nothing else: wl (3, ...) local directions"""
    a = float(roughness)
    wil = np.asarray(wil, np.float64)
    c = np.maximum(wl[2], 0) / np.pi
    h = wl + wil.reshape(3, *([1] * (wl.ndim - 1)))
    h = h / np.sqrt((h * h).sum(axis=0))
    t = (h[0] / a) ** 2 + (h[1] / a) ** 2 + h[2] ** 2
    D = 1 / (np.pi * a * a * t * t)
    xy = (a * wil[0]) ** 2 + (a * wil[1]) ** 2
    G1 = 2 / (1 + np.sqrt(1 + xy / wil[2] ** 2))
    wih = (h * wil.reshape(3, *([1] * (wl.ndim - 1)))).sum(axis=0)
    woh = (h * wl).sum(axis=0)
    g = np.where((wl[2] > 0) & (wih > 0) & (woh > 0), D * G1 / (4 * wil[2]), 0.0)
    return specular * g + (1 - specular) * c


def truth_by_quadrature(tree, roughness, specular, grid=2048):
    """The integral over the sphere of f = 4 pi q b, q the tree's density at the centre of the box and the normal +z: the midpoint
    rule in float64 on grid x grid cells of the equal-area square (x = phi / 2 pi, y = (cos theta + 1) / 2, so d omega = 4 pi dx dy).
    q is constant on the 16 x 16 cells of horizon_lobe_tree() and is read at their centres by OracleTree.pdf; no sampling code
    and nothing of the float32 model is used."""
    cells = 16
    assert grid % cells == 0
    cy, cx = np.meshgrid((np.arange(cells) + 0.5) / cells, (np.arange(cells) + 0.5) / cells, indexing="ij")
    ct = 2 * cy.ravel() - 1
    st_, ph = np.sqrt(1 - ct * ct), 2 * np.pi * cx.ravel()
    d = np.stack([st_ * np.cos(ph), st_ * np.sin(ph), ct]).astype(F)
    q = tree.pdf(np.full((3, cells * cells), 50, F), np.ascontiguousarray(d)).astype(np.float64).reshape(cells, cells)
    assert abs(q.mean() * 4 * np.pi - 1) < 1e-5                # a density over the sphere, constant per cell
    rep = grid // cells
    total = 0.0
    x = (np.arange(grid) + 0.5) / grid
    phi = 2 * np.pi * x
    for iy in range(grid // 2, grid):                           # (b is zero below the horizon)
        cos_t = 2 * (iy + 0.5) / grid - 1
        sin_t = np.sqrt(1 - cos_t * cos_t)
        wl = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), np.full(grid, cos_t)])
        b = lobe_f64(wl, WI, roughness, specular)
        total += float((np.repeat(q[iy // rep], rep) * b).sum())
    return 4 * np.pi * total * (4 * np.pi / (grid * grid))


def product_estimates(tree, roughness, specular, M, weight=weight_of_the_header, cosine_only=False, N=N_LANES, seed=SEED):
    """f(dir) * W per lane, float64, f = 4 pi q b with b from the model's own kept target: t = b * (d4 + omd * q).
    cosine_only: the directions and weights of resample_model.resample (pg_resample_cosine), against the same f."""
    p, nrm, wi, rough, spec = fixed_vertex(N, roughness, specular)
    st, inc = po.rng_seed(N, seed)
    if cosine_only:
        r = rs.resample(tree, p, nrm, st, inc, M, ALPHA, DELTA, weight=weight)
    else:
        r = resample(tree, p, nrm, wi, rough, spec, st, inc, M, ALPHA, DELTA, weight=weight)
    q = tree.pdf(p, r["dir"]).astype(np.float64)
    b = lobe_f64(r["dir"].astype(np.float64), WI, roughness, specular)   # (the normal is +z: local is world)
    return np.where(r["index"] != NONE, 4 * np.pi * q * b * r["weight"].astype(np.float64), 0.0)


if __name__ == "__main__":
    tree = rs.horizon_lobe_tree()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_lobe", "variance.txt")
    with open(path, "w") as f:
        f.write("# tests/resample_lobe_model.py: the estimator f(dir) * W of the integral of f = 4 pi q(w) b(w) on horizon_lobe_tree(),\n"
                "# normal +z, wi (0.6, 0, 0.8), alpha 0.5, delta 0.1, 2^16 lanes of the float32 model (seed 1234); truth: float64\n"
                "# midpoint quadrature on 2048 x 2048 cells of the equal-area square\n"
                "# roughness | specular | truth | M | mean | standard errors off | sample variance | variance / variance at M = 1"
                " | variance of pg_resample_cosine's model at this M / variance\n")
        for roughness, specular in SETTINGS:
            truth = truth_by_quadrature(tree, roughness, specular)
            v1 = None
            for M in (1, 4, 16):
                e = product_estimates(tree, roughness, specular, M)
                ec = product_estimates(tree, roughness, specular, M, cosine_only=True)
                var, se = e.var(ddof=1), e.std(ddof=1) / np.sqrt(e.shape[0])
                v1 = var if v1 is None else v1
                f.write("%g | %g | %.6f | %d | %.6f | %.2f | %.6f | %.4f | %.2f\n"
                        % (roughness, specular, truth, M, e.mean(), abs(e.mean() - truth) / se, var, var / v1, ec.var(ddof=1) / var))
    print(open(path).read())
