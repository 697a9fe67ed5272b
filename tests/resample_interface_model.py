"""pg_resample_interface (include/ext/guiding/pg_resample_interface.h) restated in numpy float32: vectorised over the lanes, a
Python loop over the candidates.  Built from the unchanged oracle -- OracleTree.sample, OracleTree.pdf and rng_next_f32 of
oracle/pg_oracle.py -- from resample_model's duff_frame and to_world, and, for the lobe, from the oracle's own rough dielectric:
bsdf_probe of one ONE-SIDED ROUGH_DIELECTRIC row per lane with alpha = -roughness (GGX) and eta = (eta, 0, 0), the columns of
tests/bsdf_sets._row.  The pdf of its eval is the header's b; with u = (xi2, u1, u2) its sampled wo is the header's o, and a
sample whose pdf is 0 comes back with wo = (0, 0, 0); the sample's eta (1 for a reflection) names its branch for the header's
side test.  It takes nothing from the device.

Every array operation below is ONE fp32 operation per element (numpy rounds each on its own; there is no contraction), in the
order the header states them.

Test infrastructure; the product never imports it.  Run as a program it writes profiles/resample_interface/variance.txt.
"""
from __future__ import annotations

import os

import numpy as np

import bsdf_model as BM
import resample_lobe_model as rl
import resample_model as rs
from oracle import pg_oracle as po
from resample_lobe_model import to_local
from resample_model import (INV_4PI, NONE, weight_of_the_header, weight_one_over_source,  # noqa: F401
                            weight_without_one_over_m)

F = np.float32
MIN_ROUGHNESS = F(1e-3)                                      # PG_RESAMPLE_INTERFACE_MIN_ROUGHNESS
MIN_ETA, MAX_ETA = F(0.25), F(4.0)                           # PG_RESAMPLE_INTERFACE_MIN_ETA, _MAX_ETA
TREE, LOBE, LOBE_FAILED = 0, 1, 2                            # "kind" of a candidate (kinds=True; 255: the lane was not served)


def rows_of(roughness, eta):
    """one ONE-SIDED GGX rough-dielectric row per lane (tests/bsdf_sets._row's columns), (m, 16)"""
    r = np.zeros((roughness.shape[0], BM.STRIDE), F)
    r[:, 0], r[:, 1:4], r[:, 4], r[:, 5], r[:, 11] = BM.ROUGH_DIELECTRIC, 1, -roughness, eta, 1
    return r


def interface_density(roughness, eta, wil, wl):
    """b(wl) per lane: wil, wl (3, m) -> (m,), the pdf of the oracle's eval; then b = isfinite(b) ? b : 0"""
    m = roughness.shape[0]
    if m == 0:
        return np.zeros(0, F)
    b = po.bsdf_probe(rows_of(roughness, eta), np.arange(m, dtype=np.int32), wil.T, wl.T, np.zeros((m, 3), F), level=3)[1]
    return np.where(np.isfinite(b), b, F(0)).astype(F)


def interface_sample(roughness, eta, wil, xi2, u1, u2):
    """-> o (3, m), ok (m,): the oracle's sampled wo, and whether the sample did not fail: its pdf is not 0, and it left on the
    side of the macro-surface its branch names -- a reflection (the sample's eta is 1) on wil's side, a refraction not"""
    m = roughness.shape[0]
    if m == 0:
        return np.zeros((3, 0), F), np.zeros(0, bool)
    u = np.stack([xi2, u1, u2], axis=1).astype(F)
    r = po.bsdf_probe(rows_of(roughness, eta), np.arange(m, dtype=np.int32), wil.T, wil.T, u, level=3)
    swo, spdf, seta = r[2], r[3], r[5]
    return np.ascontiguousarray(swo.T), (spdf != 0) & ((seta == 1) == (wil[2] * swo[:, 2] > 0))


def valid_lanes(normal, wi, roughness, eta, active=None):
    with np.errstate(invalid="ignore"):
        live = np.isfinite(normal).all(axis=0) & np.isfinite(wi).all(axis=0)
        live &= (roughness >= MIN_ROUGHNESS) & (roughness <= F(1)) & (eta >= MIN_ETA) & (eta <= MAX_ETA) & (eta != F(1))
    if active is not None:
        live &= np.asarray(active) != 0
    return live


def resample(tree, p, normal, wi, roughness, eta, st, inc, M, alpha, delta, active=None, weight=weight_of_the_header,
             candidates=False, kinds=False):
    """-> {"dir" (3, n), "weight", "target", "source", "eta" fp32 (n,), "index" uint32 (n,)} (+ "cand_dir" (M, 3, n),
    "cand_target", "cand_source" (M, n); + "kind" uint8 (M, n), the model's own note of where a candidate came from).
    st (uint64 (n,)) is advanced in place, as the oracle's own calls do."""
    p, normal, wi = (np.ascontiguousarray(x, F) for x in (p, normal, wi))
    roughness, eta = np.ascontiguousarray(roughness, F), np.ascontiguousarray(eta, F)
    n = p.shape[1]
    assert p.shape == normal.shape == wi.shape == (3, n) and roughness.shape == eta.shape == (n,)
    assert st.shape == inc.shape == (n,) and st.dtype == inc.dtype == np.uint64
    assert 1 <= M <= 64
    alpha, delta = F(alpha), F(delta)
    assert 0 <= alpha <= 1 and 0 <= delta <= 1
    om, d4, omd = F(1) - alpha, delta * INV_4PI, F(1) - delta
    idx = np.nonzero(valid_lanes(normal, wi, roughness, eta, active))[0]
    m = idx.shape[0]
    P, Nn, Wi = (np.ascontiguousarray(x[:, idx]) for x in (p, normal, wi))
    R, E = roughness[idx], eta[idx]
    S, I = st[idx].copy(), inc[idx].copy()
    wsum = np.zeros(m, F)
    kdir = np.tile(np.array([[0], [0], [-1]], F), (1, m))
    kt, ks, kk = np.zeros(m, F), np.zeros(m, F), np.full(m, NONE, np.uint32)
    cd, ct, cs = np.zeros((M, 3, n), F), np.zeros((M, n), F), np.zeros((M, n), F)
    kind = np.full((M, n), 255, np.uint8)
    with np.errstate(all="ignore"):
        fs, ft = rs.duff_frame(Nn)
        wil = to_local(fs, ft, Nn, Wi)
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
                o, okj = interface_sample(R[j], E[j], np.ascontiguousarray(wil[:, j]), xi2, u1, u2)
                wj = rs.to_world(fs[:, j], ft[:, j], Nn[:, j], o)
                jo = j[okj]
                w[:, jo] = wj[:, okj]
                if jo.size:
                    q[jo] = tree.pdf(np.ascontiguousarray(P[:, jo]), np.ascontiguousarray(wj[:, okj]))
                ok[j] = okj
                kd[j] = np.where(okj, LOBE, LOBE_FAILED)
            wl = to_local(fs, ft, Nn, w)
            b = np.zeros(m, F)
            e = np.nonzero(ok)[0]
            b[e] = interface_density(R[e], E[e], np.ascontiguousarray(wil[:, e]), np.ascontiguousarray(wl[:, e]))
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
        wlk = to_local(fs, ft, Nn, kdir)
        eo = np.where(wil[2] * wlk[2] > 0, F(1), np.where(wil[2] > 0, E, F(1) / E)).astype(F)
        eo = np.where(kept, eo, F(0)).astype(F)
    st[idx] = S
    out = {"dir": np.tile(np.array([[0], [0], [-1]], F), (1, n)), "weight": np.zeros(n, F), "target": np.zeros(n, F),
           "source": np.zeros(n, F), "index": np.full(n, NONE, np.uint32), "eta": np.zeros(n, F)}
    out["dir"][:, idx], out["weight"][idx], out["target"][idx], out["source"][idx], out["index"][idx] = kdir, W, kt, ks, kk
    out["eta"][idx] = eo
    for v in out.values():
        assert v.dtype in (F, np.uint32)
    if candidates:
        out.update(cand_dir=cd, cand_target=ct, cand_source=cs)
    if kinds:
        out["kind"] = kind
    return out


# ---- the product the estimator is measured on (tests/test_resample_interface_model.py; the issue's settings) -------------------
SETTINGS = ((0.1, 1.5, (0.6, 0.0, 0.8)), (0.3, 1.5, (0.6, 0.0, -0.8)), (0.07, 1.33, (0.28, 0.0, 0.96)))   # (roughness, eta, wi)
# (the issue's third roughness was 0.05: there 1024^2 and 2048^2 cells differ by 0.8 of a standard error at M = 16, so it was raised)
N_LANES, SEED, ALPHA, DELTA = 1 << 16, 1234, 0.5, 0.1


def fixed_vertex(n, roughness, eta, wi):
    """n lanes at the centre of the box with the normal +z, the viewer at wi"""
    p, nrm = rs.fixed_vertex(n)
    return p, nrm, np.tile(np.array(wi, F)[:, None], (1, n)), np.full(n, roughness, F), np.full(n, eta, F)


def fresnel_f64(c, eta):
    """the header's fresnel(c, eta) in float64: F only"""
    eta_it = np.where(c >= 0, eta, 1 / eta)
    eta_ti = 1 / eta_it
    ac = np.abs(c)
    ct = np.sqrt(np.maximum(1 - (1 - c * c) * eta_ti * eta_ti, 0))
    a_s = (eta_it * ct - ac) / (eta_it * ct + ac)
    a_p = (eta_it * ac - ct) / (eta_it * ac + ct)
    return np.where(ac == 0, 1.0, 0.5 * (a_s * a_s + a_p * a_p))


def lobe_f64(wl, wil, roughness, eta):
    """b in float64, written out from the header's formulas and from nothing else: wl (3, ...) local directions, wil (3,)"""
    a, eta = float(roughness), float(eta)
    wil = np.asarray(wil, np.float64)
    ci, co = wil[2], wl[2]
    if ci == 0:
        return np.zeros(wl.shape[1:])
    wv = wil.reshape(3, *([1] * (wl.ndim - 1)))
    reflect = ci * co > 0
    e = eta if ci > 0 else 1 / eta
    with np.errstate(all="ignore"):
        h = wv + wl * np.where(reflect, 1.0, e)
        h = h / np.sqrt((h * h).sum(axis=0))
        h = np.where(h[2] < 0, -h, h)
        t = (h[0] / a) ** 2 + (h[1] / a) ** 2 + h[2] ** 2
        D = 1 / (np.pi * a * a * t * t)
        wim, wom = (h * wv).sum(axis=0), (h * wl).sum(axis=0)
        Fr = fresnel_f64(wim, eta)
        den = wim + e * wom
        jac = np.where(reflect, 1 / (4 * wom), e * e * wom / (den * den))
        wiu = wil if ci > 0 else -wil
        xy = (a * wiu[0]) ** 2 + (a * wiu[1]) ** 2
        wiuh = wim if ci > 0 else -wim
        G1 = np.where(wiuh * wiu[2] > 0, 2 / (1 + np.sqrt(1 + xy / wiu[2] ** 2)), 0.0)
        b = D * G1 * np.abs(wiuh) / wiu[2] * np.where(reflect, Fr, 1 - Fr) * np.abs(jac)
        b = np.where((wim * ci > 0) & (wom * co > 0) & np.isfinite(b), b, 0.0)
    return b


def truth_by_quadrature(tree, roughness, eta, wi, grid=2048):
    """The integral over the WHOLE sphere of f = 4 pi q b, q the tree's density at the centre of the box and the normal +z: the
    midpoint rule in float64 on grid x grid cells of the equal-area square (x = phi / 2 pi, y = (cos theta + 1) / 2, so
    d omega = 4 pi dx dy).  q is constant on the 16 x 16 cells of horizon_lobe_tree() and is read at their centres by
    OracleTree.pdf; no sampling code and nothing of the float32 model is used."""
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
    phi = 2 * np.pi * (np.arange(grid) + 0.5) / grid
    cphi, sphi = np.cos(phi), np.sin(phi)
    rows = 64
    assert rep % rows == 0
    for y0 in range(0, grid, rows):                             # (both hemispheres)
        cos_t = (2 * (np.arange(y0, y0 + rows) + 0.5) / grid - 1)[:, None]
        sin_t = np.sqrt(1 - cos_t * cos_t)
        wl = np.stack([sin_t * cphi[None, :], sin_t * sphi[None, :], np.broadcast_to(cos_t, (rows, grid))])
        b = lobe_f64(wl, wi, roughness, eta)
        total += float((np.repeat(q[y0 // rep], rep)[None, :] * b).sum())   # (the rows of a block lie in one row of q's cells)
    return 4 * np.pi * total * (4 * np.pi / (grid * grid))


def product_estimates(tree, roughness, eta, wi, M, weight=weight_of_the_header, reflection_lobe=False, N=N_LANES, seed=SEED):
    """f(dir) * W per lane, float64, f = 4 pi q b with b the float64 lobe of the kept direction.
    reflection_lobe: the directions and weights of resample_lobe_model.resample (pg_resample_lobe) with specular = 1 and the
    same inputs, against the same f."""
    p, nrm, wiv, rough, e = fixed_vertex(N, roughness, eta, wi)
    st, inc = po.rng_seed(N, seed)
    if reflection_lobe:
        r = rl.resample(tree, p, nrm, wiv, rough, np.ones(N, F), st, inc, M, ALPHA, DELTA, weight=weight)
    else:
        r = resample(tree, p, nrm, wiv, rough, e, st, inc, M, ALPHA, DELTA, weight=weight)
    q = tree.pdf(p, r["dir"]).astype(np.float64)
    b = lobe_f64(r["dir"].astype(np.float64), wi, roughness, eta)   # (the normal is +z: local is world)
    return np.where(r["index"] != NONE, 4 * np.pi * q * b * r["weight"].astype(np.float64), 0.0)


def verdict_on_the_reflection_lobe(est, ref, truth):
    """what pg_resample_lobe's model does on this f: 'biased low' (beyond five of its standard errors) or 'larger variance'"""
    se = ref.std(ddof=1) / np.sqrt(ref.shape[0])
    if truth - ref.mean() > 5 * se:
        return "biased low"
    return "larger variance" if ref.var(ddof=1) > est.var(ddof=1) else "neither"


if __name__ == "__main__":
    tree = rs.horizon_lobe_tree()
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_interface", "variance.txt")
    with open(path, "w") as f:
        f.write("# tests/resample_interface_model.py: the estimator f(dir) * W of the integral over the whole sphere of f = 4 pi q(w) b(w) on\n"
                "# horizon_lobe_tree(), normal +z, alpha 0.5, delta 0.1, 2^16 lanes of the float32 model (seed 1234); truth: float64\n"
                "# midpoint quadrature on 2048 x 2048 cells of the equal-area square; |1024^2 - 2048^2| is given in standard errors at M = 1\n"
                "# reflection lobe: pg_resample_lobe's model (specular 1) on the same inputs and the same f, at this M\n"
                "# roughness | eta | wi | truth | quadrature 1024^2 against 2048^2 (standard errors) | M | mean | standard errors off"
                " | sample variance | variance / variance at M = 1 | reflection lobe: mean | standard errors off | variance | verdict\n")
        for roughness, eta, wi in SETTINGS:
            truth = truth_by_quadrature(tree, roughness, eta, wi)
            coarse = truth_by_quadrature(tree, roughness, eta, wi, grid=1024)
            v1 = se1 = None
            for M in (1, 4, 16):
                e = product_estimates(tree, roughness, eta, wi, M)
                ec = product_estimates(tree, roughness, eta, wi, M, reflection_lobe=True)
                var, se = e.var(ddof=1), e.std(ddof=1) / np.sqrt(e.shape[0])
                sec = ec.std(ddof=1) / np.sqrt(ec.shape[0])
                v1, se1 = (var, se) if v1 is None else (v1, se1)
                f.write("%g | %g | (%g, %g, %g) | %.6f | %.4f | %d | %.6f | %.2f | %.6f | %.4f | %.6f | %.2f | %.6f | %s\n"
                        % (roughness, eta, *wi, truth, abs(coarse - truth) / se1, M, e.mean(), abs(e.mean() - truth) / se, var, var / v1,
                           ec.mean(), abs(ec.mean() - truth) / sec, ec.var(ddof=1), verdict_on_the_reflection_lobe(e, ec, truth)))
    print(open(path).read())
