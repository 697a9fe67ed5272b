"""pg_resample_cosine (include/pg_resample.h) restated in numpy float32: vectorised over the lanes, a Python loop over the
candidates.  Built from the unchanged oracle -- OracleTree.sample, OracleTree.pdf and rng_next_f32 of oracle/pg_oracle.py -- and,
for the cosine candidates, from the oracle's own diffuse BSDF sample (bsdf_probe of a diffuse row with wi = +z: Mitsuba's
square_to_cosine_hemisphere) and Duff et al.'s basis written out below operation by operation.  It takes nothing from the device.

Every array operation below is ONE fp32 operation per element (numpy rounds each on its own; there is no contraction), in the
order the header states them.

Test infrastructure; the product never imports it.  Run as a program it writes profiles/resample/variance.txt.
"""
from __future__ import annotations

import os

import numpy as np

from oracle import pg_oracle as po

F = np.float32
INV_PI = F(0.31830988618379067154)
INV_4PI = F(0.07957747154594766788)
NONE = 0xFFFFFFFF
OUT_FIELDS = ("dir", "weight", "target", "source")          # fp32 columns of a result
CAND_FIELDS = ("cand_dir", "cand_target", "cand_source")


# ---- the contribution weight: the header's, and two deliberately wrong ones (tests/test_resample_model.py rejects them) ----
def weight_of_the_header(wsum, M, t_kept, s_kept):
    return (wsum / F(M)) / t_kept


def weight_without_one_over_m(wsum, M, t_kept, s_kept):
    return wsum / t_kept


def weight_one_over_source(wsum, M, t_kept, s_kept):
    return F(1) / s_kept


def cosine_local(u1, u2):
    """square_to_cosine_hemisphere(u1, u2) per lane, (3, m): the direction the oracle's diffuse BSDF samples for wi = +z."""
    m = u1.shape[0]
    if m == 0:
        return np.zeros((3, 0), F)
    wi = np.tile(np.array([0, 0, 1], F), (m, 1))
    u = np.stack([np.full(m, 0.5, F), u1, u2], axis=1).astype(F)
    swo = po.bsdf_probe(np.zeros((1, 16), F), np.zeros(m, np.int32), wi, wi, u, level=0)[2]
    return np.ascontiguousarray(swo.T)


def duff_frame(n):
    """Mitsuba's coordinate_system(n) (Duff et al. 2017) as the renderer computes it: s, t of n (3, m), fp32."""
    nx, ny, nz = n
    sign = np.where(np.signbit(nz), F(-1), F(1)).astype(F)
    a = F(-1) / (sign + nz)
    b = (nx * ny) * a
    s = np.stack([F(1) + (sign * (nx * nx)) * a, sign * b, (-sign) * nx])
    t = np.stack([b, sign + (ny * ny) * a, -ny])
    return s.astype(F), t.astype(F)


def to_world(s, t, n, v):
    """(s * v.x + t * v.y) + n * v.z, per component"""
    return ((s * v[0] + t * v[1]) + n * v[2]).astype(F)


def resample(tree, p, normal, st, inc, M, alpha, delta, active=None, weight=weight_of_the_header, candidates=False):
    """-> {"dir" (3, n), "weight", "target", "source" fp32 (n,), "index" uint32 (n,)} (+ "cand_dir" (M, 3, n), "cand_target",
    "cand_source" (M, n)).  st (uint64 (n,)) is advanced in place, as the oracle's own calls do."""
    p = np.ascontiguousarray(p, F)
    normal = np.ascontiguousarray(normal, F)
    n = p.shape[1]
    assert p.shape == normal.shape == (3, n) and st.shape == inc.shape == (n,) and st.dtype == inc.dtype == np.uint64
    assert 1 <= M <= 64
    alpha, delta = F(alpha), F(delta)
    assert 0 <= alpha <= 1 and 0 <= delta <= 1
    om, d4, omd = F(1) - alpha, delta * INV_4PI, F(1) - delta
    live = np.isfinite(normal).all(axis=0)
    if active is not None:
        live &= np.asarray(active) != 0
    idx = np.nonzero(live)[0]
    m = idx.shape[0]
    P, Nn = np.ascontiguousarray(p[:, idx]), np.ascontiguousarray(normal[:, idx])
    S, I = st[idx].copy(), inc[idx].copy()
    wsum = np.zeros(m, F)
    kdir = np.tile(np.array([[0], [0], [-1]], F), (1, m))
    kt, ks, kk = np.zeros(m, F), np.zeros(m, F), np.full(m, NONE, np.uint32)
    cd, ct, cs = np.zeros((M, 3, n), F), np.zeros((M, n), F), np.zeros((M, n), F)
    with np.errstate(all="ignore"):
        fs, ft = duff_frame(Nn)
        for k in range(M):
            xi = po.rng_next_f32(S, I)
            from_tree = xi > alpha
            w, q = np.empty((3, m), F), np.empty(m, F)
            j = np.nonzero(from_tree)[0]
            if j.size:
                sj, ij = S[j].copy(), I[j].copy()
                w[:, j], q[j] = tree.sample(np.ascontiguousarray(P[:, j]), sj, ij)
                S[j] = sj
            j = np.nonzero(~from_tree)[0]
            if j.size:
                sj, ij = S[j].copy(), I[j].copy()
                u1 = po.rng_next_f32(sj, ij)
                u2 = po.rng_next_f32(sj, ij)
                S[j] = sj
                wj = to_world(fs[:, j], ft[:, j], Nn[:, j], cosine_local(u1, u2))
                w[:, j], q[j] = wj, tree.pdf(np.ascontiguousarray(P[:, j]), np.ascontiguousarray(wj))
            d = (Nn[0] * w[0] + Nn[1] * w[1]) + Nn[2] * w[2]
            c = np.where(d > 0, d * INV_PI, F(0)).astype(F)
            s = alpha * c + om * q
            t = c * (d4 + omd * q)
            r = t / s
            wk = np.where((s > 0) & (t > 0) & np.isfinite(r), r, F(0)).astype(F)
            zeta = po.rng_next_f32(S, I)
            wsum = wsum + wk
            keep = (wk > 0) & (zeta * wsum < wk)
            kk[keep] = k
            kdir[:, keep], kt[keep], ks[keep] = w[:, keep], t[keep], s[keep]
            cd[k][:, idx], ct[k, idx], cs[k, idx] = w, t, s
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
    return out


# ---- the trees of the tests ---------------------------------------------------------------------------------------------------
BB0, BB1 = [0.0] * 3, [100.0] * 3
HORIZON_NORMAL = (0.0, 0.0, 1.0)


def single_leaf_tree():
    """One KD leaf whose quadtree is one leaf: isotropic, the pdf is 1 / (4 pi) everywhere."""
    t = po.OracleTree()
    t.setup(BB0, BB1, 20, 20, True)
    return t


def complete_tree(depth, leaf_energy, seed=7):
    """One KD leaf with a complete quadtree of `depth` levels; leaf_energy(tree, ix, iy, d, u) as irradiance_synth.set_energies."""
    import irradiance_synth as isy
    t = po.OracleTree()
    t.setup(BB0, BB1, 20, 20, True)
    for _ in range(depth):
        t.quad_split(t.quad_all_leaves())
    t.load(isy.set_energies(t.export(), seed, leaf_energy))
    return t


def dark_tree():
    """A tree without energy: every node of its two-level quadtree holds 0."""
    return complete_tree(2, lambda tree, ix, iy, d, u: np.zeros_like(u))


def horizon_lobe_tree():
    """16 x 16 cells; canonical y is (cos theta + 1) / 2, so rows 7 and 8 lie on either side of the horizon of the normal +z:
    a bright lobe of 2 x 2 cells there -- half of it behind the surface, the other half at a cosine below 1/8 -- over a dim
    background.  The tree alone samples the lobe at full rate; the product is almost nothing there."""
    def energy(tree, ix, iy, d, u):
        lobe = ((iy == 7) | (iy == 8)) & ((ix == 3) | (ix == 4))
        return np.where(lobe, F(40), F(0.02) + F(0.1) * u).astype(F)
    return complete_tree(4, energy)


def fixed_vertex(n):
    """n lanes at the centre of the box with the normal +z"""
    return np.full((3, n), 50, F), np.tile(np.array(HORIZON_NORMAL, F)[:, None], (1, n))


def variance_of_the_product(tree, M, N=1 << 16, seed=1234, delta=0.1, alpha=0.5):
    """sample variance of the estimator of the integral of 4 pi q(w) c(w), q the tree's density: f(dir) * W over N lanes"""
    p, nrm = fixed_vertex(N)
    st, inc = po.rng_seed(N, seed)
    r = resample(tree, p, nrm, st, inc, M, alpha, delta)
    q = tree.pdf(p, r["dir"]).astype(np.float64)
    c = np.maximum(r["dir"][2].astype(np.float64), 0) / np.pi
    est = 4 * np.pi * q * c * r["weight"].astype(np.float64)
    return float(est.var(ddof=1)), float(est.mean())


if __name__ == "__main__":
    tree = horizon_lobe_tree()
    rows = [(M,) + variance_of_the_product(tree, M) for M in (1, 4, 16)]
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample", "variance.txt")
    with open(path, "w") as f:
        f.write("# tests/resample_model.py: the estimator f(dir) * W of the integral of f = 4 pi q(w) c(w) on horizon_lobe_tree(),\n"
                "# normal +z, alpha 0.5, delta 0.1, 2^16 lanes of the float32 model (seed 1234)\n"
                "# M | mean | sample variance | variance / variance at M = 1\n")
        for M, var, mean in rows:
            f.write("%d | %.6f | %.6f | %.4f\n" % (M, mean, var, var / rows[0][1]))
    print(open(path).read())
