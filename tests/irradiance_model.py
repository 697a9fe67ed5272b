"""Model of include/pgsd_irradiance.h in numpy, written from the header, one operation per header operation: the means of
the nine polynomials over a cell, the exact integer sums of a tree, the coefficients, the estimate (pg_irradiance_query) and
the decision (pg_irradiance_rr: radiance_model.decide with L replaced by E).  It runs on the columns of an export() plus the
weight array of pgsd_radiance.h.

The table is float64 arithmetic with + - * / sqrt rint only, so the device must equal it bit for bit.  `ftype` chooses what
the estimate is evaluated in: float32 is the device's, float64 (coefficients left unrounded) the reference of the bound of
tests/test_irradiance_model.py.

Test infrastructure; the product never imports it.
"""
from __future__ import annotations

import numpy as np

import radiance_model as rm
from oracle import pg_oracle as po

D = np.float64
TWO_PI = D(6.283185307179586)
FOUR_PI = D(12.566370614359172)
HALF_PI = D(1.57079632679489661923)
G = np.array([0.25, 0.5, 0.5, 0.5, 0.9375, 0.9375, 0.078125, 0.9375, 0.234375], D)     # A_l K_lm^2, all exact
Q = D(2.0 ** 50)


def atan_unit(t):
    """pgsd.h's atan on [0, 1]: reduction at sqrt 2 - 1, twenty terms."""
    t = np.asarray(t, D)
    big = t > D(0.41421356237309504880)
    u = np.where(big, (t - D(1)) / (t + D(1)), t)
    base = np.where(big, D(0.78539816339744830962), D(0))
    z = u * u
    p = D(-1.0 / 39.0)
    for k in range(37, 0, -2):
        sign = 1.0 if (k // 2) % 2 == 0 else -1.0
        p = D(sign / k) + z * p
    return base + u * p


def asin_zs(z, s):
    a = np.abs(z)
    steep = a > s
    hi, lo = np.where(steep, a, s), np.where(steep, s, a)
    v = atan_unit(lo / hi)
    v = np.where(steep, HALF_PI - v, v)
    return np.where(z < 0, -v, v)


_PS = [1.0 / 355687428096000.0, -1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0,
       1.0 / 120.0, -1.0 / 6.0]
_PC = [-1.0 / 6402373705728000.0, 1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0,
       1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5]


def turn(f):
    """(sin, cos) of 2 pi f for a dyadic f in [0, 2]: k = rint(4 f), r = (f - k / 4) 2 pi, the two series of pgsd.h's sincos."""
    f = np.asarray(f, D)
    k = np.rint(D(4) * f)
    r = (f - k * D(0.25)) * TWO_PI
    z = r * r
    ps = D(_PS[0])
    for c in _PS[1:]:
        ps = D(c) + z * ps
    sr = r + r * (z * ps)
    pc = D(_PC[0])
    for c in _PC[1:]:
        pc = D(c) + z * pc
    cr = D(1) + z * pc
    q = k.astype(np.int64) & 3
    s = np.where(q == 0, sr, np.where(q == 1, cr, np.where(q == 2, -sr, -cr)))
    c = np.where(q == 0, cr, np.where(q == 1, -sr, np.where(q == 2, -cr, sr)))
    return s, c


def cell_means(ix, iy, d):
    """(9, n) float64: the means of b = (1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2) over the cells (ix, iy) of depth d."""
    ix, iy = np.asarray(ix, np.int64).astype(D), np.asarray(iy, np.int64).astype(D)
    w = np.ldexp(D(1), -np.asarray(d, np.int32))
    x0, x1 = ix * w, (ix + D(1)) * w
    y0, y1 = iy * w, (iy + D(1)) * w
    z0, z1 = D(2) * y0 - D(1), D(2) * y1 - D(1)
    s0, s1 = np.sqrt(D(1) - z0 * z0), np.sqrt(D(1) - z1 * z1)
    F0, F1 = (z0 * s0 + asin_zs(z0, s0)) / D(2), (z1 * s1 + asin_zs(z1, s1)) / D(2)
    Zz = (z0 + z1) / D(2)
    Zs = (F1 - F0) / (D(2) * w)
    Zzs = (D(0) - ((s1 * s1) * s1 - (s0 * s0) * s0)) / (D(6) * w)
    Zss = ((z1 - ((z1 * z1) * z1) / D(3)) - (z0 - ((z0 * z0) * z0) / D(3))) / (D(2) * w)
    Z20 = ((z1 * z1 + z1 * z0) + z0 * z0) - D(1)
    sa0, ca0 = turn(x0)
    sa1, ca1 = turn(x1)
    sb0, cb0 = turn(D(2) * x0)
    sb1, cb1 = turn(D(2) * x1)
    C1, S1 = (sa1 - sa0) / (TWO_PI * w), (ca0 - ca1) / (TWO_PI * w)
    C2, S2 = (sb1 - sb0) / (FOUR_PI * w), (cb0 - cb1) / (FOUR_PI * w)
    return np.stack([np.ones_like(Zz), Zs * S1, Zz, Zs * C1, (Zss * S2) / D(2), Zzs * S1, Z20, Zzs * C1, Zss * C2])


def leaves_of(cols):
    """(tree, ix, iy, d, e) of every directional leaf of every quadtree: child k + 1 of the export is child k of the header."""
    root = np.asarray(cols["quadtree_rootNodeIndex"], np.int64)
    is_leaf = np.asarray(cols["quadtree_isLeaf"], bool)
    irr = np.asarray(cols["quadtree_irradiance"], np.float32)
    ch = [np.asarray(cols["quadtree_child_%d_index" % k], np.int64) for k in (1, 2, 3, 4)]
    node, tree = root.copy(), np.arange(root.shape[0], dtype=np.int64)
    ix, iy, d = np.zeros_like(node), np.zeros_like(node), np.zeros_like(node)
    out = []
    while node.size:
        lf = is_leaf[node]
        out.append((tree[lf], ix[lf], iy[lf], d[lf], irr[node[lf]]))
        node, tree, ix, iy, d = node[~lf], tree[~lf], ix[~lf], iy[~lf], d[~lf]
        node = np.concatenate([ch[k][node] for k in range(4)])
        ix = np.concatenate([2 * ix + (1 if k in (0, 3) else 0) for k in range(4)])
        iy = np.concatenate([2 * iy + (1 if k in (0, 1) else 0) for k in range(4)])
        tree, d = np.tile(tree, 4), np.tile(d + 1, 4)
    return tuple(np.concatenate(c) for c in zip(*out))


def tree_sums(cols, order=None):
    """(n_trees, 9) uint64: the exact sums modulo 2^64.  order: a permutation of the leaves (the sums do not depend on it)."""
    tree, ix, iy, d, e = leaves_of(cols)
    if order is not None:
        tree, ix, iy, d, e = (a[order] for a in (tree, ix, iy, d, e))
    root = np.asarray(cols["quadtree_rootNodeIndex"], np.int64)
    R = np.asarray(cols["quadtree_irradiance"], np.float32)[root].astype(D)[tree]
    m = cell_means(ix, iy, d)
    with np.errstate(all="ignore"):
        t = (e.astype(D) / R) * m
        t = np.where(t == t, t, D(0))
        t = np.clip(t, D(-1024), D(1024))
        q = np.rint(t * Q).astype(np.int64)
    sums = np.zeros((root.shape[0], 9), np.uint64)
    for j in range(9):
        np.add.at(sums[:, j], tree, q[j].view(np.uint64))
    return sums


def coefficients(cols, weights, ftype=np.float32, sums=None):
    """(n_trees, 9): k_j = (ftype)(((sum_j 2^-50) g_j) (R / N)); 0 where N == 0 or R is not positive or not finite."""
    root = np.asarray(cols["quadtree_rootNodeIndex"], np.int64)
    R = np.asarray(cols["quadtree_irradiance"], np.float32)[root]
    N = np.asarray(weights, np.uint64)
    s = tree_sums(cols) if sums is None else sums
    usable = (N != 0) & (R > 0) & np.isfinite(R)
    with np.errstate(all="ignore"):
        ratio = R.astype(D) / np.where(usable, N, 1).astype(D)
        k = ((s.view(np.int64).astype(D) * D(2.0 ** -50)) * G[None, :]) * ratio[:, None]
        k = np.where(usable[:, None], k, D(0)).astype(ftype)
    return k


def evaluate(k, normal, ftype=np.float32):
    """E of rows k (n, 9) for normals (3, n) or None, operation by operation in ftype."""
    T = ftype
    k = np.asarray(k).astype(T)
    S = k[:, 0]
    if normal is None:
        with np.errstate(all="ignore"):
            return np.where(S > 0, S, T(0)).astype(T)
    nx, ny, nz = (np.asarray(normal)[a].astype(T) for a in range(3))
    with np.errstate(all="ignore"):
        S = (S + (k[:, 1] * ny).astype(T)).astype(T)
        S = (S + (k[:, 2] * nz).astype(T)).astype(T)
        S = (S + (k[:, 3] * nx).astype(T)).astype(T)
        S = (S + ((k[:, 4] * nx).astype(T) * ny).astype(T)).astype(T)
        S = (S + ((k[:, 5] * ny).astype(T) * nz).astype(T)).astype(T)
        S = (S + (k[:, 6] * (((T(3) * nz).astype(T) * nz).astype(T) - T(1)).astype(T)).astype(T)).astype(T)
        S = (S + ((k[:, 7] * nx).astype(T) * nz).astype(T)).astype(T)
        S = (S + (k[:, 8] * ((nx * nx).astype(T) - (ny * ny).astype(T)).astype(T)).astype(T)).astype(T)
        E = np.where(S > 0, S, T(0)).astype(T)
        ok = np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz)
    return np.where(ok, E, T(0)).astype(T)


class IrradianceModel:
    def __init__(self, cols, weights, ftype=np.float32, coeff=None):
        self.T = ftype
        self.rad = rm.RadianceModel(cols, weights)
        self.k = coefficients(cols, weights, ftype) if coeff is None else np.asarray(coeff, ftype)

    def estimate(self, p, normal=None, active=None):
        n = np.asarray(p).shape[1]
        act = np.ones(n, bool) if active is None else np.asarray(active) != 0
        t = self.rad.tree_of(p, None)
        E = evaluate(self.k[t], normal, self.T)
        return np.where(act, E, self.T(0)).astype(self.T)

    def roulette(self, p, normal, weight, reference, state, inc, window, max_split, active=None):
        """(count uint32, scale, E); `state` advances in place by ONE draw per active lane."""
        n = np.asarray(p).shape[1]
        act = np.ones(n, bool) if active is None else np.asarray(active) != 0
        E = self.estimate(p, normal, active)
        st = np.ascontiguousarray(state[act])
        xi_act = po.rng_next_f32(st, np.ascontiguousarray(inc[act]))
        state[act] = st
        xi = np.zeros(n, np.float32)
        xi[act] = xi_act
        count, scale = rm.decide(E, weight, reference, xi, window, max_split, self.T)
        count = np.where(act, count, 1).astype(np.uint32)
        scale = np.where(act, scale, self.T(1)).astype(self.T)
        return count, scale, E
