"""tests/irradiance_model.py (the numpy model of include/pgsd_irradiance.h that tests/test_gpu_irradiance.py holds the device to,
bit for bit) against independent references: the nine cell means against a float64 quadrature, the estimate against the true
irradiance of the tree within the bound the header derives, order freedom of the sums, and the statistical weights behind a KD
split.  No GPU."""
import numpy as np
import pytest

import irradiance_model as im
import irradiance_synth as isy
import radiance_model as rm
import synth
from oracle import pg_oracle as po

D = np.float64
EPS = 2.0 ** -53


def basis(x, y, z):
    return [np.ones_like(x), y, z, x, x * y, y * z, 3 * z * z - 1, x * z, x * x - y * y]


def _directions(ix, iy, d, n):
    """Gauss-Legendre nodes of order n over the cell, as unit directions (outer product: z rows, phi columns) with weights
    that sum to 1: the map is equal-area, so the mean over the cell is the mean over (cx, cy)."""
    w = 2.0 ** -d
    t, wt = np.polynomial.legendre.leggauss(n)
    u, wt = (t + 1) / 2, wt / 2
    z = 2 * ((iy + u) * w) - 1
    s = np.sqrt(np.maximum(0.0, 1 - z * z))
    phi = 2 * np.pi * ((ix + u) * w)
    return np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(z, np.ones(n)), np.outer(wt, wt)


def quadrature_means(ix, iy, d, n):
    x, y, z, W = _directions(ix, iy, d, n)
    return np.array([(W * f).sum() for f in basis(x, y, z)])


def converged_means(ix, iy, d):
    """The quadrature refined (order 16, 32, ... 256) until two successive refinements agree to a few ulps or the order is 256
    (sqrt(1 - z^2) is not differentiable at the poles: there the convergence is algebraic); returns the finest values and the
    largest difference between the last two refinements."""
    prev, n = quadrature_means(ix, iy, d, 16), 32
    while True:
        cur = quadrature_means(ix, iy, d, n)
        diff = float(np.abs(cur - prev).max())
        if diff <= 8 * EPS or n == 256:
            return cur, diff
        prev, n = cur, 2 * n


# depth -> cells: a corner at each pole (iy = 0: z = -1; iy = 2^d - 1: z = +1), cells at the seam phi = 0 / 2 pi (ix = 0 and
# ix = 2^d - 1), and cells inside
CELLS = [(0, 0, 0),
         (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1),
         (3, 0, 0), (3, 7, 7), (3, 3, 5), (3, 0, 4), (3, 7, 2), (3, 5, 0),
         (8, 0, 0), (8, 255, 255), (8, 100, 37), (8, 0, 128), (8, 255, 3), (8, 17, 255),
         (20, 0, 0), (20, (1 << 20) - 1, (1 << 20) - 1), (20, 123456, 654321), (20, 0, 777777), (20, (1 << 20) - 1, 31), (20, 99, 0)]


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "d%d-%d-%d" % c)
def test_the_cell_means_equal_a_quadrature(cell):
    """Tolerance, none of it taken from the model: (a) 4 x the difference between the quadrature's last two refinements --
    measured: 1e-16 .. 1e-14 for cells off the poles, 4e-8 (depth 1) .. 8e-11 (depth 20) for cells that touch a pole, where the
    error left at order 256 is a seventh of that difference (n^-3); (b) the precision of float64 in the header's own formulas:
    Zs, Zzs, Zss, C1, S1, C2, S2 are difference quotients -- numerators that are differences of two values of magnitude <= 1,
    each the result of at most eight operations rounded to 2^-53, divided by 2 w or more -- so they carry up to 8 * 2^-53 / w,
    which at depth 20 (1e-9) is what limits them, not the quadrature (whose nodes are not differenced)."""
    d, ix, iy = cell
    m = im.cell_means([ix], [iy], [d])[:, 0]
    ref, diff = converged_means(ix, iy, d)
    tol = 4 * diff + 8 * EPS * 2.0 ** d + 8 * EPS
    err = np.abs(m - ref)
    print("cell", cell, "quadrature difference %.3e" % diff, "tolerance %.3e" % tol, "largest error %.3e" % err.max())
    assert (err <= tol).all(), (cell, err, tol)


def test_a_whole_turn_and_the_whole_square_are_exact():
    """sin of a whole and of half a turn is 0 through the reduction by quarter turns, so the root cell has no harmonics at all."""
    s, c = im.turn(np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0]))
    np.testing.assert_array_equal(s, [0, 1, 0, -1, 0, 0, 0])
    np.testing.assert_array_equal(c, [1, 0, -1, 0, 1, -1, 1])
    m = im.cell_means([0], [0], [0])[:, 0]
    np.testing.assert_array_equal(m, [1, 0, 0, 0, 0, 0, 0, 0, 0])


# ---- the bound ---------------------------------------------------------------------------------------------------------------
def _unit_normals(n, seed):
    return po.canonical_to_dir(synth.canonical_uniform(n, seed)).astype(D)


def _true_irradiance(cols, weights, normals, order):
    """(n_trees, n_normals): the leaf sum of e / N times the quadrature of max(0, n.w) over the cell."""
    tree, ix, iy, d, e = im.leaves_of(cols)
    out = np.zeros((np.asarray(cols["quadtree_rootNodeIndex"]).shape[0], normals.shape[1]), D)
    for t, a, b, dd, ee in zip(tree, ix, iy, d, e):
        x, y, z, W = _directions(int(a), int(b), int(dd), order)
        c = np.maximum(0.0, normals[0][:, None, None] * x + normals[1][:, None, None] * y + normals[2][:, None, None] * z)
        out[t] += (D(ee) / D(weights[t])) * (c * W).sum(axis=(1, 2))
    return out


@pytest.fixture(scope="module")
def bound_forest():
    """Eight ragged trees of depths 0 .. 7, and a ninth with all its energy in ONE cell of the deepest level (the worst case: the
    radiance is a point light).  Read-only."""
    cols = isy.ragged_forest(3, 1, [0, 1, 2, 3, 4, 5, 6, 7, 7], seed=11)

    def energy(tree, ix, iy, d, u):
        e = (np.float32(1) - u).astype(np.float32)
        deepest = np.nonzero((tree == 8) & (d == d[tree == 8].max()))[0]
        return np.where(tree == 8, np.float32(0), e) + np.where(np.arange(e.shape[0]) == deepest[len(deepest) // 2], np.float32(2.5), 0)
    cols = isy.set_energies(cols, 11, energy)
    weights = np.array([1000, 3, 77, 12345, 1 << 20, 5, 40000, 9, 250], np.uint64)
    return cols, weights


def test_the_estimate_lies_within_three_thirtyseconds_of_the_mean_radiance(bound_forest):
    """|E_model - E_true| <= (3/32) R / N, the model at float64, for 300 unit normals per tree.  The only slack is the difference
    between the quadrature of max(0, n.w) at orders 12 and 24, per tree the largest over the normals (measured: 6e-3 of
    R / N for the tree that is one cell, which the kink crosses whatever the normal, down to 1e-5 for the deep trees)."""
    cols, weights = bound_forest
    tree, ix, iy, d, e = im.leaves_of(cols)
    assert np.unique(tree).shape[0] == 9 and d.max() == 7 and (np.bincount(tree) > 64).any()
    root = np.asarray(cols["quadtree_rootNodeIndex"], np.int64)
    R = np.asarray(cols["quadtree_irradiance"], np.float32)[root].astype(D)
    lit = e[tree == 8]
    assert (lit > 0).sum() == 1 and R[8] == 2.5
    normals = _unit_normals(300, 41)
    k = im.coefficients(cols, weights, D)
    E_model = np.stack([im.evaluate(np.repeat(k[t:t + 1], normals.shape[1], axis=0), normals, D) for t in range(9)])
    coarse, fine = _true_irradiance(cols, weights, normals, 12), _true_irradiance(cols, weights, normals, 24)
    slack = np.abs(fine - coarse).max(axis=1)
    bound = (3.0 / 32.0) * R / weights.astype(D)
    err = np.abs(E_model - fine)
    for t in range(9):
        print("tree %d: largest error %.4f of R/N, bound 0.09375, quadrature slack %.2e of R/N"
              % (t, err[t].max() * weights[t] / R[t], slack[t] * weights[t] / R[t]))
    assert (err <= (bound + slack)[:, None]).all()
    # the point light comes close to the bound for normals nearly perpendicular to it; the bound is not slack
    assert err[8].max() > 0.5 * bound[8]


def test_an_isotropic_tree_gives_pi_times_its_radiance():
    """A tree whose root is the leaf, R = 4 pi N L0 (rounded to fp32): pi L0 for every normal to fp32 rounding (k0 itself is one
    rounding of R / (4 N); the other coefficients are exactly 0 for the whole square, a few quanta at the most)."""
    cols = isy.ragged_forest(0, 0, [0], seed=3)
    L0, N = 0.7, 12345
    cols["quadtree_irradiance"] = np.array([4 * np.pi * N * L0], np.float32)
    k = im.coefficients(cols, np.array([N], np.uint64))
    quantum = 2.0 ** -50 * im.G * float(cols["quadtree_irradiance"][0]) / N
    assert (np.abs(k[0, 1:].astype(D)) <= 4 * quantum[1:]).all()
    assert abs(float(k[0, 0]) - np.pi * L0) <= 2.0 ** -23 * np.pi * L0
    normals = _unit_normals(200, 9).astype(np.float32)
    E = im.evaluate(np.repeat(k, 200, axis=0), normals)
    assert (np.abs(E.astype(D) - np.pi * L0) <= 2.0 ** -22 * np.pi * L0).all()
    np.testing.assert_array_equal(im.evaluate(k, None), k[:, 0])


def test_the_sums_do_not_depend_on_the_order_of_the_leaves(bound_forest):
    cols, weights = bound_forest
    n = im.leaves_of(cols)[0].shape[0]
    s = im.tree_sums(cols)
    np.testing.assert_array_equal(im.tree_sums(cols, np.arange(n)[::-1]), s)
    np.testing.assert_array_equal(im.tree_sums(cols, np.argsort(synth.uniform(n, 5)[0], kind="stable")), s)
    # the polynomials lie within [-1, 2], so |sum_j| < 2.1 * 2^50 for consistent energies (3 z^2 - 1 of a point light at a pole
    # comes close to 2), and sum_0 is the leaves' share of the root: 2^50 up to the fp32 roundings
    assert (np.abs(s.view(np.int64)) < 2.1 * 2.0 ** 50).all()
    assert (np.abs(s.view(np.int64)[:, 0] - 2.0 ** 50) < 2.0 ** 50 * 64 * 2.0 ** -24).all()


def test_zero_weight_and_unusable_roots_give_zero():
    cols = isy.ragged_forest(2, 0, [2], seed=4)
    irr = cols["quadtree_irradiance"].copy()
    tree = isy.node_cells(cols)[0]
    irr[tree == 1] = 0                       # a tree without energy
    irr[cols["quadtree_rootNodeIndex"][2]] = np.inf
    cols["quadtree_irradiance"] = irr
    k = im.coefficients(cols, np.array([0, 5, 5, 5], np.uint64))
    assert not k[:3].any() and k[3, 0] > 0 and np.isfinite(k).all()


def test_both_children_of_a_kd_split_carry_the_parents_weight():
    """A refine that splits KD leaves hands each child a copy of the quadtree with the full energy: with carried_weights (the
    record count of the leaf the energies were resolved from) both children give the same E; vertCount, which is halved per
    split, would double it."""
    BB0, BB1 = isy.BB0, isy.BB1
    pair = po.OracleSDTreePair()
    pair.setup(BB0, BB1, 20, 20, True)
    for it in range(2):
        rec = rm.corner_records(1 << (14 + it), 500 + it, BB0, BB1, radiance=1.0)
        synth.splat(pair.current, rec)
        old_cols, count = pair.current.export(), pair.current.kd_column("count")
        pair.refine_and_prepare(it)
    cols = pair.prev.export()
    w = rm.carried_weights(old_cols, count, cols)
    splits = rm.splits_between(old_cols, cols)
    assert splits.max() >= 1
    leaf, tree, src = rm.source_leaves(old_cols, cols)
    k = im.coefficients(cols, w, D)
    halved = np.asarray(cols["kdtree_vertCount"], D)[leaf]
    normal = np.array([[0.0], [0.6], [0.8]])
    seen = 0
    for s in np.unique(src):
        sib = tree[src == s]
        if sib.shape[0] < 2:
            continue
        E = np.array([im.evaluate(k[t:t + 1], normal, D)[0] for t in sib])
        assert E[0] > 0 and (E == E[0]).all()              # copies of one quadtree, one weight
        # the constant field of radiance 1 has E = pi; with N records behind the energies the estimate is near it ...
        assert abs(E[0] / np.pi - 1) < 0.25, E[0]
        # ... and vertCount (N / 2^splits) would give 2^splits times as much
        vc = halved[np.isin(tree, sib)]
        assert (w[sib][0] / vc >= 1.9).all()
        seen += 1
    assert seen >= 1
