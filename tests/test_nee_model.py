"""tests/nee_model.py -- the numpy float32 restatement of include/ext/lights/pg_nee.h -- held to answers that are known without it
(no GPU needed): the prepare step against a float64 cross product, W s = 1 at M = 1, the streams' advance, the kept point on its
light, the lights that can never be kept, and the unbiasedness of f(y) W against a float64 quadrature of a scene written out
below, at M = 1, 4 and 16, with two wrong weights rejected by the same test.

Run as a program it writes profiles/nee/variance.txt."""
import functools
import os

import numpy as np
import pytest

import nee_model as nm
from oracle import pg_oracle as po

F = np.float32
ULP = float(np.finfo(F).eps)             # 2^-23: one step of a number in [1, 2)


# ---- a few lights of every kind around a vertex, for the known answers ---------------------------------------------------------
def _some_lights(L, seed):
    """L lights in a box of side 100: parallelograms and triangles, one- and two-sided, radiance 0.5 .. 8"""
    import synth
    u = synth.uniform(L, seed, 12)
    o = np.stack([u[0], u[1], u[2]], axis=1) * F(100)
    a = (np.stack([u[3], u[4], u[5]], axis=1) - F(0.5)) * F(40)
    b = (np.stack([u[6], u[7], u[8]], axis=1) - F(0.5)) * F(40)
    return nm.table(o, a, b, F(0.5) + u[9] * F(7.5), u[10] < 0.5, u[11] < 0.5)


def _lanes(n, seed):
    import synth
    p = synth.positions_uniform(n, seed, [0.0] * 3, [100.0] * 3)
    return p, synth.directions_uniform(n, seed + 1)


def _one_leaf(L, row=None):
    """rows of a single leaf (unlearned unless a row is given) and every lane in it"""
    rows = np.zeros((1, L), np.uint32) if row is None else np.array(row, np.uint32).reshape(1, L)
    return rows


def _row_of(k):
    return np.cumsum(np.array(k, np.uint64)).astype(np.uint32)


# ---- the prepare step ------------------------------------------------------------------------------------------------------
def test_prepare_agrees_with_a_float64_cross_product():
    t = _some_lights(257, 3)
    r = nm.prepare(t)
    a, b = t["edge_a"].astype(np.float64), t["edge_b"].astype(np.float64)
    c = np.cross(a, b)
    ln = np.linalg.norm(c, axis=1)
    # a component of c is a difference of two rounded products: 2 * 2^-24 of the products' magnitude, one more rounding of the
    # difference; the length adds three roundings of squares, two of sums and the root's: 1e-6 of |a| |b| covers them all
    scale = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
    assert (ln > 1e-2 * scale).all()                                   # (no light of the set is close to degenerate)
    area = np.where(t["triangle"], 0.5 * ln, ln)
    assert (np.abs(r["N"].astype(np.float64) * ln[:, None] - c) <= 1e-6 * scale[:, None]).all()
    assert (np.abs(1.0 / r["invA"].astype(np.float64) - area) <= 1e-6 * scale).all()
    assert (np.abs(np.linalg.norm(r["N"].astype(np.float64), axis=1) - 1) <= 4 * ULP).all()
    np.testing.assert_array_equal(r["radiance"], t["radiance"])
    assert r["kind"].any() and (~r["kind"]).any() and r["two_sided"].any() and (~r["two_sided"]).any()


def test_a_degenerate_light_has_no_area():
    # parallel edges, a zero edge, both zero, and edges so long that the squared length overflows
    t = nm.table([[0, 0, 0]] * 5, [[1, 2, 3], [0, 0, 0], [0, 0, 0], [3e19, 0, 0], [1, 0, 0]],
                 [[2, 4, 6], [1, 0, 0], [0, 0, 0], [0, 3e19, 0], [0, 1, 0]], [1] * 5, [0, 1, 0, 1, 1], [1] * 5)
    r = nm.prepare(t)
    np.testing.assert_array_equal(r["invA"], np.array([0, 0, 0, 0, 2], F))
    assert not nm.accepted(nm.table([[0, 0, np.nan]], [[1, 0, 0]], [[0, 1, 0]], [1], [0], [0]))
    assert not nm.accepted(nm.table([[0, 0, 0]], [[np.inf, 0, 0]], [[0, 1, 0]], [1], [0], [0]))
    assert not nm.accepted(nm.table([[0, 0, 0]], [[1, 0, 0]], [[0, 1, 0]], [-1e-3], [0], [0]))
    assert not nm.accepted(nm.table([[0, 0, 0]], [[1, 0, 0]], [[0, 1, 0]], [np.inf], [0], [0]))
    # in a launch it is never kept, whatever the row says
    n = 4096
    p, nrm = _lanes(n, 5)
    st, inc = po.rng_seed(n, 6)
    out = nm.resample(_one_leaf(5, _row_of([65536, 65536, 65536, 65536, 1])), np.zeros(n, int), 0.1, r, p, nrm, st, inc, 8, candidates=True)
    kept = out["index"] != nm.NONE
    assert kept.sum() > 50 and (out["light"][kept] == 4).all() and (out["cand_light"] != 4).sum() > 8 * n // 2


# ---- M = 1 is the one-sample estimator of the source -----------------------------------------------------------------------------
@pytest.mark.parametrize("row", ["unlearned", "learned"])
def test_one_candidate_weighs_one_over_the_source(row):
    L, n = 16, 1 << 14
    lights = nm.prepare(_some_lights(L, 11))
    p, nrm = _lanes(n, 12)
    st, inc = po.rng_seed(n, 13)
    rows = _one_leaf(L, None if row == "unlearned" else _row_of([(7 * j) % 5 * 16384 + (j == 3) * 65536 for j in range(L)]))
    out = nm.resample(rows, np.zeros(n, int), 0.1, lights, p, nrm, st, inc, 1)
    kept = out["index"] != nm.NONE
    assert kept.sum() > n // 16 and (~kept).sum() > n // 16
    # W = (t / s) / t, two roundings: within 2 ulp of 1 / s
    ws = out["weight"][kept].astype(np.float64) * out["source"][kept].astype(np.float64)
    assert (np.abs(ws - 1) <= 2 * ULP).all(), np.abs(ws - 1).max() / ULP
    assert (out["index"][kept] == 0).all() and (out["weight"][~kept] == 0).all() and (out["light"][~kept] == nm.NONE).all()


# ---- the streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 64])
def test_valid_lanes_advance_by_four_draws_a_candidate_and_invalid_lanes_by_none(M):
    L, n = 9, 515
    lights = nm.prepare(_some_lights(L, 21))
    p, nrm = _lanes(n, 22)
    nrm = nrm.copy()
    nrm[0, 3], nrm[1, 4], nrm[2, 5] = np.nan, np.inf, -np.inf
    p = p.copy()
    p[:, 10] = [np.nan, 1, 1]                                 # a position is never a reason to skip the draws
    p[:, 11] = [-5, 50, 50]
    act = np.ones(n, np.uint8)
    act[20::3] = 0
    off = np.zeros(n, bool)
    off[[3, 4, 5]] = True
    off |= act == 0
    st, inc = po.rng_seed(n, 23)
    want = st.copy()
    for _ in range(4 * M):
        po.rng_next_f32(want, inc)
    want[off] = po.rng_seed(n, 23)[0][off]
    out = nm.resample(_one_leaf(L), np.where(np.arange(n) == 11, -1, 0), 0.1, lights, p, nrm, st, inc, M, active=act, candidates=True)
    np.testing.assert_array_equal(st, want)
    assert (out["index"][off] == nm.NONE).all() and (out["light"][off] == nm.NONE).all()
    for k in nm.OUT_FIELDS + nm.CAND_FIELDS + nm.CAND_FLAGS:
        assert (out[k][..., off] == 0).all(), k
    assert (out["index"][10] == nm.NONE) and (out["cand_target"][:, 10] == 0).all() and (out["cand_source"][:, 10] > 0).any()


# ---- the kept point lies on its light ----------------------------------------------------------------------------------------
def _barycentric(t, light, y):
    """float64 (e1, e2, distance from the light's plane) of points y (3, n) on lights `light`"""
    o, a, b = (t[k].astype(np.float64)[light] for k in ("origin", "edge_a", "edge_b"))
    v = y.astype(np.float64).T - o
    aa, ab, bb = (a * a).sum(1), (a * b).sum(1), (b * b).sum(1)
    va, vb = (v * a).sum(1), (v * b).sum(1)
    det = aa * bb - ab * ab
    e1, e2 = (va * bb - vb * ab) / det, (vb * aa - va * ab) / det
    off = np.linalg.norm(v - e1[:, None] * a - e2[:, None] * b, axis=1)
    return e1, e2, off


def test_the_kept_point_lies_on_its_light():
    L, n = 12, 1 << 14
    t = _some_lights(L, 31)
    lights = nm.prepare(t)
    p, nrm = _lanes(n, 32)
    st, inc = po.rng_seed(n, 33)
    out = nm.resample(_one_leaf(L), np.zeros(n, int), 0.1, lights, p, nrm, st, inc, 4, candidates=True)
    kept = out["index"] != nm.NONE
    assert kept.sum() > n // 8
    # y = (o + e1 a) + e2 b in fp32 with coordinates up to 120: 4 roundings of 2^-24 * 120 -- 1e-4 in space, 1e-5 of an edge of 10
    tol = 1e-4
    for light, y in [(out["light"][kept], out["point"][:, kept])] + [(out["cand_light"][k], out["cand_point"][k]) for k in range(4)]:
        e1, e2, off = _barycentric(t, light, y)
        assert (off <= tol).all()
        assert (e1 >= -tol).all() and (e2 >= -tol).all() and (e1 <= 1 + tol).all() and (e2 <= 1 + tol).all()
        tri = t["triangle"][light]
        assert tri.sum() > 100 and (e1[tri] + e2[tri] <= 1 + tol).all()
        assert (e1[~tri] + e2[~tri] > 1.2).any()                           # a parallelogram is not folded
    # the direction and the distance are the point's
    d = out["point"][:, kept].astype(np.float64) - p[:, kept].astype(np.float64)
    dist = np.linalg.norm(d, axis=0)
    assert (np.abs(out["dist"][kept] - dist) <= 4 * ULP * dist).all()
    assert (np.abs(out["dir"][:, kept] - d / dist) <= 4 * ULP).all()


def test_the_triangles_fold_and_its_diagonal():
    """the fold itself, on draws that are given: past the diagonal a point is reflected into the triangle, on it it stays"""
    t = nm.table([[10, 20, 30]], [[8, 0, 0]], [[0, 4, 0]], [1], [1], [1])
    lights = nm.prepare(t)
    e = np.array([[0.75, 0.75], [0.5, 0.5], [0.25, 0.75], [1 - 2.0 ** -24, 2.0 ** -23], [0.25, 0.25], [0.0, 0.0]], F)
    # (the fourth: e1 + e2 = 1 + 2^-24 rounds to 1 in fp32, which is not past the diagonal)
    want = np.array([[0.25, 0.25], [0.5, 0.5], [0.25, 0.75], [1 - 2.0 ** -24, 2.0 ** -23], [0.25, 0.25], [0.0, 0.0]], np.float64)
    n = e.shape[0]

    class Given:                                              # the stream of a lane, with the two draws of the point given
        calls = 0

    def fake(S, I):
        Given.calls += 1
        return {2: e[:, 0].copy(), 3: e[:, 1].copy()}.get(Given.calls, np.full(n, 0.25, F))

    real, po.rng_next_f32 = po.rng_next_f32, fake
    try:
        st, inc = po.rng_seed(n, 1)
        out = nm.resample(_one_leaf(1), np.zeros(n, int), 0.1, lights, np.tile(np.array([[12], [21], [35]], F), (1, n)),
                          np.tile(np.array([[0], [0], [-1]], F), (1, n)), st, inc, 1, candidates=True)
    finally:
        po.rng_next_f32 = real
    assert Given.calls == 4
    e1, e2, off = _barycentric(t, np.zeros(n, int), out["cand_point"][0])
    np.testing.assert_allclose(np.stack([e1, e2], axis=1), want, atol=1e-6)
    assert (e1 + e2 <= 1 + 1e-6).all() and (np.abs((e1 + e2)[[1, 2, 3]] - 1) <= 1e-6).all() and (off <= 1e-5).all()


# ---- lights that can never be kept -------------------------------------------------------------------------------------------
def test_a_one_sided_light_seen_from_behind_is_never_kept_and_two_sided_it_is():
    n = 4096
    p = np.tile(np.array([[50], [50], [10]], F), (1, n))
    nrm = np.tile(np.array([[0], [0], [1]], F), (1, n))
    for two_sided in (False, True):
        # cross(a, b) = +z: the light above the vertex faces up, away from it
        lights = nm.prepare(nm.table([[40, 40, 30]], [[20, 0, 0]], [[0, 20, 0]], [3], [0], [two_sided]))
        assert lights["N"][0, 2] == 1
        st, inc = po.rng_seed(n, 41)
        out = nm.resample(_one_leaf(1), np.zeros(n, int), 0.1, lights, p, nrm, st, inc, 4, candidates=True)
        kept = out["index"] != nm.NONE
        if two_sided:
            assert kept.all() and (out["cand_target"] > 0).all()
        else:
            assert not kept.any() and (out["cand_target"] == 0).all() and (out["cand_source"] > 0).all() and (out["weight"] == 0).all()


def test_a_light_of_radiance_zero_is_never_kept():
    n = 4096
    p = np.tile(np.array([[50], [50], [10]], F), (1, n))
    nrm = np.tile(np.array([[0], [0], [1]], F), (1, n))
    t = nm.table([[40, 40, 30], [20, 20, 40]], [[0, 20, 0]] * 2, [[20, 0, 0]] * 2, [0, 2], [0, 0], [0, 0])
    st, inc = po.rng_seed(n, 43)
    out = nm.resample(_one_leaf(2, _row_of([65536, 100])), np.zeros(n, int), 0.1, nm.prepare(t), p, nrm, st, inc, 3, candidates=True)
    kept = out["index"] != nm.NONE
    assert (out["cand_light"] == 0).mean() > 0.9 and (out["light"][kept] == 1).all() and 10 < kept.sum() < n


# ---- unbiasedness, and two wrong weights rejected -----------------------------------------------------------------------------
# The scene: a vertex at VERTEX with the normal +z and eight lights around it.  cross(edge_a, edge_b) is a light's normal.
VERTEX, NORMAL = (50.0, 50.0, 10.0), (0.0, 0.0, 1.0)
SCENE = nm.table(
    origin=[[40, 40, 30], [62, 30, 18], [10, 10, 90], [60, 70, 80], [45, 60, 40], [35, 20, 25], [51, 47, 14], [90, 20, 0]],
    edge_a=[[0, 20, 0], [0, 0, 15], [30, 0, 0], [25, 0, 5], [10, 0, 0], [0, 15, 10], [0, 3, 0], [0, 0, 40]],
    edge_b=[[20, 0, 0], [6, 18, 0], [0, 30, 0], [0, 20, -5], [0, 10, 0], [30, 0, 0], [3, 0, 1], [0, 60, 0]],
    radiance=[5, 8, 20, 30, 50, 6, 40, 1.5],
    triangle=[0, 1, 0, 1, 0, 1, 0, 0],      # parallelograms and triangles
    two_sided=[0, 0, 1, 1, 0, 1, 0, 0])     # 0: near, faces down.  1: near, beside.  2, 3: far, two-sided.  4: above, FACES AWAY.
#                                             5: near, tilted, two-sided.  6: small, bright, near.  7: a wall that reaches below the horizon
X0 = 50.0                                   # the occluder: a point y is visible when y.x > X0 -- it cuts through lights 0, 4 and 5 and hides light 2
DELTA = 0.1
N_LANES = 1 << 16
SEED = 2024
ROWS = {
    # the row prefers the light that faces away and the one the occluder hides
    "wrong": _row_of([1000, 2000, 40000, 500, 65536, 1000, 300, 2000]),
    # about the lights' unshadowed contributions at the vertex
    "right": _row_of([65536, 9000, 5000, 7000, 0, 4000, 40000, 1500]),
    "unlearned": np.zeros(8, np.uint32),
}


def _integrand(light, y):
    """f(y) = radiance g(y) V(y) in float64, y (3, n) on lights `light`"""
    o, a, b = (SCENE[k].astype(np.float64) for k in ("origin", "edge_a", "edge_b"))
    N = np.cross(a, b)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    v = y - np.array(VERTEX)[:, None]
    d2 = (v * v).sum(0)
    w = v / np.sqrt(d2)
    cs = (np.array(NORMAL)[:, None] * w).sum(0)
    cl = -(N[light].T * w).sum(0)
    cl = np.where(SCENE["two_sided"][light], np.abs(cl), cl)
    g = np.where((cs > 0) & (cl > 0), cs * cl / d2, 0.0)
    return SCENE["radiance"].astype(np.float64)[light] * g * (y[0] > X0)


@functools.lru_cache(maxsize=None)
def _truth(res=2048):
    """float64 midpoint quadrature over every light's parameter square, res x res cells; a triangle over its own half by
    e1 = s, e2 = t (1 - s), whose Jacobian is 1 - s.  No sampling code."""
    o, a, b = (SCENE[k].astype(np.float64) for k in ("origin", "edge_a", "edge_b"))
    area2 = np.linalg.norm(np.cross(a, b), axis=1)
    mid = (np.arange(res) + 0.5) / res
    s, t = [g.ravel() for g in np.meshgrid(mid, mid, indexing="ij")]
    total = 0.0
    for j in range(8):
        e1, e2, jac = (s, t * (1 - s), 1 - s) if SCENE["triangle"][j] else (s, t, np.ones_like(s))
        y = o[j][:, None] + e1 * a[j][:, None] + e2 * b[j][:, None]
        total += float((_integrand(np.full(s.shape[0], j), y) * jac).sum()) * area2[j] / (res * res)
    return total


@functools.lru_cache(maxsize=None)
def _launch(row, M, weight=nm.weight_of_the_header):
    p = np.tile(np.array(VERTEX, F)[:, None], (1, N_LANES))
    nrm = np.tile(np.array(NORMAL, F)[:, None], (1, N_LANES))
    st, inc = po.rng_seed(N_LANES, SEED)
    return nm.resample(ROWS[row].reshape(1, 8), np.zeros(N_LANES, int), DELTA, nm.prepare(SCENE), p, nrm, st, inc, M, weight=weight)


def _estimates(row, M, weight=nm.weight_of_the_header):
    """f(y) W of every lane, float64"""
    out = _launch(row, M, weight)
    kept = out["index"] != nm.NONE
    f = np.zeros(N_LANES)
    f[kept] = _integrand(out["light"][kept].astype(np.int64), out["point"][:, kept].astype(np.float64))
    return f * out["weight"].astype(np.float64)


def _check_unbiased(row, M, weight):
    """raises AssertionError unless the mean is the quadrature's within five standard errors"""
    truth = _truth()
    est = _estimates(row, M, weight)
    mean, se = est.mean(), est.std(ddof=1) / np.sqrt(est.shape[0])
    print("row %-9s M = %2d  %-28s mean %.6f  truth %.6f  standard error %.6f  (%.2f of them off)"
          % (row, M, weight.__name__, mean, truth, se, abs(mean - truth) / se))
    assert abs(mean - truth) <= 5 * se, (row, M, weight.__name__, mean, truth, se)


def test_the_scene_is_what_it_says():
    r = nm.prepare(SCENE)
    assert (r["invA"] > 0).all() and r["N"][4, 2] > 0 and r["N"][0, 2] < 0
    lo = SCENE["origin"][:, 0] + np.minimum(SCENE["edge_a"][:, 0], 0) + np.minimum(SCENE["edge_b"][:, 0], 0)
    hi = SCENE["origin"][:, 0] + np.maximum(SCENE["edge_a"][:, 0], 0) + np.maximum(SCENE["edge_b"][:, 0], 0)
    cut = (lo < X0) & (hi > X0)
    assert cut.sum() >= 2 and cut[0] and cut[5] and hi[2] < X0           # the occluder cuts through lights and hides one
    # every light but the averted one contributes where it is visible, and the wall reaches below the horizon
    out = _launch("unlearned", 1)
    kept = out["index"] != nm.NONE
    assert set(np.unique(out["light"][kept])) == {0, 1, 2, 3, 5, 6, 7}
    assert SCENE["origin"][7, 2] < VERTEX[2]


def test_the_quadrature_is_converged():
    fine, coarse = _truth(), _truth(1024)
    se = min(_estimates(row, M).std(ddof=1) / np.sqrt(N_LANES) for row in ROWS for M in (1, 4, 16))
    print("2048^2 %.8f, 1024^2 %.8f, apart by %.4f of the smallest standard error %.6f" % (fine, coarse, abs(fine - coarse) / se, se))
    assert abs(fine - coarse) < se / 5


@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("row", list(ROWS))
def test_the_estimator_is_unbiased(row, M):
    _check_unbiased(row, M, nm.weight_of_the_header)


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("row", list(ROWS))
@pytest.mark.parametrize("wrong", [nm.weight_without_one_over_m, nm.weight_one_over_source], ids=lambda f: f.__name__)
def test_a_wrong_weight_is_rejected(wrong, row, M):
    with pytest.raises(AssertionError):
        _check_unbiased(row, M, wrong)


def variance_table():
    lines = ["# tests/test_nee_model.py: the estimator f(y) * W of the direct light at the vertex of the scene written out there (eight",
             "# lights, the occluder y.x > 50), the lights' delta 0.1, 2^16 lanes of the float32 model (seed %d); truth %.6f" % (SEED, _truth()),
             "# M = 1 is the method a host uses today: lightsSample plus a uniform point on the light",
             "# row | M | mean | sample variance | variance / variance at M = 1"]
    for row in ROWS:
        v1 = _estimates(row, 1).var(ddof=1)
        for M in (1, 4, 16):
            est = _estimates(row, M)
            lines.append("%s | %d | %.6f | %.6f | %.4f" % (row, M, est.mean(), est.var(ddof=1), est.var(ddof=1) / v1))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nee", "variance.txt")
    with open(path, "w") as fh:
        fh.write(variance_table())
    print(open(path).read())
