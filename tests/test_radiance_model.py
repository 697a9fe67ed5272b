"""The model of include/pgsd_radiance.h (tests/radiance_model.py) on the CPU oracle: what the estimate means (a constant field is
recovered), which weights a refine has to carry, and that the decision is unbiased.  No GPU; tests/test_gpu_radiance.py compares
the device with this model bit for bit."""
import numpy as np
import pytest

import radiance_model as rm
import synth
from oracle import pg_oracle as po

F = np.float32
BB0, BB1 = [0.0] * 3, [100.0] * 3
U = 2.0 ** -24


def _constant_records(m, seed, c):
    """Records of radiance c whose directions were drawn uniformly over the sphere: wo_pdf = 1 / (4 pi); no emitter deposit.
    Positions towards one corner of the box, so that KD leaves split unevenly."""
    return rm.corner_records(m, seed, BB0, BB1, radiance=c)


def _iterate(pair, k, rec):
    """One training iteration of the oracle pair; returns (columns before, KD record counts before, columns after)."""
    synth.splat(pair.current, rec)
    old_cols, count = pair.current.export(), pair.current.kd_column("count")
    pair.refine_and_prepare(k)
    return old_cols, count, pair.prev.export()


@pytest.fixture(scope="module")
def constant_field():
    """Two iterations (the second one's tree has quadtrees several levels deep and KD leaves of different ages); computed once."""
    pair = po.OracleSDTreePair()
    pair.setup(BB0, BB1, 20, 20, True)
    c = F(0.75)
    _iterate(pair, 0, _constant_records(1 << 15, 900, c))
    old_cols, count, cols = _iterate(pair, 1, _constant_records(1 << 17, 910, c))
    return c, cols, rm.carried_weights(old_cols, count, cols), old_cols, count


def test_a_constant_field_is_recovered(constant_field):
    """L_mean = ((S * INV_FOUR_PI) / Nf with S the fp32 of an exact sum of N deposits c / wo_pdf: three roundings after the sum,
    the rounding of the deposit itself and of the two constants, each <= 2^-24 relative -- 8 * 2^-24 bounds them; the 2^-40
    truncation of a deposit of 9.4 is 1e-13 relative."""
    c, cols, w, _, _ = constant_field
    m = rm.RadianceModel(cols, w)
    assert (w > 0).all() and cols["kdtree_isLeaf"].sum() >= 4 and cols["quadtree_depth"].max() >= 2
    p = synth.positions_uniform(4096, 77, BB0, BB1)
    d = synth.directions_uniform(4096, 78)
    L_dir, L_mean = m.estimate(p, d)
    assert L_mean.dtype == F and L_dir.dtype == F
    assert (np.abs(L_mean.astype(np.float64) - float(c)) <= 8 * U * float(c)).all()
    # every quadtree was visited
    assert np.unique(m.tree_of(p)).shape[0] == w.shape[0]
    # the directional estimate is the same constant up to the noise of the records in one leaf (thousands per leaf here)
    assert np.abs(np.median(L_dir) / float(c) - 1) < 0.05


def _leaves_of(m, t):
    """(node, depth) of every leaf of quadtree t."""
    out, stack = [], [(int(m.root[t]), 0)]
    while stack:
        n, d = stack.pop()
        if m.q_leaf[n]:
            out.append((n, d))
        else:
            stack += [(int(m.q_ch[k, n]), d + 1) for k in range(4)]
    return out


def test_the_leaves_of_a_quadtree_integrate_to_its_mean(constant_field):
    """sum over the leaves of L_dir * 4^-d against L_mean.  In exact arithmetic the two differ because every leaf's energy and
    the root's are separate fp32 roundings of exact sums: the float64 model on the same columns gives that difference, D.
    The float32 model adds two roundings per leaf term (e * 4^d is exact), each at most half an ulp of a term that is no
    larger than the sum: at most one ulp of L_mean per leaf summed.  Bound: |D| + n_leaves * ulp(L_mean)."""
    _, cols, w, _, _ = constant_field
    m32, m64 = rm.RadianceModel(cols, w), rm.RadianceModel(cols, w, np.float64)
    checked = 0
    for t in range(w.shape[0]):
        lv = _leaves_of(m32, t)
        nodes = np.array([n for n, _ in lv])
        depth = np.array([d for _, d in lv])
        sums = []
        for m in (m32, m64):
            T = m.T
            Nf = w[t].astype(F).astype(T) if T is F else T(w[t])
            k = T(F(rm.INV_FOUR_PI))
            L_dir = (((m.q_irr[nodes].astype(T) * np.ldexp(T(1), 2 * depth).astype(T)).astype(T) * k).astype(T) / Nf).astype(T)
            L_mean = T(T(m.q_irr[m.root[t]].astype(T) * k) / Nf)
            sums.append((np.sum(L_dir.astype(np.float64) * np.ldexp(1.0, -2 * depth)), float(L_mean)))
        (s32, mean32), (s64, mean64) = sums
        bound = abs(s64 - mean64) + len(lv) * float(np.spacing(F(mean32)))
        assert abs(s32 - mean32) <= bound, (t, s32, mean32, bound)
        checked += len(lv) > 1
    assert checked >= 4


def test_kd_descent_and_leaf_choice_are_the_oracles(constant_field):
    """The two walks of the model against the oracle: the KD node, positions outside, on faces and NaN included; and the leaf
    that a record adds to -- a single record into empty accumulators marks it -- for directions on cell edges and corners."""
    _, cols, w, _, _ = constant_field
    m = rm.RadianceModel(cols, w)
    o = po.OracleTree()
    o.load(cols)
    p = synth.positions_uniform(20000, 5, BB0, BB1)
    p[:, 0] = [-1.0, 50.0, 50.0]; p[:, 1] = [0.0, 0.0, 0.0]; p[:, 2] = [100.0, 100.0, 100.0]; p[:, 3] = [50.0, 50.0, 50.0]
    p[:, 4] = [25.0, 75.0, 12.5]; p[:, 5] = [np.nan, 1.0, 1.0]; p[:, 6] = [100.00001, 1.0, 1.0]
    act = (synth.uniform(20000, 6)[0] < 0.8).astype(np.uint8)
    np.testing.assert_array_equal(m.kd_node(p).astype(np.uint32), o.get_leaf_node_index(p))
    np.testing.assert_array_equal(m.kd_node(p, act).astype(np.uint32), o.get_leaf_node_index(p, act))
    dirs = [(0.5, 0.5), (0.25, 0.5), (0.5, 0.25), (1.0, 1.0), (0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.75, 0.75), (0.125, 0.875),
            (0.3, 0.5), (0.5, 0.7), (0.3, 0.7), (0.625, 0.375), (0.015625, 0.5)]
    pos = np.array([[30.0], [40.0], [50.0]], F)
    t = m.tree_of(pos)
    for cx, cy in dirs:
        o.reset()
        o.add_data_propagate(pos, np.array([[cx], [cy]], F), np.ones(1, F), np.ones(1, F), np.array([[cx], [cy]], F), np.zeros(1, F))
        lo = o.quad_column("acc_lo")
        marked = np.nonzero((lo != 0) & m.q_leaf)[0]
        e, d, node = m.leaf(t, np.array([cx], F), np.array([cy], F))
        assert marked.tolist() == [int(node[0])], (cx, cy, marked, node)
        assert d[0] == cols["quadtree_depth"][node[0]]


def test_grid_directions_lie_on_the_cell_edges():
    """The directions the GPU test takes for cell edges and corners: every one maps onto an exact multiple of 2^-7 in both
    coordinates, every multiple occurs in y, and most in x (the axes among them)."""
    d = rm.grid_directions(7)
    c = po.dir_to_canonical(d).astype(np.float64) * 128
    assert (c == np.round(c)).all() and c.min() == 0 and c.max() == 128
    assert np.unique(c[1]).shape[0] == 129 and np.unique(c[0]).shape[0] >= 96
    for k in range(1, 8):   # every level's edges: odd multiples of 2^-k, in x, in y, and at corners
        odd = lambda v: (v % (1 << (7 - k)) == 0) & ((v / (1 << (7 - k))) % 2 == 1)   # noqa: E731
        assert odd(c[0]).any() and odd(c[1]).any() and (odd(c[0]) & odd(c[1])).any(), k


def test_weights_after_a_refine_are_the_parents(constant_field):
    """A KD leaf that splits hands every child a copy of its quadtree WITH the energy of all N records: the children's estimates
    divide by the parent's N, whatever number of splits lies between them, while vertCount halves per split."""
    c, cols, w, old_cols, count = constant_field
    splits = rm.splits_between(old_cols, cols)
    assert splits.max() >= 2 and splits.min() == 0, np.bincount(splits)
    leaf = np.nonzero(cols["kdtree_isLeaf"])[0]
    tree = cols["kdtree_quadTreeRootIndex"][leaf]
    vc = np.asarray(cols["kdtree_vertCount"], F)[leaf]
    assert (w[tree] < (1 << 24)).all()
    np.testing.assert_array_equal(np.ldexp(vc, splits[tree].astype(np.int32)), w[tree].astype(F))
    # the weights are the old leaves' counts: together the old leaves hold every record of the iteration
    old_leaf = np.asarray(old_cols["kdtree_isLeaf"], bool)
    assert set(w.tolist()) <= set(np.asarray(count)[old_leaf].tolist()) and int(np.asarray(count)[old_leaf].sum()) == 1 << 17
    # with the child's own count in N's place the estimate would be 2^splits too large
    m = rm.RadianceModel(cols, w)
    wrong = rm.RadianceModel(cols, np.ldexp(vc, 0).astype(np.uint64)[np.argsort(tree)])
    centre = ((np.asarray(cols["kdtree_bbox_min"], F).reshape(-1, 3)[leaf] + np.asarray(cols["kdtree_bbox_max"], F).reshape(-1, 3)[leaf]) / 2).T.astype(F)
    np.testing.assert_array_equal(m.tree_of(centre), tree)
    _, L_mean = m.estimate(centre)
    _, L_wrong = wrong.estimate(centre)
    assert (np.abs(L_mean.astype(np.float64) - float(c)) <= 8 * U * float(c)).all()
    twice = splits[tree] >= 2
    assert (L_wrong[twice] > 3.9 * float(c)).all()


def _mean_and_bound(count, scale, variance):
    y = count.astype(np.float64) * scale.astype(np.float64)
    return abs(y.mean() - 1.0), 5.0 * np.sqrt(variance / y.shape[0])


def test_the_decision_is_unbiased():
    """2^20 stream draws at a fixed q.  Roulette: count * scale is lo / q with probability P = q / lo, else 0: variance
    (1 - P) / P.  Split: (floor(r) + Bernoulli(f)) / r with f = r - floor(r): variance f (1 - f) / r^2."""
    n = 1 << 20
    xi = synth.uniform(n, 4242)[0]
    one = np.ones(n, F)
    lo, hi = rm.rr_window(5.0)
    assert lo == F(F(2) / F(6)) and hi == F(F(5) * lo)
    for P in (0.1, 0.15, 0.5, 0.9):
        q = F(P) * lo
        count, scale = rm.decide(np.full(n, q, F), one, one, xi, 5.0, 8)
        assert set(np.unique(count).tolist()) == {0, 1} and (scale[count == 0] == 0).all() and (scale[count == 1] == F(lo / q)).all()
        err, bound = _mean_and_bound(count, scale, (1 - P) / P)
        assert err < bound, (P, err, bound)
    for r in (1.25, 2.3, 7.5):
        q = F(r) * hi
        count, scale = rm.decide(np.full(n, q, F), one, one, xi, 5.0, 8)
        assert set(np.unique(count).tolist()) == {int(r), int(r) + 1}
        f = r - int(r)
        err, bound = _mean_and_bound(count, scale, f * (1 - f) / r ** 2)
        assert err < bound, (r, err, bound)
    # the clamp: above max_split the path is split max_split times exactly, and scale = 1 / max_split (no longer unbiased: the
    # host chose the bound)
    count, scale = rm.decide(np.full(n, F(100) * hi, F), one, one, xi, 5.0, 8)
    assert (count == 8).all() and (scale == F(0.125)).all()


def test_the_cases_without_an_opinion():
    xi = synth.uniform(64, 7)[0]
    one = np.ones(64, F)
    small = np.full(64, 1e-3, F)
    big = np.full(64, 1e3, F)
    for bad in (0.0, -1.0, -0.0, np.inf, -np.inf, np.nan):
        b = np.full(64, bad, F)
        for args in ((b, one, small), (small, b, one), (small, one, b), (b, one, big), (big, b, one)):
            count, scale = rm.decide(*args, xi, 5.0, 8)
            assert (count == 1).all() and (scale == 1).all(), (bad,)
    # q overflows
    count, scale = rm.decide(np.full(64, 3e38, F), np.full(64, 3e38, F), one, xi, 5.0, 8)
    assert (count == 1).all() and (scale == 1).all()
    # max_split = 1: no splitting, the roulette stays
    count, scale = rm.decide(big, one, one, xi, 5.0, 1)
    assert (count == 1).all() and (scale == 1).all()
    count, scale = rm.decide(small, one, one, xi, 5.0, 1)
    assert (count == 0).any()
    # window = 1: lo = hi = 1, only q == 1 has no opinion
    assert rm.rr_window(1.0) == (F(1), F(1))
    count, scale = rm.decide(one, one, one, xi, 1.0, 8)
    assert (count == 1).all() and (scale == 1).all()
    count, scale = rm.decide(np.full(64, 2.5, F), one, one, xi, 1.0, 8)
    assert set(np.unique(count).tolist()) <= {2, 3} and (scale == F(1 / F(2.5))).all()
    # inside the window
    for q in (0.34, 1.0, 1.66):
        count, scale = rm.decide(np.full(64, q, F), one, one, xi, 5.0, 8)
        assert (count == 1).all() and (scale == 1).all()


def test_one_draw_per_active_lane(constant_field):
    _, cols, w, _, _ = constant_field
    m = rm.RadianceModel(cols, w)
    n = 1000
    p = synth.positions_uniform(n, 3, BB0, BB1)
    d = synth.directions_uniform(n, 4)
    act = (synth.uniform(n, 5)[0] < 0.7).astype(np.uint8)
    st, inc = po.rng_seed(n, 9)
    st0 = st.copy()
    ref, _ = po.rng_seed(n, 9)
    po.rng_next_f32(ref, inc)
    count, scale, L = m.roulette(p, d, np.full(n, 0.01, F), np.ones(n, F), st, inc, 5.0, 4, act)
    np.testing.assert_array_equal(st, np.where(act != 0, ref, st0))
    assert (count[act == 0] == 1).all() and (scale[act == 0] == 1).all() and (L[act == 0] == 0).all()
    assert (count[act != 0] == 0).any() and (count[act != 0] == 1).any()
