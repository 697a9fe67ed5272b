"""tests/bounce_model.py by itself (no GPU): the selection rule, the draws of the drawn form, and the conditions on the inputs
that tests/test_gpu_bounce.py shares -- asserted here on the model alone, so that a device test cannot pass by leaving a branch
empty."""
import numpy as np
import pytest

import bounce_model as bm
import fraction_model as fm
import radiance_model as rm
import synth
from oracle import pg_oracle as po
from test_gpu_parity import BB0, BB1
from test_gpu_radiance import WEIGHTS, make_inputs
from test_gpu_target import _mixed_roots

F = np.float32


def test_the_selection_rule():
    f = np.array([0.0, 0.25, 0.5, 0.99999994, 1.0, 1.1920929e-07], F)
    below, above = np.nextafter(f, F(-1)), np.nextafter(f, F(2))
    ch = np.full(f.shape[0], bm.CHOOSE, np.uint8)
    np.testing.assert_array_equal(bm.select(ch, f, f), 1)                      # xi == f selects 1 (the reference's `>`)
    np.testing.assert_array_equal(bm.select(ch, below, f), 1)
    np.testing.assert_array_equal(bm.select(ch, above, f), 2)
    np.testing.assert_array_equal(bm.select(ch, np.full_like(f, np.nan), f), 1)  # a NaN xi selects 1
    np.testing.assert_array_equal(bm.select(ch, f, np.full_like(f, np.nan)), 1)
    # forced modes ignore xi; bytes > 3 are NONE
    md = np.array([0, 1, 2, 3, 4, 255], np.uint8)
    np.testing.assert_array_equal(bm.select(md, np.ones(6, F), np.zeros(6, F)), [0, 1, 2, 2, 0, 0])
    np.testing.assert_array_equal(bm.select(md, np.zeros(6, F), np.ones(6, F)), [0, 1, 2, 1, 0, 0])


@pytest.fixture(scope="module")
def trees():
    """cols of the four topologies of tests/test_gpu_radiance.py (the mixed-roots tree in the oracle's node order here, in the
    device's there), computed once, never written to."""
    init = po.OracleTree()
    init.setup(BB0, BB1, 20, 20, True)
    e = init.export()
    e["kdtree_maxLeafSize"] = np.float64(1.0)
    e["quadtree_irradiance"] = np.array([3.5], F)
    mx = _mixed_roots().export()
    mx["quadtree_irradiance"] = (F(1) - synth.uniform(mx["quadtree_depth"].shape[0], 31)[0]).astype(F)
    return {"initial": e, "balanced": synth.build_balanced(3, 5).export(), "skewed": synth.build_skewed(1 << 14, 4).prev.export(),
            "mixed roots": mx}


@pytest.fixture(scope="module")
def inputs():
    return bm.make_inputs(make_inputs())


def _model(cols, learned=True, radiance=True):
    tree = po.OracleTree()
    tree.load(cols)
    n_trees = cols["quadtree_rootNodeIndex"].shape[0]
    frac = None
    if learned:
        frac = fm.FractionModel(tree, theta0=bm.THETA0)
        frac.load_state(bm.fraction_state(n_trees))
    w = WEIGHTS[np.arange(n_trees) % WEIGHTS.shape[0]] if radiance else None
    return bm.BounceModel(tree, frac, 0.5, w, cols=cols)


@pytest.mark.parametrize("which", ["initial", "balanced", "skewed", "mixed roots"])
def test_the_shared_inputs_reach_every_branch(trees, inputs, which):
    m = _model(trees[which])
    res = m.bounce(inputs["p"], inputs["dir_nee"], inputs["nee_active"], inputs["dir_io"], inputs["mode"], inputs["u_select"],
                   u=inputs["u"])
    bm.check_conditions(which, inputs, res, ~m.fraction.inside(inputs["p"]))
    th = m.fraction.theta
    assert th.min() == F(-20) or th.shape[0] == 1
    assert th.max() == F(20) or th.shape[0] == 1
    # the non-live lanes: what pg_fraction_query gives an inactive lane, and nothing else
    off = ~res["live"]
    assert off.sum() > 100
    np.testing.assert_array_equal(res["fraction"][off].view(np.uint32), fm.logistic(bm.THETA0).view(np.uint32)[0])
    assert (res["select"][off] == 0).all() and (res["pdf"][off] == 1).all() and (res["pdf_nee"][off] == 1).all()
    assert (res["L_dir"][off] == 0).all() and (res["L_mean"][off] == 0).all()
    np.testing.assert_array_equal(res["dir"][:, res["select"] != 2].view(np.uint32), inputs["dir_io"][:, res["select"] != 2].view(np.uint32))
    # lanes with sel == 0 that are live (an emitter sample only) have a pdf_nee and no estimate
    only_nee = res["live"] & (res["select"] == 0)
    assert only_nee.sum() > 100 and (res["L_dir"][only_nee] == 0).all() and (res["pdf_nee"][only_nee] != 1).any()
    # the ties: f itself and its predecessor select 1, its successor 2
    u_t = bm.with_ties(inputs["u_select"], res["fraction"])
    sel_t = m.bounce(inputs["p"], inputs["dir_nee"], inputs["nee_active"], inputs["dir_io"], inputs["mode"], u_t, u=inputs["u"])["select"]
    k = np.arange(bm.TIES0, bm.TIES0 + 3 * bm.TIES)
    expect = np.tile(np.array([1, 1, 2], np.uint8), bm.TIES)
    np.testing.assert_array_equal(sel_t[k], expect)


def test_the_drawn_form_consumes_one_draw_per_choose_lane(trees, inputs):
    m = _model(trees["balanced"])
    n = bm.N
    st0, inc = po.rng_seed(n, 41)
    st = st0.copy()
    res = m.bounce(inputs["p"], inputs["dir_nee"], inputs["nee_active"], inputs["dir_io"], inputs["mode"], None, st, inc)
    md = m.modes(n, inputs["mode"])
    ch = md == bm.CHOOSE
    one = st0.copy()
    xi = po.rng_next_f32(one, inc)                       # every stream advanced by exactly one draw
    np.testing.assert_array_equal(res["select"], bm.select(md, xi, res["fraction"]))
    sel = res["select"]
    quiet = ~ch & (sel != 2)
    np.testing.assert_array_equal(st[quiet], st0[quiet])                       # no CHOOSE, no sample: untouched
    np.testing.assert_array_equal(st[ch & (sel == 1)], one[ch & (sel == 1)])  # chose the pdf: the one draw
    # a lane that samples goes on from where it stands: a CHOOSE lane behind its draw, a forced one from the start
    start = np.where(ch, one, st0)
    d, pdf = m.tree.sample(inputs["p"], start, inc, (sel == 2).astype(np.uint8))
    np.testing.assert_array_equal(st[sel == 2], start[sel == 2])
    assert (st[sel == 2] != one[sel == 2]).all()
    np.testing.assert_array_equal(res["dir"][:, sel == 2].view(np.uint32), d[:, sel == 2].view(np.uint32))
    np.testing.assert_array_equal(res["pdf"][sel == 2].view(np.uint32), pdf[sel == 2].view(np.uint32))
    assert (ch & (sel == 1)).sum() > 1000 and (ch & (sel == 2)).sum() > 1000 and (~ch & (sel == 2)).sum() > 1000


def test_without_the_learned_fraction_f_is_the_constant(trees, inputs):
    for c in (0.5, 0.3):
        tree = po.OracleTree()
        tree.load(trees["balanced"])
        m = bm.BounceModel(tree, None, c, None)
        res = m.bounce(inputs["p"], inputs["dir_nee"], inputs["nee_active"], inputs["dir_io"], inputs["mode"], inputs["u_select"], u=inputs["u"])
        assert (res["fraction"] == F(c)).all() and res["L_dir"] is None
        ch = m.modes(bm.N, inputs["mode"]) == bm.CHOOSE
        with np.errstate(invalid="ignore"):
            np.testing.assert_array_equal(res["select"][ch], np.where(inputs["u_select"][ch] > F(c), 2, 1))


def test_the_estimate_is_of_the_direction_behind_the_bounce(trees, inputs):
    """A sampled lane's estimate is radiance_model's for the direction just written, a pdf lane's for dir_io."""
    cols = trees["balanced"]
    m = _model(cols)
    res = m.bounce(inputs["p"], inputs["dir_nee"], inputs["nee_active"], inputs["dir_io"], inputs["mode"], inputs["u_select"], u=inputs["u"])
    r = rm.RadianceModel(cols, m.rad.w)
    L_new, _ = r.estimate(inputs["p"], res["dir"])
    L_old, _ = r.estimate(inputs["p"], inputs["dir_io"])
    s2, s1 = res["select"] == 2, res["select"] == 1
    np.testing.assert_array_equal(res["L_dir"][s2].view(np.uint32), L_new[s2].view(np.uint32))
    np.testing.assert_array_equal(res["L_dir"][s1].view(np.uint32), L_old[s1].view(np.uint32))
    assert (L_new[s2] != L_old[s2]).any()
