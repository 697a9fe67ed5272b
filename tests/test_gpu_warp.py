"""Sample warping on the device (pg_sample_warp, pg_invert_warp, pg_guide_bounce_warp; include/pgsd_warp.h) against the numpy
model of the header (tests/warp_model.py): every lane, the bit patterns of dir, pdf and u.  n = 2^14 + 77 lanes, so the last
workgroup is partial."""

import numpy as np
import pytest

import synth
from oracle import pg_oracle as po
from test_gpu_kd_grid_faces import face_positions
from test_gpu_parity import BB0, BB1, dev, gpu_tree_from
from warp_model import WarpModel, with_dead_quadtree

pytestmark = pytest.mark.gpu

N = (1 << 14) + 77
ONE_M = np.float32(1) - np.float32(2.0 ** -24)
SPECIAL0 = 100                      # first lane of the special values of u (face_positions keeps the lanes below 16)
INTERIOR = (30.0, 40.0, 50.0)       # their position


@pytest.fixture(autouse=True)
def _synchronise_behind_every_call():
    """A GPU fault then names the call that launched the faulting kernel."""
    from practical_path_guiding_lab_amd import sdtree
    sdtree.SYNC_EVERY_CALL = True
    yield
    sdtree.SYNC_EVERY_CALL = False


TREES = ["initial", "balanced", "skewed", "dead", "skewed, no jump tables"]


@pytest.fixture(scope="module")
def oracle_trees():
    init = po.OracleTree()
    init.setup(BB0, BB1, 20, 20, True)
    bal = synth.build_balanced(3, 4)
    skew = synth.build_skewed(4096, 4).prev      # deep quadtrees, leaves without energy
    trees = {"initial": init, "balanced": bal, "skewed": skew, "dead": with_dead_quadtree(bal, 0), "skewed, no jump tables": skew}
    return {k: (t, WarpModel(t)) for k, t in trees.items()}


def _gpu_tree(which, tree, monkeypatch):
    from practical_path_guiding_lab_amd.sdtree import SDTree
    if which == "initial":
        g = SDTree()
        g.setup(BB0, BB1, 0, 0, 20, 20, True, 0.5)
        return g
    if which.endswith("no jump tables"):   # (the way test_jump_tables_follow_their_memory_budget switches them off)
        monkeypatch.setenv("PGSD_JUMP_TABLE_MAX_BYTES", "8")   # (less than one tree's smallest table)
    else:
        monkeypatch.delenv("PGSD_JUMP_TABLE_MAX_BYTES", raising=False)
    g = gpu_tree_from(tree)
    assert (g.stats().jump_bits == 0) == which.endswith("no jump tables")
    return g


def _ulp(v, up):
    return np.nextafter(np.float32(v), np.float32(2.0 if up else -1.0))


def warp_inputs(model, seed):
    """Positions on faces, outside and NaN (tests/test_gpu_kd_grid_faces.py); u random, and from lane SPECIAL0 on every pair of:
    the edges 0, 2^-24, ONE_M; out of range -0.5, 1.0, 2.0, +inf, NaN; the thresholds Py and Pl (both rows) of the root of
    INTERIOR's quadtree and one ulp either side, taken from the model."""
    p = face_positions(N, seed)
    u = synth.uniform(N, seed + 1, 2)
    vals = [0.0, 2.0 ** -24, ONE_M, -0.5, 1.0, 2.0, np.inf, np.nan]
    root = model.root_of(np.array(INTERIOR, np.float32).reshape(3, 1))[0]
    if not model.leaf[root]:
        for thr in model.root_thresholds(root):
            vals += [_ulp(thr, False), thr, _ulp(thr, True)]
    vals = np.array(vals, np.float32)
    k = vals.shape[0] ** 2
    p[:, SPECIAL0:SPECIAL0 + k] = np.array(INTERIOR, np.float32)[:, None]
    u[0, SPECIAL0:SPECIAL0 + k] = np.tile(vals, vals.shape[0])
    u[1, SPECIAL0:SPECIAL0 + k] = np.repeat(vals, vals.shape[0])
    active = (synth.uniform(N, seed + 2)[0] < 0.85).astype(np.uint8)
    active[SPECIAL0:SPECIAL0 + k] = 1
    return p, u, active


def invert_directions(d_warp, seed):
    """The warp's own outputs (first third), uniform directions, and at the head the poles and non-finite ones."""
    d = synth.directions_uniform(N, seed)
    d[:, :N // 3] = d_warp[:, :N // 3]
    head = [(0, 0, 1), (0, 0, -1), (0.0, -0.0, 1.0), (np.nan, 0, 0), (0, np.inf, 0), (0.5, 0.5, -np.inf), (1, 0, 0), (0, 1, 0),
            (-1, 0, 0), (0, -1, 0), (1e-30, -1e-30, 0.5), (3.0, 4.0, 12.0)]
    d[:, 16:16 + len(head)] = np.array(head, np.float32).T
    return d


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


@pytest.mark.parametrize("which", TREES)
def test_warp_and_inverse_equal_the_model(oracle_trees, which, monkeypatch):
    import torch
    tree, model = oracle_trees[which]
    g = _gpu_tree(which, tree, monkeypatch)
    p, u, active = warp_inputs(model, 60)
    dp, du, dact = dev(torch, p), dev(torch, u), dev(torch, active)
    # the warp, with a mask with holes and without a mask
    for act, dact_ in ((active, dact), (None, None)):
        d_m, pdf_m = model.sample_warp(p, u, act)
        d_g, pdf_g = g.sampleWarp(dp, du, dact_)
        np.testing.assert_array_equal(bits(d_g), bits(d_m))
        np.testing.assert_array_equal(bits(pdf_g), bits(pdf_m))
    np.testing.assert_array_equal(bits(pdf_g), bits(g.pdf(dp, d_g)))     # the contract: pdf_out IS pg_pdf of (p, dir)
    assert np.isfinite(d_m).all() and np.isfinite(pdf_m).all()
    if which in ("skewed", "dead"):
        assert (pdf_m == 0).any() == (which == "dead")   # a leaf without energy is never chosen; a tree without energy has only such
    # the inverse
    d = invert_directions(d_m, 64)
    dd = dev(torch, d)
    for act, dact_ in ((active, dact), (None, None)):
        u_m, pdf_m = model.invert_warp(p, d, act)
        u_g, pdf_g = g.invertWarp(dp, dd, dact_)
        np.testing.assert_array_equal(bits(u_g), bits(u_m))
        np.testing.assert_array_equal(bits(pdf_g), bits(pdf_m))
    assert (u_m >= 0).all() and (u_m <= ONE_M).all()
    assert (pdf_m == 0).any() == (which in ("skewed", "dead", "skewed, no jump tables"))   # directions of zero probability
    # pdf_out may be NULL
    u_n = torch.full((2, N), -7.0, device="cuda")
    g._ck(g._lib.pg_invert_warp(g._h, N, dp.data_ptr(), dd.data_ptr(), None, u_n.data_ptr(), None,
                                torch.cuda.current_stream().cuda_stream))
    np.testing.assert_array_equal(bits(u_n), bits(u_m))
    # a NULL required pointer
    assert g._lib.pg_sample_warp(g._h, N, dp.data_ptr(), None, None, d_g.data_ptr(), pdf_g.data_ptr(), None) == -1
    assert g._lib.pg_invert_warp(g._h, N, dp.data_ptr(), dd.data_ptr(), None, None, None, None) == -1
    # no lanes: nothing is launched, nothing is written
    g._ck(g._lib.pg_sample_warp(g._h, 0, None, None, None, None, None, None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("which", ["balanced", "skewed", "dead"])
def test_guide_bounce_warp(oracle_trees, which, monkeypatch):
    """The three lane classes mixed, with and without pg_compact_lanes' list: the select == 2 lanes against the model, every
    other output against pg_guide_bounce on the same inputs; the PCG32 state of a sampler created beside the call is unchanged."""
    import torch
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    tree, model = oracle_trees[which]
    g = _gpu_tree(which, tree, monkeypatch)
    p, u, _ = warp_inputs(model, 70)
    d_nee, d_bsdf = synth.directions_uniform(N, 73), synth.directions_uniform(N, 74)
    r = synth.uniform(N, 75, 2)
    sel = np.where(r[1] < 0.3, 0, np.where(r[1] < 0.6, 1, 2)).astype(np.uint8)
    sel[SPECIAL0:SPECIAL0 + 289] = 2
    nee = (r[0] < 0.8).astype(np.uint8)
    dp, du, dsel, dnee, dd_nee = dev(torch, p), dev(torch, u), dev(torch, sel), dev(torch, nee), dev(torch, d_nee)
    smp = PCG32Sampler(g, N, seed=76)
    state0 = smp.state.cpu().numpy().copy()
    d_m, pdf_m = model.sample_warp(p, u, (sel == 2).astype(np.uint8))
    dio_ref = dev(torch, d_bsdf)
    pn_ref, po_ref = g.guideBounce(dp, dd_nee, dnee, dsel, dio_ref, PCG32Sampler(g, N, seed=77))
    pn_ref, po_ref = pn_ref.cpu().numpy(), po_ref.cpu().numpy()
    exp_dir = np.where(sel == 2, d_m, d_bsdf).astype(np.float32)
    exp_pdf = np.where(sel == 2, pdf_m, po_ref).astype(np.float32)
    idx, cnt = g.compactLanes(dsel, dnee)
    live = (sel != 0) | (nee != 0)
    assert not live.all()
    for lanes in (None, (idx, cnt)):
        dio = dev(torch, d_bsdf)
        sent = torch.full((N,), -7.0, device="cuda")
        pn, pw = g.guideBounceWarp(dp, dd_nee, dnee, dsel, dio, du, sent.clone(), sent.clone(),
                                   *(lanes if lanes else (None, None)))
        touched = live if lanes else np.ones(N, bool)
        np.testing.assert_array_equal(bits(pn)[touched], bits(pn_ref)[touched])
        np.testing.assert_array_equal(bits(pw)[touched], bits(exp_pdf)[touched])
        np.testing.assert_array_equal(bits(dio), bits(exp_dir))
        assert (pn.cpu().numpy()[~touched] == -7.0).all() and (pw.cpu().numpy()[~touched] == -7.0).all()
    # NULL masks: every lane has an emitter sample and is warped
    dio = dev(torch, d_bsdf)
    pn, pw = g.guideBounceWarp(dp, dd_nee, None, None, dio, du)
    d_all, pdf_all = model.sample_warp(p, u)
    np.testing.assert_array_equal(bits(dio), bits(d_all))
    np.testing.assert_array_equal(bits(pw), bits(pdf_all))
    np.testing.assert_array_equal(bits(pn), bits(tree.pdf(p, d_nee)))
    np.testing.assert_array_equal(smp.state.cpu().numpy(), state0)
    torch.cuda.synchronize()


def test_the_default_queries_do_not_notice_the_warp(oracle_trees, monkeypatch):
    """pg_sample, pg_pdf and pg_guide_bounce give the same bits on the same inputs before and after warp calls: no state is shared."""
    import torch
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    tree, model = oracle_trees["skewed"]
    g = _gpu_tree("skewed", tree, monkeypatch)
    p, u, active = warp_inputs(model, 80)
    d = synth.directions_uniform(N, 83)
    sel = np.where(u[0] < 0.3, 0, np.where(u[0] < 0.6, 1, 2)).astype(np.uint8)
    dp, du, dd, dsel, dact = dev(torch, p), dev(torch, u), dev(torch, d), dev(torch, sel), dev(torch, active)

    def defaults():
        s1, s2 = PCG32Sampler(g, N, seed=84), PCG32Sampler(g, N, seed=85)
        ds, ps = g.sample(dp, s1, dact)
        pp = g.pdf(dp, dd, dact)
        dio = dd.clone()
        pn, pw = g.guideBounce(dp, dd, dact, dsel, dio, s2)
        return [bits(x).copy() for x in (ds, ps, pp, dio, pn, pw)] + [s1.state.cpu().numpy(), s2.state.cpu().numpy()]

    before = defaults()
    dw, _ = g.sampleWarp(dp, du, dact)
    g.invertWarp(dp, dw)
    g.guideBounceWarp(dp, dd, dact, dsel, dd.clone(), du)
    for a, b in zip(before, defaults()):
        np.testing.assert_array_equal(a, b)
    # and the oracle's, as ever
    st, inc = po.rng_seed(N, 84)
    d_o, pdf_o = tree.sample(p, st, inc, active)
    np.testing.assert_array_equal(before[0], d_o.view(np.uint32))
    np.testing.assert_array_equal(before[1], pdf_o.view(np.uint32))
    torch.cuda.synchronize()
