"""Recording render passes that keep their path vertices' geometry (pg_render_record_geometry): the same results at
nearest / nearest, the vertices as an exported record stream (pg_render_export_records), and the training filters of
pg_set_splat_filter applied by the pass itself -- against the CPU oracle, the numpy model of the filters
(tests/filter_model.py) and the library's own pg_splat.  Runs on the MI355X box only (-m gpu)."""
import os

import numpy as np
import pytest

import filter_model as fm
from oracle import pg_oracle as po
from test_gpu_filter import COMBOS, assert_is_model, gpu_tree, same_accumulators
from test_gpu_render import _same_tree

pytestmark = pytest.mark.gpu

F = np.float32
RECORD_KEYS = ("position", "direction", "radiance", "woPdf", "direction_nee", "radiance_nee_lum")


def _scene(which):
    from practical_path_guiding_lab_amd import scene as S
    return {"cornell-box": lambda: S.cornell_box(48, 48, 8, 8, boxes=True),   # feature level 0 through the forced split pipeline
            "torus": lambda: S.torus(48, 36),                                   # level 3, max_depth 32: bounces 0-3 k_wave_guide, then k_wave_tail
            "veach-ajar": lambda: S.veach_ajar(64, 36),                         # level 2, textures
            "veach-ajar 320x180": lambda: S.veach_ajar(320, 180)}[which]()     # deep sorted bounces through k_wave_guide


SMALL = ["cornell-box", "torus", "veach-ajar"]
# samples per pixel of the tested pass.  320x180 x 8 = 460 800 paths, the shape of tests/test_gpu_render.py's deep test: at the 4 spp
# first planned (230 400 paths) 121 517 paths are alive after bounce 3 (measured), fewer than kTailPaths, so k_wave_tail takes over at
# bounce 4 and renderLiveCounts(13)[5] > 128 Ki -- the assertion that the per-bounce kernels ran deep -- cannot hold
TEST_SPP = {"cornell-box": 32, "torus": 32, "veach-ajar": 32, "veach-ajar 320x180": 8}
_trained = {}


def _bbox(sc):
    return sc.bbox_min - F(1e-4), sc.bbox_max + F(1e-4)


def trained(which):
    """The scene, an integrator whose tree was trained with nearest over iterations 0-2 (4, 8, 16 spp) -- and, where that leaves
    the KD tree a single leaf (torus at 48x36: too few vertices inside the box), over further doubling iterations until it has
    split --, a geometry-recording WavefrontScene, the exported columns of that tree and the iteration the tested pass belongs
    to; made once per scene.  A test reloads the columns (which also zeroes sdTree_current) and renders ITS pass."""
    if which not in _trained:
        from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
        from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene
        sc = _scene(which)
        g = PathGuidingIntegrator({"max_depth": sc.max_depth, "rr_depth": sc.rr_depth})
        g.setup(sc.camera.width * sc.camera.height, *_bbox(sc), 20, 20, True, 0.5)
        ws = WavefrontScene(sc, record_geometry=True)
        k = 0
        while k < 3 or (g.sdTree.stats().n_kd_leaves <= 1 and k < 7):
            g.setIteration(k, False)
            g.sample(ws, IndependentSampler(4 << k, 300 + k))
            g.refineAndPrepareSDTreeForNextIteration()
            k += 1
        st = g.sdTree.stats()
        assert st.n_kd_leaves > 1 and st.max_quad_depth >= 3, (which, k, st.n_kd_leaves, st.max_quad_depth)
        _trained[which] = (sc, g, ws, g.sdTree.export(), k)
    return _trained[which]


def recording_pass(which, spatial, directional, filter_seed=11, seed=4242):
    """One recording pass of the iteration behind the training on the trained tree; returns what the test compares."""
    from practical_path_guiding_lab_amd.render import IndependentSampler
    sc, g, ws, cols, k = trained(which)
    g.sdTree.load(cols)
    g.setIteration(k, False)
    g.setSplatFilter(spatial, directional, filter_seed)
    L, valid, _ = g.sample(ws, IndependentSampler(TEST_SPP[which], seed))
    ws.join()
    return sc, g, cols, L, g.sdTree.exportPassRecords(0)


def host_records(exp):
    """The exported stream as filter_model.splat takes it: the first `count` records of every column, and their slots."""
    n = int(exp["count"].cpu().numpy()[0])
    rec = {k: np.ascontiguousarray(exp[k].cpu().numpy()[..., :n]) for k in RECORD_KEYS}
    return rec, exp["slot"].cpu().numpy()[:n].view(np.uint32).astype(np.int64), n


# ---- 1. geometry on changes nothing at nearest -------------------------------------------------------------------------
@pytest.mark.parametrize("which", SMALL)
def test_recording_geometry_changes_nothing_at_nearest(which):
    """tests/test_gpu_render.py::_guided_lifecycle_bit_exact with record_geometry=True: radiance, sums, accumulators and refined
    trees against the oracle over a guided lifecycle (the recording passes run k_wave_guide<true> / k_wave_tail<., true>)."""
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene

    sc = _scene(which)
    D, RR = sc.max_depth, sc.rr_depth
    bmin, bmax = _bbox(sc)
    npix = sc.camera.width * sc.camera.height
    o = po.OracleSDTreePair()
    o.setup(bmin, bmax, 20, 20, True)
    o_sumL, o_sumL2 = np.zeros((3, npix), F), np.zeros((3, npix), F)
    g = PathGuidingIntegrator({"max_depth": D, "rr_depth": RR})
    g.setup(npix, bmin, bmax, sdTreeMaxDepth=20, quadTreeMaxDepth=20, isStoreNEERadiance=True, bsdfSamplingFraction=0.5)
    ws = WavefrontScene(sc, record_geometry=True)
    cumm = 0
    for k in range(4):
        final = k == 3
        g.setIteration(k, final)
        for spp in ([1, 3] if k == 0 else [2 ** (k + 2)]):
            seed = 5000 + cumm
            Lo, vo = po.render_pass(o, sc, sc.camera, D, RR, k, final, seed, spp, True, 0.5, o_sumL, o_sumL2)
            Lg, vg, _ = g.sample(ws, IndependentSampler(spp, seed))
            np.testing.assert_array_equal(Lg.cpu().numpy().view(np.uint32), Lo.view(np.uint32))
            np.testing.assert_array_equal(vg.cpu().numpy(), vo)
            cumm += spp
        np.testing.assert_array_equal(g.sumL.cpu().numpy().view(np.uint32), o_sumL.view(np.uint32))
        kd, lo, hi = g.sdTree.exportAccumulators()
        np.testing.assert_array_equal(kd, o.current.kd_column("count"))
        np.testing.assert_array_equal(lo, o.current.quad_column("acc_lo"))
        np.testing.assert_array_equal(hi, o.current.quad_column("acc_hi"))
        if not final:
            o.refine_and_prepare(k)
            g.refineAndPrepareSDTreeForNextIteration()
            _same_tree(o.prev.export(), g.sdTree.export())


# ---- 2. the exported stream is the pass ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SMALL)
def test_exported_stream_is_the_pass(which):
    sc, g, cols, _, exp = recording_pass(which, "nearest", "nearest")
    g2 = gpu_tree(cols)
    g2.addDataPropagate({k: exp[k] for k in RECORD_KEYS}, exp["count"])
    assert same_accumulators(g.sdTree, g2)
    assert g.sdTree.exportAccumulators()[0][0] > 0
    rec, slot, n = host_records(exp)
    D = sc.max_depth
    n_lanes = sc.camera.width * sc.camera.height * TEST_SPP[which]
    assert n > 1000 and np.unique(slot).shape[0] == n and slot.max() < n_lanes * D
    # slot % max_depth is the depth of the record: a path has a vertex at depth d > 0 only if it was alive after bounce d - 1
    # (test_exported_geometry_is_the_path_vertex checks the order of a path's vertices against their positions)
    live = g.sdTree.renderLiveCounts(D)
    depth = slot % D
    for d in range(1, D):
        assert (depth == d).sum() <= live[d - 1], (d, int((depth == d).sum()), live[d - 1])
    assert (depth == 0).sum() <= n_lanes


# ---- 3. the geometry is the vertex --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SMALL)
def test_exported_geometry_is_the_path_vertex(which):
    """Independent of the code under test and loose by design (1e-2): swapped planes or entries are errors of order one."""
    sc, g, cols, _, exp = recording_pass(which, "nearest", "nearest")
    rec, slot, n = host_records(exp)
    bmin, bmax = _bbox(sc)
    p = rec["position"]
    assert (p >= bmin[:, None]).all() and (p <= bmax[:, None]).all()
    assert (rec["direction_nee"] >= 0).all() and (rec["direction_nee"] <= 1).all()  # (also where the bounce computed none)
    # consecutive depths of one path: the next vertex lies along the recorded path direction
    order = np.argsort(slot)
    s, ps = slot[order], p[:, order]
    wo = po.canonical_to_dir(np.ascontiguousarray(rec["direction"][:, order]))
    D = sc.max_depth
    pair = np.nonzero((s[1:] == s[:-1] + 1) & (s[1:] % D != 0))[0]
    step = ps[:, pair + 1] - ps[:, pair]
    dist = np.sqrt((step.astype(np.float64) ** 2).sum(axis=0))
    far = dist > 0.01 * float(np.linalg.norm((bmax - bmin).astype(np.float64)))
    assert far.sum() > 1000, int(far.sum())
    err = np.abs(step[:, far] / dist[far] - wo[:, pair[far]])
    print("%s: %d vertex pairs, largest direction error %.3e" % (which, int(far.sum()), float(err.max())))
    assert err.max() < 1e-2
    if which == "cornell-box":  # the emitter direction of a record that carries emitter light meets the light's rectangle
        q = sc.quads[sc.quads[:, 15] == 1.0]
        assert q.shape[0] == 1
        o, e1, e2, nrm = (q[0, 0:3].astype(np.float64), q[0, 3:6].astype(np.float64), q[0, 6:9].astype(np.float64),
                          q[0, 9:12].astype(np.float64))
        lit = rec["radiance_nee_lum"] > 0
        assert lit.sum() > 1000
        d = po.canonical_to_dir(np.ascontiguousarray(rec["direction_nee"][:, lit])).astype(np.float64)
        pp = p[:, lit].astype(np.float64)
        t = ((o[:, None] - pp) * nrm[:, None]).sum(axis=0) / (d * nrm[:, None]).sum(axis=0)
        hit = pp + t * d - o[:, None]
        u = (hit * e1[:, None]).sum(axis=0) / (e1 @ e1)
        v = (hit * e2[:, None]).sum(axis=0) / (e2 @ e2)
        assert (t > 0).all() and u.min() > -1e-2 and u.max() < 1 + 1e-2 and v.min() > -1e-2 and v.max() < 1 + 1e-2, \
            (t.min(), u.min(), u.max(), v.min(), v.max())


# ---- 4. a filtered pass is the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SMALL + ["veach-ajar 320x180"])
@pytest.mark.parametrize("spatial,directional", COMBOS)
def test_filtered_recording_pass_is_the_model(which, spatial, directional):
    from practical_path_guiding_lab_amd.render import pass_filter_seed
    sc, g, cols, _, exp = recording_pass(which, spatial, directional, filter_seed=11, seed=4242)
    if which == "veach-ajar 320x180":
        live = g.sdTree.renderLiveCounts(13)
        assert live[5] > 128 * 1024, live  # the per-bounce kernels did run deep (sorted bounces through k_wave_guide<true>)
    rec, slot, n = host_records(exp)
    r = fm.splat(cols, rec, spatial, directional, seed=pass_filter_seed(11, 4242), index=slot)
    print("%s %s / %s: %d records, %.3f deposits per record" % (which, spatial, directional, n, r["deposits"] / max(n, 1)))
    assert_is_model(g.sdTree, r)
    if spatial == "nearest":  # no record numbers involved: the exported stream through pg_splat gives the same sums
        g2 = gpu_tree(cols)
        g2.setSplatFilter(spatial, directional)
        g2.addDataPropagate({k: exp[k] for k in RECORD_KEYS}, exp["count"])
        assert same_accumulators(g.sdTree, g2)


# ---- 5. batching and order ----------------------------------------------------------------------------------------------
def test_directional_box_is_independent_of_batching_and_of_passes_in_flight():
    import torch
    from practical_path_guiding_lab_amd import scene as S
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene

    sc = S.cornell_box(40, 28, 6, 3)
    npix = 40 * 28

    def fresh(cols=None, **kw):
        g = PathGuidingIntegrator({"max_depth": sc.max_depth, "rr_depth": sc.rr_depth})
        g.setup(npix, *_bbox(sc), 20, 20, True, 0.5)
        if cols is not None:
            g.sdTree.load(cols)
        return g, WavefrontScene(sc, record_geometry=True, **kw)

    g, ws = fresh()
    for k in range(3):
        g.setIteration(k, False)
        g.sample(ws, IndependentSampler(4 << k, 700 + k))
        g.refineAndPrepareSDTreeForNextIteration()
    cols = g.sdTree.export()
    assert g.sdTree.stats().n_quad_records > 0

    def run(batched, **kw):
        g, ws = fresh(cols, **kw)
        g.setIteration(3, False)
        g.setSplatFilter("nearest", "box")
        if batched:
            g.sample(ws, IndependentSampler(4, 900, batched=True))
        else:
            for s in range(4):
                g.sample(ws, IndependentSampler(1, 900 + s))
        ws.join()
        torch.cuda.synchronize()
        return g.sdTree.exportAccumulators()

    ref = run(False)
    assert ref[0][0] > 0
    for other in (run(True), run(False, in_flight=2), run(True, in_flight=2)):
        for a, b in zip(ref, other):
            np.testing.assert_array_equal(a, b)


# ---- 6. the switch's boundaries -----------------------------------------------------------------------------------------
def test_the_switch_is_opt_in():
    import torch
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd import scene as S
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene

    sc = S.cornell_box(24, 24, 6, 8)

    def fresh(**kw):
        g = PathGuidingIntegrator({"max_depth": sc.max_depth, "rr_depth": sc.rr_depth})
        g.setup(24 * 24, *_bbox(sc), 20, 20, True, 0.5)
        return g, WavefrontScene(sc, **kw)

    # off: the refusal of tests/test_gpu_filter.py::test_recording_render_pass_refuses_a_filter, through the Python layer
    g, ws = fresh()
    g.setIteration(1, False)
    g.setSplatFilter("stochastic", "box", 3)
    with pytest.raises(ValueError, match="record_geometry"):
        g.sample(ws, IndependentSampler(1, 5))
    g.sdTree.setSplatFilter("nearest", "box")  # ... and below it, the library's own
    g.splat_filter = None
    with pytest.raises(N.PgError, match="pg_set_splat_filter"):
        g.sample(ws, IndependentSampler(1, 5))
    with pytest.raises(ValueError):
        g.setSplatFilter("box", "nearest")
    # no records to export after a pass that kept no geometry, or after a final pass of a scene that does
    g.sdTree.setSplatFilter("nearest", "nearest")
    g.sample(ws, IndependentSampler(1, 5))
    with pytest.raises(N.PgError) as e:
        g.sdTree.exportPassRecords(0)
    assert e.value.code == -1 and "recorded no geometry" in str(e.value)
    g2, ws2 = fresh(record_geometry=True)
    g2.setIteration(1, False)
    g2.sample(ws2, IndependentSampler(1, 5))
    assert int(g2.sdTree.exportPassRecords(0)["count"].cpu()[0]) > 0
    with pytest.raises(N.PgError):
        g2.sdTree.exportPassRecords(1)  # (the other buffer set has not rendered)
    g2.setIteration(1, True)
    g2.setSplatFilter("stochastic", "box", 3)
    Lf, _, _ = g2.sample(ws2, IndependentSampler(2, 9))
    with pytest.raises(N.PgError) as e:
        g2.sdTree.exportPassRecords(0)
    assert e.value.code == -1
    # a final pass is untouched by the switch and by the filter
    g.setIteration(1, True)
    Lr, _, _ = g.sample(ws, IndependentSampler(2, 9))
    assert torch.equal(Lf.view(torch.int32), Lr.view(torch.int32)) and float(Lr.max()) > 0


# ---- 7. training through the filters converges --------------------------------------------------------------------------
def test_guided_render_through_the_filters_converges_to_the_ground_truth():
    """The configuration and the bounds of tests/test_gpu_render.py::test_guided_render_converges_to_the_ground_truth, with the
    recording passes depositing through stochastic / box.  Measured on an MI355X (profiles/render_filter/README.md): final MSE
    3.2527e-4 filtered against 3.2406e-4 nearest -- the bounds hold, no gain shown."""
    from practical_path_guiding_lab_amd.driver import load_ground_truth, run_guided_render
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import WavefrontScene
    from practical_path_guiding_lab_amd.scene import cornell_box

    sc = cornell_box(256, 256, 8, 8)
    gt = load_ground_truth(os.path.join(os.path.dirname(__file__), "golden", "cornell_gt_256_f16.npy"), 256, 256)
    final = {}
    for name, filt in (("nearest", None), ("stochastic,box", ("stochastic", "box"))):
        g = PathGuidingIntegrator({"max_depth": 8, "rr_depth": 8})
        ws = WavefrontScene(sc, record_geometry=filt is not None)
        res = run_guided_render(ws, g, 1020, initial_seed=3, ground_truth=gt, training_spp_per_pass=4, log=lambda s: None,
                                splat_filter=filt)
        assert res["cumm_spp"] == 1020
        mse = [r[5] for r in res["records"]["mse_groundTruth_endIter"].rows]
        final[name] = (mse[0], mse[-1], len(mse))
        print("final MSE, %s: %.4e (first iteration %.4e)" % (name, mse[-1], mse[0]))
        if filt is not None:
            assert len(mse) == 8 and all(np.isfinite(mse))
            assert mse[-1] < 0.12 * mse[0] and mse[-1] < 4e-4
