"""PG_SPATIAL_OVERLAP_BOX ("overlap") on the device against its numpy model (tests/filter_overlap_model.py), bit for bit through
exportAccumulators(): every limb, every count, every canonical node -- the stream, the dense buffer and the renderer's own
record list; and that its sums do not depend on order, launches or batching.  Runs on the MI355X box only (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

import filter_overlap_model as fom
import synth
from oracle import pg_oracle as po
from test_filter_overlap_model import (BB0, BB1, assert_lopsided, dyadic_cases, energy_by_leaf, lopsided_kd_tree, lopsided_records,
                                       one_record)
from test_gpu_filter import assert_is_model, dense_records, dev, gpu_splat, gpu_tree, same_accumulators

pytestmark = pytest.mark.gpu

F = np.float32
DIRECTIONAL = ["nearest", "box"]


@pytest.fixture(autouse=True)
def _synchronise_behind_every_call():
    """a GPU fault then names the call that launched the faulting kernel"""
    from practical_path_guiding_lab_amd import sdtree
    sdtree.SYNC_EVERY_CALL = True
    yield
    sdtree.SYNC_EVERY_CALL = False


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    return torch


@pytest.fixture(scope="module")
def skewed_cols():
    return synth.build_skewed(1 << 15, 5).prev.export()


@pytest.fixture(scope="module")
def stream():
    """the main stream: 2^17 records with the hazard rows of tests/test_gpu_filter.py"""
    rec = synth.records(1 << 17, 41, BB0, BB1)
    rec["position"][:, 0] = [-5.0, 1.0, 1.0]        # outside the root box: as without a filter
    rec["position"][:, 1] = [np.nan, 1.0, 1.0]
    rec["position"][:, 2] = [0.0, 0.0, 0.0]          # the root's corners and a face: the box is shifted
    rec["position"][:, 3] = [100.0, 100.0, 100.0]
    rec["position"][:, 4] = [50.0, 50.0, 50.0]       # on the split planes
    rec["direction"][:, 5] = [0.5, 0.5]              # cell corners and edges
    rec["direction"][:, 6] = [0.25, 0.5]
    rec["direction"][:, 7] = [1.0, 1.0]
    rec["direction"][:, 8] = [0.0, 0.0]
    rec["direction"][:, 9] = [1.5, 0.5]              # outside the unit square: fallback counter, the emitter pair still deposits
    rec["direction_nee"][:, 10] = [np.nan, 0.5]
    rec["radiance"][11] = 1e-13                      # below 2^-40
    rec["radiance"][12] = -3.0
    rec["radiance"][13] = np.nan
    rec["woPdf"][14] = 0.0
    rec["direction"][:, 15] = [1.5, 0.5]             # neither direction reaches a leaf
    rec["direction_nee"][:, 15] = [0.5, -0.5]
    return rec


@pytest.fixture(scope="module")
def stream_models(skewed_cols, stream):
    """the model of the main stream on the skewed tree per directional filter, computed once and shared by the tests that need it"""
    made = {}

    def get(directional):
        if directional not in made:
            made[directional] = fom.splat(skewed_cols, stream, directional)
        return made[directional]

    return get


def overlap_tree(cols, directional):
    g = gpu_tree(cols)
    g.setSplatFilter("overlap", directional, seed=17)    # (the seed is ignored)
    return g


# ---- a. the dyadic cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directional", DIRECTIONAL)
def test_dyadic_cases_on_the_device(torch_mod, directional):
    cols = synth.build_balanced(3, 0).export()
    for pos, exp in dyadic_cases(cols):
        g = overlap_tree(cols, directional)
        rec = one_record(pos)
        gpu_splat(torch_mod, g, rec)
        kd, lo, hi = g.exportAccumulators()
        assert energy_by_leaf(cols, lo) == exp and (hi == 0).all() and kd[0] == 1, (pos, energy_by_leaf(cols, lo), exp)
        assert_is_model(g, fom.splat(cols, rec, directional))
    one = synth.build_balanced(0, 3).export()          # a single KD leaf: nearest
    rec = synth.records(1 << 10, 31, BB0, BB1)
    a, b = overlap_tree(one, directional), gpu_tree(one)
    b.setSplatFilter("nearest", directional)
    gpu_splat(torch_mod, a, rec)
    gpu_splat(torch_mod, b, rec)
    assert same_accumulators(a, b)


# ---- b. the stream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directional", DIRECTIONAL)
def test_overlap_splat_is_the_model(torch_mod, skewed_cols, stream, stream_models, directional):
    g = overlap_tree(skewed_cols, directional)
    gpu_splat(torch_mod, g, stream)
    r = stream_models(directional)
    print("overlap / %s: %.3f deposits per record, %.2f KD leaves per filtered record"
          % (directional, r["deposits"] / (1 << 17), r["item"].size / r["filtered"].sum()))
    assert r["filtered"].mean() > 0.9
    assert_is_model(g, r)


# ---- c. the lopsided KD tree --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directional", DIRECTIONAL)
def test_lopsided_kd_tree_on_the_device(torch_mod, directional):
    cols = lopsided_kd_tree()
    assert_lopsided(cols)
    rec = lopsided_records(1 << 12, 55)
    r = fom.splat(cols, rec, directional)
    per_record = np.bincount(r["item"], minlength=64 + (1 << 12))
    assert (per_record[:64] > 512).all()                # 64 consecutive records of > 512 deposits each: the queue drains many times
    g = overlap_tree(cols, directional)
    gpu_splat(torch_mod, g, rec)
    assert_is_model(g, r)


# ---- d. order freedom ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directional", DIRECTIONAL)
def test_overlap_sums_do_not_depend_on_order_or_launches(torch_mod, skewed_cols, stream, stream_models, directional):
    back = {k: np.ascontiguousarray(v[..., ::-1]) for k, v in stream.items()}
    cut = 50_001
    g = overlap_tree(skewed_cols, directional)
    gpu_splat(torch_mod, g, {k: np.ascontiguousarray(v[..., :cut]) for k, v in back.items()})
    gpu_splat(torch_mod, g, {k: np.ascontiguousarray(v[..., cut:]) for k, v in back.items()})
    assert_is_model(g, stream_models(directional))


# ---- e. the routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("directional", DIRECTIONAL)
def test_overlap_process_and_splat_is_the_model(torch_mod, skewed_cols, directional):
    R, D = 2_003, 8
    Lfinal, rec = dense_records(R, D, 77)
    exp = po.process_records(R, D, Lfinal, rec)
    g = overlap_tree(skewed_cols, directional)
    g.processAndSplat(R, D, dev(torch_mod, Lfinal), {k: dev(torch_mod, v) for k, v in rec.items()})
    r = fom.splat(skewed_cols, exp, directional)
    assert r["filtered"].sum() > 1000
    assert_is_model(g, r)


@pytest.mark.parametrize("directional", DIRECTIONAL)
def test_overlap_recording_pass_is_pg_splat_of_its_records(directional):
    from test_gpu_render_filter import RECORD_KEYS, host_records, recording_pass

    sc, g, cols, _, exp = recording_pass("cornell-box", "overlap", directional)
    g2 = overlap_tree(cols, directional)
    g2.addDataPropagate({k: exp[k] for k in RECORD_KEYS}, exp["count"])
    assert same_accumulators(g.sdTree, g2)
    rec, slot, n = host_records(exp)
    r = fom.splat(cols, rec, directional)
    assert n > 1000 and r["filtered"].sum() > 1000 and r["item"].size > r["filtered"].sum()   # (records did reach second leaves)
    assert_is_model(g.sdTree, r)


# ---- f. batching --------------------------------------------------------------------------------------------------------------
def test_overlap_is_independent_of_batching():
    import torch
    from practical_path_guiding_lab_amd import scene as S
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene

    sc = S.cornell_box(40, 28, 6, 3)
    bmin, bmax = sc.bbox_min - F(1e-4), sc.bbox_max + F(1e-4)

    def fresh(cols=None):
        g = PathGuidingIntegrator({"max_depth": sc.max_depth, "rr_depth": sc.rr_depth})
        g.setup(40 * 28, bmin, bmax, 20, 20, True, 0.5)
        if cols is not None:
            g.sdTree.load(cols)
        return g, WavefrontScene(sc, record_geometry=True)

    g, ws = fresh()
    for k in range(3):
        g.setIteration(k, False)
        g.sample(ws, IndependentSampler(4 << k, 700 + k))
        g.refineAndPrepareSDTreeForNextIteration()
    cols = g.sdTree.export()
    assert g.sdTree.stats().n_kd_leaves > 1 and g.sdTree.stats().n_quad_records > 0

    def run(batched):
        g, ws = fresh(cols)
        g.setIteration(3, False)
        g.setSplatFilter("overlap", "box")
        if batched:
            g.sample(ws, IndependentSampler(4, 900, batched=True))
        else:
            for s in range(4):
                g.sample(ws, IndependentSampler(1, 900 + s))
        ws.join()
        torch.cuda.synchronize()
        return g.sdTree.exportAccumulators()

    ref, one_launch = run(False), run(True)
    assert ref[0][0] > 0
    for a, b in zip(ref, one_launch):
        np.testing.assert_array_equal(a, b)


# ---- g. refine ----------------------------------------------------------------------------------------------------------------
def test_overlap_iteration_refines_and_reimports(torch_mod, skewed_cols):
    g = gpu_tree(skewed_cols)
    g.setIteration(5)
    g.setSplatFilter("overlap", "box")
    gpu_splat(torch_mod, g, synth.records(1 << 17, 61, BB0, BB1))
    g.refineAndPrepare()
    e = g.export()
    assert e["kdtree_isLeaf"].sum() >= skewed_cols["kdtree_isLeaf"].sum() and np.isfinite(e["quadtree_irradiance"]).all()
    assert e["quadtree_irradiance"].max() > 0
    g2 = gpu_tree(e)
    for k, v in g2.export().items():
        np.testing.assert_array_equal(np.asarray(v), np.asarray(e[k]), err_msg=k)


# ---- the C side's boundaries --------------------------------------------------------------------------------------------------
def test_value_2_stays_refused_and_a_pass_without_geometry_names_the_filter():
    import torch
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd import scene as S

    L = N.lib()
    h = C.c_void_p()
    assert L.pg_create(C.byref(h), 0) == 0
    try:
        lo, hi = (C.c_float * 3)(-2, -1, -2), (C.c_float * 3)(2, 3, 2)
        assert L.pg_setup(h, lo, hi, 64, 4, 20, 20, 1, 0.5) == 0
        assert L.pg_set_splat_filter(h, 2, 0, 0) == -1 and b"spatial" in L.pg_last_error(h)
        assert L.pg_set_splat_filter(h, 4, 0, 0) == -1
        sc = S.cornell_box(8, 8, 4, 8)
        cam = N.pg_camera()
        for k in ("origin", "axis_x", "axis_y", "axis_z"):
            setattr(cam, k, (C.c_float * 3)(*[float(v) for v in getattr(sc.camera, k)]))
        cam.tan_half_fov_x, cam.width, cam.height = float(sc.camera.tan_half_fov_x), 8, 8
        q = np.ascontiguousarray(sc.quads, np.float32)
        assert L.pg_scene_set(h, q.shape[0], q.ctypes.data, C.byref(cam)) == 0
        prm = N.pg_pass_params(1, 1, 8, 0, 0, 0)
        Lout = torch.zeros((3, 64), device="cuda")
        assert L.pg_set_iteration(h, 1, 0) == 0
        for directional, word in ((0, "spatial overlap box, directional nearest"), (1, "spatial overlap box, directional box")):
            assert L.pg_set_splat_filter(h, N.PG_SPATIAL_OVERLAP_BOX, directional, 3) == 0
            rc = L.pg_render_pass(h, C.byref(prm), Lout.data_ptr(), None, None, None, None)
            torch.cuda.synchronize()
            assert rc == -1                                         # PG_ERR_INVALID, never a silent nearest splat
            msg = L.pg_last_error(h).decode()
            assert "pg_set_splat_filter" in msg and word in msg, msg
    finally:
        L.pg_destroy(h)
