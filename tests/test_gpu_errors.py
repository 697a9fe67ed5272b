"""Error behaviour at the C ABI on a live device: every misuse returns a negative status and leaves a
message in pg_last_error, nothing is launched, the context stays usable.  (The two Python
exceptions of the reference, path_guiding_integrator.py:35-41, live in the Python mirror and are
covered by tests/test_host_logic.py.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from practical_path_guiding_lab_amd import _native as N

    L = N.lib()
    h = C.c_void_p()
    assert L.pg_create(C.byref(h), 0) == 0
    yield N, L, h
    L.pg_destroy(h)


def _msg(L, h):
    return L.pg_last_error(h).decode()


def test_exchange_entry_points_before_their_preconditions(ctx):
    """pg_exchange_pack / _unpack / pg_comm_info: a configured tree, a packed buffer, a communicator."""
    N, L, h = ctx
    p, n = C.c_void_p(), C.c_uint64()
    assert L.pg_exchange_pack(h, C.byref(p), C.byref(n), None) < 0 and "pg_setup" in _msg(L, h)
    assert L.pg_exchange_unpack(h, None) < 0
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    assert L.pg_setup(h, lo, hi, 16, 4, 20, 20, 1, 0.5) == 0
    assert L.pg_exchange_unpack(h, None) < 0 and "pg_exchange_pack first" in _msg(L, h)
    assert L.pg_exchange_pack(h, None, C.byref(n), None) < 0
    assert L.pg_exchange_pack(h, C.byref(p), C.byref(n), None) == 0 and n.value == 3 + 1 and p.value   # one tree: its root accumulator + fallback counter
    assert L.pg_exchange_unpack(h, None) == 0
    a, b = C.c_int32(), C.c_int32()
    assert L.pg_comm_info(h, C.byref(a), C.byref(b)) < 0 and "pg_comm_init" in _msg(L, h)
    assert L.pg_exchange_pack_words(None, 1, None) < 0 and L.pg_exchange_unpack_words(None, 1, None) < 0


def test_calls_before_setup_and_bad_arguments(ctx):
    import torch

    N, L, h = ctx
    x = torch.zeros((3, 8), device="cuda")
    out = torch.zeros(8, device="cuda")
    # queries and recording need a configured tree
    assert L.pg_pdf(h, 8, x.data_ptr(), x.data_ptr(), None, out.data_ptr(), None) < 0
    assert "pg_setup" in _msg(L, h)
    assert L.pg_refine_and_swap(h, None) < 0
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    assert L.pg_setup(h, hi, lo, 16, 4, 20, 20, 1, 0.5) < 0          # inverted bounding box
    assert L.pg_setup(h, lo, hi, 16, 4, -1, 20, 1, 0.5) < 0           # tree depth limits are in [0, 30]
    assert L.pg_setup(h, lo, hi, 16, 4, 20, 31, 1, 0.5) < 0
    assert L.pg_setup(h, lo, hi, 16, 4, 20, 20, 1, 0.5) == 0
    # NULL arrays with a non-zero count
    assert L.pg_pdf(h, 8, None, x.data_ptr(), None, out.data_ptr(), None) < 0
    assert L.pg_sample(h, 8, x.data_ptr(), None, None, None, x.data_ptr(), out.data_ptr(), None) < 0
    # empty batches are fine
    assert L.pg_pdf(h, 0, None, None, None, None, None) == 0
    # the context still works
    assert L.pg_pdf(h, 8, x.data_ptr(), x.data_ptr(), None, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    # NULL context
    assert L.pg_pdf(None, 8, x.data_ptr(), x.data_ptr(), None, out.data_ptr(), None) < 0
    # the scheduling switches take the values the header names and nothing else
    assert L.pg_render_stages(h, 3) < 0 and "pg_render_stages" in _msg(L, h)
    assert L.pg_render_stages(h, -1) < 0
    assert L.pg_render_overlap(h, 2) < 0 and "pg_render_overlap" in _msg(L, h)
    for mode in (2, 1, 0):
        assert L.pg_render_stages(h, mode) == 0
    assert L.pg_render_stages(None, 0) < 0


def test_scene_and_render_pass_misuse(ctx):
    import torch
    from practical_path_guiding_lab_amd import scene as S

    N, L, h = ctx
    lo, hi = (C.c_float * 3)(-2, -1, -2), (C.c_float * 3)(2, 3, 2)
    assert L.pg_setup(h, lo, hi, 64, 4, 20, 20, 1, 0.5) == 0
    sc = S.cornell_box(8, 8, 4, 8)
    cam = N.pg_camera()
    for k in ("origin", "axis_x", "axis_y", "axis_z"):
        setattr(cam, k, (C.c_float * 3)(*[float(v) for v in getattr(sc.camera, k)]))
    cam.tan_half_fov_x, cam.width, cam.height = float(sc.camera.tan_half_fov_x), 8, 8
    prm = N.pg_pass_params(1, 1, 8, 0, 0, 0)
    Lout = torch.zeros((3, 64), device="cuda")
    assert L.pg_render_pass(h, C.byref(prm), Lout.data_ptr(), None, None, None, None) < 0
    assert "pg_scene_set" in _msg(L, h)
    q = np.ascontiguousarray(sc.quads, np.float32)
    assert L.pg_scene_set(h, 0, q.ctypes.data, C.byref(cam)) < 0                      # no shapes
    assert L.pg_scene_set(h, 5000, q.ctypes.data, C.byref(cam)) < 0                   # more than 4096 quads
    bad_cam = N.pg_camera()
    C.memmove(C.byref(bad_cam), C.byref(cam), C.sizeof(cam))
    bad_cam.width = 0
    assert L.pg_scene_set(h, q.shape[0], q.ctypes.data, C.byref(bad_cam)) < 0
    # material table: index out of range, unknown type, spheres without materials, bad radius, alpha <= 0
    mats = np.stack([S.diffuse_material((0.5, 0.5, 0.5)), S.roughconductor_material(0.1, (0.2, 0.9, 1.1), (3.9, 2.4, 2.1))])
    q2 = q.copy()
    q2[:, 22] = 7
    d = N.pg_scene_desc(q2.shape[0], q2.ctypes.data, 0, None, 2, mats.ctypes.data)
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) < 0 and "material index" in _msg(L, h)
    m3 = mats.copy()
    m3[0, 0] = 9
    q2[:, 22] = 0
    d = N.pg_scene_desc(q2.shape[0], q2.ctypes.data, 0, None, 2, m3.ctypes.data)
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) < 0 and "material type" in _msg(L, h)
    m4 = mats.copy()
    m4[1, 4] = 0.0
    d = N.pg_scene_desc(q2.shape[0], q2.ctypes.data, 0, None, 2, m4.ctypes.data)
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) < 0 and "alpha" in _msg(L, h)
    sph = S.sphere((0, 1, 0), 0.2, 0)[None].copy()
    d = N.pg_scene_desc(q.shape[0], q.ctypes.data, 1, sph.ctypes.data, 0, None)
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) < 0 and "material table" in _msg(L, h)
    sph[0, 3] = -1.0
    d = N.pg_scene_desc(q2.shape[0], q2.ctypes.data, 1, sph.ctypes.data, 2, mats.ctypes.data)
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) < 0 and "radius" in _msg(L, h)
    # meshes: the kernels trust the BVH, so a malformed one must be refused here
    from practical_path_guiding_lab_amd import mesh as MS
    v, f = MS.icosphere(1)
    nodes, tris = MS.build_bvh(MS.triangles(v, f, np.eye(4), 0))

    def mesh_desc(nd, tr, m=mats):
        d = N.pg_scene_desc(q2.shape[0], q2.ctypes.data, 0, None, m.shape[0], m.ctypes.data, 0, None)
        d.n_tris, d.tris, d.n_bvh_nodes, d.bvh = tr.shape[0], tr.ctypes.data, nd.shape[0], nd.ctypes.data
        return d

    assert L.pg_scene_set_ex(h, C.byref(mesh_desc(nodes, tris)), C.byref(cam)) == 0
    refs = nodes[:, 24:28]
    is_node = (refs & MS.LEAF_FLAG) == 0
    ni, nc = [int(x[0]) for x in np.nonzero(is_node)]                         # a reference to a node ...
    li, lc = [int(x[0]) for x in np.nonzero(~is_node & (refs != MS.EMPTY_CHILD))]   # ... and one to a leaf
    other = int(refs[is_node][1])
    for what, edit in (("follow their parent", lambda nd: nd.__setitem__((ni, 24 + nc), ni)),             # a cycle
                       ("follow their parent", lambda nd: nd.__setitem__((ni, 24 + nc), nd.shape[0])),     # child past the array
                       ("two parents", lambda nd: nd.__setitem__((ni, 24 + nc), other)),                   # a node referenced twice
                       ("without children", lambda nd: nd.__setitem__((ni, slice(24, 28)), MS.EMPTY_CHILD)),
                       ("triangle array", lambda nd: nd.__setitem__((li, 24 + lc), MS.LEAF_FLAG | (3 << 28) | (tris.shape[0] - 2)))):  # leaf past the triangles
        bad = nodes.copy()
        edit(bad)
        rc = L.pg_scene_set_ex(h, C.byref(mesh_desc(bad, tris)), C.byref(cam))
        assert rc < 0 and what in _msg(L, h), (what, _msg(L, h))
    # a chain of nodes with three waiting siblings each would overflow the walk's 32-entry stack (8 in LDS + 24 in the workspace)
    chain = np.zeros((30, MS.BVH_STRIDE), np.uint32)
    chain[:, 0:12] = np.float32(-1).view(np.uint32)
    chain[:, 12:24] = np.float32(1).view(np.uint32)
    chain[:, 24:28] = MS.LEAF_FLAG  # one-triangle leaves on triangle 0
    chain[:-1, 24] = np.arange(1, 30)
    assert L.pg_scene_set_ex(h, C.byref(mesh_desc(chain, tris)), C.byref(cam)) < 0 and "stack" in _msg(L, h)
    assert L.pg_scene_set_ex(h, C.byref(mesh_desc(chain[:20], tris)), C.byref(cam)) < 0   # (its last node points past the array)
    bad_t = tris.copy()
    bad_t[3, 12] = 5
    assert L.pg_scene_set_ex(h, C.byref(mesh_desc(nodes, bad_t)), C.byref(cam)) < 0 and "triangle material" in _msg(L, h)
    d = mesh_desc(nodes, tris)
    d.n_bvh_nodes = 0
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) < 0 and "go together" in _msg(L, h)
    # a good scene, then pass parameters
    assert L.pg_scene_set(h, q.shape[0], q.ctypes.data, C.byref(cam)) == 0
    for bad in (N.pg_pass_params(1, 0, 8, 0, 0, 0), N.pg_pass_params(1, 1, 8, 0, 65, 0), N.pg_pass_params(1, 1, 8, 0, 10, 60)):
        assert L.pg_render_pass(h, C.byref(bad), Lout.data_ptr(), None, None, None, None) < 0
    s1 = torch.zeros((3, 64), device="cuda")
    assert L.pg_render_pass(h, C.byref(prm), Lout.data_ptr(), None, s1.data_ptr(), None, None) < 0   # sumL without sumL2
    assert L.pg_render_pass(h, C.byref(prm), None, None, None, None, None) < 0
    assert L.pg_film_tent(h, 1, 0, Lout.data_ptr(), Lout.data_ptr(), None) < 0
    assert L.pg_math_eval(h, 9, 4, Lout.data_ptr(), Lout.data_ptr(), None) < 0
    # stripes (interleaved sharding): rows per band, rank index, and the pixel count must be consistent
    for bad in (N.pg_pass_params(1, 1, 8, 0, 0, 0, 0, 0, 2, 0), N.pg_pass_params(1, 1, 8, 0, 0, 0, 2, 2, 2, 0),
                N.pg_pass_params(1, 1, 8, 0, 8, 0, 2, 0, 2, 0), N.pg_pass_params(1, 1, 8, 0, 0, 24, 2, 0, 2, 0)):
        assert L.pg_render_pass(h, C.byref(bad), Lout.data_ptr(), None, None, None, None) < 0 and "stripe" in _msg(L, h)
    assert L.pg_render_pass(h, C.byref(N.pg_pass_params(1, 1, 8, 0, 0, 32, 2, 1, 2, 0)), Lout.data_ptr(), None, None, None, None) == 0
    # the per-pixel sums are film-sized arrays: a context set up for fewer rays than the film has pixels must
    # not be handed sums (k_finish would write past what setup(numRays) made the caller allocate)
    assert L.pg_setup(h, lo, hi, 32, 4, 20, 20, 1, 0.5) == 0
    s2 = torch.zeros((3, 64), device="cuda")
    assert L.pg_render_pass(h, C.byref(prm), Lout.data_ptr(), None, s1.data_ptr(), s2.data_ptr(), None) < 0 and "num_rays" in _msg(L, h)
    assert L.pg_render_pass(h, C.byref(prm), Lout.data_ptr(), None, None, None, None) == 0   # without sums it is fine
    assert L.pg_setup(h, lo, hi, 64, 4, 20, 20, 1, 0.5) == 0
    assert L.pg_render_pass(h, C.byref(prm), Lout.data_ptr(), None, s1.data_ptr(), s2.data_ptr(), None) == 0
    # textures: a material naming a texture that is not there, a bitmap reaching past the texel array
    tm = np.stack([S.diffuse_material((0.5, 0.5, 0.5), texture=0), S.diffuse_material((0.1, 0.1, 0.1))])
    tex, texels = S.pack_textures([S.bitmap_texture(np.zeros((4, 4, 3), np.uint8))])
    lut = S.srgb_to_linear_lut()
    uvs = np.zeros((tris.shape[0], 6), np.float32)
    d = mesh_desc(nodes, tris, tm)
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) < 0 and "texture index" in _msg(L, h)
    d.tri_uvs, d.n_textures, d.textures, d.n_texels, d.texels, d.srgb_lut = (uvs.ctypes.data, 1, tex.ctypes.data, 15, texels.ctypes.data,
                                                                              lut.ctypes.data)
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) < 0 and "texel array" in _msg(L, h)
    d.n_texels = 16
    assert L.pg_scene_set_ex(h, C.byref(d), C.byref(cam)) == 0
    assert L.pg_scene_set(h, q.shape[0], q.ctypes.data, C.byref(cam)) == 0
    # and the good call still works afterwards
    assert L.pg_render_pass(h, C.byref(prm), Lout.data_ptr(), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Lout).all()) and float(Lout.sum()) > 0
    live = (C.c_uint32 * 4)()
    assert L.pg_render_live_counts(h, live, 4) == 0 and live[3] == 0 and live[0] > 0


def _same_cols(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and (x.astype(np.float64) == y.astype(np.float64)).all(), k


def test_a_refine_that_fails_leaves_both_trees_exactly_as_they_were():
    """pg_refine_and_swap is a transaction (the reference grows by allocate-new + copy, common.py:161-189, so
    its sdTree_prev survives a failed split): with pg_debug_fail_alloc the FIRST device allocation every attempt still needs is
    refused -- attempt after attempt, so that every allocation site of a refine is the failing one once (resolve scratch, the KD
    copy, the quadtree rebuild level by level, the spare accumulators).  After every failed attempt (PG_ERR_NOMEM) the context
    is still configured and answers as before, bit for bit: the 23 exported columns (sdTree_prev), every accumulator limb and
    KD count of the running iteration (sdTree_current), pg_pdf and pg_sample on 4096 queries, pg_get_stats.  Then a guided
    render pass runs on it and on a twin that never failed (same radiance, same accumulators), the refine goes through, and
    tree and next iteration equal the twin's and the ORACLE's.  A refused allocation of the jump tables (after the commit) is
    no error: the forest is walked from its roots with the same results."""
    import torch
    from oracle import pg_oracle as po
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene
    from practical_path_guiding_lab_amd.scene import cornell_box
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler

    L = N.lib()
    w = h = 96
    depth = 6
    sc = cornell_box(w, h, depth, 8)
    bmin, bmax = sc.bbox_min - np.float32(1e-4), sc.bbox_max + np.float32(1e-4)

    def make():
        g = PathGuidingIntegrator({"max_depth": depth, "rr_depth": 8})
        g.setup(w * h, bmin, bmax, 20, 20, True, 0.5)
        return g, WavefrontScene(sc)

    (a, wa), (b, wb) = make(), make()
    o = po.OracleSDTreePair()
    o.setup(bmin, bmax, 20, 20, True)
    spp = [4, 8, 16, 256]     # (the last iteration brings 16 times the records: the tree outgrows every buffer the earlier refines left)
    for k in range(3):
        for g, ws in ((a, wa), (b, wb)):
            g.setIteration(k, False)
            g.sample(ws, IndependentSampler(spp[k], 100 + k))
            g.refineAndPrepareSDTreeForNextIteration()
        po.render_pass(o, sc, sc.camera, depth, 8, k, False, 100 + k, spp[k], True, 0.5)
        o.refine_and_prepare(k)
    for g, ws in ((a, wa), (b, wb)):
        g.setIteration(3, False)
        g.sample(ws, IndependentSampler(spp[3], 103))
    Lo3, _ = po.render_pass(o, sc, sc.camera, depth, 8, 3, False, 103, spp[3], True, 0.5)

    tree = a.sdTree
    n = 4096
    gen = torch.Generator(device="cuda").manual_seed(3)
    lo_ = torch.from_numpy(np.asarray(sc.bbox_min, np.float32)).cuda().reshape(3, 1)
    ext = torch.from_numpy(np.asarray(sc.bbox_max - sc.bbox_min, np.float32)).cuda().reshape(3, 1)
    P = (lo_ + ext * torch.rand((3, n), generator=gen, device="cuda")).contiguous()
    z = 2.0 * torch.rand(n, generator=gen, device="cuda") - 1.0
    phi = 6.2831853 * torch.rand(n, generator=gen, device="cuda")
    s_ = (1.0 - z * z).clamp_min(0).sqrt()
    D = torch.stack([s_ * torch.cos(phi), s_ * torch.sin(phi), z]).contiguous()

    def snapshot():
        st = tree.stats()
        d, pdf_s = tree.sample(P, PCG32Sampler(tree, n, seed=9))
        return {"cols": tree.export(), "acc": tree.exportAccumulators(), "raw": tree.accumulators().clone(),
                "pdf": tree.pdf(P, D).clone(), "dir": d.clone(), "pdf_s": pdf_s.clone(),
                "stats": (st.n_kd_nodes, st.n_kd_leaves, st.n_quad_records, st.n_trees, st.jump_bits, st.kd_grid_bits)}

    before = snapshot()
    assert before["cols"]["kdtree_depth"].shape[0] > 3 and int(before["acc"][0][0]) > 0
    failures, sites, skip = 0, set(), 0
    fired_after_commit = False
    for attempt in range(200):
        # the allocation after `skip` successful ones is refused: at first the first one an attempt still needs (buffers keep what
        # earlier attempts allocated, so the refused one moves on through the refine); a buffer that is grown through a temporary,
        # or handed back and forth between levels, keeps nothing of a failed attempt -- then one more allocation is let through
        assert L.pg_debug_fail_alloc(skip) == 0
        try:
            tree.refineAndPrepare()
        except N.PgError as e:
            assert e.code == -3 and L.pg_debug_fail_alloc_pending() == 0, e      # PG_ERR_NOMEM, from the hook
            assert "no longer valid" not in str(e)
            failures += 1
            if str(e) in sites:   # (no new place reached: let one more allocation through from now on)
                skip += 1
            sites.add(str(e))
            now = snapshot()                            # (a context that lost its tree would refuse every one of these calls)
            _same_cols(before["cols"], now["cols"])
            for x, y in zip(before["acc"], now["acc"]):
                np.testing.assert_array_equal(x, y)
            assert torch.equal(before["raw"], now["raw"]) and before["stats"] == now["stats"]
            for key in ("pdf", "dir", "pdf_s"):
                assert torch.equal(before[key].view(torch.int32), now[key].view(torch.int32)), key
            continue
        fired_after_commit = L.pg_debug_fail_alloc_pending() == 0   # (refused behind the commit: the jump tables' buffer)
        L.pg_debug_fail_alloc(-1)
        break
    else:
        pytest.fail("the refine never went through: " + str(sorted(sites)))
    # resolve scratch, the KD copy, the quadtree rebuild, the spare accumulators: many different allocations were the refused one
    assert failures >= 8 and len(sites) >= 8, sorted(sites)
    assert any("new_kd" in m for m in sites) and any("new_acc" in m for m in sites) and any("new_rec" in m for m in sites), sorted(sites)
    b.refineAndPrepareSDTreeForNextIteration()
    o.refine_and_prepare(3)
    cols = tree.export()
    _same_cols(cols, b.sdTree.export())
    _same_cols(cols, o.prev.export())
    assert cols["kdtree_depth"].shape[0] > before["cols"]["kdtree_depth"].shape[0]       # the refine did split
    assert int(tree.accumulators().abs().sum()) == 0                                      # sdTree_current reset
    # the next iteration on the once-failed context: radiance of the twin and of the oracle, then equal trees again
    for g, ws in ((a, wa), (b, wb)):
        g.setIteration(4, False)
    La = a.sample(wa, IndependentSampler(4, 500))[0]
    Lb = b.sample(wb, IndependentSampler(4, 500))[0]
    Lo, _ = po.render_pass(o, sc, sc.camera, depth, 8, 4, False, 500, 4, True, 0.5)
    assert torch.equal(La.view(torch.int32), Lb.view(torch.int32))
    np.testing.assert_array_equal(La.cpu().numpy().view(np.uint32), Lo.view(np.uint32))
    assert torch.equal(a.sdTree.accumulators(), b.sdTree.accumulators())
    a.refineAndPrepareSDTreeForNextIteration()
    b.refineAndPrepareSDTreeForNextIteration()
    _same_cols(a.sdTree.export(), b.sdTree.export())
    if fired_after_commit:   # (the tables came back with the refine that followed)
        assert a.sdTree.stats().jump_bits == b.sdTree.stats().jump_bits


def test_a_scene_set_that_fails_leaves_the_context_without_a_scene():
    """pg_scene_set_ex commits at its end: a device allocation refused half-way through the upload of a BIGGER scene (the host-side
    hook pg_debug_fail_alloc: a torus-class scene after the cornell box -- triangles, BVH nodes, a directional light, none of which
    the resident buffers hold, so DevBuf::ensure really allocates; one allocation is let through, the second is refused) is
    PG_ERR_NOMEM and leaves the context WITHOUT a scene -- the old tables are partly gone, so the next pg_render_pass answers
    PG_ERR_INVALID "call pg_scene_set first" instead of launching on the old counts.  Setting the first scene again renders the
    first run's radiance, byte for byte; the bigger scene then goes through as well (memory is back)."""
    import torch
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene
    from practical_path_guiding_lab_amd.scene import cornell_box, torus

    L = N.lib()
    w, h, depth, spp = 32, 24, 4, 2
    small, big = cornell_box(w, h, depth, 8), torus(w, h, depth, 8)
    assert big.tris.shape[0] > 0 and big.bvh.shape[0] > 0 and big.dir_lights.shape[0] > 0 and small.tris.shape[0] == 0
    g = PathGuidingIntegrator({"max_depth": depth, "rr_depth": 8})
    g.setup(w * h, small.bbox_min - np.float32(1e-4), small.bbox_max + np.float32(1e-4), 20, 20, True, 0.5)
    g.setIteration(0, False)
    ws, wb = WavefrontScene(small), WavefrontScene(big)
    first = g.sample(ws, IndependentSampler(spp, 7))[0].clone()
    assert bool((first != 0).any())
    tree = g.sdTree
    try:
        assert L.pg_debug_fail_alloc(1) == 0
        with pytest.raises(N.PgError) as e:
            wb._upload(tree)
        assert e.value.code == -3 and L.pg_debug_fail_alloc_pending() == 0, e.value      # PG_ERR_NOMEM, from the hook
    finally:
        L.pg_debug_fail_alloc(-1)
    with pytest.raises(N.PgError) as e:                      # (ws believes its scene is still the context's: no upload, the pass itself)
        g.sample(ws, IndependentSampler(spp, 7))
    assert e.value.code == -1 and "pg_scene_set first" in str(e.value), e.value          # PG_ERR_INVALID: nothing was launched
    prm = N.pg_pass_params(7, spp, 8, 0, 0, 0)
    out = torch.zeros((3, w * h * spp), device="cuda")
    assert L.pg_render_pass(tree._h, C.byref(prm), out.data_ptr(), None, None, None, None) == -1
    assert "pg_scene_set first" in L.pg_last_error(tree._h).decode()
    torch.cuda.synchronize()
    assert not bool(out.any())
    ws._uploaded_to = None
    again = g.sample(ws, IndependentSampler(spp, 7))[0]
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    wb._upload(tree)                                         # memory is back: the bigger scene goes through
    assert wb._uploaded_to is tree


def test_reserve_then_pass_with_a_small_jump_table_budget_and_with_refused_allocations(monkeypatch):
    """pg_render_reserve takes the PASS BUFFERS first and the jump tables' buffer only afterwards, never as
    an error.  (a) With a 1 MiB budget ($PGSD_JUMP_TABLE_MAX_BYTES) a film of 2^20 lanes reserves, renders and refines; the
    tables get the resolution that budget allows and the radiance equals the default budget's, bit for bit.  (b) A refused
    allocation inside the reservation's own part (the table) changes nothing; a refused allocation of a pass buffer is
    PG_ERR_NOMEM and the next call, with memory back, succeeds.  (c) $PGSD_JUMP_TABLE_RESERVE=0 switches the reservation off."""
    import torch
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene
    from practical_path_guiding_lab_amd.scene import cornell_box

    L = N.lib()
    w = h = 256
    depth, spp = 4, 16          # 2^20 lanes per pass: the size from which the reservation is made
    sc = cornell_box(w, h, depth, 8)
    bmin, bmax = sc.bbox_min - np.float32(1e-4), sc.bbox_max + np.float32(1e-4)

    def run(env):
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        g = PathGuidingIntegrator({"max_depth": depth, "rr_depth": 8})
        for k_ in env:
            monkeypatch.delenv(k_)
        g.setup(w * h, bmin, bmax, 20, 20, True, 0.5)
        ws = WavefrontScene(sc)
        ws.reserve(g, spp)
        out = []
        for k in range(3):
            g.setIteration(k, False)
            out.append(g.sample(ws, IndependentSampler(spp, 10 + k))[0].clone())
            g.refineAndPrepareSDTreeForNextIteration()
        st = g.sdTree.stats()
        return out, (int(st.jump_bits), int(st.bytes_jump_tables), int(st.n_trees)), g, ws

    ref, (bits0, bytes0, trees0), g0, _ = run({})
    small, (bits1, bytes1, trees1), _, _ = run({"PGSD_JUMP_TABLE_MAX_BYTES": str(1 << 20)})
    assert trees0 == trees1 and trees0 >= 8 and bytes1 <= (1 << 20) and bits1 < bits0 == 6
    for x, y in zip(ref, small):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    off, (bits2, _, _), _, _ = run({"PGSD_JUMP_TABLE_RESERVE": "0"})
    assert bits2 == bits0 and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ref, off))
    # (b) refused allocations under pg_render_reserve: a bigger pass than anything allocated so far
    tree = g0.sdTree
    lanes = w * h * spp * 2
    assert L.pg_debug_fail_alloc(0) == 0
    rc = L.pg_render_reserve(tree._h, lanes)
    assert rc == -3 and L.pg_debug_fail_alloc_pending() == 0, L.pg_last_error(tree._h)     # a pass buffer: a hard error
    assert L.pg_render_reserve(tree._h, lanes) == 0                                         # memory is back: fine
    # ... and of the table itself: a context whose pass buffers exist (reserved with the reservation switched off) and whose table
    # does not yet -- the one allocation the call still makes is refused, and the call succeeds all the same
    monkeypatch.setenv("PGSD_JUMP_TABLE_RESERVE", "0")
    g1 = PathGuidingIntegrator({"max_depth": depth, "rr_depth": 8})
    g1.setup(w * h, bmin, bmax, 20, 20, True, 0.5)
    w1 = WavefrontScene(sc)
    w1.reserve(g1, spp)
    monkeypatch.delenv("PGSD_JUMP_TABLE_RESERVE")
    assert L.pg_debug_fail_alloc(0) == 0
    assert L.pg_render_reserve(g1.sdTree._h, w * h * spp) == 0 and L.pg_debug_fail_alloc_pending() == 0
    assert L.pg_render_reserve(g1.sdTree._h, w * h * spp) == 0
    g1.setIteration(0, False)
    assert torch.equal(g1.sample(w1, IndependentSampler(spp, 10))[0].view(torch.int32), ref[0].view(torch.int32))
    L.pg_debug_fail_alloc(-1)


def test_the_probe_build_renders_the_same_image_and_stamps_its_phases(tmp_path):
    """The probe build (csrc/Makefile `probe`, -DPG_SHADE_PHASES=1: libpgsd_phases.so, what bench.py runs for
    roofline.value_region_sdtree_*) is the product's code plus stamps: in a process of its own ($PGSD_LIBRARY) a guided
    veach-ajar pass gives the ORACLE's radiance bit for bit, with the stamps on (pg_enable_depth_counters(2)) and off, and
    pg_read_shade_phases reports one wave count and seven non-empty phases.
    The product build has no stamps: compiled_in false, zeros."""
    import json
    import os
    import subprocess
    import sys
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd.sdtree import SDTree

    t = SDTree(0)
    t.setup([0, 0, 0], [1, 1, 1], 16, 4, 20, 20, True, 0.5)
    t.enableDepthCounters(2)
    assert t.readShadePhases() == (False, 0, [0] * 7)       # the product: nothing compiled in, nothing counted
    t.enableDepthCounters(False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    probe = os.path.join(os.path.dirname(N.LIB_PATH), "libpgsd_phases.so")
    assert os.path.exists(probe), "make -C practical_path_guiding_lab_amd/csrc probe (__graft_entry__.build() does)"
    code = r'''
import json, sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from oracle import pg_oracle as po
from practical_path_guiding_lab_amd import _native as N
from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene
from practical_path_guiding_lab_amd.scene import veach_ajar
assert N.LIB_PATH.endswith("libpgsd_phases.so")
sa = veach_ajar(64, 36)
amin, amax = sa.bbox_min - np.float32(1e-4), sa.bbox_max + np.float32(1e-4)
ao = po.OracleSDTreePair(); ao.setup(amin, amax, 20, 20, True)
ag = PathGuidingIntegrator({"max_depth": 13, "rr_depth": 8}); ag.setup(64 * 36, amin, amax, 20, 20, True, 0.5)
wa = WavefrontScene(sa)
same, phases = True, None
for k in range(4):
    ag.setIteration(k, False)
    ag.sdTree.enableDepthCounters(2 if k >= 2 else 0)      # guided iterations with the stamps on
    Lo, _ = po.render_pass(ao, sa, sa.camera, 13, 8, k, False, 90 + k, 4, True, 0.5)
    Lg = ag.sample(wa, IndependentSampler(4, 90 + k))[0].cpu().numpy()
    same = same and bool((Lg.view(np.uint32) == Lo.view(np.uint32)).all())
    ao.refine_and_prepare(k); ag.refineAndPrepareSDTreeForNextIteration()
phases = ag.sdTree.readShadePhases()
print(json.dumps({"same": same, "phases": phases}))
''' % (root, os.path.join(root, "tests"))
    env = dict(os.environ, PGSD_LIBRARY=probe)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["same"] is True
    compiled, waves, cyc = out["phases"]
    assert compiled is True and waves > 0
    assert all(c > 0 for c in cyc)                                                                # seven phases, every one passed
    assert 0.05 < cyc[4] / sum(cyc) < 0.6                                                         # the SD-tree calls: a share, not everything
