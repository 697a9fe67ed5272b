"""The joint form's first launch (pg_render_stages 0) makes the camera rays and walks their closest hits inside k_wave_shade
itself -- no k_wave_trace ahead of it, no ray / sampler / hit round trip through device memory.  The shapes at which that can
go wrong and the separate launch could not: lane counts that leave dead lanes at the workgroup barriers, a wave-pipeline scene without a BVH, the level-3 kernel, passes whose
first launch is also their last bounce, striped shards, batched seeds, the second buffer set -- all against the CPU oracle,
bit for bit (radiance, valid flags, per-pixel sums, every accumulator limb and KD count, the refined trees) -- and the
joint form against the split one."""
import numpy as np
import pytest

from oracle import pg_oracle as po
from test_gpu_render import _same_tree, mixed_scene

pytestmark = pytest.mark.gpu


def _box(sc):
    return sc.bbox_min - np.float32(1e-4), sc.bbox_max + np.float32(1e-4)


def _same_accumulators(g, o):
    kd, lo, hi = g.sdTree.exportAccumulators()
    np.testing.assert_array_equal(kd, o.current.kd_column("count"))
    np.testing.assert_array_equal(lo, o.current.quad_column("acc_lo"))
    np.testing.assert_array_equal(hi, o.current.quad_column("acc_hi"))


class _Pair:
    """The oracle and the device integrator side by side on one scene, with their per-pixel sums."""

    def __init__(self, sc, nee=True, **ws_kwargs):
        from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
        from practical_path_guiding_lab_amd.render import WavefrontScene
        self.sc, self.nee = sc, nee
        self.npix = sc.camera.width * sc.camera.height
        bmin, bmax = _box(sc)
        self.o = po.OracleSDTreePair()
        self.o.setup(bmin, bmax, 20, 20, nee)
        self.o_sumL = np.zeros((3, self.npix), np.float32)
        self.o_sumL2 = np.zeros((3, self.npix), np.float32)
        self.g = PathGuidingIntegrator({"max_depth": sc.max_depth, "rr_depth": sc.rr_depth})
        self.g.setup(self.npix, bmin, bmax, sdTreeMaxDepth=20, quadTreeMaxDepth=20, isStoreNEERadiance=nee, bsdfSamplingFraction=0.5)
        self.ws = WavefrontScene(sc, **ws_kwargs)
        self.k = 0

    def begin(self, k, final=False):
        self.k, self.final = k, final
        self.g.setIteration(k, final)

    def oracle_pass(self, seed, spp):
        sc = self.sc
        return po.render_pass(self.o, sc, sc.camera, sc.max_depth, sc.rr_depth, self.k, self.final, seed, spp, self.nee, 0.5,
                              self.o_sumL, self.o_sumL2)

    def both(self, seed, spp):
        """one pass on each side: radiance and valid flags equal"""
        from practical_path_guiding_lab_amd.render import IndependentSampler
        Lo, vo = self.oracle_pass(seed, spp)
        Lg, vg, _ = self.g.sample(self.ws, IndependentSampler(spp, seed))
        np.testing.assert_array_equal(Lg.cpu().numpy().view(np.uint32), Lo.view(np.uint32))
        np.testing.assert_array_equal(vg.cpu().numpy(), vo)

    def same_state(self):
        assert np.isfinite(self.o_sumL).all() and self.o_sumL.max() > 0
        np.testing.assert_array_equal(self.g.sumL.cpu().numpy().view(np.uint32), self.o_sumL.view(np.uint32))
        np.testing.assert_array_equal(self.g.sumL2.cpu().numpy().view(np.uint32), self.o_sumL2.view(np.uint32))
        _same_accumulators(self.g, self.o)

    def refine(self):
        self.o.refine_and_prepare(self.k)
        self.g.refineAndPrepareSDTreeForNextIteration()
        _same_tree(self.o.prev.export(), self.g.sdTree.export())


def _lifecycle(sc, spp, passes=2, seed=4100, **ws_kwargs):
    """iterations 0-2 (unguided, unguided, guided: both kernels' instantiations run), each refined, then one final pass that
    records nothing"""
    p = _Pair(sc, **ws_kwargs)
    for k in range(4):
        p.begin(k, final=k == 3)
        for _ in range(1 if k == 3 else passes):
            p.both(seed, spp)
            seed += spp
        p.same_state()
        if k < 3:
            p.refine()
    return p


@pytest.mark.parametrize("w,h,spp", [(50, 30, 1), (10, 7, 3)])
def test_dead_lanes_reach_every_barrier(w, h, spp):
    """Lane counts that are no multiple of the workgroup: 1 500 lanes are five full workgroups and one whose waves hold 64, 64,
    64 and 28 live lanes; 210 lanes are one workgroup with a partly dead wave.  Dead lanes make no ray and walk nothing, but
    stage the KD planes and the BVH's top and take part in the append."""
    from practical_path_guiding_lab_amd.scene import veach_ajar
    assert (w * h * spp) % 256 != 0
    _lifecycle(veach_ajar(w, h), spp)


def test_wave_pipeline_scene_without_a_bvh():
    """cornell-box through the split pipeline: quads only, no BVH table (a null pointer) -- the camera walk inside the shading
    kernel stages nothing and walks nothing, like the shadow ray's."""
    from practical_path_guiding_lab_amd.scene import cornell_box
    _lifecycle(cornell_box(24, 24, 4, 8), 2, split_pipeline=True)


@pytest.mark.parametrize("spp", [1, 5])
def test_level_3_first_launch(spp):
    """the mixed scene (dielectrics, delta lobes, one-sided surfaces, meshes beside quads, spheres and boxes): k_wave_shade_l3<true>"""
    _lifecycle(mixed_scene(24), spp)


@pytest.mark.parametrize("max_depth", [1, 2])
def test_first_launch_is_also_the_last_bounce(max_depth):
    """max_depth 1: the only launch of the pass walks the camera rays, shades, and appends nothing; 2: one append, one bounce more"""
    _lifecycle(mixed_scene(16, max_depth=max_depth, rr_depth=3), 2)


@pytest.fixture(scope="module")
def trained_ajar_64():
    """veach-ajar 64x36 after iterations 0 and 1, in iteration 2 (guided, recording): the pair, and the seed to go on with"""
    from practical_path_guiding_lab_amd.scene import veach_ajar
    p = _Pair(veach_ajar(64, 36))
    seed = 7000
    for k in range(2):
        p.begin(k)
        for _ in range(2):
            p.both(seed, 2)
            seed += 2
        p.same_state()
        p.refine()
    p.begin(2)
    return p, seed


def test_striped_shards_equal_the_oracles_pass_restricted(trained_ajar_64):
    """36 rows in 4-row bands over 3 ranks (uneven: three bands each): the camera ray is made from the lane's GLOBAL pixel.  Every
    shard's radiance and flags are the oracle's pass at that shard's pixels; the three shards' accumulators and sums add up to
    the oracle's."""
    import torch
    from practical_path_guiding_lab_amd.render import IndependentSampler
    p, seed = trained_ajar_64
    spp = 2
    Lo, vo = p.oracle_pass(seed, spp)
    seen = np.zeros(p.npix, bool)
    try:
        for r in range(3):
            p.ws.set_shard(r, 3, 4)
            px = p.ws.local_pixels()
            seen[px] = True
            lanes = (px[:, None] * spp + np.arange(spp)[None, :]).reshape(-1)
            Lg, vg, _ = p.g.sample(p.ws, IndependentSampler(spp, seed))
            np.testing.assert_array_equal(Lg.cpu().numpy().view(np.uint32), np.ascontiguousarray(Lo[:, lanes]).view(np.uint32))
            np.testing.assert_array_equal(vg.cpu().numpy(), vo[lanes])
    finally:
        p.ws.set_shard(0, 1)
    assert seen.all()
    torch.cuda.synchronize()
    p.same_state()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_batched_seeds_on_one_and_two_buffer_sets(in_flight):
    """IndependentSampler(16, seed, batched=True) is the oracle's 16 one-sample passes: the lane's stream is (seed + s, pixel).
    in_flight 2: two such passes on alternating buffer sets (each set's first launch fills nothing the other reads)."""
    import torch
    from practical_path_guiding_lab_amd.render import IndependentSampler
    from practical_path_guiding_lab_amd.scene import veach_ajar
    B = 16
    p = _Pair(veach_ajar(32, 18), in_flight=in_flight)
    seed = 300
    for k in range(3):
        p.begin(k)
        outs = []
        for _ in range(2):
            outs.append((seed, p.g.sample(p.ws, IndependentSampler(B, seed, batched=True))))
            seed += B
        p.ws.join()
        torch.cuda.synchronize()
        for s0, (Lg, vg, _) in outs:
            Lg = Lg.cpu().numpy().reshape(3, p.npix, B)
            vg = vg.cpu().numpy().reshape(p.npix, B)
            for s in range(B):
                Lo, vo = p.oracle_pass(s0 + s, 1)
                np.testing.assert_array_equal(np.ascontiguousarray(Lg[:, :, s]).view(np.uint32), Lo.view(np.uint32))
                np.testing.assert_array_equal(vg[:, s], vo)
        p.same_state()
        p.refine()


def _device_run(sc, spp=2, **ws_kwargs):
    """three iterations on the device alone -> everything they leave, and the last pass's live counts"""
    import torch
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene
    bmin, bmax = _box(sc)
    g = PathGuidingIntegrator({"max_depth": sc.max_depth, "rr_depth": sc.rr_depth})
    g.setup(sc.camera.width * sc.camera.height, bmin, bmax, 20, 20, True, 0.5)
    ws = WavefrontScene(sc, **ws_kwargs)
    out, seed = [], 910
    for k in range(3):
        g.setIteration(k, False)
        for _ in range(2):
            L, v, _ = g.sample(ws, IndependentSampler(spp, seed))
            seed += spp
            out += [L.cpu().numpy().view(np.uint32), v.cpu().numpy()]
        torch.cuda.synchronize()
        out.append([int(x) for x in g.sdTree.renderLiveCounts(sc.max_depth)])
        out += [np.asarray(x) for x in g.sdTree.exportAccumulators()]
        out += [g.sumL.cpu().numpy().view(np.uint32), g.sumL2.cpu().numpy().view(np.uint32)]
        g.refineAndPrepareSDTreeForNextIteration()
    return out


def _same_runs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, list):
            assert x == y
        else:
            np.testing.assert_array_equal(x, y)


def test_joint_form_equals_split_form():
    """stages 0 (the camera bounce inside k_wave_shade) and stages 2 (k_wave_trace<., true>
    as ever): the same radiance, flags, live counts, accumulators and sums -- a cross-check on top of the oracle's"""
    from practical_path_guiding_lab_amd.scene import veach_ajar
    sc = veach_ajar(64, 36)
    _same_runs(_device_run(sc, stages=0), _device_run(sc, stages=2))
