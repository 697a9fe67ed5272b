"""The device's ray casting by itself (pg_scene_intersect: intersect<> of csrc/pg_render_dev.hpp in the three forms the
render kernels give its walk) against the CPU oracle's (pgo_intersect) bit for bit, on ray sets aimed at what a render
pass meets only by chance -- edges, vertices, surface origins, axis-parallel directions, origins on BVH box planes, walks
whose stacks spill into the overflow strip, finite tmax at the hit itself -- and against the float64 model of
tests/raycast_model.py directly, so that a change moving oracle and device together still fails a test."""
import functools

import numpy as np
import pytest

import probe_harness as H
import raycast_model as RM
import test_raycast_model as TM

pytestmark = pytest.mark.gpu

SCENES = ("veach-ajar", "torus", "mixed", "cornell-box", "veach-mis")
BIG = 262_147   # more than 2^18 rays: 1025 workgroups, the last one of three rays
SIZES = (1, 63, 64, 65, 257, BIG)


def cast(name, o, d, tmax=None, any_hit=False, form=0):
    ws = H.scene(TM.scene, name)
    t, prim, uv = ws.intersect(H.set_scene(ws), H.dev(o), H.dev(d), None if tmax is None else H.dev(np.asarray(tmax, np.float32)), any_hit, form)
    uv = uv.cpu().numpy()
    return t.cpu().numpy(), prim.cpu().numpy(), uv[:, 0].copy(), uv[:, 1].copy()


@functools.lru_cache(maxsize=None)
def pool(name):
    """BIG rays of the scene from every generator that applies to it, shuffled (so that every prefix holds all kinds), and
    the oracle's answers: made once, shared, never changed"""
    from oracle import pg_oracle as po
    T = TM.tables(name)
    sets = list(RM.MESH_SETS) if T.tris.shape[0] else ["uniform", "axis"]
    per = BIG // len(sets) + 1
    o, d = zip(*[RM.MESH_SETS[k](T, per, 77 + i) for i, k in enumerate(sets)])
    order = np.random.default_rng(5).permutation(per * len(sets))[:BIG]
    o, d = np.concatenate(o)[order], np.concatenate(d)[order]
    return o, d, po.intersect(TM.scene(name), o, d)


def _same(dev, ora, what):
    """(t, prim, u, v) of the device and of the oracle: every bit, a NaN's included"""
    columns = lambda r: dict(zip(("t", "prim", "u", "v"), r))
    H.same_bits(columns(dev), columns(ora), ("prim",), ("t", "u", "v"), what, any_nan=False)


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("name", SCENES)
def test_device_equals_oracle(name, form):
    o, d, ora = pool(name)
    assert (ora[1] >= 0).mean() > 0.3
    for n in SIZES:
        _same(cast(name, o[:n], d[:n], form=form), H.first(ora, n), "%s form %d n %d" % (name, form, n))


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("name", SCENES + ("lattice",))
def test_tmax_is_strict(name, form):
    """tmax = the closest hit's own t must not report that hit, nor does one float below; under all three limits the device
    says what the oracle says.  One float ABOVE reports that very hit or nothing, never anything else -- "nothing" because
    the limit enters the box tests, whose padding (3.4 ulp) covers their own rounding and not the triangle test's: a t that
    Moeller-Trumbore rounded further down than that below the distance at which the ray enters the triangle's box is cut
    off with its box (met on 8-26 of 20 000 rays here, at triangle borders, where the chord through the box is shortest; the
    renderer's shadow rays keep 1e-3 relative clearance).  On the lattice no operation of the triangle test rounds and the
    box distances are off by three roundings at most, which the padding covers: there every hit must be reported."""
    from oracle import pg_oracle as po
    if name == "lattice":
        o, d, _ = TM.lattice_rays()
        ora = po.intersect(TM.scene(name), o, d)
    else:
        o, d, ora = pool(name)
    hit = np.nonzero(ora[1][:20000] >= 0)[0]
    o, d, t0, p0 = o[hit], d[hit], ora[0][hit], ora[1][hit]
    for tmax, above in ((t0, False), (np.nextafter(t0, np.float32(np.inf)), True), (np.nextafter(t0, np.float32(0)), False)):
        dev = cast(name, o, d, tmax, form=form)
        _same(dev, po.intersect(TM.scene(name), o, d, tmax), "%s form %d tmax" % (name, form))
        nothing = (dev[1] < 0) & (dev[0] == tmax)
        if above:
            that_hit = (dev[1] == p0) & (dev[0] == t0)
            assert (that_hit | nothing).all()
            print("%s form %d: %d of %d hits not reported under a limit one float above them" % (name, form, nothing.sum(), hit.size))
            if name in ("lattice", "cornell-box", "veach-mis"):  # (... and without a mesh no box test sees the limit)
                assert that_hit.all()
        else:  # nothing at t0 or beyond: whatever is reported is nearer -- and the oracle found nothing nearer without the limit
            assert nothing.all()


def test_the_overflow_strip_is_met():
    """walks with more waiting entries than the LDS holds (8 in the ray-casting kernels, 6 in k_wave_shade), picked by the
    oracle's count of them"""
    from oracle import pg_oracle as po
    T = TM.tables("torus")
    o, d = RM.rays_uniform(T, 200_000, 424242)
    ora = po.intersect(TM.scene("torus"), o, d)
    w = ora[4]
    print("torus, 200 000 uniform rays, greatest number of waiting entries -> rays:", dict(zip(*np.unique(w, return_counts=True))))
    assert (w > 8).sum() >= 32 and (w > 6).sum() >= 256
    deep = w > 6
    for form in (0, 1, 2):
        _same(cast("torus", o[deep], d[deep], form=form), [a[deep] for a in ora], "overflow, form %d" % form)
    for form in (0, 1):  # ... and among all the others, where a lost entry's neighbours walk
        _same(cast("torus", o, d, form=form), ora, "all 200 000, form %d" % form)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_any_hit_is_occluded_exactly_where_the_closest_hit_finds_something(name, form):
    from oracle import pg_oracle as po
    o, d, ora = pool(name)
    n = 100_000
    o, d, t0 = o[:n], d[:n], ora[0][:n]
    rng = np.random.default_rng(9)
    # limits before, at and behind the closest hit, and none
    tmax = np.where(np.isfinite(t0) & (ora[1][:n] >= 0), t0 * rng.choice(np.array([0.25, 0.999, 1.0, 1.001, 4.0], np.float32), n), np.float32(np.inf)).astype(np.float32)
    tmax[rng.random(n) < 0.2] = np.inf
    want = po.intersect(TM.scene(name), o, d, tmax)[1] >= 0
    assert want.any() and (~want).any()
    if name == "mixed":  # rays a quad, a sphere or a box occludes although a triangle lies behind it
        T = TM.tables(name)
        first = po.intersect(TM.scene(name), o, d, tmax)[1]
        assert ((first >= 0) & (first < T.first_tri) & (ora[1][:n] >= 0)).sum() > 100
    got = cast(name, o, d, tmax, any_hit=True, form=form)[1] >= 0
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", ["veach-ajar", "mixed", "veach-mis"])
def test_non_finite_and_degenerate_rays(name):
    """NaN origins and directions, the zero direction, origins far outside: the oracle returns for them
    (tests/test_raycast_model.py checks that on the CPU) and the device's walk is bounded by its budget; both say the same"""
    from oracle import pg_oracle as po
    o, d = TM.degenerate_rays(name)
    ora = po.intersect(TM.scene(name), o, d)
    for form in (0, 1, 2):
        _same(cast(name, o, d, form=form), ora, "%s degenerate, form %d" % (name, form))
        got = cast(name, o, d, any_hit=True, form=form)[1] >= 0
        np.testing.assert_array_equal(got, ora[1] >= 0)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_exact_and_inclusive_where_float32_is_exact(form):
    """the lattice of tests/test_raycast_model.py (no operation rounds: borders, vertices and box planes by known answer)"""
    from oracle import pg_oracle as po
    o, d, inside = TM.lattice_rays()
    dev = cast("lattice", o, d, form=form)
    TM.check_lattice(*dev)
    _same(dev, po.intersect(TM.scene("lattice"), o, d), "lattice, form %d" % form)
    np.testing.assert_array_equal(cast("lattice", o, d, any_hit=True, form=form)[1] >= 0, inside)


def test_device_against_the_model():
    name = "veach-ajar"
    o, d, m = TM.model(name, "uniform")
    assert o.shape[0] == 2048
    for form in (0, 1):
        t, prim, u, v = cast(name, o, d, form=form)
        for what, idx in RM.band_failures(TM.tables(name), m, t, prim, u, v).items():
            assert idx.size == 0, "%s: rays %s" % (what, idx[:8])
        assert not RM.leaks(m, np.where(prim >= 0, t.astype(np.float64), np.inf)).any()
    assert m.ambiguous.mean() <= RM.AMBIGUOUS_CAP


def test_misuse_is_refused_with_a_message():
    import torch
    from practical_path_guiding_lab_amd import _native as N
    from practical_path_guiding_lab_amd.sdtree import SDTree
    L = N.lib()
    o, d = torch.zeros(48, dtype=torch.float32, device="cuda"), torch.ones(48, dtype=torch.float32, device="cuda")
    tm, t = torch.full((16,), float("inf"), dtype=torch.float32, device="cuda"), torch.zeros(16, dtype=torch.float32, device="cuda")
    uv, i = torch.zeros(32, dtype=torch.float32, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda")

    def refused(h, n, args, word):
        rc = L.pg_scene_intersect(h, n, *args)
        assert rc < 0 and word in L.pg_last_error(h).decode(), (rc, L.pg_last_error(h))

    good = [o.data_ptr(), d.data_ptr(), tm.data_ptr(), 0, 0, t.data_ptr(), i.data_ptr(), uv.data_ptr(), None]
    bare = SDTree(0)
    refused(bare._h, 16, good, "pg_scene_set")          # no scene
    tree = H.set_scene(H.scene(TM.scene, "cornell-box"))
    assert L.pg_scene_intersect(tree._h, 16, *good) == 0
    for k in (0, 1, 2, 5, 6, 7):
        refused(tree._h, 16, good[:k] + [None] + good[k + 1:], "NULL")
    refused(tree._h, (1 << 20) + 1, good, "2^20")
    refused(tree._h, 16, good[:4] + [3] + good[5:], "walk_form")
    assert L.pg_scene_intersect(tree._h, 0, None, None, None, 0, 0, None, None, None, None) == 0
