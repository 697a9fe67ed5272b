"""Sample warping without a GPU: the exports of include/pgsd_warp.h, the numpy model of its semantics (tests/warp_model.py) checked
against itself -- the preimages of the leaves tile the unit square, the warp fills them in proportion to their area, their area
is the pdf, the inverse undoes the warp -- and the resource lines of the new kernels.

The float64 model (the same code in float64) is the reference of every tolerance that is not derived here."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import synth
from abi_table import native  # noqa: F401  (the fixture)
from warp_model import WarpModel, with_dead_quadtree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "practical_path_guiding_lab_amd", "csrc")
BB0, BB1 = [0.0] * 3, [100.0] * 3
EPS = 2.0 ** -24  # fp32: relative error of one rounded operation


@pytest.fixture(scope="module")
def trees():
    bal = synth.build_balanced(3, 4)
    return {"balanced": bal, "skewed": synth.build_skewed(4096, 4).prev, "dead": with_dead_quadtree(bal, 0)}


@pytest.fixture(scope="module")
def models(trees):
    return {k: (WarpModel(t), WarpModel(t, np.float64)) for k, t in trees.items()}


def test_the_library_exports_the_warp_entry_points(native):
    # (what every header shares -- the library, the probe build, the counts, the ABI version: tests/test_abi.py)
    hdr = open(os.path.join(ROOT, "include", "pgsd_warp.h")).read()
    declared = set(re.findall(r"^int\s*(pg_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert declared == set(native.EXPORTS_WARP) == {"pg_sample_warp", "pg_invert_warp", "pg_guide_bounce_warp"}
    assert "#ifndef PGSD_WARP_H" in hdr and '#include "pgsd.h"' in hdr
    L = native.lib()
    assert len(L.pg_sample_warp.argtypes) == 8 and len(L.pg_invert_warp.argtypes) == 8 and len(L.pg_guide_bounce_warp.argtypes) == 13
    # a NULL context is refused before anything touches a device
    assert L.pg_sample_warp(None, 1, None, None, None, None, None, None) == -1
    assert L.pg_invert_warp(None, 1, None, None, None, None, None, None) == -1
    assert L.pg_guide_bounce_warp(None, 1, None, None, None, None, None, None, None, None, None, None, None) == -1


def _leaf_rectangles(m, root):
    leaves = m.leaves_of(root)
    r = m._inverse(np.full(leaves.shape[0], root, np.int64), m.leaf_centres(leaves))
    assert (r["node"] == leaves).all()   # the walk by geometry ends in the leaf whose centre it was given
    return leaves, r


@pytest.mark.parametrize("which", ["balanced", "skewed", "dead"])
def test_the_preimages_of_the_leaves_tile_the_unit_square(models, which):
    """Over all leaves of a quadtree the areas bx * by of the inverse's rectangles sum to 1.  The float64 model's sum is 1 to
    float64 rounding (asserted: one 2^-53 per leaf and level, the roundings that went into it); the float32 sum may miss 1 by twice
    what the float32 and float64 sums of the same tree differ by, the largest such difference over the trees of the forest.
    With the float64 sum pinned to 1 that float32 assertion can hardly fail -- the tree with the worst sum sets the tolerance
    all are held to; the check that bites is the float64 one.  The float32 sums are therefore also held to a bound of their
    own: one 2^-24 per leaf and level.  Measured: float32 sums within 1.2e-7 of 1, float64 within 1.2e-16."""
    m32, m64 = models[which]
    sums = []
    for root in m32.roots:
        _, r32 = _leaf_rectangles(m32, root)
        _, r64 = _leaf_rectangles(m64, root)
        s32 = float(np.sum((r32["bx"] * r32["by"]).astype(np.float32), dtype=np.float32))
        s64 = float(np.sum(r64["bx"] * r64["by"]))
        assert abs(s64 - 1.0) <= 2.0 ** -53 * r64["bx"].shape[0] * max(int(r64["levels"].max()), 1), (root, s64)
        assert abs(s32 - 1.0) <= EPS * r32["bx"].shape[0] * max(int(r32["levels"].max()), 1), (root, s32)
        sums.append((s32, s64))
    tol = 2.0 * max(abs(a - b) for a, b in sums)
    print("%s: %d quadtrees, max |sum32 - 1| = %.3g, tolerance %.3g" % (which, len(sums), max(abs(a - 1) for a, _ in sums), tol))
    for s32, _ in sums:
        assert abs(s32 - 1.0) <= tol, (s32, tol)


@pytest.mark.parametrize("which", ["balanced", "skewed", "dead"])
def test_the_warp_fills_every_leaf_in_proportion_to_its_preimage(models, which):
    """Forward against inverse, two code paths: a regular G x G grid of u (cell centres, G = 256) goes through the warp, which walks
    by node index; every leaf must receive G^2 bx by points, bx x by the rectangle the inverse -- a walk by geometry from the
    leaf's centre -- names as its preimage, to within G (bx + by) + 1: an interval of length b holds between G b - 1 and G b + 1
    points of a grid of spacing 1 / G, so an axis-aligned rectangle holds (G bx + dx)(G by + dy) with |dx|, |dy| <= 1.  A leaf of
    zero probability (bx by = 0) may therefore catch no more than the points of one grid line, and catches none when its
    rectangle is a point."""
    m32, _ = models[which]
    G = 256
    g = ((np.arange(G, dtype=np.float32) + np.float32(0.5)) / np.float32(G)).astype(np.float32)   # exact
    u = np.stack([np.tile(g, G), np.repeat(g, G)])
    worst = 0.0
    for root in m32.roots:
        _, node, _ = m32._forward(np.full(G * G, root, np.int64), u)
        leaves, r = _leaf_rectangles(m32, root)
        count = np.bincount(node, minlength=m32.leaf.shape[0])[leaves]
        assert count.sum() == G * G    # every point ended in a leaf of this quadtree
        bx, by = r["bx"].astype(np.float64), r["by"].astype(np.float64)
        miss = np.abs(count - G * G * bx * by)
        bound = G * (bx + by) + 1
        worst = max(worst, float((miss / bound).max()))
        assert (miss <= bound).all(), (root, leaves[miss > bound], count[miss > bound], (G * G * bx * by)[miss > bound])
        assert (count[(bx == 0) & (by == 0)] == 0).all()
    print("%s: largest |count - G^2 bx by| / bound = %.3f" % (which, worst))


def _queries(n, seed):
    return synth.positions_uniform(n, seed, BB0, BB1), synth.directions_uniform(n, seed + 1)


@pytest.mark.parametrize("which", ["balanced", "skewed", "dead"])
def test_the_area_of_a_preimage_is_the_pdf(models, trees, which):
    """Density: for every lane bx * by / s^2 (fp32, in this order) against 4 pi * pdf, pdf the oracle's KDTree.pdf.  Node values are
    not exactly the fp32 sum of their children's, and 1 - P carries P's rounding error relative to a small 1 - P, so the two are
    not equal; the relative tolerance is the largest difference between the float32 and the float64 model's value over the same
    lanes, doubled.  Measured (20 000 lanes): balanced tree 9.88e-6 between the models and 9.86e-6 against the pdf; skewed tree
    (8 levels, improbable leaves) 2.076e-4 and 2.077e-4.  Where the preimage is empty the pdf is exactly 0, and the reverse
    (in a quadtree that has energy)."""
    m32, m64 = models[which]
    n = 20000
    p, d = _queries(n, 40)
    root = m32.root_of(p)
    c = m32.dir_to_canonical(d)
    r32, r64 = m32._inverse(root, c), m64._inverse(root, c.astype(np.float64))
    a32 = ((r32["bx"] * r32["by"]).astype(np.float32) / (r32["s"] * r32["s"]).astype(np.float32)).astype(np.float64)
    a64 = r64["bx"] * r64["by"] / (r64["s"] * r64["s"])
    pdf = trees[which].pdf(p, d).astype(np.float64) * 4.0 * np.pi
    # a quadtree without energy: the warp falls back to uniform at every level (its preimages are the cells themselves), the
    # pdf is 0 all the same -- pdfQuadTree's 0/0.  Those lanes are checked for exactly that and left out below.
    dead = m32.irr[root] == 0
    assert dead.any() == (which == "dead")
    assert (pdf[dead] == 0).all() and (a32[dead] == 1).all()
    a32, a64, pdf = a32[~dead], a64[~dead], pdf[~dead]
    zero = a64 == 0
    assert ((pdf == 0) == zero).all() and (a32[zero] == 0).all()
    tol = 2.0 * float((np.abs(a32 - a64)[~zero] / a64[~zero]).max())
    rel = np.abs(a32 - pdf)[~zero] / a64[~zero]
    print("%s: models differ by %.4g (relative), model against pdf %.4g, tolerance %.4g" % (which, tol / 2, rel.max(), tol))
    assert (rel <= tol).all(), (rel.max(), tol)


# the constants of the round trip's tolerance: measured against the float64 model (0.752 and 2.105), doubled (see the test)
RT_A, RT_B = 1.504, 4.21


def test_the_inverse_undoes_the_warp(models):
    """Round trip u -> dir -> u' on synth.build_balanced(3, 4), per lane and axis:

        |u' - u'_64| <= 2^-24 * (A * levels + B * b * max(p, s) / s)

    u'_64 the float64 model's round trip of the same u (it returns u to 1e-15), levels / s / b the depth, cell size and preimage
    extent (on that axis) of the leaf, p the canonical coordinate.  The error is NOT uniform: the warp quantises the position
    inside the leaf to fp32 (x0 + u s and the trip through the direction err by a few 2^-24 of max(p, s), and by a few 2^-24
    outright), and the inverse stretches a leaf of size s over a preimage of extent b, so a small, probable leaf (b / s large)
    returns u' with an error b / s times larger.

    A and B are set from the float64 model as reference, doubled.  Their proportion, 10 : 28, comes from counting roundings
    (below); their size from the measurement: with A = 10, B = 28 the largest error / bound over the 20 000 lanes is 0.0752 (x;
    0.0475 on y), so the measured constants are A = 0.752, B = 2.105, and the test asserts twice that, A = 1.504, B = 4.21
    (largest error / bound 0.50 on x, 0.32 on y; largest error 3.6e-7 in u; float64 round trip 5.6e-16; no lane changed leaf).
    The counting: both directions compute Py and Pl by the same fp32 operations, so only the roundings of the other
    operations count, each at most 2^-24 relative (e below):
      per level (10): the warp's u - P, 1 - P and division, 3 e of a v <= 1, and its clamp to ONE_M, 1 e; pulled back to u
        they scale by the extent of that level's preimage, <= 1.  The inverse's b * P and a + b P, 2 e absolute, and
        b * (1 - P), 2 e relative to b; its two final operations where levels >= 1.
      the position (28, for a tree whose cells are no smaller than 2^-4): u * s and x0 + u s, 2 e max(p, s); y through the
        direction, 2 y - 1 and (z + 1) / 2, 0.5 e + e p; x through the direction, 2 pi x, sin / cos, their products with
        sin(theta), atan2, the wrap and the division, e (3 p + 0.32) -- the parts not proportional to p are covered by
        max(p, s) >= 2^-4: 2 + 1.5 * 16 = 26 for y, 5 + 0.32 * 16 = 10.2 for x; c - x0, 1 e s.  Divided by s, times b.
    levels, s and b are those of the leaf the inverse answered from.
    Lanes whose position has y = 0 exactly are left out (the pole: the direction holds no x), there are none among these."""
    m32, m64 = models["balanced"]
    n = 20000
    p = synth.positions_uniform(n, 50, BB0, BB1)
    u = synth.uniform(n, 51, 2)
    root = m32.root_of(p)
    c, node, _ = m32._forward(root, u)
    d = m32.canonical_to_dir(c)
    np.testing.assert_array_equal(d.view(np.uint32), m32.sample_warp(p, u)[0].view(np.uint32))
    u_back, r = m32.invert_canonical(root, m32.dir_to_canonical(d))
    d64, _ = m64.sample_warp(p, u.astype(np.float64))
    u64, _ = m64.invert_warp(p, d64)
    assert np.abs(u64 - u).max() < 1e-13
    assert (c >= 0).all() and (c <= 1).all() and (u_back >= 0).all() and (u_back < 1).all()   # no point left the square
    use = c[1] != 0
    s, levels = r["s"].astype(np.float64), r["levels"]
    for axis, key in ((0, "bx"), (1, "by")):
        b = r[key].astype(np.float64)
        tol = EPS * (RT_A * levels + RT_B * b * np.maximum(c[axis], s) / s)
        err = np.abs(u_back[axis].astype(np.float64) - u64[axis])
        print("axis %d: largest error %.3g, largest error / bound %.3f, leaves changed %d"
              % (axis, err[use].max(), (err / tol)[use].max(), int((r["node"] != node).sum())))
        assert (err <= tol)[use].all(), (axis, (err / tol)[use].max())


def test_the_warp_kernels_keep_eight_waves_and_no_scratch():
    """pg_kernels_query.hip's header says why: occupancy is what hides the dependent gathers of a walk."""
    f = os.path.join(CSRC, "pg_kernels_warp.remarks")
    if not os.path.exists(f):
        subprocess.run(["make", "-C", CSRC, "-j4"], check=True, capture_output=True)
    kernels, cur = {}, None
    for line in open(f, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    assert len(kernels) == 3 and all("warp" in k for k in kernels), sorted(kernels)
    for k, v in kernels.items():
        assert v["occupancy"] >= 8 and v["scratch"] == 0, (k, v)
    assert len(glob.glob(os.path.join(CSRC, "*.remarks"))) >= 12
