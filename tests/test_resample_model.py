"""tests/resample_model.py -- pg_resample_cosine (include/pg_resample.h) restated in numpy float32 -- held to answers that are
known without it, and the call's ABI.  No GPU; fixed seeds; seconds.

Known answers (bounds from the roundings counted on the header's formulas, 1 ulp = 2^-23, the spacing of fp32 above 1):
  * M = 1: W = fl(fl(t / s) / t), two roundings, so W * s is within 2 ulp of 1 on every lane that kept its candidate.
  * the isotropic single-leaf tree with alpha = 1 (cosine candidates only, q = 1 / 4 pi, s = c): every weight is
    v = delta / 4 pi + (1 - delta) q up to the roundings of t (one) and of t / s (one), W = fl(fl(wsum / M) / t_kept); for
    M = 1 and M = 4 (wsum / M exact, three additions) W * c is within 4 ulp of 1.
  * a tree without energy, alpha = 0, delta = 0: q = 0 everywhere, so s = t = 0 and nothing is kept; the stream still
    advances by every candidate's draws (1 for the choice, 3 per visited quadtree node, 1 for the reservoir).
  * alpha = 0: every candidate is the tree's; candidate 0 is OracleTree.sample taken after ONE discarded draw, and its
    source 0 * c + 1 * q is q itself.
Unbiasedness: on resample_model.horizon_lobe_tree(), normal +z, delta = 0.1, N = 2^16 lanes, M in {1, 4, 16}, the mean of
g(dir) * W is 1 within five standard errors (of the model's own sample) for g = c, the clamped cosine density, and for
g = 1 / (2 pi) on the hemisphere: both integrate to exactly 1 and vanish where n.w <= 0.  The same check REJECTS two wrong
weights -- W without 1 / M and W = 1 / s_kept -- at M = 4 and M = 16 (at M = 1 the three formulas are the same number).
What it buys: for f = 4 pi q c the sample variance at M = 16 is below that at M = 1 (the order only;
profiles/resample/variance.txt has the ratio, written by `python tests/resample_model.py`)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import abi_table
import resample_model as rs
from abi_table import native  # noqa: F401  (the fixture)
from oracle import pg_oracle as po

F = np.float32
ULP = 2.0 ** -23
N_KNOWN = 4099
N_UNBIASED = 1 << 16


def _vertices(n, seed):
    """positions in the box and unit-ish normals all over the sphere"""
    import synth
    return synth.positions_uniform(n, seed, rs.BB0, rs.BB1), synth.directions_uniform(n, seed + 1)


@pytest.fixture(scope="module")
def lobe_tree():
    return rs.horizon_lobe_tree()


# ---- known answers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,delta", [(0.5, 0.1), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.25, 0.5)])
def test_one_candidate_is_the_one_sample_mixture(lobe_tree, alpha, delta):
    p, nrm = _vertices(N_KNOWN, 11)
    st, inc = po.rng_seed(N_KNOWN, 21)
    r = rs.resample(lobe_tree, p, nrm, st, inc, 1, alpha, delta)
    kept = r["index"] != rs.NONE
    assert kept.sum() > N_KNOWN // 8 and (r["index"][kept] == 0).all()
    err = np.abs(r["weight"][kept].astype(np.float64) * r["source"][kept].astype(np.float64) - 1)
    print("M = 1, alpha %g delta %g: max |W s - 1| = %.3f ulp on %d lanes" % (alpha, delta, err.max() / ULP, kept.sum()))
    assert (err <= 2 * ULP).all()
    assert (r["weight"][~kept] == 0).all() and (r["target"][~kept] == 0).all() and (r["source"][~kept] == 0).all()
    assert (r["dir"][:, ~kept] == np.array([[0], [0], [-1]], F)).all()


@pytest.mark.parametrize("M", [1, 4])
def test_isotropic_tree_with_cosine_candidates_only(M):
    tree = rs.single_leaf_tree()
    p, nrm = _vertices(N_KNOWN, 12)
    st, inc = po.rng_seed(N_KNOWN, 22)
    r = rs.resample(tree, p, nrm, st, inc, M, 1.0, 0.1, candidates=True)
    kept = r["index"] != rs.NONE
    assert kept.sum() > N_KNOWN * 0.99                          # (a cosine candidate fails only at the horizon's rounding)
    assert (tree.pdf(p, r["dir"]).view(np.uint32) == rs.INV_4PI.view(np.uint32)).all()
    d = r["dir"].astype(np.float64)
    c = (nrm.astype(np.float64) * d).sum(axis=0) / np.pi
    # the model's own fp32 c of the kept candidate: its source (alpha = 1: s = 1 * c + 0 * q = c)
    c32 = r["source"].astype(np.float64)
    assert np.abs(c32[kept] / c[kept] - 1).max() < 1e-5
    err = np.abs(r["weight"][kept].astype(np.float64) * c32[kept] - 1)
    print("isotropic, M = %d: max |W c - 1| = %.3f ulp" % (M, err.max() / ULP))
    assert (err <= 4 * ULP).all()


def test_a_tree_without_energy_keeps_nothing_and_still_draws():
    tree = rs.dark_tree()
    M = 5
    p, nrm = _vertices(N_KNOWN, 13)
    st, inc = po.rng_seed(N_KNOWN, 23)
    ref = st.copy()
    r = rs.resample(tree, p, nrm, st, inc, M, 0.0, 0.0, candidates=True)
    assert (r["index"] == rs.NONE).all() and (r["weight"] == 0).all() and (r["target"] == 0).all() and (r["source"] == 0).all()
    assert (r["dir"] == np.array([[0], [0], [-1]], F)).all()
    assert (r["cand_target"] == 0).all() and (r["cand_source"] == 0).all()
    # per candidate: the choice, three draws at each of the three nodes a sampling walk of the two-level tree visits, the reservoir
    for _ in range(M * (1 + 3 * 3 + 1)):
        po.rng_next_f32(ref, inc)
    np.testing.assert_array_equal(st, ref)


def test_with_alpha_zero_candidate_zero_is_the_trees_sample(lobe_tree):
    p, nrm = _vertices(N_KNOWN, 14)
    st, inc = po.rng_seed(N_KNOWN, 24)
    ref = st.copy()
    r = rs.resample(lobe_tree, p, nrm, st, inc, 3, 0.0, 0.1, candidates=True)
    po.rng_next_f32(ref, inc)                                    # the draw that chose the tree
    d, pdf = lobe_tree.sample(p, ref, inc)
    np.testing.assert_array_equal(r["cand_dir"][0].view(np.uint32), d.view(np.uint32))
    np.testing.assert_array_equal(r["cand_source"][0].view(np.uint32), pdf.view(np.uint32))


def test_masked_lanes_and_bad_normals_are_left_alone(lobe_tree):
    p, nrm = _vertices(257, 15)
    nrm = nrm.copy()
    nrm[0, 3], nrm[1, 4], nrm[2, 5] = np.nan, np.inf, -np.inf
    act = np.ones(257, np.uint8)
    act[7::3] = 0
    st, inc = po.rng_seed(257, 25)
    st0 = st.copy()
    r = rs.resample(lobe_tree, p, nrm, st, inc, 4, 0.5, 0.1, active=act, candidates=True)
    off = (act == 0) | ~np.isfinite(nrm).all(axis=0)
    assert off[[3, 4, 5, 7]].all() and not off.all()
    assert (st[off] == st0[off]).all() and (st[~off] != st0[~off]).all()
    assert (r["index"][off] == rs.NONE).all() and (r["weight"][off] == 0).all()
    assert (r["cand_dir"][:, :, off] == 0).all() and (r["cand_target"][:, off] == 0).all() and (r["cand_source"][:, off] == 0).all()


# ---- unbiasedness, and two wrong weights rejected -----------------------------------------------------------------------------
def _check_unbiased(tree, M, weight):
    """raises AssertionError unless both means are 1 within five standard errors"""
    p, nrm = rs.fixed_vertex(N_UNBIASED)
    st, inc = po.rng_seed(N_UNBIASED, 31 + M)
    r = rs.resample(tree, p, nrm, st, inc, M, 0.5, 0.1, weight=weight)
    W = r["weight"].astype(np.float64)
    cos = r["dir"][2].astype(np.float64)                        # (the normal is +z)
    up = (cos > 0) & (r["index"] != rs.NONE)
    for name, g in (("cosine", np.where(up, cos / np.pi, 0.0)), ("hemisphere", np.where(up, 1 / (2 * np.pi), 0.0))):
        est = g * W
        mean, se = est.mean(), est.std(ddof=1) / np.sqrt(N_UNBIASED)
        print("M = %2d  %-28s g = %-10s mean %.5f  standard error %.5f  (%.2f of them off 1)"
              % (M, weight.__name__, name, mean, se, abs(mean - 1) / se))
        assert abs(mean - 1) <= 5 * se, (M, weight.__name__, name, mean, se)


@pytest.mark.parametrize("M", [1, 4, 16])
def test_the_estimator_is_unbiased(lobe_tree, M):
    _check_unbiased(lobe_tree, M, rs.weight_of_the_header)


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("wrong", [rs.weight_without_one_over_m, rs.weight_one_over_source], ids=lambda f: f.__name__)
def test_a_wrong_weight_is_rejected(lobe_tree, M, wrong):
    with pytest.raises(AssertionError):
        _check_unbiased(lobe_tree, M, wrong)


def test_at_one_candidate_the_three_weights_coincide(lobe_tree):
    """why the rejections above start at M = 4: (w / 1) / t = w / t, and 1 / s is the same number up to its two roundings"""
    p, nrm = rs.fixed_vertex(N_KNOWN)
    res = []
    for wt in (rs.weight_of_the_header, rs.weight_without_one_over_m, rs.weight_one_over_source):
        st, inc = po.rng_seed(N_KNOWN, 41)
        res.append(rs.resample(lobe_tree, p, nrm, st, inc, 1, 0.5, 0.1, weight=wt)["weight"])
    np.testing.assert_array_equal(res[0].view(np.uint32), res[1].view(np.uint32))
    np.testing.assert_allclose(res[0], res[2], rtol=2 * ULP, atol=0)


def test_more_candidates_lower_the_variance_of_the_product(lobe_tree):
    v1, m1 = rs.variance_of_the_product(lobe_tree, 1)
    v16, m16 = rs.variance_of_the_product(lobe_tree, 16)
    print("f = 4 pi q c: variance %.6f at M = 1 (mean %.5f), %.6f at M = 16 (mean %.5f), ratio %.4f" % (v1, m1, v16, m16, v16 / v1))
    assert v16 < v1


# ---- the ABI: header, SURFACE_EXTRA and the two builds name the same call -----------------------------------------------------
HEADER = "pg_resample.h"


def test_header_table_and_libraries_agree(native):  # noqa: F811
    declared = abi_table.declarations(HEADER)
    assert declared == [("pg_resample_cosine", 5)]
    assert [n for n, _ in declared] == re.findall(r"^(?:int|const char \*)\s*(pg_[a-z_0-9]+)\s*\(", abi_table.header_text(HEADER), flags=re.M)
    assert list(native.SURFACE_EXTRA) == [HEADER] and native.EXPORTS_RESAMPLE == ("pg_resample_cosine",)
    bound = native.SURFACE_EXTRA[HEADER]
    assert list(bound) == ["pg_resample_cosine"] and len(bound["pg_resample_cosine"]) == 5
    product, probe, L = abi_table.product_library(native), abi_table.probe_library(native), native.lib()
    assert hasattr(product, "pg_resample_cosine") and hasattr(probe, "pg_resample_cosine")
    fn = L.pg_resample_cosine
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 5
    assert fn.argtypes[2]._type_ is native.pg_resample_params and fn.argtypes[3]._type_ is native.pg_resample_args
    # the build and the source hash see the header
    mk = open(os.path.join(native.CSRC, "Makefile")).read()
    assert re.search(r"^HDRS = .*\$\(wildcard \.\./\.\./include/pg_\*\.h\) \$\(wildcard \.\./\.\./include/pgsd\*\.h\)$", mk, flags=re.M)
    assert "pg_kernels_resample.hip" in re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()


def test_struct_layouts(native):  # noqa: F811
    assert ctypes.sizeof(native.pg_resample_params) == 16
    assert [f[0] for f in native.pg_resample_params._fields_] == ["candidates", "alpha", "delta", "reserved"]
    assert ctypes.sizeof(native.pg_resample_args) == 13 * 8
    text = re.sub(r"/\*.*?\*/", "", abi_table.header_text(HEADER), flags=re.S)
    body = re.search(r"typedef struct pg_resample_args \{(.*?)\} pg_resample_args;", text, flags=re.S).group(1)
    names = re.findall(r"\*\s*([a-z_]+)\s*[,;]", body)
    assert names == [f[0] for f in native.pg_resample_args._fields_]
    assert native.PG_RESAMPLE_MAX_CANDIDATES == 64 and native.PG_RESAMPLE_NONE == rs.NONE
    assert "#define PG_RESAMPLE_MAX_CANDIDATES 64" in text and "#define PG_RESAMPLE_NONE 0xFFFFFFFFu" in text


def test_the_pinned_surface_is_untouched(native):  # noqa: F811
    assert HEADER not in native.SURFACE and tuple(native.SURFACE) == abi_table.HEADERS
    assert sum(len(v) for v in native.SURFACE.values()) == abi_table.TOTAL == 89   # (87 when this header came; pg_vertex_probe and pg_head_probe, probes of the tests in pgsd.h, since)
    assert not any("pg_resample_cosine" in v for v in native.SURFACE.values())
    assert native.ABI_VERSION == abi_table.ABI_VERSION == 6
    on_disk = sorted(os.path.basename(f) for f in glob.glob(os.path.join(abi_table.INCLUDE, "*.h")))
    assert on_disk == sorted(abi_table.HEADERS + (HEADER,))
    assert HEADER not in [os.path.basename(f) for f in glob.glob(os.path.join(abi_table.INCLUDE, "pgsd*.h"))]
