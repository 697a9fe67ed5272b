"""tests/resample_interface_model.py -- pg_resample_interface (include/ext/guiding/pg_resample_interface.h) restated in numpy
float32 -- held to answers that are known without it, and the call's ABI.  No GPU; fixed seeds; seconds.

Known answers (1 ulp = 2^-23, the spacing of fp32 above 1):
  * the isotropic single-leaf tree with M = 1: W = fl(fl(t / s) / t), two roundings, so W * s is within 2 ulp of 1 on every lane
    that kept its candidate -- viewers inside the glass and transmitted directions included.
  * a viewer exactly in the plane (wil.z == 0) keeps nothing -- b is 0 everywhere and every lobe sample fails -- yet with
    alpha = 1 its stream advances by exactly 5 draws per candidate (xi; xi2, u1, u2; zeta).
  * every kind of invalid lane gets the "nothing kept" outputs, zeros in its candidate slots, and its stream is not touched.
  * eta_out is 1 exactly when dot(dir, n) and dot(wi, n) share a sign, else eta (viewer above) or 1 / eta (below); 0 with nothing kept.
  * under total internal reflection (a viewer inside, eta 1.5, wi 60 degrees off the inner normal, roughness 1e-3) no kept
    direction crosses the surface.
Unbiasedness: on resample_model.horizon_lobe_tree(), normal +z, alpha 0.5, delta 0.1, seed 1234, 2^16 lanes, for the three
(roughness, eta, wi) of resample_interface_model.SETTINGS and M in {1, 4, 16} the mean of f(dir) * W, f = 4 pi q b, lies within
five standard errors (of the model's own sample) of a float64 midpoint quadrature of f over the WHOLE sphere on 2048 x 2048
cells of the equal-area square, which uses no sampling code; the quadrature on 1024 x 1024 cells differs from it by less than
a fifth of the smallest of those standard errors (the third setting's roughness is 0.07 for that: at 0.05 the coarse grid is
0.8 of a standard error off).  The same check REJECTS the two wrong weights of resample_model at M = 4 and M = 16.
What it buys: the sample variance at M = 16 is below that at M = 1; and pg_resample_lobe's model with specular = 1 on the same
inputs and the same f is biased LOW beyond the bound at every setting (it never keeps a direction across the surface) --
profiles/resample_interface/variance.txt, written by `python tests/resample_interface_model.py`.

What the unbiasedness check found while the call was built: a lobe sample that its microfacet reflected THROUGH the
macro-surface (or refracted back) lands where b holds only the other branch's density; kept as candidates, such samples put the
mean 4.3 and 8.3 standard errors high at M = 4 and 16 of the second setting.  They fail (the header's side test)."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import abi_table
import resample_interface_model as ri
import resample_model as rs
from abi_table import native  # noqa: F401  (the fixture)
from oracle import pg_oracle as po

F = np.float32
ULP = 2.0 ** -23
N_KNOWN = 4099
ETAS = np.array([1.49 / 1.000277, 1.0 / 1.5, 2.419, 0.25, 4.0], F)


def _vertices(n, seed):
    """positions in the box, unit-ish normals and viewers all over the sphere (either side), roughness in [1e-3, 1], five etas"""
    import synth
    u = synth.uniform(n, seed + 3)[0].astype(F)
    rough = np.maximum(u * u, ri.MIN_ROUGHNESS).astype(F)
    return (synth.positions_uniform(n, seed, rs.BB0, rs.BB1), synth.directions_uniform(n, seed + 1), synth.directions_uniform(n, seed + 2),
            rough, ETAS[np.arange(n) % ETAS.shape[0]])


@pytest.fixture(scope="module")
def lobe_tree():
    return rs.horizon_lobe_tree()


@functools.lru_cache(maxsize=None)
def _truth(setting, grid=2048):
    return ri.truth_by_quadrature(rs.horizon_lobe_tree(), *setting, grid=grid)


@functools.lru_cache(maxsize=None)
def _estimates(setting, M, weight=rs.weight_of_the_header, reflection_lobe=False):
    """computed once, shared, read-only"""
    e = ri.product_estimates(rs.horizon_lobe_tree(), *setting, M, weight=weight, reflection_lobe=reflection_lobe)
    e.setflags(write=False)
    return e


def _dot(a, b):
    return (a[0].astype(np.float64) * b[0] + a[1].astype(np.float64) * b[1]) + a[2].astype(np.float64) * b[2]


# ---- known answers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,delta", [(0.5, 0.1), (1.0, 1.0), (0.0, 0.0)])
def test_isotropic_tree_with_one_candidate_is_the_one_sample_mixture(alpha, delta):
    tree = rs.single_leaf_tree()
    p, nrm, wi, rough, eta = _vertices(N_KNOWN, 52)
    st, inc = po.rng_seed(N_KNOWN, 62)
    r = ri.resample(tree, p, nrm, wi, rough, eta, st, inc, 1, alpha, delta, kinds=True)
    kept = r["index"] != rs.NONE
    assert kept.sum() > N_KNOWN // 8 and (r["index"][kept] == 0).all()
    inside = _dot(wi, nrm) < 0
    crossed = _dot(r["dir"], nrm) * _dot(wi, nrm) < 0
    assert (kept & inside).sum() > 100 and (kept & crossed).sum() > 100            # viewers inside the glass count too
    if alpha > 0:
        assert (r["kind"][0][kept] == ri.LOBE).sum() > 100 and (r["kind"][0][kept & crossed] == ri.LOBE).sum() > 50
    err = np.abs(r["weight"][kept].astype(np.float64) * r["source"][kept].astype(np.float64) - 1)
    print("M = 1, alpha %g delta %g: max |W s - 1| = %.3f ulp on %d lanes" % (alpha, delta, err.max() / ULP, kept.sum()))
    assert (err <= 2 * ULP).all()
    assert (r["weight"][~kept] == 0).all() and (r["target"][~kept] == 0).all() and (r["source"][~kept] == 0).all()
    assert (r["eta"][~kept] == 0).all() and (r["dir"][:, ~kept] == np.array([[0], [0], [-1]], F)).all()


def test_a_viewer_in_the_plane_keeps_nothing_and_draws_five_per_lobe_candidate(lobe_tree):
    n, M = 1024, 5
    p, nrm = rs.fixed_vertex(n)
    wi = np.tile(np.array([[0.6], [0.8], [0.0]], F), (1, n))
    wi[2, n // 2:] = F(-0.8)                                     # the second half looks from inside
    st, inc = po.rng_seed(n, 63)
    ref = st.copy()
    r = ri.resample(lobe_tree, p, nrm, wi, np.full(n, 0.2, F), np.full(n, 1.5, F), st, inc, M, 1.0, 0.1, kinds=True, candidates=True)
    flat = wi[2] == 0
    assert (r["kind"][:, flat] == ri.LOBE_FAILED).all() and (r["index"][flat] == rs.NONE).all() and (r["weight"][flat] == 0).all()
    assert (r["eta"][flat] == 0).all() and (r["cand_dir"][:, :, flat] == 0).all() and (r["cand_target"][:, flat] == 0).all()
    assert (r["kind"][:, ~flat] == ri.LOBE).any() and (r["index"][~flat] != rs.NONE).sum() > n // 4
    for _ in range(M * 5):                                       # xi; xi2, u1, u2; zeta
        po.rng_next_f32(ref, inc)
    np.testing.assert_array_equal(st, ref)
    # ... and with tree candidates too nothing is kept in the plane: b is 0 for every direction
    st, inc = po.rng_seed(n, 64)
    r = ri.resample(lobe_tree, p, nrm, wi, np.full(n, 0.2, F), np.full(n, 1.5, F), st, inc, M, 0.5, 0.1)
    assert (r["index"][flat] == rs.NONE).all()


def test_invalid_lanes_are_left_alone(lobe_tree):
    n = 257
    p, nrm, wi, rough, eta = _vertices(n, 55)
    nrm, wi, rough, eta = nrm.copy(), wi.copy(), rough.copy(), eta.copy()
    nrm[0, 3], nrm[1, 4], nrm[2, 5] = np.nan, np.inf, -np.inf
    wi[0, 13], wi[1, 14], wi[2, 15] = np.nan, np.inf, -np.inf
    rough[[23, 24, 25, 26]] = [0.0, 5e-4, 1.5, np.nan]
    eta[[33, 34, 35, 36, 37, 38, 39]] = [0.0, 0.2, 1.0, 4.5, -1.5, np.nan, np.inf]
    rough[[43, 44]], eta[[45, 46]] = [1e-3, 1.0], [0.25, 4.0]    # the ends of the ranges are valid
    act = np.ones(n, np.uint8)
    act[50::3] = 0
    bad = [3, 4, 5, 13, 14, 15, 23, 24, 25, 26, 33, 34, 35, 36, 37, 38, 39]
    st, inc = po.rng_seed(n, 65)
    st0 = st.copy()
    r = ri.resample(lobe_tree, p, nrm, wi, rough, eta, st, inc, 4, 0.5, 0.1, active=act, candidates=True)
    off = np.zeros(n, bool)
    off[bad] = True
    off |= act == 0
    assert not off[[43, 44, 45, 46]].any()
    assert (st[off] == st0[off]).all() and (st[~off] != st0[~off]).all()
    assert (r["index"][off] == rs.NONE).all() and (r["weight"][off] == 0).all() and (r["target"][off] == 0).all()
    assert (r["source"][off] == 0).all() and (r["eta"][off] == 0).all() and (r["dir"][:, off] == np.array([[0], [0], [-1]], F)).all()
    assert (r["cand_dir"][:, :, off] == 0).all() and (r["cand_target"][:, off] == 0).all() and (r["cand_source"][:, off] == 0).all()
    assert (r["index"][~off] != rs.NONE).sum() > 50


@pytest.mark.parametrize("M", [1, 6])
def test_eta_out_is_one_exactly_on_the_viewers_side(lobe_tree, M):
    p, nrm, wi, rough, eta = _vertices(N_KNOWN, 57)
    st, inc = po.rng_seed(N_KNOWN, 67)
    r = ri.resample(lobe_tree, p, nrm, wi, rough, eta, st, inc, M, 0.5, 0.1)
    kept = r["index"] != rs.NONE
    # (fp32, the header's dot3: the sign of a float64 dot product could differ for a direction in the plane)
    dn = (r["dir"][0] * nrm[0] + r["dir"][1] * nrm[1]) + r["dir"][2] * nrm[2]
    vn = (wi[0] * nrm[0] + wi[1] * nrm[1]) + wi[2] * nrm[2]
    same = dn * vn > 0
    assert (kept & same).sum() > 500 and (kept & ~same).sum() > 500
    assert (r["eta"][kept & same] == 1).all()
    enters = np.where(vn > 0, eta, F(1) / eta).astype(F)
    np.testing.assert_array_equal(r["eta"][kept & ~same], enters[kept & ~same])
    assert (r["eta"][kept & ~same] != 1).all() and (r["eta"][~kept] == 0).all()


def test_under_total_internal_reflection_no_kept_direction_crosses(lobe_tree):
    n = 2048
    p, nrm = rs.fixed_vertex(n)
    s, c = math.sin(math.radians(60)), math.cos(math.radians(60))       # past the critical angle asin(1 / 1.5) = 41.8 degrees
    wi = np.tile(np.array([[s], [0.0], [-c]], F), (1, n))
    for alpha in (1.0, 0.5):
        st, inc = po.rng_seed(n, 68)
        r = ri.resample(lobe_tree, p, nrm, wi, np.full(n, 1e-3, F), np.full(n, 1.5, F), st, inc, 8, alpha, 0.1, candidates=True, kinds=True)
        kept = r["index"] != rs.NONE
        assert kept.sum() > (n // 2 if alpha == 1.0 else 10)
        assert (r["dir"][2, kept] < 0).all() and (r["eta"][kept] == 1).all()
        # no lobe candidate crosses: F = 1 at every microfacet the viewer can see, the transmitted share is 0.  (The tree proposes
        # far-side directions, whose half vector is a steeply tilted microfacet: D leaves them next to nothing, not exactly 0.)
        far = r["cand_dir"][:, 2] > 0
        assert far.any() or alpha == 1.0
        lobe = r["kind"] == ri.LOBE
        assert lobe.any() and (r["cand_dir"][:, 2][lobe] < 0).all()


# ---- unbiasedness, and two wrong weights rejected -----------------------------------------------------------------------------
def _check_unbiased(setting, M, weight, reflection_lobe=False):
    """raises AssertionError unless the mean is the quadrature's within five standard errors"""
    truth = _truth(setting)
    est = _estimates(setting, M, weight, reflection_lobe)
    mean, se = est.mean(), est.std(ddof=1) / np.sqrt(est.shape[0])
    print("roughness %g eta %g wi %s M = %2d  %-28s%s mean %.6f  truth %.6f  standard error %.6f  (%.2f of them off)"
          % (*setting, M, weight.__name__, " (pg_resample_lobe's model)" if reflection_lobe else "", mean, truth, se, abs(mean - truth) / se))
    assert abs(mean - truth) <= 5 * se, (setting, M, weight.__name__, mean, truth, se)


@pytest.mark.parametrize("setting", ri.SETTINGS)
def test_the_quadrature_is_converged(setting):
    fine, coarse = _truth(setting), _truth(setting, 1024)
    se = min(_estimates(setting, M).std(ddof=1) / np.sqrt(ri.N_LANES) for M in (1, 4, 16))
    print("roughness %g eta %g wi %s: 2048^2 %.8f, 1024^2 %.8f, apart by %.4f of the smallest standard error %.6f"
          % (*setting, fine, coarse, abs(fine - coarse) / se, se))
    assert abs(fine - coarse) < se / 5


@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("setting", ri.SETTINGS)
def test_the_estimator_is_unbiased(setting, M):
    _check_unbiased(setting, M, rs.weight_of_the_header)


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("setting", ri.SETTINGS)
@pytest.mark.parametrize("wrong", [rs.weight_without_one_over_m, rs.weight_one_over_source], ids=lambda f: f.__name__)
def test_a_wrong_weight_is_rejected(wrong, setting, M):
    with pytest.raises(AssertionError):
        _check_unbiased(setting, M, wrong)


@pytest.mark.parametrize("setting", ri.SETTINGS)
def test_more_candidates_lower_the_variance_of_the_product(setting):
    v1, v16 = _estimates(setting, 1).var(ddof=1), _estimates(setting, 16).var(ddof=1)
    print("roughness %g eta %g wi %s, f = 4 pi q b: variance %.6f at M = 1, %.6f at M = 16 (ratio %.4f)" % (*setting, v1, v16, v16 / v1))
    assert v16 < v1


@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("setting", ri.SETTINGS)
def test_the_reflection_lobe_is_biased_low_or_noisier_on_this_product(setting, M):
    """the case for the call: pg_resample_lobe's model, specular = 1, the same inputs, the same f"""
    est, ref = _estimates(setting, M), _estimates(setting, M, reflection_lobe=True)
    verdict = ri.verdict_on_the_reflection_lobe(est, ref, _truth(setting))
    print("roughness %g eta %g wi %s M = %2d: pg_resample_lobe's model: mean %.6f against %.6f, variance %.6f against %.6f: %s"
          % (*setting, M, ref.mean(), _truth(setting), ref.var(ddof=1), est.var(ddof=1), verdict))
    assert verdict in ("biased low", "larger variance")
    if verdict == "biased low":
        with pytest.raises(AssertionError):
            _check_unbiased(setting, M, rs.weight_of_the_header, reflection_lobe=True)


def test_the_float64_lobe_is_the_oracles_pdf():
    """lobe_f64, written from the header alone, against the oracle's rough dielectric on directions all over the sphere"""
    import synth
    n = 4096
    wl = synth.directions_uniform(n, 71)
    for roughness, eta, wi in ri.SETTINGS:
        wil = np.tile(np.array(wi, F)[:, None], (1, n))
        b32 = ri.interface_density(np.full(n, roughness, F), np.full(n, eta, F), wil, wl)
        b64 = ri.lobe_f64(wl.astype(np.float64), np.array(wi, F).astype(np.float64), roughness, eta)
        # fp32 against float64: some forty roundings of 2^-24 each in a chain of products and quotients -- 1e-5 of b -- and the
        # cancellation of 1 - F next to the critical angle, a few ulp of 1 times the lobe's height -- 1e-6 of its peak
        assert (b64 > 1e-6).sum() > n // 8
        assert (np.abs(b32 - b64) <= 1e-5 * b64 + 1e-6 * b64.max()).all(), (roughness, eta, wi)


# ---- the ABI: the header, the table and the two builds name the same call -----------------------------------------------------
HEADER = "ext/guiding/pg_resample_interface.h"
NAME = "pg_resample_interface"
FIELDS = ["p", "normal", "wi", "roughness", "eta", "active", "rng_state", "rng_inc", "dir_out", "weight_out", "target_out", "source_out",
          "index_out", "eta_out", "cand_dir_out", "cand_target_out", "cand_source_out"]


def test_header_table_and_libraries_agree(native):  # noqa: F811
    assert os.path.exists(os.path.join(abi_table.INCLUDE, *HEADER.split("/")))
    assert HEADER in native.SURFACE_MORE and list(native.SURFACE_MORE[HEADER]) == [NAME] and NAME in native.EXPORTS_MORE
    assert abi_table.declarations(HEADER) == [(NAME, 5)]
    product, probe, L = abi_table.product_library(native), abi_table.probe_library(native), native.lib()
    assert hasattr(product, NAME) and hasattr(probe, NAME)
    fn = L.pg_resample_interface
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 5
    assert fn.argtypes[2]._type_ is native.pg_resample_params and fn.argtypes[3]._type_ is native.pg_resample_interface_args
    assert '#include "../../pg_resample.h"' in abi_table.header_text(HEADER)
    assert native.ABI_VERSION == abi_table.ABI_VERSION == 6
    mk = open(os.path.join(native.CSRC, "Makefile")).read()
    assert "pg_kernels_resample_interface.hip" in re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()


def test_struct_layout_and_constants(native):  # noqa: F811
    assert ctypes.sizeof(native.pg_resample_interface_args) == 17 * 8
    text = re.sub(r"/\*.*?\*/", "", abi_table.header_text(HEADER), flags=re.S)
    body = re.search(r"typedef struct pg_resample_interface_args \{(.*?)\} pg_resample_interface_args;", text, flags=re.S).group(1)
    names = re.findall(r"\*\s*([a-z_]+)\s*[,;]", body)
    assert names == [f[0] for f in native.pg_resample_interface_args._fields_] == FIELDS
    assert all(f[1] is ctypes.c_void_p for f in native.pg_resample_interface_args._fields_)
    # reused, not restated
    assert "typedef struct pg_resample_params" not in text and "#define PG_RESAMPLE_NONE" not in text
    assert "#define PG_RESAMPLE_LOBE_MIN_ROUGHNESS" not in text
    assert "#define PG_RESAMPLE_INTERFACE_MIN_ROUGHNESS 1e-3f" in text
    assert "#define PG_RESAMPLE_INTERFACE_MIN_ETA 0.25f" in text and "#define PG_RESAMPLE_INTERFACE_MAX_ETA 4.0f" in text
    assert F(native.PG_RESAMPLE_INTERFACE_MIN_ROUGHNESS) == ri.MIN_ROUGHNESS == F(1e-3)
    assert (native.PG_RESAMPLE_INTERFACE_MIN_ETA, native.PG_RESAMPLE_INTERFACE_MAX_ETA) == (ri.MIN_ETA, ri.MAX_ETA) == (0.25, 4.0)


def test_the_header_says_what_is_not_built_and_what_b_is():
    text = " ".join(abi_table.header_text(HEADER).split())
    assert "NOT BUILT" in text
    for what in ("Beckmann", "anisotropy", "diffuse share", "warp form", "learned fraction", "pg_render_pass", "compacted lane lists"):
        assert what in text.split("NOT BUILT", 1)[1], what
    assert "transmission" not in text.split("NOT BUILT", 1)[1]
    assert "unbiased for every f that vanishes where b does" in text and "integrates to LESS than 1" in text
    assert "the density the lobe candidates are drawn with" in text and "wil.z == 0" in text
    for what in ("roughness, eta, rng_state", "candidates outside 1..64", "reserved != 0", "n > 2^32 - 1"):
        assert what in text.split("REFUSALS", 1)[1], what
