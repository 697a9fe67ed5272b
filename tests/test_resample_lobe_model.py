"""tests/resample_lobe_model.py -- pg_resample_lobe (include/ext/guiding/pg_resample_lobe.h) restated in numpy float32 -- held
to answers that are known without it, and the call's ABI.  No GPU; fixed seeds; seconds.

Known answers (1 ulp = 2^-23, the spacing of fp32 above 1):
  * specular = 0: b is the clamped cosine, so every candidate's t and s are pg_resample.h's formulas of its direction, bit for
    bit -- q being the tree's pdf of that direction -- whatever the roughness and the viewer are.
  * the isotropic single-leaf tree with M = 1: W = fl(fl(t / s) / t), two roundings, so W * s is within 2 ulp of 1 on every lane
    that kept its candidate -- glossy lanes included.
  * a viewer below the surface (wil.z <= 0) never draws a GGX candidate, yet every lobe candidate consumes its three draws: with
    alpha = 1 the stream advances by exactly 5 draws per candidate (xi; xi2, u1, u2; zeta), below and above the surface alike.
  * every kind of invalid lane gets the "nothing kept" outputs, zeros in its candidate slots, and its stream is not touched.
Unbiasedness: on resample_model.horizon_lobe_tree(), normal +z, wi = (0.6, 0, 0.8), alpha 0.5, delta 0.1, seed 1234, 2^16 lanes,
for (roughness, specular) in {(0.1, 0.7), (0.02, 1), (0.5, 0.3)} and M in {1, 4, 16} the mean of f(dir) * W, f = 4 pi q b, lies
within five standard errors (of the model's own sample) of a float64 midpoint quadrature of f on 2048 x 2048 cells of the
equal-area square, which uses no sampling code (resample_lobe_model.truth_by_quadrature).  The same check REJECTS the two wrong
weights of resample_model -- W without 1 / M and W = 1 / s_kept -- at M = 4 and M = 16.
What it buys: the sample variance at M = 16 is below that at M = 1 (the order only; profiles/resample_lobe/variance.txt has the
ratios, and those against pg_resample_cosine's model on the same f, written by `python tests/resample_lobe_model.py`)."""
import ctypes
import functools
import glob
import os
import re

import numpy as np
import pytest

import abi_table
import resample_lobe_model as rl
import resample_model as rs
from abi_table import native  # noqa: F401  (the fixture)
from oracle import pg_oracle as po

F = np.float32
ULP = 2.0 ** -23
N_KNOWN = 4099


def _vertices(n, seed):
    """positions in the box, unit-ish normals and viewers all over the sphere, roughness in [1e-3, 1], specular in [0, 1]"""
    import synth
    u = synth.uniform(n, seed + 3)[0].astype(F)
    v = synth.uniform(n, seed + 4)[0].astype(F)
    rough = np.maximum(u * u, rl.MIN_ROUGHNESS).astype(F)
    return (synth.positions_uniform(n, seed, rs.BB0, rs.BB1), synth.directions_uniform(n, seed + 1), synth.directions_uniform(n, seed + 2),
            rough, v)


@pytest.fixture(scope="module")
def lobe_tree():
    return rs.horizon_lobe_tree()


@functools.lru_cache(maxsize=None)
def _truth(roughness, specular):
    return rl.truth_by_quadrature(rs.horizon_lobe_tree(), roughness, specular, grid=2048)


@functools.lru_cache(maxsize=None)
def _estimates(roughness, specular, M, weight=rs.weight_of_the_header, cosine_only=False):
    """computed once, shared, read-only"""
    e = rl.product_estimates(rs.horizon_lobe_tree(), roughness, specular, M, weight=weight, cosine_only=cosine_only)
    e.setflags(write=False)
    return e


# ---- known answers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,delta", [(0.5, 0.1), (1.0, 0.0), (0.25, 1.0)])
def test_without_a_specular_part_the_target_and_source_are_the_cosine_calls(lobe_tree, alpha, delta):
    p, nrm, wi, rough, _ = _vertices(N_KNOWN, 51)
    st, inc = po.rng_seed(N_KNOWN, 61)
    M = 3
    r = rl.resample(lobe_tree, p, nrm, wi, rough, np.zeros(N_KNOWN, F), st, inc, M, alpha, delta, candidates=True, kinds=True)
    assert not np.isin(r["kind"], (rl.GGX, rl.GGX_FAILED)).any()
    a, dl = F(alpha), F(delta)
    om, d4, omd = F(1) - a, dl * rs.INV_4PI, F(1) - dl
    for k in range(M):
        w = r["cand_dir"][k]
        q = lobe_tree.pdf(p, np.ascontiguousarray(w))
        d = (nrm[0] * w[0] + nrm[1] * w[1]) + nrm[2] * w[2]
        c = np.where(d > 0, d * rs.INV_PI, F(0)).astype(F)
        np.testing.assert_array_equal((a * c + om * q).view(np.uint32), r["cand_source"][k].view(np.uint32))
        np.testing.assert_array_equal((c * (d4 + omd * q)).view(np.uint32), r["cand_target"][k].view(np.uint32))
    assert (r["index"] != rs.NONE).sum() > N_KNOWN // 4


@pytest.mark.parametrize("alpha,delta", [(0.5, 0.1), (1.0, 1.0), (0.0, 0.0)])
def test_isotropic_tree_with_one_candidate_is_the_one_sample_mixture(alpha, delta):
    tree = rs.single_leaf_tree()
    p, nrm, wi, rough, spec = _vertices(N_KNOWN, 52)
    st, inc = po.rng_seed(N_KNOWN, 62)
    r = rl.resample(tree, p, nrm, wi, rough, spec, st, inc, 1, alpha, delta, kinds=True)
    kept = r["index"] != rs.NONE
    assert kept.sum() > N_KNOWN // 8 and (r["index"][kept] == 0).all()
    if alpha > 0:
        assert (r["kind"][0][kept] == rl.GGX).sum() > 100          # glossy candidates were kept too
    err = np.abs(r["weight"][kept].astype(np.float64) * r["source"][kept].astype(np.float64) - 1)
    print("M = 1, alpha %g delta %g: max |W s - 1| = %.3f ulp on %d lanes" % (alpha, delta, err.max() / ULP, kept.sum()))
    assert (err <= 2 * ULP).all()
    assert (r["weight"][~kept] == 0).all() and (r["target"][~kept] == 0).all() and (r["source"][~kept] == 0).all()
    assert (r["dir"][:, ~kept] == np.array([[0], [0], [-1]], F)).all()


def test_a_viewer_below_the_surface_draws_no_ggx_candidate_but_its_three_draws(lobe_tree):
    n, M = 1024, 5
    p, nrm = rs.fixed_vertex(n)
    wi = np.tile(np.array([[0.6], [0.0], [-0.8]], F), (1, n))
    wi[2, n // 2:] = F(0.8)                                      # the second half looks from above
    wi[2, 0] = F(0.0)                                            # on the horizon: wil.z > 0 fails
    st, inc = po.rng_seed(n, 63)
    ref = st.copy()
    r = rl.resample(lobe_tree, p, nrm, wi, np.full(n, 0.2, F), np.ones(n, F), st, inc, M, 1.0, 0.1, kinds=True)
    below = wi[2] <= 0
    assert (r["kind"][:, below] == rl.COSINE).all()
    assert np.isin(r["kind"][:, ~below], (rl.GGX, rl.GGX_FAILED)).all() and (r["kind"][:, ~below] == rl.GGX).any()
    for _ in range(M * 5):                                       # xi; xi2, u1, u2; zeta
        po.rng_next_f32(ref, inc)
    np.testing.assert_array_equal(st, ref)


def test_invalid_lanes_are_left_alone(lobe_tree):
    n = 257
    p, nrm, wi, rough, spec = _vertices(n, 55)
    nrm, wi, rough, spec = nrm.copy(), wi.copy(), rough.copy(), spec.copy()
    nrm[0, 3], nrm[1, 4], nrm[2, 5] = np.nan, np.inf, -np.inf
    wi[0, 13], wi[1, 14], wi[2, 15] = np.nan, np.inf, -np.inf
    rough[[23, 24, 25, 26]] = [0.0, 5e-4, 1.5, np.nan]
    spec[[33, 34, 35]] = [-0.1, 1.5, np.nan]
    rough[[43, 44]], spec[[45, 46]] = [1e-3, 1.0], [0.0, 1.0]    # the ends of the ranges are valid
    act = np.ones(n, np.uint8)
    act[50::3] = 0
    bad = [3, 4, 5, 13, 14, 15, 23, 24, 25, 26, 33, 34, 35]
    st, inc = po.rng_seed(n, 65)
    st0 = st.copy()
    r = rl.resample(lobe_tree, p, nrm, wi, rough, spec, st, inc, 4, 0.5, 0.1, active=act, candidates=True)
    off = np.zeros(n, bool)
    off[bad] = True
    off |= act == 0
    assert not off[[43, 44, 45, 46]].any()
    assert (st[off] == st0[off]).all() and (st[~off] != st0[~off]).all()
    assert (r["index"][off] == rs.NONE).all() and (r["weight"][off] == 0).all() and (r["target"][off] == 0).all()
    assert (r["source"][off] == 0).all() and (r["dir"][:, off] == np.array([[0], [0], [-1]], F)).all()
    assert (r["cand_dir"][:, :, off] == 0).all() and (r["cand_target"][:, off] == 0).all() and (r["cand_source"][:, off] == 0).all()
    assert (r["index"][~off] != rs.NONE).sum() > 50


# ---- unbiasedness, and two wrong weights rejected -----------------------------------------------------------------------------
def _check_unbiased(roughness, specular, M, weight):
    """raises AssertionError unless the mean is the quadrature's within five standard errors"""
    truth = _truth(roughness, specular)
    est = _estimates(roughness, specular, M, weight)
    mean, se = est.mean(), est.std(ddof=1) / np.sqrt(est.shape[0])
    print("roughness %g specular %g M = %2d  %-28s mean %.6f  truth %.6f  standard error %.6f  (%.2f of them off)"
          % (roughness, specular, M, weight.__name__, mean, truth, se, abs(mean - truth) / se))
    assert abs(mean - truth) <= 5 * se, (roughness, specular, M, weight.__name__, mean, truth, se)


@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("roughness,specular", rl.SETTINGS)
def test_the_estimator_is_unbiased(roughness, specular, M):
    assert roughness >= 0.02                                     # (below, a 2048 x 2048 quadrature is no truth)
    _check_unbiased(roughness, specular, M, rs.weight_of_the_header)


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("roughness,specular", rl.SETTINGS)
@pytest.mark.parametrize("wrong", [rs.weight_without_one_over_m, rs.weight_one_over_source], ids=lambda f: f.__name__)
def test_a_wrong_weight_is_rejected(wrong, roughness, specular, M):
    with pytest.raises(AssertionError):
        _check_unbiased(roughness, specular, M, wrong)


@pytest.mark.parametrize("roughness,specular", rl.SETTINGS)
def test_more_candidates_lower_the_variance_of_the_product(roughness, specular):
    v1 = _estimates(roughness, specular, 1).var(ddof=1)
    v16 = _estimates(roughness, specular, 16).var(ddof=1)
    c16 = _estimates(roughness, specular, 16, cosine_only=True).var(ddof=1)
    print("roughness %g specular %g, f = 4 pi q b: variance %.6f at M = 1, %.6f at M = 16 (ratio %.4f); the cosine-only source at "
          "M = 16: %.6f (%.2f times as much)" % (roughness, specular, v1, v16, v16 / v1, c16, c16 / v16))
    assert v16 < v1


# ---- the ABI: the headers of SURFACE_MORE, the table and the two builds name the same calls ------------------------------------
HEADER = "ext/guiding/pg_resample_lobe.h"
NAME = "pg_resample_lobe"
TABLES = ("SURFACE", "SURFACE_EXTRA", "SURFACE_EXT", "SURFACE_MORE")


def test_headers_table_and_libraries_agree(native):  # noqa: F811
    assert HEADER in native.SURFACE_MORE and NAME in native.SURFACE_MORE[HEADER] and NAME in native.EXPORTS_MORE
    assert native.EXPORTS_MORE == tuple(n for calls in native.SURFACE_MORE.values() for n in calls)
    product, probe, L = abi_table.product_library(native), abi_table.probe_library(native), native.lib()
    for header, calls in native.SURFACE_MORE.items():            # (whatever headers the table holds by now: every one of them)
        assert os.path.exists(os.path.join(abi_table.INCLUDE, *header.split("/"))), header
        declared = abi_table.declarations(header)
        assert declared == [(n, len(a)) for n, a in calls.items()], header
        for name, n_params in declared:
            assert hasattr(product, name) and hasattr(probe, name), name
            fn = getattr(L, name)
            assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_params, name
    assert abi_table.declarations(HEADER) == [(NAME, 5)]
    fn = L.pg_resample_lobe
    assert fn.argtypes[2]._type_ is native.pg_resample_params and fn.argtypes[3]._type_ is native.pg_resample_lobe_args
    assert '#include "../../pg_resample.h"' in abi_table.header_text(HEADER)


def test_no_call_is_in_two_tables_and_every_header_in_one(native):  # noqa: F811
    names = [n for t in TABLES for calls in getattr(native, t).values() for n in calls]
    assert len(names) == len(set(names))
    headers = [h for t in TABLES for h in getattr(native, t)]
    assert len(headers) == len(set(headers))
    on_disk = sorted(os.path.relpath(f, abi_table.INCLUDE).replace(os.sep, "/")
                     for f in glob.glob(os.path.join(abi_table.INCLUDE, "**", "*.h"), recursive=True))
    assert on_disk == sorted(headers)
    # the table comes last: bound after the other three, hashed after them
    assert len(native.source_hash()) == 16
    saved = dict(native.SURFACE_MORE)
    with_it = native.source_hash()
    try:
        native.SURFACE_MORE.clear()
        without = native.source_hash()
    finally:
        native.SURFACE_MORE.update(saved)
    assert with_it != without and native.source_hash() == with_it


def test_the_build_sees_the_header(native):  # noqa: F811
    mk = open(os.path.join(native.CSRC, "Makefile")).read()
    assert re.search(r"^HDRS = .*\$\(wildcard \.\./\.\./include/\*/\*/\*\.h\) \$\(wildcard \.\./\.\./include/\*/\*\.h\) "
                     r"\$\(wildcard \.\./\.\./include/pg_\*\.h\) \$\(wildcard \.\./\.\./include/pgsd\*\.h\)$", mk, flags=re.M)
    assert "pg_kernels_resample_lobe.hip" in re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()


def test_struct_layout_and_constant(native):  # noqa: F811
    assert ctypes.sizeof(native.pg_resample_lobe_args) == 16 * 8
    text = re.sub(r"/\*.*?\*/", "", abi_table.header_text(HEADER), flags=re.S)
    body = re.search(r"typedef struct pg_resample_lobe_args \{(.*?)\} pg_resample_lobe_args;", text, flags=re.S).group(1)
    names = re.findall(r"\*\s*([a-z_]+)\s*[,;]", body)
    assert names == [f[0] for f in native.pg_resample_lobe_args._fields_]
    assert names == ["p", "normal", "wi", "roughness", "specular", "active", "rng_state", "rng_inc", "dir_out", "weight_out", "target_out",
                     "source_out", "index_out", "cand_dir_out", "cand_target_out", "cand_source_out"]
    assert all(f[1] is ctypes.c_void_p for f in native.pg_resample_lobe_args._fields_)
    assert "typedef struct pg_resample_params" not in text and "#define PG_RESAMPLE_NONE" not in text     # reused, not restated
    assert "#define PG_RESAMPLE_LOBE_MIN_ROUGHNESS 1e-3f" in text
    assert F(native.PG_RESAMPLE_LOBE_MIN_ROUGHNESS) == rl.MIN_ROUGHNESS == F(1e-3)


def test_the_pinned_surfaces_are_untouched(native):  # noqa: F811
    assert tuple(native.SURFACE) == abi_table.HEADERS and sum(len(v) for v in native.SURFACE.values()) == abi_table.TOTAL == 89
    assert list(native.SURFACE_EXTRA) == ["pg_resample.h"] and list(native.SURFACE_EXTRA["pg_resample.h"]) == ["pg_resample_cosine"]
    assert list(native.SURFACE_EXT) == ["ext/pg_lights.h"] and len(native.SURFACE_EXT["ext/pg_lights.h"]) == 9
    assert native.ABI_VERSION == abi_table.ABI_VERSION == 6


def test_the_header_says_what_is_not_built_and_what_b_is():
    text = " ".join(abi_table.header_text(HEADER).split())
    assert "NOT BUILT" in text
    for what in ("Beckmann", "anisotropy", "transmission", "warp form", "learned fraction", "pg_render_pass", "compacted lane lists"):
        assert what in text.split("NOT BUILT", 1)[1], what
    assert "unbiased for every f that vanishes where b does" in text and "integrates to LESS than 1" in text
