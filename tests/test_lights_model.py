"""tests/lights_model.py -- the learned light selection (include/ext/pg_lights.h) restated in numpy float32 -- held to answers
that are known without it, and the calls' ABI.  No GPU; fixed seeds.

Known answers: four lights with means 1, 1/2, 1/4 and 0 give the weights 65536, 32768, 16384 and 0 (every quotient is a power of
two: no rounding anywhere), and the pmf follows; an unlearned leaf selects uniformly; a build without counts keeps the row; `root`
takes the square root (means 1, 1/4, 1/16 -> 65536, 32768, 16384).

Self-consistency of the map: over ALL 2^24 values u = i / 2^24 (every fp32 in [0, 1) the stream can draw, and exact), the share
of u that SELECT maps to light j is within 6 * 2^-24 of PMF(j).  The bound, counted on the header: an end of a light's interval
in u is the image of an exact boundary (j / L in the uniform branch, C[j] / K in the tree branch) under the inverse of two rounded
operations ((u / delta) * L, resp. (u - delta) / (1 - delta) and the truncated product with K), each of which moves the end by
at most one step of 2^-24: two steps per end, four per interval; the pmf's own three roundings (the quotient, the two products;
the sum is of two numbers below 1) are below 2^-24 each relative to numbers below 1, two steps together.  Six.  Measured here for
ten (L, delta) pairs, L = 1 .. 1024, delta = 0 .. 1: the maximum is printed (1.9 steps on these rows).  And the tree branch
never chooses a light with k_j = 0.

Variance: on a leaf where one light in 64 carries the energy, the estimator value / pmf has a strictly lower variance with the
learned row than with the uniform choice, and its mean is the same within five standard errors (the ratio is printed)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import abi_table
import lights_model as lm
import synth
from abi_table import native  # noqa: F401  (the fixture)
from oracle import pg_oracle as po

F = np.float32
BB0, BB1 = [0.0] * 3, [100.0] * 3
STEP = 2.0 ** -24
HEADER = "ext/pg_lights.h"
CALLS = [("pg_lights_enable", 3), ("pg_lights_record", 5), ("pg_lights_build", 2), ("pg_lights_sample", 10), ("pg_lights_pmf", 7),
         ("pg_lights_accumulators", 3), ("pg_lights_status", 3), ("pg_lights_export", 5), ("pg_lights_import", 4)]


@pytest.fixture(scope="module")
def one_leaf():
    t = po.OracleTree()
    t.setup(BB0, BB1, 20, 20, True)
    return t


def _record_means(mod, means, copies=4, position=(30.0, 40.0, 50.0)):
    """`copies` records of every light j with value means[j] (lights with None get no record), all at one position"""
    lights = [j for j, v in enumerate(means) if v is not None for _ in range(copies)]
    p = np.tile(np.asarray(position, F)[:, None], (1, len(lights)))
    mod.record({"position": p, "light": np.array(lights, np.uint32), "value": np.array([means[j] for j in lights], F)})


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_four_lights_with_known_means(one_leaf):
    mod = lm.LightsModel(one_leaf, 4, delta=0.25)
    _record_means(mod, [1.0, 0.5, 0.25, 0.0])
    assert mod.acc_words()[0, :, 3].tolist() == [4, 4, 4, 4]            # the zero-valued records count
    assert mod.acc_words()[0, :, 0].tolist() == [0, 0, 0, 0] and mod.acc_words()[0, :, 1].tolist() == [4 << 8, 2 << 8, 1 << 8, 0]
    assert mod.build() == 1 and mod.learned_leaves() == 1
    assert lm.weights(mod.rows[0]).tolist() == [65536, 32768, 16384, 0]
    assert mod.rows[0].tolist() == [65536, 98304, 114688, 114688]
    p = np.tile(np.array([[10.0], [20.0], [30.0]], F), (1, 5))
    got = mod.pmf(p, np.array([0, 1, 2, 3, 4], np.uint32))
    want = [0.25 * 0.25 + 0.75 * (k / 114688.0) for k in (65536, 32768, 16384, 0)] + [0.0]
    np.testing.assert_allclose(got, want, rtol=3 * 2.0 ** -24, atol=0)
    assert got[3] == F(0.0625) and abs(float(got[:4].astype(np.float64).sum()) - 1) < 4 * STEP
    # delta = 0: light 3 has probability 0 and is never selected; delta = 1: the uniform choice
    u = (np.arange(1 << 12, dtype=np.float64) / (1 << 12)).astype(F)
    leaf = np.zeros(u.shape[0], np.int64)
    j, tree_branch = lm.select(mod.rows, leaf, u, 0.0)
    assert tree_branch.all() and set(j.tolist()) == {0, 1, 2}
    # x = floor(28 i) for u = i / 4096 (K / 4096 = 28): light 0 while 28 i < 65536, light 1 while 28 i < 98304
    np.testing.assert_array_equal(np.bincount(j, minlength=4), [2341, 1170, 585, 0])
    j, tree_branch = lm.select(mod.rows, leaf, u, 1.0)
    assert not tree_branch.any() and np.bincount(j, minlength=4).tolist() == [1 << 10] * 4
    assert (lm.pmf(mod.rows, leaf[:4], np.arange(4), 1.0) == F(0.25)).all()


def test_an_unlearned_leaf_and_positions_outside_select_uniformly(one_leaf):
    mod = lm.LightsModel(one_leaf, 5, delta=0.3)
    assert mod.learned_leaves() == 0
    u = np.array([0.0, 0.19, 0.2, 0.5, 0.99999994, 1.0, -0.0, -1.0, np.nan, np.inf, 0.4], F)
    p = np.tile(np.array([[10.0], [20.0], [30.0]], F), (1, u.shape[0]))
    light, pm = mod.sample(p, u)
    assert light.tolist() == [0, 0, 1, 2, 4, 0, 0, 0, 0, 0, 2] and (pm == F(1) / F(5)).all()
    # a learned leaf: positions outside the box and NaN positions still select uniformly
    _record_means(mod, [None, None, 3.0, None, None])
    assert mod.build() == 1
    q = p.copy()
    q[0, 1], q[1, 2], q[2, 3] = -1.0, np.nan, 100.00001
    light, pm = mod.sample(q, np.full(u.shape[0], 0.9, F))
    assert light[[1, 2, 3]].tolist() == [4, 4, 4] and (pm[[1, 2, 3]] == F(1) / F(5)).all()
    assert (np.delete(light, [1, 2, 3]) == 2).all()                       # the tree branch: the only light with a weight
    act = np.ones(u.shape[0], np.uint8)
    act[5] = 0
    light, pm = mod.sample(q, np.full(u.shape[0], 0.9, F), active=act)
    assert light[5] == lm.NONE and pm[5] == 0


def test_a_build_without_counts_keeps_the_row(one_leaf):
    mod = lm.LightsModel(one_leaf, 3)
    assert mod.build() == 0 and (mod.rows == 0).all()
    mod.load_state({"rows": np.array([[7, 7, 65543]], np.uint32)})
    assert mod.build() == 0 and mod.rows[0].tolist() == [7, 7, 65543]
    # records whose values are all zero: counts but no energy, M = 0 -- the row stays
    _record_means(mod, [0.0, 0.0, 0.0])
    assert (mod.acc_words()[0, :, 3] == 4).all() and mod.build() == 0 and mod.rows[0].tolist() == [7, 7, 65543]
    # energy arrives: the row is replaced, and a second build of the same accumulators gives it again
    _record_means(mod, [None, 2.0, None])
    assert mod.build() == 1 and mod.rows[0].tolist() == [0, 65536, 65536]
    assert mod.build() == 1 and mod.rows[0].tolist() == [0, 65536, 65536]


def test_root_takes_the_square_root(one_leaf):
    means = [1.0, 0.25, 0.0625, None]
    plain, root = lm.LightsModel(one_leaf, 4), lm.LightsModel(one_leaf, 4, root=True)
    for mod in (plain, root):
        _record_means(mod, means)
        mod.build()
    assert lm.weights(plain.rows[0]).tolist() == [65536, 16384, 4096, 0]
    assert lm.weights(root.rows[0]).tolist() == [65536, 32768, 16384, 0]


def test_the_stream_gives_u_and_masked_lanes_keep_theirs(one_leaf):
    mod = lm.LightsModel(one_leaf, 7, delta=0.5)
    n = 257
    p = synth.positions_uniform(n, 3, BB0, BB1)
    act = (np.arange(n) % 3 != 0).astype(np.uint8)
    st, inc = po.rng_seed(n, 9)
    st0, ref = st.copy(), st.copy()
    u = po.rng_next_f32(ref, inc)
    light, pm = mod.sample(p, None, st, inc, active=act)
    assert (st[act == 0] == st0[act == 0]).all() and (st[act != 0] == ref[act != 0]).all()
    want, _ = mod.sample(p, u)
    assert (light[act != 0] == want[act != 0]).all() and (light[act == 0] == lm.NONE).all()


# ---- the map agrees with its pmf --------------------------------------------------------------------------------------------
def _row(L, seed):
    """a built row: weights in [0, 65536] with the maximum present, a third of them zero (the first and the last too where L allows)"""
    u = synth.uniform(L, seed, 2)
    k = np.where(u[1] < F(1 / 3), 0, (u[0] * F(65536)).astype(np.uint32)).astype(np.uint64)
    if L > 2:
        k[0] = k[-1] = 0
    k[L // 2] = 65536
    return np.cumsum(k).astype(np.uint32)[None, :]


PAIRS = [(1, 0.0), (1, 0.5), (2, 0.1), (3, 2.0 ** -16), (4, 0.5), (64, 0.1), (65, 1.0), (257, 0.3), (1024, 0.0), (1024, 0.1)]


@pytest.mark.parametrize("L,delta", PAIRS)
def test_the_share_of_u_that_selects_a_light_is_its_pmf(L, delta):
    rows = _row(L, 40 + L)
    k = lm.weights(rows[0])
    counts = np.zeros(L, np.int64)
    chunk = 1 << 22
    for base in range(0, 1 << 24, chunk):
        u = (np.arange(base, base + chunk, dtype=np.float64) * STEP).astype(F)       # exact
        j, tree_branch = lm.select(rows, np.zeros(chunk, np.int64), u, delta)
        assert (j < L).all() and (k[j[tree_branch]] > 0).all()                        # no light without a weight from the tree branch
        counts += np.bincount(j, minlength=L)
    pm = lm.pmf(rows, np.zeros(L, np.int64), np.arange(L), delta).astype(np.float64)
    err = np.abs(counts * STEP - pm) / STEP
    print("L = %4d delta = %-10g max |share - pmf| = %.2f steps of 2^-24; sum of pmf - 1 = %.2f steps" % (
        L, delta, err.max(), (pm.sum() - 1) / STEP))
    assert (err <= 6).all()
    if delta == 0.0:
        assert (counts[k == 0] == 0).all()
    # the unlearned leaf of the same length (delta plays no part: once per L)
    if (L, delta) != next(pair for pair in PAIRS if pair[0] == L):
        return
    counts0 = np.zeros(L, np.int64)
    for base in range(0, 1 << 24, chunk):
        u = (np.arange(base, base + chunk, dtype=np.float64) * STEP).astype(F)
        counts0 += np.bincount(lm.select(rows, np.full(chunk, -1, np.int64), u, delta)[0], minlength=L)
    assert (np.abs(counts0 * STEP - float(F(1) / F(L))) / STEP <= 6).all()


# ---- what it buys -------------------------------------------------------------------------------------------------------------
def test_the_learned_row_lowers_the_variance_of_next_event_estimation(one_leaf):
    L, n_train, n_eval = 64, 1 << 15, 1 << 16
    strength = np.full(L, 0.02, F)
    strength[17] = 40.0                                                    # one light in 64 carries the energy
    visible = F(0.75)                                                      # a sample is occluded with probability 1/4

    def contributions(light, seed):
        vis = synth.uniform(light.shape[0], seed)[0] < visible
        return np.where(vis, strength[light], F(0)).astype(F)

    mod = lm.LightsModel(one_leaf, L, delta=0.1)
    p_train = synth.positions_uniform(n_train, 50, BB0, BB1)
    lt = np.minimum((synth.uniform(n_train, 51)[0] * F(L)).astype(np.uint32), L - 1)
    mod.record({"position": p_train, "light": lt, "value": contributions(lt, 52)})
    assert mod.build() == 1
    p = synth.positions_uniform(n_eval, 53, BB0, BB1)
    u = synth.uniform(n_eval, 54)[0]
    truth = float(strength.astype(np.float64).sum() * float(visible))
    est = {}
    for name, m in (("uniform", lm.LightsModel(one_leaf, L, delta=0.1)), ("learned", mod)):
        light, pm = m.sample(p, u)
        e = contributions(light, 55).astype(np.float64) / pm.astype(np.float64)
        mean, se = e.mean(), e.std(ddof=1) / np.sqrt(n_eval)
        print("%-8s mean %.4f (truth %.4f, %.2f standard errors off)  variance %.4f" % (name, mean, truth, abs(mean - truth) / se, e.var(ddof=1)))
        assert abs(mean - truth) <= 5 * se, (name, mean, truth, se)
        est[name] = e.var(ddof=1)
    print("variance of value / pmf, learned : uniform = %.5f" % (est["learned"] / est["uniform"]))
    assert est["learned"] < est["uniform"]


# ---- the ABI: header, SURFACE_EXT and the two builds name the same nine calls ---------------------------------------------------
def test_header_table_and_libraries_agree(native):  # noqa: F811
    declared = abi_table.declarations(HEADER)
    assert declared == CALLS
    assert [n for n, _ in declared] == re.findall(r"^(?:int|const char \*)\s*(pg_[a-z_0-9]+)\s*\(", abi_table.header_text(HEADER), flags=re.M)
    assert list(native.SURFACE_EXT) == [HEADER] and native.EXPORTS_LIGHTS == tuple(n for n, _ in CALLS)
    bound = native.SURFACE_EXT[HEADER]
    assert [(n, len(a)) for n, a in bound.items()] == CALLS
    product, probe, L = abi_table.product_library(native), abi_table.probe_library(native), native.lib()
    for name, n_params in CALLS:
        assert hasattr(product, name) and hasattr(probe, name), name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_params, name
    assert L.pg_lights_enable.argtypes[2]._type_ is native.pg_lights_params
    assert L.pg_lights_record.argtypes[2]._type_ is native.pg_lights_records
    # no call is in two tables
    others = set().union(*map(set, list(native.SURFACE.values()) + list(native.SURFACE_EXTRA.values())))
    assert not others & set(bound)
    # the build and the source hash see the header: the wildcard for subdirectories stands in front of the two pinned ones
    mk = open(os.path.join(native.CSRC, "Makefile")).read()
    assert re.search(r"^HDRS = .*\$\(wildcard \.\./\.\./include/\*/\*\.h\) \$\(wildcard \.\./\.\./include/pg_\*\.h\) "
                     r"\$\(wildcard \.\./\.\./include/pgsd\*\.h\)$", mk, flags=re.M)
    assert "pg_kernels_lights.hip" in re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()
    assert os.path.exists(os.path.join(abi_table.INCLUDE, *HEADER.split("/")))
    text = open(os.path.join(abi_table.INCLUDE, *HEADER.split("/")), "rb").read()
    assert '#include "../pgsd.h"' in text.decode() and len(native.source_hash()) == 16


def test_struct_layouts(native):  # noqa: F811
    assert ctypes.sizeof(native.pg_lights_params) == 12
    assert [(f[0], f[1]) for f in native.pg_lights_params._fields_] == [("delta", ctypes.c_float), ("root", ctypes.c_uint32),
                                                                       ("reserved", ctypes.c_uint32)]
    assert ctypes.sizeof(native.pg_lights_records) == 3 * 8
    text = re.sub(r"/\*.*?\*/", "", abi_table.header_text(HEADER), flags=re.S)
    body = re.search(r"typedef struct pg_lights_records \{(.*?)\} pg_lights_records;", text, flags=re.S).group(1)
    assert re.findall(r"\*\s*([a-z_]+)\s*[,;]", body) == [f[0] for f in native.pg_lights_records._fields_]
    body = re.search(r"typedef struct pg_lights_params \{(.*?)\} pg_lights_params;", text, flags=re.S).group(1)
    assert re.findall(r"(?:float|uint32_t)\s+([a-z_]+)\s*;", body) == [f[0] for f in native.pg_lights_params._fields_]
    assert (native.PG_LIGHTS_MAX, native.PG_LIGHTS_WEIGHT_ONE, native.PG_LIGHTS_NONE) == (lm.MAX_LIGHTS, lm.WEIGHT_ONE, lm.NONE)
    assert "#define PG_LIGHTS_MAX 4096" in text and "#define PG_LIGHTS_WEIGHT_ONE 65536" in text
    assert "#define PG_LIGHTS_NONE 0xFFFFFFFFu" in text


def test_the_pinned_surfaces_are_untouched(native):  # noqa: F811
    assert tuple(native.SURFACE) == abi_table.HEADERS and sum(len(v) for v in native.SURFACE.values()) == abi_table.TOTAL == 89
    assert list(native.SURFACE_EXTRA) == ["pg_resample.h"] and list(native.SURFACE_EXTRA["pg_resample.h"]) == ["pg_resample_cosine"]
    assert native.ABI_VERSION == abi_table.ABI_VERSION == 6
    on_disk = sorted(os.path.basename(f) for f in glob.glob(os.path.join(abi_table.INCLUDE, "*.h")))
    assert on_disk == sorted(abi_table.HEADERS + ("pg_resample.h",))
    assert [os.path.relpath(f, abi_table.INCLUDE) for f in glob.glob(os.path.join(abi_table.INCLUDE, "*", "*.h"))] == [os.path.join(*HEADER.split("/"))]


def test_the_header_says_what_is_not_built():
    text = " ".join(abi_table.header_text(HEADER).split())
    assert "NOT BUILT" in text
    for what in ("pg_render_pass", "remapped u", "light hierarchies", "compacted lane lists", "npz schema"):
        assert what in text.split("NOT BUILT", 1)[1], what
