"""The learned light selection on the device (include/ext/pg_lights.h) against the numpy model of the header
(tests/lights_model.py), bit for bit: integer sums and one rounding per operation, so there is no tolerance anywhere.
ctypes -> C ABI through SDTree.

The row lengths straddle the kernels' shapes: 1, 2, 3 (less than a wave), 64 and 65 (one chunk of the wave's scan and one more),
257 (the first row one workgroup builds, two chunks) and 1025 (five chunks), 4096 (the longest) on the one-leaf tree."""
import ctypes as C

import numpy as np
import pytest

import lights_model as lm
import synth
from oracle import pg_oracle as po
from test_gpu_fraction import _deep, _leaves, _uneven_records
from test_gpu_kd_grid_faces import face_positions
from test_gpu_parity import BB0, BB1, assert_same_tree, dev, gpu_tree_from

pytestmark = pytest.mark.gpu

F = np.float32
NQ = 4099                   # query lanes: the last workgroup is partial
M = (1 << 16) - 3           # records of a set
ONE_LEAF = (30.0, 40.0, 50.0)
TREES = ["initial", "balanced", "skewed"]
LIGHTS = [1, 2, 3, 64, 65, 257, 1025]
CASES = [(w, L) for w in TREES for L in LIGHTS] + [("initial", 4096)]
DELTAS = [0.0, 2.0 ** -16, 0.1, 0.5, 1.0]
PG_ERR_INVALID = -1


@pytest.fixture(autouse=True)
def _synchronise_behind_every_call():
    """A GPU fault then names the call that launched the faulting kernel."""
    from practical_path_guiding_lab_amd import sdtree
    sdtree.SYNC_EVERY_CALL = True
    yield
    sdtree.SYNC_EVERY_CALL = False


@pytest.fixture(scope="module")
def oracle_trees():
    init = po.OracleTree()
    init.setup(BB0, BB1, 20, 20, True)
    return {"initial": init, "balanced": synth.build_balanced(3, 4), "skewed": synth.build_skewed(4096, 4).prev}


_SETS, _KINDS = {}, {}


def record_sets(L):
    """Computed once per row length, shared, never written to: uniform records, all records in one (leaf, light), and a set on
    the cell faces of the KD grid salted with every hostile record."""
    if L not in _SETS:
        sets = {"uniform": lm.synthetic_records(M, 101, BB0, BB1, L),
                "one key": lm.synthetic_records(M, 103, BB0, BB1, L, ONE_LEAF, L - 1),
                "edges": lm.synthetic_records(M, 105, BB0, BB1, L)}
        sets["edges"]["position"] = face_positions(M, 107)
        kinds = lm.salt_with_edges(sets["edges"], BB0, BB1, L)
        assert all((kinds == k).any() for k in lm.EDGE_KINDS)
        _KINDS[L] = kinds
        for r in sets.values():
            for v in r.values():
                v.setflags(write=False)
        _SETS[L] = sets
    return _SETS[L]


def _gpu_tree(which, tree):
    from practical_path_guiding_lab_amd.sdtree import SDTree
    if which == "initial":
        g = SDTree()
        g.setup(BB0, BB1, 0, 0, 20, 20, True, 0.5)
        return g
    return gpu_tree_from(tree)


def distinct_rows(n, L, seed):
    """Rows no two leaves share: weights in [0, 65536], about a third of them zero, the maximum somewhere; every fifth leaf
    (not the first) unlearned."""
    u = synth.uniform(n * L, seed, 2)
    k = np.where(u[1] < F(1 / 3), 0, (u[0] * F(65536)).astype(np.uint32)).astype(np.uint64).reshape(n, L)
    k[np.arange(n), (np.arange(n) * 7) % L] = 65536
    rows = np.cumsum(k, axis=1).astype(np.uint32)
    rows[4::5] = 0
    return rows


def both(which, tree, L, seed=None, delta=0.1, root=False):
    """(device tree, model) with the feature on; with a seed, the same distinct rows loaded."""
    g = _gpu_tree(which, tree)
    mod = lm.LightsModel(tree, L, delta=delta, root=root)
    g.lightsEnable(L, delta=delta, root=root)
    if seed is not None:
        st = {"rows": distinct_rows(mod.n, L, seed)}
        g.lightsLoadState(st)
        mod.load_state(st)
    return g, mod


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).view(np.uint32)


def same_state(dev_state, model_state, acc=True):
    np.testing.assert_array_equal(dev_state["rows"], model_state["rows"])
    if acc:
        np.testing.assert_array_equal(dev_state["acc"], model_state["acc"])


def to_dev(torch, rec, idx=None):
    """a copy on the device (the shared sets are read-only); idx: the records to take"""
    out = {}
    for k, v in rec.items():
        v = np.array(v if idx is None else v[..., idx])
        out[k] = dev(torch, v.view(np.int32) if v.dtype == np.uint32 else v)
    return out


def edge_u(n, seed, delta):
    """n numbers in [0, 1) with the edges of SELECT in front"""
    d = F(delta)
    u = synth.uniform(n, seed)[0].copy()
    edges = [0.0, 1.0 - 2.0 ** -24, d, np.nextafter(d, F(-1)), np.nextafter(d, F(2)), 1.0, -0.0, -0.25, np.nan, np.inf, -np.inf,
             2.0 ** -24, 0.5, np.nextafter(F(1), F(2))]
    u[:len(edges)] = np.array(edges, F)
    return u


# ---- sample and pmf -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,L", CASES)
def test_sample_and_pmf_equal_the_model(oracle_trees, which, L):
    import torch
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    tree = oracle_trees[which]
    n = NQ
    p = face_positions(n, 60 + L)                    # cell faces, outside the box, NaN
    # (the special positions stay in front; behind them sixteen lanes at one position of a leaf that distinct_rows leaves learned)
    cand = synth.positions_uniform(64, 5, BB0, BB1)
    cand_leaf = lm.LightsModel(tree, 1).leaf_of(cand, np.ones(64, bool))
    p[:, 16:32] = cand[:, np.nonzero(cand_leaf % 5 != 4)[0][0]][:, None]
    active = (synth.uniform(n, 62)[0] < 0.85).astype(np.uint8)
    active[16:32] = 1
    lights = np.minimum((synth.uniform(n, 63)[0] * F(L + 2)).astype(np.uint32), L + 1)    # some are L and L + 1: no such light
    lights[:4] = [0, L - 1, L, 0xFFFFFFFF]
    dp, dact, dl = dev(torch, p), dev(torch, active), dev(torch, lights.view(np.int32))
    g = _gpu_tree(which, tree)
    learned_branches = 0
    for delta in DELTAS:
        g.lightsEnable(L, delta=delta)
        mod = lm.LightsModel(tree, L, delta=delta)
        st = {"rows": distinct_rows(mod.n, L, 7)}
        g.lightsLoadState(st)
        mod.load_state(st)
        assert g.lightsStatus() == (L, mod.learned_leaves())
        u = edge_u(n, 64, delta)
        u = np.concatenate([u[:16], u[:16], u[32:]])             # the edges once at the special positions, once inside the box
        for act, dact_ in ((active, dact), (None, None)):
            # u given: the streams are not needed
            light, pmf = g.lightsSample(dp, u=dev(torch, u), active=dact_)
            want_light, want_pmf = mod.sample(p, u, active=act)
            np.testing.assert_array_equal(bits(light), want_light, err_msg="delta %g" % delta)
            np.testing.assert_array_equal(bits(pmf), bits(want_pmf), err_msg="delta %g" % delta)
            # u from the stream: the sampler's state moves on the active lanes only
            smp = PCG32Sampler(g, n, seed=11)
            st_, inc = po.rng_seed(n, 11)
            light, pmf = g.lightsSample(dp, sampler=smp, active=dact_)
            want_light, want_pmf = mod.sample(p, None, st_, inc, active=act)
            np.testing.assert_array_equal(bits(light), want_light)
            np.testing.assert_array_equal(bits(pmf), bits(want_pmf))
            np.testing.assert_array_equal(smp.state.cpu().numpy().view(np.uint64), st_)
            # the pmf of given lights; of the sampled light it is the sample's
            np.testing.assert_array_equal(bits(g.lightsPmf(dp, dl, dact_)), bits(mod.pmf(p, lights, act)))
            chosen = dev(torch, want_light.view(np.int32))
            np.testing.assert_array_equal(bits(g.lightsPmf(dp, chosen, dact_)), bits(want_pmf))
        ins = mod.inside(p)
        leaf = mod.leaf_of(p, ins)
        _, tree_branch = lm.select(mod.rows, leaf, u, delta)
        learned_branches += int(tree_branch.any()) + int((~tree_branch & (leaf >= 0)).any())
        assert (want_pmf[~ins] == F(1) / F(L)).all() and (~ins).any()
    assert learned_branches >= len(DELTAS) + 2       # both branches were taken
    L_, h = g._lib, g._h
    assert L_.pg_lights_sample(h, n, dp.data_ptr(), None, None, None, None, dl.data_ptr(), dp.data_ptr(), None) == PG_ERR_INVALID
    assert L_.pg_lights_sample(h, n, dp.data_ptr(), dp.data_ptr(), None, None, None, None, dp.data_ptr(), None) == PG_ERR_INVALID
    assert L_.pg_lights_pmf(h, n, dp.data_ptr(), None, None, dp.data_ptr(), None) == PG_ERR_INVALID
    g._ck(L_.pg_lights_sample(h, 0, None, None, None, None, None, None, None, None))
    g._ck(L_.pg_lights_pmf(h, 0, None, None, None, None, None))
    torch.cuda.synchronize()


# ---- record -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,L", CASES)
def test_record_accumulators_equal_the_model(oracle_trees, which, L):
    import torch
    tree = oracle_trees[which]
    for name, rec in record_sets(L).items():
        g, mod = both(which, tree, L, seed=9)
        kept = mod.record(rec)
        want = mod.acc_words()
        assert int(want[..., 3].sum()) == int(kept.sum()) > M // 3, name
        if name == "one key":
            assert (want[..., 3] > 0).sum() == 1       # the worst contention: every record in one sector
        if name == "edges":
            kinds = _KINDS[L]
            assert not kept[np.isin(kinds, lm.EDGE_DROPPED)].any()
            on_face = np.array(rec["position"])[:, kinds == "on the box face"]
            assert kept[(kinds == "above the clamp") | (kinds == "zero") | (kinds == "negative zero")].sum() > 100 and on_face.size
        g.lightsRecord(to_dev(torch, rec))
        same_state(g.lightsState(), mod.state())
        # the same set shuffled and split over three launches, into a second context: chunks padded behind their d_count with
        # records that must not count
        g2, _ = both(which, tree, L, seed=9)
        order = np.argsort(synth.uniform(M, 120)[0], kind="stable")
        for part in np.array_split(order, 3):
            idx = np.concatenate([part, order[:257]])
            g2.lightsRecord(to_dev(torch, rec, idx), torch.tensor([part.size], dtype=torch.int32, device="cuda"))
        same_state(g2.lightsState(), mod.state())
        # a d_count above m is m
        if name == "uniform":
            g3, mod3 = both(which, tree, L, seed=9)
            idx = np.arange(1000)
            mod3.record({k: v[..., idx] for k, v in rec.items()})
            g3.lightsRecord(to_dev(torch, rec, idx), torch.tensor([5000], dtype=torch.int32, device="cuda"))
            same_state(g3.lightsState(), mod3.state())
    torch.cuda.synchronize()


# ---- build --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,L", CASES)
def test_build_gives_the_models_rows_for_both_targets(oracle_trees, which, L):
    import torch
    tree = oracle_trees[which]
    sets = record_sets(L)
    pair = [both(which, tree, L, seed=13, root=root) for root in (False, True)]
    before = pair[0][1].rows.copy()
    for rnd, name in enumerate(("edges", "uniform")):
        drec = to_dev(torch, sets[name])
        pair[0][1].record(sets[name])
        pair[1][1].acc = pair[0][1].acc.copy()       # (the same records: the same sums)
        for g, mod in pair:
            g.lightsRecord(drec)
            built = mod.build()
            g.lightsBuild()
            same_state(g.lightsState(), mod.state())          # the rows, and the accumulators the build left alone
            assert built >= 1 and g.lightsStatus() == (L, mod.learned_leaves())
            k = np.diff(mod.rows.astype(np.int64), axis=1, prepend=0)
            assert (k.max(axis=1)[mod.rows[:, -1] > 0] == 65536).all() and k.min() >= 0
    if L > 1:
        assert (pair[0][1].rows != pair[1][1].rows).any()      # the two targets differ
        assert (pair[0][1].rows != before).any()               # (a row of one light is [65536] whatever was recorded)
    # a leaf no record reached keeps its row: all records in one leaf, every other row stays
    g, mod = both(which, tree, L, seed=15)
    before = mod.rows.copy()
    mod.record(sets["one key"])
    g.lightsRecord(to_dev(torch, sets["one key"]))
    assert mod.build() == 1
    g.lightsBuild()
    same_state(g.lightsState(), mod.state())
    t = int(mod.leaf_of(np.array(ONE_LEAF, F)[:, None], np.array([True]))[0])
    assert mod.rows[t].tolist() == [0] * (L - 1) + [65536] and (np.delete(mod.rows, t, 0) == np.delete(before, t, 0)).all()
    torch.cuda.synchronize()


def test_two_contexts_that_sum_their_buffers_equal_one(oracle_trees):
    import torch
    L = 65
    rec = record_sets(L)["uniform"]
    tree = oracle_trees["skewed"]
    whole, _ = both("skewed", tree, L, seed=17)
    whole.lightsRecord(to_dev(torch, rec))
    halves = []
    for part in (np.arange(0, M, 2), np.arange(1, M, 2)):
        h, _ = both("skewed", tree, L, seed=17)
        h.lightsRecord(to_dev(torch, rec, part))
        halves.append(h)
    a, b = halves[0].lightsAccumulators(), halves[1].lightsAccumulators()
    assert a.dtype == torch.int64 and a.numel() == b.numel() == whole.lightsAccumulators().numel() == 4 * L * whole.sizes().n_roots
    total = a + b
    assert torch.equal(total, whole.lightsAccumulators()) and not torch.equal(a, total)
    a.copy_(total)
    b.copy_(total)
    whole.lightsBuild()
    want = whole.lightsState()
    assert (want["rows"] != distinct_rows(want["rows"].shape[0], L, 17)).any()
    for h in halves:
        h.lightsBuild()
        same_state(h.lightsState(), want)
    torch.cuda.synchronize()


# ---- refine -------------------------------------------------------------------------------------------------------------------
def assert_carried(old_cols, old_state, new_cols, new_state):
    """Every new leaf's row is the row of the old leaf whose box contains the new leaf's centre; accumulators are zero.
    Returns the number of leaves that did not split."""
    _, omin, omax, otree = _leaves(old_cols)
    _, nmin, nmax, ntree = _leaves(new_cols)
    centre = (nmin + nmax) / 2
    inside = ((centre[:, None, :] >= omin[None]) & (centre[:, None, :] <= omax[None])).all(axis=2)
    assert (inside.sum(axis=1) == 1).all()
    src = otree[inside.argmax(axis=1)]
    assert sorted(ntree) == list(range(new_state["rows"].shape[0]))
    np.testing.assert_array_equal(new_state["rows"][ntree], old_state["rows"][src])
    assert (new_state["acc"] == 0).all()
    return int(((nmin[:, None, :] == omin[None]) & (nmax[:, None, :] == omax[None])).all(axis=2).any(axis=1).sum())


def _tree_ready_to_split(oracle_trees, L, seed, recs):
    """The balanced tree with the feature on, distinct rows, and enough clustered records splatted to split some KD leaves."""
    g = _deep(oracle_trees["balanced"])
    g.lightsEnable(L)
    g.lightsLoadState({"rows": distinct_rows(int(g.sizes().n_roots), L, seed)})
    g.setIteration(0, False)
    g.addDataPropagate(recs)
    return g


@pytest.mark.parametrize("L", [3, 257])
def test_refine_carries_the_rows_and_zeroes_the_accumulators(oracle_trees, L):
    import torch
    rec = record_sets(L)["uniform"]
    g = _tree_ready_to_split(oracle_trees, L, 19, _uneven_records(torch))
    g.lightsRecord(to_dev(torch, rec))
    old_cols, old_state = g.export(), g.lightsState()
    assert (old_state["acc"] != 0).any()
    g.refineAndPrepare()
    new_cols, new_state = g.export(), g.lightsState()
    n_old, n_new = old_state["rows"].shape[0], new_state["rows"].shape[0]
    unsplit = assert_carried(old_cols, old_state, new_cols, new_state)
    assert n_new > n_old + 2 and 0 < unsplit < n_old, (n_old, n_new, unsplit)     # some leaves split, more than once; some did not
    assert g.lightsAccumulators().numel() == 4 * L * n_new
    # the refined tree learns on: the model of the new tree, the carried rows loaded, one round
    o = po.OracleTree()
    o.load(new_cols)
    mod = lm.LightsModel(o, L)
    mod.load_state(new_state)
    mod.record(rec)
    g.lightsRecord(to_dev(torch, rec))
    mod.build()
    g.lightsBuild()
    same_state(g.lightsState(), mod.state())
    p = face_positions(NQ, 70)
    u = synth.uniform(NQ, 71)[0]
    light, pmf = g.lightsSample(dev(torch, p), u=dev(torch, u))
    want_light, want_pmf = mod.sample(p, u)
    np.testing.assert_array_equal(bits(light), want_light)
    np.testing.assert_array_equal(bits(pmf), bits(want_pmf))
    torch.cuda.synchronize()


def test_a_refine_that_fails_leaves_the_lights_state_as_it_was(oracle_trees):
    """For k = 0, 1, ... pg_debug_fail_alloc(k) refuses the allocation after k successful ones of a FRESH context's refine, so
    every allocation site of the refine is the refused one once -- the lights' spare table, the last before the commit, among
    them (tests/test_gpu_fraction.py has the scheme, and the one-context variant)."""
    import torch
    from practical_path_guiding_lab_amd import _native as N
    L = 65
    recs = _uneven_records(torch)
    rec = to_dev(torch, record_sets(L)["uniform"])
    g = _tree_ready_to_split(oracle_trees, L, 23, recs)
    g.lightsRecord(rec)
    lib = g._lib
    old_cols, old_state = g.export(), g.lightsState()
    assert (old_state["acc"] != 0).any()
    failures, sites = 0, []
    try:
        for k in range(64):
            if k:
                g = _tree_ready_to_split(oracle_trees, L, 23, recs)
                g.lightsRecord(rec)
            assert lib.pg_debug_fail_alloc(k) == 0
            try:
                g.refineAndPrepare()
            except N.PgError as e:
                assert e.code == -3 and lib.pg_debug_fail_alloc_pending() == 0, e     # PG_ERR_NOMEM, from the hook
                failures += 1
                sites.append(str(e))
                assert_same_tree(g.export(), old_cols)
                same_state(g.lightsState(), old_state)
                continue
            break
        else:
            pytest.fail("the refine never went through: " + str(sites))
    finally:
        lib.pg_debug_fail_alloc(-1)
    assert failures >= 3 and "li.spare" in sites[-1] and len(set(sites)) > 10, sites     # the lights' own table was the refused one once
    new_state = g.lightsState()
    assert new_state["rows"].shape[0] > old_state["rows"].shape[0]
    assert_carried(old_cols, old_state, g.export(), new_state)
    torch.cuda.synchronize()


# ---- export, import, refusals -------------------------------------------------------------------------------------------------
def test_export_import_and_every_refusal(oracle_trees):
    """Every refusal of the header's calls but the bound on leaves x lights, which has its own test below."""
    import torch
    from practical_path_guiding_lab_amd import _native as N
    tree = oracle_trees["balanced"]
    L = 5
    never, g = _deep(tree), _deep(tree)
    lib, h = g._lib, g._h
    n = int(g.sizes().n_roots)
    p = dev(torch, face_positions(256, 1))
    out = torch.zeros(256, device="cuda")
    iout = torch.zeros(256, dtype=torch.int32, device="cuda")
    rec = N.pg_lights_records()
    rows, acc = np.zeros((n, L), np.uint32), np.zeros((n, L, 4), np.int64)
    rp, ap = rows.ctypes.data, acc.ctypes.data
    ptr, cnt = C.c_void_p(), C.c_uint64()

    def every_call_is_refused():
        calls = [lib.pg_lights_sample(h, 256, p.data_ptr(), out.data_ptr(), None, None, None, iout.data_ptr(), out.data_ptr(), None),
                 lib.pg_lights_pmf(h, 256, p.data_ptr(), iout.data_ptr(), None, out.data_ptr(), None),
                 lib.pg_lights_record(h, 0, C.byref(rec), None, None), lib.pg_lights_build(h, None),
                 lib.pg_lights_accumulators(h, C.byref(ptr), C.byref(cnt)), lib.pg_lights_export(h, n, L, rp, ap),
                 lib.pg_lights_import(h, n, L, rp)]
        assert calls == [PG_ERR_INVALID] * 7, calls
        assert b"pg_lights_enable" in lib.pg_last_error(h)
        assert g.lightsStatus() == (0, 0)

    every_call_is_refused()
    # pg_lights_enable: every refusal of the header
    ok = N.pg_lights_params(0.1, 0, 0)
    for bad_n, prm in ((4097, ok), (1 << 31, ok), (L, N.pg_lights_params(-0.01, 0, 0)), (L, N.pg_lights_params(1.0001, 0, 0)),
                       (L, N.pg_lights_params(float("nan"), 0, 0)), (L, N.pg_lights_params(0.1, 2, 0)),
                       (L, N.pg_lights_params(0.1, 0, 1))):
        assert lib.pg_lights_enable(h, bad_n, C.byref(prm)) == PG_ERR_INVALID, (bad_n, prm.delta, prm.root, prm.reserved)
    assert lib.pg_lights_enable(h, L, None) == PG_ERR_INVALID
    every_call_is_refused()
    with pytest.raises(ValueError):
        g.lightsEnable(0)
    g.lightsEnable(L, delta=1.0)                     # (the ends of the range are in it)
    g.lightsEnable(L, delta=0.0, root=True)
    st = g.lightsState()
    assert st["rows"].shape == (n, L) and (st["rows"] == 0).all() and (st["acc"] == 0).all() and g.lightsStatus() == (L, 0)
    # a round trip, accumulators and all; h_acc may be NULL
    rs = record_sets(L)["uniform"]
    g.lightsRecord(to_dev(torch, rs))
    g.lightsBuild()
    st = g.lightsState()
    assert g.lightsStatus() == (L, n) and (st["acc"][..., 3] > 0).all()
    g._ck(lib.pg_lights_export(h, n, L, rp, None))
    np.testing.assert_array_equal(rows, st["rows"])
    g2 = _deep(tree)
    g2.lightsEnable(L, delta=0.0, root=True)
    g2.lightsLoadState(st)
    st2 = g2.lightsState()
    np.testing.assert_array_equal(st2["rows"], st["rows"])
    assert (st2["acc"] == 0).all()
    g.lightsLoadState(st)                            # import zeroes the accumulators
    assert (g.lightsState()["acc"] == 0).all()
    # import and export: sizes that do not match, NULL, rows that do not ascend, steps above 65536
    assert lib.pg_lights_export(h, n + 1, L, rp, ap) == PG_ERR_INVALID and lib.pg_lights_export(h, n, L + 1, rp, ap) == PG_ERR_INVALID
    assert lib.pg_lights_export(h, n, L, None, ap) == PG_ERR_INVALID
    assert lib.pg_lights_import(h, n + 1, L, rp) == PG_ERR_INVALID and lib.pg_lights_import(h, n, L - 1, rp) == PG_ERR_INVALID
    assert lib.pg_lights_import(h, n, L, None) == PG_ERR_INVALID
    for leaf, row in ((n - 1, [10, 9, 9, 9, 9]), (0, [65537] * 5), (n // 2, [0, 0, 7, 7, 65544]), (1, [5, 5, 5, 5, 4])):
        bad = st["rows"].copy()
        bad[leaf] = row
        with pytest.raises(N.PgError):
            g.lightsLoadState({"rows": bad})
        np.testing.assert_array_equal(g.lightsState()["rows"], st["rows"])            # a refused import changes nothing
    edge = st["rows"].copy()
    edge[0] = np.arange(1, L + 1, dtype=np.uint32) * 65536                            # steps of exactly 65536, and
    edge[1] = 0                                                                       # an unlearned row, are accepted
    g.lightsLoadState({"rows": edge})
    assert g.lightsStatus() == (L, n - 1)
    # record: NULL columns
    assert lib.pg_lights_record(h, 16, None, None, None) == PG_ERR_INVALID
    assert lib.pg_lights_record(h, 16, C.byref(rec), None, None) == PG_ERR_INVALID
    assert lib.pg_lights_accumulators(h, None, C.byref(cnt)) == PG_ERR_INVALID
    g.lightsRecord(to_dev(torch, rs))
    g.lightsDisable()
    every_call_is_refused()
    # a refine of the once-enabled context and of one that never was: export for export
    recs = _uneven_records(torch)
    for t in (g, never):
        t.setIteration(0, False)
        t.addDataPropagate(recs)
        t.refineAndPrepare()
    assert_same_tree(g.export(), never.export())
    assert g.export()["kdtree_depth"].shape[0] > tree.export()["kdtree_depth"].shape[0]
    assert torch.equal(g.accumulators(), never.accumulators())
    every_call_is_refused()
    # setup and load switch the feature off
    g.lightsEnable(L)
    g.load(tree.export())
    every_call_is_refused()
    g.lightsEnable(L)
    g.setup(BB0, BB1, 0, 0, 20, 20, True, 0.5)
    every_call_is_refused()
    torch.cuda.synchronize()


def test_more_than_two_to_the_31_leaves_times_lights_is_refused():
    """pg_lights_enable refuses when n_roots * n_lights exceeds 2^31, before it allocates: 2^20 KD leaves (a complete tree, every
    leaf with a quadtree of one level) and 4096 lights are 2^32 entries, 2049 lights 2^31 + 2^20.  The feature stays off and the
    context goes on working; with one light it is enabled and selects.  (2048 lights, exactly 2^31 entries, are accepted and
    would allocate 77 GB: not asked for here.  The refine's PG_ERR_NOMEM for the same bound is not tested either: it can be
    reached only from an enabled table of about that size.)"""
    import torch
    from practical_path_guiding_lab_amd import _native as N
    tree = synth.build_balanced(20, 1)
    g = gpu_tree_from(tree)
    lib, h = g._lib, g._h
    n = int(g.sizes().n_roots)
    assert n == 1 << 20
    free_before = torch.cuda.mem_get_info()[0]
    prm = N.pg_lights_params(0.1, 0, 0)
    for L in (4096, 2049):
        assert n * L > 1 << 31
        assert lib.pg_lights_enable(h, L, C.byref(prm)) == PG_ERR_INVALID
        assert b"2^31" in lib.pg_last_error(h)
        with pytest.raises(N.PgError):
            g.lightsEnable(L)
        assert g.lightsStatus() == (0, 0)
        ptr, cnt = C.c_void_p(), C.c_uint64()
        assert lib.pg_lights_accumulators(h, C.byref(ptr), C.byref(cnt)) == PG_ERR_INVALID       # the feature stayed off
    assert torch.cuda.mem_get_info()[0] >= free_before - (64 << 20)                              # and nothing was allocated for it
    # the context still works: the tree answers as the oracle does, and a row length within the bound is enabled and selects
    p = face_positions(NQ, 80)
    dp = dev(torch, p)
    with np.errstate(invalid="ignore"):
        ins = ((p >= F(0)) & (p <= F(100))).all(axis=0)
    got = g.getLeafNodeIndex(dp).cpu().numpy()
    np.testing.assert_array_equal(got[ins], tree.get_leaf_node_index(np.ascontiguousarray(p[:, ins])))
    g.lightsEnable(2)
    assert g.lightsStatus() == (2, 0) and g.lightsAccumulators().numel() == 4 * 2 * n
    u = synth.uniform(NQ, 81)[0]
    light, pmf = g.lightsSample(dp, u=dev(torch, u))
    np.testing.assert_array_equal(bits(light), np.minimum((lm.sanitize(u) * F(2)).astype(np.uint32), 1))
    assert (pmf.cpu().numpy() == F(0.5)).all()
    torch.cuda.synchronize()
