"""pg_resample_cosine on the device (include/pg_resample.h) against tests/resample_model.py, bit for bit: every output array,
the candidate arrays and the lanes' stream states; there is no tolerance anywhere.  ctypes -> C ABI through SDTree.

N = 4099 lanes: seventeen workgroups, the last one ragged down to a wave of three lanes.  M in {1, 2, 5, 64}; (alpha, delta) in
{(0.5, 0.1), (0, 0), (1, 1), (0, 1)}.  Trees: the golden tree (the lifecycle of tests/golden/make_golden.py, held to the
committed digest), a single-leaf tree, and a ragged forest one of whose quadtrees holds no energy.  Positions: uniform, the box's
faces and corners, split planes, outside the box, NaN.  Normals: uniform, the axes, zero and minus zero, non-unit, NaN and
+-inf.  An `active` mask with holes."""
import functools
import os
import sys

import numpy as np
import pytest

import irradiance_synth as isy
import resample_model as rs
import synth
from oracle import pg_oracle as po
from probe_harness import same_bits

pytestmark = pytest.mark.gpu

F = np.float32
N = 4099
MS = (1, 2, 5, 64)
PAIRS = ((0.5, 0.1), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0))
TREES = ("golden", "single leaf", "one dark quadtree")
PG_ERR_INVALID = -1
FLAGS = ("index", "state")
SEED = 77


@pytest.fixture(autouse=True)
def _synchronise_behind_every_call():
    """A GPU fault then names the call that launched the faulting kernel."""
    from practical_path_guiding_lab_amd import sdtree
    sdtree.SYNC_EVERY_CALL = True
    yield
    sdtree.SYNC_EVERY_CALL = False


@functools.lru_cache(maxsize=None)
def columns(which):
    """export() columns of the tree `which`"""
    if which == "golden":
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
        import make_golden as G
        pair = po.OracleSDTreePair()
        pair.setup(G.BB0, G.BB1, 20, 20, True)
        digests = G.lifecycle(lambda r: synth.splat(pair.current, r), lambda k: pair.refine_and_prepare(k), lambda: pair.prev.export())
        golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdtree_golden.npz"))
        assert digests == golden["digests"].tolist()
        return pair.prev.export()
    if which == "single leaf":
        return rs.single_leaf_tree().export()
    # five KD leaves, quadtrees 0, 3 and 5 levels deep; quadtree 1 (three levels) holds no energy at all
    return isy.set_energies(isy.ragged_forest(2, 1, (0, 3, 5)), 9,
                            lambda tree, ix, iy, d, u: np.where(tree == 1, F(0), F(1) - u).astype(F))


@functools.lru_cache(maxsize=None)
def oracle_tree(which):
    t = po.OracleTree()
    t.load(columns(which))
    return t


@functools.lru_cache(maxsize=None)
def gpu_tree(which):
    from practical_path_guiding_lab_amd.sdtree import SDTree
    g = SDTree()
    g.load(columns(which))
    return g


@functools.lru_cache(maxsize=None)
def inputs():
    """Computed once, shared, read-only."""
    p = synth.positions_uniform(N, 5, rs.BB0, rs.BB1)
    special = [[-1, 50, 50], [0, 0, 0], [100, 100, 100], [50, 50, 50], [25, 75, 12.5], [np.nan, 1, 1], [100.00001, 1, 1], [0, 37, 64],
               [12, 100, 3], [50, 0, 100], [1, np.nan, np.nan], [1e30, -1e30, 5], [np.inf, 5, 5], [50, 50, -0.0]]
    p[:, :len(special)] = np.array(special, F).T
    p[:, 3000:3100] += F(150)                                            # a block outside the box
    nrm = synth.directions_uniform(N, 6)
    odd = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [0, 0, 0], [0, 0, -0.0], [-0.0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0],
           [0.5, 0.5, -np.inf], [3, 0, 0], [0, 0, 0.25], [1, 1, 1], [-2, 0.5, -0.125], [np.nan, np.nan, np.nan], [1e-20, 0, 1e-20]]
    nrm[:, 20:20 + len(odd)] = np.array(odd, F).T
    nrm[:, 1000:1100] *= F(3)                                            # non-unit, long and short
    nrm[:, 1100:1200] *= F(0.25)
    # (the specials of p and of the normals meet ordinary partners: they sit in different lanes)
    act = (synth.uniform(N, 7)[0] < 0.85).astype(np.uint8)
    act[[0, 5, 24, 27]] = 1                                              # an outside point, a NaN point, a zero and a NaN normal: served
    act[[1, 21]] = 0
    for a in (p, nrm, act):
        a.setflags(write=False)
    assert (act == 0).sum() > 300 and not np.isfinite(nrm).all()
    return p, nrm, act


@functools.lru_cache(maxsize=None)
def model(which, M, alpha, delta, masked=True):
    """the model's answer (with the candidate arrays and the stream states), computed once and never written to"""
    p, nrm, act = inputs()
    st, inc = po.rng_seed(N, SEED)
    r = rs.resample(oracle_tree(which), p, nrm, st, inc, M, alpha, delta, active=act if masked else None, candidates=True)
    r["state"] = st
    for v in r.values():
        v.setflags(write=False)
    return r


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def run(g, p, nrm, act, M, alpha, delta, candidates, seed=SEED, lane0=0):
    """the device's answer as the model's dict"""
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    n = p.shape[1]
    smp = PCG32Sampler(g, n, seed=seed, lane0=lane0)
    d, w, info = g.resampleCosine(dev(p), dev(nrm), smp, M, alpha, delta, None if act is None else dev(act), return_candidates=candidates)
    out = {"dir": d, "weight": w, "target": info["target"], "source": info["source"], "index": info["index"], "state": smp.state}
    if candidates:
        out.update({k: info[k] for k in rs.CAND_FIELDS})
    out = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in out.items()}
    out["index"], out["state"] = out["index"].view(np.uint32), out["state"].view(np.uint64)
    return out


def without_candidates(r):
    return {k: v for k, v in r.items() if k not in rs.CAND_FIELDS}


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("which", TREES)
def test_equals_the_model(which, M):
    p, nrm, act = inputs()
    g = gpu_tree(which)
    for alpha, delta in PAIRS:
        want = model(which, M, alpha, delta)
        what = "%s M=%d alpha=%g delta=%g" % (which, M, alpha, delta)
        got = run(g, p, nrm, act, M, alpha, delta, True)
        same_bits(got, dict(want), FLAGS, rs.OUT_FIELDS + rs.CAND_FIELDS, what)
        # without the cand_* outputs (the kernel's other instantiation) the common outputs are the same
        got = run(g, p, nrm, act, M, alpha, delta, False)
        same_bits(got, without_candidates(want), FLAGS, rs.OUT_FIELDS, what + ", no candidate arrays")
    # the inputs do what they are there for: lanes that kept and lanes that could not, every candidate slot used
    want = model(which, M, 0.5, 0.1)
    kept = want["index"] != rs.NONE
    assert kept.any() and (~kept & (act != 0)).any()
    if M <= 5:
        assert set(np.unique(want["index"][kept])) == set(range(M))
    assert (want["state"] != po.rng_seed(N, SEED)[0])[act != 0].sum() > N // 2


@pytest.mark.parametrize("which", TREES)
def test_null_mask_serves_every_lane(which):
    p, nrm, _ = inputs()
    want = model(which, 5, 0.5, 0.1, masked=False)
    got = run(gpu_tree(which), p, nrm, None, 5, 0.5, 0.1, True)
    same_bits(got, dict(want), FLAGS, rs.OUT_FIELDS + rs.CAND_FIELDS, which + ", NULL mask")


@pytest.mark.parametrize("candidates", [False, True], ids=["common outputs", "with candidate arrays"])
def test_two_launches_over_halves_give_one_launch(candidates):
    p, nrm, act = inputs()
    g = gpu_tree("golden")
    h = 2050                                                             # (no multiple of a wave: both halves end ragged)
    want = model("golden", 5, 0.5, 0.1)
    fields = rs.OUT_FIELDS + (rs.CAND_FIELDS if candidates else ())
    for lo, hi in ((0, h), (h, N)):
        got = run(g, np.ascontiguousarray(p[:, lo:hi]), np.ascontiguousarray(nrm[:, lo:hi]), np.ascontiguousarray(act[lo:hi]), 5, 0.5, 0.1,
                  candidates, lane0=lo)
        part = {k: np.ascontiguousarray(v[..., lo:hi]) for k, v in want.items() if k in FLAGS + fields}
        same_bits(got, part, FLAGS, fields, "lanes %d..%d" % (lo, hi))


def test_refusals_launch_nothing():
    import torch
    from practical_path_guiding_lab_amd import _native as N_
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler, SDTree
    p, nrm, act = inputs()
    g = gpu_tree("golden")
    L, hd = g._lib, g._h
    dp, dn = dev(p), dev(nrm)
    smp = PCG32Sampler(g, N, seed=SEED)
    state0 = smp.state.clone()
    pre = {k: torch.full(shape, -7.0, device="cuda") for k, shape in (("dir", (3, N)), ("weight", (N,)), ("target", (N,)), ("source", (N,)))}
    pre["index"] = torch.full((N,), 99, dtype=torch.int32, device="cuda")
    good = dict(p=dp.data_ptr(), normal=dn.data_ptr(), rng_state=smp.state.data_ptr(), rng_inc=smp.inc.data_ptr(),
                dir_out=pre["dir"].data_ptr(), weight_out=pre["weight"].data_ptr(), target_out=pre["target"].data_ptr(),
                source_out=pre["source"].data_ptr(), index_out=pre["index"].data_ptr())
    ok = N_.pg_resample_params(5, 0.5, 0.1, 0)
    C = __import__("ctypes")

    def refused(n, prm, args, word):
        rc = L.pg_resample_cosine(hd, n, None if prm is None else C.byref(prm), None if args is None else C.byref(args), None)
        msg = L.pg_last_error(hd)
        assert rc == PG_ERR_INVALID and b"pg_resample_cosine" in msg and word in msg, (rc, msg, word)

    refused(N, None, N_.pg_resample_args(**good), b"NULL params")
    refused(N, ok, None, b"NULL args")
    for missing in ("p", "normal", "rng_state", "rng_inc", "dir_out", "weight_out"):
        refused(N, ok, N_.pg_resample_args(**{k: v for k, v in good.items() if k != missing}), b"NULL pointer")
    for M in (0, 65, 0xFFFFFFFF):
        refused(N, N_.pg_resample_params(M, 0.5, 0.1, 0), N_.pg_resample_args(**good), b"candidates")
    for bad in (-0.001, 1.0000001, float("nan"), float("inf"), -float("inf")):
        refused(N, N_.pg_resample_params(5, bad, 0.1, 0), N_.pg_resample_args(**good), b"alpha")
        refused(N, N_.pg_resample_params(5, 0.5, bad, 0), N_.pg_resample_args(**good), b"delta")
    refused(N, N_.pg_resample_params(5, 0.5, 0.1, 1), N_.pg_resample_args(**good), b"reserved")
    refused(1 << 32, ok, N_.pg_resample_args(**good), b"2^32")
    assert L.pg_resample_cosine(None, N, C.byref(ok), C.byref(N_.pg_resample_args(**good)), None) == PG_ERR_INVALID   # a NULL context
    assert L.pg_resample_cosine(hd, 0, C.byref(ok), C.byref(N_.pg_resample_args()), None) == 0                        # n = 0 does nothing
    with pytest.raises(N_.PgError):
        SDTree().resampleCosine(dp, dn, smp)                                                  # a context that was never configured
    with pytest.raises(N_.PgError) as e:
        g.resampleCosine(dp, dn, smp, candidates=65, return_candidates=True)                  # the Python call refuses alike
    assert e.value.code == PG_ERR_INVALID and "candidates" in str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(smp.state, state0)
    assert all((pre[k] == -7.0).all() for k in ("dir", "weight", "target", "source")) and (pre["index"] == 99).all()
    # ... and the same arguments with nothing wrong are served
    assert L.pg_resample_cosine(hd, N, C.byref(ok), C.byref(N_.pg_resample_args(**good)), None) == 0
    torch.cuda.synchronize()
    assert not torch.equal(smp.state, state0) and (pre["index"] != 99).all()
