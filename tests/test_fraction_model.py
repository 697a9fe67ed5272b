"""The learned BSDF sampling fraction without a GPU: the exports of include/pgsd_fraction.h, the numpy model of its semantics
(tests/fraction_model.py) checked against itself -- order independence, sharding, the direction of learning, the edge rules --
and the resource lines of the new kernels.  There is no tolerance anywhere: the sums are integers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import synth
from abi_table import native  # noqa: F401  (the fixture)
from fraction_model import (EDGE_DROPPED, LOSS_KL, LOSS_VARIANCE, FractionModel, limbs, logistic, salt_with_edges,
                            synthetic_records)
from oracle import pg_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "practical_path_guiding_lab_amd", "csrc")
BB0, BB1 = [0.0] * 3, [100.0] * 3
F = np.float32


@pytest.fixture(scope="module")
def balanced():
    return synth.build_balanced(3, 4)     # 8 KD leaves


@pytest.fixture(scope="module")
def initial():
    t = po.OracleTree()
    t.setup(BB0, BB1, 20, 20, True)
    return t


def test_the_library_exports_the_fraction_entry_points(native):
    # (what every header shares -- the library, the probe build, the counts, the ABI version: tests/test_abi.py)
    hdr = open(os.path.join(ROOT, "include", "pgsd_fraction.h")).read()
    declared = set(re.findall(r"^int\s*(pg_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    assert declared == set(native.EXPORTS_FRACTION) == {
        "pg_fraction_enable", "pg_fraction_query", "pg_fraction_record", "pg_fraction_step", "pg_fraction_accumulators",
        "pg_fraction_export", "pg_fraction_import"}
    assert "#ifndef PGSD_FRACTION_H" in hdr and '#include "pgsd.h"' in hdr
    L = native.lib()
    assert [len(getattr(L, n).argtypes) for n in native.EXPORTS_FRACTION] == [2, 6, 5, 2, 3, 9, 8]
    assert ctypes.sizeof(native.pg_fraction_params) == 28 and ctypes.sizeof(native.pg_fraction_records) == 48
    # a NULL context is refused before anything touches a device
    for n in native.EXPORTS_FRACTION:
        f = getattr(L, n)
        assert f(*([None] + [0 if a is ctypes.c_uint64 else None for a in f.argtypes[1:]])) == -1, n


def _subset(rec, idx):
    return {k: np.ascontiguousarray(v[..., idx]) for k, v in rec.items()}


def _same_state(a, b):
    for k in ("theta", "m", "v", "p1", "p2"):
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(a["steps"], b["steps"])
    np.testing.assert_array_equal(a["acc"], b["acc"])


@pytest.mark.parametrize("loss", [LOSS_KL, LOSS_VARIANCE])
def test_order_and_batching_do_not_change_a_bit(balanced, loss):
    m = 4096
    rec = synthetic_records(m, 11, BB0, BB1)
    salt_with_edges(rec, BB0, BB1, stride=37)
    ref = FractionModel(balanced, loss=loss)
    ref.record(rec)
    words = ref.acc_words()
    assert (words[:, 3] > 0).all() and int(words[:, 3].sum()) < m       # every leaf took records, some were dropped
    ref.step()
    rng = np.random.default_rng(5)
    for batches in (1, 3, 7):
        perm = rng.permutation(m)
        mod = FractionModel(balanced, loss=loss)
        for part in np.array_split(perm, batches):
            mod.record(_subset(rec, part))
        np.testing.assert_array_equal(mod.acc_words(), words)
        mod.step()
        _same_state(mod.state(), ref.state())
    assert (ref.steps == 1).all() and (ref.acc_words() == 0).all() and (ref.theta != 0).all()


def test_four_ranks_that_sum_their_buffers_equal_one(balanced):
    m = 4096
    rec = synthetic_records(m, 21, BB0, BB1)
    one = FractionModel(balanced)
    one.record(rec)
    ranks = [FractionModel(balanced) for _ in range(4)]
    for k, r in enumerate(ranks):
        r.record(_subset(rec, np.arange(k, m, 4)))
    total = sum(r.acc_words() for r in ranks)
    np.testing.assert_array_equal(total, one.acc_words())
    one.step()
    for r in ranks:
        r.acc = [[0, 0, 0, 0] for _ in range(r.n)]
        r.add_words(total)
        r.step()
        _same_state(r.state(), one.state())


def _mixture_records(rng, f, n, product_follows_guide):
    """A 1-D stand-in for a bounce: directions x in [0,1), bsdf_pdf uniform (1), guide_pdf(x) = 2x.  x is drawn from the mixture
    f * bsdf + (1 - f) * guide and wo_pdf is that mixture's density."""
    from_bsdf = rng.random(n) < f
    x = np.where(from_bsdf, rng.random(n), np.sqrt(rng.random(n)))
    b = np.ones(n, F)
    g = (2.0 * x).astype(F)
    wo = (F(f) * b + (F(1) - F(f)) * g).astype(F)
    pr = g.copy() if product_follows_guide else b.copy()
    p = np.full((3, n), 50.0, F)
    return {"position": p, "bsdf_pdf": b, "guide_pdf": g, "product": pr, "wo_pdf": wo, "is_delta": None}


@pytest.mark.parametrize("loss", [LOSS_KL, LOSS_VARIANCE])
@pytest.mark.parametrize("follows_guide", [True, False])
def test_the_fraction_moves_towards_the_better_sampler(initial, loss, follows_guide):
    """The sign, not a rate: where the integrand is proportional to the guiding density the fraction falls below 0.5, where it is
    proportional to the BSDF's it rises -- within 50 steps at learning rate 0.1, for both losses."""
    mod = FractionModel(initial, learning_rate=0.1, loss=loss)
    rng = np.random.default_rng(1234)
    for _ in range(50):
        f = float(logistic(mod.theta[0])[0])
        mod.record(_mixture_records(rng, f, 2048, follows_guide))
        assert mod.acc[0][3] == 2048
        mod.step()
    theta, frac = mod.theta[0], logistic(mod.theta[0])[0]
    assert mod.steps[0] == 50
    if follows_guide:
        assert theta < mod.theta0 and frac < 0.5, (theta, frac)
    else:
        assert theta > mod.theta0 and frac > 0.5, (theta, frac)


def test_edge_rules(balanced):
    m = 2048
    rec = synthetic_records(m, 31, BB0, BB1)
    kinds = salt_with_edges(rec, BB0, BB1)
    mod = FractionModel(balanced)
    kept, leaf, g = mod.gradients(rec)
    for k in set(kinds):
        sel = kinds == k
        assert sel.any()
        assert (kept[sel] == (k not in EDGE_DROPPED)).all(), k
    mod.record(rec)
    words = mod.acc_words()
    assert int(words[:, 3].sum()) == int(kept.sum()) == m - sum(int((kinds == k).sum()) for k in EDGE_DROPPED)
    # a kept record whose quantised gradient is zero still counts
    zero = [i for i in np.nonzero(kinds == "zero product")[0]] + [i for i in np.nonzero(kinds == "tiny gradient")[0]]
    assert all(w == (0, 0, 0) for w in limbs(g[zero])) and kept[zero].all()
    only = FractionModel(balanced)
    only.record({k: np.ascontiguousarray(v[..., zero]) for k, v in rec.items()})
    w0 = only.acc_words()
    assert (w0[:, :3] == 0).all() and int(w0[:, 3].sum()) == len(zero)
    # the clamp of quantize: a huge gradient adds +-2^88, whatever its size
    huge = np.nonzero(kinds == "huge gradient")[0]
    assert all(abs(w[2]) == 1 << 24 and w[0] == 0 and w[1] == 0 for w in limbs(g[huge]))
    # a dropped record changes nothing: the same set without them gives the same words
    clean = FractionModel(balanced)
    clean.record({k: np.ascontiguousarray(v[..., np.nonzero(kept)[0]]) for k, v in rec.items()})
    np.testing.assert_array_equal(clean.acc_words(), words)
    # d_count: only the first records are taken
    head = FractionModel(balanced)
    head.record(rec, count=700)
    assert int(head.acc_words()[:, 3].sum()) == int(kept[:700].sum())


def test_the_theta_clamp_and_untouched_leaves(balanced):
    # (beyond |theta| ~ 16.6 the fp32 logistic is exactly 0 or 1 and f (1 - f) = 0: start inside that, one big step leaves [-20, 20])
    mod = FractionModel(balanced, learning_rate=5.0, l2=0.0, epsilon=1e-12)
    st = mod.state()
    st["theta"][:] = [16.0, -16.0, 16.0, -16.0, 0.25, -0.5, 1.0, 2.0]
    st["m"][4:] = 0.125
    st["steps"][4:] = 7
    mod.load_state(st)
    before = mod.state()
    # leaves 0..3 take records that push them over the clamp; leaves 4..7 take none
    centres = {}
    p = synth.positions_uniform(4096, 41, BB0, BB1)
    leaf = mod.leaf_of(p, mod.inside(p))
    for t in range(4):
        centres[t] = p[:, np.nonzero(leaf == t)[0][:64]]
    for t in range(4):
        n = centres[t].shape[1]
        up = t % 2 == 0          # theta rises where the gradient is negative: bsdf_pdf > guide_pdf, product > 0
        rec = {"position": centres[t], "bsdf_pdf": np.full(n, 2.0 if up else 0.5, F), "guide_pdf": np.full(n, 0.5 if up else 2.0, F),
               "product": np.ones(n, F), "wo_pdf": np.ones(n, F), "is_delta": None}
        mod.record(rec)
    mod.step()
    after = mod.state()
    np.testing.assert_array_equal(after["theta"][:4], np.array([20, -20, 20, -20], F))
    assert (after["steps"][:4] == 1).all()
    for k in ("theta", "m", "v", "p1", "p2", "steps"):
        np.testing.assert_array_equal(after[k][4:], before[k][4:], err_msg=k)
    assert (after["acc"] == 0).all()
    np.testing.assert_array_equal(logistic(np.array([0.0], F)), np.array([0.5], F))


def test_resource_lines_of_the_fraction_kernels():
    path = os.path.join(CSRC, "pg_kernels_fraction.remarks")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", CSRC, "-j4"], check=True, capture_output=True)
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        mm = re.search(r"remark: Function Name: (\S+)", line)
        if mm:
            cur = kernels.setdefault(mm.group(1), {})
            continue
        for key, pat in (("vgprs", r"remark:\s+VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            mm = re.search(pat, line)
            if mm and cur is not None:
                cur[key] = int(mm.group(1))
    names = {next(w for w in ("k_fraction_query", "k_fraction_record", "k_fraction_step", "k_fraction_carry", "k_fraction_init")
                  if w in k): v for k, v in kernels.items()}
    assert set(names) == {"k_fraction_query", "k_fraction_record", "k_fraction_step", "k_fraction_carry", "k_fraction_init"}
    assert all(v["scratch"] == 0 for v in names.values()), names       # (the rule tests/test_resources.py holds every kernel to)
    assert names["k_fraction_query"]["vgprs"] <= 64 and names["k_fraction_query"]["occupancy"] == 8, names["k_fraction_query"]
