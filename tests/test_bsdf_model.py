"""The BSDF layer pinned to the published formulas: the CPU oracle's bsdf_eval_pdf and bsdf_sample for whole arrays
(pgo_bsdf_probe) against tests/bsdf_model.py, a float64 model with a band derived from the float32 roundings and the
conditioning of each quantity, on the input sets of tests/bsdf_sets.py.  The device is compared with the oracle bit for bit
in tests/test_gpu_bsdf.py, so what holds here holds for it -- and the same checks run there on the device's own numbers.

Measured on the oracle (python tests/test_bsdf_model.py prints the table kept in profiles/bsdf/band.txt): the worst ratio of
|difference| to the band's bracket is 1.249 / 1.252 (value, pdf: the mirror set, alpha = 1e-3), 1.088 (a sampled direction's
pdf: horizon_wo) and 1.426 (a delta lobe's pdf, 1 - F: the equal set); four times that is bsdf_model.BAND_C
(test_band_constants_are_four_times_what_is_measured), far below the 64 at which the bracket would have to be missing
something.  Ambiguous shares: at most 0.20 % of the broad sets and 1.79 % of u_edges (cap 2 %); the two sets aimed at a
branch on purpose reach 7.67 % (grazing, its sampled directions: the normals of alpha = 1e-3, whose D no float32 input
determines) and 5.91 % (critical: half its angles are within float32 of the critical one) and are held to those figures
rounded up (bsdf_sets.NARROW).

The density test pushes a 300 x 300 grid of 2-D samples (the lobe sample from the golden-ratio sequence) through the
sampler and compares the histogram over 12 x 24 bins of (cos theta, phi) with the model's pdf integrated over each bin:
worst bin 9.25e-4 of all samples, worst difference between the valid fraction and the pdf's mass 3.63e-3 (Beckmann at
grazing incidence: the sampler inverts the exact visible-normal distribution, the pdf uses the rational fit of G1, and
their masses differ by that much); twice those are the tolerances.  profiles/bsdf/mutations.txt: what ten deliberate
errors in a scratch copy of the oracle do to these tests."""
import functools
import math

import numpy as np
import pytest

import bsdf_model as BM
import bsdf_sets as BS
from oracle import pg_oracle as po

BIN_TOLERANCE = 2 * 9.3e-4     # of all samples, per bin: twice the oracle's worst (rc beckmann, grazing)
MASS_TOLERANCE = 2 * 3.7e-3    # valid fraction against the pdf's mass: twice the oracle's worst (the same pair)
GRID, BINS_C, BINS_P = 300, 12, 24
NAMES = ("value", "pdf", "sampled_wo", "sampled_pdf", "weight", "eta", "delta")


@functools.lru_cache(maxsize=None)
def oracle(name, level=3):
    """the oracle's outputs on a set: computed once, shared, never changed"""
    idx, wi, wo, u = BS.get(name)
    out = po.bsdf_probe(BS.table()[0], idx, wi, wo, u, level)
    for a in out:
        a.setflags(write=False)
    return out


def check_finite(out, what=""):
    """for finite inputs no output is NaN or infinite; pdfs and weights are not negative"""
    for name, a in zip(NAMES, out):
        assert np.isfinite(a).all(), "%s: %s not finite at lanes %s" % (what, name, np.nonzero(~np.isfinite(a).reshape(a.shape[0], -1).all(-1))[0][:8])
    assert (out[1] >= 0).all() and (out[3] >= 0).all() and (out[4] >= 0).all() and (out[0] >= 0).all(), what


@functools.lru_cache(maxsize=None)
def oracle_verdicts(name, level=3):
    """the model's verdicts on the oracle's outputs: computed once, shared"""
    return judge(name, oracle(name, level), level)


def judge(name, out, level=3):
    """-> the model's verdicts on the eval and the sample outputs of a set"""
    rows = BS.table()[0]
    idx, wi, wo, u = BS.get(name)
    return (BM.judge_eval(rows, idx, wi, wo, out[0], out[1], level),
            BM.judge_sample(rows, idx, wi, u, out[2], out[3], out[4], out[5], out[6], level))


def check_against_model(name, out, level=3, what="oracle"):
    rows = BS.table()[0]
    idx, wi, wo, u = BS.get(name)
    cap = BS.NARROW.get(name, BM.AMBIGUOUS_CAP)
    print("%s: %d lanes within reach of sincos_phi's switch" % (name, BM.phi_switch(rows, idx, wi).sum()))
    for tag, v in zip(("eval", "sample"), oracle_verdicts(name, level) if what == "oracle" else judge(name, out, level)):
        worst = {k: float(r.max()) for k, r in v.ratio.items()}
        print("%s %s level %d %s: %d lanes, ambiguous %.2f %% (cap %.0f %%) %s, worst |difference| / bracket %s"
              % (what, name, level, tag, idx.shape[0], 100 * v.ambiguous.mean(), 100 * cap, v.why, {k: round(r, 2) for k, r in worst.items()}))
        bad = v.failures()
        assert bad.size == 0, "%s %s %s: neither in the band nor one of the branch answers: lanes %s, first: row %s wi %s wo %s u %s -> %s" % (
            what, name, tag, bad[:8], rows[idx[bad[0]]][:12], wi[bad[0]], wo[bad[0]], u[bad[0]], [a[bad[0]] for a in out])
        assert v.ambiguous.mean() <= cap, (name, tag, v.ambiguous.mean())


@pytest.mark.parametrize("name", list(BS.SETS))
def test_oracle_against_the_model(name):
    out = oracle(name)
    check_finite(out, name)
    check_against_model(name, out)


def rows_as_level_reads_them(level):
    """the table rewritten so that a level 3 kernel computes what a kernel of `level` makes of the original"""
    rows = BS.table()[0].copy()
    if level < 3:
        rows[:, 11] = 0.0
        rows[rows[:, 0] >= BM.CONDUCTOR, 0] = BM.DIFFUSE
    if level < 1:
        rows[:, 0] = BM.DIFFUSE
    return rows


@pytest.mark.parametrize("level", [0, 1, 2])
def test_lower_feature_levels(level):
    """level 0 treats every row as a two-sided diffuse material; roughconductor rows are honoured from level 1, one-sided
    rows and the types from the smooth conductor on from level 3 only: exactly the level 3 answers for the rewritten table,
    and the model's for that level"""
    for name in ("uniform", "axes"):
        out = oracle(name, level)
        idx, wi, wo, u = BS.get(name)
        want = po.bsdf_probe(rows_as_level_reads_them(level), idx, wi, wo, u, 3)
        for k, a, b in zip(NAMES, out, want):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg="%s level %d: %s" % (name, level, k))
        check_finite(out, name)
        check_against_model(name, out, level)
    if level == 0:  # nothing but diffuse: no delta lobe, eta 1 wherever a sample succeeded
        assert not out[6].any() and (out[5][out[3] > 0] == 1).all()


def check_zeros(out, name):
    """an index ratio of exactly 1 on a rough dielectric and wi exactly on the horizon give zeros, all outputs (the smooth
    dielectric alone has an answer on the horizon: the mirror direction with probability 1)"""
    rows = BS.table()[0]
    idx, wi, wo, u = BS.get(name)
    kind = rows[idx, 0]
    no_interface = (kind == BM.ROUGH_DIELECTRIC) & (rows[idx, 5] == 1.0)
    horizon = (wi[:, 2] == 0.0) & (kind != BM.DIELECTRIC)
    one_sided_behind = (rows[idx, 11] != 0) & (wi[:, 2] < 0) & (kind < BM.DIELECTRIC)
    for what, sel in (("eta == 1", no_interface), ("wi.z == 0", horizon), ("one-sided from behind", one_sided_behind)):
        for k, a in zip(NAMES, out):
            assert not a[sel].any(), "%s, %s: %s is not zero" % (name, what, k)
    return no_interface.sum(), horizon.sum(), one_sided_behind.sum()


def test_zeros_where_there_is_no_answer():
    counts = np.zeros(3, int)
    for name in BS.SETS:
        counts += check_zeros(oracle(name), name)
    assert (counts > 500).all(), counts   # the sets do hold such lanes


# ---- sampling density, deterministic ------------------------------------------------------------------------------------------
def find_row(kind, alpha=0.0, eta=None, conductor=None, one_sided=None):
    rows = BS.table()[0]
    for i, r in enumerate(rows):
        if r[0] != kind or r[4] != np.float32(alpha):
            continue
        if eta is not None and r[5] != np.float32(eta):
            continue
        if conductor is not None and r[5] != np.float32(BS.CONDUCTORS[conductor][0][0]):
            continue
        if one_sided is not None and bool(r[11]) != one_sided:
            continue
        return i
    raise KeyError((kind, alpha, eta, conductor))


def wi_at(cos_theta, phi=0.3):
    s = math.sqrt(1.0 - cos_theta * cos_theta)
    return np.array([s * math.cos(phi), s * math.sin(phi), cos_theta], np.float32)


ACRYLIC = BS.ETAS[0]
PAIRS = {   # row, wi, is the lobe sample used
    "beckmann conductor, 45 degrees": (lambda: find_row(BM.ROUGH_CONDUCTOR, 0.5, conductor="veach-mis"), wi_at(math.cos(math.radians(45))), False),
    "ggx conductor, 60 degrees": (lambda: find_row(BM.ROUGH_CONDUCTOR, -0.5, conductor="Al"), wi_at(0.5), False),
    "ggx conductor alpha 0.1, 30 degrees": (lambda: find_row(BM.ROUGH_CONDUCTOR, -0.1, conductor="Al"), wi_at(math.cos(math.radians(30))), False),
    "beckmann conductor, grazing (cos 0.05)": (lambda: find_row(BM.ROUGH_CONDUCTOR, 0.5, conductor="veach-mis"), wi_at(0.05), False),
    "beckmann glass from outside, 40 degrees": (lambda: find_row(BM.ROUGH_DIELECTRIC, 0.5, eta=ACRYLIC), wi_at(math.cos(math.radians(40))), True),
    "ggx glass from inside, 30 degrees": (lambda: find_row(BM.ROUGH_DIELECTRIC, -0.5, eta=ACRYLIC), wi_at(-math.cos(math.radians(30))), True),
    "beckmann glass from the dense side, past the critical angle": (lambda: find_row(BM.ROUGH_DIELECTRIC, 0.5, eta=BS.ETAS[1]), wi_at(math.cos(math.radians(50))), True),
    "one-sided diffuse, 30 degrees": (lambda: find_row(BM.DIFFUSE, one_sided=True), wi_at(math.cos(math.radians(30))), False),
}


def density_inputs(pair, grid=GRID):
    """the grid of samples of a pair: cell centres of grid x grid for the 2-D sample; the lobe sample runs through the
    golden-ratio sequence (equidistributed against the grid) where the row has two lobes, and is 0.5 otherwise"""
    row, wi, lobes = PAIRS[pair]
    g = (np.arange(grid) + 0.5) / grid
    uv = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    n = uv.shape[0]
    u0 = np.mod((np.arange(n) + 0.5) * 0.6180339887498949, 1.0) if lobes else np.full(n, 0.5)
    u = np.concatenate([u0[:, None], uv], 1).astype(np.float32)
    return np.full(n, row(), np.int32), np.ascontiguousarray(np.tile(wi, (n, 1))), u


def histogram(swo, spdf, weight, n):
    """the share of all n samples in every (cos theta, phi) bin; a failed sample and one of weight 0 carry nothing"""
    ok = (spdf > 0) & (weight > 0).any(-1)
    d = swo[ok].astype(np.float64)
    c = d[:, 2] / np.sqrt((d * d).sum(-1))
    p = np.arctan2(d[:, 1], d[:, 0])
    ic = np.clip(((c + 1) / 2 * BINS_C).astype(int), 0, BINS_C - 1)
    ip = np.clip(((p + np.pi) / (2 * np.pi) * BINS_P).astype(int), 0, BINS_P - 1)
    h = np.zeros((BINS_C, BINS_P))
    np.add.at(h, (ic, ip), 1.0)
    return h / n


@functools.lru_cache(maxsize=None)
def model_mass(pair, sub=24):
    """the model's pdf integrated over every bin (midpoint rule, sub x sub points a bin; d omega = d cos theta d phi)"""
    row, wi, _ = PAIRS[pair]
    rows = BS.table()[0]
    cs = (np.arange(BINS_C * sub) + 0.5) / (BINS_C * sub) * 2 - 1
    ps = (np.arange(BINS_P * sub) + 0.5) / (BINS_P * sub) * 2 * np.pi - np.pi
    C, P = np.meshgrid(cs, ps, indexing="ij")
    s = np.sqrt(1 - C * C)
    d = np.stack([s * np.cos(P), s * np.sin(P), C], -1).reshape(-1, 3).astype(np.float32)
    idx = np.full(d.shape[0], row(), np.int32)
    kind, one_sided = BM.effective_rows(rows, idx, 3)
    q, _ = BM.eval_core(BM.pack(rows, idx, np.tile(wi, (d.shape[0], 1)), d), kind, one_sided)
    return q["pdf"].reshape(BINS_C, sub, BINS_P, sub).sum((1, 3)) * (2.0 / (BINS_C * sub)) * (2 * np.pi / (BINS_P * sub))


def density_differences(pair, probe, grid=GRID):
    """-> (worst bin difference, |valid fraction - pdf mass|) of a sampler: probe(rows, idx, wi, wo, u) -> the seven outputs"""
    idx, wi, u = density_inputs(pair, grid)
    n = idx.shape[0]
    swo, spdf, weight = [], [], []
    for a in range(0, n, 1 << 16):
        out = probe(BS.table()[0], idx[a:a + 65536], wi[a:a + 65536], wi[a:a + 65536], u[a:a + 65536])
        swo.append(np.asarray(out[2])), spdf.append(np.asarray(out[3])), weight.append(np.asarray(out[4]))
    h = histogram(np.concatenate(swo), np.concatenate(spdf), np.concatenate(weight), n)
    m = model_mass(pair)
    return float(np.abs(h - m).max()), float(abs(h.sum() - m.sum()))


@pytest.mark.parametrize("pair", list(PAIRS))
def test_sampling_density(pair):
    worst, mass = density_differences(pair, po.bsdf_probe)
    print("%s: worst bin %.2e (tolerance %.2e), valid fraction against the pdf's mass %.2e (tolerance %.2e)" % (pair, worst, BIN_TOLERANCE, mass, MASS_TOLERANCE))
    assert worst <= BIN_TOLERANCE and mass <= MASS_TOLERANCE


# ---- the model's own sanity --------------------------------------------------------------------------------------------------
def _model_value(row, wi, wo):
    rows = BS.table()[0]
    idx = np.full(wi.shape[0], row, np.int32)
    kind, one_sided = BM.effective_rows(rows, idx, 3)
    return BM.eval_core(BM.pack(rows, idx, wi, wo), kind, one_sided)[0]


def test_model_conductor_lobes_are_reciprocal():
    rng = np.random.default_rng(3)
    n = 2000
    wi, wo = (np.abs(BS._sphere(rng, n)).astype(np.float32) * np.array([1, -1, 1], np.float32) for _ in range(2))
    for row in BS.table()[1]["rough_conductor"]:
        a, b = _model_value(row, wi, wo)["value"], _model_value(row, wo, wi)["value"]
        # value = f cos(theta_o): f(wi, wo) = f(wo, wi)
        np.testing.assert_allclose(a * wi[:, 2:3].astype(np.float64), b * wo[:, 2:3].astype(np.float64), rtol=1e-8, atol=1e-300)  # (float64 itself: exp(-tan^2 / alpha^2) at alpha = 1e-3)


def test_model_albedo_is_at_most_one():
    sub = 16
    cs = (np.arange(BINS_C * sub) + 0.5) / (BINS_C * sub) * 2 - 1
    ps = (np.arange(BINS_P * sub) + 0.5) / (BINS_P * sub) * 2 * np.pi - np.pi
    C, P = np.meshgrid(cs, ps, indexing="ij")
    s = np.sqrt(1 - C * C)
    d = np.stack([s * np.cos(P), s * np.sin(P), C], -1).reshape(-1, 3).astype(np.float32)
    dw = (2.0 / cs.size) * (2 * np.pi / ps.size)
    rows, groups = BS.table()
    for row in np.concatenate([groups["diffuse"], groups["rough"]]):
        if abs(rows[row, 4]) not in (0.0, np.float32(0.5), np.float32(1.0)):
            continue  # (the sharper lobes need a finer rule than this test is worth)
        for cz in (0.95, 0.5, -0.7):
            v = _model_value(row, np.tile(wi_at(cz), (d.shape[0], 1)), d)["value"]
            albedo = v.sum(0) * dw
            # rough glass under radiance transport carries 1 / eta^2 across: the bound is for the energy, eta^2 * radiance
            if rows[row, 0] == BM.ROUGH_DIELECTRIC:
                e = float(rows[row, 5]) if cz > 0 else 1.0 / float(rows[row, 5])
                below = (d[:, 2] * cz < 0)
                albedo = (v[~below].sum(0) + v[below].sum(0) * e * e) * dw
            # (1 + the 0.35 % by which the fit of the Beckmann G1 may exceed the exact one, and the rule's own error)
            assert (albedo <= 1.0 + 5e-3).all(), (row, cz, albedo)


def test_model_fresnel_limits():
    for eta, k, _ in BS.CONDUCTORS.values():
        eta, k = np.array(eta), np.array(k)
        normal = ((eta - 1) ** 2 + k ** 2) / ((eta + 1) ** 2 + k ** 2)
        np.testing.assert_allclose(BM.fresnel_conductor(np.ones(3), eta, k), normal, rtol=1e-13)
        np.testing.assert_allclose(BM.fresnel_conductor(np.zeros(3), eta, k), 1.0, rtol=1e-13)
    for eta in BS.ETAS[:3]:
        for side in (1.0, -1.0):
            F, ct, eta_it = BM.fresnel_dielectric(np.array([side]), np.array([eta]))
            np.testing.assert_allclose(F, ((eta - 1) / (eta + 1)) ** 2, rtol=1e-13)
            assert ct[0] == -side and eta_it[0] == (eta if side > 0 else 1 / eta)
        F, _, _ = BM.fresnel_dielectric(np.array([1e-9, -1e-9, 0.0]), np.full(3, eta))
        np.testing.assert_allclose(F, 1.0, atol=1e-7)
        # Brewster's angle: no p-polarised reflection, so F = r_s^2 / 2
        cb = math.cos(math.atan(eta))
        F, ct, _ = BM.fresnel_dielectric(np.array([cb]), np.array([eta]))
        r_s = (cb - eta * -ct[0]) / (cb + eta * -ct[0])
        np.testing.assert_allclose(F, 0.5 * r_s * r_s, rtol=1e-12)
    # a dielectric is a conductor without absorption
    c = np.linspace(0.01, 1, 50)
    np.testing.assert_allclose(BM.fresnel_conductor(c, 1.5, 0.0), BM.fresnel_dielectric(c, np.full(50, 1.5))[0], rtol=1e-12)
    # total internal reflection from the dense side
    F, ct, _ = BM.fresnel_dielectric(np.array([-0.7]), np.array([1.5]))
    assert F[0] == 1.0 and ct[0] == 0.0


def test_model_beckmann_fit_against_the_exact_g1():
    """Walter et al. give the rational fit a relative error below 0.35 %; at the switch, where the fit is replaced by 1, the
    exact G1 is 0.9982"""
    a = np.linspace(1e-3, 1.6, 4000, endpoint=False)
    assert np.abs(BM.g1_beckmann_fit(a) / BM.g1_beckmann_exact(a) - 1).max() < 3.5e-3
    b = np.linspace(1.6, 20, 2000)
    exact = BM.g1_beckmann_exact(b)
    assert (exact <= 1 + 1e-15).all() and (1 - exact).max() < 2e-3 and abs(exact[0] - 0.9982) < 1e-4


def test_band_constants_are_four_times_what_is_measured():
    """C of every kind of quantity is four times the oracle's worst ratio over all sets, rounded up to a tenth: a drift of
    that ratio in either direction is noticed"""
    worst = {}
    for name in BS.SETS:
        for v in oracle_verdicts(name):
            for k, r in v.ratio.items():
                worst[k] = max(worst.get(k, 0.0), float(r.max()))
    kinds = {"value": ("value",), "pdf": ("pdf",), "sample": ("sample_pdf", "sample_value", "weightless_pdf"),
             "delta": ("delta_wo", "delta_pdf", "delta_weight", "delta_eta", "delta_delta")}
    assert set(worst) == {q for names in kinds.values() for q in names}
    for kind, names in kinds.items():
        four = 4 * max(worst[q] for q in names)
        print("%s: 4 x %.3f = %.3f, C = %.1f" % (kind, four / 4, four, BM.BAND_C[kind]))
        assert four <= BM.BAND_C[kind] <= four + 0.1
    assert max(BM.BAND_C.values()) <= 64 and BM.BRANCH_C == 64


if __name__ == "__main__":  # the table of profiles/bsdf/band.txt
    worst = {}
    for name in BS.SETS:
        out = oracle(name)
        for tag, v in zip(("eval", "sample"), judge(name, out)):
            r = {k: float(x.max()) for k, x in v.ratio.items()}
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
            print("%-10s %-6s %6d lanes  ambiguous %5.2f %%  %s  %s" % (name, tag, out[1].shape[0], 100 * v.ambiguous.mean(),
                                                                        " ".join("%s %.2f" % kv for kv in r.items()), v.why))
    print("worst ratio of |difference| to the bracket:", {k: round(x, 3) for k, x in worst.items()})
    for pair in PAIRS:
        print("density  %-62s worst bin %.2e  valid fraction - mass %.2e" % ((pair,) + density_differences(pair, po.bsdf_probe)))
