"""The device's BSDF layer by itself (pg_bsdf_probe: load_material, bsdf_eval_pdf<> and bsdf_sample<> of
csrc/pg_render_dev.hpp, the functions the render kernels call) against the CPU oracle's (pgo_bsdf_probe) bit for bit, on
the input sets of tests/bsdf_sets.py -- angles, roughnesses and random numbers a render pass meets only by chance -- at
every feature level, and against the float64 model of tests/bsdf_model.py directly, so that a change moving oracle and
device together still fails a test."""
import functools

import numpy as np
import pytest

import bsdf_model as BM
import bsdf_sets as BS
import probe_harness as H
import test_bsdf_model as TB

pytestmark = pytest.mark.gpu


def probe(rows, idx, wi, wo, u, level=3):
    out = H.bare_context().bsdfProbe(H.dev(rows), H.dev(idx), H.dev(wi), H.dev(wo), H.dev(u), level)
    return tuple(o.cpu().numpy() for o in out)


@functools.lru_cache(maxsize=None)
def device(name, level=3):
    """the device's outputs on a set: computed once, shared, never changed"""
    return probe(BS.table()[0], *BS.get(name), level=level)


def _same(dev, ora, what):
    """the seven outputs of the device and of the oracle: every bit, a NaN's included"""
    H.same_bits(dict(zip(TB.NAMES, dev)), dict(zip(TB.NAMES, ora)), (), TB.NAMES, what, any_nan=False)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(BS.SETS))
def test_device_equals_oracle(name, level):
    _same(device(name, level), TB.oracle(name, level), "%s level %d" % (name, level))


def test_sizes_that_are_no_multiple_of_the_workgroup():
    rows = BS.table()[0]
    idx, wi, wo, u = BS.get("uniform")
    ora = TB.oracle("uniform")
    for n in (1, 63, 64, 65, 255, 257, 4097):
        _same(probe(rows, idx[:n], wi[:n], wo[:n], u[:n]), H.first(ora, n), "uniform, %d lanes" % n)
    one = rows[idx[:777]]   # a table of one row per lane, and a table of one row
    _same(probe(one, np.arange(777, dtype=np.int32), wi[:777], wo[:777], u[:777]), [a[:777] for a in ora], "a row per lane")
    k = int(idx[0])
    lanes = np.nonzero(idx == k)[0]
    _same(probe(rows[k:k + 1], np.zeros(lanes.size, np.int32), wi[lanes], wo[lanes], u[lanes]), [a[lanes] for a in ora], "one row")


@pytest.mark.parametrize("name", list(BS.SETS))
def test_device_against_the_model(name):
    out = device(name)
    TB.check_finite(out, name)
    TB.check_zeros(out, name)
    TB.check_against_model(name, out, what="device")


@pytest.mark.parametrize("level", [0, 1, 2])
def test_lower_feature_levels_against_the_model(level):
    out = device("uniform", level)
    TB.check_finite(out, "uniform")
    TB.check_against_model("uniform", out, level, what="device")
    _same(out, probe(TB.rows_as_level_reads_them(level), *BS.get("uniform"), level=3), "level %d as level 3 reads the rewritten table" % level)


def test_sampling_density_of_one_pair():
    """the device's samples are the oracle's bit for bit (above), so one pair confirms the plumbing: 256 x 256 samples, one call"""
    pair = "beckmann conductor, 45 degrees"
    worst, mass = TB.density_differences(pair, probe, grid=256)
    want = TB.density_differences(pair, TB.po.bsdf_probe, grid=256)
    print("%s, 256 x 256: worst bin %.2e, valid fraction against the pdf's mass %.2e" % (pair, worst, mass))
    assert (worst, mass) == want and worst <= TB.BIN_TOLERANCE and mass <= TB.MASS_TOLERANCE


def test_misuse_is_refused_with_a_message():
    import torch
    from practical_path_guiding_lab_amd import _native as N
    L = N.lib()
    h = H.bare_context()._h
    rows = torch.from_numpy(BS.table()[0]).cuda()
    n_mat = rows.shape[0]
    f3 = lambda: torch.full((16, 3), 0.5, dtype=torch.float32, device="cuda")
    f1 = lambda: torch.zeros(16, dtype=torch.float32, device="cuda")
    idx = torch.zeros(16, dtype=torch.int32, device="cuda")
    wi, wo, u, value, pdf, swo, spdf, weight, eta = f3(), f3(), f3(), f3(), f1(), f3(), f1(), f3(), f1()
    delta = torch.zeros(16, dtype=torch.int32, device="cuda")

    def args(n=16, n_mat=n_mat, rows=rows, idx=idx, level=3):
        return [h, n, n_mat, rows.data_ptr(), idx.data_ptr(), wi.data_ptr(), wo.data_ptr(), u.data_ptr(), level, value.data_ptr(),
                pdf.data_ptr(), swo.data_ptr(), spdf.data_ptr(), weight.data_ptr(), eta.data_ptr(), delta.data_ptr(), None]

    def refused(a, word):
        rc = L.pg_bsdf_probe(*a)
        assert rc < 0 and word in L.pg_last_error(h).decode(), (rc, L.pg_last_error(h))

    assert L.pg_bsdf_probe(*args()) == 0           # needs no scene: this context never had one
    assert L.pg_bsdf_probe(None, *args()[1:]) < 0
    for k in (3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15):
        a = args()
        a[k] = None
        refused(a, "NULL")
    refused(args(n=(1 << 20) + 1), "2^20")
    refused(args(level=4), "level")
    refused(args(level=-1), "level")
    refused(args(n_mat=0), "material rows")
    past, negative = (torch.full((16,), v, dtype=torch.int32, device="cuda") for v in (n_mat, -1))
    refused(args(idx=past), "outside the table")
    refused(args(idx=negative), "outside the table")
    for column, bad, word in ((0, 5.0, "unknown material type"), (0, 0.5, "unknown material type"), (4, 0.0, "alpha"),
                              (4, float("nan"), "alpha"), (5, 0.0, "index ratio"), (5, -1.5, "index ratio")):
        r = rows.clone()
        k = int(np.nonzero(BS.table()[0][:, 0] == BM.ROUGH_DIELECTRIC)[0][0])
        r[k, column] = bad
        refused(args(rows=r), word)
    a = args(n=0)
    a[3:8] = [None] * 5
    assert L.pg_bsdf_probe(*a) == 0                # n == 0: nothing is read
    assert L.pg_bsdf_probe(*args()) == 0           # ... and a refusal leaves the context usable
