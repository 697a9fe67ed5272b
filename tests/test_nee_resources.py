"""What the compiler made of pg_kernels_nee.hip (csrc/*.remarks, no GPU needed).  k_nee_resample has k_lights_sample's descent and
k_resample_cosine's loop, so: no scratch, and of LDS the staged KD planes only, k_lights_sample's.  Without the candidate stores it
takes 63 registers and reaches eight waves per SIMD, with them 71 and seven; no launch bound asks for either.
The floor below is what profiles/nee/resource_usage.txt records for this build.  And every kernel the parent commit had keeps its
resource line -- the seven k_lights_* kernels among them, whose SELECT and PMF moved into pg_lights_dev.hpp:
resource_usage_parent.txt against resource_usage.txt."""
import os

from test_resample_lobe_resources import _recorded
from test_resources import ROOT, kernels  # noqa: F401  (the fixture: the resource report of every kernel of the build)

PROFILE = os.path.join(ROOT, "profiles", "nee")
NEW = ("pg::k_nee_prepare", "pg::k_nee_resample<false>", "pg::k_nee_resample<true>")
SAMPLE = "pg::k_lights_sample"
COLUMNS = ("vgprs", "sgprs", "scratch", "occupancy", "lds")


def test_the_three_kernels_without_scratch_and_with_the_samples_lds(kernels):  # noqa: F811
    ne = {k: v for k, v in kernels.items() if k.startswith("pg::k_nee_")}
    assert sorted(ne) == sorted(NEW), sorted(kernels)
    recorded = _recorded(os.path.join(PROFILE, "resource_usage.txt"))
    for k, v in ne.items():
        assert v["file"] == "pg_kernels_nee.remarks"
        assert v["scratch"] == 0, (k, v)
        floor = int(dict(zip(COLUMNS, recorded[k]))["occupancy"])
        assert floor >= 7 and v["occupancy"] >= floor, (k, v, floor)
    for k in NEW[1:]:
        assert ne[k]["lds"] == kernels[SAMPLE]["lds"] > 0, (k, ne[k], kernels[SAMPLE])   # the staged KD planes, nothing else
    assert ne[NEW[0]]["lds"] == 0
    # the names keep clear of the prefixes the resource tests of 5.22 to 5.25 pin to their own sets
    for prefix in ("pg::k_lights_", "pg::k_resample_cosine<", "pg::k_resample_lobe<", "pg::k_resample_interface<"):
        assert not any(k.startswith(prefix) for k in ne)


def test_every_parent_kernel_keeps_its_resource_lines(kernels):  # noqa: F811
    parent, now = _recorded(os.path.join(PROFILE, "resource_usage_parent.txt")), _recorded(os.path.join(PROFILE, "resource_usage.txt"))
    assert len(parent) > 80 and SAMPLE in parent and "pg::k_resample_cosine<false>" in parent and "pg::k_pdf" in parent
    assert sorted(set(now) - set(parent)) == sorted(NEW) and not set(parent) - set(now)
    for k, line in parent.items():
        assert now[k] == line, k
    # ... and the table's new lines are this build's (the others are the parent's, and later commits may move them)
    for k in NEW:
        got = dict(zip(COLUMNS, now[k]))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
    # the kernels whose device functions moved into pg_lights_dev.hpp are the build's too
    lights = [k for k in parent if k.startswith("pg::k_lights_")]
    assert len(lights) == 7
    for k in lights:
        got = dict(zip(COLUMNS, parent[k]))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
