"""What the compiler made of pg_kernels_lights.hip (csrc/*.remarks, no GPU needed).  The seven kernels use no scratch; the sample
and the pmf hold of LDS the staged KD planes only, as pg_fraction_query does, and the record what the fraction's record holds
(its table has the same size).  All of them reach eight waves per SIMD.  And every kernel the parent commit had keeps its
resource line: profiles/lights/resource_usage_parent.txt against resource_usage.txt."""
import os

from test_resources import ROOT, kernels  # noqa: F401  (the fixture: the resource report of every kernel of the build)

PROFILE = os.path.join(ROOT, "profiles", "lights")
NEW = ("pg::k_lights_sample", "pg::k_lights_pmf", "pg::k_lights_record", "pg::k_lights_build_wave", "pg::k_lights_build_group",
       "pg::k_lights_zero", "pg::k_lights_carry")
QUERY, RECORD = "pg::k_fraction_query", "pg::k_fraction_record"


def test_the_new_kernels_use_no_scratch(kernels):  # noqa: F811
    li = {k: v for k, v in kernels.items() if k.startswith("pg::k_lights_")}
    assert sorted(li) == sorted(NEW), sorted(kernels)
    for k, v in li.items():
        assert v["file"] == "pg_kernels_lights.remarks"
        assert v["scratch"] == 0, (k, v)
        assert v["occupancy"] == 8, (k, v)
    for k in ("pg::k_lights_sample", "pg::k_lights_pmf"):
        assert li[k]["lds"] == kernels[QUERY]["lds"], (k, li[k], kernels[QUERY])        # the staged KD planes, nothing else
    assert li["pg::k_lights_record"]["lds"] == kernels[RECORD]["lds"]
    assert li["pg::k_lights_build_wave"]["lds"] == 0 and li["pg::k_lights_build_group"]["lds"] == 32


def _recorded(path):
    """kernel -> its resource line, of a table tools/resource_lines.py wrote."""
    out = {}
    for line in open(path):
        f = [x.strip() for x in line.split("|")]
        if len(f) == 6 and not line.startswith("#") and f[0]:
            out[f[0]] = f[1:]
    return out


def test_every_parent_kernel_keeps_its_resource_lines(kernels):  # noqa: F811
    parent, now = _recorded(os.path.join(PROFILE, "resource_usage_parent.txt")), _recorded(os.path.join(PROFILE, "resource_usage.txt"))
    assert len(parent) > 80 and QUERY in parent and RECORD in parent and "pg::k_resample_cosine<false>" in parent
    assert sorted(set(now) - set(parent)) == sorted(NEW) and not set(parent) - set(now)
    for k, line in parent.items():
        assert now[k] == line, k
    # ... and the table's new lines are this build's (the others are the parent's, and later commits may move them)
    for k in NEW:
        got = dict(zip(("vgprs", "sgprs", "scratch", "occupancy", "lds"), now[k]))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
