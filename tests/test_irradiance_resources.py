"""What the compiler made of pg_kernels_irradiance.hip (csrc/*.remarks, no GPU needed).  The query kernels are bound by the
latency of dependent gathers, like k_radiance, and hide it by occupancy: eight waves per SIMD, no scratch, and of LDS the staged
KD planes only.  The build kernels use no scratch.  And every kernel the parent commit had keeps its resource lines:
profiles/irradiance/resource_usage_parent_kernels.diff is the (empty) difference, resource_usage.txt what it was taken from."""
import os

from test_resources import ROOT, kernels  # noqa: F401  (the fixture: the resource report of every kernel of the build)

PROFILE = os.path.join(ROOT, "profiles", "irradiance")
BUILD_KERNELS = ("pg::k_irr_roots", "pg::k_irr_level", "pg::k_irr_finish")


def test_the_query_kernels_run_at_eight_waves_without_scratch(kernels):  # noqa: F811
    irr = {k: v for k, v in kernels.items() if k.startswith("pg::k_irradiance<")}
    assert sorted(irr) == ["pg::k_irradiance<false>", "pg::k_irradiance<true>"], sorted(kernels)
    rad = kernels["pg::k_radiance<false>"]
    for k, v in irr.items():
        assert v["file"] == "pg_kernels_irradiance.remarks"
        assert v["occupancy"] >= 8 and v["occupancy"] >= rad["occupancy"], (k, v, rad)
        assert v["scratch"] == 0 and v["lds"] == rad["lds"], (k, v)     # the staged KD planes, nothing else


def test_the_build_kernels_use_no_scratch(kernels):  # noqa: F811
    for k in BUILD_KERNELS:
        assert kernels[k]["file"] == "pg_kernels_irradiance.remarks" and kernels[k]["scratch"] == 0 and kernels[k]["lds"] == 0, (k, kernels[k])


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
    assert len(parent) > 80 and "pg::k_radiance<true>" in parent and "pg::k_pdf" in parent
    new = sorted(set(now) - set(parent))
    assert new == sorted(BUILD_KERNELS + ("pg::k_irradiance<false>", "pg::k_irradiance<true>")), new
    for k, line in parent.items():
        assert now[k] == line, k
    # the committed diff of the two tables adds this file's section and changes nothing else
    diff = [x for x in open(os.path.join(PROFILE, "resource_usage_parent_kernels.diff")).read().splitlines() if x[:1] in "<>"]
    assert len(diff) == 1 + len(new) and all(x.startswith("> ") for x in diff) and diff[0] == "> ## pg_kernels_irradiance.hip"
    # ... and the table's new lines are this build's (the others are the parent's, and later commits may move them)
    for k in new:
        line = now[k]
        got = dict(zip(("vgprs", "sgprs", "scratch", "occupancy", "lds"), line))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
