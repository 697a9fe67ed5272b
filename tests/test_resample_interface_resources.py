"""What the compiler made of pg_kernels_resample_interface.hip (csrc/*.remarks, no GPU needed).  k_resample_interface has
k_resample_lobe's shape -- the two walks inside a loop over the candidates -- so: no scratch, and of LDS the staged KD planes only,
k_resample_cosine's.  Its occupancy is four waves per SIMD in both instantiations, 103 registers without the candidate stores and
109 with them: beside what k_resample_lobe carries across the walks the loop carries the interface's index, and between the
walks it holds the Fresnel term, the refracted direction and the second Jacobian.  Held to five waves by its launch bounds the
instantiation without candidate stores takes 96 registers and 32 bytes of scratch per lane, so it is left at the four it reaches
by itself.  The floor below is what profiles/resample_interface/resource_usage.txt records for this build.  And
every kernel the parent commit had keeps its resource line: resource_usage_parent.txt against resource_usage.txt."""
import os

from test_resample_lobe_resources import _recorded
from test_resources import ROOT, kernels  # noqa: F401  (the fixture: the resource report of every kernel of the build)

PROFILE = os.path.join(ROOT, "profiles", "resample_interface")
NEW = ("pg::k_resample_interface<false>", "pg::k_resample_interface<true>")
COSINE = "pg::k_resample_cosine<false>"
COLUMNS = ("vgprs", "sgprs", "scratch", "occupancy", "lds")


def test_the_two_instantiations_without_scratch_and_with_the_cosine_kernels_lds(kernels):  # noqa: F811
    ri = {k: v for k, v in kernels.items() if "k_resample_interface" in k}
    assert sorted(ri) == sorted(NEW), sorted(kernels)
    recorded = _recorded(os.path.join(PROFILE, "resource_usage.txt"))
    for k, v in ri.items():
        assert v["file"] == "pg_kernels_resample_interface.remarks"
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] == kernels[COSINE]["lds"], (k, v, kernels[COSINE])       # the staged KD planes, nothing else
        floor = int(dict(zip(COLUMNS, recorded[k]))["occupancy"])
        assert floor >= 4 and v["occupancy"] >= floor, (k, v, floor)
    # the names keep clear of the prefixes the resource tests of 5.22 and 5.24 pin to their own two instantiations
    assert not any(k.startswith("pg::k_resample_lobe<") or k.startswith("pg::k_resample_cosine<") for k in ri)


def test_every_parent_kernel_keeps_its_resource_lines(kernels):  # noqa: F811
    parent, now = _recorded(os.path.join(PROFILE, "resource_usage_parent.txt")), _recorded(os.path.join(PROFILE, "resource_usage.txt"))
    assert len(parent) > 80 and COSINE in parent and "pg::k_resample_lobe<false>" in parent and "pg::k_pdf" in parent
    assert sorted(set(now) - set(parent)) == sorted(NEW) and not set(parent) - set(now)
    for k, line in parent.items():
        assert now[k] == line, k
    # ... and the table's new lines are this build's (the others are the parent's, and later commits may move them)
    for k in NEW:
        got = dict(zip(COLUMNS, now[k]))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
    # the kernels this one is measured beside are the build's too: their files were not touched
    for k in (COSINE, "pg::k_resample_cosine<true>", "pg::k_resample_lobe<false>", "pg::k_resample_lobe<true>"):
        got = dict(zip(COLUMNS, parent[k]))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
