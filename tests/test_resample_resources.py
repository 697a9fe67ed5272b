"""What the compiler made of pg_kernels_resample.hip (csrc/*.remarks, no GPU needed).  k_resample_cosine performs the two walks
of k_guided_bounce's PCG32 kernel inside a loop over the candidates: no scratch, and of LDS the staged KD planes only -- that
kernel's.  Its occupancy target, that kernel's eight waves per SIMD, is MISSED: the loop carries the stream, the tree's head, the
normal and its frame, and the reservoir across walks that need k_sample's 45 registers on their own -- 71 registers, seven waves
(77 and six with the candidate stores).  A build that recomputes the frame per candidate and is held to 64 registers ran no
faster, so the floors below are what the plain kernel reaches.  And every kernel the parent commit had keeps
its resource line: profiles/resample/resource_usage_parent.txt against resource_usage.txt."""
import os

from test_resources import ROOT, kernels  # noqa: F401  (the fixture: the resource report of every kernel of the build)

PROFILE = os.path.join(ROOT, "profiles", "resample")
NEW = ("pg::k_resample_cosine<false>", "pg::k_resample_cosine<true>")
FLOOR = {"pg::k_resample_cosine<false>": 7, "pg::k_resample_cosine<true>": 6}     # waves per SIMD (71 and 77 VGPRs)
BOUNCE = "pg::k_guided_bounce<false, false>"                                       # the PCG32 kernel of pg_bounce


def test_the_two_instantiations_without_scratch_and_with_the_bounce_kernels_lds(kernels):  # noqa: F811
    rs = {k: v for k, v in kernels.items() if k.startswith("pg::k_resample_cosine<")}
    assert sorted(rs) == sorted(NEW), sorted(kernels)
    for k, v in rs.items():
        assert v["file"] == "pg_kernels_resample.remarks"
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] == kernels[BOUNCE]["lds"], (k, v, kernels[BOUNCE])       # the staged KD planes, nothing else
        assert v["occupancy"] >= FLOOR[k], (k, v)


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
    assert len(parent) > 80 and BOUNCE in parent and "pg::k_pdf" in parent and "pg::k_irradiance<true>" in parent
    assert sorted(set(now) - set(parent)) == sorted(NEW) and not set(parent) - set(now)
    for k, line in parent.items():
        assert now[k] == line, k
    # ... and the table's new lines are this build's (the others are the parent's, and later commits may move them)
    for k in NEW:
        got = dict(zip(("vgprs", "sgprs", "scratch", "occupancy", "lds"), now[k]))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
