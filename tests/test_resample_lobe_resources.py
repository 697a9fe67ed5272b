"""What the compiler made of pg_kernels_resample_lobe.hip (csrc/*.remarks, no GPU needed).  k_resample_lobe has k_resample_cosine's
shape -- the two walks inside a loop over the candidates -- so: no scratch, and of LDS the staged KD planes only, that kernel's.
Its occupancy is BELOW that kernel's seven waves per SIMD: beside what k_resample_cosine carries across the walks (the stream, the
tree's head, the frame, the reservoir) the loop carries the viewer's local direction, the roughness and the specular share, and
between the walks it holds a GGX visible-normal sample or a GGX density with its normalisations -- 96 registers and five waves
without the candidate stores (held there by the kernel's launch bounds: left alone the compiler takes 97 and four waves, which
measured 7 % slower), 103 registers and four waves with them (five would cost scratch).  The floors below are what
the build reaches.  And every kernel the parent commit had keeps its resource line:
profiles/resample_lobe/resource_usage_parent.txt against resource_usage.txt."""
import os

from test_resources import ROOT, kernels  # noqa: F401  (the fixture: the resource report of every kernel of the build)

PROFILE = os.path.join(ROOT, "profiles", "resample_lobe")
NEW = ("pg::k_resample_lobe<false>", "pg::k_resample_lobe<true>")
FLOOR = {"pg::k_resample_lobe<false>": 5, "pg::k_resample_lobe<true>": 4}         # waves per SIMD (96 and 103 VGPRs)
COSINE = "pg::k_resample_cosine<false>"


def test_the_two_instantiations_without_scratch_and_with_the_cosine_kernels_lds(kernels):  # noqa: F811
    rl = {k: v for k, v in kernels.items() if k.startswith("pg::k_resample_lobe<")}
    assert sorted(rl) == sorted(NEW), sorted(kernels)
    for k, v in rl.items():
        assert v["file"] == "pg_kernels_resample_lobe.remarks"
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] == kernels[COSINE]["lds"], (k, v, kernels[COSINE])       # the staged KD planes, nothing else
        assert v["occupancy"] >= FLOOR[k], (k, v)
    assert not any(k.startswith("pg::k_resample_cosine") for k in rl)


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
    assert len(parent) > 80 and COSINE in parent and "pg::k_resample_cosine<true>" in parent and "pg::k_pdf" in parent
    assert sorted(set(now) - set(parent)) == sorted(NEW) and not set(parent) - set(now)
    for k, line in parent.items():
        assert now[k] == line, k
    # ... and the table's new lines are this build's (the others are the parent's, and later commits may move them)
    for k in NEW:
        got = dict(zip(("vgprs", "sgprs", "scratch", "occupancy", "lds"), now[k]))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
    # the two kernels of pg_kernels_resample.hip are the build's too: that file was not touched
    for k in (COSINE, "pg::k_resample_cosine<true>"):
        got = dict(zip(("vgprs", "sgprs", "scratch", "occupancy", "lds"), parent[k]))
        for key in ("vgprs", "scratch", "occupancy", "lds"):
            assert int(got[key]) == kernels[k][key], (k, key, got, kernels[k])
