"""What the compiler made of pg_kernels_bounce.hip (csrc/*.remarks, no GPU needed).  k_guided_bounce is bound by the latency of
dependent gathers like the kernels it stands for, and hides it by occupancy: without the estimate it reaches at least the waves
per SIMD of k_guide_bounce and k_guide_bounce_warp of the same build; with it, the floor is what this build reached when the
kernel was written -- eight waves per SIMD at 54 (PCG32 form) and 48 (warp form) registers, k_guide_bounce's own occupancy, so
the floor is not below it."""
from test_resources import kernels  # noqa: F401  (the fixture: the resource report of every kernel of the build)

RADIANCE_FLOOR = 8      # waves per SIMD of k_guided_bounce<*, true> (54 and 48 VGPRs: the 64-register step)


def test_the_four_instantiations_and_their_occupancy(kernels):  # noqa: F811
    b = {k: v for k, v in kernels.items() if k.startswith("pg::k_guided_bounce<")}
    assert sorted(b) == ["pg::k_guided_bounce<false, false>", "pg::k_guided_bounce<false, true>",
                         "pg::k_guided_bounce<true, false>", "pg::k_guided_bounce<true, true>"], sorted(kernels)
    pdf = kernels["pg::k_pdf"]
    for k, v in b.items():
        assert v["file"] == "pg_kernels_bounce.remarks"
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] == pdf["lds"], (k, v, pdf)             # the staged KD planes, nothing else
    assert b["pg::k_guided_bounce<false, false>"]["occupancy"] >= kernels["pg::k_guide_bounce"]["occupancy"]
    assert b["pg::k_guided_bounce<true, false>"]["occupancy"] >= kernels["pg::k_guide_bounce_warp"]["occupancy"]
    for k in ("pg::k_guided_bounce<false, true>", "pg::k_guided_bounce<true, true>"):
        assert b[k]["occupancy"] >= RADIANCE_FLOOR, (k, b[k])
    assert RADIANCE_FLOOR >= kernels["pg::k_guide_bounce"]["occupancy"]
