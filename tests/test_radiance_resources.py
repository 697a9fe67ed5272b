"""What the compiler made of pg_kernels_radiance.hip (csrc/*.remarks, no GPU needed): the query kernels are bound by the latency of
dependent gathers, like k_pdf, and hide it by occupancy -- every k_radiance instantiation reaches at least the waves per SIMD
k_pdf reaches in the same build.  (That no kernel uses scratch is tests/test_resources.py's, for every kernel.)"""
from test_resources import kernels  # noqa: F401  (the fixture: the resource report of every kernel of the build)


def test_the_radiance_kernels_reach_the_occupancy_of_k_pdf(kernels):  # noqa: F811
    pdf = kernels["pg::k_pdf"]
    rad = {k: v for k, v in kernels.items() if k.startswith("pg::k_radiance<")}
    assert sorted(rad) == ["pg::k_radiance<false>", "pg::k_radiance<true>"], sorted(kernels)
    for k, v in rad.items():
        assert v["file"] == "pg_kernels_radiance.remarks"
        assert v["occupancy"] >= pdf["occupancy"], (k, v, pdf)
        assert v["scratch"] == 0 and v["lds"] == pdf["lds"], (k, v)     # the staged KD planes, nothing else
    assert kernels["pg::k_radiance_carry"]["occupancy"] >= pdf["occupancy"]
