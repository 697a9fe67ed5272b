#!/usr/bin/env python3
"""Can the BSDF tests fail?  Builds scratch copies of the CPU oracle with one deliberate error each (in a temporary
directory: nothing of the tree is touched), runs the checks of tests/test_bsdf_model.py against every copy and prints what
profiles/bsdf/mutations.txt records: which check catches the error and by how much.

    python tools/bsdf_mutants.py > profiles/bsdf/mutations.txt      (a few numbers behind it: those mutants only)
"""
import numpy as np

import oracle_mutants as OM   # (puts the tree and tests/ on sys.path)

import bsdf_model as BM  # noqa: E402
import bsdf_sets as BS  # noqa: E402
import test_bsdf_model as TB  # noqa: E402
from oracle import pg_oracle as po  # noqa: E402

# name, [(text of oracle/pg_oracle_render.c, its replacement)]: every text occurs exactly once
MUTANTS = [
    ("a G1 coefficient altered by 1 % (3.535 -> 3.57035)", [("(3.535f * a + 2.181f * a2)", "(3.57035f * a + 2.181f * a2)")]),
    ("r_p dropped from the conductor Fresnel", [("return 0.5f * (r_s + r_p);", "return 0.5f * (r_s + r_s);")]),
    ("a cos factor lost from D (Beckmann)", [("pgo_exp(-((ax * ax + ay * ay) / ct2)) / (((PI_F * a) * a) * (ct2 * ct2))",
                                              "pgo_exp(-((ax * ax + ay * ay) / ct2)) / (((PI_F * a) * a) * (ct2 * ct))")]),
    ("eta_ti for eta_it in the transmission Jacobian (rd_sample)", [("dwh_dwo = ((eta_it * eta_it) * om) / (denom * denom);",
                                                                     "dwh_dwo = ((eta_ti * eta_ti) * om) / (denom * denom);")]),
    ("G1 missing from the sampled pdf (rc_sample_m)", [("*pdf = ((rc_D(m, signed_alpha) * rc_G1(wi, m, signed_alpha)) * fabsf(dot3(wi, m))) / wi.z;",
                                                        "*pdf = (rc_D(m, signed_alpha) * fabsf(dot3(wi, m))) / wi.z;")]),
    ("the a >= 1.6 switch moved to 1.4", [("a >= 1.6f ? 1.0f", "a >= 1.4f ? 1.0f")]),
    ("the two-sided flip applied to a one-sided row", [("if (wi.z < 0.0f && !mt->one_sided) { wi.z = -wi.z; wo.z = -wo.z; }", "if (wi.z < 0.0f) { wi.z = -wi.z; wo.z = -wo.z; }"),
                                                       ("int flip = wi.z < 0.0f && !mt->one_sided;", "int flip = wi.z < 0.0f;")]),
    # None of the seven above moves a sampled DIRECTION (they change values and pdfs), so the density test cannot see them; and
    # an error in a sampler alone leaves pdf and weight consistent at the direction returned, so nothing else sees these three:
    ("GGX visible normals: the compression (1 + cos) / 2 taken as (1 + 0.9 cos) / 2", [("const float s = 0.5f * (1.0f + cos_i);", "const float s = 0.5f * (1.0f + 0.9f * cos_i);")]),
    ("Beckmann visible normals: the Newton steps left out", [("for (int i = 0; i < 3; ++i) {\n\t\tconst float slope = pgo_erfinv(x);", "for (int i = 0; i < 0; ++i) {\n\t\tconst float slope = pgo_erfinv(x);")]),
    ("the sampled slope not stretched back by alpha in x", [("const float rx = (cos_phi * sx - sin_phi * sy) * alpha;", "const float rx = (cos_phi * sx - sin_phi * sy);")]),
]
RESULTS = []   # (name, set checks failed, least and greatest worst ratio of them, greatest multiple of a density tolerance)


def report(name):
    TB.oracle.cache_clear()
    caught = []   # (lanes out of band, lanes, worst ratio, set/check)
    for s in BS.SETS:
        out = TB.oracle(s)
        finite = all(np.isfinite(a).all() for a in out)
        for tag, v in zip(("eval", "sample"), TB.judge(s, out)):
            bad = v.failures().size
            if bad or not finite:
                worst = max(float(np.nan_to_num(r, posinf=1e30).max()) for r in v.ratio.values())
                caught.append((bad, v.ok.size, min(worst, 1e30), "%s/%s%s" % (s, tag, "" if finite else " (non-finite outputs)")))
    dens, factors = [], []
    for pair in TB.PAIRS:
        worst, mass = TB.density_differences(pair, po.bsdf_probe)
        if worst > TB.BIN_TOLERANCE or mass > TB.MASS_TOLERANCE:
            factors.append(max(worst / TB.BIN_TOLERANCE, mass / TB.MASS_TOLERANCE))
            dens.append("      %s: bin %.2e (%.1f x tolerance), mass %.2e (%.1f x)" % (pair, worst, worst / TB.BIN_TOLERANCE, mass, mass / TB.MASS_TOLERANCE))
    print("== %s" % name)
    if caught:
        print("   test_oracle_against_the_model fails in %d of %d checks (9 sets, eval and sample); lanes out of band, and the worst" % (len(caught), 2 * len(BS.SETS)))
        print("   |difference| in brackets of the band (the band is at most %.1f brackets wide):" % max(BM.BAND_C.values()))
        for bad, n, worst, what in caught:
            print("      %-18s %5d of %5d   %.3g" % (what, bad, n, worst))
    else:
        print("   test_oracle_against_the_model passes")
    if dens:
        print("   test_sampling_density fails for %d of %d pairs:" % (len(dens), len(TB.PAIRS)))
        print("\n".join(dens))
    else:
        print("   test_sampling_density passes")
    if not caught and not dens:
        print("   NOTHING FAILS")
    RESULTS.append((name, len(caught), min([c[2] for c in caught], default=0.0), max([c[2] for c in caught], default=0.0), max(factors, default=0.0)))


def main():
    print("""# profiles/bsdf/mutations.txt -- can the BSDF tests fail?  Written by: python tools/bsdf_mutants.py
# One deliberate error at a time in a scratch copy of oracle/pg_oracle_render.c (never committed), then the checks of
# tests/test_bsdf_model.py: every input set at level 3 against the model (eval and sample outputs), and every density pair.
# Tolerances of the density test: bin %.2e, mass %.2e.  The last three errors sit in a sampler alone: they move sampled
# directions and leave pdf and weight consistent at the direction returned.  The summary at the end is computed from the run.""" % (TB.BIN_TOLERANCE, TB.MASS_TOLERANCE))
    for name in OM.each_oracle(MUTANTS):
        report(name)
    lines = []
    for name, checks, least, greatest, factor in RESULTS:
        what = []
        if checks:
            what.append("band checks fail in %d of %d, worst lane %.3g to %.3g brackets" % (checks, 2 * len(BS.SETS), least, greatest))
        if factor:
            what.append("density test fails, by up to %.1f times a tolerance" % factor)
        lines.append((name, "; ".join(what)))
    OM.summary(lines, width=80)


if __name__ == "__main__":
    main()
