#!/usr/bin/env python3
"""Can the emitter-sampling tests fail?  Builds scratch copies of the CPU oracle with one deliberate error each (in a temporary
directory: nothing of the tree is touched, and nothing is ever built for the device), runs the tests of
tests/test_emitter_model.py against every copy and prints what profiles/emitter/mutations.txt records: which tests catch
the error.

    python tools/emitter_mutants.py > profiles/emitter/mutations.txt      (a few numbers behind it: those mutants only)
    python tools/emitter_mutants.py --band > profiles/emitter/band.txt    (the oracle as it is: worst |difference| / bracket per
                                                                           quantity and set, C = 4 x worst, ambiguous shares,
                                                                           the density differences behind the tolerances)
"""
import numpy as np

import oracle_mutants as OM   # (puts the tree and tests/ on sys.path)

import emitter_model as EM  # noqa: E402
import test_emitter_model as TE  # noqa: E402

SHADOW = "*sh_o = so; *sh_d = vdivs(sd, sdist); *sh_tmax = sdist * (1.0f - SHADOW_EPS_F);"
# name, [(text of oracle/pg_oracle_render.c, its replacement[, how often the text occurs: 1])]
MUTANTS = [
    ("e1 not rescaled after the choice", [("e1 = e1 * count - (float)idx;", "(void)idx;")]),
    # (the probe's list has one spare entry, which this mutant reads at e1 = 1: zeroed, so that the copy reads shape 0 and not the heap)
    ("the count - 1 clamp dropped", [("if (idx > (uint32_t)(n_em - 1)) idx = (uint32_t)(n_em - 1);", ""),
                                     ("int *em = malloc(sizeof(int) * (sc->n_quads + sc->n_spheres + sc->n_dir_lights + 1));",
                                      "int *em = calloc(sc->n_quads + sc->n_spheres + sc->n_dir_lights + 1, sizeof(int));")]),
    ("quad E1 and E2 swapped", [("pl = vadd(vadd(ld3(E), vscale(ld3(E + 3), e1)), vscale(ld3(E + 6), e2));",
                                 "pl = vadd(vadd(ld3(E), vscale(ld3(E + 6), e1)), vscale(ld3(E + 3), e2));")]),
    ("(e1, e2) swapped on the sphere", [("pgo_sincos(e2 * (2.0f * PI_F), &sin_phi, &cos_phi);", "pgo_sincos(e1 * (2.0f * PI_F), &sin_phi, &cos_phi);"),
                                         ("const float tt = 1.0f + (cos_max - 1.0f) * e1;", "const float tt = 1.0f + (cos_max - 1.0f) * e2;"),
                                         ("} else sin_theta_2 = sin_max2 * e1;", "} else sin_theta_2 = sin_max2 * e2;")]),
    ("cos_alpha without its first term", [("const float cos_alpha = sin_theta_2 * inv_sin_max +", "const float cos_alpha = 0.0f * inv_sin_max +")]),
    ("+axis in place of -axis in the sphere's frame", [("fr.n = vscale(dc_v, -inv_dc);", "fr.n = vscale(dc_v, inv_dc);")]),
    ("d in place of d^2 in the quad's density", [("pdf_cone) : d2 / (fabsf(dp) *", "pdf_cone) : dist / (fabsf(dp) *")]),
    ("1 / count dropped from ds_pdf only", [("*ds_pdf = pdf * inv_count;", "*ds_pdf = pdf;")]),
    ("the offset's sign flipped", [("if (dot3(n, dir0) < 0.0f) mag = -mag;", "if (dot3(n, dir0) > 0.0f) mag = -mag;")]),
    ("kShadowEps = 0", [(SHADOW, SHADOW.replace("(1.0f - SHADOW_EPS_F)", "1.0f"), 2)]),
    ("sh_tmax past the light: 1 + kShadowEps", [(SHADOW, SHADOW.replace("1.0f - SHADOW_EPS_F", "1.0f + SHADOW_EPS_F"), 2)]),
    ("the directional light's distance: max in place of 2 max", [("const float dist = 2.0f * (sc->bsphere[3] > dc", "const float dist = 1.0f * (sc->bsphere[3] > dc")]),
    ("the small-angle switch inverted", [("if (sin_max2 > 0.00068523f) {", "if (!(sin_max2 > 0.00068523f)) {")]),
    ("the facing test dropped: a light seen from behind is sampled", [("if (dp < 0.0f) pdf = is_sphere", "if (dp != 0.0f) pdf = is_sphere")]),
]
TESTS = [(name, getattr(TE, name), args) for name, args in (
    ("test_oracle_against_the_model", TE.SCENES), ("test_mis_consistency", TE.SCENES), ("test_shadow_rays", TE.SCENES),
    ("test_choice_of_emitter", (1, 2, 3, 7)), ("test_quad_light_at_grazing_incidence", None),
    ("test_sphere_light_from_every_distance", (2.0, 0.03)), ("test_between_the_inside_cut_and_the_cap_limit", (2.0, 0.03)),
    ("test_directional_light", None), ("test_a_scene_without_emitters_gives_zero_lanes", None),
    ("test_oracle_returns_for_non_finite_points_and_normals", ("mixed", "torus", "cornell-box")),
    ("test_sampling_density", TE.PAIRS))]
HEADER = """# profiles/emitter/mutations.txt -- can the emitter-sampling tests fail?  Written by: python tools/emitter_mutants.py
# One deliberate error at a time in a scratch copy of oracle/pg_oracle_render.c (never committed, never built for the device),
# then every test of tests/test_emitter_model.py against that copy: the failing tests and the first line of each failure.
# The summary at the end is computed from the run."""

def band():
    print("""# profiles/emitter/band.txt -- the band of tests/emitter_model.py measured on the CPU oracle.  Written by:
# python tools/emitter_mutants.py --band
# Per input set: lanes, the share of ALL lanes with a doubtful decision, lanes whose point lies on the emitter they sample
# (undecided in exact arithmetic -- cos = 0 on a quad's own plane, a gap of 0 from a sphere -- and all ambiguous), the share
# of the OTHER lanes with a doubtful decision (this is what the cap of %.0f %% is on, on the broad sets), and per quantity the worst
# |oracle - model| / bracket over the lanes without one (bracket = 2^-24 ops |q| + sum |dq/dx_j| ulp(x_j) + the named terms,
# emitter_model.py).  The decisions are taken with the committed BAND_C.  C = 4 x the worst ratio over all sets; 64 would
# mean a missing term.""" % (100 * EM.AMBIGUOUS_CAP))
    worst = {}
    sets = [("%s broad" % n, TE.scene(n), TE.broad(n)) for n in TE.SCENES] + [(label + " (aimed)", sc, L) for label, sc, L in TE.known_cases()]
    for label, sc, L in sets:
        T = EM.Tables(sc)
        bad, ratio, amb, v = EM.judge(T, L["p"], L["n"], L["e"], TE.probe_oracle(sc, L))
        assert not bad, (label, bad)
        own = (v.prim == L["prim"]) if "prim" in L else np.zeros(amb.shape[0], bool)
        print("%-28s %5d lanes  %6.3f %% ambiguous  %4d on their emitter  %6.3f %% of the others ambiguous   %s" % (
            label, amb.shape[0], 100 * amb.mean(), own.sum(), 100 * amb[~own].mean(), "  ".join("%s %.3f" % (k, r.max()) for k, r in sorted(ratio.items()))))
        for k, r in ratio.items():
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
    OM.worst_ratios(worst, EM.BAND_C)
    print("the sampling density at the committed grid (%d x %d samples, %d x %d bins -- %s --, %d^2 midpoints per bin): worst bin difference, "
          "|valid fraction - the model's mass|" % (TE.GRID, TE.GRID, TE.BINS_C, TE.BINS_P, ", ".join("%s: %d x %d over the exact extent" % (k, v[0], v[1]) for k, v in TE.PAIR_BINS.items()), TE.SUB))
    for pair in TE.PAIRS:
        a, b, _ = TE.density_differences(pair, TE.probe_oracle)
        print("   %-26s %.3e   %.3e   twice that: %.2e  %.2e   committed tolerances: %.2e  %.2e" % (
            pair, a, b, 2 * a, 2 * b, TE.BIN_TOLERANCE[pair], TE.MASS_TOLERANCE[pair]))


if __name__ == "__main__":
    OM.main(HEADER, MUTANTS, TESTS, band)
