#!/usr/bin/env python3
"""Can the tests of a vertex's head fail?  Builds scratch copies of the CPU oracle with one deliberate error each (in a
temporary directory: nothing of the tree is touched, and nothing is ever built for the device), runs the tests of
tests/test_head_model.py against every copy and prints what profiles/head/mutations.txt records: which tests catch the error.

    python tools/head_mutants.py > profiles/head/mutations.txt      (a few numbers behind it: those mutants only)
    python tools/head_mutants.py --band > profiles/head/band.txt    (the oracle as it is: worst |difference| / bracket per
                                                                     quantity and set, C = 4 x worst, ambiguous shares)
"""
import oracle_mutants as OM   # (puts the tree and tests/ on sys.path)

import head_model as HM  # noqa: E402
import test_head_model as TH  # noqa: E402

MIS = "mis_weight(prev_bsdf_pdf, emitter_pdf)"
HIT_PDF = "emitter_hit_pdf(sc, q, prev_p, p, n, inv_em_count);"
PICK = "\tint pick_tree = 0;\n\tif (active_next) pick_tree = pgo_pcg32_next_f32(rng) > f; /* :286 */\n"
SAMPLE = "\tfloat s1 = 0.0f, s2x = 0.0f, s2y = 0.0f;\n\tif (active_next) { /* next_1d"
DO_MIS = "const int do_mis = active_next && !delta && guided; /* :283 */"
# name, [(text of oracle/pg_oracle_render.c, its replacement[, how often the text occurs: 1])]
MUTANTS = [
    ("mis_weight's arguments exchanged", [(MIS, "mis_weight(emitter_pdf, prev_bsdf_pdf)")]),
    ("the balance heuristic", [(MIS, "(prev_bsdf_pdf > 0.0f ? prev_bsdf_pdf / (emitter_pdf + prev_bsdf_pdf) : 0.0f)")]),
    ("the emitter density taken from p", [(HIT_PDF, "emitter_hit_pdf(sc, q, p, p, n, inv_em_count);")]),
    ("the emitter density taken from the ray's origin", [(HIT_PDF, "emitter_hit_pdf(sc, q, ray_o, p, n, inv_em_count);")]),
    ("the back of a lamp emits", [("(is_em && wi.z > 0.0f) ? sf.radiance", "(is_em) ? sf.radiance")]),
    ("depth < max_depth", [("(depth + 1 < (uint32_t)D) && valid;", "(depth < (uint32_t)D) && valid;")]),
    (">= at f", [("pgo_pcg32_next_f32(rng) > f; /* :286 */", "pgo_pcg32_next_f32(rng) >= f;")]),
    ("the emitter draws masked", [("const float e1 = pgo_pcg32_next_f32(rng), e2 = pgo_pcg32_next_f32(rng); /* :214 next_2d, unmasked */",
                                   "float e1 = 0.0f, e2 = 0.0f;\n\tif (active_em) { e1 = pgo_pcg32_next_f32(rng); e2 = pgo_pcg32_next_f32(rng); }")]),
    ("ng for n in the frame of wo_em", [("const v3 wo_em = to_local(&fr, o->ds_d);",
                                         "frame fg;\n\tfg.n = ng;\n\tframe_from_normal(ng, &fg.s, &fg.t);\n\tconst v3 wo_em = to_local(&fg, o->ds_d);")]),
    ("emitter_pdf not zeroed behind a delta lobe", [("if (is_em && !prev_delta) emitter_pdf", "if (is_em) emitter_pdf")]),
    ("wi not negated", [("const v3 wi = to_local(&fr, V(-ray_d.x, -ray_d.y, -ray_d.z));\n\tconst int is_em",
                         "const v3 wi = to_local(&fr, ray_d);\n\tconst int is_em")]),
    ("Le without thr", [("const v3 Le = vmul(vscale(thr, mis), em_radiance);", "const v3 Le = vscale(em_radiance, mis);")]),
    ("active_em ignores Smooth at level 3", [("active_next && material_is_smooth(mt); /* :210", "active_next; /* :210")]),
    ("active_em not cleared at ds_pdf == 0", [("active_em = active_em && (o->ds_pdf != 0.0f); /* :216 */", "")]),
    ("the BSDF sample's draws unmasked", [("if (active_next) { /* next_1d (the lobe choice", "if (1) { /* next_1d (the lobe choice")]),
    ("the lobe draw dropped below level 3", [("const float lobe = pgo_pcg32_next_f32(rng);\n\t\tif (level >= 3) s1 = lobe;",
                                              "if (level >= 3) s1 = pgo_pcg32_next_f32(rng);")]),
    ("the pick drawn before the BSDF sample's draws", [(PICK, ""), (SAMPLE, PICK + SAMPLE)]),
    ("e1 and e2 exchanged", [("sample_emitter_ray(sc, em, n_em, p, ng, e1, e2, &o->ds_d", "sample_emitter_ray(sc, em, n_em, p, ng, e2, e1, &o->ds_d")]),
    ("s2x and s2y exchanged", [("bsdf_sample(mt, wi, s1, s2x, s2y, active_next, &wo_local", "bsdf_sample(mt, wi, s1, s2y, s2x, active_next, &wo_local")]),
    ("do_mis ignores delta", [(DO_MIS, "const int do_mis = active_next && guided;")]),
    ("do_mis ignores guided", [(DO_MIS, "const int do_mis = active_next && !delta;")]),
    ("bsdf_mis = do_mis & pick", [("const int bsdf_mis = do_mis && !smp_tree;", "const int bsdf_mis = do_mis && pick_tree;")]),
    ("wo left in the local frame", [("o->wo = to_world(&fr, wo_local);", "o->wo = wo_local;")]),
    ("1 / n_emitters missing from the hit density", [(HIT_PDF, "emitter_hit_pdf(sc, q, prev_p, p, n, 1.0f);")]),
    ("the emitter sample from the shading normal", [("sample_emitter_ray(sc, em, n_em, p, ng, e1, e2, &o->ds_d", "sample_emitter_ray(sc, em, n_em, p, n, e1, e2, &o->ds_d")]),
    ("a dead emitter sample keeps its shadow ray", [("if (!nee_live) need_shadow = 0;", "")]),
    ("HAS_LE from the radiance, not from Le", [("(pgo_f2u(Le.x) | pgo_f2u(Le.y) | pgo_f2u(Le.z)) != 0u ? PGO_F_HAS_LE",
                                                "(pgo_f2u(em_radiance.x) | pgo_f2u(em_radiance.y) | pgo_f2u(em_radiance.z)) != 0u ? PGO_F_HAS_LE")]),
]
TESTS = [("test_oracle_against_the_model", lambda a: TH.test_oracle_against_the_model(*a), [(name, g) for name in TH.SCENES for g in (0, 1)]),
         ("test_the_draw_ledger", TH.test_the_draw_ledger, None),
         ("test_depth_and_miss", TH.test_depth_and_miss, None),
         ("test_lamps", TH.test_lamps, None),
         ("test_emitter_sampling", TH.test_emitter_sampling, None),
         ("test_the_pick", TH.test_the_pick, None),
         ("test_level_three", TH.test_level_three, None),
         ("test_four_chained_bounces", TH.test_four_chained_bounces, ["cornell-box", "torus"])]
HEADER = """# profiles/head/mutations.txt -- can the tests of a vertex's head fail?  Written by: python tools/head_mutants.py
# One deliberate error at a time in a scratch copy of oracle/pg_oracle_render.c (never committed, never built for the device),
# then every test of tests/test_head_model.py against that copy: the failing tests and the first line of each failure.
# The summary at the end is computed from the run."""


def band():
    print("""# profiles/head/band.txt -- the band of tests/head_model.py measured on the CPU oracle.  Written by:
# python tools/head_mutants.py --band
# Per broad set (scene and its feature level; guided; the four f over a quarter of the lanes each): lanes, the share with a
# doubtful decision (cap %.0f %%), and per quantity the worst |oracle - model| / bracket over the lanes without one.  The new
# brackets are wi, Le, unit and dir (head_model.py); the others are the composed models' own, shown beside their committed
# constants' scale: p, n, refl surface_model's, emitter ... emitter_model's (both with C = 1), bsdf_em and bsdf_sample the
# ratio to bsdf_model's committed band as vertex_model widens it (1 is the band's edge).  The decisions are taken with the
# committed BAND_C.  C = 4 x the worst ratio over all sets; 64 would mean a missing term.""" % (100 * HM.AMBIGUOUS_CAP))
    worst = {}
    for name in TH.SCENES:
        for guided in (0, 1):
            amb, n, w = TH.check_set(name, TH.broad(name, guided), TH.probe_oracle, "%s guided %d" % (name, guided))
            print("%-11s level %d  guided %d  %5d lanes  %6.3f %% ambiguous   %s" % (
                name, TH.level_of(name), guided, n, 100.0 * amb / n, "  ".join("%s %.3f" % kv for kv in sorted(w.items()))))
            for k, r in w.items():
                if k in HM.BAND_C:
                    worst[k] = max(worst.get(k, 0.0), r)
    OM.worst_ratios(worst, HM.BAND_C)


if __name__ == "__main__":
    OM.main(HEADER, MUTANTS, TESTS, band)
