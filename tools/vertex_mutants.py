#!/usr/bin/env python3
"""Can the tests of a vertex's bookkeeping fail?  Builds scratch copies of the CPU oracle with one deliberate error each (in a
temporary directory: nothing of the tree is touched, and nothing is ever built for the device), runs the tests of
tests/test_vertex_model.py against every copy and prints what profiles/vertex/mutations.txt records: which tests catch the error.

    python tools/vertex_mutants.py > profiles/vertex/mutations.txt      (a few numbers behind it: those mutants only)
    python tools/vertex_mutants.py --band > profiles/vertex/band.txt    (the oracle as it is: worst |difference| / bracket per
                                                                         quantity and set, C = 4 x worst, ambiguous shares)
"""
import oracle_mutants as OM   # (puts the tree and tests/ on sys.path)

import test_vertex_model as TV  # noqa: E402
import vertex_model as VM  # noqa: E402

SCRUB = ["if (rn.%s != rn.%s) rn.%s = 0.0f;" % (c, c, c) for c in "xyz"]
# name, [(text of oracle/pg_oracle_render.c, its replacement[, how often the text occurs: 1])]
MUTANTS = [
    ("f and 1 - f exchanged in the emitter sample's mixture", [("float surface_pdf_em = f * bp_em + ((1.0f - f) * sdtree_pdf_em) * pdf_diffuse;",
                                                                "float surface_pdf_em = (1.0f - f) * bp_em + (f * sdtree_pdf_em) * pdf_diffuse;")]),
    ("f and 1 - f exchanged in woPdf", [("woPdf = f * bsdf_pdf + (1.0f - f) * A->pdf_tree;", "woPdf = (1.0f - f) * bsdf_pdf + f * A->pdf_tree;")]),
    ("the MIS arguments swapped", [("mis_weight(ds_pdf, surface_pdf_em); /* :253 */", "mis_weight(surface_pdf_em, ds_pdf);")]),
    ("the delta light ignored", [("(level >= 3 && ds_delta && nee_live) ? 1.0f :", "(0) ? 1.0f :")]),
    ("occlusion ignored", [("(A->occluded || !nee_live) ? V(0, 0, 0) : A->em_w;", "(!nee_live) ? V(0, 0, 0) : A->em_w;")]),
    ("the unguided pass takes the mixture too", [("if (!guided) surface_pdf_em = bp_em;", "")]),
    ("Le added whether flagged or not", [("(A->flags & PGO_F_HAS_LE) ? A->Le : V(0, 0, 0);", "A->Le;")]),
    ("prev_pdf from the BSDF sample", [("*prev_pdf = woPdf;", "*prev_pdf = A->bsdf_pdf;")]),
    ("no re-evaluation on tree lanes", [("if (smp_tree) { /* :302-304 */", "if (0) {")]),
    ("to_local about ng", [("fr.n = A->n;\n\t\tframe_from_normal(A->n, &fr.s, &fr.t);", "fr.n = A->ng;\n\t\tframe_from_normal(A->ng, &fr.s, &fr.t);")]),
    ("the woPdf guard removed", [("if (!(woPdf > 0.0f)) bsdf_weight = V(0, 0, 0);", "")]),
    ("L recorded before the add", [("rec->thr = thr; rec->L = L; rec->woPdf = woPdf;", "rec->thr = thr; rec->L = *L_io; rec->woPdf = woPdf;")]),
    ("thr recorded after the multiply", [("rec->thr = thr; rec->L = L; rec->woPdf = woPdf;", "rec->thr = vmul(thr, bsdf_weight); rec->L = L; rec->woPdf = woPdf;")]),
    ("the record's woPdf from the BSDF sample", [("rec->thr = thr; rec->L = L; rec->woPdf = woPdf;", "rec->thr = thr; rec->L = L; rec->woPdf = A->bsdf_pdf;")]),
    ("nee_lum undivided", [("v3 rn = vdiv(Lr_dir, thr);", "v3 rn = Lr_dir;")]),
    ("nee_lum unscrubbed", [(s, "") for s in SCRUB]),
    ("nee_lum scrubs infinities too", [(s, s.replace("rn.%s != rn.%s" % (c, c), "!isfinite(rn.%s)" % c)) for s, c in zip(SCRUB, "xyz")]),
    ("ior in place of ior^2", [("float rr_prob = tmax * (ior * ior);", "float rr_prob = tmax * ior;")]),
    ("ior updated after the roulette", [("if (level >= 3) ior = ior * A->eta; /* :353", "/* :353"),
                                        ("*thr_io = thr; *L_io = L; *ior_io = ior;", "if (level >= 3) ior = ior * A->eta;\n\t*thr_io = thr; *L_io = L; *ior_io = ior;")]),
    ("ior follows eta below level 3", [("if (level >= 3) ior = ior * A->eta; /* :353", "ior = ior * A->eta; /* :353")]),
    ("<= in the roulette", [("const int rr_continue = rr < rr_prob;", "const int rr_continue = rr <= rr_prob;")]),
    ("the throughput divided by rr_prob", [("active_next = active_next && (!rr_active || rr_continue);\n\t/* :352 spawn_ray",
                                           "active_next = active_next && (!rr_active || rr_continue);\n\tif (rr_active) thr = vdivs(thr, rr_prob);\n\t/* :352 spawn_ray")]),
    ("depth > rr_depth", [("const int rr_active = depth >= (uint32_t)rr_depth;", "const int rr_active = depth > (uint32_t)rr_depth;")]),
    ("the 0.95 cap dropped", [("if (!(rr_prob < 0.95f)) rr_prob = 0.95f; /* dr.minimum(x, 0.95): NaN -> 0.95 */\n\tconst int rr_active", "const int rr_active")]),
    ("the zero-throughput stop dropped", [("active_next = active_next && (tmax != 0.0f);\n\tfloat rr_prob", "float rr_prob")]),
    ("the roulette's draw only where the roulette is on", [("const float rr = pgo_pcg32_next_f32(rng); /* :377, unmasked */",
                                                           "const float rr = rr_active ? pgo_pcg32_next_f32(rng) : 0.0f;")]),
    ("the offset without 1 + max |p|", [("float mag = (1.0f + max3(V(fabsf(A->p.x), fabsf(A->p.y), fabsf(A->p.z)))) * RAY_EPS_F;", "float mag = RAY_EPS_F;")]),
    ("the offset's sign reversed", [("if (dot3(A->ng, wo_world) < 0.0f) mag = -mag;", "if (dot3(A->ng, wo_world) > 0.0f) mag = -mag;")]),
    ("the offset along the shading normal", [("*ray_o = vadd(A->p, vscale(A->ng, mag));", "*ray_o = vadd(A->p, vscale(A->n, mag));")]),
]
TESTS = [("test_oracle_against_the_model", lambda a: TV.test_oracle_against_the_model(*a), [(lv, sw) for lv in range(4) for sw in TV.SWITCHES]),
         ("test_edges_of_the_mixture", TV.test_edges_of_the_mixture, None),
         ("test_edges_of_the_emitter_sample", TV.test_edges_of_the_emitter_sample, None),
         ("test_roulette_and_advance", TV.test_roulette_and_advance, None),
         ("test_six_chained_bounces", TV.test_six_chained_bounces, None)]
HEADER = """# profiles/vertex/mutations.txt -- can the tests of a vertex's bookkeeping fail?  Written by: python tools/vertex_mutants.py
# One deliberate error at a time in a scratch copy of oracle/pg_oracle_render.c (never committed, never built for the device),
# then every test of tests/test_vertex_model.py against that copy: the failing tests and the first line of each failure.
# The summary at the end is computed from the run."""


def band():
    print("""# profiles/vertex/band.txt -- the band of tests/vertex_model.py measured on the CPU oracle.  Written by:
# python tools/vertex_mutants.py --band
# Per broad set (feature level; guided, record, store_nee; the four f over a quarter of the lanes each): lanes, the share with a
# doubtful decision (cap %.0f %%), and per quantity the worst |oracle - model| / bracket over the lanes without one (bracket =
# 2^-24 ops |q| + sum |dq/dx_j| ulp(x_j), vertex_model.py; weight and nee are seen in the record only).  The decisions are
# taken with the committed BAND_C.  C = 4 x the worst ratio over all sets; 64 would mean a missing term.""" % (100 * VM.AMBIGUOUS_CAP))
    worst = {}
    for level in range(4):
        for sw in TV.SWITCHES:
            amb, n, w = TV.check_set(TV.broad(level, sw), level, TV.probe_oracle, "level %d %s" % (level, sw))
            print("level %d  %s  %5d lanes  %6.3f %% ambiguous   %s" % (level, sw, n, 100.0 * amb / n, "  ".join("%s %.3f" % kv for kv in sorted(w.items()))))
            for k, r in w.items():
                worst[k] = max(worst.get(k, 0.0), r)
    OM.worst_ratios(worst, VM.BAND_C)


if __name__ == "__main__":
    OM.main(HEADER, MUTANTS, TESTS, band)
