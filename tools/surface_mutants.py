#!/usr/bin/env python3
"""Can the surface tests fail?  Builds scratch copies of the CPU oracle with one deliberate error each (in a temporary
directory: nothing of the tree is touched, and nothing is ever built for the device), runs the tests of
tests/test_surface_model.py against every copy and prints what profiles/surface/mutations.txt records: which tests catch
the error.

    python tools/surface_mutants.py > profiles/surface/mutations.txt      (a few numbers behind it: those mutants only)
    python tools/surface_mutants.py --band > profiles/surface/band.txt    (the oracle as it is: worst |difference| / bracket per
                                                                           quantity and set, C = 4 x worst, ambiguous shares)
"""
import numpy as np

import oracle_mutants as OM   # (puts the tree and tests/ on sys.path)

import surface_model as SM  # noqa: E402
import test_surface_model as TS  # noqa: E402
from oracle import pg_oracle as po  # noqa: E402

# name, [(text of oracle/pg_oracle_render.c, its replacement[, how often the text occurs: 1])]
MUTANTS = [
    ("bu and bv swapped in the normal blend", [("vscale(ld3(Nn + 3), u)), vscale(ld3(Nn + 6), v));", "vscale(ld3(Nn + 3), v)), vscale(ld3(Nn + 6), u));")]),
    # (blending the vertices' uv and the affine to_uv commute: taking one before the other is the same function.  The order
    # error that is one: to_uv's offset added before its scale.)
    ("to_uv out of order: (uv + offset) * scale", [("const float uu = pgo_u2f(T[10]) * u + pgo_u2f(T[12]);", "const float uu = pgo_u2f(T[10]) * (u + pgo_u2f(T[12]));"),
                                                    ("const float vv = pgo_u2f(T[11]) * v + pgo_u2f(T[13]);", "const float vv = pgo_u2f(T[11]) * (v + pgo_u2f(T[13]));")]),
    ("the wrap replaced by a clamp", [("const int32_t ix0 = ((ix % W) + W) % W, ix1 = (((ix + 1) % W) + W) % W;",
                                       "const int32_t ix0 = ix < 0 ? 0 : ix >= W ? W - 1 : ix, ix1 = ix + 1 < 0 ? 0 : ix + 1 >= W ? W - 1 : ix + 1;"),
                                      ("const int32_t iy0 = ((iy % H) + H) % H, iy1 = (((iy + 1) % H) + H) % H;",
                                       "const int32_t iy0 = iy < 0 ? 0 : iy >= H ? H - 1 : iy, iy1 = iy + 1 < 0 ? 0 : iy + 1 >= H ? H - 1 : iy + 1;")]),
    ("texel centres at i / size", [("float x = uu * (float)W - 0.5f, y = vv * (float)H - 0.5f;", "float x = uu * (float)W, y = vv * (float)H;")]),
    ("the sRGB table applied after the blend", [("out[c] = (c00 * wx0 + c10 * wx1) * wy0 + (c01 * wx0 + c11 * wx1) * wy1;",
                                                 "(void)c00; (void)c10; (void)c01; (void)c11; out[c] = lut[(int)((((float)((t00 >> (8 * c)) & 255u) * wx0 + (float)((t10 >> (8 * c)) & 255u) * wx1) * wy0 + ((float)((t01 >> (8 * c)) & 255u) * wx0 + (float)((t11 >> (8 * c)) & 255u) * wx1) * wy1) + 0.5f)];")]),
    ("checkerboard: >= in place of >", [("const int mx = fu > 0.5f, my = fv > 0.5f;", "const int mx = fu >= 0.5f, my = fv >= 0.5f;")]),
    ("a box face's sign flipped for one axis (y)", [("return (face & 1) ? V(-n.x, -n.y, -n.z) : n;", "return ((face & 1) != ((face >> 1) == 1)) ? V(-n.x, -n.y, -n.z) : n;")]),
    ("the sphere's normal taken from the unprojected point", [("s.n = normalize3(vsub(s.p, c));", "s.n = n0;")]),
    ("cos alpha in place of 1 - cos alpha in the cone pdf", [("pdf = INV_TWO_PI_F / (1.0f - cos_alpha);", "pdf = INV_TWO_PI_F / cos_alpha;")]),
    ("the quad's pdf by area: 1 / A in place of d^2 / (cos A)", [("pdf = d2 / (fabsf(dp) * Q[14]);", "pdf = 1.0f / Q[14];")]),
    ("a left-handed frame (t negated)", [("*t = V(b, sign + (n.y * n.y) * a, -n.y);", "*t = V(-b, -(sign + (n.y * n.y) * a), n.y);")]),
]
TESTS = [(name, getattr(TS, name), args) for name, args in (
    ("test_oracle_against_the_model", TS.SCENES), ("test_the_next_bounce_finds_the_same_normal", TS.SCENES),
    ("test_bitmap_known_answers", None), ("test_texture_coordinates_on_the_wrap_negative_huge_and_not_finite", None),
    ("test_to_uv_with_a_negative_scale", None), ("test_checkerboard_at_one_half", None), ("test_vertex_normals_that_cancel", None),
    ("test_a_blend_whose_squared_length_underflows", None), ("test_all_six_faces_of_a_rotated_box", None),
    ("test_sphere_head_on_and_grazing", None), ("test_quad_emitter_at_grazing_incidence", None),
    ("test_sphere_emitter_around_the_cap_limit", None),
    ("test_oracle_returns_for_non_finite_and_degenerate_hits", ("veach-ajar", "mixed", "veach-mis")))]
HEADER = """# profiles/surface/mutations.txt -- can the surface tests fail?  Written by: python tools/surface_mutants.py
# One deliberate error at a time in a scratch copy of oracle/pg_oracle_render.c (never committed, never built for the device),
# then every test of tests/test_surface_model.py against that copy: the failing tests and the first line of each failure.
# The summary at the end is computed from the run."""

def band():
    print("""# profiles/surface/band.txt -- the band of tests/surface_model.py measured on the CPU oracle.  Written by:
# python tools/surface_mutants.py --band
# Per input set: lanes, the share of lanes with a doubtful decision (cap %.0f %% on the broad sets), and per quantity the worst
# |oracle - model| / bracket over the lanes without one (bracket = 2^-24 ops |q| + sum |dq/dx_j| ulp(x_j), surface_model.py).
# The decisions are taken with the committed BAND_C.  C = 4 x the worst ratio over all sets; 64 would mean a missing term.""" % (100 * SM.AMBIGUOUS_CAP))
    worst = {}
    sets = [("%s broad" % n, n, TS.hits(n), None) for n in TS.SCENES]
    for which in ("3x2", "5x7", "3x2 flipped"):   # the texture grid of test_bitmap_known_answers (aimed at texel borders and the wrap)
        g = np.array([(a, b) for a in (0.0, 1 / 6, 1 / 3, 0.5, 0.25, 2 ** -24, 0.75) for b in (0.0, 0.25, 0.125, 2 ** -24) if a + b <= 1], np.float32)
        h = TS.texture_hits(which, g)
        h["u"], h["v"] = po.intersect(TS.texture_scene(), h["o"], h["d"])[2:4]
        sets.append(("textures %s (aimed)" % which, "textures", h, None))
    for label, name, h, _ in sets:
        T = TS.tables(name)
        m = SM.surface(T, h["prim"], h["o"], h["d"], h["t"], h["u"], h["v"])
        bad, ratio, amb = SM.judge(T, m, TS.probe_oracle(name, h), h["d"], h["ref"], po.feature_level(TS.scene(name)))
        assert not bad, (label, bad)
        print("%-28s %5d lanes  %5.2f %% ambiguous   %s" % (label, h["prim"].shape[0], 100 * amb.mean(),
                                                           "  ".join("%s %.3f" % (k, v.max()) for k, v in sorted(ratio.items()))))
        for k, v in ratio.items():
            worst[k] = max(worst.get(k, 0.0), float(v.max()))
    OM.worst_ratios(worst, SM.BAND_C)


if __name__ == "__main__":
    OM.main(HEADER, MUTANTS, TESTS, band)
