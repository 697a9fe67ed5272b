/*
 * pgsd_warp.h -- hierarchical sample warping over the SD-tree: three entry points of libpgsd.so beside the 60 of pgsd.h.
 *
 * pg_sample draws a direction the reference's way: a per-lane PCG32 stream, three draws per visited quadtree node
 * (quadtree.py:931-998).  A host that brings its own sample points -- stratified, low-discrepancy, mutated in primary sample
 * space -- needs a MAP instead: a 2-D point u of the unit square is pushed through the quadtree of the KD leaf that holds p by
 * the marginal probability of a row of children and the conditional probability of a child within the row.  The map is a
 * bijection of [0,1)^2 onto the canonical square (up to rounding), its density is KDTree.pdf, and it can be inverted.
 * Nothing here is in the reference; nothing of pgsd.h changes (PGSD_ABI_VERSION stays: entry points were added, no struct).
 *
 * Conventions are those of pgsd.h: device pointers, planar layout (u, u_out: Vector2f[n] = x[0..n) y[0..n)), byte masks with
 * NULL = all active, queries go to sdTree_prev, calls are asynchronous on `stream`, the same status codes; a NULL context or a
 * NULL required pointer (with n > 0) gives PG_ERR_INVALID.  The KD leaf of p is found exactly as pg_sample finds it (positions on faces,
 * outside the root box and NaN included: kdtree.py:435-470).  The calls draw no random numbers and keep no state.
 * The depth counters of pg_enable_depth_counters do not count these calls.
 *
 * ---- semantics: fp32, every operation rounded on its own (no contraction), in this order ----------------------------------
 *
 * ONE_M = 1 - 2^-24 (the largest float below 1).  The energies e* are the quad_irradiance values of sdTree_prev.  A node's
 * cell is [x0, x0+s] x [y0, y0+s] of the canonical square; its children by geometry are TR (upper x, upper y), TL, BL, BR =
 * the reference's children 1, 2, 3, 4 (quadtree.py:153-175; quad_child[0..3] of pg_tree_columns).  A walk visits at most 32
 * levels.
 *
 * WARP (u -> dir), pg_sample_warp and the select == 2 lanes of pg_guide_bounce_warp:
 *
 *   ux = (ux > 0) ? (ux < ONE_M ? ux : ONE_M) : 0                       (NaN -> 0); uy likewise
 *   x0 = y0 = 0; s = 1; node = root of the leaf's quadtree
 *   while node is not a leaf:
 *       t = eTR + eTL;  b = eBL + eBR;  tot = t + b
 *       if !(tot > 0) or tot is not finite:  eTR = eTL = eBL = eBR = 1, t = b = 2, tot = 4          (the uniform fallback)
 *       Py = t / tot
 *       uy < Py ?  row = top,    vy = uy / Py,               rs = t, eL = eTL
 *               :  row = bottom, vy = (uy - Py) / (1 - Py),  rs = b, eL = eBL
 *       Pl = eL / rs
 *       ux < Pl ?  col = left,   vx = ux / Pl
 *               :  col = right,  vx = (ux - Pl) / (1 - Pl)
 *       vx = (vx < ONE_M) ? vx : ONE_M;  vy likewise                                                 (also catches NaN)
 *       h = s * 0.5;  if right: x0 = x0 + h;  if top: y0 = y0 + h;  s = h;  node = that child;  (ux, uy) = (vx, vy)
 *   px = x0 + ux * s;  py = y0 + uy * s
 *   dir = canonicalToDir(px, py)  (common.py:100-129);   pdf_out = KDTree.pdf(p, dir)  (kdtree.py:489-496)
 *
 *   A child of zero energy is never chosen while a sibling has energy (its Py or Pl is exactly 0 or 1 and u < 1).  A root that
 *   is a leaf makes the warp the identity on the canonical square.  pdf_out is BY DEFINITION what pg_pdf returns for
 *   (p, dir) -- the contract of pg_sample: the kernel accumulates pdf * ((4 * child) / node) on the way down and uses that
 *   value when the round trip dir -> canonical lands strictly inside the leaf cell; otherwise it takes the literal second
 *   descent.
 *
 * INVERSE (dir -> u), pg_invert_warp:
 *
 *   (cx, cy) = dirToCanonical(dir)  (common.py:132-158; always inside the square, a non-finite dir gives (0, 0))
 *   ax = ay = 0;  bx = by = 1;  x0 = y0 = 0;  s = 1
 *   while node is not a leaf:
 *       h = s * 0.5;  child = the one pdfQuadTree descends into: the highest-numbered child whose cell, edges included,
 *                             contains (cx, cy)  (quadtree.py:1095-1098)
 *       t, b, tot and the uniform fallback as above;  Py = t / tot
 *       top    : by = by * Py
 *       bottom : ay = ay + by * Py;  by = by * (1 - Py)                  (ay from the by before this line's second statement)
 *       rs, eL of that row;  Pl = (rs > 0) ? eL / rs : 0.5
 *       left   : bx = bx * Pl
 *       right  : ax = ax + bx * Pl;  bx = bx * (1 - Pl)
 *       if right: x0 = x0 + h;  if top: y0 = y0 + h;  s = h
 *   vx = (cx - x0) / s;  vy = (cy - y0) / s
 *   ux = ax + bx * vx;  uy = ay + by * vy,  each clamped to [0, ONE_M] as the warp clamps its input
 *   pdf_out = KDTree.pdf(p, dir)
 *
 *   [ax, ax+bx] x [ay, ay+by] is the preimage of the leaf cell: over the leaves of a quadtree these rectangles tile the unit
 *   square, and bx * by / s^2 = 4 pi * pdf up to rounding.  A direction inside a leaf of zero probability has an empty
 *   preimage: the call returns its limit point (bx or by is 0, so u is the corner (ax, ay) the neighbouring preimages share)
 *   and pdf 0.  The warp of that u is a direction of a neighbouring leaf, not this one.
 *
 * A quadtree (or a subtree) without any energy: the warp splits uniformly all the way down, so its preimages are the cells
 * themselves, and the pdf is 0 all the same -- KDTree.pdf's 0/0 (quadtree.py:1090-1092), the value pg_sample reports there too.
 *
 * Rounding: invert(warp(u)) returns u to within a few 2^-24 per level where the leaf's preimage is large; the warp quantises a
 * position inside a small leaf to fp32, so in a small, probable leaf the error in u is up to 2^-24 * max(|p|, s) / s times the
 * preimage's extent on that axis (tests/test_warp_model.py states the bound it checks).
 */
#ifndef PGSD_WARP_H
#define PGSD_WARP_H

#include "pgsd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The warp of u through the quadtree of the KD leaf that holds p.  Inactive lanes return dir (0,0,-1) and pdf 1, as
 * pg_sample's do. */
int pg_sample_warp(pg_context *ctx, uint64_t n, const float *p, const float *u, const uint8_t *active,
                   float *dir_out, float *pdf_out, void *stream);

/* The inverse: the u whose warp is dir (see above for directions of zero probability).  pdf_out may be NULL.  Inactive lanes
 * return u = (0, 0) and pdf 1. */
int pg_invert_warp(pg_context *ctx, uint64_t n, const float *p, const float *dir, const uint8_t *active,
                   float *u_out, float *pdf_out, void *stream);

/* pg_guide_bounce word for word, except that the lanes with select[i] == 2 take their direction from (u[i], u[n + i]) by
 * the warp: (dir_io, pdf_out) = warp(p, u).  There is no sampler argument; u is read on those lanes only. */
int pg_guide_bounce_warp(pg_context *ctx, uint64_t n, const float *p, const float *dir_nee,
                         const uint8_t *nee_active, const uint8_t *select, float *dir_io, const float *u,
                         float *pdf_nee_out, float *pdf_out, const uint32_t *lane_index,
                         const uint32_t *d_lane_count, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PGSD_WARP_H */
