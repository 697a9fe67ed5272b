/*
 * pgsd_irradiance.h -- irradiance estimates per spatial leaf (order-2 spherical harmonics) and Russian roulette / splitting on
 * them: six entry points of libpgsd.so beside those of pgsd.h, pgsd_warp.h, pgsd_fraction.h, pgsd_target.h, pgsd_radiance.h and
 * pgsd_bounce.h.
 *
 * pgsd_radiance.h answers "how much radiance arrives at p from direction w".  A diffuse surface needs none of that for ONE
 * direction: its cache entry, and Vorba and Krivanek's adjoint at a vertex, is rho / pi times
 *
 *       E(p, n) = integral of L(p, w) max(0, n.w) dw,
 *
 * the irradiance around the normal n.  This header answers that FOURTH question.  The quadtree of a KD leaf is piecewise constant
 * over an equal-area map (canonicalToDir: z = 2 cy - 1, phi = 2 pi cx), so the projection of its radiance onto the nine real
 * spherical harmonics up to order 2 is a closed-form sum over its leaves, done once per tree and iteration (pg_irradiance_build);
 * the irradiance for any normal is then nine multiply-adds behind one KD descent (Ramamoorthi and Hanrahan, "An Efficient
 * Representation for Irradiance Environment Maps", SIGGRAPH 2001).  The order-2 approximation of the clamped cosine,
 * 1/4 + c/2 + (15/32)(c^2 - 1/3), differs from max(c, 0) by at most 3/32 (at c = 0), so with L >= 0
 *
 *       |E_estimate - E_of_the_tree| <= (3/32) R / N          (R: the tree's root energy, N: its statistical weight).
 *
 * Nothing here is in the reference; nothing of pgsd.h or of the other headers changes (PGSD_ABI_VERSION stays: entry points were
 * added).  Conventions are those of pgsd_radiance.h: planar float[3][n] arrays in device memory, byte masks (NULL = all lanes
 * active), calls asynchronous on `stream`, the same status codes, a NULL context gives PG_ERR_INVALID, one kernel launch and no
 * allocation in the two query calls.  A context that never calls pg_irradiance_build allocates and launches exactly what it did
 * before.
 *
 * ---- state ----------------------------------------------------------------------------------------------------------------
 *
 * Nine fp32 per quadtree of sdTree_prev (numbered as pg_radiance_export numbers them), and a flag `built`.
 *
 *   pg_irradiance_build    needs what the estimates of pgsd_radiance.h need -- the radiance feature on, valid = 1, of_target = 0
 *                          (it reads N, the statistical weights) -- and refuses otherwise (PG_ERR_INVALID, pg_last_error names the
 *                          reason).  It allocates or reuses the table and the buffers of the build (they are kept between builds),
 *                          launches on `stream`, and sets built = 1.
 *   built is cleared by whatever replaces sdTree_prev or its weights: the commit of pg_refine_and_swap (a refine that FAILS leaves
 *                          built, the table and every answer as they were: pgsd.h, a refine is a transaction), pg_setup, pg_import,
 *                          pg_radiance_enable(0) and pg_radiance_import.
 *   pg_irradiance_import   the checkpoint path, as pg_radiance_import is: n_trees must equal pg_export_sizes' n_roots, the same
 *                          three conditions as the build; built = 1, the host vouches for the values.
 *   pg_irradiance_export   refuses while built = 0.  Both synchronise the device.
 *
 * ---- the table: fp64, every operation rounded on its own (no contraction), only + - * / sqrt rint, in this order ----------
 *
 * Per tree t:  R = the root's energy (fp32),  N = weight[t] (pgsd_radiance.h).  Every directional LEAF of the tree has an energy e
 * (fp32) and a cell [x0, x1] x [y0, y1] of the unit square: with d its depth (the root is 0) and (ix, iy) its integer position,
 * w = 2^-d, x0 = ix w, x1 = (ix + 1) w, y0 = iy w, y1 = (iy + 1) w, all exact.  (Child 0 of a node is the half x >= mx, y >= my,
 * child 1 x <= mx, y >= my, child 2 x <= mx, y <= my, child 3 x >= mx, y <= my: pgsd_radiance.h.)
 *
 *   of the interval [y0, y1]:
 *       z_i = 2 y_i - 1                                    exact
 *       s_i = sqrt(1 - z_i * z_i)
 *       A_i = asin z_i = atan2(z_i, s_i):   a = |z_i|;  hi = max(a, s_i), lo = min(a, s_i);  u = lo / hi;  v = atan_unit(u), the
 *             double series of pgsd.h's atan2 (reduction at sqrt 2 - 1, twenty terms);  if a > s_i: v = pi/2 - v;  if z_i < 0: v = -v
 *       F_i = (z_i * s_i + A_i) / 2
 *       Zz  = (z0 + z1) / 2
 *       Zs  = (F_1 - F_0) / (2 w)
 *       Zzs = (0 - ((s1 * s1) * s1 - (s0 * s0) * s0)) / (6 w)
 *       Zss = ((z1 - ((z1 * z1) * z1) / 3) - (z0 - ((z0 * z0) * z0) / 3)) / (2 w)
 *       Z20 = ((z1 * z1 + z1 * z0) + z0 * z0) - 1
 *   of the interval [x0, x1], with turn(f) = (sin, cos) of 2 pi f for a dyadic f in [0, 2]:  k = rint(4 f) (exact),
 *       r = (f - k * 0.25) * 6.283185307179586, then the two double series of pgsd.h's sincos (sine to r^17, cosine to r^18)
 *       and its quadrant selection by k mod 4 -- so that the sine of a whole turn is 0:
 *       (sa_i, ca_i) = turn(x_i),   (sb_i, cb_i) = turn(2 x_i)
 *       C1 = (sa_1 - sa_0) / (6.283185307179586 w)          S1 = (ca_0 - ca_1) / (6.283185307179586 w)
 *       C2 = (sb_1 - sb_0) / (12.566370614359172 w)         S2 = (cb_0 - cb_1) / (12.566370614359172 w)
 *   the means over the cell of the nine polynomials b = (1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2) of the unit direction:
 *       m = (1,  Zs * S1,  Zz,  Zs * C1,  (Zss * S2) / 2,  Zzs * S1,  Z20,  Zzs * C1,  Zss * C2)
 *   the leaf's share of coefficient j:
 *       t_j = ((double)e / (double)R) * m_j;   NaN -> 0;   clamped to +-2^10;   q_j = (int64) rint(t_j * 2^50)
 *   and sum_j = the sum of q_j over the leaves of the tree as an EXACT INTEGER MODULO 2^64 (the project's way): the
 *   table does not depend on the order in which leaves are visited.  For a tree this library resolved, the leaves' energies sum
 *   to the root's up to one rounding each and the polynomials lie in [-1, 2], so |sum_j| < 2.1 * 2^50; an IMPORTED tree with
 *   inconsistent energies wraps, always the same way.  A tree whose root is the leaf has the one cell [0, 1]^2 with e = R.
 *
 *   With g = (1/4, 1/2, 1/2, 1/2, 15/16, 15/16, 5/64, 15/16, 15/64) (A_l K_lm^2 folded; all exact):
 *       k_j = (float)((((double)sum_j * 2^-50) * g_j) * ((double)R / (double)N))        sum_j as a signed int64
 *   All nine are 0 where N == 0, or R is not positive, or R is not finite.   (An isotropic tree has R = 4 pi N L0: k_0 = pi L0.)
 *
 * ---- the estimate: fp32, every operation rounded on its own, in this order ------------------------------------------------
 *
 *   KD leaf:  pg_pdf's; a position outside the root box (inclusive test) or NaN gets the root node and ITS tree.  k = the nine
 *   coefficients of the node's tree, n = (nx, ny, nz) the normal AS GIVEN (unit length is the host's business):
 *       S = ((((((((k0 + k1 * ny) + k2 * nz) + k3 * nx) + (k4 * nx) * ny) + (k5 * ny) * nz) + k6 * ((3 * nz) * nz - 1))
 *              + (k7 * nx) * nz) + k8 * (nx * nx - ny * ny))
 *       E = S > 0 ? S : 0                                  (a NaN gives 0)
 *   A normal with a non-finite component gives E = 0.  normal == NULL: S = k0, the mean over all orientations.
 *   Inactive lanes: E = 0.
 *
 * ---- the decision (pg_irradiance_rr) ----------------------------------------------------------------------------------------
 *
 *   The DECISION of pgsd_radiance.h with L replaced by E: q = (w * E) / I, the same window, branches and exactly ONE PCG32 draw
 *   per active lane.  The host folds rho / pi into `weight`.  Inactive lanes: count = 1, scale = 1, E = 0, the stream is not touched.
 *
 * REFUSALS of the two query calls (PG_ERR_INVALID): built = 0 ("call pg_irradiance_build"); a NULL required pointer; for
 *   pg_irradiance_rr the parameter checks of pg_radiance_rr.  n = 0 does nothing.
 *
 * NOT BUILT: any use by the library's own renderer (pg_render_pass); estimates from a second-moment tree; RGB; compacted lane
 *   lists; and the npz schema of the tree files does not change -- a host saves pg_irradiance_export's array beside the tree.
 */
#ifndef PGSD_IRRADIANCE_H
#define PGSD_IRRADIANCE_H

#include "pgsd_radiance.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Projects every quadtree of sdTree_prev (see above).  Asynchronous on `stream` once its buffers exist. */
int pg_irradiance_build(pg_context *ctx, void *stream);

/* The flag; the pointer may be NULL. */
int pg_irradiance_status(pg_context *ctx, int32_t *built);

/* The coefficients to / from host memory: float[n_trees][9], n_trees = pg_export_sizes' n_roots. */
int pg_irradiance_export(pg_context *ctx, uint64_t n_trees, float *h_coeff);
int pg_irradiance_import(pg_context *ctx, uint64_t n_trees, const float *h_coeff);

/* p: float[3][n]; normal: float[3][n] or NULL; active: uint8[n] or NULL; E_out: float[n]. */
int pg_irradiance_query(pg_context *ctx, uint64_t n, const float *p, const float *normal, const uint8_t *active, float *E_out,
                        void *stream);

/* p: float[3][n]; normal: float[3][n] or NULL; weight, reference: float[n]; rng_state, rng_inc: the lanes' PCG32 streams; active:
 * uint8[n] or NULL; count_out: uint32[n]; scale_out: float[n]; E_out: float[n] or NULL. */
int pg_irradiance_rr(pg_context *ctx, uint64_t n, const float *p, const float *normal, const float *weight,
                     const float *reference, const pg_rr_params *params, uint64_t *rng_state, const uint64_t *rng_inc,
                     const uint8_t *active, uint32_t *count_out, float *scale_out, float *E_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PGSD_IRRADIANCE_H */
