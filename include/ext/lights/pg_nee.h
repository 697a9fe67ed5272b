/*
 * pg_nee.h -- resampled next-event estimation: a light AND a point on it per path vertex, by resampled importance sampling of
 * candidates drawn from the learned row of the vertex's KD leaf.  Three entry points of libpgsd.so beside those of pg_lights.h.
 *
 * pg_lights_sample draws a light from the row of the KD leaf.  The row is an average over every vertex the leaf has seen: it
 * knows nothing of THIS vertex's normal or of its distance to each light, and nothing of where on a large light to sample.
 * pg_nee_resample multiplies the row's knowledge by what only the vertex knows (Talbot, Cline and Egbert 2005, with a learned
 * source): M candidates (a light from the row, then a uniform point on it), each weighted by target over source -- the target is
 * the unshadowed contribution on a diffuse surface --, one of them kept in proportion to its weight by a running reservoir, and
 * the unbiased contribution weight W handed back.  The host traces ONE shadow ray, not M.  A host could compose the method
 * from M pg_lights_sample launches (M KD descents) and element-wise passes over (M, n) arrays, and would have to bring every
 * point sample and geometry term itself: the library knew nothing of a light beyond its index.  Here it is ONE kernel with ONE
 * KD descent, M row selections, M gathers of a 64-byte light record and a reservoir in registers.
 *
 * Nothing here is in the reference; nothing of pgsd.h or pg_lights.h changes (PGSD_ABI_VERSION stays: entry points were added).
 * The library's own renderer (pg_render_pass) does not use the calls.  Conventions are those of pg_lights.h: device pointers
 * unless named h_*, planar layout, byte masks with NULL = all active, calls asynchronous on `stream`, the same status codes.
 *
 * ---- the light table: pg_nee_set_lights ---------------------------------------------------------------------------------------
 *
 * h_table is a HOST array of 12 words per light j < n_lights:
 *     o[3], a[3], b[3]      float: a corner and the two edges that leave it
 *     radiance              float: a scalar, such as the host's luminance of the emitted radiance; finite and >= 0
 *     kind                  uint32 bits: 0 a parallelogram { o + e1 a + e2 b : e1, e2 in [0, 1) }, 1 the triangle o, o + a, o + b
 *     two_sided             uint32 bits: 0 the light emits on the side its normal N points to, 1 on both
 * n_lights is in 1 .. PG_LIGHTS_MAX; 0 frees the table (h_table may be NULL).  The call refuses (PG_ERR_INVALID) a NULL
 * h_table, a non-finite or negative radiance, kind > 1, two_sided > 1 and any non-finite coordinate of o, a or b; a refused call
 * leaves the table that was there.  A prepare kernel writes one 64-byte device record per light -- o, a, b, N, invA, radiance,
 * and in the spare words kind and two_sided.  All arithmetic is fp32, every operation rounded on its own (no contraction), in the
 * order written:
 *     c    = cross(a, b)                          cx = ay * bz - az * by,  cy = az * bx - ax * bz,  cz = ax * by - ay * bx
 *     len2 = (cx * cx + cy * cy) + cz * cz
 *     len  = sqrt(len2)                           (IEEE)
 *     N    = c / len                              component-wise (a degenerate light: whatever that gives; it is never used)
 *     area = kind ? 0.5f * len : len
 *     invA = (len > 0 && isfinite(len)) ? 1 / area : 0
 * A degenerate light (len 0, or edges so long that len2 overflows) has invA = 0 and is never kept.
 * The table belongs to the context and does not depend on the tree: pg_setup, pg_import and a refine leave it alone, setting it
 * again replaces it, pg_destroy frees it.  A context that never sets it allocates and behaves exactly as before.  The call
 * synchronises the device.
 *
 * pg_nee_status: *n_lights = the table's, 0 when none is set.
 *
 * ---- pg_nee_resample: semantics of one lane i ---------------------------------------------------------------------------------
 *
 * The call requires a table and the lights feature enabled (pg_lights_enable) with n_lights equal to the table's.
 * A lane is VALID when it is active and every component of its normal is finite.  n = (nx, ny, nz) is the normal AS GIVEN.
 * The row is found as pg_lights_sample finds it: the KD leaf of p; a position outside the root box or with a NaN coordinate
 * behaves as an unlearned leaf.  M = candidates, wsum = 0, nothing kept.  Then for k = 0 .. M-1, on the lane's PCG32 stream
 * (pgsd.h), every candidate makes EXACTLY FOUR draws:
 *
 *   1. u = next_f32;  j = SELECT(leaf, u);  pm = PMF(leaf, j)         the two functions of pg_lights.h as they are, with the
 *                                                                      lights feature's own delta
 *   2. e1 = next_f32, e2 = next_f32.  A triangle: if (e1 + e2 > 1) { e1 = 1 - e1; e2 = 1 - e2; }
 *      y = (o + e1 * a) + e2 * b                                       per component
 *   3. v = y - p;  d2 = (vx * vx + vy * vy) + vz * vz;  dist = sqrt(d2);  w = v / dist   component-wise
 *   4. cs = (nx * wx + ny * wy) + nz * wz
 *      cl = -((Nx * wx + Ny * wy) + Nz * wz);  a two-sided light: cl = fabsf(cl)
 *      g  = (d2 > 0 && cs > 0 && cl > 0) ? (cs * cl) / d2 : 0
 *      t  = radiance_j * g                                             the TARGET: the unshadowed contribution on a diffuse
 *                                                                      surface, up to the albedo
 *      s  = pm * invA_j                                                the SOURCE: the density of y in area measure
 *      wgt = (s > 0 && t > 0 && isfinite(t / s)) ? t / s : 0
 *   5. zeta = next_f32;  wsum = wsum + wgt;  if (wgt > 0 && zeta * wsum < wgt) keep k, j, y, w, dist, t and s.
 *
 * After the loop, with a candidate kept:
 *      light_out = j_kept,  point_out = y_kept,  W = weight_out = (wsum / (float)M) / t_kept,
 *      dir_out = w_kept,  dist_out = dist_kept,  target_out = t_kept,  source_out = s_kept,  index_out = k_kept
 * and with nothing kept: light_out = PG_LIGHTS_NONE, index_out = PG_RESAMPLE_NONE, zeros everywhere else.
 * rng_state[i] is the stream behind the last draw: a valid lane's stream advances by 4 M draws whatever happens.
 *
 * With the candidate arrays (the layouts of pg_resample_args): cand_light_out[k * n + i] = j, cand_point_out[(k * 3 + axis) * n
 * + i] = y, cand_target_out[k * n + i] = t and cand_source_out[k * n + i] = s of every candidate k < M, kept or not.  They are
 * for a host whose BSDF is not diffuse and that resamples the same candidates itself.
 *
 * An INVALID lane gets the "nothing kept" outputs, zeros in all its candidate slots, and its stream is not touched.
 *
 * THE ESTIMATOR the host forms is f(y) * W, f being the WHOLE integrand in area measure: emitted radiance times BSDF times both
 * cosines over the squared distance times the visibility the host's one shadow ray decides.  It is unbiased when every light has
 * pm > 0 -- the lights feature's delta > 0, or an unlearned leaf -- and f vanishes where t does: behind the surface, behind a
 * one-sided light, on a light of radiance 0.  W * t_kept = wsum / M estimates the target's integral over the lights; with M = 1,
 * W = 1 / s_kept: what a host gets today from pg_lights_sample and a uniform point.
 *
 * REFUSALS (PG_ERR_INVALID; pg_last_error names the reason): those of pg_resample_cosine -- a NULL context, params or args; with
 *   n > 0 a NULL p, normal, rng_state, rng_inc, light_out, point_out or weight_out; candidates outside 1..64; a reserved word
 *   != 0; n > 2^32 - 1 -- and: no table set; the lights feature disabled; its n_lights not the table's.  A refused call launches
 *   nothing.  n = 0 does nothing.  One kernel launch, no allocation, no synchronisation.
 *
 * NOT BUILT.  None of these exists:
 *   - spheres, point, directional and environment lights;
 *   - targets with a glossy lobe (the cand_* arrays serve that host);
 *   - feeding the rows from this call (a host records with pg_lights_record as before);
 *   - a remapped u;
 *   - compacted lane lists;
 *   - any use by pg_render_pass.
 */
#ifndef PG_NEE_H
#define PG_NEE_H

#include "../../pg_resample.h"
#include "../pg_lights.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_NEE_TABLE_WORDS 12 /* 32-bit words of h_table per light */

typedef struct pg_nee_params {
	uint32_t candidates;  /* M, 1..PG_RESAMPLE_MAX_CANDIDATES */
	uint32_t reserved[3]; /* 0 */
} pg_nee_params;

typedef struct pg_nee_args {
	const float *p, *normal;          /* Vector3f[n] each */
	const uint8_t *active;            /* [n] or NULL */
	uint64_t *rng_state; const uint64_t *rng_inc;
	uint32_t *light_out;              /* [n], required: the kept light, PG_LIGHTS_NONE if none */
	float *point_out;                 /* Vector3f[n], required: y */
	float *weight_out;                /* Float[n], required: W */
	float *dir_out;                   /* Vector3f[n] or NULL: the unit direction from p to y */
	float *dist_out;                  /* Float[n] or NULL */
	float *target_out, *source_out;   /* Float[n], each may be NULL: t and s of the kept candidate */
	uint32_t *index_out;              /* [n] or NULL: k of the kept candidate, PG_RESAMPLE_NONE if none */
	uint32_t *cand_light_out;         /* uint32[M][n] or NULL */
	float *cand_point_out;            /* float[M][3][n] or NULL */
	float *cand_target_out, *cand_source_out; /* float[M][n] or NULL */
} pg_nee_args;

int pg_nee_set_lights(pg_context *ctx, uint32_t n_lights, const float *h_table, void *stream);

int pg_nee_status(pg_context *ctx, uint32_t *n_lights);

int pg_nee_resample(pg_context *ctx, uint64_t n, const pg_nee_params *params, const pg_nee_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PG_NEE_H */
