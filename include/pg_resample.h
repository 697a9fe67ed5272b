/*
 * pg_resample.h -- product guiding for diffuse surfaces: one entry point of libpgsd.so beside those of the pgsd*.h headers.
 *
 * The SD-tree samples a direction in proportion to incident radiance (pg_sample) and knows the integral of radiance times the
 * cosine about a normal (pgsd_irradiance.h), but cannot sample that product.  pg_resample_cosine does, by resampled importance
 * sampling (Talbot, Cline and Egbert 2005): M cheap candidates from the one-sample mixture of the cosine lobe and the tree,
 * each weighted by target over source, one of them kept in proportion to its weight by a running reservoir, and the unbiased
 * contribution weight W handed back.  A host could compose the method from pg_sample and pg_pdf: M KD descents, 2M launches
 * and M round trips of the candidates through memory.  Here it is ONE kernel with ONE KD descent and one read of the tree's
 * head, M quadtree walks and a reservoir of four numbers and a direction.
 *
 * Nothing here is in the reference; nothing of pgsd.h changes (PGSD_ABI_VERSION stays: an entry point was added).  The
 * library's own renderer (pg_render_pass) does not use the call.  Conventions are those of pgsd_bounce.h: planar arrays in
 * device memory, byte masks with NULL meaning all lanes, the call asynchronous on `stream`, the same status codes.  One kernel
 * launch, no allocation, no synchronisation.
 *
 * ---- semantics of one active lane i -------------------------------------------------------------------------------------------
 *
 * All arithmetic is fp32, every operation rounded on its own (no contraction), in the order written.
 * INV_PI = 0.31830988618379067154f, INV_4PI = 0.07957747154594766788f.
 *
 * The KD leaf, and with it the quadtree, are pg_sample's for p -- also for a p outside the root box or with a NaN coordinate
 * (the root node's quadtree).  n = (nx, ny, nz) is the normal AS GIVEN: unit length is the caller's business.
 * M = candidates, om = 1 - alpha, wsum = 0, nothing kept.  Then for k = 0 .. M-1, on the lane's PCG32 stream (pgsd.h):
 *
 *   1. xi = next_f32.  The candidate comes from the tree when xi > alpha, otherwise from the cosine lobe -- the reference's
 *      comparison (path_guiding_integrator.py:286): xi == alpha gives cosine, and so would a NaN xi.
 *   2. A tree candidate: (w_k, q) are exactly pg_sample's direction and pdf, with the draws pg_sample makes (three per visited
 *      quadtree node).
 *      A cosine candidate: u1 = next_f32, u2 = next_f32,
 *          w_k = to_world(coordinate_system(n), square_to_cosine_hemisphere(u1, u2))
 *      the renderer's own functions (Duff et al.'s basis of n; the concentric disk map with z = sqrt(1 - r^2), 1e-10 in the
 *      place of 0), and q = what pg_pdf(p, w_k) returns.
 *   3. d = (nx * wx + ny * wy) + nz * wz
 *      c = d > 0 ? d * INV_PI : 0                                  the clamped cosine lobe's density
 *      s = alpha * c + om * q                                      the SOURCE density of the candidate
 *      t = c * (delta * INV_4PI + (1 - delta) * q)                 the TARGET: cosine times the defensive mixture of the tree
 *      w = (s > 0 && t > 0 && isfinite(t / s)) ? t / s : 0
 *   4. zeta = next_f32;  wsum = wsum + w;  if (w > 0 && zeta * wsum < w) keep k, w_k, t and s.
 *
 * Every candidate consumes its draws whether or not it can be kept.  After the loop, with a candidate kept:
 *      dir_out = w_kept,   W = weight_out = (wsum / (float)M) / t_kept,   target_out = t_kept,   source_out = s_kept,
 *      index_out = k_kept
 * and with nothing kept:
 *      dir_out = (0, 0, -1),   W = 0,   target_out = 0,   source_out = 0,   index_out = 0xFFFFFFFF.
 * rng_state[i] is the stream behind the last draw.
 *
 * With the candidate arrays: cand_dir_out[(k * 3 + axis) * n + i] = w_k, cand_target_out[k * n + i] = t and
 * cand_source_out[k * n + i] = s of every candidate k < M, kept or not.
 *
 * An INACTIVE lane (active[i] == 0), or a lane whose normal has a non-finite component, gets the "nothing kept" outputs,
 * zeros in all its candidate slots, and its stream is not touched.
 *
 * THE ESTIMATOR the host forms is f(dir_out) * W, f being the WHOLE integrand (radiance times BSDF times cosine).  For
 * delta > 0 it is unbiased for every f that vanishes where n.w <= 0: the target is then positive wherever such an f is.  With
 * delta = 0 the target vanishes where the tree's density does, and the estimator is unbiased only for an f that vanishes there
 * too.  W * t_kept = wsum / M estimates the target's integral; with M = 1, W = 1 / s_kept: the one-sample mixture.
 *
 * REFUSALS (PG_ERR_INVALID; pg_last_error names the reason): a NULL context, params or args; with n > 0 a NULL p, normal,
 *   rng_state, rng_inc, dir_out or weight_out; candidates outside 1..64; alpha or delta outside [0, 1] or NaN; reserved != 0;
 *   n > 2^32 - 1.  A refused call launches nothing.  n = 0 does nothing.
 *
 * NOT BUILT: a warp form (caller-supplied points in the place of the stream); targets other than the clamped cosine (the
 *   cand_* arrays are what a host with another BSDF resamples itself); the learned fraction of pgsd_fraction.h as alpha; any
 *   use by pg_render_pass; compacted lane lists (pg_compact_lanes).
 */
#ifndef PG_RESAMPLE_H
#define PG_RESAMPLE_H

#include "pgsd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_RESAMPLE_MAX_CANDIDATES 64
#define PG_RESAMPLE_NONE 0xFFFFFFFFu   /* index_out of a lane that kept nothing */

typedef struct pg_resample_params {
	uint32_t candidates;   /* M, 1..64 */
	float alpha;           /* share of cosine candidates, [0,1] */
	float delta;           /* defensive share of the target, [0,1] */
	uint32_t reserved;     /* 0 */
} pg_resample_params;

typedef struct pg_resample_args {
	const float *p, *normal;          /* Vector3f[n] each */
	const uint8_t *active;            /* [n] or NULL */
	uint64_t *rng_state; const uint64_t *rng_inc;
	float *dir_out;                   /* Vector3f[n], required */
	float *weight_out;                /* Float[n], required: W */
	float *target_out, *source_out;   /* Float[n], each may be NULL: t and s of the kept candidate */
	uint32_t *index_out;              /* [n] or NULL: k of the kept candidate, 0xFFFFFFFF if none */
	float *cand_dir_out;              /* float[M][3][n] or NULL */
	float *cand_target_out, *cand_source_out; /* float[M][n] or NULL */
} pg_resample_args;

int pg_resample_cosine(pg_context *ctx, uint64_t n, const pg_resample_params *params,
                       const pg_resample_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PG_RESAMPLE_H */
