/*
 * pgsd_bounce.h -- one call for a whole guided bounce: one entry point of libpgsd.so beside the 60 of pgsd.h, the three of
 * pgsd_warp.h, the seven of pgsd_fraction.h, the two of pgsd_target.h and the six of pgsd_radiance.h.
 *
 * A host that drives a bounce of the improved method ("Path Guiding in Production" ch. 10 for the learned BSDF sampling fraction,
 * Vorba and Krivanek 2016 for adjoint-driven roulette) asks the SD-tree four things at a path vertex p:
 *
 *   1. pg_fraction_query                          the leaf's fraction f                        (a KD descent)
 *   2. its own element-wise pass                  select = u > f ? 2 : 1
 *   3. pg_guide_bounce / pg_guide_bounce_warp     the NEE pdf; the pdf of, or a sample for, the continuation direction
 *                                                                                              (a second KD descent, the tree's head)
 *   4. pg_radiance_query                          the radiance estimate along the continuation direction
 *                                                                                              (a third KD descent, the head again)
 *
 * pg_bounce is that sequence as ONE kernel with ONE KD descent: the selection is made on the device from the leaf's fraction.
 * Every output is, bit for bit, what the sequence gives.  Nothing here is in the reference; nothing of pgsd.h changes
 * (PGSD_ABI_VERSION stays: an entry point was added).  The library's own renderer (pg_render_pass) does not use the call.
 * Conventions are those of pgsd.h: planar arrays in device memory, byte masks, the call asynchronous on `stream`, the same status
 * codes.  One kernel launch, no allocation, no synchronisation.
 *
 * ---- semantics of one processed lane i: the existing calls, composed in this order ----------------------------------------
 *
 * PROCESSED lanes.  Without a list (lane_index == NULL): every i < n.  With the list of pg_compact_lanes (lane_index,
 *   d_lane_count; built from `mode` in the place of pg_guide_bounce's select, and nee_active): the d_lane_count[0] slots from
 *   the front of lane_index and the d_lane_count[1] slots from its end, exactly the slots pg_guide_bounce would serve; no other
 *   slot of any output is written.  An entry i >= n (a list that pg_compact_lanes did not write for this n) touches nothing.
 *
 * LIVE lanes.   nee = nee_active ? nee_active[i] != 0 : 1;   m = mode ? mode[i] : PG_BOUNCE_CHOOSE;   m > 3 is PG_BOUNCE_NONE.
 *   A lane is live when nee or m != PG_BOUNCE_NONE -- when it would be in pg_guide_bounce.
 *
 * FRACTION f.
 *   With the learned fraction enabled (pg_fraction_enable): what pg_fraction_query answers for p with the lane active --
 *       f = logistic(theta of the KD leaf of p);   p outside the root box (inclusive test) or with a NaN coordinate:
 *       f = logistic(theta0).
 *   With it disabled: f = the context's constant as fp32 -- pg_setup's bsdf_sampling_fraction (0.5 on a context that only
 *       pg_import configured).
 *   A lane that is not live gets what pg_fraction_query gives an inactive lane, logistic(theta0) (the constant where the
 *   feature is disabled), and select 0, pdf_nee = pdf = 1, L_dir = L_mean = 0; dir_io and the stream are not touched.
 *
 * SELECTION sel.
 *       m = NONE: 0      m = PDF: 1      m = SAMPLE: 2
 *       m = CHOOSE:  xi = u_select[i];  with u_select == NULL, xi = ONE next_f32 of the lane's PCG32 stream (pgsd.h), drawn
 *                    before anything else by every live CHOOSE lane, whatever it then selects.
 *                    sel = xi > f ? 2 : 1          the reference's comparison (path_guiding_integrator.py:286): xi == f selects
 *                                                  1, and so does a NaN xi.
 *
 * GUIDE BOUNCE.  pdf_nee_out, pdf_out, dir_io and rng_state are those of
 *       pg_guide_bounce(select = sel, nee_active)         the PCG32 form (u == NULL); with a drawn xi the sample's draws follow
 *                                                         that one draw in the lane's stream
 *       pg_guide_bounce_warp(select = sel, nee_active, u) the warp form (u != NULL); no stream is read or written
 *   that is: pdf_nee = nee ? pg_pdf(p, dir_nee) : 1;  sel == 1: pdf = pg_pdf(p, dir_io);  sel == 2: dir_io and pdf are pg_sample's
 *   (pg_sample_warp's);  sel == 0: pdf = 1.
 *
 * RADIANCE (when L_dir_out or L_mean_out is given).  L_dir and L_mean are pg_radiance_query's answers for
 *       (p, dir_io AS IT STANDS AFTER THE GUIDE BOUNCE, active = sel != 0):
 *   the leaf is the one the descent reaches (the highest-numbered containing child, pgsd_radiance.h), positions outside the box
 *   get the root node's quadtree, N == 0 gives 0, and a lane with sel == 0 gets 0.  For a sampled lane the canonical form is
 *   derived again from the direction just written, as the sequence of calls would.
 *
 * DEPTH COUNTERS (pg_enable_depth_counters): the call adds nothing to them, like the calls of pgsd_warp.h.
 *
 * CHOOSE lanes of one wave take the sampling and the pdf-only path side by side.  pg_compact_lanes exists to keep a wave on one
 * of them, and that cannot be had when the device makes the choice: the list puts CHOOSE lanes among its pdf-only ones.  A host
 * that wants homogeneous waves keeps deciding itself and forces `mode` to PDF / SAMPLE.
 *
 * REFUSALS (PG_ERR_INVALID; pg_last_error names the reason): a NULL context or NULL args; with n > 0 a NULL p, dir_nee,
 *   dir_io, pdf_nee_out or pdf_out; lane_index and d_lane_count not given together; n > 2^32 - 1; neither u nor the rng_state /
 *   rng_inc pair; u_select == NULL without that pair, or together with u (the warp form has no stream to draw from); L_dir_out
 *   or L_mean_out given while pg_radiance_query would refuse -- the feature is off, valid = 0, or of_target != 0
 *   (pgsd_radiance.h).  A refused call launches nothing.  n = 0 does nothing.
 */
#ifndef PGSD_BOUNCE_H
#define PGSD_BOUNCE_H

#include "pgsd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_BOUNCE_NONE   0   /* no continuation query on this lane */
#define PG_BOUNCE_PDF    1   /* forced "bsdf-mis": pdf of dir_io */
#define PG_BOUNCE_SAMPLE 2   /* forced "sdtree-mis": sample the tree */
#define PG_BOUNCE_CHOOSE 3   /* decided on the device from the leaf's fraction */

typedef struct pg_bounce_args {
	/* in */
	const float *p;              /* Vector3f[n] */
	const float *dir_nee;        /* Vector3f[n] */
	const uint8_t *nee_active;   /* [n] or NULL = all */
	const uint8_t *mode;         /* [n] PG_BOUNCE_*, or NULL = all CHOOSE; a value > 3 is treated as NONE */
	const float *u_select;       /* Float[n] or NULL (PCG32 form only: drawn from the lane's stream) */
	const float *u;              /* Vector2f[n]: warp form (pgsd_warp.h); NULL: PCG32 form */
	uint64_t *rng_state;         /* PCG32 form; also required when u_select is NULL */
	const uint64_t *rng_inc;
	const uint32_t *lane_index;  /* both NULL or both set: the list of pg_compact_lanes, as in pg_guide_bounce */
	const uint32_t *d_lane_count;
	/* in/out */
	float *dir_io;               /* Vector3f[n]: the BSDF-sampled direction on entry */
	/* out */
	uint8_t *select_out;         /* [n]: 0, 1, 2 as pg_guide_bounce's select; may be NULL */
	float *fraction_out;         /* Float[n]; may be NULL */
	float *pdf_nee_out, *pdf_out;/* Float[n], required */
	float *L_dir_out, *L_mean_out; /* Float[n]; each may be NULL; both NULL: the radiance table is not needed */
} pg_bounce_args;

int pg_bounce(pg_context *ctx, uint64_t n, const pg_bounce_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PGSD_BOUNCE_H */
