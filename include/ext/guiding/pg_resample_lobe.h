/*
 * pg_resample_lobe.h -- product guiding for glossy surfaces: one entry point of libpgsd.so beside pg_resample_cosine
 * (pg_resample.h), whose parameters, conventions and outputs it shares.
 *
 * pg_resample_cosine samples radiance times the cosine about a normal: the product of a diffuse surface.  A rough conductor or a
 * plastic-like surface has a lobe that may be two degrees wide, and cosine candidates almost never land in it.
 * pg_resample_lobe resamples against a GGX reflection lobe: M candidates from the THREE-way mixture of the renderer's GGX
 * visible-normal sampling about the viewer's direction, the cosine lobe and the tree, each weighted by target over source, one
 * kept in a running reservoir, the unbiased contribution weight W handed back.  It is ONE kernel with ONE KD descent and one
 * read of the tree's head per lane, M quadtree walks and a reservoir of four numbers and a direction.
 *
 * Nothing here is in the reference; nothing of pgsd.h or pg_resample.h changes (PGSD_ABI_VERSION stays: an entry point was
 * added).  The library's own renderer (pg_render_pass) does not use the call.  Conventions are those of pg_resample_cosine:
 * planar arrays in device memory, byte masks with NULL meaning all lanes, the call asynchronous on `stream`, the same status
 * codes.  One kernel launch, no allocation, no synchronisation.  pg_resample_params is that call's, as it is: candidates 1..64,
 * alpha the share of LOBE candidates (GGX and cosine together), delta the defensive share of the target, reserved 0.
 *
 * ---- semantics of one lane i --------------------------------------------------------------------------------------------------
 *
 * All arithmetic is fp32, every operation rounded on its own (no contraction), in the order written.
 * INV_PI = 0.31830988618379067154f, INV_4PI = 0.07957747154594766788f.  make_frame, to_local, to_world, dot3 and normalize3 are
 * the renderer's: Duff et al.'s basis (s, t, n) of n;  to_local(v) = (dot3(v, s), dot3(v, t), dot3(v, n));
 * to_world(v) = ((s * v.x + t * v.y) + n * v.z);  dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z;
 * normalize3(v) = v / sqrt(dot3(v, v)).  rc_D, rc_G1 and rc_sample_m are the renderer's microfacet functions (Mitsuba's
 * MicrofacetDistribution::eval, smith_g1 and sample with sample_visible), a negative alpha naming GGX.
 *
 * A lane is VALID when it is active (active == NULL or active[i] != 0), every component of normal and of wi is finite,
 * PG_RESAMPLE_LOBE_MIN_ROUGHNESS = 1e-3f <= roughness <= 1 and 0 <= specular <= 1 (a NaN fails either range).  Any other lane
 * gets the "nothing kept" outputs below and zeros in all its candidate slots, and its stream is not touched.
 *
 * The KD leaf, and with it the quadtree, are pg_sample's for p -- also for a p outside the root box or with a NaN coordinate.
 * n is the normal AS GIVEN, wi the world direction away from the surface towards the viewer AS GIVEN: unit length is the
 * caller's business.  Per valid lane:
 *      fr  = make_frame(n)          wil = to_local(fr, wi)          a = -roughness      (the renderer's sign for GGX)
 *      sg  = wil.z > 0 ? specular : 0                               oms = 1 - sg
 *      om  = 1 - alpha              d4 = delta * INV_4PI            omd = 1 - delta
 *
 * THE GGX DENSITY g(wl) of a local direction wl is 0 unless wil.z > 0 && wl.z > 0, and then
 *      H  = normalize3(wl + wil)
 *      D  = rc_D(H, a)                     when D == 0: g = 0
 *      gi = rc_G1(wil, H, a)
 *      g  = (dot3(wil, H) > 0 && dot3(wl, H) > 0) ? (D * gi) / (4 * wil.z) : 0
 * the pdf of the renderer's rough conductor (rc_eval_pdf): the density of the reflection of wil about a visible normal.
 *
 * M = candidates, wsum = 0, nothing kept.  Then for k = 0 .. M-1, on the lane's PCG32 stream (pgsd.h):
 *
 *   1. xi = next_f32.  The candidate comes from the tree when xi > alpha (xi == alpha: the lobe).  A tree candidate: (w_k, q)
 *      are exactly pg_sample's direction and pdf, with the draws pg_sample makes (three per visited quadtree node).
 *   2. Otherwise it comes from the lobe and ALWAYS draws xi2 = next_f32, u1 = next_f32, u2 = next_f32, in that order.
 *      When xi2 < sg it is a GGX candidate:
 *          m   = rc_sample_m(wil, a, u1, u2, pdf_m)
 *          wim = dot3(wil, m)
 *          o   = m * (2 * wim) - wil
 *      It FAILED when !(pdf_m != 0 && o.z > 0): then w_k = (0, 0, 0), no pdf walk is made and t = s = 0 (so w = 0 in step 3).
 *      Otherwise w_k = to_world(fr, o).
 *      When !(xi2 < sg) it is a cosine candidate, pg_resample_cosine's: w_k = to_world(fr, square_to_cosine_hemisphere(u1, u2)).
 *      q = what pg_pdf(p, w_k) returns, for a lobe candidate that did not fail.
 *   3. For a candidate that did not fail:
 *          wl = to_local(fr, w_k)
 *          c  = wl.z > 0 ? wl.z * INV_PI : 0                           the clamped cosine lobe's density
 *          b  = sg == 0 ? c : (sg * g(wl)) + (oms * c)                 with sg == 0, g is not evaluated
 *          b  = isfinite(b) ? b : 0
 *          s  = alpha * b + om * q                                     the SOURCE density of the candidate
 *          t  = b * (d4 + omd * q)                                     the TARGET: b times the defensive mixture of the tree
 *          w  = (s > 0 && t > 0 && isfinite(t / s)) ? t / s : 0
 *   4. zeta = next_f32;  wsum = wsum + w;  if (w > 0 && zeta * wsum < w) keep k, w_k, t and s.
 *
 * Every candidate consumes its draws whether or not it can be kept.  After the loop, with a candidate kept:
 *      dir_out = w_kept,   W = weight_out = (wsum / (float)M) / t_kept,   target_out = t_kept,   source_out = s_kept,
 *      index_out = k_kept
 * and with nothing kept:
 *      dir_out = (0, 0, -1),   W = 0,   target_out = 0,   source_out = 0,   index_out = PG_RESAMPLE_NONE.
 * rng_state[i] is the stream behind the last draw.
 *
 * With the candidate arrays (the layouts of pg_resample_args): cand_dir_out[(k * 3 + axis) * n + i] = w_k,
 * cand_target_out[k * n + i] = t and cand_source_out[k * n + i] = s of every candidate k < M, kept or not.
 *
 * WHAT b IS.  The density of every candidate, GGX ones included, is evaluated by g; the sample's own pdf_m serves the failure
 * test only.  b = sg * g + (1 - sg) * c is the density the lobe candidates are drawn with, and a proxy for BSDF times cosine: for
 * a plastic-like surface it mixes the visible-normal density of the specular part with the cosine of the diffuse part; specular
 * 1 is a rough conductor, specular 0 is pg_resample_cosine's target.  b integrates to LESS than 1: a reflection below the
 * horizon is lost (the failed candidates), not redistributed.
 *
 * THE ESTIMATOR the host forms is f(dir_out) * W, f being the WHOLE integrand (radiance times BSDF times cosine).  For
 * delta > 0 it is unbiased for every f that vanishes where b does: the target is then positive wherever such an f is, and a
 * failed candidate has weight 0 as a candidate outside the support has.  With delta = 0 the target also vanishes where the
 * tree's density does, and the estimator is unbiased only for an f that vanishes there too.  W * t_kept = wsum / M estimates the
 * target's integral; with M = 1, W = 1 / s_kept: the one-sample mixture.
 *
 * REFUSALS (PG_ERR_INVALID; pg_last_error names the reason): a NULL context, params or args; with n > 0 a NULL p, normal, wi,
 *   roughness, specular, rng_state, rng_inc, dir_out or weight_out; candidates outside 1..64; alpha or delta outside [0, 1] or
 *   NaN; reserved != 0; n > 2^32 - 1.  A refused call launches nothing.  n = 0 does nothing.
 *
 * NOT BUILT: Beckmann lobes; anisotropy (one roughness per lane); transmission (rough dielectrics: reflection lobes only); a
 *   warp form (caller-supplied points in the place of the stream); the learned fraction of pgsd_fraction.h as alpha; any use
 *   by pg_render_pass; compacted lane lists (pg_compact_lanes).
 */
#ifndef PG_RESAMPLE_LOBE_H
#define PG_RESAMPLE_LOBE_H

#include "../../pg_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_RESAMPLE_LOBE_MIN_ROUGHNESS 1e-3f   /* a lane with a smaller roughness is not valid */

typedef struct pg_resample_lobe_args {
	const float *p, *normal, *wi;     /* Vector3f[n] each */
	const float *roughness, *specular; /* Float[n] each */
	const uint8_t *active;            /* [n] or NULL */
	uint64_t *rng_state; const uint64_t *rng_inc;
	float *dir_out;                   /* Vector3f[n], required */
	float *weight_out;                /* Float[n], required: W */
	float *target_out, *source_out;   /* Float[n], each may be NULL: t and s of the kept candidate */
	uint32_t *index_out;              /* [n] or NULL: k of the kept candidate, PG_RESAMPLE_NONE if none */
	float *cand_dir_out;              /* float[M][3][n] or NULL */
	float *cand_target_out, *cand_source_out; /* float[M][n] or NULL */
} pg_resample_lobe_args;

int pg_resample_lobe(pg_context *ctx, uint64_t n, const pg_resample_params *params,
                     const pg_resample_lobe_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PG_RESAMPLE_LOBE_H */
