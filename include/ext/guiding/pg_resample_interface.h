/*
 * pg_resample_interface.h -- product guiding through rough glass: one entry point of libpgsd.so beside pg_resample_lobe
 * (pg_resample_lobe.h) and pg_resample_cosine (pg_resample.h), whose parameters, conventions and outputs it shares.
 *
 * pg_resample_lobe samples radiance times a GGX REFLECTION lobe: its density is 0 below the horizon, and light that arrives
 * THROUGH a frosted pane gets no lobe candidate and no target.  pg_resample_interface resamples against the two-sided lobe of a
 * rough dielectric interface: M candidates from the TWO-way mixture of the renderer's rough-dielectric sampling (reflection or
 * refraction, chosen by Fresnel, about a GGX visible normal) and the tree, each weighted by target over source, one kept in a
 * running reservoir, the unbiased contribution weight W handed back.  The SD-tree's quadtree covers both hemispheres, so the
 * tree's half of the product exists on the far side as it stands.  It is ONE kernel with ONE KD descent and one read of the
 * tree's head per lane, M quadtree walks and a reservoir of four numbers and a direction.
 *
 * Nothing here is in the reference; nothing of pgsd.h, pg_resample.h or pg_resample_lobe.h changes (PGSD_ABI_VERSION stays: an
 * entry point was added).  The library's own renderer (pg_render_pass) does not use the call.  Conventions are those of
 * pg_resample_cosine: planar arrays in device memory, byte masks with NULL meaning all lanes, the call asynchronous on `stream`,
 * the same status codes.  One kernel launch, no allocation, no synchronisation.  pg_resample_params is that call's, as it is:
 * candidates 1..64, alpha the share of LOBE candidates, delta the defensive share of the target, reserved 0.
 *
 * ---- semantics of one lane i --------------------------------------------------------------------------------------------------
 *
 * All arithmetic is fp32, every operation rounded on its own (no contraction), in the order written.
 * INV_4PI = 0.07957747154594766788f.  make_frame, to_local, to_world, dot3 and normalize3 are the renderer's: Duff et al.'s basis
 * (s, t, n) of n;  to_local(v) = (dot3(v, s), dot3(v, t), dot3(v, n));  to_world(v) = ((s * v.x + t * v.y) + n * v.z);
 * dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z;  normalize3(v) = v / sqrt(dot3(v, v)).  rc_D, rc_G1 and rc_sample_m are the
 * renderer's microfacet functions (Mitsuba's MicrofacetDistribution::eval, smith_g1 and sample with sample_visible), a negative
 * alpha naming GGX.  fresnel(c, eta) is the renderer's fresnel_dielectric (Mitsuba's fresnel): with rcp = 1 / eta,
 *      (eta_it, eta_ti) = c >= 0 ? (eta, rcp) : (rcp, eta)
 *      ct2 = 1 - ((1 - c * c) * (eta_ti * eta_ti))          ac = |c|          ct = ct2 > 0 ? sqrt(ct2) : 0
 *      a_s = (eta_it * ct - ac) / (eta_it * ct + ac)        a_p = (eta_it * ac - ct) / (eta_it * ac + ct)
 *      F   = 0.5 * (a_s * a_s + a_p * a_p),   1 when ac == 0          cos_t = c >= 0 ? -ct : ct
 * Under total internal reflection ct = 0, a_s = -1, a_p = 1 and F = 1 exactly.
 *
 * A lane is VALID when it is active (active == NULL or active[i] != 0), every component of normal and of wi is finite,
 * PG_RESAMPLE_INTERFACE_MIN_ROUGHNESS = 1e-3f <= roughness <= 1, PG_RESAMPLE_INTERFACE_MIN_ETA = 0.25f <= eta <=
 * PG_RESAMPLE_INTERFACE_MAX_ETA = 4.0f (a NaN fails either range) and eta != 1: with eta == 1 there is no interface, the
 * renderer's rough dielectric returns nothing, and the host passes straight through.  Any other lane gets the "nothing kept"
 * outputs below and zeros in all its candidate slots, and its stream is not touched.
 *
 * The KD leaf, and with it the quadtree, are pg_sample's for p -- also for a p outside the root box or with a NaN coordinate.
 * n is the normal AS GIVEN and points to the exterior (the side of ext_ior); wi is the world direction away from the surface
 * towards the viewer AS GIVEN: unit length is the caller's business.  eta[i] is int_ior / ext_ior of the interface, the
 * renderer's MAT_ETA.  Per valid lane:
 *      fr  = make_frame(n)          wil = to_local(fr, wi)          a = -roughness      (the renderer's sign for GGX)
 *      om  = 1 - alpha              d4 = delta * INV_4PI            omd = 1 - delta
 * wil.z may have either sign: the viewer may be inside the glass.
 *
 * THE DENSITY b(wl) of a local direction wl is the pdf of the renderer's rough dielectric (rd_eval_pdf) for the row
 * {alpha = a, eta = eta[i]}, without its value.  With ci = wil.z, co = wl.z:
 *      ci == 0: b = 0
 *      reflect = ci * co > 0
 *      e   = ci > 0 ? eta[i] : 1 / eta[i]                                     the index the viewer looks INTO, relative to its own
 *      m   = normalize3(wil + wl * (reflect ? 1 : e)),  negated when m.z < 0   the half vector, in the exterior hemisphere
 *      D   = rc_D(m, a)
 *      wim = dot3(wil, m)        wom = dot3(wl, m)        F = fresnel(wim, eta[i])
 *      !(wim * ci > 0 && wom * co > 0): b = 0                                 micro- and macro-surface must agree on the sides
 *      den = wim + e * wom
 *      dwh_dwo = reflect ? 1 / (4 * wom) : ((e * e) * wom) / (den * den)
 *      wiu = ci < 0 ? -wil : wil
 *      prob = ((D * rc_G1(wiu, m, a)) * |dot3(wiu, m)|) / wiu.z
 *      prob = prob * (reflect ? F : 1 - F)
 *      b   = prob * |dwh_dwo|;  a NaN becomes 0;  then b = isfinite(b) ? b : 0
 * Under total internal reflection F = 1 and the transmitted share is 0 by this arithmetic, not by a special case.
 *
 * M = candidates, wsum = 0, nothing kept.  Then for k = 0 .. M-1, on the lane's PCG32 stream (pgsd.h):
 *
 *   1. xi = next_f32.  The candidate comes from the tree when xi > alpha (xi == alpha: the lobe).  A tree candidate: (w_k, q)
 *      are exactly pg_sample's direction and pdf, with the draws pg_sample makes (three per visited quadtree node).
 *   2. Otherwise it comes from the lobe and ALWAYS draws xi2 = next_f32, u1 = next_f32, u2 = next_f32, in that order.  It is the
 *      renderer's rd_sample(row, wil, xi2, u1, u2):
 *          ci == 0: failed
 *          m   = rc_sample_m(ci < 0 ? -wil : wil, a, u1, u2, pdf_m)          !(pdf_m != 0): failed
 *          wim = dot3(wil, m)          F = fresnel(wim, eta[i]), with its cos_t, eta_it, eta_ti
 *          p   = pdf_m * (xi2 <= F ? F : 1 - F)
 *          xi2 <= F, reflection:  o = m * (2 * wim) - wil;   om_ = dot3(o, m);   !(om_ * wim > 0): failed
 *                                 dwh_dwo = 1 / (4 * om_)
 *          otherwise, refraction: o = m * (wim * eta_ti + cos_t) - wil * eta_ti;   om_ = dot3(o, m);   den = wim + eta_it * om_
 *                                 !(om_ * wim < 0): failed;   dwh_dwo = ((eta_it * eta_it) * om_) / (den * den)
 *          p   = p * |dwh_dwo|;   a NaN p, or a NaN rc_G1(o, m, a): failed
 *      A sample that failed has the pdf 0, and so has one whose p is 0.  The candidate FAILED when the sample's pdf is 0, and
 *      ALSO when o left on the other side of the macro-surface than its branch names:
 *          !((xi2 <= F) == (wil.z * o.z > 0)): failed
 *      (the microfacet reflected it THROUGH the surface, or refracted it back: the renderer gives such a sample the weight 0
 *      through rc_G1(o, m, a); b, which tells the branches apart by the side, holds only the OTHER branch's density there, so
 *      kept as a candidate the sample would be weighted by a density it was not drawn with).  A failed candidate has
 *      w_k = (0, 0, 0), no pdf walk is made and t = s = 0 (so w = 0 in step 3).
 *      Otherwise w_k = to_world(fr, o) and q = what pg_pdf(p, w_k) returns.
 *   3. For a candidate that did not fail:
 *          wl = to_local(fr, w_k)
 *          b  = b(wl)
 *          s  = alpha * b + om * q                                     the SOURCE density of the candidate
 *          t  = b * (d4 + omd * q)                                     the TARGET: b times the defensive mixture of the tree
 *          w  = (s > 0 && t > 0 && isfinite(t / s)) ? t / s : 0
 *   4. zeta = next_f32;  wsum = wsum + w;  if (w > 0 && zeta * wsum < w) keep k, w_k, t and s.
 *
 * Every candidate consumes its draws whether or not it can be kept.  After the loop, with a candidate kept:
 *      dir_out = w_kept,   W = weight_out = (wsum / (float)M) / t_kept,   target_out = t_kept,   source_out = s_kept,
 *      index_out = k_kept,
 *      eta_out = wil.z * to_local(fr, w_kept).z > 0 ? 1 : (wil.z > 0 ? eta[i] : 1 / eta[i])
 * and with nothing kept:
 *      dir_out = (0, 0, -1),   W = 0,   target_out = 0,   source_out = 0,   index_out = PG_RESAMPLE_NONE,   eta_out = 0.
 * eta_out is 1 for a kept direction on wi's side and otherwise the relative index the path ENTERS -- eta for a viewer above,
 * 1 / eta for one below: what rd_sample hands the renderer for its running index of refraction, here of a tree candidate too.
 * rng_state[i] is the stream behind the last draw.
 *
 * With the candidate arrays (the layouts of pg_resample_args): cand_dir_out[(k * 3 + axis) * n + i] = w_k,
 * cand_target_out[k * n + i] = t and cand_source_out[k * n + i] = s of every candidate k < M, kept or not.
 *
 * WHAT b IS.  The density of EVERY candidate, lobe ones included, is evaluated by b; the sample's own pdf serves the failure
 * test only.  b is the density the lobe candidates are drawn with: F times the density of reflecting wil about a GGX visible
 * normal on wi's side, (1 - F) times the density of refracting it on the far side, and a proxy for BSDF times cosine of a
 * rough dielectric.  b integrates to LESS than 1: a sample that failed is lost, not redistributed.  With wil.z == 0 b is 0
 * everywhere and every lobe sample fails: nothing is kept, and the stream advances by the candidates' draws all the same.
 *
 * THE ESTIMATOR the host forms is f(dir_out) * W, f being the WHOLE integrand (radiance times BSDF times cosine).  For
 * delta > 0 it is unbiased for every f that vanishes where b does: the target is then positive wherever such an f is, and a
 * failed candidate has weight 0 as a candidate outside the support has.  With delta = 0 the target also vanishes where the
 * tree's density does, and the estimator is unbiased only for an f that vanishes there too.  W * t_kept = wsum / M estimates the
 * target's integral; with M = 1, W = 1 / s_kept: the one-sample mixture.
 *
 * REFUSALS (PG_ERR_INVALID; pg_last_error names the reason): a NULL context, params or args; with n > 0 a NULL p, normal, wi,
 *   roughness, eta, rng_state, rng_inc, dir_out or weight_out; candidates outside 1..64; alpha or delta outside [0, 1] or
 *   NaN; reserved != 0; n > 2^32 - 1.  A refused call launches nothing.  n = 0 does nothing.
 *
 * NOT BUILT: Beckmann lobes; anisotropy (one roughness per lane); a diffuse share beside the interface (a coated or plastic-like
 *   dielectric); a warp form (caller-supplied points in the place of the stream); the learned fraction of pgsd_fraction.h as
 *   alpha; any use by pg_render_pass; compacted lane lists (pg_compact_lanes).
 */
#ifndef PG_RESAMPLE_INTERFACE_H
#define PG_RESAMPLE_INTERFACE_H

#include "../../pg_resample.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_RESAMPLE_INTERFACE_MIN_ROUGHNESS 1e-3f   /* a lane with a smaller roughness is not valid */
#define PG_RESAMPLE_INTERFACE_MIN_ETA 0.25f         /* a lane with an eta outside [MIN_ETA, MAX_ETA], or of exactly 1, is not valid */
#define PG_RESAMPLE_INTERFACE_MAX_ETA 4.0f

typedef struct pg_resample_interface_args {
	const float *p, *normal, *wi;     /* Vector3f[n] each */
	const float *roughness, *eta;     /* Float[n] each */
	const uint8_t *active;            /* [n] or NULL */
	uint64_t *rng_state; const uint64_t *rng_inc;
	float *dir_out;                   /* Vector3f[n], required */
	float *weight_out;                /* Float[n], required: W */
	float *target_out, *source_out;   /* Float[n], each may be NULL: t and s of the kept candidate */
	uint32_t *index_out;              /* [n] or NULL: k of the kept candidate, PG_RESAMPLE_NONE if none */
	float *eta_out;                   /* Float[n] or NULL: 1, or the relative index the kept direction enters; 0 if none */
	float *cand_dir_out;              /* float[M][3][n] or NULL */
	float *cand_target_out, *cand_source_out; /* float[M][n] or NULL */
} pg_resample_interface_args;

int pg_resample_interface(pg_context *ctx, uint64_t n, const pg_resample_params *params,
                          const pg_resample_interface_args *args, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PG_RESAMPLE_INTERFACE_H */
