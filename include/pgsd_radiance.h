/*
 * pgsd_radiance.h -- radiance estimates from the SD-tree and guided Russian roulette / splitting: six entry points of libpgsd.so
 * beside the 60 of pgsd.h, the three of pgsd_warp.h, the seven of pgsd_fraction.h and the two of pgsd_target.h.
 *
 * pgsd.h answers two questions about sdTree_prev: "give me a direction" (pg_sample) and "what is its pdf" (pg_pdf).  This header
 * answers the third: HOW MUCH RADIANCE ARRIVES AT p FROM DIRECTION w?  That number is what adjoint-driven Russian roulette and
 * splitting needs (Vorba and Krivanek, "Adjoint-Driven Russian Roulette and Splitting in Light Transport Simulation", SIGGRAPH
 * 2016), what Rath et al. pair their variance-aware target with, and what a host needs to use the tree as a radiance cache or to
 * look at what the tree learned.
 *
 * A directional leaf of area 4^-d (depth d, the root is 0) of the quadtree of a KD leaf holds S = sum_k L_k / p_k over the N
 * records the KD leaf's quadtree received; the directions of the records are distributed with density p, so S / N estimates the
 * integral of L over the leaf's solid angle, 4 pi 4^-d, and
 *
 *       L(p, w) ~ S 4^d / (4 pi N).
 *
 * N CANNOT BE RECOVERED FROM AN EXPORTED TREE.  A KD leaf that splits hands each child a copy of its quadtree with the full
 * energy, and halves vertCount per split; how often a leaf was split since its energies were resolved is stored nowhere (and
 * vertCount is an fp32 that stops counting at 2^24).  The library therefore keeps N, the STATISTICAL WEIGHT of every quadtree, and
 * carries it through pg_refine_and_swap inside the refine's transaction.
 *
 * Nothing here is in the reference; nothing of pgsd.h changes (PGSD_ABI_VERSION stays: entry points were added).  Conventions are
 * those of pgsd.h: planar arrays in device memory, calls asynchronous on `stream`, the same status codes, a NULL context gives
 * PG_ERR_INVALID.  A context that never calls pg_radiance_enable allocates and launches exactly what it did before.
 *
 * ---- state ----------------------------------------------------------------------------------------------------------------
 *
 * One uint64 per quadtree of sdTree_prev (numbered as pg_export writes them in kd_quad_root_index):
 *       weight[t] = the number of in-box records that the accumulators which were resolved into tree t had received -- the
 *                   exact integer a refine computes for the KD count of the leaf: word 3 (pgsd.h) summed over the tree's
 *                   accumulators, plus the tree's fallback counter.
 * and three flags: `enabled`; `valid` (the table describes sdTree_prev); `of_target` (the energies of sdTree_prev were resolved
 * from accumulators that pg_target_apply had transformed: the value of pg_target_applied at that refine, PG_TARGET_SECOND_MOMENT).
 *
 *   pg_radiance_enable(on != 0)  on a configured context (after pg_setup / pg_import): allocates the table; valid = 0, of_target
 *                                = 0: the weights of the present sdTree_prev are unknown.  On a context that has the feature on
 *                                already it changes nothing.
 *   pg_radiance_enable(0)        frees the table; all three flags 0.
 *   pg_setup, pg_import          leave the feature OFF, as they do the learned fraction.
 *   pg_refine_and_swap           with the feature on, the new table is built beside the new tree: weight_new[t] = the count
 *                                resolved for the old tree that new tree t is a copy or refinement of.  It is committed together
 *                                with the tree: valid = 1, of_target = pg_target_applied as it stood before the commit cleared it.
 *                                A refine that fails leaves the table and the three flags exactly as they were (pgsd.h: a refine
 *                                is a transaction).  The weights come from the summed accumulators, so all ranks of a multi-GPU
 *                                run (pg_allreduce before the refine) hold the same table.
 *   pg_radiance_import           the checkpoint path for a tree loaded from a file (pg_import, then pg_radiance_enable, then this):
 *                                n_trees must equal pg_export_sizes' n_roots.  valid = 1, of_target = 0: the host vouches for
 *                                the values.
 *   pg_radiance_export           refuses while valid = 0 (PG_ERR_INVALID).  Both synchronise the device.
 *
 * ---- semantics: fp32, every operation rounded on its own (no contraction), in this order ----------------------------------
 *
 * ESTIMATE of one active lane (position p, direction dir):
 *       KD leaf:  the node pg_pdf finds for p -- KDTree.getLeafNodeIndex; a position outside the root box (inclusive test) or NaN
 *                 gets the root node and ITS quadtree.   t = the node's quadtree,  N = weight[t],
 *                 Nf = (float)N                       uint64 -> fp32, round to nearest even (NOT vertCount's conversion, which
 *                                                      stops at 2^24)
 *       (cx, cy) = dirToCanonical(dir)                 pgsd.h; a non-finite direction gives (0, 0)
 *       leaf:     the leaf that the DESCENT of pdfQuadTree / addIrradiancePropagate reaches, i.e. the leaf that a record with
 *                 this direction adds to.  From the root cell [0, 1]^2, level by level: with (mx, my) the cell's centre, child 0
 *                 is x >= mx and y >= my, child 1 x <= mx and y >= my, child 2 x <= mx and y <= my, child 3 x >= mx and y <= my;
 *                 the walk enters the HIGHEST-numbered child whose test holds (edges included: a direction on a cell edge or
 *                 corner belongs to several).  pg_pdf multiplies the energies of the LOWEST-numbered one; the two differ on the
 *                 edges only.  (Should no test hold -- it cannot for the output of dirToCanonical -- the walk ends at the node
 *                 it stands on.)
 *       e = that leaf's quad_irradiance,  d = its depth (root = 0; a root that is a leaf: e = the root's energy, d = 0)
 *       L_dir  = N == 0 ? 0 : ((e * 4^d) * INV_FOUR_PI) / Nf          4^d exact;  INV_FOUR_PI = 0.07957747154594766788f
 *       L_mean = N == 0 ? 0 : (root_energy * INV_FOUR_PI) / Nf        the mean over the sphere of the radiance arriving in
 *                                                                      the KD leaf
 *   Inactive lanes: L_dir = L_mean = 0.
 *   N == 0 can coexist with e > 0: records outside the root box add their energy to tree 0 without being counted.
 *   With store_nee (pg_setup) the energies hold BOTH deposits of a record -- the path direction's and the emitter sample's -- so
 *   the estimate is of the total incident radiance, direct light included, while N counts records, not deposits.
 *
 * DECISION of one active lane (pg_radiance_rr), with s = params->window, computed once on the host in fp32:
 *       lo = 2 / (1 + s),   hi = s * lo                               the window [lo, hi] around 1, of ratio s
 *   and per lane, in this order:
 *       xi = next_f32 of the lane's PCG32 stream                      pgsd.h; exactly ONE draw per active lane, whatever follows
 *       L = L_dir as above,  w = weight[i],  I = reference[i]
 *       if !(L > 0) or !(w > 0) or !(I > 0), or one of them is not finite:        count = 1, scale = 1     (no opinion)
 *       q = (w * L) / I;  if q is not finite:                                      count = 1, scale = 1
 *       else if q < lo:  P = q / lo;  survive = xi < P;  count = survive ? 1 : 0;  scale = survive ? lo / q : 0      (roulette)
 *       else if q > hi and max_split > 1:                                                                            (split)
 *                        r = q / hi;  if r > (float)max_split: r = (float)max_split
 *                        k = floor(r);  count = (uint32)k + (xi < r - k ? 1 : 0);  scale = 1 / r
 *       else:                                                                      count = 1, scale = 1
 *   Inactive lanes: count = 1, scale = 1, L_dir = 0, the stream is not touched.
 *   `weight` is the host's throughput (a luminance) behind the bounce, `reference` its estimate of the pixel's value: q is the
 *   path's expected contribution relative to it.  The host continues the path `count` times (0: it ends) with its throughput
 *   multiplied by `scale`.  Both branches are unbiased by construction: E[count * scale] = 1.
 *
 * REFUSALS of pg_radiance_query and pg_radiance_rr (PG_ERR_INVALID, pg_last_error names the reason): the feature is off; valid = 0;
 *   of_target != 0 (sdTree_prev then holds roots of second moments, not radiance); a NULL required pointer; for pg_radiance_rr a
 *   window that is not finite or < 1, or a max_split outside 1 .. 65536.  n = 0 does nothing.
 *
 * ELSEWHERE: pgsd_bounce.h declares pg_bounce, the pg_guide_bounce variant that also returns the estimate of the continuation
 *   direction (behind the same KD descent, with the list of pg_compact_lanes).
 * NOT BUILT: compacted lane lists for the two query calls of this header; any use by the library's own renderer (pg_render_pass
 *   keeps its throughput-based roulette); estimates from a second-moment tree; and the npz schema of the tree files does not
 *   change -- a host that saves a tree saves pg_radiance_export's array beside it.
 */
#ifndef PGSD_RADIANCE_H
#define PGSD_RADIANCE_H

#include "pgsd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: switch the feature on (see above); 0: off, the table is freed.  Synchronises the device. */
int pg_radiance_enable(pg_context *ctx, int32_t on);

/* The three flags; each pointer may be NULL. */
int pg_radiance_status(pg_context *ctx, int32_t *enabled, int32_t *valid, int32_t *of_target);

/* The weights to / from host memory, n_trees = pg_export_sizes' n_roots entries. */
int pg_radiance_export(pg_context *ctx, uint64_t n_trees, uint64_t *h_weight);
int pg_radiance_import(pg_context *ctx, uint64_t n_trees, const uint64_t *h_weight);

/* p: float[3][n]; dir: float[3][n]; active: uint8[n] or NULL; L_dir_out, L_mean_out: float[n].
 * dir and L_dir_out may be NULL TOGETHER: only the mean is computed then and no quadtree is walked.  L_mean_out may be NULL when
 * dir is given.  One kernel launch, no allocation. */
int pg_radiance_query(pg_context *ctx, uint64_t n, const float *p, const float *dir, const uint8_t *active,
                      float *L_dir_out, float *L_mean_out, void *stream);

typedef struct pg_rr_params {
	float window;       /* s: finite, >= 1 (Vorba and Krivanek use 5) */
	uint32_t max_split; /* 1 .. 65536; 1 = Russian roulette only */
} pg_rr_params;

/* p, dir: float[3][n]; weight, reference: float[n]; rng_state, rng_inc: the lanes' PCG32 streams (pg_rng_seed); active: uint8[n]
 * or NULL; count_out: uint32[n]; scale_out: float[n]; L_dir_out: float[n] or NULL.  One kernel launch, no allocation. */
int pg_radiance_rr(pg_context *ctx, uint64_t n, const float *p, const float *dir, const float *weight,
                   const float *reference, const pg_rr_params *params, uint64_t *rng_state, const uint64_t *rng_inc,
                   const uint8_t *active, uint32_t *count_out, float *scale_out, float *L_dir_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PGSD_RADIANCE_H */
