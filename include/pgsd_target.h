/*
 * pgsd_target.h -- a variance-aware guiding target for the SD-tree: two entry points of libpgsd.so beside the 60 of pgsd.h,
 * the three of pgsd_warp.h and the seven of pgsd_fraction.h.
 *
 * Every quadtree of pgsd.h learns a density proportional to the MEAN incident radiance: a record deposits L / p in the
 * directional leaf it lands in, and a refine turns the sums into sdTree_prev.  Rath et al., "Variance-Aware Path Guiding"
 * (SIGGRAPH 2020), show that the variance-optimal target for a noisy radiance estimate is proportional to sqrt(E[L^2]), the
 * square root of its second moment.  For an SD-tree that is two steps:
 *
 *   - the host records L^2 / p instead of L / p (it squares `radiance` and `radiance_nee_lum`, one fp32 multiply each, and
 *     calls pg_splat: no new recording kernel, and all three splat filters of pg_set_splat_filter apply unchanged);
 *   - pg_target_apply takes the square root of every directional LEAF of sdTree_current before the tree is refined.
 *
 * A leaf of area A = 4^-d (depth d, the root is 0) holds S = sum_k L_k^2 / p_k, an estimate of N * integral over the leaf of
 * E[L^2 | w].  Its mass under the new target is the integral of sqrt(E[L^2 | w]), about A * sqrt(S / (N A)) =
 * 2^-d * sqrt(S) / sqrt(N).  N is one constant per quadtree; pdfs and the split / merge threshold (root / 100) are ratios
 * inside a quadtree, so N is dropped.  Interior nodes are resolved from the leaves by pg_refine_and_swap as always (exact
 * integer sums, each rounded once), so the refine needs no change and does not know that a target was applied.
 *
 * Nothing here is in the reference; nothing of pgsd.h changes (PGSD_ABI_VERSION stays: entry points were added).  Conventions are
 * those of pgsd.h: calls are asynchronous on `stream`, the same status codes, a NULL context gives PG_ERR_INVALID.
 *
 * ---- semantics: fp32, every operation rounded on its own (no contraction), in this order ----------------------------------
 *
 * TRANSFORM of one leaf accumulator (words l0, l1, l2, count: pgsd.h) of a leaf at depth d:
 *       s = acc_to_float(l0 + l1 2^32 + l2 2^64)     the accumulator-to-fp32 conversion of a refine: one round-to-nearest-even,
 *                                                     then the exact 2^-PG_FRAC_BITS
 *       t = s > 0 ? sqrt(s) : 0                      IEEE, correctly rounded; s <= 0 (a host that fed negative weights) gives 0
 *       t = t * 2^-d                                 exact
 *       q = quantize(t)                              pgsd.h: trunc(clamp(t, +-2^PG_W_CLAMP_LOG2) * 2^PG_FRAC_BITS)
 *       word k = 0, 1 <- (q >> 32 k) mod 2^32,  word 2 <- q >> 64     (what a single record of weight t leaves in an empty
 *                                                                      accumulator)
 *       word 3, the count, keeps its value.
 *
 * WHICH accumulators are transformed:
 *   - the four child slots of a quadtree record whose child is a leaf, and the root slot of a tree whose root is a leaf;
 *   - slots of interior nodes, the fallback counters and the KD counts are not part of the transform: a refine never reads the
 *     former and the latter are counts.
 *   The children of a record on level l of the forest (root records are level 0) lie at depth l + 1; a root slot at depth 0.
 *
 * ORDER.  pg_target_apply is called ONCE per iteration: after the last record, after the multi-GPU sum (pg_allreduce, or the
 *   host's own sum over pg_accumulators / pg_exchange_pack), and before pg_refine_and_swap.  sqrt does not commute with the sum
 *   over ranks: every rank sums first and applies then, and all ranks hold the same words.  Records added, or buffers summed
 *   across ranks, between pg_target_apply and pg_refine_and_swap are the HOST'S ERROR: nothing detects it, and the refine
 *   then resolves a mixture of moments and roots.
 *
 * THE "APPLIED" FLAG lives in the context.  pg_target_apply sets it; a second pg_target_apply before the next refine returns
 *   PG_ERR_INVALID with a message and changes nothing.  It is cleared by the commit of pg_refine_and_swap, by pg_setup and by
 *   pg_import.  A refine that fails (it is a transaction, pgsd.h) leaves the transformed accumulators AND the flag in place:
 *   calling pg_refine_and_swap again gives the tree that an unfailed refine would have given.
 *
 * NOT BUILT.  The library's own renderer (pg_render_pass) and pg_process_and_splat record first moments, as before.  A host on the
 *   dense layout calls pg_process_records, squares `radiance` and `radiance_nee_lum`, and calls pg_splat.
 *
 * A context that never calls pg_target_apply allocates and launches exactly what it did before.
 */
#ifndef PGSD_TARGET_H
#define PGSD_TARGET_H

#include "pgsd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_TARGET_SECOND_MOMENT 1

/* Transforms the accumulators of sdTree_current in place (see above), asynchronously on `stream`.  target:
 * PG_TARGET_SECOND_MOMENT; any other value is PG_ERR_INVALID.  No allocation, one kernel launch. */
int pg_target_apply(pg_context *ctx, int32_t target, void *stream);

/* *out = the target applied since the last refine / setup / import (PG_TARGET_SECOND_MOMENT), or 0. */
int pg_target_applied(pg_context *ctx, int32_t *out);

#ifdef __cplusplus
}
#endif

#endif /* PGSD_TARGET_H */
