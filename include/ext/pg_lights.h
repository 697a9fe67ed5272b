/*
 * pg_lights.h -- light selection for next-event estimation, learned per spatial leaf: nine entry points of libpgsd.so beside
 * those of pgsd*.h and pg_resample.h.
 *
 * The library answers, at a path vertex, which direction to continue in, how to mix BSDF and tree sampling, how much radiance
 * arrives and whether the path lives.  This header adds which light to sample.  The reference picks an emitter uniformly; in a
 * scene with many lights most of them contribute nothing at a given place, and the place is what the SD-tree's KD tree
 * partitions.  So every KD leaf learns a table over the host's lights: the host records what a light's samples contributed
 * there, a build turns the means into integer weights, and a sample draws a light in proportion to them, mixed with the uniform
 * choice so that no light's probability is ever zero.  A "light" is an index 0 .. n_lights - 1 the host assigns; the library
 * knows nothing else about it.  Nothing here is in the reference; nothing of pgsd.h changes (PGSD_ABI_VERSION stays).
 *
 * Conventions are those of pgsd.h: device pointers unless named h_*, planar layout, byte masks with NULL = all active, calls
 * are asynchronous on `stream`, the same status codes; a NULL context or a NULL required pointer (with n > 0) gives
 * PG_ERR_INVALID.  A "leaf" is a KD leaf; its number is its quadtree's (what pg_export writes in kd_quad_root_index), and
 * there are n_roots (pg_export_sizes) of them.
 *
 * pg_setup and pg_import leave the feature DISABLED (and free its state).  A context that never enables it behaves, allocates
 * and times exactly as before.  Every pg_lights_* call but pg_lights_enable and pg_lights_status fails with PG_ERR_INVALID on a
 * disabled context.
 *
 * ---- state per leaf, L = n_lights ---------------------------------------------------------------------------------------------
 *
 *   acc[j]   PG_ACC_WORDS int64 words per light j, the contract of pgsd.h: the three limbs of the sum of quantize(value) and,
 *            in word 3, the number of kept records
 *   C[j]     uint32, the row: inclusive prefix sums of integer weights k_j in [0, 65536] (k_0 = C[0], k_j = C[j] - C[j-1]);
 *            K = C[L-1].  K == 0: the leaf has learned nothing yet and selects uniformly.  A fresh leaf has K = 0.
 *
 * Everything that depends on an order is an integer sum or a maximum: the same records give the same rows bit for bit, in any
 * order, over any number of launches or ranks.
 *
 * ---- semantics: fp32, every operation rounded on its own (no contraction), in this order --------------------------------------
 *
 * (uint32)x truncates toward zero (x is never negative or out of range where it is written).  invL = 1 / (float)L.
 *
 * RECORD, pg_lights_record, per record i < (d_count ? min(*d_count, m) : m)   (planes keep stride m, as in pg_splat):
 *   value is the host's estimate of the light's contribution at the position BEFORE the division by the selection
 *   probability: luminance of BSDF value x emitted radiance x geometry term x visibility, over the pdf of the point on that
 *   light.  A host that wants the variance-aware target records the square of it and enables with root = 1.
 *   The record is KEPT when all of these hold:
 *     - its position lies inside the root box (inclusive: bmin <= p <= bmax on every axis; a NaN coordinate fails);
 *     - light[i] < L;
 *     - value[i] is finite and >= 0.
 *   The accumulator of (leaf of the position, light[i]) receives quantize(value[i]), the contract of pgsd.h
 *   (q = trunc(min(value, 2^PG_W_CLAMP_LOG2) * 2^PG_FRAC_BITS)): word k = 0, 1, 2 grows by (q >> 32 k) mod 2^32 (word 2 by
 *   q >> 64), word 3 by 1.  A kept record whose value is 0 still counts: an occluded sample is information.  A dropped record
 *   changes nothing.  At most 2^31 kept records per (leaf, light), over all ranks (the bound the limbs rely on, pgsd.h).
 *
 * BUILD, pg_lights_build, per leaf:
 *       count_j = word 3 of acc[j];    T_j = word0 + word1 2^32 + word2 2^64
 *       m_j = count_j > 0 ? acc_to_float(T_j) / (float)count_j : 0      (acc_to_float: the accumulator-to-fp32 conversion of a
 *                                                                        refine, one round-to-nearest-even, then the exact 2^-40)
 *       root != 0:  m_j = sqrt(m_j)                                      (IEEE)
 *       m_j = (m_j is finite and m_j > 0) ? m_j : 0
 *       M = max_j m_j
 *       !(M > 0): the leaf keeps its row.  Otherwise
 *       k_j = (uint32)((m_j / M) * 65536.0f);     C[j] = k_0 + ... + k_j
 *   The accumulators are left as they are: a host may record, build, record more and build again, and every build sees all
 *   records since the feature was enabled (or the state imported, or the tree refined).  The light of the maximum has
 *   k_j = 65536, so a built row has K >= 65536.
 *
 * SELECT(leaf, u) -> j, the map pg_lights_sample applies:
 *       u = (0 <= u && u < 1) ? u : 0                                    (NaN, negative, >= 1 and infinite become 0; -0 stays)
 *   an unlearned leaf (K == 0):
 *       j = min((uint32)(u * (float)L), L - 1)
 *   a learned leaf, u < delta  (the uniform branch):
 *       j = min((uint32)((u / delta) * (float)L), L - 1)
 *   a learned leaf otherwise  (the tree branch):
 *       v = (u - delta) / (1 - delta)
 *       t = min((uint32)(v * 16777216.0f), 16777215)
 *       x = ((uint64)t * K) >> 24
 *       j = the smallest index with C[j] > x                             (x < K: it exists, and k_j > 0)
 *
 * PMF(leaf, j), what pg_lights_sample returns beside j and pg_lights_pmf returns for a given light:
 *       j >= L:            0
 *       an unlearned leaf: invL
 *       a learned leaf:    (delta * invL) + ((1 - delta) * ((float)k_j / (float)K))
 *
 * SAMPLE, pg_lights_sample, per lane:
 *   u is u[i]; when the array `u` is NULL, u is one next_f32 of the lane's PCG32 stream (rng_state / rng_inc as in pg_sample,
 *   both required then), drawn by every active lane before anything else, and the advanced state is written back.  With `u`
 *   given the streams are not touched and may be NULL.
 *   The leaf is found as pg_fraction_query finds it; a position outside the root box or with a NaN coordinate behaves as an
 *   unlearned leaf.  light_out = SELECT(leaf, u), pmf_out = PMF(leaf, light_out).
 *   Inactive lanes get light_out = PG_LIGHTS_NONE and pmf_out = 0, and their stream is untouched.
 *
 * PMF, pg_lights_pmf, per lane: pmf_out = PMF(leaf of p, light[i]), for MIS when a BSDF sample hits an emitter; positions
 *   outside the box as above; inactive lanes get 0.
 *
 * With delta > 0 every light of every leaf has pmf >= delta / L > 0, so value / pmf is an unbiased selection however poor
 * the row; delta = 0 trusts the row and never selects a light with k_j = 0 from a learned leaf.  The share of u in [0, 1)
 * that SELECT maps to light j equals PMF(leaf, j) up to the map's roundings: within 6 * 2^-24 (tests/test_lights_model.py
 * walks all 2^24 values of i / 2^24).
 *
 * MULTI-GPU: pg_lights_accumulators returns the accumulators of all leaves as one contiguous int64 buffer
 *   (n_roots * L * PG_ACC_WORDS words, leaf-major, then light).  Ranks that took different records sum their buffers
 *   element-wise (int64) before the build; every rank that then builds holds the same rows.
 *
 * REFINE: pg_refine_and_swap carries the state.  A KD leaf that splits hands its row to both children; leaves that do not
 *   split keep theirs.  The accumulators of the refined tree are ZERO.  The refine stays a transaction: a failed refine leaves
 *   the state exactly as it was.  A refine that would take n_roots * L above 2^31 fails with PG_ERR_NOMEM.
 *
 * NOT BUILT.  None of these exists:
 *   - any use by pg_render_pass: the library's own renderer picks its emitter uniformly, as the reference does;
 *   - a remapped u for reuse (the part of u left over after the selection, rescaled to [0, 1));
 *   - light hierarchies (a tree over the lights; the row is flat, which is what bounds n_lights);
 *   - compacted lane lists (the lane_index / d_lane_count of pg_guide_bounce);
 *   - the npz schema: SDTree.save / load do not store the rows; lightsState / lightsLoadState are the checkpoint.
 */
#ifndef PG_LIGHTS_H
#define PG_LIGHTS_H

#include "../pgsd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_LIGHTS_MAX 4096
#define PG_LIGHTS_WEIGHT_ONE 65536
#define PG_LIGHTS_NONE 0xFFFFFFFFu

typedef struct pg_lights_params {
	float delta;       /* share of the uniform choice on a learned leaf; in [0, 1], not NaN */
	uint32_t root;     /* 0: the weights follow the means; 1: their square roots */
	uint32_t reserved; /* 0 */
} pg_lights_params;

typedef struct pg_lights_records { /* planar, stride m */
	const float *position; /* Vector3f[m] */
	const uint32_t *light; /* [m] */
	const float *value;    /* Float[m] */
} pg_lights_records;

/* Enables the feature on a configured context (after pg_setup / pg_import) for n_lights in 1 .. PG_LIGHTS_MAX, every leaf
 * unlearned with zero accumulators; on an enabled context it resets the state to that.  Refuses when n_roots * n_lights exceeds
 * 2^31.  n_lights = 0: disable and free the state (params may be NULL).  Synchronises the device. */
int pg_lights_enable(pg_context *ctx, uint32_t n_lights, const pg_lights_params *params);

/* d_count: as in pg_splat (device uint32, may be NULL = all m records).  At most 2^32 - 1 records per call. */
int pg_lights_record(pg_context *ctx, uint64_t m, const pg_lights_records *rec, const uint32_t *d_count, void *stream);

int pg_lights_build(pg_context *ctx, void *stream);

/* u: Float[n] or NULL (then rng_state / rng_inc, uint64[n] each, are required); light_out: uint32[n]; pmf_out: Float[n]. */
int pg_lights_sample(pg_context *ctx, uint64_t n, const float *p, const float *u, uint64_t *rng_state, const uint64_t *rng_inc,
                     const uint8_t *active, uint32_t *light_out, float *pmf_out, void *stream);

int pg_lights_pmf(pg_context *ctx, uint64_t n, const float *p, const uint32_t *light, const uint8_t *active, float *pmf_out,
                  void *stream);

/* The library-owned accumulator buffer (valid until the next refine, enable, setup or import) and its length in words. */
int pg_lights_accumulators(pg_context *ctx, int64_t **d_buffer, uint64_t *count);

/* n_lights: 0 on a disabled context (and then *n_learned_leaves = 0); n_learned_leaves: leaves with K > 0.  Either pointer may
 * be NULL.  Synchronises the device. */
int pg_lights_status(pg_context *ctx, uint32_t *n_lights, uint64_t *n_learned_leaves);

/* Checkpoint: host arrays, leaf-major then light; n_trees must equal pg_export_sizes' n_roots and n_lights the enabled count.
 * h_rows: uint32[n_trees * n_lights]; h_acc (int64[n_trees * n_lights * PG_ACC_WORDS]) may be NULL.  Both synchronise the
 * device.  Import zeroes the accumulators and refuses a row that does not ascend (C[j] < C[j-1]) or one of whose steps (C[0],
 * C[j] - C[j-1]) exceeds 65536. */
int pg_lights_export(pg_context *ctx, uint64_t n_trees, uint32_t n_lights, uint32_t *h_rows, int64_t *h_acc);
int pg_lights_import(pg_context *ctx, uint64_t n_trees, uint32_t n_lights, const uint32_t *h_rows);

#ifdef __cplusplus
}
#endif

#endif /* PG_LIGHTS_H */
