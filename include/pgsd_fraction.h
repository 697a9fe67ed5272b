/*
 * pgsd_fraction.h -- the BSDF sampling fraction, learned per spatial leaf: seven entry points of libpgsd.so beside the 60 of
 * pgsd.h and the three of pgsd_warp.h.
 *
 * The mixture between BSDF sampling and SD-tree sampling is one constant of pg_setup (bsdf_sampling_fraction).  "Path Guiding
 * in Production" (SIGGRAPH 2019 course, ch. 10) learns it per spatial leaf instead: fraction = logistic(theta), theta moved by
 * Adam along the gradient of the KL divergence (or of the variance) of the mixture.  The published optimiser takes one Adam
 * step per record under a spinlock, so its result depends on the order of the records.  This library's form does not:
 *
 *   - a record's gradient is evaluated at the theta that is in force while the records are taken (a step changes it, a record
 *     does not);
 *   - gradients are summed per leaf in the fixed-point accumulators of pgsd.h (exact integer sums);
 *   - ONE Adam step per leaf is taken when the host calls pg_fraction_step.
 *
 * The same records in any order, in any number of launches, on any number of ranks give the same parameters bit for bit.
 * Nothing here is in the reference; nothing of pgsd.h changes (PGSD_ABI_VERSION stays: entry points were added).  The library's
 * own renderer (pg_render_pass) does not use the learned fraction: it is for hosts that drive pg_guide_bounce themselves.
 *
 * Conventions are those of pgsd.h: device pointers unless named h_*, planar layout, byte masks with NULL = all active, calls
 * are asynchronous on `stream`, the same status codes; a NULL context or a NULL required pointer (with n > 0) gives
 * PG_ERR_INVALID.  A "leaf" is a KD leaf; its number is its quadtree's (KdNode::tree: what pg_export writes in
 * kd_quad_root_index), and there are n_roots (pg_export_sizes) of them.
 *
 * pg_setup and pg_import leave the feature DISABLED (and free its state).  A context that never enables it behaves, allocates
 * and times exactly as before.  Every pg_fraction_* call but pg_fraction_enable fails with PG_ERR_INVALID on a disabled context.
 *
 * ---- state per leaf ---------------------------------------------------------------------------------------------------------
 *
 *   theta  = theta0    the parameter                 p1    = 1   running product of beta1
 *   m      = 0         Adam's first moment           p2    = 1   running product of beta2
 *   v      = 0         Adam's second moment          steps = 0   steps taken
 *   acc    = 0         PG_ACC_WORDS int64 words: the three limbs of the gradient sum and the number of kept records
 *
 * ---- semantics: fp32, every operation rounded on its own (no contraction), in this order ----------------------------------
 *
 * exp_f32 is the library's own exponential (pgsd.h: pg_math_eval 0; oracle/pgo_math.h), / and sqrt are IEEE.
 *
 * logistic(theta):   e = exp_f32(0 - theta);   f = 1 / (1 + e)
 *
 * QUERY, pg_fraction_query, per lane:
 *   the KD leaf of p is found exactly as pg_sample finds it;  fraction_out = logistic(theta of that leaf).
 *   Inactive lanes, lanes whose position lies outside the root box (the inclusive test of the record boundary:
 *   bmin <= p <= bmax on every axis) and lanes with a NaN coordinate return logistic(theta0).
 *
 * RECORD, pg_fraction_record, per record i < (d_count ? *d_count : m)   (planes keep stride m, as in pg_splat):
 *   guide_pdf is what pg_pdf / pg_guide_bounce returned for the sampled direction, product the host's luminance of BSDF value
 *   x cosine x incident radiance estimate, wo_pdf the mixture density the direction was drawn with.
 *   The record is KEPT when all of these hold:
 *     - is_delta is NULL or is_delta[i] == 0;
 *     - its position lies inside the root box (inclusive; a NaN coordinate fails);
 *     - bsdf_pdf, guide_pdf, product and wo_pdf are finite;
 *     - wo_pdf > 0;
 *     - mix > 0, with  f = logistic(theta of the record's leaf, as it stands)  and
 *         mix = (f * bsdf_pdf) + ((1 - f) * guide_pdf).
 *   For a kept record:
 *       r = product / mix;                 loss == PG_FRACTION_LOSS_VARIANCE:  r = r * r
 *       dLdf = ((0 - r) / wo_pdf) * (bsdf_pdf - guide_pdf)
 *       g = dLdf * (f * (1 - f))
 *   and the leaf's accumulator receives quantize(g), the contract of pgsd.h: q = trunc(clamp(g, +-2^PG_W_CLAMP_LOG2) *
 *   2^PG_FRAC_BITS), NaN -> 0.  Word k = 0, 1, 2 of the accumulator grows by sign(q) * ((|q| >> 32 k) mod 2^32) (word 2 by
 *   sign(q) * (|q| >> 64)), word 3 by 1.  A kept record whose q is 0 still counts.  A dropped record changes nothing.
 *   The words are sums of integers: the order of the records, their distribution over launches and the way the kernel merges
 *   them cannot change a bit.  At most 2^31 kept records per leaf between two steps (the bound the limbs rely on, pgsd.h).
 *
 * STEP, pg_fraction_step, for every leaf whose word 3 (count) is > 0:
 *       g = acc_to_float(word0 + word1 2^32 + word2 2^64) / (float)count      (the accumulator-to-fp32 conversion of a refine:
 *                                                                              one round-to-nearest-even, then the exact 2^-40)
 *       g = g + l2 * theta
 *       m = beta1 * m + (1 - beta1) * g
 *       v = beta2 * v + (1 - beta2) * (g * g)
 *       p1 = p1 * beta1;   p2 = p2 * beta2;   steps = steps + 1
 *       a = learning_rate * (sqrt(1 - p2) / (1 - p1))
 *       theta = theta - a * (m / (sqrt(v) + epsilon))
 *       theta = theta < -20 ? -20 : (theta > 20 ? 20 : theta)
 *   then the leaf's four words are zeroed.  Leaves with count 0 keep everything.  There is no pow: p1 and p2 stand in for
 *   beta^t.
 *
 * MULTI-GPU: pg_fraction_accumulators returns the accumulators of all leaves as one contiguous int64 buffer
 *   (n_roots * PG_ACC_WORDS words, leaf-major).  Ranks that took different records sum their buffers element-wise (int64)
 *   before the step; every rank that then steps holds the same parameters.
 *
 * REFINE: pg_refine_and_swap carries the state.  A KD leaf that splits hands theta, m, v, p1, p2 and steps to both children;
 *   leaves that do not split keep theirs.  The accumulators of the refined tree are ZERO: gradients that were recorded and not
 *   stepped are dropped, so step before refining.  The refine stays a transaction: a failed refine leaves the fraction state
 *   exactly as it was.
 *
 * Defaults.  The Python surface offers learning_rate 0.01, beta1 0.9, beta2 0.999, epsilon 1e-8, l2 0.01 and the KL loss: the
 *   publication's values, which it chose for one step PER RECORD.  A batch step happens far less often; which learning rate
 *   suits it is a number nobody has measured, and it is not tuned here.
 */
#ifndef PGSD_FRACTION_H
#define PGSD_FRACTION_H

#include "pgsd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PG_FRACTION_LOSS_KL 0
#define PG_FRACTION_LOSS_VARIANCE 1
#define PG_FRACTION_THETA_MAX 20.0f

typedef struct pg_fraction_params {
	float theta0;        /* initial parameter of every leaf; finite, |theta0| <= 20 (fraction = logistic(theta0); 0 -> 0.5) */
	float learning_rate; /* > 0, finite */
	float beta1, beta2;  /* in [0, 1) */
	float epsilon;       /* > 0 */
	float l2;            /* >= 0: regularisation weight on theta */
	int32_t loss;        /* PG_FRACTION_LOSS_KL | PG_FRACTION_LOSS_VARIANCE */
} pg_fraction_params;

typedef struct pg_fraction_records { /* planar, stride m */
	const float *position;  /* Vector3f[m] */
	const float *bsdf_pdf;  /* Float[m] */
	const float *guide_pdf; /* Float[m] */
	const float *product;   /* Float[m] */
	const float *wo_pdf;    /* Float[m] */
	const uint8_t *is_delta; /* [m], may be NULL (no record is delta) */
} pg_fraction_records;

/* Enables the feature on a configured context (after pg_setup / pg_import) with every leaf at its start values; on an enabled
 * context it resets the state to them.  NULL params: disable and free the state.  Synchronises the device. */
int pg_fraction_enable(pg_context *ctx, const pg_fraction_params *params);

int pg_fraction_query(pg_context *ctx, uint64_t n, const float *p, const uint8_t *active, float *fraction_out, void *stream);

/* d_count: as in pg_splat (device uint32, may be NULL = all m records).  At most 2^32 - 1 records per call. */
int pg_fraction_record(pg_context *ctx, uint64_t m, const pg_fraction_records *rec, const uint32_t *d_count, void *stream);

int pg_fraction_step(pg_context *ctx, void *stream);

/* The library-owned accumulator buffer (valid until the next refine, enable, setup or import) and its length in words. */
int pg_fraction_accumulators(pg_context *ctx, int64_t **d_buffer, uint64_t *count);

/* Checkpoint: host arrays indexed by leaf; n_trees must equal pg_export_sizes' n_roots.  h_acc (int64[n_trees * PG_ACC_WORDS])
 * may be NULL.  Both synchronise the device.  Import zeroes the accumulators and refuses a non-finite value or |theta| > 20. */
int pg_fraction_export(pg_context *ctx, uint64_t n_trees, float *h_theta, float *h_m, float *h_v, float *h_p1, float *h_p2,
                       uint32_t *h_steps, int64_t *h_acc);
int pg_fraction_import(pg_context *ctx, uint64_t n_trees, const float *h_theta, const float *h_m, const float *h_v,
                       const float *h_p1, const float *h_p2, const uint32_t *h_steps);

#ifdef __cplusplus
}
#endif

#endif /* PGSD_FRACTION_H */
