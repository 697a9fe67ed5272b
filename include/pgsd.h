/*
 * pgsd.h -- C ABI of libpgsd.so, the MI355X-native SD-tree ("spatial-directional tree")
 * path-guiding library.  This is the drop-in boundary for the hot path of
 * takkasila/practical_path_guiding_lab: everything the reference's Python integrator does
 * with its two KDTree objects (src/path_guiding_integrator.py -> src/kdtree.py ->
 * src/quadtree.py) is reachable through these entry points.  Citations below are
 * file:line in that repository.
 *
 * Conventions
 *  - Plain C, no exceptions cross the boundary.  Every call returns PG_OK (0) or a negative
 *    pg_status; pg_last_error() returns a human-readable message for the last failure.
 *  - All bulk pointers are DEVICE pointers owned by the caller unless a parameter is named
 *    `h_*` (host).  The library owns the trees.  `stream` is a hipStream_t (NULL = default
 *    stream); calls are asynchronous on it unless stated otherwise.
 *  - Vector arrays are planar SoA: a Vector3f[n] is 3*n floats, plane-major
 *    (x[0..n) y[0..n) z[0..n)); a Vector2f[n] likewise with 2 planes.  This is how Dr.Jit
 *    stores mi.Vector3f and gives coalesced per-lane loads.
 *  - Masks are one byte per lane (0 = inactive); a NULL mask means "all active".
 *  - Arithmetic contract: DESIGN.md section 4 (fp32, no contraction; fixed-point accumulation).
 */
#ifndef PGSD_H
#define PGSD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 3): pg_pass_params gained `slot`, pg_kernel_timing gained shade_a_ms / shade_b_ms / sort_ms, pg_scene_desc's
 * BVH is limited to 2^25 nodes; new entry points pg_film_stripes, pg_render_overlap, pg_render_sort, pg_render_stages.
 * A caller compiled against version 2 must be rebuilt (the two structs changed size): check pg_abi_version(). */
/* 4 (round 4): pg_depth_counters gained layout_bytes, pg_stats gained bytes_jump_tables / jump_bits / kd_grid_bits,
 * pg_pass_params.reserved2 became `batched` (same size); new entry points pg_film_batched, pg_film_batched_accumulate. */
/* 5 (round 5): new entry points pg_comm_info, pg_exchange_pack, pg_exchange_unpack, pg_exchange_pack_words,
 * pg_exchange_unpack_words; pg_allreduce moves the accumulators in the 24-byte exchange format (same sums).  No struct changed. */
/* 6 (round 6): pg_refine_and_swap is a transaction (on any error both trees are exactly what they were; the context stays usable);
 * new entry points pg_debug_fail_alloc, pg_debug_fail_alloc_pending (fault injection for the tests), pg_read_shade_phases (probe
 * builds); pg_enable_depth_counters takes mode 2.  No struct changed. */
/* (still 6): new entry point pg_set_splat_filter (the training filters of pg_splat / pg_process_and_splat); an added entry
 * point breaks no caller and no struct changed, so the number stays. */
/* (still 6): new entry points pg_render_record_geometry, pg_render_export_records (the filters in recording render passes, the
 * renderer's path vertices as records); no struct changed. */
#define PGSD_ABI_VERSION 6

typedef struct pg_context pg_context;

typedef enum pg_status {
	PG_OK = 0,
	PG_ERR_INVALID = -1,    /* bad argument / state                                   */
	PG_ERR_HIP = -2,        /* a HIP runtime call failed (message has the HIP error)   */
	PG_ERR_NOMEM = -3,      /* allocation failed                                       */
	PG_ERR_FORMAT = -4,     /* imported tree violates the layout the kernels rely on   */
	PG_ERR_NO_DEVICE = -5   /* no usable gfx950 device                                 */
} pg_status;

/* Fixed-point accumulation contract: weights are truncated to multiples of
 * 2^-PG_FRAC_BITS after clamping |w| to 2^PG_W_CLAMP_LOG2; each accumulator is three signed
 * 64-bit limbs of 32 payload bits (value = l0 + l1*2^32 + l2*2^64). */
#define PG_FRAC_BITS 40
#define PG_W_CLAMP_LOG2 48
#define PG_ACC_LIMBS 3
/* An accumulator occupies PG_ACC_WORDS int64 in one 32-byte sector: the three limbs and a record
 * counter (records inside the KD bbox whose path direction ended in this quadtree leaf). */
#define PG_ACC_WORDS 4

/* ---- lifetime ------------------------------------------------------------------------- */

/* Creates a context bound to HIP device `device_ordinal`.  Fails with PG_ERR_NO_DEVICE when
 * no GPU is visible: there is no CPU fallback. */
int pg_create(pg_context **out, int device_ordinal);
int pg_destroy(pg_context *ctx);
/* ctx may be NULL: returns the message of the last failed pg_create on this thread. */
const char *pg_last_error(const pg_context *ctx);
int pg_abi_version(void);

/* PathGuidingIntegrator.setup (path_guiding_integrator.py:77-105): both SD-trees become a
 * single-leaf KD tree over [bbox_min,bbox_max] owning a single-leaf quadtree
 * (kdtree.py:117-138, quadtree.py:350-362).  num_rays / max_depth size the dense record
 * buffer of pg_process_records (path_guiding_integrator.py:93). */
int pg_setup(pg_context *ctx, const float h_bbox_min[3], const float h_bbox_max[3],
             uint64_t num_rays, int32_t max_depth, int32_t kd_max_depth, int32_t quad_max_depth,
             int32_t store_nee, float bsdf_sampling_fraction);

/* PathGuidingIntegrator.setIteration (path_guiding_integrator.py:121-123). */
int pg_set_iteration(pg_context *ctx, int32_t iteration, int32_t is_final);

/* ---- queries on sdTree_prev ----------------------------------------------------------- */

/* KDTree.getLeafNodeIndex (kdtree.py:435-470): node index in the reference's numbering. */
int pg_get_leaf_node_index(pg_context *ctx, uint64_t n, const float *p, const uint8_t *active,
                           uint32_t *node_out, void *stream);

/* KDTree.sample (kdtree.py:473-486): direction sampled from the quadtree of the leaf that
 * contains p, and its pdf.  rng_state/rng_inc are per-lane PCG32 streams, advanced in place
 * by 3 draws per visited quadtree node (quadtree.py:956, 980).  Inactive lanes return
 * dir (0,0,-1), pdf 1 and leave their stream untouched. */
int pg_sample(pg_context *ctx, uint64_t n, const float *p, uint64_t *rng_state,
              const uint64_t *rng_inc, const uint8_t *active, float *dir_out, float *pdf_out,
              void *stream);

/* KDTree.pdf (kdtree.py:489-496). */
int pg_pdf(pg_context *ctx, uint64_t n, const float *p, const float *dir, const uint8_t *active,
           float *pdf_out, void *stream);

/* The three SD-tree calls of one bounce (path_guiding_integrator.py:244, 301, 307) with a
 * single KD descent:
 *   pdf_nee_out[i] = sdTree_prev.pdf(p, dir_nee)             if nee_active[i]   (else 1)
 *   select[i] == 2 : (dir_io, pdf_out) = sdTree_prev.sample(p, rng)   ("sdtree-mis" lanes)
 *   select[i] == 1 : pdf_out = sdTree_prev.pdf(p, dir_io)             ("bsdf-mis" lanes)
 *   select[i] == 0 : pdf_out = 1, dir_io untouched, stream untouched
 * dir_io holds the BSDF-sampled world direction on entry.
 * lane_index / d_lane_count (both NULL, or both set): the compacted list of live ray slots and
 * its two counters as written by pg_compact_lanes; only those slots are processed (and written),
 * and the launch costs waves in proportion to the counters, which are read on the device (no
 * host round trip between bounces). */
int pg_guide_bounce(pg_context *ctx, uint64_t n, const float *p, const float *dir_nee,
                    const uint8_t *nee_active, const uint8_t *select, float *dir_io,
                    uint64_t *rng_state, const uint64_t *rng_inc, float *pdf_nee_out,
                    float *pdf_out, const uint32_t *lane_index, const uint32_t *d_lane_count,
                    void *stream);

/* Active-ray stream compaction between bounces of the wavefront loop (the reference masks dead
 * lanes instead, path_guiding_integrator.py:179, 380).  A lane is live when select[i] != 0 or
 * nee_active[i] != 0 (nee_active may be NULL).  idx_out (uint32[n]) receives the lanes with
 * select == 2 packed from the front, idx_out[0 .. d_count[0]), and the other live lanes packed
 * from the back, idx_out[n-1], idx_out[n-2], ... (d_count[1] of them), so that waves of the
 * bounce kernel do not mix the sampling and the pdf-only code paths.  Order inside each class
 * is unspecified.  d_count is a device uint32[2], zeroed by the call; masks 16-byte aligned. */
int pg_compact_lanes(pg_context *ctx, uint64_t n, const uint8_t *select, const uint8_t *nee_active,
                     uint32_t *idx_out, uint32_t *d_count, void *stream);

/* Mitsuba `independent` sampler seeding for lanes lane0..lane0+n (PCG32 + TEA). */
int pg_rng_seed(pg_context *ctx, uint64_t n, uint32_t seed, uint32_t lane0, uint64_t *rng_state,
                uint64_t *rng_inc, void *stream);

/* ---- recording into sdTree_current ---------------------------------------------------- */

/* Compact record stream = what KDTree.addDataPropagate consumes (kdtree.py:180-225,
 * quadtree.py:389-464) after scatterDataIntoSDTree's gathers
 * (path_guiding_integrator.py:485-497).  radiance_nee_lum = mi.luminance(radiance_nee). */
typedef struct pg_records {
	const float *position;         /* Vector3f[m] planar */
	const float *direction;        /* Vector2f[m] canonical, planar */
	const float *radiance;         /* Float[m] */
	const float *wo_pdf;           /* Float[m] */
	const float *direction_nee;    /* Vector2f[m] canonical, planar (ignored if !store_nee) */
	const float *radiance_nee_lum; /* Float[m]                       (ignored if !store_nee) */
} pg_records;

/* KDTree.addDataPropagate: adds the m records to sdTree_current.  If d_count is non-NULL it
 * points to a device uint32 holding the number of valid records (<= m), e.g. the counter
 * written by pg_process_records; otherwise all m are used. */
int pg_splat(pg_context *ctx, uint64_t m, const pg_records *rec, const uint32_t *d_count,
             void *stream);

/* Dense per-pass record buffer, slot = ray*max_depth + depth
 * (path_guiding_integrator.py:318-346). */
typedef struct pg_dense_records {
	const uint8_t *active;
	const float *position;            /* Vector3f[S] */
	const float *direction;           /* Vector2f[S] canonical */
	const float *bsdf;                /* Color3f[S]  bsdf_weight */
	const float *throughput_bsdf;     /* Color3f[S]  */
	const float *throughput_radiance; /* Color3f[S]  */
	const float *radiance_nee;        /* Color3f[S]  */
	const float *direction_nee;       /* Vector2f[S] canonical */
	const float *wo_pdf;              /* Float[S] */
} pg_dense_records;

typedef struct pg_records_out {
	float *position, *direction, *radiance, *wo_pdf, *direction_nee, *radiance_nee_lum;
} pg_records_out;

/* processPathData + scatterDataIntoSDTree's filter (path_guiding_integrator.py:434-497):
 * writes the surviving records (any order) with plane stride S = num_rays*max_depth and their
 * number to *d_count (device uint32, zeroed by the call). */
int pg_process_records(pg_context *ctx, uint64_t num_rays, int32_t max_depth, const float *l_final,
                       const pg_dense_records *rec, const pg_records_out *out, uint32_t *d_count,
                       void *stream);

/* Same, fused with pg_splat: no intermediate stream (path_guiding_integrator.py:388-395). */
int pg_process_and_splat(pg_context *ctx, uint64_t num_rays, int32_t max_depth,
                         const float *l_final, const pg_dense_records *rec, void *stream);

/* ---- training filters of the record boundary (not in the reference) -------------------- */

/* How pg_splat and pg_process_and_splat deposit a record.  The default, and the reference's behaviour, is nearest / nearest:
 * a record adds to the one quadtree leaf its direction falls in, inside the one KD leaf its position falls in; those calls then
 * run exactly the kernels they ran before this entry point existed.  The two filters of the 2019 follow-up of the method
 * ("Path Guiding in Production", ch. 10) are extensions beyond the reference.  Context state; pg_setup resets it to
 * nearest / nearest, seed 0.  Unknown values: PG_ERR_INVALID.  All arithmetic below is fp32, every operation rounded on its
 * own (the arithmetic contract), in exactly the order written; names of columns are those of pg_tree_columns.
 *
 * PG_SPATIAL_STOCHASTIC_BOX.  For record number i with position p inside the root box (inclusive; a record outside it or
 * with a NaN coordinate is handled exactly as without the filter): L = the KD leaf of p (KDTree.getLeafNodeIndex),
 *     e[a]  = kd_bbox_max[L][a] - kd_bbox_min[L][a]                                   a = x, y, z
 *     u[a]  = the first three next_f32 of the PCG32 stream pg_rng_seed(seed, lane = i) seeds, in the order x, y, z
 *     p'[a] = min(max(p[a] + (u[a] - 0.5) * e[a], root_min[a]), root_max[a])
 * and the whole record -- its count and both of its directional deposits -- goes to the KD leaf of p'.  i is the record's
 * index in pg_splat's stream; in pg_process_and_splat it is the dense slot g = ray * max_depth + depth modulo 2^32.  The two
 * routes therefore jitter the same record differently (a compacted stream numbers the survivors, the dense buffer the slots).
 *
 * PG_SPATIAL_OVERLAP_BOX.  The box filter itself, of which the stochastic box is a one-sample estimate: the record is shared
 * between all KD leaves that a box the size of its own KD leaf, placed around its position, overlaps, each in proportion to the
 * overlap's volume.  No random numbers: `seed` is ignored.  For a record with position p inside the root box (inclusive; a
 * record outside it or with a NaN coordinate is handled exactly as without the filter): L = the KD leaf of p,
 *     e[a]  = kd_bbox_max[L][a] - kd_bbox_min[L][a]                                   a = x, y, z
 * The record's COUNT goes to L alone, and within L's quadtree to the leaf the nearest walk of the path direction finds -- also
 * where that leaf's share of the energy comes out zero; a counted record whose direction reaches no leaf increments the fallback
 * counter of L's quadtree once, as without the filter.  If L is the root (depth 0), or an e[a] is not finite or is <= 0, the
 * record is handled exactly as with PG_SPATIAL_NEAREST.  Else the box B = [lo, hi] is, per axis,
 *     lo[a] = max(p[a] - 0.5 * e[a], root_min[a])          hi[a] = lo[a] + e[a]
 *     if hi[a] > root_max[a]:  hi[a] = root_max[a],  lo[a] = max(hi[a] - e[a], root_min[a])
 * i.e. B is SHIFTED to stay inside the root box; nothing is clipped away (as the directional footprint in y).  For every KD
 * leaf M of the tree
 *     len[a] = min(kd_bbox_max[M][a], hi[a]) - max(kd_bbox_min[M][a], lo[a])
 * (The leaves are found from the root, entering a child only if B reaches across its parent's split plane.  That finds every
 * leaf with len[a] > 0 in a tree whose boxes nest -- a child's box is its parent's, cut at the split plane on the split axis --
 * which holds for every tree this library builds or refines; pg_import verifies that the children of a node meet at its split
 * plane, not the nesting, and on an imported tree whose boxes do not nest the leaves the walk does not reach receive nothing.)
 * M takes part exactly when len[a] > 0 on all three axes, with the share
 *     s = ((len[0] / e[0]) * (len[1] / e[1])) * (len[2] / e[2])          (three IEEE divisions, two products)
 * and for each (direction, weight w) pair of the record -- (direction, radiance / wo_pdf) and, with store_nee, (direction_nee,
 * radiance_nee_lum / wo_pdf) -- M's quadtree receives the pair (direction, w * s) (one product) through the directional filter
 * that is set: PG_DIRECTIONAL_NEAREST deposits quantize(w * s) in the nearest leaf of M's quadtree, PG_DIRECTIONAL_BOX follows
 * the rules below with w := w * s and N found in M's own quadtree.  No counts are added in M != L.  A direction outside the unit
 * square deposits nothing in any M.  Energy is conserved up to these roundings and one truncation to 2^-PG_FRAC_BITS per deposit.
 *
 * PG_DIRECTIONAL_BOX.  For a (direction c = (cx, cy), weight w) pair of a record -- (direction, radiance / wo_pdf) and, with
 * store_nee, (direction_nee, radiance_nee_lum / wo_pdf) -- in the quadtree of the record's KD leaf.  A direction outside the
 * unit square is handled exactly as without the filter (fallback counter included).  Otherwise N = the leaf the nearest walk
 * finds (QuadTree.addIrradiancePropagate's descent), d = quad_depth[N] - quad_depth[root] (at most 30, the
 * depth limit of pg_setup), G = 2^d.  The record COUNT goes to
 * N alone, as without the filter.  If d = 0 (the root is the leaf), N receives quantize(w): identical to nearest.  Else the
 * footprint is the square of side 2^-d centred on c; in units of that side (every scaling by G is exact):
 *     vx = cx * G - 0.5          jx = floor(vx)    tx = vx - jx       X0 = jx mod G (jx = -1 wraps to G - 1), X1 = (X0 + 1) mod G
 *     vy = max(cy * G - 0.5, 0)  jy = floor(vy)    ty = vy - jy       if jy >= G - 1: jy = G - 1, ty = 0      Y0 = jy, Y1 = jy + 1
 * i.e. in x (cx = phi / 2 pi, periodic) the footprint WRAPS modulo 1, in y (not periodic) it is SHIFTED to stay inside
 * [0, 1]; nothing is clipped away.  The footprint meets at most the 2 x 2 block of depth-d cells (X_a, Y_b), a, b in {0, 1}.
 * In the local frame of cell (X_a, Y_b) -- the cell is [0, 1]^2 -- the footprint is the rectangle [lx, hx] x [ly, hy] with
 *     (lx, hx) = (tx, 1) for a = 0, (0, tx) for a = 1          (ly, hy) = (ty, 1) for b = 0, (0, ty) for b = 1.
 * Column a is EMPTY when hx - lx <= 0 (one subtraction: 1 - tx, or tx - 0), row b likewise; cells of an empty column or row
 * receive nothing.  Every leaf M of the tree that meets the footprint with positive area receives ONE deposit
 *     quantize(w * (ox * oy))          (one product ox * oy, then one product with w; quantize = the fixed-point truncation)
 * where ox, oy are M's overlap lengths with the footprint in units of the footprint's side (the division of the overlap
 * area by the footprint's area is a scaling by a power of two: exact, and already made):
 *   - M at depth <= d, containing one or more of the non-empty cells: ox = 1 exactly if both columns are non-empty and
 *     both lie in M, else hx - lx of its one column; oy likewise for the rows.
 *   - M below a non-empty cell (X_a, Y_b), with the local cell [u0, u0 + h] x [v0, v0 + h] (h a power of two, u0, v0 multiples
 *     of h: exact): ox = min(u0 + h, hx) - max(u0, lx), oy = min(v0 + h, hy) - max(v0, ly); M receives its deposit when
 *     ox > 0 and oy > 0.
 * Energy is conserved up to the roundings of these products and one truncation to 2^-PG_FRAC_BITS per deposit.  A weight
 * whose own quantize(w) is zero (0, NaN, |w| < 2^-PG_FRAC_BITS) deposits nothing anywhere, as every part of it would.
 *
 * A spatial and the directional filter may be set together: the jitter first, then the directional deposits in the quadtree of
 * the KD leaf of p'; or the directional deposits of (direction, w * s) in every KD leaf under the overlap box.
 * Sums stay exact integers: filtered results do not depend on the order of the records or of the launches, and refine, the
 * exchange format, pg_allreduce and export see nothing new.
 * The library's own renderer by default does not carry a vertex's position and directions to its splat (it names the two leaves
 * found during the bounce): while a filter other than nearest / nearest is set, a RECORDING pg_render_pass (iteration not final)
 * fails with PG_ERR_INVALID and names the filter; it never falls back to nearest.  A final-iteration pass is unaffected.
 * A scene set with pg_render_record_geometry on lifts the refusal: its recording passes keep the vertices' geometry and deposit
 * through the filters (see there).
 * pg_enable_depth_counters: a filtered launch adds nothing to the depth counters. */
#define PG_SPATIAL_NEAREST 0
#define PG_SPATIAL_STOCHASTIC_BOX 1
#define PG_SPATIAL_OVERLAP_BOX 3   /* 2 is not assigned and stays refused */
#define PG_DIRECTIONAL_NEAREST 0
#define PG_DIRECTIONAL_BOX 1
int pg_set_splat_filter(pg_context *ctx, int32_t spatial, int32_t directional, uint32_t seed);

/* ---- per-iteration refinement --------------------------------------------------------- */

/* refineAndPrepareSDTreeForNextIteration (path_guiding_integrator.py:566-586) with the
 * iteration number given to pg_set_iteration: KD split, quadtree threshold/merge/split,
 * canonical re-layout, prev <- current, reset.  Synchronises `stream`.
 * A TRANSACTION, as the reference's allocate-new + copy growth is (common.py:161-189: its arrays are replaced, never edited, so
 * sdTree_prev survives a failed split): the refined KD tree, the new quadtree forest and the next iteration's accumulators are
 * built in spare buffers and committed by pointer swap.  On ANY error (PG_ERR_NOMEM from an allocation, a limit) sdTree_prev and
 * sdTree_current -- topology, sampling values and the running iteration's accumulators -- are exactly what they were before the
 * call: every query, pass and export answers bit for bit as before, and the call may simply be repeated. */
int pg_refine_and_swap(pg_context *ctx, void *stream);

/* Fault injection for the tests of that guarantee (tests/test_gpu_errors.py); process-wide, not for production use:
 * after `successes_before_failure` further device allocations of the library have succeeded, the next one reports out of memory
 * exactly as a refused hipMalloc does, and the hook disarms itself (-1 disarms it at once).  pg_debug_fail_alloc_pending
 * returns 1 while a failure is armed and has not happened yet, 0 otherwise (the hook fired or was never armed). */
int pg_debug_fail_alloc(int64_t successes_before_failure);
int pg_debug_fail_alloc_pending(void);

/* Views of sdTree_current's integer accumulators for the multi-GPU exchange: one contiguous
 * device buffer of `count` int64 that is element-wise summable across ranks (topology is
 * frozen during an iteration, so the buffers are index-aligned).  Sum it with an RCCL
 * all-reduce (ncclInt64, ncclSum) before pg_refine_and_swap. */
int pg_accumulators(pg_context *ctx, int64_t **d_buffer, uint64_t *count);

/* The exchange itself for hosts that do not bring their own collective library: one RCCL
 * all-reduce (ncclAllReduce, ncclInt64, ncclSum, in place) of that buffer over the ranks, asynchronous
 * on `stream`; call it on every rank after the iteration's last pass and before pg_refine_and_swap --
 * exact integer sums, so every rank then refines the same tree.  RCCL is loaded at run
 * time (the copy the process already holds, else librccl.so.1 from the library path, else
 * $PGSD_RCCL_LIBRARY); nothing of it is touched before the first pg_comm_* call.
 *   pg_comm_unique_id : ncclGetUniqueId into h_id_out[PG_COMM_ID_BYTES] (rank 0 calls it and hands the
 *                       bytes to the other ranks by whatever channel the host has)
 *   pg_comm_init      : ncclCommInitRank on the context's device; collective over the n_ranks callers
 *   pg_comm_attach    : use a communicator the host already owns (an ncclComm_t of the same RCCL
 *                       library; it stays the host's: pg_comm_destroy / pg_destroy do not destroy it)
 * There is no reference counterpart (single process, single GPU: SURVEY 8e). */
#define PG_COMM_ID_BYTES 128
int pg_comm_unique_id(pg_context *ctx, uint8_t *h_id_out);
int pg_comm_init(pg_context *ctx, int32_t n_ranks, int32_t rank, const uint8_t *h_id);
int pg_comm_attach(pg_context *ctx, void *nccl_comm, int32_t n_ranks);
int pg_comm_destroy(pg_context *ctx);
int pg_allreduce(pg_context *ctx, void *stream);
/* What RCCL itself says about the context's communicator -- ncclCommCount and ncclCommUserRank read back, not the numbers
 * the caller passed to pg_comm_init: a witness that the library's exchange really spans n ranks. */
int pg_comm_info(pg_context *ctx, int32_t *n_ranks_out, int32_t *rank_out);

/* The exchange format.  An accumulator is four int64 words on the device (three limbs of 32 payload bits + a record
 * count: 32 bytes, cheap to add to with 64-bit atomics); what has to travel between GPUs is its VALUE, 24 bytes:
 *     T = l0 + l1 2^32 + l2 2^64      p0 = T mod 2^52    p1 = (T >> 52) mod 2^52    p2 = (count << 24) + (T >> 104)
 * (|T| < 2^119 and sum of counts < 2^31 per accumulator and iteration over all ranks -- the bounds the limbs rely on
 * anyway).  Element-wise int64 sums of packed buffers over up to 2^11 ranks cannot overflow and decode to the exact sums.
 *   pg_exchange_pack   : packs sdTree_current's accumulators into a library-owned device buffer of *count int64
 *                        ([accumulators x 3 | per-tree fallback counters]) on `stream`; the accumulators stay as they are
 *   pg_exchange_unpack : writes the (summed) packed buffer back into the accumulators on `stream`: same values, same counts
 * A host with its own collective: pack, all-reduce *d_buffer (int64, sum), unpack, pg_refine_and_swap.  pg_allreduce does
 * exactly that with RCCL.  Summing the raw pg_accumulators buffer stays valid (a third more bytes).
 *   pg_exchange_pack_words / _unpack_words : the same arithmetic on HOST arrays of n_acc accumulators (4 words in, 3 out and
 *                        back); no context, no device. */
int pg_exchange_pack(pg_context *ctx, int64_t **d_buffer, uint64_t *count, void *stream);
int pg_exchange_unpack(pg_context *ctx, void *stream);
int pg_exchange_pack_words(const int64_t *h_acc, uint64_t n_acc, int64_t *h_out);
int pg_exchange_unpack_words(const int64_t *h_in, uint64_t n_acc, int64_t *h_acc_out);

/* ---- import / export in the reference's schema (kdtree.py:539-602) -------------------- */

typedef struct pg_tree_sizes {
	uint64_t n_kd, n_quad, n_roots;
} pg_tree_sizes;

/* HOST arrays in the reference's column layout: bbox columns are row-major [n][3] / [n][2]
 * exactly as `.numpy()` yields them. */
typedef struct pg_tree_columns {
	double kd_max_leaf_size;
	int32_t kd_max_depth, quad_max_depth, quad_store_nee;
	float *kd_bbox_min, *kd_bbox_max;
	uint32_t *kd_depth;
	float *kd_vert_count;
	uint8_t *kd_is_leaf;
	uint32_t *kd_quad_root_index, *kd_child_left, *kd_child_right;
	uint32_t *quad_root_node_index;
	float *quad_bbox_min, *quad_bbox_max;
	uint32_t *quad_depth;
	float *quad_irradiance;
	uint8_t *quad_is_leaf;
	float *quad_threshold;
	uint32_t *quad_child[4];
} pg_tree_columns;

/* Sizes of sdTree_prev in canonical layout. Synchronous. */
int pg_export_sizes(pg_context *ctx, pg_tree_sizes *sizes);
/* KDTree.saveToFile's columns for sdTree_prev (path_guiding_integrator.py:589-594). */
int pg_export(pg_context *ctx, const pg_tree_sizes *sizes, pg_tree_columns *h_out);
/* loadSDTreeFromFile (path_guiding_integrator.py:597-608): prev <- file, current <- reset copy. */
int pg_import(pg_context *ctx, const pg_tree_sizes *sizes, const pg_tree_columns *h_in);
/* Exact accumulators of sdTree_current resolved per canonical node (tests, diagnostics):
 * kd_count[n_kd] (records through each KD node), quad_acc_lo/hi[n_quad] (128-bit sums). */
int pg_export_accumulators(pg_context *ctx, const pg_tree_sizes *sizes, uint64_t *h_kd_count,
                           uint64_t *h_quad_acc_lo, int64_t *h_quad_acc_hi);

/* ---- renderer substrate: PathGuidingIntegrator.sample() on device ----- */

/* Scene subset of the reference's scenes/cornell-box/scene.xml: parallelograms ("rectangle" and
 * the six faces of "cube" shapes) with twosided diffuse BSDFs, one one-sided area emitter, a
 * perspective sensor.  h_quads is a HOST array of n_quads*24 floats:
 *   0-2 origin  3-5 edge1  6-8 edge2  9-11 unit normal (= normalised e1 x e2)
 *   12 1/|e1|^2  13 1/|e2|^2  14 area  15 emitter flag  16-18 diffuse reflectance
 *   19-21 emitted radiance  22 material index (pg_scene_set_ex with a material table)  23 unused
 * (practical_path_guiding_lab_amd/scene.py builds it from Mitsuba XML). */
#define PG_QUAD_STRIDE 24
/* sphere: 0-2 centre  3 radius  4 material index  5 emitter flag  6-8 emitted radiance  9-11 unused */
#define PG_SPHERE_STRIDE 12
/* material: 0 type (0 diffuse; 1 roughconductor, beckmann, sample_visible; 2 smooth conductor;
 *   3 smooth dielectric; 4 roughdielectric, beckmann, sample_visible)  1-3 reflectance |
 *   specular_reflectance  4 alpha (> 0: beckmann; < 0: ggx of roughness -alpha)
 *   5-7 eta (dielectrics: 5 = int_ior / ext_ior)  8-10 k
 *   11 one-sided flag (0 = wrapped in `twosided`)
 *   12 texture index + 1 (0: none): on triangles with texture coordinates the texture replaces
 *      words 1-3 (scenes/veach-ajar/scene.xml:29-80: `bitmap` reflectances, a `checkerboard`
 *      specular_reflectance)  13-15 unused */
#define PG_MATERIAL_STRIDE 16
/* texture, 16 32-bit words: 0 kind (1 `bitmap`, bilinear, repeat; 2 `checkerboard`)  1 width  2 height
 *   3 index of its first texel in `texels`  4-6 color0  7-9 color1 (checkerboard; f32 bit patterns)
 *   10-11 to_uv scale  12-13 to_uv offset (f32 bit patterns)  14-15 unused */
#define PG_TEXTURE_STRIDE 16
/* box (Mitsuba's `cube`: [-1,1]^3 under an affine to_world), intersected as three slabs in its local
 * frame instead of six quads: 0-8 rows of A = (linear part of to_world)^-1, 9-11 centre c
 * (local = A (p - c)), 12-20 outward unit normals of the +x, +y, +z faces (the normalised rows
 * of A), 21 material index, 22-31 unused by the library */
#define PG_BOX_STRIDE 32
typedef struct pg_camera {
	float origin[3];
	float axis_x[3], axis_y[3], axis_z[3]; /* columns of the sensor's to_world rotation */
	float tan_half_fov_x;
	int32_t width, height;
} pg_camera;
int pg_scene_set(pg_context *ctx, uint64_t n_quads, const float *h_quads, const pg_camera *cam);

/* The scene subset of scenes/veach-mis/scene.xml on top of that: "sphere" shapes (also as area
 * emitters, sampled over the cone they subtend), several emitters (one is chosen uniformly per
 * sample, scene.sample_emitter_direction), and a material table with twosided rough conductors
 * (Beckmann, visible-normal sampling).  Shapes are numbered quads first, then spheres.  All HOST
 * arrays; materials == NULL means "quad i is diffuse with quads[i][16..18]" (no spheres then). */
typedef struct pg_scene_desc {
	uint64_t n_quads;
	const float *quads;     /* PG_QUAD_STRIDE floats each */
	uint64_t n_spheres;
	const float *spheres;   /* PG_SPHERE_STRIDE floats each */
	uint64_t n_materials;
	const float *materials; /* PG_MATERIAL_STRIDE floats each */
	uint64_t n_boxes;
	const float *boxes;     /* PG_BOX_STRIDE floats each; need a material table */
	/* triangle meshes (`obj` / `serialized` shapes of the reference's scenes) behind one four-wide
	 * BVH, built by the caller (practical_path_guiding_lab_amd/mesh.py):
	 *   triangle, PG_TRI_STRIDE floats: 0-2 v0, 3-5 v1 - v0, 6-8 v2 - v0, 9-11 unit geometric
	 *     normal, 12 material index; stored in BVH leaf order
	 *   node, PG_BVH_STRIDE 32-bit words (128 bytes): 0-23 (f32) the boxes of its up to four
	 *     children, lo_x[4] lo_y[4] lo_z[4] hi_x[4] hi_y[4] hi_z[4]; 24-27 (u32) the children: a node
	 *     index, or 0x80000000 | (count-1) << 28 | first triangle for a leaf of 1..8 triangles, or
	 *     0xffffffff for none; 28-31 unused by the library.  Node 0 is the root (also when it holds
	 *     a single leaf), children have larger indices than their parent and one parent each, leaves
	 *     stay inside the triangle array, no root-to-node path leaves more than 32 siblings waiting,
	 *     at most 2^25 nodes (all checked).  The boxes of absent children are ignored.  The ray-casting
	 *     kernels read the first 48 nodes of the table from LDS: a builder that gives the lowest numbers
	 *     to the nodes most rays open (the biggest boxes; mesh.build_bvh does) makes them faster, any
	 *     numbering that keeps children behind their parent is walked correctly.  Shape numbers of
	 *     triangles follow the box faces. */
	uint64_t n_tris;
	const float *tris;
	uint64_t n_bvh_nodes;
	const uint32_t *bvh;
	/* `directional` emitters (scenes/torus/scene.xml), PG_DIRLIGHT_STRIDE floats each: 0-2 unit
	 * direction the light travels in, 3-5 irradiance.  They follow the area emitters in the uniform
	 * emitter choice.  bsphere: centre and radius of the scene's bounding sphere (Mitsuba places a
	 * directional sample two radii up the light's direction). */
	uint64_t n_dir_lights;
	const float *dir_lights;
	float bsphere[4];
	/* optional unit vertex normals, 9 floats per triangle in the order of `tris` (NULL: face
	 * normals).  The shading frame follows the interpolated normal, ray offsets the geometric one
	 * (Mitsuba's si.sh_frame.n and si.n). */
	const float *tri_normals;
	/* optional texture coordinates, 6 floats per triangle (uv0 uv1 uv2) in the order of `tris`, with v
	 * already flipped as Mitsuba's obj loader does (row 0 of a bitmap is v = 0); the texture table; the
	 * texels of all bitmaps (8-bit sRGB packed R | G << 8 | B << 16) and the 256 linear values they are
	 * looked up in (8-bit sRGB -> linear, as Mitsuba converts a JPG texel).  All HOST arrays. */
	const float *tri_uvs;
	uint64_t n_textures;
	const uint32_t *textures; /* PG_TEXTURE_STRIDE words each */
	uint64_t n_texels;
	const uint32_t *texels;
	const float *srgb_lut;    /* 256 floats */
} pg_scene_desc;
#define PG_DIRLIGHT_STRIDE 8
#define PG_TRI_STRIDE 16
#define PG_BVH_STRIDE 32
int pg_scene_set_ex(pg_context *ctx, const pg_scene_desc *scene, const pg_camera *cam);

typedef struct pg_pass_params {
	uint32_t seed;    /* sampler seed of the pass (main.py:218: initial_seed + cumm_spp) */
	int32_t spp;      /* samples per pixel traced by this pass; lane = pixel*spp + s (:414-417); see `batched` */
	int32_t rr_depth; /* Russian roulette from this depth on (:39, 375) */
	/* 0 or 1: the set of pass buffers this pass uses.  The passes of an iteration are independent (main.py:208-218 seeds
	 * each with initial_seed + cumm_spp), so two may be on the device at once: issue them alternately with slot 0 on one
	 * stream and slot 1 on another.  The per-pixel sums are still added in the order the passes were issued (the library
	 * orders the two streams there); sdTree_current receives integer adds, whose order is free.  Passes of one slot must
	 * be issued on one stream.  0 everywhere = the reference's one-pass-at-a-time behaviour. */
	int32_t slot;
	/* image tile traced by this call (multi-GPU sharding): pixels [pixel_begin, pixel_begin +
	 * pixel_count) in row-major film order; pixel_count 0 = up to the end of the film.  Sampler
	 * streams are keyed by the global lane id, so the union of tiles equals the full-frame pass.
	 * L_out / valid_out hold only the tile's lanes; sumL / sumL2 are full-film arrays. */
	uint64_t pixel_begin, pixel_count;
	/* Interleaved sharding (load balance across GPUs): with stripe_count > 1 the call traces the rows r
	 * of the film with (r / stripe_rows) % stripe_count == stripe_index -- bands of stripe_rows rows dealt
	 * round-robin -- in ascending order; pixel_begin must be 0 and pixel_count the number of pixels of
	 * those rows (or 0).  The tile-local pixel i of L_out / valid_out is column i % width of the
	 * (i / width)-th owned row.  stripe_count 0 or 1: the contiguous range above. */
	uint32_t stripe_rows, stripe_index, stripe_count;
	/* 0: one pass of `spp` samples per pixel, lane = pixel*spp + s, sampler stream = lane of `seed` (mi.render(spp=spp, seed)).
	 * 1: the call stands for `spp` consecutive ONE-sample passes with the seeds seed, seed + 1, ... seed + spp - 1 -- the
	 *    reference's training passes (main.py:192 renders them with spp 1, :218 seeds them initial_seed + cumm_spp) --
	 *    traced together in one wavefront: sample s of a pixel is the sample pass seed + s gives that pixel (stream =
	 *    pixel of seed + s).  Radiance per sample, the per-pixel sums (added in pass order), sdTree_current and -- with
	 *    pg_film_batched -- the developed images are those of the spp separate calls, bit for bit; only the number of
	 *    kernel launches differs.  L_out keeps the lane order pixel*spp + s. */
	uint32_t batched;
} pg_pass_params;

/* One call of PathGuidingIntegrator.sample() for all width*height*spp lanes
 * (path_guiding_integrator.py:126-431): camera rays, max_depth bounces with NEE + one-sample MIS
 * between BSDF and sdTree_prev sampling (guiding active when iteration > 1), record store, then
 * processPathData + scatterDataIntoSDTree into sdTree_current unless the iteration is final.
 * max_depth, iteration, is_final, store_nee and the sampling fraction come from pg_setup /
 * pg_set_iteration.  L_out: Color3f[lanes] planar (device); valid_out: uint8[lanes] or NULL;
 * sumL/sumL2: Color3f[width*height] planar accumulators (:400-429) or both NULL. */
int pg_render_pass(pg_context *ctx, const pg_pass_params *prm, float *L_out, uint8_t *valid_out,
                   float *sumL, float *sumL2, void *stream);

/* Not in the reference (Dr.Jit orders its kernels by data dependence on one stream): mode 1 lets the two kernels
 * of a mesh scene's bounce that do not depend on each other -- the SD-tree queries (k_wave_guide,
 * src/path_guiding_integrator.py:244, 301, 307) and the shadow rays (k_wave_cast, :213 test_visibility) -- run side by
 * side, the queries on a library-owned stream that forks from and joins the caller's stream inside pg_render_pass.
 * Results are identical (the two write disjoint buffers).  Default 0: every kernel on the caller's stream. */
int pg_render_overlap(pg_context *ctx, int32_t mode);

/* How the pipeline of mesh scenes cuts a bounce into kernels behind the closest hits (k_wave_trace) -- the same device
 * functions on the same numbers either way, results identical:
 *   0 (default)  one kernel, k_wave_shade: surface, emitter sample, BSDF sample, the SD-tree calls
 *                (src/path_guiding_integrator.py:244, 301, 307 and the leaves a record adds to), the shadow ray (:213), mixture
 *                pdfs, record, throughput, roulette, the next ray -- on one lane's registers, nothing of it through memory;
 *   1            three: k_wave_shade_a (:189-220, 272-297 and the SD-tree calls), k_wave_cast (:213, a persistent any-hit
 *                kernel), k_wave_shade_b (:247-261, 302-381), handing their results on through workspace planes;
 *   2            four: the SD-tree calls as a kernel of their own, k_wave_guide, which reads the vertex back from the
 *                workspace -- the hot path of SURVEY 8 by itself, for timing and counters (pg_kernel_timing.guide_ms;
 *                bench.py measures its roofline this way).  pg_render_overlap(1) implies it. */
int pg_render_stages(pg_context *ctx, int32_t mode);

/* Not in the reference (Dr.Jit's wavefront keeps pixel order): with `on`, the bounces of a mesh scene from the second one
 * (bounce 1) to bounce min(rr_depth, max_depth - 1) inclusive -- the bounce at whose end Russian roulette first thins the list
 * out still shades every path that reached it -- process the live list in a global spatial order, those of them that enough
 * lanes reached in the buffer set's previous pass: the places sorted by the Morton cell of the vertex
 * the ray has just found (a device radix sort of 16-bit keys per bounce) -- so that the lanes of a wave stand next to
 * each other in the scene for the shading, the shadow rays, the SD-tree queries and, after the survivors are appended
 * in that order, the next bounce's closest hits.  A lane's result depends on its own state only: radiance, sums,
 * accumulators and trees are those of the unsorted run, bit for bit.  Default 0. */
int pg_render_sort(pg_context *ctx, int32_t on);

/* Allocates what pg_render_pass needs for passes of up to n_lanes lanes (pixels of the tile x spp) ahead
 * of time -- the reference allocates its numRays x max_depth record arrays in setup()
 * (path_guiding_integrator.py:93, 116); without this call the first pass of a size allocates them.
 * After the pass buffers, for passes of >= 2^20 lanes and only while the device still has four times the jump tables' budget
 * ($PGSD_JUMP_TABLE_MAX_BYTES, default 2 GiB) free, the tables' buffer is also taken at that budget, so that no refine of the
 * training allocates it; $PGSD_JUMP_TABLE_RESERVE=0 switches that off.  It changes allocation times only, never a result, and
 * a refused allocation of it is not an error. */
int pg_render_reserve(pg_context *ctx, uint64_t n_lanes);

/* Which kernels run a bounce.  Scenes of quads, boxes, spheres with diffuse / rough-conductor BSDFs run
 * one fused kernel per bounce; scenes with meshes or the other BSDFs run the split pipeline (ray casting,
 * shading, the SD-tree queries and the rest of the bounce as kernels of their own).  on != 0: every scene
 * set from now on runs the split pipeline.  Results are the same bit for bit either way (the two are
 * independent implementations of path_guiding_integrator.py:126-431: a cross-check, and a way to time the
 * SD-tree queries of any scene as a kernel of their own).  Takes effect at the next pg_scene_set[_ex]. */
int pg_render_split_pipeline(pg_context *ctx, int32_t on);

/* Opt-in vertex geometry in recording passes.  on != 0: every scene set from now on runs the split pipeline (as
 * pg_render_split_pipeline, which this implies), and a RECORDING pg_render_pass of it (iteration not final)
 *   - runs the four-kernel form of a bounce whatever pg_render_stages says (closest hits, shading A, shadow rays, the SD-tree
 *     calls as a kernel of their own, shading B, and the tail kernel at its checkpoints), in the variants of the SD-tree and tail
 *     kernels that also store, for every entry of the pass's record list, eight 32-bit words in planes of the list's stride
 *     n_lanes * max_depth: the vertex's position (3), the canonical path direction (2), the canonical emitter direction (2; (0, 0)
 *     where the bounce computed none -- such an entry's emitter luminance is zero and deposits nothing under either filter) and
 *     the entry's bounce (1).  The planes exist only while the switch is on (32 bytes per entry more than the list's 60);
 *   - with nearest / nearest set: deposits exactly as without the switch (the same kernel on the accumulators the entries name);
 *     radiance, sums, accumulators and refined trees are those of a context with the switch off, bit for bit;
 *   - with another filter set (pg_set_splat_filter) no longer fails: it deposits every kept entry -- one that survives
 *     processPathData and the drop rules of the record boundary -- through the filters, exactly as pg_process_and_splat would for
 *     the dense buffer the reference would have written for the pass.  The jitter's record number is the dense slot
 *     g = ray * max_depth + depth modulo 2^32 (ray: the entry's lane of the pass, depth: its bounce), the seed the one given to
 *     pg_set_splat_filter.  (On the initial tree every filter is the nearest deposit, as for pg_splat.)
 *     Directional-box results are integer sums of per-record deposits: independent of launch order, of sharding (tiles, stripes,
 *     ranks) and of batching.  PG_SPATIAL_OVERLAP_BOX results belong to the same class, with either directional filter: no
 *     record number and no seed enters them.  Stochastic-jitter results are deterministic for a given launch, but do not equal
 *     those of a differently batched or sharded run: record numbers are per launch.  A filtered splat does not touch the depth
 *     counters.
 * A final-iteration pass is untouched and runs the form pg_render_stages selects.  A context with the switch off behaves exactly
 * as before this entry point existed, the filter refusal included.  Takes effect at the next pg_scene_set[_ex].  Default 0. */
int pg_render_record_geometry(pg_context *ctx, int32_t on);

/* The kept records of the most recent pass of buffer set `slot` (pg_pass_params.slot), which must have been a recording pass of a
 * scene set with pg_render_record_geometry on (else PG_ERR_INVALID): pg_process_records' output for the dense buffer the reference
 * would have written -- columns of plane stride n_lanes * max_depth of THAT pass, in any order, *d_count (a device uint32, zeroed
 * by the call) their number.  radiance and radiance_nee_lum are what processPathData yields (the list splat's division chain on
 * the path's final radiance; the NaN-scrubbed luminance).  slot_out (device uint32[n_lanes * max_depth], may be NULL): the dense
 * slot ray * max_depth + depth of record k.  Stream-ordered on `stream`, which must be ordered behind the pass; what it reads is
 * valid until the next pass of that buffer set is issued.  Fed to pg_splat, the stream produces the pass's own accumulators. */
int pg_render_export_records(pg_context *ctx, int32_t slot, const pg_records_out *out, uint32_t *slot_out, uint32_t *d_count,
                             void *stream);

/* Film reconstruction of one full-frame pass with Mitsuba's `tent` reconstruction filter of radius
 * one pixel -- the <rfilter type="tent"/> of the reference's scenes (scenes/cornell-box/scene.xml:27),
 * i.e. the image mi.render returns at main.py:218.  `seed` and `spp` are those of the pass that
 * produced L (Color3f[W*H*spp] planar, as pg_render_pass wrote it): a sample's film position is
 * pixel + its first two sampler draws, which the kernel recomputes.  image_out: Color3f[W*H] planar,
 * sum(w L) / sum(w) over the samples of the pixel's 3x3 neighbourhood, summed in a fixed order. */
int pg_film_tent(pg_context *ctx, uint32_t seed, int32_t spp, const float *L, float *image_out, void *stream);
/* The same with a choice of filter: PG_FILTER_TENT, or PG_FILTER_GAUSSIAN = Mitsuba's default
 * gaussian (stddev 0.5, radius 2, w(d) = max(0, exp(-2 d^2) - exp(-8)) per axis; 5x5 neighbourhood),
 * the film of scenes/torus/scene.xml:46. */
#define PG_FILTER_TENT 0
#define PG_FILTER_GAUSSIAN 1
int pg_film(pg_context *ctx, int32_t filter, uint32_t seed, int32_t spp, const float *L, float *image_out, void *stream);

/* The same for a film sharded by interleaved bands of rows (pg_pass_params.stripe_*; not in the reference, which has
 * one device): develops only the pixels of the rows r with (r / stripe_rows) % stripe_count == stripe_index and leaves
 * the rest of image_out untouched.  L is still indexed by the full frame's lanes, but only this rank's rows and the
 * filter's reach beyond them -- one row for the tent filter, two for the gaussian -- are read: what a rank has to
 * fetch from its neighbours is that halo, not the film.  stripe_count 0 or 1: the whole film (pg_film). */
int pg_film_stripes(pg_context *ctx, int32_t filter, uint32_t seed, int32_t spp, const float *L, float *image_out,
                    uint32_t stripe_rows, uint32_t stripe_index, uint32_t stripe_count, void *stream);

/* The film of a batched call (pg_pass_params.batched = 1): n_passes images, image s = what pg_film_stripes develops for the
 * one-sample pass seed + s alone, from L as the batched pg_render_pass wrote it (lane = pixel*n_passes + s).
 * images_out: n_passes x Color3f[W*H] planar, image-major. */
int pg_film_batched(pg_context *ctx, int32_t filter, uint32_t seed, int32_t n_passes, const float *L, float *images_out,
                    uint32_t stripe_rows, uint32_t stripe_index, uint32_t stripe_count, void *stream);

/* The same without the n_passes images: the running mean main.py keeps of an iteration's passes (:218-239: every pass's image
 * times spp_of_pass / spp_of_iteration, summed in pass order).  acc_io (Color3f[W*H] planar) becomes
 * ((acc + image_0 * scale) + image_1 * scale) + ... in fp32, each product and each sum rounded on its own -- what a host
 * makes of the separate images; with acc_has_value 0 the first image is assigned, not added (acc_io may then be
 * uninitialised on the developed pixels).  A striped call touches its own rows only. */
int pg_film_batched_accumulate(pg_context *ctx, int32_t filter, uint32_t seed, int32_t n_passes, const float *L, float *acc_io,
                               float scale, int32_t acc_has_value, uint32_t stripe_rows, uint32_t stripe_index,
                               uint32_t stripe_count, void *stream);

/* Element-wise evaluation of the library's own fp32 transcendental functions (fixed
 * sequences of double operations, no vendor math library), so that a caller -- the parity tests --
 * can compare them with another implementation of the same contract.
 * which: 0 exp, 1 log, 2 erf, 3 erfinv, 4 sin, 5 cos.  x, out: float[n] device pointers. */
int pg_math_eval(pg_context *ctx, int32_t which, uint64_t n, const float *x, float *out, void *stream);

/* The ordering step of a sorted bounce (pg_render_sort) by itself, for tests: d_places_out[0 .. live) becomes a permutation of
 * the places 0 .. live-1 in the order of their 16-bit keys' HIGH byte -- for every n -- and, inside one high byte, in the order of
 * the low byte only as far as one 4096-pair tile of the second pass allows: equal or adjacent low bytes for n >= 2^21, coarser
 * below, none for n < 2^20 (csrc/pg_sort.hip: two unstable counting passes; the permutation differs from run to run; the
 * renderer's results do not depend on the order at all).  live = min(n, *d_live) -- the places that hold a path, read from device memory; d_live NULL: all n.  Entries of
 * d_places_out behind `live` are not written.  d_keys: uint16[n], d_places_out: uint32[n], device pointers.  Synchronises. */
int pg_sort_places(pg_context *ctx, uint64_t n, const uint16_t *d_keys, const uint32_t *d_live, uint32_t *d_places_out, void *stream);

/* The renderer's ray casting by itself, for tests: ray i = (d_origin[3 i ..], d_dir[3 i ..]) is cast against the scene set on
 * the context, through the very device functions the render kernels call, at the scene's feature level, for hits with
 * 0 < t < d_tmax[i] (strictly; +inf: no limit).  d_t[i] becomes the distance of the closest hit (d_tmax[i] itself where there is
 * none), d_prim[i] its shape number (quads, spheres, 6 box faces per box, triangles in BVH leaf order; -1: no hit) and
 * d_uv[2 i], d_uv[2 i + 1] the barycentrics of a triangle hit (0 for every other shape and for a miss).
 * any_hit != 0: the shadow rays' walk, which stops at the first occluder it meets -- d_prim[i] >= 0 exactly where the closest-hit
 * walk finds something; WHICH occluder, its t and its uv are not specified beyond that.
 * walk_form: how the BVH walk is laid out (the results do not depend on it) -- 0: as in the ray-casting kernels (8 stack
 * entries per lane and the first 48 nodes in LDS), 1: as in k_wave_shade (6 entries, 40 nodes, the register-saving walk),
 * 2: no nodes in LDS.  Deeper stack entries go to overflow strips the call allocates and frees itself.
 * d_origin, d_dir: float[3 n]; d_tmax, d_t: float[n]; d_prim: int32[n]; d_uv: float[2 n]; device pointers, none NULL.
 * n = 0 does nothing; n > 2^20 is refused, as are a context without a scene and a walk_form outside 0..2.  Any float input
 * (NaN, infinities, the zero direction) is safe: the walk is bounded by a step budget.  Synchronises the stream. */
int pg_scene_intersect(pg_context *ctx, uint64_t n, const float *d_origin, const float *d_dir, const float *d_tmax,
                       int32_t any_hit, int32_t walk_form, float *d_t, int32_t *d_prim, float *d_uv, void *stream);

/* The renderer's BSDF layer by itself, for tests: lane i evaluates and samples material row d_material_index[i] of the table
 * d_materials (n_mat rows of PG_MATERIAL_STRIDE floats, the layout of pg_scene_desc.materials) through the very device
 * functions the render kernels call, as a kernel of feature level `level` reads the row (0: every row is a two-sided diffuse
 * material; 1, 2: roughconductor rows too; 3: every type, and one-sided rows).  Directions are in the local frame (z: the
 * normal) and are taken as given, not normalised.
 *   eval:   d_value[3 i ..] = f(wi, wo) cos(theta_o) and d_pdf[i], for wi = d_wi[3 i ..], wo = d_wo[3 i ..];
 *   sample: from d_u[3 i] (the lobe sample) and d_u[3 i + 1], d_u[3 i + 2] (the 2-D sample): d_sampled_wo[3 i ..],
 *           d_sampled_pdf[i], d_weight[3 i ..] = value / pdf, d_eta[i] (the relative index along the sampled direction) and
 *           d_delta[i] (1: a delta lobe was sampled).  A failed sample leaves zeros.
 * The table must pass the material-row checks of pg_scene_set_ex (known type, alpha finite and not 0, index ratio > 0); a
 * row's texture is ignored: the plain reflectance is used.  Needs no scene.  n = 0 does nothing; n > 2^20, n_mat outside
 * 1..65536, a row number outside the table, a level outside 0..3 and a NULL pointer are refused.  All pointers are device
 * pointers.  Synchronises the stream (before reading the table and the row numbers back for the checks, and after the kernel). */
int pg_bsdf_probe(pg_context *ctx, uint64_t n, uint64_t n_mat, const float *d_materials, const int32_t *d_material_index,
                  const float *d_wi, const float *d_wo, const float *d_u, int32_t level, float *d_value, float *d_pdf,
                  float *d_sampled_wo, float *d_sampled_pdf, float *d_weight, float *d_eta, int32_t *d_delta, void *stream);

/* The renderer's description of the surface at a hit by itself, for tests: lane i is a hit of shape d_prim[i] of the scene set
 * on the context by the ray (d_origin[3 i ..], d_dir[3 i ..]) at distance d_t[i], with the barycentrics d_uv[2 i], d_uv[2 i + 1]
 * where the shape is a triangle (what pg_scene_intersect reports for that ray), and d_ref[3 i ..] is the previous path vertex.
 * The lane goes through the very device functions the render kernels call at every vertex, at the scene's feature level:
 * the surface (point, shading and geometric normal, material, texture), the normal recomputed from the point alone, the
 * shading frame, the ray direction taken into it and back, and the density emitter sampling has for the hit.
 * d_out: PG_SURFACE_PROBE_FLOATS floats per lane --
 *   0 p, 3 n (shading normal), 6 ng (geometric normal), 9 reflectance (a texture's colour where the material has one),
 *   12 emitted radiance, 15 the normal of the shape at p as the next bounce recomputes it, 18 the solid-angle density of
 *   emitter sampling from d_ref for this hit times 1 / (number of emitters) where the shape is an emitter, else 0,
 *   19 s, 22 t of the frame (s, t, n), 25 wi = -d_dir in the frame, 28 wi taken back to the world;
 * d_flags: four int32 per lane -- the material's row (-1 at feature level 0, whose kernels read none), its type as the level
 * reads it, one-sided (0 / 1), emitter (0 / 1).
 * A lane whose shape is an emitter divides by the number of emitters, which is then at least 1: the scene's emitter list is made
 * from the same flags.  The shape numbers are read back and checked against the scene before a lane follows one; any float
 * input (NaN, infinities, the zero direction) is safe.  n = 0 does nothing; n > 2^20, a shape number outside
 * [0, shapes of the scene), a context without a scene and a NULL pointer are refused.  All pointers are device pointers.
 * Synchronises the stream (before reading the shape numbers back, and after the kernel). */
#define PG_SURFACE_PROBE_FLOATS 31
int pg_surface_probe(pg_context *ctx, uint64_t n, const int32_t *d_prim, const float *d_origin, const float *d_dir,
                     const float *d_t, const float *d_uv, const float *d_ref, float *d_out, int32_t *d_flags, void *stream);

/* The renderer's emitter sampling by itself, for tests: lane i samples the emitters of the scene set on the context from the
 * point d_p[3 i ..] whose geometric normal is d_n[3 i ..], with the 2-D sample d_e[2 i], d_e[2 i + 1], through the very device
 * function the render kernels call at every vertex (at the scene's feature level, with the scene's own emitter list --
 * flagged quads, then flagged spheres, then directional lights -- and bounding sphere), WITHOUT the visibility test: the
 * shadow ray is returned instead, for pg_scene_intersect(any_hit = 1) to cast.
 * d_out: PG_EMITTER_PROBE_FLOATS floats per lane --
 *   0 ds_d (unit direction to the light point), 3 ds_pdf (its solid-angle density times 1 / (number of emitters); a
 *   directional light: 1 / (number of emitters)), 4 em_weight = radiance / ds_pdf as if unoccluded, 7 sh_o, 10 sh_d, 13 sh_tmax:
 *   the shadow ray's origin, unit direction and the length within which any hit occludes;
 * d_flags: two int32 per lane -- ds_delta (1: a directional light was sampled), need_shadow (1: there is a shadow ray to cast).
 * A lane without a sample (a scene without emitters, a point inside a sphere light, a light that faces away) has ds_pdf = 0,
 * a zero weight and no shadow ray: sh_o = 0, sh_d = (0, 0, 1), sh_tmax = 0.
 * The samples are read back and checked before a lane uses one (the first picks the emitter); d_p and d_n may hold any
 * float (NaN, infinities, zeros).  n = 0 does nothing; n > 2^20, a sample that is NaN or outside [0, 1], a context without a
 * scene and a NULL pointer are refused.  All pointers are device pointers.  Synchronises the stream (before reading the
 * samples back, and after the kernel). */
#define PG_EMITTER_PROBE_FLOATS 14
int pg_emitter_probe(pg_context *ctx, uint64_t n, const float *d_p, const float *d_n, const float *d_e, float *d_out,
                     int32_t *d_flags, void *stream);

/* The renderer's bookkeeping of one path vertex by itself, for tests: lane i goes through the very device function the render
 * kernels call once a vertex's surface, emitter sample, BSDF sample and SD-tree answers are known (stage_b of
 * csrc/pg_render_stages.hpp) -- the emitter sample's MIS weight against the mixture pdf frac * bsdf + (1 - frac) * tree, the
 * radiance add, the BSDF re-evaluated at a direction the SD-tree proposed, woPdf and the BSDF weight it overwrites, the record
 * entry, ior, the throughput, Russian roulette and the spawned ray -- as a kernel of feature level `level` (0..3) runs it.
 * Needs no scene: what the earlier stages and the SD-tree give a vertex comes in as columns (pg_vertex_lanes; a 3-vector
 * column holds lane i at [3 i ..]), the material table as in pg_bsdf_probe (read only where PG_VERTEX_SMP_TREE is set, and
 * not at level 0, which takes the lane's reflectance as a two-sided diffuse material).
 * flags: the lane's class as the stages before set it -- */
#define PG_VERTEX_VALID 1u        /* the ray hit something; only such a lane is recorded */
#define PG_VERTEX_ACTIVE_NEXT 2u  /* the path may go on (depth + 1 < max_depth and valid) */
#define PG_VERTEX_DS_DELTA 16u    /* the emitter sample came from a delta light: MIS weight 1 at level 3 where it is live */
#define PG_VERTEX_DELTA 32u       /* the BSDF sample is a delta lobe (handed on in delta) */
#define PG_VERTEX_DO_MIS 64u      /* woPdf is the mixture, and the BSDF weight value / woPdf */
#define PG_VERTEX_SMP_TREE 128u   /* wo came from the SD-tree: the BSDF is evaluated at it */
#define PG_VERTEX_NEE_LIVE 512u   /* the emitter sample can contribute: em_w, bv_em, bp_em, ds_pdf are read */
#define PG_VERTEX_HAS_LE 1024u    /* emitted radiance reached the path here: Le is read */
/* (other bits are ignored.)  Call parameters: frac (the BSDF sampling fraction), guided (the mixture is in use), record and
 * store_nee (the record entry is written; it holds the emitter sample's luminance), rr_depth (roulette from that depth on). */
typedef struct pg_vertex_lanes {  /* device pointers, n lanes each */
	const float *thr, *L, *ior;            /* the path's state: float[3 n], float[3 n], float[n] */
	const uint32_t *depth, *flags;         /* uint32[n] each */
	const float *Le;                       /* float[3 n] */
	const float *p, *n, *ng, *wi, *refl;   /* float[3 n] each: the vertex, shading and geometric normal, -ray direction in the
	                                          shading frame, the reflectance the surface left (a texture's colour) */
	const int32_t *mat;                    /* int32[n]: row of the material table (checked on the host) */
	const float *em_w, *bv_em, *bp_em, *ds_pdf; /* float[3 n], float[3 n], float[n], float[n]: the emitter sample's radiance /
	                                          pdf as if unoccluded, the BSDF value and pdf towards it, its solid-angle density */
	const float *bsdf_w, *bsdf_pdf, *eta;  /* float[3 n], float[n], float[n]: the BSDF sample */
	const float *wo, *pdf_nee, *pdf_tree;  /* float[3 n], float[n], float[n]: the continuation direction (world), the SD-tree's
	                                          pdf of the emitter direction and of wo */
	const int32_t *occluded;               /* int32[n]: the shadow ray found an occluder */
	const uint64_t *rng_state, *rng_inc;   /* uint64[n] each: the lane's sampler, as pg_sample takes it */
} pg_vertex_lanes;
typedef struct pg_vertex_out {    /* device pointers */
	int32_t *go;                           /* int32[n]: 1 where the path continues */
	float *thr, *L, *ior, *ray_o, *ray_d, *prev_pdf; /* float[3 n], float[3 n], float[n], float[3 n], float[3 n], float[n]: the
	                                          state the next bounce reads (prev_pdf = woPdf) and the spawned ray */
	int32_t *delta;                        /* int32[n] */
	uint64_t *rng_state;                   /* uint64[n]: the sampler after the roulette's one draw */
	/* the record entry, planes of stride n (a channel c of lane i at [c n + i]): ray_of[i] = i, or 0xffffffff for a lane that
	 * is not valid, written when `record`; the others are written for a recorded lane only (record and PG_VERTEX_VALID) and
	 * keep what they held otherwise -- the BSDF weight, the throughput before it is multiplied, L after the add, the luminance
	 * of the emitter sample's share over the throughput (0 unless store_nee), woPdf */
	uint32_t *ray_of;
	float *r_bsdf, *r_tb, *r_tr, *r_nee, *r_wp; /* float[3 n], float[3 n], float[3 n], float[n], float[n] */
} pg_vertex_out;
/* Any float is safe in any column.  n = 0 does nothing; n > 2^20, a level outside 0..3, n_mat outside 1..65536, a table that
 * fails the material-row checks of pg_scene_set_ex, a row number outside the table and a NULL pointer (the structs', or any
 * of their members) are refused.  Synchronises the stream (before reading the table and the row numbers back, and after the
 * kernel). */
int pg_vertex_probe(pg_context *ctx, uint64_t n, uint64_t n_mat, const float *d_materials, int32_t level,
                    const pg_vertex_lanes *lanes, float frac, int32_t guided, int32_t record, int32_t store_nee, int32_t rr_depth,
                    const pg_vertex_out *out, void *stream);

/* The head of one path vertex by itself, for tests: lane i goes through the very device function the render kernels call
 * between the closest hit and the SD-tree calls (stage_a of csrc/pg_render_stages.hpp, that is stage_a1 then stage_a2) at the
 * scene's feature level -- the surface at the hit, wi, emitted radiance with its MIS weight against emitter sampling from the
 * previous vertex, active_next, the emitter sample and the BSDF towards it, the shadow ray, the BSDF sample, wo in the world
 * and the lane's class.  Needs a scene (pg_scene_set).  The lane's inputs are columns (pg_head_lanes; a 3-vector column
 * holds lane i at [3 i ..]): the ray, the path's throughput, the previous vertex with its BSDF pdf and delta flag, the hit as
 * pg_scene_intersect reports it (prim -1: a miss), the depth and the sampler.  The outputs are every field of the stage's
 * result; flags holds the lane's class, the eight bits PG_VERTEX_* above and */
#define PG_VERTEX_ACTIVE_EM 4u    /* emitter sampling happened and the sample's density is not zero */
#define PG_VERTEX_NEED_SHADOW 8u  /* em_w holds the unoccluded value: (sh_o, sh_d, sh_tmax) is to be cast */
#define PG_VERTEX_BSDF_MIS 256u   /* wo is the BSDF's, woPdf the mixture */
typedef struct pg_head_lanes {    /* device pointers, n lanes each */
	const float *ray_o, *ray_d, *thr, *prev_p; /* float[3 n] each */
	const float *prev_bsdf_pdf;            /* float[n] */
	const int32_t *prev_delta;             /* int32[n]: the previous vertex sampled a delta lobe (the camera counts as one) */
	const int32_t *prim;                   /* int32[n]: the shape hit, -1 for a miss (checked on the host) */
	const float *t, *uv;                   /* float[n], float[2 n] */
	const uint32_t *depth;                 /* uint32[n] */
	const uint64_t *rng_state, *rng_inc;   /* uint64[n] each: the lane's sampler, as pg_sample takes it */
} pg_head_lanes;
typedef struct pg_head_out {      /* device pointers */
	float *p, *n, *ng, *wi, *refl, *Le, *ds_d, *em_w, *bv_em, *sh_o, *sh_d, *wo, *bsdf_w; /* float[3 n] each */
	float *ds_pdf, *bp_em, *sh_tmax, *bsdf_pdf, *eta; /* float[n] each */
	int32_t *mat;                          /* int32[n]: the material row (0 at feature level 0 and for a miss) */
	uint32_t *flags;                       /* uint32[n] */
	uint64_t *rng_state;                   /* uint64[n]: the sampler after the head's draws (2, or 6 where PG_VERTEX_ACTIVE_NEXT) */
} pg_head_out;
/* Call parameters: max_depth (>= 1), frac (the BSDF sampling fraction), guided.  Any float is safe in any column.  n = 0 does
 * nothing; no scene, max_depth < 1, n > 2^20, a NULL pointer (the structs', or any of their members) and a shape number
 * outside [-1, shapes of the scene) are refused.  Synchronises the stream (before reading the shape numbers back, and after
 * the kernel). */
int pg_head_probe(pg_context *ctx, uint64_t n, const pg_head_lanes *lanes, int32_t max_depth, float frac, int32_t guided,
                  const pg_head_out *out, void *stream);

/* Per-kernel device time of pg_render_pass, measured with HIP events recorded on the launch
 * stream around each kernel (off by default).  pg_read_kernel_timing synchronises. */
typedef struct pg_kernel_timing {
	double bounce_ms, splat_ms, generate_ms, finish_ms, compact_ms;
	uint64_t bounce_launches, splat_launches, passes;
	/* mesh scenes run a bounce as two to five kernels (pg_render_stages: closest hits; then one shading kernel,
	 * or shading before and after the shadow rays with the SD-tree calls in the first, or those calls as a kernel
	 * of their own): their shares of bounce_ms; bounce_launches then counts bounces.  shade_ms = the shading
	 * kernels (pg_render_stages(0): the one, with shadow_ms = guide_ms = shade_b_ms = 0); tail_ms = the launch
	 * that finishes the last paths. */
	double trace_ms, shade_ms, shadow_ms, guide_ms, tail_ms;
	/* trace_launches counts the bounces' closest-hit passes: pg_render_stages(0) walks the camera rays inside the first
	 * shading launch, which is counted here and adds its whole time to shade_ms, none to trace_ms */
	uint64_t trace_launches, guide_launches;
	double shade_a_ms, shade_b_ms; /* the two shading kernels of shade_ms, each on its own */
	double sort_ms;                /* pg_render_sort: the radix sorts of the sorted bounces */
} pg_kernel_timing;
int pg_enable_kernel_timing(pg_context *ctx, int32_t on);
int pg_read_kernel_timing(pg_context *ctx, pg_kernel_timing *out, int32_t reset);

/* Paths still alive after each bounce of the most recent pg_render_pass: out[b] for
 * b < min(n, max_depth) (the loop condition `active` of path_guiding_integrator.py:179 counted
 * per iteration).  Synchronises the device. */
int pg_render_live_counts(pg_context *ctx, uint32_t *out, int32_t n);

/* ---- statistics for the roofline model ------------------------------------ */
typedef struct pg_stats {
	uint64_t n_kd_nodes, n_kd_leaves, n_quad_records, n_quad_nodes, n_trees;
	double mean_kd_leaf_depth;   /* over KD leaves                           */
	double mean_quad_leaf_depth; /* over quadtree leaves of all trees        */
	uint32_t max_kd_depth, max_quad_depth;
	uint64_t bytes_kd, bytes_quad_records, bytes_accumulators;
	/* the tables that stand in for the top levels of the descents (not in the reference): the quadtree jump tables
	 * (4^jump_bits entries of 16 bytes per quadtree; 0 bits: none -- the forest is too big for its memory budget,
	 * $PGSD_JUMP_TABLE_MAX_BYTES, default 2 GiB: a function of the forest and the budget alone, so that every rank and
	 * every run builds the same tables; coarser only when the table cannot be allocated) and the KD jump grid
	 * (8^kd_grid_bits cells of 16 bytes) */
	uint64_t bytes_jump_tables;
	uint32_t jump_bits, kd_grid_bits;
} pg_stats;
int pg_get_stats(pg_context *ctx, pg_stats *out);

/* Measured mean descent depths of the last pg_guide_bounce / pg_splat launch (device counters;
 * enabled by pg_enable_depth_counters(ctx, 1); off by default because they add atomics). */
typedef struct pg_depth_counters {
	uint64_t kd_levels, kd_queries;     /* sum of KD leaf depths, number of descents  */
	uint64_t quad_levels, quad_queries; /* sum of quadtree leaf depths, descents      */
	/* bytes the lanes of those descents gathered from the tables of the BUILT layout, nothing credited for lanes
	 * that share a cache line: 16 per KD grid entry and per KD node below it, 16 per jump-table entry, 32 per quadtree
	 * record of a pdf or sampling walk, 16 per record of a leaf walk (the 8-byte tree heads not included: add 8 per
	 * KD descent that is followed by a quadtree walk) */
	uint64_t layout_bytes;
} pg_depth_counters;
int pg_enable_depth_counters(pg_context *ctx, int32_t on);
int pg_read_depth_counters(pg_context *ctx, pg_depth_counters *out, int32_t reset);

/* Where a wave of k_wave_shade spends its life -- a PROBE BUILD's instrument (the library compiled with -DPG_SHADE_PHASES=1,
 * csrc/Makefile target `probe`: libpgsd_phases.so; the product build has no stamps, h_out[0] = 0 and zeros): the kernel that makes
 * the three SD-tree calls of a bounce (path_guiding_integrator.py:244, 301, 307) in the default pipeline also shades, walks the
 * shadow ray and appends the survivors, so the calls cannot be timed apart by events; the probe stamps the wave clock at the
 * kernel's start and at its seven phase boundaries (a wave's stamps wait in LDS and leave in one striped atomic: the probe's
 * kernel takes the product's time, profiles/r06/phase_probe.txt).  pg_enable_depth_counters(ctx, 2) switches the stamps on WITHOUT the depth counters (no atomics in the
 * walks themselves); pg_enable_depth_counters(ctx, 1) switches both on.  h_out[10]:
 *   [0] 1 when the stamps are compiled in, [1] waves that ran the kernel's body,
 *   [2..8] wave-clock cycles summed over those waves: records + staging, stage_a1, shadow walk, stage_a2, SD-tree calls,
 *          stage_b, survivors' append;  [9] 0. */
int pg_read_shade_phases(pg_context *ctx, uint64_t *h_out, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* PGSD_H */
