// pg_context.hpp -- host-side state of one pg_context (library-owned device memory).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pgsd.h"
#include "../../include/pgsd_fraction.h"
#include "../../include/ext/pg_lights.h"
#include "pg_kernels.hpp"
#include "pg_math.hpp"
#include "pg_tree.hpp"

namespace pg {

// Growable device array.  ensure() discards contents when it has to reallocate.  Growth is geometric where the caller
// asks for slack: a hipFree synchronises the whole device and a fresh hipMalloc of a gigabyte maps pages for tens of
// milliseconds, so a buffer that follows a growing tree must not be reallocated every time the tree grows a little
// (round 3's refine spent 20-190 ms per iteration there).
// Fault injection for the tests (pg_debug_fail_alloc, include/pgsd.h): when >= 0, the number of device allocations that still
// succeed -- the one after them reports hipErrorOutOfMemory exactly as a refused hipMalloc does (the buffer is left empty), and
// the hook disarms itself.  One variable for the whole library (C++17 inline variable); -1 = off.
inline long long g_alloc_fail_countdown = -1;

template <class T> struct DevBuf {
	T *p = nullptr;
	size_t cap = 0;
	~DevBuf() { release(); }
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	void release()
	{
		if (p) (void)hipFree(p);
		p = nullptr;
		cap = 0;
	}
	hipError_t ensure(size_t n, double slack = 1.0)
	{
		if (n <= cap) return hipSuccess;
		release();
		size_t want = (size_t)((double)n * slack);
		if (want < n) want = n;
		if (want < 16) want = 16;
		if (g_alloc_fail_countdown >= 0 && g_alloc_fail_countdown-- == 0) return hipErrorOutOfMemory; // (tests only; p is empty)
		hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
		if (e != hipSuccess) { p = nullptr; return e; }
		cap = want;
		return hipSuccess;
	}
	void swap(DevBuf &o)
	{
		T *tp = p; p = o.p; o.p = tp;
		size_t tc = cap; cap = o.cap; o.cap = tc;
	}
};

// ensure + copy: n elements of a host array become the contents of d
template <class T> hipError_t upload(DevBuf<T> &d, const T *h, size_t n, double slack = 1.0)
{
	hipError_t e = d.ensure(n, slack);
	if (e != hipSuccess || n == 0) return e;
	return hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice);
}
template <class T> hipError_t upload(DevBuf<T> &d, const std::vector<T> &h, double slack = 1.0) { return upload(d, h.data(), h.size(), slack); }

// One SD-tree topology + sampling values (sdTree_prev) + integer accumulators (sdTree_current).
// The two reference objects always share their topology (prev <- copy of current after every
// refine, path_guiding_integrator.py:582), so it is stored once.
struct Forest {
	// KD tree, reference node numbering
	DevBuf<KdNode> kd;
	DevBuf<float> kd_bmin, kd_bmax;  // [n_kd][3], kept for refine/export only
	DevBuf<float> kd_vcount;         // fp32 vertCount column of sdTree_prev (export only)
	uint32_t n_kd = 0;
	// quadtree forest
	DevBuf<QuadRec> rec;
	uint32_t n_rec = 0;
	std::vector<uint32_t> level_off; // level l records are [level_off[l], level_off[l+1])
	DevBuf<TreeHead> head;
	DevBuf<float> tree_thr;          // refinementThreshold of each tree (export only)
	uint32_t n_trees = 0;
	DevBuf<QuadJump> jump;           // n_trees << (2 * jump_bits) entries, rebuilt whenever rec/head change
	bool jump_valid = false;
	int jump_bits = 0;               // levels the tables of this forest cover (<= kJumpBits; what fits the memory budget)
	DevBuf<KdGridEntry> kd_grid;     // 8^kd_grid_bits cells + kKdGridRootEntries, rebuilt whenever the KD tree changes
	DevBuf<float> kd_planes;         // 3 * kKdGridPlanes cell boundaries (they follow the root box)
	bool kd_grid_valid = false;
	int kd_grid_bits = 0;            // cells per axis = 2^kd_grid_bits
	// accumulators of the running iteration: [rec_acc | root_acc | leaf_count]
	DevBuf<long long> acc;
	DevBuf<long long> xchg;          // the accumulators in their 24-byte exchange format (pg_exchange_pack): what travels
	uint64_t n_acc() const { return (uint64_t)n_rec * 4 + n_trees; }             // four-word accumulators
	uint64_t xchg_count() const { return n_acc() * kXchgWords + n_trees; }       // [n_acc x 3 | fallback counters]
	uint64_t acc_count() const
	{
		return (uint64_t)n_rec * 4 * kAccWords + (uint64_t)n_trees * kAccWords + n_trees;
	}
	// what a refine needs besides the forest itself: kept between refines (pg_refine.hip) so that a refine of a tree that
	// did not outgrow them allocates nothing
	struct RefineScratch {
		DevBuf<I128> tot;
		DevBuf<float> slot_irr, root_irr, new_thr;
		DevBuf<unsigned long long> kd_cnt, cnt_tot, tree_count, plan;
		DevBuf<uint32_t> tree_src, counts, cnt, pos, scan_sums, scan_total;
		DevBuf<TreeHead> new_head;
		DevBuf<QuadRec> new_rec;
		// the refined KD tree and the next iteration's accumulators are built HERE and become the forest's by a pointer swap
		// (pg_refine.hip: a refine is a transaction); what they replace becomes the next refine's scratch
		DevBuf<KdNode> new_kd;
		DevBuf<float> new_bmin, new_bmax, new_vc;
		DevBuf<long long> new_acc;
		DevBuf<unsigned char> pend_a, pend_b; // (Pending entries: the type lives in pg_refine.hip)
		void *pinned = nullptr;             // 64 bytes of page-locked host memory for the counters a refine reads back
		~RefineScratch() { if (pinned) (void)hipHostFree(pinned); }
	} scratch;
	AccumView accum_view()
	{
		AccumView a;
		a.rec_acc = acc.p;
		a.root_acc = acc.p + (uint64_t)n_rec * 4 * kAccWords;
		a.leaf_count = reinterpret_cast<unsigned long long *>(a.root_acc + (uint64_t)n_trees * kAccWords);
		return a;
	}
};

// The learned BSDF sampling fraction (include/pgsd_fraction.h, pg_kernels_fraction.hip): off unless pg_fraction_enable switched it
// on.  One table for the n_trees leaves of the forest, [ acc: n x kAccWords int64 | state: n x FracLeaf ], so that a refine
// builds the next one in ONE spare buffer and commits it by one pointer swap (pg_refine.hip).
struct alignas(32) FracLeaf {
	float theta, m, v, p1, p2;
	uint32_t steps;
	uint32_t pad[2];
};
static_assert(sizeof(FracLeaf) == 4 * sizeof(long long), "a leaf's state is four words of the table");
constexpr size_t kFracWords = kAccWords + sizeof(FracLeaf) / sizeof(long long); // words of the table per leaf
struct Fraction {
	bool on = false;
	pg_fraction_params prm = {};
	DevBuf<long long> tab, spare; // spare: the next refine's table (what a commit replaced)
	long long *acc() const { return tab.p; }
	FracLeaf *leaves(uint32_t n_trees) const { return reinterpret_cast<FracLeaf *>(tab.p + (size_t)n_trees * kAccWords); }
	void disable()
	{
		on = false;
		tab.release();
		spare.release();
	}
};

// Light selection learned per KD leaf (include/ext/pg_lights.h, pg_kernels_lights.hip): off unless pg_lights_enable switched it
// on.  One table for the n_trees leaves and L = n_lights lights, [ acc: n x L x kAccWords int64 | rows: n x L uint32 ], so that a
// refine builds the next one in ONE spare buffer and commits it by one pointer swap (pg_refine.hip).
constexpr uint64_t kLightsMaxEntries = 1ull << 31; // n_trees * n_lights: a record's key (tree * L + light) is a uint32
struct Lights {
	uint32_t n_lights = 0; // 0: the feature is off
	pg_lights_params prm = {};
	DevBuf<long long> tab, spare; // spare: the next refine's table (what a commit replaced)
	bool on() const { return n_lights != 0; }
	static size_t words(uint64_t entries) { return (size_t)(entries * kAccWords + (entries + 1) / 2); }
	long long *acc() const { return tab.p; }
	uint32_t *rows(uint32_t n_trees) const { return rows_of(tab.p, n_trees, n_lights); }
	static uint32_t *rows_of(long long *tab, uint32_t n_trees, uint32_t n_lights)
	{
		return reinterpret_cast<uint32_t *>(tab + (size_t)n_trees * n_lights * kAccWords);
	}
	void disable()
	{
		n_lights = 0;
		tab.release();
		spare.release();
	}
};

// The lights' geometry for the resampled next-event estimation (include/ext/lights/pg_nee.h, pg_kernels_nee.hip): nothing unless
// pg_nee_set_lights gave a table.  One 64-byte record per light, what k_nee_prepare made of the host's twelve words; a candidate
// gathers one whole record.  It belongs to the context, not to the tree: setup, import and a refine leave it alone.
struct alignas(64) NeeLight {
	float o[3], a[3], b[3], N[3];
	float invA, radiance;
	uint32_t kind, two_sided;
};
static_assert(sizeof(NeeLight) == 64, "a light's record is one 64-byte line");
struct Nee {
	uint32_t n_lights = 0; // 0: no table
	DevBuf<NeeLight> tab;
	void release()
	{
		n_lights = 0;
		tab.release();
	}
};

// Radiance estimates (include/pgsd_radiance.h, pg_kernels_radiance.hip): off unless pg_radiance_enable switched it on.  One uint64
// per quadtree of sdTree_prev, the number of in-box records its energies were resolved from; a refine builds the next table in the
// spare buffer and commits it, with the two flags, by one pointer swap (pg_refine.hip).
// Irradiance estimates (include/pgsd_irradiance.h, pg_kernels_irradiance.hip): nothing unless pg_irradiance_build /
// pg_irradiance_import ran.  The projection of every quadtree of sdTree_prev onto the nine spherical harmonics up to order 2,
// kIrrStride floats per tree (nine coefficients, padded to three 16-byte gathers).  It lives with the weights it was projected
// with: whatever replaces them or the tree clears `built`.
constexpr uint32_t kIrrCoeffs = 9, kIrrStride = 12;
struct Irradiance {
	int32_t built = 0;
	DevBuf<float> tab;      // [n_trees][kIrrStride]
	DevBuf<long long> sums; // [n_trees][kIrrCoeffs]: the build's exact sums, kept between builds
	DevBuf<uint4> cells;    // one per quadtree record: (tree, ix, iy, depth) of the node's cell, kept between builds
	void release()
	{
		built = 0;
		tab.release();
		sums.release();
		cells.release();
	}
};

struct Radiance {
	bool on = false;
	int32_t valid = 0;     // the table describes sdTree_prev (a refine committed it, or pg_radiance_import loaded it)
	int32_t of_target = 0; // pg_target_applied at the refine that built sdTree_prev: its energies are not radiance
	DevBuf<unsigned long long> tab, spare; // spare: the next refine's table (what a commit replaced)
	Irradiance irr;        // built from tab and sdTree_prev on request
	void disable()
	{
		on = false;
		valid = 0;
		of_target = 0;
		tab.release();
		spare.release();
		irr.release();
	}
};

} // namespace pg

struct pg_render_state; // pg_render.hip (its scene: pg_scene_state.hpp)
struct pg_rr_params;    // include/pgsd_radiance.h
namespace pg {
struct RrArgs;          // pg_guide_dev.hpp
struct RisConsts;       // pg_ris_dev.hpp
}
struct pg_resample_params; // include/pg_resample.h

struct pg_context {
	pg_render_state *render = nullptr;
	int device = 0;
	int n_cus = 256; // compute units of the device (sizes the persistent grids)
	std::string err;
	bool configured = false;
	float bmin[3] = {0, 0, 0}, bmax[3] = {1, 1, 1};
	uint64_t num_rays = 0;
	int32_t max_depth = 0, kd_max_depth = 10, quad_max_depth = 30, store_nee = 1;
	float bsdf_fraction = 0.5f;
	int32_t iteration = 0, is_final = 0;
	int32_t filter_spatial = 0, filter_directional = 0; // pg_set_splat_filter: PG_SPATIAL_* / PG_DIRECTIONAL_*
	uint32_t filter_seed = 0;
	double kd_max_leaf_size = 1.0;
	pg::Forest f;
	pg::Fraction frac;               // the learned sampling fraction (disabled by pg_setup / pg_import)
	pg::Radiance rad;                // the quadtrees' statistical weights (disabled by pg_setup / pg_import)
	pg::Lights lights;               // the learned light selection (disabled by pg_setup / pg_import)
	pg::Nee nee;                     // the lights' geometry of pg_nee_resample (kept by pg_setup / pg_import / a refine)
	int32_t target_applied = 0;      // the target pg_target_apply gave f.acc since the last refine commit / setup / import (pgsd_target.h)
	pg::DepthCounters *dc = nullptr; // device
	bool dc_on = false;
	bool ph_on = false;              // a probe build's phase stamps are on (pg_enable_depth_counters 1 or 2; never in the product build)
	pg::DevBuf<unsigned long long> ph_buf; // their striped counters (kPhaseStripes x kPhaseWords), allocated by the first enable of a probe build
	// memory budget of the quadtree jump tables (bytes): $PGSD_JUMP_TABLE_MAX_BYTES at pg_create, default 2 GiB.  The resolution a
	// forest gets follows from the forest and this budget alone (pg_refine.hip: rebuild_jump)
	uint64_t jump_budget = 2ull << 30;
	void *comm = nullptr;            // ncclComm_t of the multi-GPU exchange (pg_comm.hip)
	bool comm_owned = false;         // made by pg_comm_init (destroyed with the context) or attached by the caller
	int comm_ranks = 0;

	pg::TreeView view() const
	{
		pg::TreeView t;
		t.kd = f.kd.p;
		t.rec = f.rec.p;
		t.head = f.head.p;
		t.jump.p = f.jump_valid ? f.jump.p : nullptr;
		t.jump.bits = f.jump_valid ? f.jump_bits : 0;
		t.kd_grid = f.kd_grid_valid ? f.kd_grid.p : nullptr;
		t.kd_planes = f.kd_planes.p;
		for (int a = 0; a < 3; ++a) {
			t.bmin[a] = bmin[a]; t.bmax[a] = bmax[a];
			t.grid_inv[a] = (float)(1 << f.kd_grid_bits) / (bmax[a] - bmin[a]);
		}
		t.grid_bits = f.kd_grid_bits;
		t.n_kd = f.n_kd;
		t.n_rec = f.n_rec;
		t.n_trees = f.n_trees;
		return t;
	}
	bool filtered() const { return filter_spatial != PG_SPATIAL_NEAREST || filter_directional != PG_DIRECTIONAL_NEAREST; }
	// The filtered kernels' arguments.  (On the initial tree -- one KD leaf owning a single-leaf quadtree -- every filter is the
	// nearest deposit bit for bit, and the callers run the nearest kernels, with their one-accumulator fast path.)
	pg::pg_filter_args filter_args() const
	{
		pg::pg_filter_args a;
		a.spatial = filter_spatial;
		a.directional = filter_directional;
		a.seed = filter_seed;
		a.kd_bmin = f.kd_bmin.p;
		a.kd_bmax = f.kd_bmax.p;
		return a;
	}
	bool filtered_launch() const { return filtered() && !(f.n_rec == 0 && f.n_trees == 1); }
};

namespace pg {
// pg_refine.hip
int refine_and_swap(pg_context *ctx, hipStream_t s);
int rebuild_jump(pg_context *ctx, hipStream_t s); // after every change of the quadtree records or heads
// pg_kernels_fraction.hip: the table of the refined forest -- new leaf t takes the state of old leaf tree_src[t], zero accumulators
void launch_fraction_carry(const long long *old_tab, uint32_t n_old, const uint32_t *tree_src, long long *new_tab, uint32_t n_new,
                           hipStream_t s);
// pg_kernels_lights.hip: the table of the refined forest -- new leaf t takes the row of old leaf tree_src[t], zero accumulators
hipError_t launch_lights_carry(long long *old_tab, uint32_t n_old, const uint32_t *tree_src, long long *new_tab, uint32_t n_new,
                               uint32_t n_lights, int n_cus, hipStream_t s);
// pg_kernels_radiance.hip: the weights of the refined forest -- new tree t takes the count resolved for old tree tree_src[t]
void launch_radiance_carry(const unsigned long long *tree_count, uint32_t n_old, const uint32_t *tree_src, unsigned long long *w_new,
                           uint32_t n_new, hipStream_t s);
// the host checks the calls on the estimates share (pg_radiance_query / _rr, pg_irradiance_build / _import, pg_bounce), each
// PG_OK or the refusal with `who` in front: radiance is enabled, its weights are known, the tree is not a second-moment tree;
int radiance_source(pg_context *ctx, const char *who);
// and pg_rr_params are valid, which fills the window (lo, hi) and the split limit (max_split, max_split_f) of rr
int rr_window(pg_context *ctx, const char *who, const pg_rr_params *params, RrArgs &rr);
// pg_kernels_resample.hip: the host checks the resampled calls share (pg_resample_cosine / _lobe / _interface, pg_nee_resample),
// each PG_OK or the refusal with `who` in front: candidates lies in 1..64; n fits 32 bits;
int resample_candidates(pg_context *ctx, const char *who, uint32_t candidates);
int resample_lanes(pg_context *ctx, const char *who, uint64_t n);
// and all the refusals of pg_resample_params in the order of include/pg_resample.h (candidates, alpha, delta, reserved, n), which
// fills the kernels' constants c
int resample_consts(pg_context *ctx, const char *who, uint64_t n, const pg_resample_params &prm, RisConsts &c);
// pg_render.hip
void destroy_render_state(pg_context *ctx);
// pg_render_wave.hip
bool shade_phases_compiled_in();
// pg_comm.hip
void destroy_comm(pg_context *ctx);
// pg_sort.hip
size_t sort_pairs_temp_bytes(uint32_t n);
hipError_t sort_places16(void *temp, size_t temp_bytes, const uint16_t *keys_in, uint16_t *keys_out, uint32_t *places_out, uint32_t n,
                         const uint32_t *d_live, hipStream_t s);
// helpers shared by pg_context.hip / pg_refine.hip
int fail(pg_context *ctx, int code, const std::string &msg);
int hip_fail(pg_context *ctx, hipError_t e, const char *what);
} // namespace pg

#define PG_HIP(ctx, call)                                                      \
	do {                                                                       \
		hipError_t e__ = (call);                                               \
		if (e__ != hipSuccess) return pg::hip_fail((ctx), e__, #call);        \
	} while (0)

// what every query / recording entry point does before it launches, and behind the launch (pg_context.hip, pg_kernels_warp.hip)
#define PG_READY(ctx)                                                                  \
	do {                                                                               \
		if (!(ctx)) return PG_ERR_INVALID;                                             \
		if (!(ctx)->configured) return pg::fail((ctx), PG_ERR_INVALID, "call pg_setup or pg_import first"); \
		PG_HIP((ctx), hipSetDevice((ctx)->device));                                    \
	} while (0)

#define PG_LAUNCHED(ctx)                                                               \
	do {                                                                               \
		hipError_t e__ = hipGetLastError();                                            \
		if (e__ != hipSuccess) return pg::hip_fail((ctx), e__, "kernel launch");      \
	} while (0)
