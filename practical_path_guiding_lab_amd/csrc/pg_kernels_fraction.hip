// pg_kernels_fraction.hip -- the BSDF sampling fraction learned per KD leaf (include/pgsd_fraction.h, which states the semantics
// operation by operation): the query, the gradient record, the Adam step, the refine's carry, and the seven
// entry points.  wave64, 256-thread groups.
//
// The default kernels are not touched (a shared body moved a default kernel's code once): the kernels here use
// the descent of pg_descent.hpp and the quantisation of pg_math.hpp as they are.
//
// k_fraction_record is the one that matters.  Spatially coherent records put most of a wave -- on the initial tree all of it --
// into ONE leaf, whose accumulator is one 32-byte sector: an atomic per lane and word would queue on it.  So the sums are merged
// before they leave the CU, in three stages, all of them exact 64-bit integer adds (any order gives the same words):
//   1. the wave: lanes are matched by tree number (a ballot against the lowest pending lane's tree, up to kWaveRounds distinct
//      trees), and a matched group's four words are summed across the lanes with shuffles -- no memory at all;
//   2. the workgroup: group leaders and unmatched lanes add into a hash table in LDS keyed by tree (LDS atomics);
//   3. the device: behind the block's last tile, four adjacent lanes send a table entry's four words in one wave-instruction:
//      one sector update per distinct leaf of the WORKGROUP (a persistent block takes many tiles).
// Limb discipline: a limb's payload is below 2^32 per record, and every partial sum here lives in a 64-bit word
// exactly like the accumulator itself -- a wave's sum stays below 2^38, a block's below 2^32 * (its records) -- so what reaches
// the accumulator is the same integer per word as record-by-record adds would leave, and the 2^31-record bound is unchanged.
// (k_lights_record, lights_table_add and lights_wave_sum_u64 of pg_kernels_lights.hip are copies of the three stages below with
// another key: a fix to one belongs in the other.)
#include "../../include/pgsd_fraction.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_guide_dev.hpp"

#include <cmath>
#include <vector>

namespace pg {

constexpr float kThetaMax = PG_FRACTION_THETA_MAX;

// logistic_f32 (the logistic of pgsd_fraction.h): pg_guide_dev.hpp -- pg_kernels_bounce.hip inlines it too
__device__ __forceinline__ float load_theta(const FracLeaf *leaves, uint32_t tree) { return leaves[tree].theta; }

// ---- query -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kQueryBlock) void k_fraction_query(TreeView t, const FracLeaf *__restrict__ leaves, float theta0,
                                                            uint64_t n, const float *__restrict__ p,
                                                            const uint8_t *__restrict__ active,
                                                            float *__restrict__ fraction_out)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = active ? active[i] != 0 : true;
	float theta = theta0;
	if (act) {
		const float x = p[i], y = p[n + i], z = p[2 * n + i];
		if (inside_root(t, x, y, z)) {
			KdNode leaf;
			uint32_t kd_lv;
			kd_descend_grid(t, s_planes, x, y, z, true, leaf, kd_lv);
			theta = load_theta(leaves, leaf.tree);
		}
	}
	fraction_out[i] = logistic_f32(theta);
}

// ---- record ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t kNoTree = 0xffffffffu;
constexpr int kWaveRounds = 4;     // distinct trees of a wave merged in registers; the rest go to the table lane by lane
constexpr int kTableSlots = 512;   // LDS hash table of the workgroup: tree -> four words
constexpr int kProbes = 4;         // linear probes before a lane gives up on the table and adds to the device itself
constexpr unsigned kRecordGroupsPerCu = 8;
static_assert((kTableSlots & (kTableSlots - 1)) == 0 && kTableSlots % (kQueryBlock / 4) == 0, "the flush takes 64 slots per pass");

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// RECORD of pgsd_fraction.h for one record: keep test and gradient.  Returns the record's tree, kNoTree when it is dropped.
__device__ __forceinline__ uint32_t record_gradient(const TreeView &t, const float *s_planes, const FracLeaf *leaves, int loss,
                                                    float x, float y, float z, float bsdf_pdf, float guide_pdf, float product,
                                                    float wo_pdf, bool delta, Limbs &q)
{
	q.l0 = q.l1 = q.l2 = 0;
	const bool fin = finite_f32(bsdf_pdf) && finite_f32(guide_pdf) && finite_f32(product) && finite_f32(wo_pdf);
	if (delta || !inside_root(t, x, y, z) || !fin || !(wo_pdf > 0.0f)) return kNoTree;
	KdNode leaf;
	uint32_t lv;
	kd_descend_grid(t, s_planes, x, y, z, true, leaf, lv);
	const float f = logistic_f32(load_theta(leaves, leaf.tree));
	const float omf = 1.0f - f;
	const float mix = (f * bsdf_pdf) + (omf * guide_pdf);
	if (!(mix > 0.0f)) return kNoTree;
	float r = product / mix;
	if (loss == PG_FRACTION_LOSS_VARIANCE) r = r * r;
	const float dLdf = ((0.0f - r) / wo_pdf) * (bsdf_pdf - guide_pdf);
	const float g = dLdf * (f * omf);
	q = quantize_weight(g);
	return leaf.tree;
}

// stage 2: (tree, w) into the workgroup's table; a lane that finds no slot within kProbes adds to the device itself
__device__ __forceinline__ void table_add(uint32_t *s_key, unsigned long long *s_val, long long *acc, uint32_t tree,
                                          const unsigned long long (&w)[4])
{
	uint32_t h = (tree * 0x9e3779b1u) >> 23; // (top 9 bits: kTableSlots = 512)
	static_assert(kTableSlots == 512, "the hash takes nine bits");
	bool placed = false;
#pragma unroll
	for (int k = 0; k < kProbes; ++k) {
		if (!placed) {
			const uint32_t prev = atomicCAS(&s_key[h], kNoTree, tree);
			if (prev == kNoTree || prev == tree) placed = true;
			else h = (h + 1u) & (kTableSlots - 1);
		}
	}
	if (placed) { // (two branches, two address spaces: no pointer that is "LDS or device")
#pragma unroll
		for (int k = 0; k < 4; ++k)
			if (w[k]) atomicAdd(s_val + 4 * h + k, w[k]);
	} else {
		unsigned long long *dst = reinterpret_cast<unsigned long long *>(acc + (size_t)kAccWords * tree);
#pragma unroll
		for (int k = 0; k < 4; ++k)
			if (w[k]) atomicAdd(dst + k, w[k]);
	}
}

__global__ __launch_bounds__(kQueryBlock) void k_fraction_record(TreeView t, const FracLeaf *__restrict__ leaves,
                                                             long long *__restrict__ acc, int loss, uint64_t m,
                                                             pg_fraction_records r, const uint32_t *__restrict__ d_count)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	__shared__ uint32_t s_key[kTableSlots];
	__shared__ unsigned long long s_val[kTableSlots * 4];
	for (int k = threadIdx.x; k < kTableSlots; k += kQueryBlock) s_key[k] = kNoTree;
	for (int k = threadIdx.x; k < kTableSlots * 4; k += kQueryBlock) s_val[k] = 0ull;
	stage_kd_planes(s_planes, t); // (holds the barrier behind the table's initialisation)
	uint64_t valid = d_count ? (uint64_t)*d_count : m; // plane stride stays m
	if (valid > m) valid = m;
	const uint64_t tiles = (valid + kQueryBlock - 1) / kQueryBlock;
	const unsigned lane = threadIdx.x & 63u;
	for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (uniform over the workgroup)
		const uint64_t i = tile * kQueryBlock + threadIdx.x;
		uint32_t tree = kNoTree;
		Limbs q = {0, 0, 0};
		if (i < valid) {
			const bool delta = r.is_delta ? r.is_delta[i] != 0 : false;
			tree = record_gradient(t, s_planes, leaves, loss, r.position[i], r.position[m + i], r.position[2 * m + i], r.bsdf_pdf[i],
			                       r.guide_pdf[i], r.product[i], r.wo_pdf[i], delta, q);
		}
		unsigned long long w[4] = {(unsigned long long)q.l0, (unsigned long long)q.l1, (unsigned long long)q.l2,
		                           tree != kNoTree ? 1ull : 0ull};
		// stage 1: the wave's lanes matched by tree.  `pending` lanes still hold a record nobody has taken over.
		bool pending = tree != kNoTree;
#pragma unroll 1
		for (int round = 0; round < kWaveRounds; ++round) {
			const unsigned long long pend = __ballot(pending);
			if (pend == 0) break; // (uniform over the wave)
			const int lead = __builtin_ctzll(pend);
			const uint32_t lead_tree = (uint32_t)__shfl((int)tree, lead, 64);
			const bool peer = pending && tree == lead_tree;
			const unsigned long long peers = __ballot(peer);
			if (peers != (1ull << lead)) { // more than the leader: sum the group's words across the wave
				unsigned long long s[4];
#pragma unroll
				for (int k = 0; k < 4; ++k) s[k] = wave_sum_u64(peer ? w[k] : 0ull);
				if (peer) {
#pragma unroll
					for (int k = 0; k < 4; ++k) w[k] = lane == (unsigned)lead ? s[k] : 0ull;
					if (lane != (unsigned)lead) tree = kNoTree; // (taken over by the leader)
				}
			}
			if (peer) {
				pending = false;
				if (tree != kNoTree) table_add(s_key, s_val, acc, tree, w); // the group's leader
			}
		}
		if (pending) table_add(s_key, s_val, acc, tree, w); // a wave of many leaves: lane by lane
	}
	// stage 3: the table leaves the CU, four adjacent lanes per entry -- one sector update per distinct leaf of the workgroup
	__syncthreads();
	const unsigned word = threadIdx.x & 3u;
#pragma unroll 1
	for (int base = 0; base < kTableSlots; base += kQueryBlock / 4) {
		const int slot = base + (int)(threadIdx.x >> 2);
		const uint32_t key = s_key[slot];
		const unsigned long long v = s_val[4 * slot + word];
		if (key != kNoTree && v != 0ull)
			atomicAdd(reinterpret_cast<unsigned long long *>(acc + (size_t)kAccWords * key + word), v);
	}
}

// ---- step ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kQueryBlock) void k_fraction_step(FracLeaf *__restrict__ leaves, long long *__restrict__ acc,
                                                           uint32_t n_trees, pg_fraction_params prm)
{
	const uint32_t t = blockIdx.x * kQueryBlock + threadIdx.x;
	if (t >= n_trees) return;
	long long *a = acc + (size_t)kAccWords * t;
	const long long count = a[3];
	if (count <= 0) return;
	FracLeaf s = leaves[t];
	float g = i128_to_f32(limbs_resolve(a[0], a[1], a[2])) / (float)count;
	g = g + prm.l2 * s.theta;
	s.m = prm.beta1 * s.m + (1.0f - prm.beta1) * g;
	s.v = prm.beta2 * s.v + (1.0f - prm.beta2) * (g * g);
	s.p1 = s.p1 * prm.beta1;
	s.p2 = s.p2 * prm.beta2;
	s.steps = s.steps + 1u;
	const float step = prm.learning_rate * (__builtin_sqrtf(1.0f - s.p2) / (1.0f - s.p1));
	float theta = s.theta - step * (s.m / (__builtin_sqrtf(s.v) + prm.epsilon));
	theta = theta < -kThetaMax ? -kThetaMax : (theta > kThetaMax ? kThetaMax : theta);
	s.theta = theta;
	leaves[t] = s;
	a[0] = 0; a[1] = 0; a[2] = 0; a[3] = 0;
}

// ---- tables ----------------------------------------------------------------------------------------------------------------
// every leaf at its start values, zero accumulators (pg_fraction_enable)
__global__ __launch_bounds__(kQueryBlock) void k_fraction_init(long long *__restrict__ tab, uint32_t n_trees, float theta0)
{
	const uint32_t t = blockIdx.x * kQueryBlock + threadIdx.x;
	if (t >= n_trees) return;
	long long *a = tab + (size_t)kAccWords * t;
	a[0] = 0; a[1] = 0; a[2] = 0; a[3] = 0;
	FracLeaf s;
	s.theta = theta0; s.m = 0.0f; s.v = 0.0f; s.p1 = 1.0f; s.p2 = 1.0f; s.steps = 0u; s.pad[0] = 0u; s.pad[1] = 0u;
	reinterpret_cast<FracLeaf *>(tab + (size_t)n_trees * kAccWords)[t] = s;
}

// the table of a refined forest: new leaf t is a copy of old leaf tree_src[t] (pg_refine.hip), its accumulator zero
__global__ __launch_bounds__(kQueryBlock) void k_fraction_carry(const long long *__restrict__ old_tab, uint32_t n_old,
                                                            const uint32_t *__restrict__ tree_src,
                                                            long long *__restrict__ new_tab, uint32_t n_new)
{
	const uint32_t t = blockIdx.x * kQueryBlock + threadIdx.x;
	if (t >= n_new) return;
	long long *a = new_tab + (size_t)kAccWords * t;
	a[0] = 0; a[1] = 0; a[2] = 0; a[3] = 0;
	uint32_t src = tree_src[t];
	if (src >= n_old) src = 0; // (never: tree_src names pre-refine trees)
	reinterpret_cast<FracLeaf *>(new_tab + (size_t)n_new * kAccWords)[t] =
	    reinterpret_cast<const FracLeaf *>(old_tab + (size_t)n_old * kAccWords)[src];
}

void launch_fraction_carry(const long long *old_tab, uint32_t n_old, const uint32_t *tree_src, long long *new_tab, uint32_t n_new,
                           hipStream_t s)
{
	if (n_new == 0) return;
	hipLaunchKernelGGL(k_fraction_carry, query_grid(n_new), dim3(kQueryBlock), 0, s, old_tab, n_old, tree_src, new_tab, n_new);
}

static bool params_ok(const pg_fraction_params &p)
{
	return std::isfinite(p.theta0) && std::fabs(p.theta0) <= kThetaMax && std::isfinite(p.learning_rate) && p.learning_rate > 0.0f &&
	       p.beta1 >= 0.0f && p.beta1 < 1.0f && p.beta2 >= 0.0f && p.beta2 < 1.0f && std::isfinite(p.epsilon) && p.epsilon > 0.0f &&
	       std::isfinite(p.l2) && p.l2 >= 0.0f && (p.loss == PG_FRACTION_LOSS_KL || p.loss == PG_FRACTION_LOSS_VARIANCE);
}

} // namespace pg

using namespace pg;

// PG_READY, and the feature is on
#define PG_FRACTION_ON(ctx, who)                                                                              \
	do {                                                                                                      \
		PG_READY(ctx);                                                                                        \
		if (!(ctx)->frac.on) return fail((ctx), PG_ERR_INVALID, who ": call pg_fraction_enable first");      \
	} while (0)

extern "C" {

int pg_fraction_enable(pg_context *ctx, const pg_fraction_params *params)
{
	PG_READY(ctx);
	if (!params) {
		PG_HIP(ctx, hipDeviceSynchronize()); // (kernels that read the table have finished)
		ctx->frac.disable();
		return PG_OK;
	}
	if (!params_ok(*params)) return fail(ctx, PG_ERR_INVALID, "pg_fraction_enable: parameter out of range (pgsd_fraction.h)");
	Fraction &fr = ctx->frac;
	const uint32_t n = ctx->f.n_trees;
	PG_HIP(ctx, hipDeviceSynchronize());
	hipError_t e = fr.tab.ensure((size_t)n * kFracWords);
	if (e != hipSuccess) {
		fr.disable();
		return hip_fail(ctx, e, "pg_fraction_enable: table");
	}
	hipLaunchKernelGGL(k_fraction_init, query_grid(n), dim3(kQueryBlock), 0, nullptr, fr.tab.p, n, params->theta0);
	PG_LAUNCHED(ctx);
	PG_HIP(ctx, hipDeviceSynchronize());
	fr.prm = *params;
	fr.on = true;
	return PG_OK;
}

int pg_fraction_query(pg_context *ctx, uint64_t n, const float *p, const uint8_t *active, float *fraction_out, void *stream)
{
	PG_FRACTION_ON(ctx, "pg_fraction_query");
	if (n && (!p || !fraction_out)) return fail(ctx, PG_ERR_INVALID, "pg_fraction_query: NULL pointer");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_fraction_query: too many lanes for one launch");
	if (n == 0) return PG_OK;
	hipLaunchKernelGGL(k_fraction_query, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(),
	                   ctx->frac.leaves(ctx->f.n_trees), ctx->frac.prm.theta0, n, p, active, fraction_out);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_fraction_record(pg_context *ctx, uint64_t m, const pg_fraction_records *rec, const uint32_t *d_count, void *stream)
{
	PG_FRACTION_ON(ctx, "pg_fraction_record");
	if (!rec) return fail(ctx, PG_ERR_INVALID, "pg_fraction_record: NULL records");
	if (m && (!rec->position || !rec->bsdf_pdf || !rec->guide_pdf || !rec->product || !rec->wo_pdf))
		return fail(ctx, PG_ERR_INVALID, "pg_fraction_record: NULL record column");
	if (m >= 0xffffffffull) return fail(ctx, PG_ERR_INVALID, "pg_fraction_record: more than 2^32 - 1 records in one call");
	if (m == 0) return PG_OK;
	// a persistent grid: a block merges all its tiles in LDS before it sends a leaf's sum out
	const uint64_t tiles = (m + kQueryBlock - 1) / kQueryBlock, cap = (uint64_t)ctx->n_cus * kRecordGroupsPerCu;
	hipLaunchKernelGGL(k_fraction_record, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(kQueryBlock), 0, (hipStream_t)stream,
	                   ctx->view(), ctx->frac.leaves(ctx->f.n_trees), ctx->frac.acc(), (int)ctx->frac.prm.loss, m, *rec, d_count);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_fraction_step(pg_context *ctx, void *stream)
{
	PG_FRACTION_ON(ctx, "pg_fraction_step");
	const uint32_t n = ctx->f.n_trees;
	hipLaunchKernelGGL(k_fraction_step, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->frac.leaves(n), ctx->frac.acc(), n,
	                   ctx->frac.prm);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_fraction_accumulators(pg_context *ctx, int64_t **d_buffer, uint64_t *count)
{
	PG_FRACTION_ON(ctx, "pg_fraction_accumulators");
	if (!d_buffer || !count) return fail(ctx, PG_ERR_INVALID, "pg_fraction_accumulators: NULL pointer");
	*d_buffer = reinterpret_cast<int64_t *>(ctx->frac.acc());
	*count = (uint64_t)ctx->f.n_trees * kAccWords;
	return PG_OK;
}

int pg_fraction_export(pg_context *ctx, uint64_t n_trees, float *h_theta, float *h_m, float *h_v, float *h_p1, float *h_p2,
                       uint32_t *h_steps, int64_t *h_acc)
{
	PG_FRACTION_ON(ctx, "pg_fraction_export");
	if (n_trees != ctx->f.n_trees) return fail(ctx, PG_ERR_INVALID, "pg_fraction_export: n_trees does not match pg_export_sizes' n_roots");
	if (!h_theta || !h_m || !h_v || !h_p1 || !h_p2 || !h_steps) return fail(ctx, PG_ERR_INVALID, "pg_fraction_export: NULL pointer");
	PG_HIP(ctx, hipDeviceSynchronize());
	std::vector<long long> tab((size_t)n_trees * kFracWords);
	PG_HIP(ctx, hipMemcpy(tab.data(), ctx->frac.tab.p, tab.size() * sizeof(long long), hipMemcpyDeviceToHost));
	const FracLeaf *s = reinterpret_cast<const FracLeaf *>(tab.data() + (size_t)n_trees * kAccWords);
	for (uint64_t t = 0; t < n_trees; ++t) {
		h_theta[t] = s[t].theta; h_m[t] = s[t].m; h_v[t] = s[t].v; h_p1[t] = s[t].p1; h_p2[t] = s[t].p2; h_steps[t] = s[t].steps;
	}
	if (h_acc)
		for (uint64_t k = 0; k < n_trees * kAccWords; ++k) h_acc[k] = (int64_t)tab[k];
	return PG_OK;
}

int pg_fraction_import(pg_context *ctx, uint64_t n_trees, const float *h_theta, const float *h_m, const float *h_v,
                       const float *h_p1, const float *h_p2, const uint32_t *h_steps)
{
	PG_FRACTION_ON(ctx, "pg_fraction_import");
	if (n_trees != ctx->f.n_trees) return fail(ctx, PG_ERR_INVALID, "pg_fraction_import: n_trees does not match pg_export_sizes' n_roots");
	if (!h_theta || !h_m || !h_v || !h_p1 || !h_p2 || !h_steps) return fail(ctx, PG_ERR_INVALID, "pg_fraction_import: NULL pointer");
	std::vector<long long> tab((size_t)n_trees * kFracWords, 0ll); // (zero accumulators)
	FracLeaf *s = reinterpret_cast<FracLeaf *>(tab.data() + (size_t)n_trees * kAccWords);
	for (uint64_t t = 0; t < n_trees; ++t) {
		if (!(std::isfinite(h_theta[t]) && std::isfinite(h_m[t]) && std::isfinite(h_v[t]) && std::isfinite(h_p1[t]) && std::isfinite(h_p2[t])))
			return fail(ctx, PG_ERR_INVALID, "pg_fraction_import: non-finite value");
		if (std::fabs(h_theta[t]) > kThetaMax) return fail(ctx, PG_ERR_INVALID, "pg_fraction_import: |theta| > 20");
		s[t].theta = h_theta[t]; s[t].m = h_m[t]; s[t].v = h_v[t]; s[t].p1 = h_p1[t]; s[t].p2 = h_p2[t]; s[t].steps = h_steps[t];
	}
	PG_HIP(ctx, hipDeviceSynchronize());
	PG_HIP(ctx, hipMemcpy(ctx->frac.tab.p, tab.data(), tab.size() * sizeof(long long), hipMemcpyHostToDevice));
	return PG_OK;
}

} // extern "C"
