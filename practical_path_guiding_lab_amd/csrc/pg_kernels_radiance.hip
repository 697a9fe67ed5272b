// pg_kernels_radiance.hip -- radiance estimates from sdTree_prev and the guided Russian roulette / splitting decision
// (include/pgsd_radiance.h; not in the reference): one lane per query, wave64, 256-thread groups, the pattern of k_pdf.
//
// Bound like k_pdf: the latency of dependent gathers -- the KD grid entry, then ONE round trip for the three things that need
// only the tree's number (its head, the jump-table entry of the direction, its 8-byte statistical weight), then 32 bytes per
// quadtree level below the table.  No reuse inside a lane; occupancy hides the latency (tests/test_radiance_resources.py).
#include <cmath>

#include "../../include/pgsd_radiance.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_guide_dev.hpp"

namespace pg {

// radiance_leaf (the leaf a record with a canonical direction adds to: its energy and depth): pg_guide_dev.hpp --
// pg_kernels_bounce.hip inlines it too

// RrArgs (what the decision needs beside the estimate, kDecide) and rr_decide (the decision): pg_guide_dev.hpp --
// pg_kernels_irradiance.hip decides on its estimate the same way

// dir == nullptr (uniform; never with kDecide): only the mean, no quadtree is walked.
template <bool kDecide>
__global__ __launch_bounds__(kQueryBlock) void k_radiance(TreeView t, const unsigned long long *__restrict__ wtab, uint64_t n,
                                                        const float *__restrict__ p, const float *__restrict__ dir,
                                                        const uint8_t *__restrict__ active, float *__restrict__ L_dir_out,
                                                        float *__restrict__ L_mean_out, RrArgs rr)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = active ? active[i] != 0 : true;
	const bool walk = dir != nullptr;
	float L_dir = 0.0f, L_mean = 0.0f;
	uint32_t count = 1u;
	float scale = 1.0f;
	if (act) {
		// (everything that does not depend on the tree first: the loads leave before the descent's gathers)
		Pcg32 rng = {0ull, 0ull};
		float w = 0.0f, I = 0.0f;
		if (kDecide) {
			rng.state = rr.rng_state[i];
			rng.inc = rr.rng_inc[i];
			w = rr.weight[i];
			I = rr.reference[i];
		}
		const float x = p[i], y = p[n + i], z = p[2 * n + i];
		float cx = 0.0f, cy = 0.0f;
		if (walk) dir_to_canonical(dir[i], dir[n + i], dir[2 * n + i], cx, cy);
		KdNode leaf;
		uint32_t kd_lv;
		kd_descend_grid(t, s_planes, x, y, z, inside_root(t, x, y, z), leaf, kd_lv);
		// one round trip: the three need the leaf's tree number only.  (The two unconditional gathers first: the table's entry
		// is fetched inside a branch -- the direction may miss the table -- and what is issued behind that branch waits for it.)
		const TreeHead head = load_head(t.head, leaf.tree);
		const uint2 wv = gather8(wtab + leaf.tree);
		const JumpPre pre = jump_prefetch(t.jump, leaf.tree, cx, cy, walk);
		const unsigned long long N = ((unsigned long long)wv.y << 32) | wv.x;
		const float Nf = (float)N; // round to nearest even (not count_to_f32: that one stops at 2^24)
		if (walk) {
			const RadLeaf lf = radiance_leaf(t.rec, head, cx, cy, pre);
			const float area_inv = __uint_as_float((127u + 2u * lf.d) << 23); // 4^d, exact
			L_dir = N == 0ull ? 0.0f : ((lf.e * area_inv) * kInvFourPiF) / Nf;
		}
		L_mean = N == 0ull ? 0.0f : (head.root_irr * kInvFourPiF) / Nf;
		if (kDecide) {
			const float xi = rng.next_f32(); // exactly one draw per active lane
			rr.rng_state[i] = rng.state;
			rr_decide(rr, xi, L_dir, w, I, count, scale);
		}
	}
	if (L_dir_out) L_dir_out[i] = L_dir;
	if (kDecide) {
		rr.count_out[i] = count;
		rr.scale_out[i] = scale;
	} else if (L_mean_out) {
		L_mean_out[i] = L_mean;
	}
}

// the table of a refined forest (pg_refine.hip): new tree t is a copy or refinement of old tree tree_src[t], whose energies
// were resolved from accumulators that had received tree_count[tree_src[t]] in-box records (k_resolve_roots)
__global__ __launch_bounds__(kQueryBlock) void k_radiance_carry(const unsigned long long *__restrict__ tree_count, uint32_t n_old,
                                                              const uint32_t *__restrict__ tree_src,
                                                              unsigned long long *__restrict__ w_new, uint32_t n_new)
{
	const uint32_t t = blockIdx.x * kQueryBlock + threadIdx.x;
	if (t >= n_new) return;
	uint32_t src = tree_src[t];
	if (src >= n_old) src = 0; // (never: tree_src names pre-refine trees)
	w_new[t] = tree_count[src];
}

void launch_radiance_carry(const unsigned long long *tree_count, uint32_t n_old, const uint32_t *tree_src, unsigned long long *w_new,
                           uint32_t n_new, hipStream_t s)
{
	if (n_new == 0) return;
	hipLaunchKernelGGL(k_radiance_carry, query_grid(n_new), dim3(kQueryBlock), 0, s, tree_count, n_old, tree_src, w_new, n_new);
}

int radiance_source(pg_context *ctx, const char *who)
{
	const std::string w = std::string(who) + ": ";
	if (!ctx->rad.on) return fail(ctx, PG_ERR_INVALID, w + "call pg_radiance_enable first");
	if (!ctx->rad.valid)
		return fail(ctx, PG_ERR_INVALID, w + "the weights of this tree are unknown (no refine since pg_radiance_enable, no pg_radiance_import)");
	if (ctx->rad.of_target)
		return fail(ctx, PG_ERR_INVALID, w + "sdTree_prev was refined from a second-moment target (pg_target_apply): it holds roots of second moments, not radiance");
	return PG_OK;
}

int rr_window(pg_context *ctx, const char *who, const pg_rr_params *params, RrArgs &rr)
{
	const std::string w = std::string(who) + ": ";
	if (!params) return fail(ctx, PG_ERR_INVALID, w + "NULL params");
	if (!(std::isfinite(params->window) && params->window >= 1.0f)) return fail(ctx, PG_ERR_INVALID, w + "window must be finite and >= 1");
	if (params->max_split < 1u || params->max_split > 65536u) return fail(ctx, PG_ERR_INVALID, w + "max_split must lie in 1 .. 65536");
	const float s = params->window; // (fp32, each operation rounded on its own: the build's -ffp-contract=off holds for the host too)
	rr.lo = 2.0f / (1.0f + s);
	rr.hi = s * rr.lo;
	rr.max_split = params->max_split;
	rr.max_split_f = (float)params->max_split;
	return PG_OK;
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_radiance_enable(pg_context *ctx, int32_t on)
{
	PG_READY(ctx);
	Radiance &r = ctx->rad;
	if (!on) {
		PG_HIP(ctx, hipDeviceSynchronize()); // (kernels that read the table have finished)
		r.disable(); // (and with the weights the irradiance table built from them, pgsd_irradiance.h)
		return PG_OK;
	}
	if (r.on) return PG_OK;
	PG_HIP(ctx, hipDeviceSynchronize());
	hipError_t e = r.tab.ensure(ctx->f.n_trees);
	if (e != hipSuccess) {
		r.disable();
		return hip_fail(ctx, e, "pg_radiance_enable: table");
	}
	r.on = true;
	r.valid = 0;
	r.of_target = 0;
	return PG_OK;
}

int pg_radiance_status(pg_context *ctx, int32_t *enabled, int32_t *valid, int32_t *of_target)
{
	PG_READY(ctx);
	if (enabled) *enabled = ctx->rad.on ? 1 : 0;
	if (valid) *valid = ctx->rad.valid;
	if (of_target) *of_target = ctx->rad.of_target;
	return PG_OK;
}

int pg_radiance_export(pg_context *ctx, uint64_t n_trees, uint64_t *h_weight)
{
	PG_READY(ctx);
	if (!ctx->rad.on) return fail(ctx, PG_ERR_INVALID, "pg_radiance_export: call pg_radiance_enable first");
	if (!ctx->rad.valid) return fail(ctx, PG_ERR_INVALID, "pg_radiance_export: the weights of this tree are unknown (no refine since pg_radiance_enable, no pg_radiance_import)");
	if (n_trees != ctx->f.n_trees) return fail(ctx, PG_ERR_INVALID, "pg_radiance_export: n_trees does not match pg_export_sizes' n_roots");
	if (!h_weight) return fail(ctx, PG_ERR_INVALID, "pg_radiance_export: NULL pointer");
	PG_HIP(ctx, hipDeviceSynchronize());
	PG_HIP(ctx, hipMemcpy(h_weight, ctx->rad.tab.p, (size_t)n_trees * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return PG_OK;
}

int pg_radiance_import(pg_context *ctx, uint64_t n_trees, const uint64_t *h_weight)
{
	PG_READY(ctx);
	if (!ctx->rad.on) return fail(ctx, PG_ERR_INVALID, "pg_radiance_import: call pg_radiance_enable first");
	if (n_trees != ctx->f.n_trees) return fail(ctx, PG_ERR_INVALID, "pg_radiance_import: n_trees does not match pg_export_sizes' n_roots");
	if (!h_weight) return fail(ctx, PG_ERR_INVALID, "pg_radiance_import: NULL pointer");
	PG_HIP(ctx, hipDeviceSynchronize());
	PG_HIP(ctx, hipMemcpy(ctx->rad.tab.p, h_weight, (size_t)n_trees * sizeof(uint64_t), hipMemcpyHostToDevice));
	ctx->rad.valid = 1;
	ctx->rad.of_target = 0;
	ctx->rad.irr.built = 0; // (pgsd_irradiance.h: its table was projected with the weights this call replaced)
	return PG_OK;
}

int pg_radiance_query(pg_context *ctx, uint64_t n, const float *p, const float *dir, const uint8_t *active, float *L_dir_out,
                      float *L_mean_out, void *stream)
{
	PG_READY(ctx);
	if (int rc = radiance_source(ctx, "pg_radiance_query")) return rc;
	if ((dir == nullptr) != (L_dir_out == nullptr))
		return fail(ctx, PG_ERR_INVALID, "pg_radiance_query: dir and L_dir_out are given together or both NULL");
	if (n && (!p || (!dir && !L_mean_out))) return fail(ctx, PG_ERR_INVALID, "pg_radiance_query: NULL pointer");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_radiance_query: too many lanes for one launch");
	if (n == 0) return PG_OK;
	RrArgs rr = {};
	hipLaunchKernelGGL(k_radiance<false>, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), ctx->rad.tab.p, n, p, dir,
	                   active, L_dir_out, L_mean_out, rr);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_radiance_rr(pg_context *ctx, uint64_t n, const float *p, const float *dir, const float *weight, const float *reference,
                   const pg_rr_params *params, uint64_t *rng_state, const uint64_t *rng_inc, const uint8_t *active,
                   uint32_t *count_out, float *scale_out, float *L_dir_out, void *stream)
{
	PG_READY(ctx);
	if (int rc = radiance_source(ctx, "pg_radiance_rr")) return rc;
	RrArgs rr;
	if (int rc = rr_window(ctx, "pg_radiance_rr", params, rr)) return rc;
	if (n && (!p || !dir || !weight || !reference || !rng_state || !rng_inc || !count_out || !scale_out))
		return fail(ctx, PG_ERR_INVALID, "pg_radiance_rr: NULL pointer");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_radiance_rr: too many lanes for one launch");
	if (n == 0) return PG_OK;
	rr.weight = weight; rr.reference = reference;
	rr.rng_state = rng_state; rr.rng_inc = rng_inc;
	rr.count_out = count_out; rr.scale_out = scale_out;
	hipLaunchKernelGGL(k_radiance<true>, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), ctx->rad.tab.p, n, p, dir,
	                   active, L_dir_out, (float *)nullptr, rr);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

} // extern "C"
