// pg_kernels_resample.hip -- pg_resample_cosine (include/pg_resample.h, which states the semantics operation by operation;
// DESIGN.md 5.22): a direction in proportion to radiance times the cosine about a normal, by resampled importance sampling of M
// candidates from the mixture of the cosine lobe and the SD-tree.  One lane per vertex, wave64, 256-thread groups.
//
// Bound like k_guided_bounce: the latency of dependent gathers -- the KD grid entry, the tree's head, then per candidate a
// quadtree walk of 32 bytes per level (a sampling walk from the root, or a pdf walk behind its jump-table entry).  The KD
// descent and the head are read ONCE for the M candidates; the reservoir is four numbers and a direction in registers, and
// there is no per-candidate array: nothing can spill.  No reuse inside a lane; occupancy hides the latency
// (tests/test_resample_resources.py).
// Lanes of a wave take the sampling walk and the cosine-plus-pdf walk side by side, as k_guided_bounce's CHOOSE lanes do: the
// choice is the lane's own draw, per candidate, and lanes are not reordered.
// Built from the device functions the stand-alone calls use (pg_descent.hpp) and the renderer's frame and cosine map
// (pg_render_dev.hpp) as they are.  The resampling step itself -- a candidate's weight, the reservoir's rule, W, the stores --
// is pg_ris_dev.hpp's, shared with the three calls that followed this one; the host checks they share are defined below.
#include "../../include/pg_resample.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_render_dev.hpp"
#include "pg_ris_dev.hpp"

namespace pg {

// kCand: one of the cand_* outputs is given.
template <bool kCand>
__global__ __launch_bounds__(kQueryBlock) void k_resample_cosine(TreeView t, uint64_t n, pg_resample_args a, RisConsts c)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = a.active ? a.active[i] != 0 : true;
	const float nx = a.normal[i], ny = a.normal[n + i], nz = a.normal[2 * n + i];
	// the reservoir: the kept direction, its target and source, its index; as they stand: nothing kept
	float kx = 0.0f, ky = 0.0f, kz = -1.0f, kt = 0.0f, ks = 0.0f, W = 0.0f;
	uint32_t kk = PG_RESAMPLE_NONE;
	if (act && finite_f32(nx) && finite_f32(ny) && finite_f32(nz)) {
		const float x = a.p[i], y = a.p[n + i], z = a.p[2 * n + i];
		KdNode leaf;
		uint32_t kd_lv;
		kd_descend_grid(t, s_planes, x, y, z, inside_root(t, x, y, z), leaf, kd_lv);
		const uint32_t tree = leaf.tree;
		const TreeHead head = load_head(t.head, tree);
		const v3 nrm = V(nx, ny, nz);
		const Frame fr = make_frame(nrm);
		Pcg32 rng = {a.rng_state[i], a.rng_inc[i]};
		float wsum = 0.0f;
		for (uint32_t k = 0; k < c.M; ++k) {
			const float xi = rng.next_f32();
			v3 w;
			float q;
			uint32_t lv;
			if (xi > c.alpha) { // (a NaN xi: cosine)
				quad_sample(t.rec, t.jump, tree, head, rng, w.x, w.y, w.z, q, lv);
			} else {
				const float u1 = rng.next_f32();
				const float u2 = rng.next_f32();
				w = to_world(fr, square_to_cosine_hemisphere(u1, u2));
				float cx, cy;
				dir_to_canonical(w.x, w.y, w.z, cx, cy);
				uint32_t slot;
				q = quad_pdf_pre<false>(t.rec, head, cx, cy, jump_prefetch(t.jump, tree, cx, cy, true), lv, slot);
			}
			const float d = dot3(nrm, w);
			const float cl = d > 0.0f ? d * kInvPiF : 0.0f;
			const float s = c.alpha * cl + c.om * q;
			const float tg = cl * (c.d4 + c.omd * q);
			const float wk = ris_weight(tg, s);
			if (ris_keep(rng, wk, wsum)) {
				kk = k;
				kx = w.x; ky = w.y; kz = w.z;
				kt = tg;
				ks = s;
			}
			if (kCand) ris_store_cand(a, n, i, k, w.x, w.y, w.z, tg, s);
		}
		a.rng_state[i] = rng.state;
		if (kk != PG_RESAMPLE_NONE) W = ris_W(wsum, c.Mf, kt);
	} else if (kCand) {
		ris_zero_cands(a, n, i, c.M);
	}
	ris_store_kept(a, n, i, kx, ky, kz, W, kt, ks, kk);
}

int resample_candidates(pg_context *ctx, const char *who, uint32_t candidates)
{
	if (candidates < 1u || candidates > (uint32_t)PG_RESAMPLE_MAX_CANDIDATES)
		return fail(ctx, PG_ERR_INVALID, std::string(who) + ": candidates must be 1..64");
	return PG_OK;
}

int resample_lanes(pg_context *ctx, const char *who, uint64_t n)
{
	if (n > 0xffffffffull) return fail(ctx, PG_ERR_INVALID, std::string(who) + ": more than 2^32 - 1 lanes");
	return PG_OK;
}

int resample_consts(pg_context *ctx, const char *who, uint64_t n, const pg_resample_params &prm, RisConsts &c)
{
	const std::string w = std::string(who) + ": ";
	if (int rc = resample_candidates(ctx, who, prm.candidates)) return rc;
	if (!(prm.alpha >= 0.0f && prm.alpha <= 1.0f)) return fail(ctx, PG_ERR_INVALID, w + "alpha must be in [0, 1]");
	if (!(prm.delta >= 0.0f && prm.delta <= 1.0f)) return fail(ctx, PG_ERR_INVALID, w + "delta must be in [0, 1]");
	if (prm.reserved != 0u) return fail(ctx, PG_ERR_INVALID, w + "reserved must be 0");
	if (int rc = resample_lanes(ctx, who, n)) return rc;
	c.M = prm.candidates;
	c.Mf = (float)prm.candidates;
	c.alpha = prm.alpha;
	c.om = 1.0f - prm.alpha; // (fp32, each operation rounded on its own: the build's -ffp-contract=off holds for the host too)
	c.d4 = prm.delta * kInvFourPiF;
	c.omd = 1.0f - prm.delta;
	return PG_OK;
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_resample_cosine(pg_context *ctx, uint64_t n, const pg_resample_params *params, const pg_resample_args *args, void *stream)
{
	PG_READY(ctx);
	if (!params) return fail(ctx, PG_ERR_INVALID, "pg_resample_cosine: NULL params");
	if (!args) return fail(ctx, PG_ERR_INVALID, "pg_resample_cosine: NULL args");
	const pg_resample_args &a = *args;
	if (n && (!a.p || !a.normal || !a.rng_state || !a.rng_inc || !a.dir_out || !a.weight_out))
		return fail(ctx, PG_ERR_INVALID, "pg_resample_cosine: NULL pointer");
	RisConsts c;
	if (int rc = resample_consts(ctx, "pg_resample_cosine", n, *params, c)) return rc;
	if (n == 0) return PG_OK;
	const TreeView t = ctx->view();
	const hipStream_t s = (hipStream_t)stream;
	if (a.cand_dir_out || a.cand_target_out || a.cand_source_out)
		hipLaunchKernelGGL((k_resample_cosine<true>), query_grid(n), dim3(kQueryBlock), 0, s, t, n, a, c);
	else
		hipLaunchKernelGGL((k_resample_cosine<false>), query_grid(n), dim3(kQueryBlock), 0, s, t, n, a, c);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

} // extern "C"
