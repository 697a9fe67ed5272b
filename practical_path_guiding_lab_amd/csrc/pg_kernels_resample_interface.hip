// pg_kernels_resample_interface.hip -- pg_resample_interface (include/ext/guiding/pg_resample_interface.h, which states the
// semantics operation by operation): a direction in proportion to radiance times the two-sided lobe of a rough
// dielectric interface, by resampled importance sampling of M candidates from the two-way mixture of the renderer's
// rough-dielectric sampling (reflection or refraction about a GGX visible normal, chosen by Fresnel) and the SD-tree.
// One lane per vertex, wave64, 256-thread groups.
//
// The resampling step is pg_ris_dev.hpp's; what is written here is which lanes are served, how a candidate is drawn, the
// interface's density and eta_out.  The bound: the latency of dependent gathers -- the KD
// grid entry, the tree's head, then per candidate a quadtree walk of 32 bytes per level.  The KD descent and the head are read
// ONCE for the M candidates; the reservoir is four numbers and a direction in registers, there is no per-candidate array:
// nothing can spill.  What the interface adds over the reflection lobe is arithmetic between the gathers: the Fresnel term of
// the sample and of EVERY candidate's density, the refracted direction and the second Jacobian, with the interface's index
// carried across the walks beside the viewer's local direction and the roughness.
// Lanes of a wave take their branches side by side: the sampling walk of a tree candidate; the rough-dielectric sample of a lobe
// candidate, which then meets the others in ONE pdf walk.  The choice is the lane's own draw, per candidate; lanes are not
// reordered.
// Built from the device functions the stand-alone calls use (pg_descent.hpp) and the renderer's frame and rough dielectric
// (pg_render_dev.hpp) AS THEY ARE: rd_sample and rd_eval_pdf are inlined here on a two-word row in registers (they read MAT_ALPHA
// and MAT_ETA and nothing else), and the BSDF value rd_eval_pdf computes beside its pdf, and the weight of rd_sample, are dead
// and go.  One statement of the lobe serves the renderer, the oracle's probe and this call.
#include "../../include/ext/guiding/pg_resample_interface.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_render_dev.hpp"
#include "pg_ris_dev.hpp"

namespace pg {

// the material row rd_sample and rd_eval_pdf read: words MAT_ALPHA and MAT_ETA
struct InterfaceRow {
	float M[MAT_ETA + 1];
};

__device__ __forceinline__ InterfaceRow interface_row(float a, float eta)
{
	InterfaceRow r;
	for (int j = 0; j <= MAT_ETA; ++j) r.M[j] = 0.0f;
	r.M[MAT_ALPHA] = a;
	r.M[MAT_ETA] = eta;
	return r;
}

// b(wl): the density the lobe candidates are drawn with, rd_eval_pdf's pdf
__device__ __forceinline__ float interface_density(const InterfaceRow &row, v3 wil, v3 wl)
{
	v3 value;
	float pdf;
	rd_eval_pdf(row.M, wil, wl, value, pdf);
	return finite_f32(pdf) ? pdf : 0.0f;
}

// kCand: one of the cand_* outputs is given.
// Left alone the compiler takes 103 registers without the candidate stores and 109 with them: four waves per SIMD, no scratch.
// Held to five waves the first would take 96 registers and 32 bytes of scratch per lane, so there is no such bound here.
template <bool kCand>
__global__ __launch_bounds__(kQueryBlock) void k_resample_interface(TreeView t, uint64_t n, pg_resample_interface_args a, RisConsts c)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = a.active ? a.active[i] != 0 : true;
	const float nx = a.normal[i], ny = a.normal[n + i], nz = a.normal[2 * n + i];
	const float vx = a.wi[i], vy = a.wi[n + i], vz = a.wi[2 * n + i];
	const float rough = a.roughness[i], eta = a.eta[i];
	// the reservoir: the kept direction, its target and source, its index; as they stand: nothing kept
	float kx = 0.0f, ky = 0.0f, kz = -1.0f, kt = 0.0f, ks = 0.0f, W = 0.0f, eo = 0.0f;
	uint32_t kk = PG_RESAMPLE_NONE;
	const bool valid = act && finite_f32(nx) && finite_f32(ny) && finite_f32(nz) && finite_f32(vx) && finite_f32(vy) && finite_f32(vz) &&
	                   rough >= PG_RESAMPLE_INTERFACE_MIN_ROUGHNESS && rough <= 1.0f && eta >= PG_RESAMPLE_INTERFACE_MIN_ETA &&
	                   eta <= PG_RESAMPLE_INTERFACE_MAX_ETA && eta != 1.0f; // (a NaN fails)
	if (valid) {
		const float x = a.p[i], y = a.p[n + i], z = a.p[2 * n + i];
		KdNode leaf;
		uint32_t kd_lv;
		kd_descend_grid(t, s_planes, x, y, z, inside_root(t, x, y, z), leaf, kd_lv);
		const uint32_t tree = leaf.tree;
		const TreeHead head = load_head(t.head, tree);
		const Frame fr = make_frame(V(nx, ny, nz));
		const v3 wil = to_local(fr, V(vx, vy, vz));
		const InterfaceRow row = interface_row(-rough, eta);
		Pcg32 rng = {a.rng_state[i], a.rng_inc[i]};
		float wsum = 0.0f;
		for (uint32_t k = 0; k < c.M; ++k) {
			const float xi = rng.next_f32();
			v3 w = V(0.0f, 0.0f, 0.0f);
			float q = 0.0f;
			uint32_t lv;
			bool ok = true;
			if (xi > c.alpha) { // (a NaN xi: the lobe)
				quad_sample(t.rec, t.jump, tree, head, rng, w.x, w.y, w.z, q, lv);
			} else {
				const float xi2 = rng.next_f32();
				const float u1 = rng.next_f32();
				const float u2 = rng.next_f32();
				v3 o, weight;
				float pdf_o, eta_o;
				rd_sample(row.M, wil, xi2, u1, u2, o, pdf_o, weight, eta_o);
				// (eta_o is 1 for a reflection and eta_it, never 1 here, for a refraction.)  A reflection that ends behind the
				// macro-surface, or a refraction in front of it, is a direction where b holds the OTHER branch's density only
				ok = pdf_o != 0.0f && (eta_o == 1.0f) == (wil.z * o.z > 0.0f);
				if (ok) {
					w = to_world(fr, o);
					float cx, cy;
					dir_to_canonical(w.x, w.y, w.z, cx, cy);
					uint32_t slot;
					q = quad_pdf_pre<false>(t.rec, head, cx, cy, jump_prefetch(t.jump, tree, cx, cy, true), lv, slot);
				}
			}
			float s = 0.0f, tg = 0.0f, wk = 0.0f;
			if (ok) {
				const float b = interface_density(row, wil, to_local(fr, w));
				s = c.alpha * b + c.om * q;
				tg = b * (c.d4 + c.omd * q);
				wk = ris_weight(tg, s);
			}
			if (ris_keep(rng, wk, wsum)) {
				kk = k;
				kx = w.x; ky = w.y; kz = w.z;
				kt = tg;
				ks = s;
			}
			if (kCand) ris_store_cand(a, n, i, k, w.x, w.y, w.z, tg, s);
		}
		a.rng_state[i] = rng.state;
		if (kk != PG_RESAMPLE_NONE) {
			W = ris_W(wsum, c.Mf, kt);
			// the index the path is in behind the kept direction, relative to the viewer's: 1 on wi's side
			eo = wil.z * to_local(fr, V(kx, ky, kz)).z > 0.0f ? 1.0f : (wil.z > 0.0f ? eta : 1.0f / eta);
		}
	} else if (kCand) {
		ris_zero_cands(a, n, i, c.M);
	}
	ris_store_kept(a, n, i, kx, ky, kz, W, kt, ks, kk);
	if (a.eta_out) a.eta_out[i] = eo;
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_resample_interface(pg_context *ctx, uint64_t n, const pg_resample_params *params, const pg_resample_interface_args *args, void *stream)
{
	PG_READY(ctx);
	if (!params) return fail(ctx, PG_ERR_INVALID, "pg_resample_interface: NULL params");
	if (!args) return fail(ctx, PG_ERR_INVALID, "pg_resample_interface: NULL args");
	const pg_resample_interface_args &a = *args;
	if (n && (!a.p || !a.normal || !a.wi || !a.roughness || !a.eta || !a.rng_state || !a.rng_inc || !a.dir_out || !a.weight_out))
		return fail(ctx, PG_ERR_INVALID, "pg_resample_interface: NULL pointer");
	RisConsts c;
	if (int rc = resample_consts(ctx, "pg_resample_interface", n, *params, c)) return rc;
	if (n == 0) return PG_OK;
	const TreeView t = ctx->view();
	const hipStream_t s = (hipStream_t)stream;
	if (a.cand_dir_out || a.cand_target_out || a.cand_source_out)
		hipLaunchKernelGGL((k_resample_interface<true>), query_grid(n), dim3(kQueryBlock), 0, s, t, n, a, c);
	else
		hipLaunchKernelGGL((k_resample_interface<false>), query_grid(n), dim3(kQueryBlock), 0, s, t, n, a, c);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

} // extern "C"
