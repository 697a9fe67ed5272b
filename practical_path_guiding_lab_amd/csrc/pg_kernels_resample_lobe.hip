// pg_kernels_resample_lobe.hip -- pg_resample_lobe (include/ext/guiding/pg_resample_lobe.h, which states the semantics operation
// by operation): a direction in proportion to radiance times a GGX-and-cosine lobe about a normal, by resampled
// importance sampling of M candidates from the three-way mixture of the GGX reflection lobe, the cosine lobe and the SD-tree.
// One lane per vertex, wave64, 256-thread groups.
//
// The resampling step is pg_ris_dev.hpp's; what is written here is which lanes are served, how a candidate is drawn and the
// lobe's density.  The bound: the latency of dependent gathers -- the KD
// grid entry, the tree's head, then per candidate a quadtree walk of 32 bytes per level.  The KD descent and the head are read
// ONCE for the M candidates; the reservoir is four numbers and a direction in registers, there is no per-candidate array:
// nothing can spill.  What the lobe adds is arithmetic between the gathers: the visible-normal sample of a GGX candidate, and
// the GGX density of EVERY candidate (two divisions and two square roots behind a normalisation), with the viewer's local
// direction, the roughness and the specular share carried across the walks beside the frame.
// Lanes of a wave take their branches side by side: the sampling walk of a tree candidate; the GGX sample or the cosine map of a
// lobe candidate, which then meet in ONE pdf walk.  The choice is the lane's own draw, per candidate; lanes are not reordered.
// Built from the device functions the stand-alone calls use (pg_descent.hpp) and the renderer's frame, cosine map and
// microfacet functions (pg_render_dev.hpp) as they are.
#include "../../include/ext/guiding/pg_resample_lobe.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_render_dev.hpp"
#include "pg_ris_dev.hpp"

namespace pg {

// g(wl): the density of the reflection of wil about a GGX visible normal, rc_eval_pdf's pdf (a = -roughness)
__device__ __forceinline__ float lobe_ggx_density(v3 wil, v3 wl, float a)
{
	if (!(wil.z > 0.0f && wl.z > 0.0f)) return 0.0f;
	const v3 H = normalize3(vadd(wl, wil));
	const float D = rc_D(H, a);
	if (D == 0.0f) return 0.0f;
	const float gi = rc_G1(wil, H, a);
	return (dot3(wil, H) > 0.0f && dot3(wl, H) > 0.0f) ? (D * gi) / (4.0f * wil.z) : 0.0f;
}

// kCand: one of the cand_* outputs is given.
// Left alone the compiler takes 97 registers for the kernel without candidate stores -- one more than five waves per SIMD allow --
// and four waves ran 7 % slower than the five it reaches when asked to (profiles/resample_lobe/timing_five_waves.txt); with
// the candidate stores five waves would cost scratch, so that instantiation stays at the four it reaches by itself.
template <bool kCand>
__global__ __launch_bounds__(kQueryBlock, kCand ? 4 : 5) void k_resample_lobe(TreeView t, uint64_t n, pg_resample_lobe_args a, RisConsts c)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = a.active ? a.active[i] != 0 : true;
	const float nx = a.normal[i], ny = a.normal[n + i], nz = a.normal[2 * n + i];
	const float vx = a.wi[i], vy = a.wi[n + i], vz = a.wi[2 * n + i];
	const float rough = a.roughness[i], spec = a.specular[i];
	// the reservoir: the kept direction, its target and source, its index; as they stand: nothing kept
	float kx = 0.0f, ky = 0.0f, kz = -1.0f, kt = 0.0f, ks = 0.0f, W = 0.0f;
	uint32_t kk = PG_RESAMPLE_NONE;
	const bool valid = act && finite_f32(nx) && finite_f32(ny) && finite_f32(nz) && finite_f32(vx) && finite_f32(vy) && finite_f32(vz) &&
	                   rough >= PG_RESAMPLE_LOBE_MIN_ROUGHNESS && rough <= 1.0f && spec >= 0.0f && spec <= 1.0f; // (a NaN fails)
	if (valid) {
		const float x = a.p[i], y = a.p[n + i], z = a.p[2 * n + i];
		KdNode leaf;
		uint32_t kd_lv;
		kd_descend_grid(t, s_planes, x, y, z, inside_root(t, x, y, z), leaf, kd_lv);
		const uint32_t tree = leaf.tree;
		const TreeHead head = load_head(t.head, tree);
		const Frame fr = make_frame(V(nx, ny, nz));
		const v3 wil = to_local(fr, V(vx, vy, vz));
		const float ga = -rough;
		const float sg = wil.z > 0.0f ? spec : 0.0f;
		const float oms = 1.0f - sg;
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
				v3 o;
				if (xi2 < sg) {
					float pdf_m;
					const v3 m = rc_sample_m(wil, ga, u1, u2, pdf_m);
					const float wim = dot3(wil, m);
					o = vsub(vscale(m, 2.0f * wim), wil); // reflect(wil, m)
					ok = pdf_m != 0.0f && o.z > 0.0f;
				} else {
					o = square_to_cosine_hemisphere(u1, u2);
				}
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
				const v3 wl = to_local(fr, w);
				const float cl = wl.z > 0.0f ? wl.z * kInvPiF : 0.0f;
				float b = sg == 0.0f ? cl : (sg * lobe_ggx_density(wil, wl, ga)) + (oms * cl);
				b = finite_f32(b) ? b : 0.0f;
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
		if (kk != PG_RESAMPLE_NONE) W = ris_W(wsum, c.Mf, kt);
	} else if (kCand) {
		ris_zero_cands(a, n, i, c.M);
	}
	ris_store_kept(a, n, i, kx, ky, kz, W, kt, ks, kk);
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_resample_lobe(pg_context *ctx, uint64_t n, const pg_resample_params *params, const pg_resample_lobe_args *args, void *stream)
{
	PG_READY(ctx);
	if (!params) return fail(ctx, PG_ERR_INVALID, "pg_resample_lobe: NULL params");
	if (!args) return fail(ctx, PG_ERR_INVALID, "pg_resample_lobe: NULL args");
	const pg_resample_lobe_args &a = *args;
	if (n && (!a.p || !a.normal || !a.wi || !a.roughness || !a.specular || !a.rng_state || !a.rng_inc || !a.dir_out || !a.weight_out))
		return fail(ctx, PG_ERR_INVALID, "pg_resample_lobe: NULL pointer");
	RisConsts c;
	if (int rc = resample_consts(ctx, "pg_resample_lobe", n, *params, c)) return rc;
	if (n == 0) return PG_OK;
	const TreeView t = ctx->view();
	const hipStream_t s = (hipStream_t)stream;
	if (a.cand_dir_out || a.cand_target_out || a.cand_source_out)
		hipLaunchKernelGGL((k_resample_lobe<true>), query_grid(n), dim3(kQueryBlock), 0, s, t, n, a, c);
	else
		hipLaunchKernelGGL((k_resample_lobe<false>), query_grid(n), dim3(kQueryBlock), 0, s, t, n, a, c);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

} // extern "C"
