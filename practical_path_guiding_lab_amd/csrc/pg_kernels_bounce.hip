// pg_kernels_bounce.hip -- pg_bounce (include/pgsd_bounce.h, which states the semantics operation by operation):
// the learned fraction's query, the selection, the guide bounce and the radiance estimate of one path vertex behind ONE KD
// descent.  One lane per ray, wave64, 256-thread groups.
//
// Bound like k_guide_bounce: the latency of dependent gathers -- the KD grid entry, then ONE round trip for everything that needs
// only the tree's number (its head, the leaf's theta, its 8-byte statistical weight, the jump-table entries of the NEE direction
// and of the continuation direction), then 32 bytes per quadtree level.  No reuse inside a lane; occupancy hides the latency
// (tests/test_bounce_resources.py).
// The default kernels are not touched: this is a kernel of its own, built from the device functions the stand-alone calls use
// (pg_descent.hpp, pg_guide_dev.hpp) as they are, not a switch in k_guide_bounce (a shared body moved the default kernel's code
// once).
#include "../../include/pgsd_bounce.h"
#include "../../include/pgsd_radiance.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_guide_dev.hpp"

namespace pg {

// what the kernel needs beside the caller's arrays
struct BounceTables {
	const FracLeaf *leaves;            // nullptr: the learned fraction is off, f = f_const
	float theta0, f_const;
	const unsigned long long *weights; // the radiance table (kRadiance)
};

// jump_prefetch (pg_descent.hpp) for the two pdf walks of a lane, with the gathers at unconditional load sites, the way
// kd_descend_grid reads its grid: both cells are worked out first, then every lane gathers two entries back to back.  A lane that
// has none to fetch (not wanted, or the direction misses the table) reads entry 0 of the table -- one address for all of them,
// a single request per wave -- and drops it.  The values are jump_prefetch's.  With each gather inside its `if (hit)` the compiler
// folded the first use of the first entry (the "pdf undefined" bit quad_pdf_pre tests) into that branch and put the
// s_waitcnt vmcnt(0) right behind the load: the second entry's gather left behind that wait, a round trip of its own
// (DESIGN.md 5.19).
__device__ __forceinline__ void jump_prefetch_pair(JumpRef jump, uint32_t tree, float ax, float ay, bool a_wanted, float bx, float by,
                                                   bool b_wanted, JumpPre &a, JumpPre &b)
{
	a.e = make_uint4(0u, 0u, 0u, 0u);
	b.e = make_uint4(0u, 0u, 0u, 0u);
	a.jx = 0.0f; a.jy = 0.0f; b.jx = 0.0f; b.jy = 0.0f;
	a.bits = jump.bits; b.bits = jump.bits;
	uint32_t a_cell = 0, b_cell = 0;
	a.hit = a_wanted && jump.p != nullptr && jump_cell(jump.bits, ax, ay, a_cell, a.jx, a.jy);
	b.hit = b_wanted && jump.p != nullptr && jump_cell(jump.bits, bx, by, b_cell, b.jx, b.jy);
	if (jump.p != nullptr) { // (uniform)
		const size_t base = (size_t)tree << (2 * jump.bits);
		const uint4 ea = gather16(jump.p + (a.hit ? base + a_cell : (size_t)0));
		const uint4 eb = gather16(jump.p + (b.hit ? base + b_cell : (size_t)0));
		if (a.hit) a.e = ea;
		if (b.hit) b.e = eb;
	}
}

// kWarp: the select == 2 lanes warp u (pg_guide_bounce_warp) instead of drawing from their PCG32 stream (pg_guide_bounce).
// kRadiance: L_dir_out or L_mean_out is given.
template <bool kWarp, bool kRadiance>
__global__ __launch_bounds__(kQueryBlock) void k_guided_bounce(TreeView t, uint64_t n, pg_bounce_args a, BounceTables tb)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	const uint64_t tid = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	// the compacted list of k_guide_bounce: [0, front) from the start of lane_index, the next `back` entries from its end
	const uint64_t front = a.lane_index ? (uint64_t)a.d_lane_count[0] : n;
	const uint64_t live = a.lane_index ? front + (uint64_t)a.d_lane_count[1] : n;
	if ((uint64_t)blockIdx.x * kQueryBlock >= live) return; // whole workgroup idle (uniform)
	stage_kd_planes(s_planes, t);
	if (!(tid < live && tid < n)) return;
	const uint64_t i = a.lane_index ? (uint64_t)a.lane_index[tid < front ? tid : n - 1 - (tid - front)] : tid;
	if (i >= n) return; // (a list not written by pg_compact_lanes for this n: nothing is touched)
	const bool nee = a.nee_active ? a.nee_active[i] != 0 : true;
	uint32_t md = a.mode ? (uint32_t)a.mode[i] : (uint32_t)PG_BOUNCE_CHOOSE;
	if (md > (uint32_t)PG_BOUNCE_CHOOSE) md = PG_BOUNCE_NONE;
	const bool choose = md == PG_BOUNCE_CHOOSE;
	const bool is_live = nee || md != PG_BOUNCE_NONE;
	if (!is_live) { // what pg_fraction_query gives an inactive lane; dir_io and the stream are not touched
		if (a.select_out) a.select_out[i] = 0;
		if (a.fraction_out) a.fraction_out[i] = tb.leaves ? logistic_f32(tb.theta0) : tb.f_const;
		a.pdf_nee_out[i] = 1.0f;
		a.pdf_out[i] = 1.0f;
		if (kRadiance) {
			if (a.L_dir_out) a.L_dir_out[i] = 0.0f;
			if (a.L_mean_out) a.L_mean_out[i] = 0.0f;
		}
		return;
	}
	// ---- everything that does not depend on the tree, then the descent, then one round trip of gathers
	const float x = a.p[i], y = a.p[n + i], z = a.p[2 * n + i];
	float ncx = 0.0f, ncy = 0.0f, wcx = 0.0f, wcy = 0.0f, ux = 0.0f, uy = 0.0f, xi = 0.0f;
	if (nee) dir_to_canonical(a.dir_nee[i], a.dir_nee[n + i], a.dir_nee[2 * n + i], ncx, ncy);
	// (a CHOOSE lane may select 1: its pdf walk's canonical form and table entry are fetched before the choice is known)
	const bool may_pdf = md == PG_BOUNCE_PDF || choose;
	if (may_pdf) dir_to_canonical(a.dir_io[i], a.dir_io[n + i], a.dir_io[2 * n + i], wcx, wcy);
	Pcg32 rng = {0ull, 0ull};
	bool stream_moved = false;
	if (md >= (uint32_t)PG_BOUNCE_SAMPLE) {
		if (kWarp) { ux = a.u[i]; uy = a.u[n + i]; }
		else { rng.state = a.rng_state[i]; rng.inc = a.rng_inc[i]; }
	}
	if (choose) {
		if (a.u_select) xi = a.u_select[i];
		else if (!kWarp) { xi = rng.next_f32(); stream_moved = true; } // exactly one draw, before anything else
	}
	const bool inside = inside_root(t, x, y, z);
	KdNode leaf;
	uint32_t kd_lv;
	kd_descend_grid(t, s_planes, x, y, z, inside, leaf, kd_lv);
	const uint32_t tree = leaf.tree;
	// one round trip: all of these need the leaf's tree number only, and none of them sits in a branch
	const TreeHead head = load_head(t.head, tree);
	float theta = tb.theta0;
	if (tb.leaves) { // (uniform)
		const float th = tb.leaves[tree].theta;
		if (inside) theta = th; // (outside the box, NaN: theta0, pg_fraction_query's answer)
	}
	uint2 wv = make_uint2(0u, 0u);
	if (kRadiance) wv = gather8(tb.weights + tree);
	JumpPre pre_nee, pre_wo;
	jump_prefetch_pair(t.jump, tree, ncx, ncy, nee, wcx, wcy, may_pdf, pre_nee, pre_wo);
	const float f = tb.leaves ? logistic_f32(theta) : tb.f_const;
	int sel = choose ? (xi > f ? 2 : 1) : (int)md; // (a NaN xi: 1)
	float pdf_nee = 1.0f, pdf = 1.0f, L_dir = 0.0f, L_mean = 0.0f;
	uint32_t lv, slot;
	if (nee) pdf_nee = quad_pdf_pre<false>(t.rec, head, ncx, ncy, pre_nee, lv, slot);
	// the estimate's direction: dir_io as it stands behind the guide bounce
	float rcx = wcx, rcy = wcy;
	JumpPre pre_rad = pre_wo;
	if (sel == 2) {
		float dx, dy, dz;
		if (kWarp) {
			quad_warp(t.rec, t.jump, tree, head, ux, uy, dx, dy, dz, pdf);
		} else {
			quad_sample(t.rec, t.jump, tree, head, rng, dx, dy, dz, pdf, lv);
			stream_moved = true;
		}
		a.dir_io[i] = dx;
		a.dir_io[n + i] = dy;
		a.dir_io[2 * n + i] = dz;
		if (kRadiance) { // (the canonical form of the direction just written, as pg_radiance_query would derive it)
			dir_to_canonical(dx, dy, dz, rcx, rcy);
			pre_rad = jump_prefetch(t.jump, tree, rcx, rcy, true);
		}
	} else if (sel == 1) {
		pdf = quad_pdf_pre<false>(t.rec, head, wcx, wcy, pre_wo, lv, slot);
	}
	if (!kWarp && stream_moved) a.rng_state[i] = rng.state;
	if (kRadiance && sel != 0) {
		const unsigned long long N = ((unsigned long long)wv.y << 32) | wv.x;
		const float Nf = (float)N; // round to nearest even (pgsd_radiance.h)
		const RadLeaf lf = radiance_leaf(t.rec, head, rcx, rcy, pre_rad);
		const float area_inv = __uint_as_float((127u + 2u * lf.d) << 23); // 4^d, exact
		L_dir = N == 0ull ? 0.0f : ((lf.e * area_inv) * kInvFourPiF) / Nf;
		L_mean = N == 0ull ? 0.0f : (head.root_irr * kInvFourPiF) / Nf;
	}
	if (a.select_out) a.select_out[i] = (uint8_t)sel;
	if (a.fraction_out) a.fraction_out[i] = f;
	a.pdf_nee_out[i] = pdf_nee;
	a.pdf_out[i] = pdf;
	if (kRadiance) {
		if (a.L_dir_out) a.L_dir_out[i] = L_dir;
		if (a.L_mean_out) a.L_mean_out[i] = L_mean;
	}
}

template <bool kWarp, bool kRadiance>
static void launch_guided_bounce(const TreeView &t, uint64_t n, const pg_bounce_args &a, const BounceTables &tb, hipStream_t s)
{
	hipLaunchKernelGGL((k_guided_bounce<kWarp, kRadiance>), query_grid(n), dim3(kQueryBlock), 0, s, t, n, a, tb);
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_bounce(pg_context *ctx, uint64_t n, const pg_bounce_args *args, void *stream)
{
	PG_READY(ctx);
	if (!args) return fail(ctx, PG_ERR_INVALID, "pg_bounce: NULL args");
	const pg_bounce_args &a = *args;
	if (n && (!a.p || !a.dir_nee || !a.dir_io || !a.pdf_nee_out || !a.pdf_out)) return fail(ctx, PG_ERR_INVALID, "pg_bounce: NULL pointer");
	if ((a.lane_index == nullptr) != (a.d_lane_count == nullptr))
		return fail(ctx, PG_ERR_INVALID, "pg_bounce: lane_index and d_lane_count go together");
	if (n > 0xffffffffull) return fail(ctx, PG_ERR_INVALID, "pg_bounce: more than 2^32 - 1 lanes");
	const bool streams = a.rng_state != nullptr && a.rng_inc != nullptr;
	const bool warp = a.u != nullptr;
	if (!warp && !streams) return fail(ctx, PG_ERR_INVALID, "pg_bounce: neither u (the warp form) nor rng_state and rng_inc (the PCG32 form) are given");
	if (!a.u_select && warp)
		return fail(ctx, PG_ERR_INVALID, "pg_bounce: u_select is NULL in the warp form, which has no stream to draw the selection from");
	if (!a.u_select && !streams) return fail(ctx, PG_ERR_INVALID, "pg_bounce: u_select is NULL and so are rng_state / rng_inc");
	const bool radiance = a.L_dir_out != nullptr || a.L_mean_out != nullptr;
	if (radiance) // (pg_radiance_query's reasons)
		if (int rc = radiance_source(ctx, "pg_bounce: a radiance output is requested")) return rc;
	if (n == 0) return PG_OK;
	BounceTables tb;
	tb.leaves = ctx->frac.on ? ctx->frac.leaves(ctx->f.n_trees) : nullptr;
	tb.theta0 = ctx->frac.on ? ctx->frac.prm.theta0 : 0.0f;
	tb.f_const = ctx->bsdf_fraction;
	tb.weights = radiance ? ctx->rad.tab.p : nullptr;
	const TreeView t = ctx->view();
	const hipStream_t s = (hipStream_t)stream;
	if (warp) {
		if (radiance) launch_guided_bounce<true, true>(t, n, a, tb, s);
		else launch_guided_bounce<true, false>(t, n, a, tb, s);
	} else {
		if (radiance) launch_guided_bounce<false, true>(t, n, a, tb, s);
		else launch_guided_bounce<false, false>(t, n, a, tb, s);
	}
	PG_LAUNCHED(ctx);
	return PG_OK;
}

} // extern "C"
