// pg_kernels_warp.hip -- hierarchical sample warping over sdTree_prev and its inverse (include/pgsd_warp.h, which states the
// semantics operation by operation): one lane per query, wave64, 256-thread groups, the three entry points.
//
// Bound like pg_kernels_query.hip's kernels: a chain of dependent 32-B gathers, one quadtree record per level, so occupancy
// (registers <= 64 -> 8 waves/SIMD) is what hides the latency.  A record carries the four energies AND the child words: the
// warp needs nothing else per level, draws no random numbers, and nothing is indexed by level (no scratch).
// The default kernels are not touched: k_guide_bounce_warp is a kernel of its own here, not a switch in k_guide_bounce (a
// shared body moved the default kernel's code once).
#include "../../include/pgsd_warp.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_guide_dev.hpp"

namespace pg {

// clamp_unit, warp_node and quad_warp (the WARP of pgsd_warp.h): pg_guide_dev.hpp -- pg_kernels_bounce.hip inlines them too

// INVERSE of pgsd_warp.h for the canonical position (cx, cy).  Every level's probabilities are needed, so the jump tables are
// of no use: the walk starts at the root and forms the pdf on the way by quad_pdf_pre's operations in its order (the lowest-
// numbered containing child's energy, the highest-numbered one's descent) -- the value the tables hold bit for bit (k_build_jump).
__device__ __forceinline__ void quad_unwarp(const QuadRec *rec, TreeHead head, float cx, float cy, float &ux, float &uy,
                                            float &pdf_out)
{
	float ax = 0.0f, ay = 0.0f, bx = 1.0f, by = 1.0f;
	float x0 = 0.0f, y0 = 0.0f, s = 1.0f;
	float pdf = 1.0f, node_irr = head.root_irr;
	bool dead = false; // the product met a 0/0: the value is 0, the walk goes on for u
	uint32_t r = head.root_rec;
	for (int it = 0; it < kMaxLevels && r != kNoRecord; ++it) {
		const QuadLoad q = load_rec(rec, r);
		const float h = s * 0.5f;
		int first, last;
		quadrant(cx, cy, x0 + h, y0 + h, first, last);
		if (!dead) {
			const float child_irr = first < 0 ? 0.0f : sel4f(first, q.i0, q.i1, q.i2, q.i3);
			pdf = pdf * ((4.0f * child_irr) / node_irr);
			if (pdf != pdf) dead = true; // quadtree.py:1090-1092
		}
		if (last < 0) break; // outside every child (a canonical position never is)
		const bool top = last == 0 || last == 1, left = last == 1 || last == 2;
		const WarpNode w = warp_node(q);
		const float Py = w.t / w.tot;
		const float yp = by * Py;
		if (top) by = yp;
		else { ay = ay + yp; by = by * (1.0f - Py); }
		const float rs = top ? w.t : w.b, eL = top ? w.eTL : w.eBL;
		const float Pl = rs > 0.0f ? eL / rs : 0.5f;
		const float xp = bx * Pl;
		if (left) bx = xp;
		else { ax = ax + xp; bx = bx * (1.0f - Pl); }
		if (!left) x0 = x0 + h;
		if (top) y0 = y0 + h;
		s = h;
		node_irr = sel4f(last, q.i0, q.i1, q.i2, q.i3);
		const uint32_t c = sel4u(last, q.c0, q.c1, q.c2, q.c3);
		r = c == 0 ? kNoRecord : c;
	}
	const float vx = (cx - x0) / s, vy = (cy - y0) / s;
	ux = clamp_unit(ax + bx * vx);
	uy = clamp_unit(ay + by * vy);
	pdf_out = dead ? 0.0f : (r == kNoRecord ? pdf * kInvFourPiF : pdf); // (a walk that reached no leaf: pdfQuadTree's value there)
}

__global__ __launch_bounds__(kQueryBlock) void k_sample_warp(TreeView t, uint64_t n, const float *__restrict__ p,
                                                         const float *__restrict__ u,
                                                         const uint8_t *__restrict__ active,
                                                         float *__restrict__ dir_out, float *__restrict__ pdf_out)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = active ? active[i] != 0 : true;
	float dx = 0.0f, dy = 0.0f, dz = -1.0f, pdf = 1.0f; // inactive lanes: pg_sample's values
	if (act) {
		const float x = p[i], y = p[n + i], z = p[2 * n + i];
		const float ux = u[i], uy = u[n + i];
		KdNode leaf;
		uint32_t kd_lv;
		kd_descend_grid(t, s_planes, x, y, z, inside_root(t, x, y, z), leaf, kd_lv);
		quad_warp(t.rec, t.jump, leaf.tree, load_head(t.head, leaf.tree), ux, uy, dx, dy, dz, pdf);
	}
	dir_out[i] = dx;
	dir_out[n + i] = dy;
	dir_out[2 * n + i] = dz;
	pdf_out[i] = pdf;
}

__global__ __launch_bounds__(kQueryBlock) void k_invert_warp(TreeView t, uint64_t n, const float *__restrict__ p,
                                                         const float *__restrict__ dir,
                                                         const uint8_t *__restrict__ active,
                                                         float *__restrict__ u_out, float *__restrict__ pdf_out)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = active ? active[i] != 0 : true;
	float ux = 0.0f, uy = 0.0f, pdf = 1.0f;
	if (act) {
		const float x = p[i], y = p[n + i], z = p[2 * n + i];
		float cx, cy;
		dir_to_canonical(dir[i], dir[n + i], dir[2 * n + i], cx, cy);
		KdNode leaf;
		uint32_t kd_lv;
		kd_descend_grid(t, s_planes, x, y, z, inside_root(t, x, y, z), leaf, kd_lv);
		quad_unwarp(t.rec, load_head(t.head, leaf.tree), cx, cy, ux, uy, pdf);
	}
	u_out[i] = ux;
	u_out[n + i] = uy;
	if (pdf_out) pdf_out[i] = pdf; // (uniform)
}

// k_guide_bounce (pg_kernels_query.hip) with the warp where it samples: the same lanes, the same list of pg_compact_lanes,
// the same two pdf walks; no depth counters.
__global__ __launch_bounds__(kQueryBlock) void k_guide_bounce_warp(TreeView t, uint64_t n, const float *__restrict__ p,
                                                               const float *__restrict__ dir_nee,
                                                               const uint8_t *__restrict__ nee_active,
                                                               const uint8_t *__restrict__ select,
                                                               float *__restrict__ dir_io, const float *__restrict__ u,
                                                               float *__restrict__ pdf_nee_out,
                                                               float *__restrict__ pdf_out,
                                                               const uint32_t *__restrict__ lane_index,
                                                               const uint32_t *__restrict__ d_lane_count)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	const uint64_t tid = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	const uint64_t front = lane_index ? (uint64_t)d_lane_count[0] : n;
	const uint64_t live = lane_index ? front + (uint64_t)d_lane_count[1] : n;
	if ((uint64_t)blockIdx.x * kQueryBlock >= live) return; // whole workgroup idle (uniform)
	stage_kd_planes(s_planes, t);
	if (!(tid < live && tid < n)) return;
	const uint64_t i = lane_index ? (uint64_t)lane_index[tid < front ? tid : n - 1 - (tid - front)] : tid;
	if (i >= n) return; // (a list not written by pg_compact_lanes for this n: nothing is touched)
	const bool nee = nee_active ? nee_active[i] != 0 : true;
	const int sel = select ? (int)select[i] : 2;
	float pdf_nee = 1.0f, pdf = 1.0f;
	if (nee || sel != 0) {
		const float x = p[i], y = p[n + i], z = p[2 * n + i];
		float ncx = 0.0f, ncy = 0.0f, wcx = 0.0f, wcy = 0.0f;
		if (nee) dir_to_canonical(dir_nee[i], dir_nee[n + i], dir_nee[2 * n + i], ncx, ncy);
		if (sel == 1) dir_to_canonical(dir_io[i], dir_io[n + i], dir_io[2 * n + i], wcx, wcy);
		float ux = 0.0f, uy = 0.0f;
		if (sel == 2) { ux = u[i]; uy = u[n + i]; }
		KdNode leaf;
		uint32_t kd_lv;
		kd_descend_grid(t, s_planes, x, y, z, inside_root(t, x, y, z), leaf, kd_lv);
		const TreeHead head = load_head(t.head, leaf.tree);
		const JumpPre pre_nee = jump_prefetch(t.jump, leaf.tree, ncx, ncy, nee);
		const JumpPre pre_wo = jump_prefetch(t.jump, leaf.tree, wcx, wcy, sel == 1);
		uint32_t lv, slot;
		if (nee) pdf_nee = quad_pdf_pre<false>(t.rec, head, ncx, ncy, pre_nee, lv, slot);
		if (sel == 2) {
			float dx, dy, dz;
			quad_warp(t.rec, t.jump, leaf.tree, head, ux, uy, dx, dy, dz, pdf);
			dir_io[i] = dx;
			dir_io[n + i] = dy;
			dir_io[2 * n + i] = dz;
		} else if (sel == 1) {
			pdf = quad_pdf_pre<false>(t.rec, head, wcx, wcy, pre_wo, lv, slot);
		}
	}
	pdf_nee_out[i] = pdf_nee;
	pdf_out[i] = pdf;
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_sample_warp(pg_context *ctx, uint64_t n, const float *p, const float *u, const uint8_t *active, float *dir_out,
                   float *pdf_out, void *stream)
{
	PG_READY(ctx);
	if (n && (!p || !u || !dir_out || !pdf_out)) return fail(ctx, PG_ERR_INVALID, "pg_sample_warp: NULL pointer");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_sample_warp: too many lanes for one launch");
	if (n == 0) return PG_OK;
	hipLaunchKernelGGL(k_sample_warp, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), n, p, u, active, dir_out,
	                   pdf_out);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_invert_warp(pg_context *ctx, uint64_t n, const float *p, const float *dir, const uint8_t *active, float *u_out,
                   float *pdf_out, void *stream)
{
	PG_READY(ctx);
	if (n && (!p || !dir || !u_out)) return fail(ctx, PG_ERR_INVALID, "pg_invert_warp: NULL pointer");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_invert_warp: too many lanes for one launch");
	if (n == 0) return PG_OK;
	hipLaunchKernelGGL(k_invert_warp, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), n, p, dir, active, u_out,
	                   pdf_out);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_guide_bounce_warp(pg_context *ctx, uint64_t n, const float *p, const float *dir_nee, const uint8_t *nee_active,
                         const uint8_t *select, float *dir_io, const float *u, float *pdf_nee_out, float *pdf_out,
                         const uint32_t *lane_index, const uint32_t *d_lane_count, void *stream)
{
	PG_READY(ctx);
	if (n && (!p || !dir_nee || !dir_io || !u || !pdf_nee_out || !pdf_out))
		return fail(ctx, PG_ERR_INVALID, "pg_guide_bounce_warp: NULL pointer");
	if ((lane_index == nullptr) != (d_lane_count == nullptr))
		return fail(ctx, PG_ERR_INVALID, "pg_guide_bounce_warp: lane_index and d_lane_count go together");
	if (n > 0xffffffffull) return fail(ctx, PG_ERR_INVALID, "pg_guide_bounce_warp: more than 2^32 lanes");
	if (n == 0) return PG_OK;
	hipLaunchKernelGGL(k_guide_bounce_warp, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), n, p, dir_nee,
	                   nee_active, select, dir_io, u, pdf_nee_out, pdf_out, lane_index, d_lane_count);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

} // extern "C"
