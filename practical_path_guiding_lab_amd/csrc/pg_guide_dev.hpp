// pg_guide_dev.hpp -- device functions of the stand-alone guiding calls that more than one translation unit inlines: the learned
// fraction's logistic (pgsd_fraction.h), the sample warp of one quadtree (pgsd_warp.h), the radiance estimate's leaf walk and
// the roulette / splitting decision (pgsd_radiance.h).  Each moved here unchanged from the file that introduced it when it got
// a second caller (pg_kernels_bounce.hip; for the decision pg_kernels_irradiance.hip); the headers named state the semantics
// operation by operation.
#pragma once

#include "pg_descent.hpp"

namespace pg {

// logistic of pgsd_fraction.h
__device__ __forceinline__ float logistic_f32(float theta)
{
	const float e = exp_f32(0.0f - theta);
	return 1.0f / (1.0f + e);
}

constexpr float kOneM = 0.99999994f; // 1 - 2^-24
static_assert(kOneM < 1.0f && kOneM == 1.0f - 5.9604644775390625e-8f, "the largest float below 1");

__device__ __forceinline__ float clamp_unit(float v) { return v > 0.0f ? (v < kOneM ? v : kOneM) : 0.0f; } // (NaN -> 0)

// the row and column probabilities of one node (pgsd_warp.h: t, b, tot, the uniform fallback)
struct WarpNode {
	float eTL, eBL, t, b, tot;
};
__device__ __forceinline__ WarpNode warp_node(const QuadLoad &q)
{
	WarpNode w;
	w.eTL = q.i1; w.eBL = q.i2;
	w.t = q.i0 + q.i1;
	w.b = q.i2 + q.i3;
	w.tot = w.t + w.b;
	if (!(w.tot > 0.0f) || !finite_f32(w.tot)) { w.eTL = 1.0f; w.eBL = 1.0f; w.t = 2.0f; w.b = 2.0f; w.tot = 4.0f; }
	return w;
}

// WARP of pgsd_warp.h.  The pdf along the path is accumulated by quad_sample_t's operations (the REAL energies, also where the
// choice fell back to uniform: the product then meets its 0/0 and the value is 0, as pdfQuadTree's is).
__device__ __forceinline__ void quad_warp(const QuadRec *rec, JumpRef jump, uint32_t tree, TreeHead head, float ux, float uy,
                                          float &dx, float &dy, float &dz, float &pdf_out)
{
	ux = clamp_unit(ux);
	uy = clamp_unit(uy);
	float x0 = 0.0f, y0 = 0.0f, s = 1.0f;
	float pdf = 1.0f, node_irr = head.root_irr;
	bool dead = false;
	uint32_t r = head.root_rec;
	for (int it = 0; it < kMaxLevels && r != kNoRecord; ++it) {
		const QuadLoad q = load_rec(rec, r);
		const WarpNode w = warp_node(q);
		const float Py = w.t / w.tot;
		const bool top = uy < Py;
		float vy = top ? uy / Py : (uy - Py) / (1.0f - Py);
		const float rs = top ? w.t : w.b, eL = top ? w.eTL : w.eBL;
		const float Pl = eL / rs;
		const bool left = ux < Pl;
		float vx = left ? ux / Pl : (ux - Pl) / (1.0f - Pl);
		vx = vx < kOneM ? vx : kOneM;
		vy = vy < kOneM ? vy : kOneM;
		const int k = top ? (left ? 1 : 0) : (left ? 2 : 3);
		const float child_irr = sel4f(k, q.i0, q.i1, q.i2, q.i3);
		if (!dead) {
			pdf = pdf * ((4.0f * child_irr) / node_irr);
			if (pdf != pdf) { pdf = 0.0f; dead = true; }
		}
		node_irr = child_irr;
		const float h = s * 0.5f;
		if (!left) x0 = x0 + h;
		if (top) y0 = y0 + h;
		s = h;
		const uint32_t c = sel4u(k, q.c0, q.c1, q.c2, q.c3);
		r = c == 0 ? kNoRecord : c;
		ux = vx;
		uy = vy;
	}
	const float px = x0 + ux * s, py = y0 + uy * s;
	canonical_to_dir(px, py, dx, dy, dz);
	float qx, qy;
	dir_to_canonical(dx, dy, dz, qx, qy);
	const bool strictly_inside = r == kNoRecord && qx > x0 && qx < x0 + s && qy > y0 && qy < y0 + s;
	if (strictly_inside) {
		pdf_out = dead ? 0.0f : pdf * kInvFourPiF;
	} else {
		uint32_t lv;
		pdf_out = quad_pdf(rec, jump, tree, head, qx, qy, lv);
	}
}

// The leaf that a record with canonical direction (cx, cy) adds to (addIrradiancePropagate, quadtree.py:398-441; the descent
// of pdfQuadTree, quadtree.py:1095-1098): the highest-numbered containing child, level by level -- `last` of `quadrant`.  Its
// energy and depth.  This is not quad_pdf_pre: that one multiplies energies of the LOWEST-numbered containing child on its
// way; here no product is formed, only the last energy and the number of levels are kept.
// pre.hit (the direction lies strictly inside a cell of the jump table: no tie on the levels the table covers): an entry that
// has ended carries the leaf's energy in `irr` and its depth in bits 26-29 of `info` (k_build_jump); one that continues gives
// the record to go on from, the energy of the node reached, and the cell.  Its "pdf undefined" bit says nothing about energies.
struct RadLeaf {
	float e;
	uint32_t d;
};
__device__ __forceinline__ RadLeaf radiance_leaf(const QuadRec *rec, TreeHead head, float cx, float cy, const JumpPre &pre)
{
	uint32_t r = head.root_rec;
	RadLeaf o;
	o.e = head.root_irr;
	o.d = 0;
	float lox = 0.0f, loy = 0.0f, h = 0.5f;
	if (pre.hit) {
		r = pre.e.x;
		o.e = __uint_as_float(pre.e.z);
		o.d = (pre.e.w >> 26) & 15u;
		lox = pre.jx; loy = pre.jy;
		h = 0.5f / (float)(1 << pre.bits); // (an entry that continues took all the levels of the table)
	}
	for (int it = 0; it < kMaxLevels && r != kNoRecord; ++it) {
		const QuadLoad q = load_rec(rec, r);
		const float mx = lox + h, my = loy + h;
		int first, last;
		quadrant(cx, cy, mx, my, first, last);
		if (last < 0) break; // outside every child: the walk ends at the node it stands on (pgsd_radiance.h)
		++o.d;
		o.e = sel4f(last, q.i0, q.i1, q.i2, q.i3);
		const uint32_t c = sel4u(last, q.c0, q.c1, q.c2, q.c3);
		if (last == 0 || last == 3) lox = mx;
		if (last == 0 || last == 1) loy = my;
		h *= 0.5f;
		r = c == 0 ? kNoRecord : c;
	}
	return o;
}

// what the decision needs beside the estimate (the kDecide kernels of pg_kernels_radiance.hip and pg_kernels_irradiance.hip)
struct RrArgs {
	const float *weight, *reference;
	uint64_t *rng_state;
	const uint64_t *rng_inc;
	uint32_t *count_out;
	float *scale_out;
	float lo, hi, max_split_f;
	uint32_t max_split;
};

// DECISION of pgsd_radiance.h behind the lane's one draw xi: L the estimate (pgsd_irradiance.h: E), w the throughput, I the
// reference.  count and scale arrive as 1 and 1 (no opinion) and are written where the lane has one.
__device__ __forceinline__ void rr_decide(const RrArgs &rr, float xi, float L_dir, float w, float I, uint32_t &count, float &scale)
{
	if (L_dir > 0.0f && w > 0.0f && I > 0.0f && finite_f32(L_dir) && finite_f32(w) && finite_f32(I)) {
		const float q = (w * L_dir) / I;
		if (finite_f32(q)) {
			if (q < rr.lo) { // roulette
				const float P = q / rr.lo;
				const bool survive = xi < P;
				count = survive ? 1u : 0u;
				scale = survive ? rr.lo / q : 0.0f;
			} else if (q > rr.hi && rr.max_split > 1u) { // split
				float r = q / rr.hi;
				if (r > rr.max_split_f) r = rr.max_split_f;
				const float k = __builtin_floorf(r);
				count = (uint32_t)k + (xi < r - k ? 1u : 0u);
				scale = 1.0f / r;
			}
		}
	}
}

} // namespace pg
