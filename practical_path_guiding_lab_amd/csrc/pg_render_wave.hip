// pg_render_wave.hip -- the bounce of PathGuidingIntegrator.sample() (src/path_guiding_integrator.py:
// 179-381) for scenes with triangle meshes (scenes/veach-ajar, scenes/torus), as a wavefront pipeline.
// The stages of a bounce are device functions -- stage_a, stage_guide, stage_b of pg_render_stages.hpp (shared with the
// fused kernels of quad scenes, pg_render.hip), the BVH walks of pg_render_dev.hpp -- and pg_render_stages chooses how many
// kernels they are cut into behind the closest hits.  This file holds the workspace and path-state planes and records, the
// sort keys, the kernels and their launchers:
//
//   k_wave_trace    :185   scene.ray_intersect: closest hit of every live ray (BVH walk; stacks and the hottest
//                          nodes in LDS); the first launch also makes the camera rays (the split forms only: the
//                          joint form has no such launch for bounce 0).  Between it and what
//                          follows the live list of a sorted bounce is put in spatial order (pg_sort.hip).
//   k_wave_shade    :189-381   (the default) everything else of the bounce on one lane's registers: stage_a,
//                          stage_guide, the shadow ray as an inline any-hit walk, stage_b, the survivors' append;
//                          its FIRST launch makes the camera ray and walks its closest hit too (:185, the slim walk on
//                          the kernel's own stack and LDS top) -- ray, sampler and hit never go through device memory
// or, handing their results on through the planes of `ws` (indexed by the lane's place in the live list):
//   k_wave_shade_a  :189-220, 272-297   stage_a: surface and textures at the hit, emitted radiance and its MIS
//                          weight, one emitter sample (a shadow ray to trace), the BSDF towards it, the
//                          BSDF sample, the lane's class (delta | bsdf | bsdf-mis | sdtree-mis) -- and stage_guide
//                          unless that runs as
//   k_wave_guide    :244, 301, 307   stage_guide alone: the three SD-tree calls of the bounce and nothing else --
//                          one KD descent, the pdf of the emitter direction, sample-or-pdf of the continuation
//                          direction, the canonical coordinates and accumulators the record needs -- the kernel
//                          the HBM roofline of the hot path is measured on
//   k_wave_cast     :213   test_visibility: any-hit walk of the shadow rays, a persistent kernel (a lane whose
//                          ray is done takes the next one: shadow rays end after very different numbers of steps)
//   k_wave_shade_b  :247-261, 302-381   stage_b: mixture pdfs and MIS weights, radiance, the path-vertex record,
//                          throughput, Russian roulette, the next ray; survivors are appended to the
//                          next live list (one atomic per workgroup)
//   k_wave_tail     all stages in sequence for the last few thousand paths of a long pass (see tail_checkpoint)
// (k_wave_guide<true>, k_wave_tail<., true>: the same two with the vertex geometry stored beside the list, pg_render_record_geometry)
//
// History in one paragraph (DESIGN.md 5.2 has the measurements): round 1's single kernel per bounce needed 153
// vector registers and kept its BVH stack in scratch memory; rounds 2 and 3 split it into the five kernels above,
// which is how each stage's bound was found -- address path for the walks, HBM for the planes between the shading
// kernels -- and round 3 put the stages that only handed each other numbers back into one kernel, with the closest
// hits and the sort still on their own.  What a path carries from bounce to bounce travels with its place in the
// live list (st_load below).  Arithmetic and sampler draw order are those of oracle/pg_oracle_render.c, operation
// by operation, in every form.
#include "pg_render_stages.hpp"

namespace pg {

// ---- the workspace: planes of n_lanes 32-bit words ----
enum : int {
	WS_HIT_PRIM = 0, WS_HIT_T, WS_HIT_U, WS_HIT_V,
	WS_P, WS_NG = WS_P + 3,
	WS_FLAGS = WS_NG + 3,
	// ten planes that hold one of two things, by the lane's class: a lane that takes its next direction from
	// the tree (F_SMP_TREE) evaluates its BSDF again for that direction in k_wave_shade_b and needs the
	// shading normal (0-2), wi (3-5), the material (6) and the reflectance (7-9); every other lane keeps its
	// BSDF sample: wo (0-2), the weight (3-5), the pdf (6).  Neither reads the other's set, so they share the
	// planes -- 42 bytes less through HBM per lane and bounce than planes of their own.
	WS_U, WS_LE = WS_U + 10,
	WS_DS_D = WS_LE + 3, WS_DS_PDF = WS_DS_D + 3, WS_EM_W, WS_BV_EM = WS_EM_W + 3, WS_BP_EM = WS_BV_EM + 3,
	WS_SH_O, WS_SH_D = WS_SH_O + 3, WS_SH_T = WS_SH_D + 3,
	WS_WO_T, WS_ETA = WS_WO_T + 3, // the direction k_wave_guide sampled from the tree (F_SMP_TREE lanes); the BSDF sample's eta
	WS_RNG_LO, WS_RNG_HI,
	WS_OCC,
	WS_PDF_NEE, WS_PDF_TREE,
	// sorted bounces (pg_render_sort): k_wave_shade_a is the one kernel that reads the state through the permutation; what
	// k_wave_guide and k_wave_shade_b need of it travels on in ten planes (ws_fwd_store and its loads, below the path-state
	// table): entry PS_THR's four words, entry PS_L's four, the two words of the sampler increment
	WS_FWD, WS_FWD_THR = WS_FWD, WS_FWD_L = WS_FWD_THR + 4, WS_FWD_INC = WS_FWD_L + 4,
	WS_COUNT = WS_FWD_INC + 2
};

// pg_render_record_geometry: a recorded vertex also keeps its position, its two canonical directions and its bounce, in planes
// of the list's stride beside the list (GEO_*, pg_render_dev.hpp) -- what the training filters and pg_render_export_records
// need and the accumulators' names cannot give.  Only the geometry instantiations of k_wave_guide and k_wave_tail store them.
// The position goes out BEFORE the SD-tree calls, so that it is not alive across them; the rest beside store_slots.
__device__ __forceinline__ void store_geo_position(const RenderArgs &a, uint32_t *geo, uint64_t rec_slot, v3 p)
{
	const uint64_t S = a.n_lanes * (uint64_t)a.max_depth;
	float *gf = reinterpret_cast<float *>(geo);
	PG_ST(gf + (GEO_P + 0) * S + rec_slot, p.x); PG_ST(gf + (GEO_P + 1) * S + rec_slot, p.y); PG_ST(gf + (GEO_P + 2) * S + rec_slot, p.z);
}
__device__ __forceinline__ void store_geo_directions(const RenderArgs &a, uint32_t *geo, uint64_t rec_slot, const GuideOut &g, uint32_t depth)
{
	const uint64_t S = a.n_lanes * (uint64_t)a.max_depth;
	float *gf = reinterpret_cast<float *>(geo);
	PG_ST(gf + (GEO_WO + 0) * S + rec_slot, g.wo_cx); PG_ST(gf + (GEO_WO + 1) * S + rec_slot, g.wo_cy);
	// (a vertex whose bounce computed no emitter direction keeps (0, 0): in the square; its nee_lum is zero)
	PG_ST(gf + (GEO_NEE + 0) * S + rec_slot, g.nee_cx); PG_ST(gf + (GEO_NEE + 1) * S + rec_slot, g.nee_cy);
	PG_ST(geo + GEO_DEPTH * S + rec_slot, depth);
}

// ---- lane state and workspace access ----
__device__ __forceinline__ float wsf(const RenderArgs &a, int plane, uint64_t i) { return __uint_as_float(a.ws[(uint64_t)plane * a.n_lanes + i]); }
__device__ __forceinline__ uint32_t wsu(const RenderArgs &a, int plane, uint64_t i) { return a.ws[(uint64_t)plane * a.n_lanes + i]; }
__device__ __forceinline__ v3 ws3(const RenderArgs &a, int plane, uint64_t i) { return V(wsf(a, plane, i), wsf(a, plane + 1, i), wsf(a, plane + 2, i)); }
__device__ __forceinline__ void wsput(const RenderArgs &a, int plane, uint64_t i, float v) { a.ws[(uint64_t)plane * a.n_lanes + i] = __float_as_uint(v); }
__device__ __forceinline__ void wsputu(const RenderArgs &a, int plane, uint64_t i, uint32_t v) { a.ws[(uint64_t)plane * a.n_lanes + i] = v; }
__device__ __forceinline__ void wsput3(const RenderArgs &a, int plane, uint64_t i, v3 v)
{
	wsput(a, plane, i, v.x); wsput(a, plane + 1, i, v.y); wsput(a, plane + 2, i, v.z);
}

// The state of a path TRAVELS WITH ITS PLACE IN THE LIVE LIST: the survivor that k_wave_shade_b appends at
// place `off` of the next bounce's list gets its state written to place `off` of the other state set (two sets,
// swapped per bounce), so that every kernel of the next bounce reads state[place] -- whole cache lines, no
// gather through a list of lane numbers, no dependent load before the first useful one.  16-byte entries, in TWO FORMS with
// one numbering: PLANES st[entry * n_lanes + place] (st_load / st_store; entries 0-4, the sampler's increment beside them in
// inc_in / inc_out) and, on a sorted bounce, ONE 128-byte RECORD per place, carry[place * 8 + entry] (st_rec; all eight):
//   entry        three floats       fourth word
//   PS_RAY_O     ray origin         sampler state, low word
//   PS_RAY_D     ray direction      sampler state, high word
//   PS_THR       throughput         index of refraction (positive), its sign bit = "the previous lobe was a delta"
//   PS_PREV      previous vertex    previous bsdf pdf (a float)
//   PS_L         radiance so far    the path's lane (pixel * spp + s)
//   PS_INC       record only: {sampler increment low word, high word, 0, 0}
//   PS_HIT       record only: {primitive, t, u, v} of the closest hit -- zero from append_survivors, filled by k_wave_trace
//   PS_SPARE     record only: unused, written as zero (a line written in part is read, merged and written back)
// The radiance is written to L_out[lane] once, where the path ends.  (Round 2 kept the state in place, indexed by
// lane: scattered 16-byte accesses whose share of each cache line shrank with every bounce's survivors.)
enum : int { PS_RAY_O = 0, PS_RAY_D, PS_THR, PS_PREV, PS_L, PS_INC, PS_HIT, PS_SPARE, PS_ENTRIES = 8 };
__device__ __forceinline__ uint4 st_load(const uint4 *st, const RenderArgs &a, int q, uint64_t i) { return st[(uint64_t)q * a.n_lanes + i]; }
__device__ __forceinline__ void st_store(uint4 *st, const RenderArgs &a, int q, uint64_t i, uint4 v) { st[(uint64_t)q * a.n_lanes + i] = v; }
__device__ __forceinline__ uint4 *st_rec(uint4 *carry, uint64_t place, int entry = 0) { return carry + place * PS_ENTRIES + entry; }
// an entry from its three floats and its fourth word, and the fields back out of it, one value each
__device__ __forceinline__ uint4 st_q(v3 v, uint32_t w) { return make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), w); }
__device__ __forceinline__ v3 st_v3(uint4 q) { return V(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z)); }
__device__ __forceinline__ float st_wf(uint4 q) { return __uint_as_float(q.w); }
__device__ __forceinline__ uint64_t st_u64(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }
__device__ __forceinline__ uint32_t st_pack_ior(float ior, bool delta) { return __float_as_uint(ior) | (delta ? 0x80000000u : 0u); }
__device__ __forceinline__ float st_ior(uint4 q_thr) { return __uint_as_float(q_thr.w & 0x7fffffffu); }
__device__ __forceinline__ bool st_delta(uint4 q_thr) { return (q_thr.w >> 31) != 0u; }
__device__ __forceinline__ uint64_t st_lane(uint4 q_l) { return q_l.w; }
__device__ __forceinline__ uint4 st_q_hit(const HitRec &h) { return make_uint4((uint32_t)h.prim, __float_as_uint(h.t), __float_as_uint(h.u), __float_as_uint(h.v)); }
__device__ __forceinline__ HitRec st_hit(uint4 q_hit) { return HitRec{(int)q_hit.x, __uint_as_float(q_hit.y), __uint_as_float(q_hit.z), __uint_as_float(q_hit.w)}; }
// (the hit of an unsorted bounce: k_wave_trace's four planes)
__device__ __forceinline__ HitRec ws_hit(const RenderArgs &a, uint64_t i) { return HitRec{(int)wsu(a, WS_HIT_PRIM, i), wsf(a, WS_HIT_T, i), wsf(a, WS_HIT_U, i), wsf(a, WS_HIT_V, i)}; }
// WS_FWD: what k_wave_shade_a read through the permutation goes on, word by word, to the kernels behind it (ws4 reads an entry back)
__device__ __forceinline__ void wsput4(const RenderArgs &a, int plane, uint64_t i, uint4 q)
{
	wsputu(a, plane, i, q.x); wsputu(a, plane + 1, i, q.y); wsputu(a, plane + 2, i, q.z); wsputu(a, plane + 3, i, q.w);
}
__device__ __forceinline__ uint4 ws4(const RenderArgs &a, int plane, uint64_t i) { return make_uint4(wsu(a, plane, i), wsu(a, plane + 1, i), wsu(a, plane + 2, i), wsu(a, plane + 3, i)); }
__device__ __forceinline__ void ws_fwd_store(const RenderArgs &a, uint64_t i, uint4 q_thr, uint4 q_l, uint4 q_inc)
{
	wsput4(a, WS_FWD_THR, i, q_thr); wsput4(a, WS_FWD_L, i, q_l);
	wsputu(a, WS_FWD_INC, i, q_inc.x); wsputu(a, WS_FWD_INC + 1, i, q_inc.y);
}
// the sampler's increment of place i: forwarded on a sorted bounce (a.perm), else beside the planes
__device__ __forceinline__ uint64_t ws_fwd_inc(const RenderArgs &a, uint64_t i) { return a.perm ? st_u64(wsu(a, WS_FWD_INC, i), wsu(a, WS_FWD_INC + 1, i)) : a.inc_in[i]; }
// the radiance of a path that ends here (:431), written once -- one 16-byte store (k_finish lays the output column out)
__device__ __forceinline__ void end_path(const RenderArgs &a, uint64_t lane, v3 L) { a.Lq[lane] = st_q(L, 0u); }

// The sort key of a vertex (pg_sort.hip), 16 bits: the Morton code of its cell in a 32^3 grid over the SD-tree's root box
// (15 bits) and, below it, which half of that cell along the box's longest axis (measured: 12 / 15 / 16 key bits ->
// 35.5 / 34.9 / 34.8 ms of shading per step; 18 bits cost a third radix pass and gain nothing more); 0xfffe for a ray that
// left the scene (it still has to be shaded: :189-200 does not apply, the path ends); places of the list that hold no
// path keep the 0xffff the buffer was filled with and sort behind everything.
__device__ __forceinline__ uint32_t spread5(uint32_t v) // bits 0-4 -> bits 0, 3, 6, 9, 12
{
	return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6) | ((v & 16u) << 8);
}
// The key's LOWEST bit on a guided pass: the lane's CLASS at this bounce -- whether it will take its direction from the SD-tree
// (:286 `next_1d() > bsdfSamplingFraction`) or from its BSDF.  The draw is the sixth of the bounce (:214 two, :272 three, :286),
// so the closest-hit kernel, which holds the path's sampler state, can look it up ahead of time.  Inside a cell of the sort the
// lanes then stand class by class and most waves hold ONE class: the sampling walk and the second BSDF evaluation run on full
// waves of "tree" lanes, the pdf walk on full waves of "BSDF" lanes, instead of every wave making all three for half its lanes
// each.  A hint, not a contract: where the guess is wrong (a delta lobe, :283) only the order differs, and the order is free.
__device__ __forceinline__ uint32_t lane_class_ahead(uint64_t state, uint64_t inc, float frac)
{
	Pcg32 r;
	r.state = state; r.inc = inc;
	r.skip(); r.skip(); r.skip(); r.skip(); r.skip();
	return r.next_f32() > frac ? 1u : 0u;
}

__device__ __forceinline__ uint32_t vertex_sort_key(const RenderArgs &a, v3 p, int cls = -1)
{
	uint32_t c[3];
	const float q[3] = {p.x, p.y, p.z};
	const float ext[3] = {a.tree.bmax[0] - a.tree.bmin[0], a.tree.bmax[1] - a.tree.bmin[1], a.tree.bmax[2] - a.tree.bmin[2]};
	const int longest = ext[0] >= ext[1] ? (ext[0] >= ext[2] ? 0 : 2) : (ext[1] >= ext[2] ? 1 : 2); // (uniform)
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		float f = (q[k] - a.tree.bmin[k]) / ext[k] * 64.0f;
		if (!(f > 0.0f)) f = 0.0f; // (NaN too)
		if (f > 63.0f) f = 63.0f;
		c[k] = (uint32_t)f;
	}
	const uint32_t half = cls >= 0 ? (uint32_t)cls : ((longest == 0 ? c[0] : (longest == 1 ? c[1] : c[2])) & 1u);
	// (measured: the class as the key's highest bit instead -- the list in two halves, each in cell order -- shades in the same time)
	const uint32_t m = ((spread5(c[0] >> 1) | (spread5(c[1] >> 1) << 1) | (spread5(c[2] >> 1) << 2)) << 1) | half;
	return m < 0xfffdu ? m : 0xfffdu; // (0xfffe and 0xffff mean something else)
}

// ---- :185 scene.ray_intersect: one ray per lane.  (The persistent form below was measured too: the walks of
// closest-hit rays are all about equally long, handing idle lanes new rays gains nothing after the second
// bounce and loses a factor of two on the coherent camera rays.) ----
template <int kLevel, bool kFirst>
__global__ __launch_bounds__(kRBlock) void k_wave_trace(RenderArgs a)
{
	__shared__ uint2 s_stack[kLdsStack][kRBlock];
	uint64_t tid;
	bool alive;
	if (!wave_entry<kFirst>(a, tid, alive)) return;
	// The ray is ASKED FOR ahead of the staging of the BVH's top (round 6): the staging ends in a workgroup barrier no load
	// moves across, and the ray's round trip used to begin behind it.
	const bool want_cls = !kFirst && a.carry_in && a.guided && a.bounce + 1 < a.max_depth; // (uniform)
	uint4 q0 = make_uint4(0u, 0u, 0u, 0u), q1 = q0, q5 = q0;
	if (!kFirst) {
		// a sorted bounce: the state is in the paths' 128-byte records only; else in the planes of the state set.  ONE
		// unconditional load site per entry: a load under a per-lane condition is merged with its zero behind the branch, and
		// that merge waits for the load -- so a lane past the list reads place 0's entries (the list is not empty: this
		// workgroup runs) and drops them, and the entry of the sort key's class bit is read whether or not it is used.
		// (Measured and removed, round 5: these three entries read by four lanes per record and handed over through the wave's
		// stack columns, as k_wave_shade reads its PERMUTED records -- here the wave's records lie side by side, consecutive
		// lanes ask for consecutive lines, and the detour through LDS cost 11.5 -> 12.8 ms per step:
		// profiles/r05/ab_trace_coop_record_load_rejected.txt.)
		const uint64_t it = alive ? tid : 0;
		const uint4 *p0 = a.carry_in ? st_rec(a.carry_in, it, PS_RAY_O) : a.st_in + it;
		const uint4 *p1 = a.carry_in ? st_rec(a.carry_in, it, PS_RAY_D) : a.st_in + a.n_lanes + it;
		const uint4 *p5 = a.carry_in ? st_rec(a.carry_in, it, PS_INC) : p0;
		q0 = *p0; q1 = *p1; q5 = *p5;
	}
	__shared__ u32x4_t s_top[kBvhTopNodes * kBvhNodeQuads];
	BvhStack stk = bvh_stack(&s_stack[0][threadIdx.x], a.bvh_ovf, (uint32_t)tid * (uint32_t)kOvfStack);
	stage_bvh_top<kBvhTopNodes>(s_top, a, stk);
	if (!alive) return;
	v3 ray_o, ray_d;
	int cls_ahead = -1; // (a sorted, guided bounce: the lane's class, for the sort key)
	if (kFirst) { // (place = lane in the first list)
		Pcg32 rng;
		camera_ray(a, tid, rng, ray_o, ray_d);
		// (this launch FILLS the set the first bounce reads: the only writer of an "in" set)
		const_cast<uint64_t *>(a.inc_in)[tid] = rng.inc;
		st_store(const_cast<uint4 *>(a.st_in), a, PS_RAY_O, tid, st_q(ray_o, (uint32_t)rng.state));
		st_store(const_cast<uint4 *>(a.st_in), a, PS_RAY_D, tid, st_q(ray_d, (uint32_t)(rng.state >> 32)));
	} else {
		ray_o = st_v3(q0);
		ray_d = st_v3(q1);
		// (the class bit of the sort key is made HERE, ahead of the walk, from the sampler state in the two entries just read: one
		// register through the walk instead of the state's four)
		if (want_cls && tid < (uint64_t)a.n_sort)
			cls_ahead = (int)lane_class_ahead(st_u64(q0.w, q1.w), st_u64(q5.x, q5.y), a.frac);
	}
	HitRec h;
	h.u = 0.0f; h.v = 0.0f;
	h.prim = intersect<kLevel, false>(a.shapes, ray_o, ray_d, __builtin_huge_valf(), h.t, stk, h.u, h.v);
	if (a.carry_in) { // a sorted bounce: the hit joins the path's record (PS_HIT), which k_wave_shade_a reads through the permutation
		*st_rec(a.carry_in, tid, PS_HIT) = st_q_hit(h);
		if (tid < (uint64_t)a.n_sort) a.sort_key[tid] = (uint16_t)(h.prim >= 0 ? vertex_sort_key(a, vadd(ray_o, vscale(ray_d, h.t)), cls_ahead) : 0xfffeu);
		return;
	}
	wsputu(a, WS_HIT_PRIM, tid, (uint32_t)h.prim);
	wsput(a, WS_HIT_T, tid, h.t);
	wsput(a, WS_HIT_U, tid, h.u);
	wsput(a, WS_HIT_V, tid, h.v);
}

// ---- :213 test_visibility ----
// Persistent: the grid is as many workgroups as the device holds at once, and a lane whose ray is done
// does not wait for the slowest ray of its wave -- as soon as kRefillIdle lanes of a wave are idle they
// take the next rays of the launch's list.  The list is dealt out in chunks of kCastChunk entries, chunk
// c to wave c mod (number of waves): no atomic counter (one counter word serialises at about 11 ns per
// atomic -- a counter bumped per refill cost more than the walks, and big chunks per atomic left the
// waves unevenly loaded at the end), and with some fifty chunks per wave the rays' costs even out.
// Shadow rays end after very different numbers of steps (an occluder may be the first thing met):
// measured on veach-ajar, the one-ray-per-lane form kept 14 % of the lanes of a wave busy.  Every ray
// still takes exactly the steps intersect() takes for it, in the same order.  The rays are the entries
// of the live list flagged F_NEED_SHADOW; WS_OCC receives 0 / 1.
constexpr int kRefillIdle = 16;
constexpr uint32_t kCastChunk = 128;
// (compiled for seven waves per SIMD -- 72 vector registers, none spilled; left alone the compiler takes 77 and six fit)
template <int kLevel, bool kFirst>
__global__ __launch_bounds__(kRBlock) __attribute__((amdgpu_waves_per_eu(7))) void k_wave_cast(RenderArgs a)
{
	__shared__ uint2 s_stack[kLdsStack][kRBlock];
	if (!kFirst && tail_took_over(a, a.bounce)) return; // a tail launch is finishing these paths
	const uint32_t total = kFirst ? (uint32_t)a.n_lanes : live_final(a, a.bounce - 1);
	const uint32_t gtid = blockIdx.x * kRBlock + threadIdx.x, n_static = gridDim.x * kRBlock;
	if (blockIdx.x * kRBlock >= total) return; // (uniform) not even a first entry for this workgroup
	const unsigned wl = threadIdx.x & 63u;
	const Shapes &sh = a.shapes;
	__shared__ u32x4_t s_top[kBvhTopNodes * kBvhNodeQuads];
	BvhStack stk = bvh_stack(&s_stack[0][threadIdx.x], a.bvh_ovf, gtid * (uint32_t)kOvfStack);
	stage_bvh_top<kBvhTopNodes>(s_top, a, stk);
	const int tri_base = sh.first_tri();
	BvhWalk w;
	w.next = kBvhNone; w.sp = 0; w.budget = 0; w.best = -1; w.bt = 0.0f; w.bu = 0.0f; w.bv = 0.0f;
	bool has = false, first_round = true;
	bool exhausted = n_static >= total; // no entries beyond the first round
	uint32_t pool_next = 0, pool_end = 0; // (wave-uniform) the entries of this wave's current chunk not dealt out yet
	const uint32_t n_waves = n_static / 64u;
	uint64_t chunk = gtid / 64u; // this wave's next chunk of the list beyond the first round
	uint32_t my = 0; // the entry this lane is walking the shadow ray of
	for (;;) {
		// ---- idle lanes take new rays ----
		const unsigned long long idle = __ballot(!has);
		const uint32_t n_idle = (uint32_t)__popcll(idle);
		if (first_round || (!exhausted && n_idle >= (uint32_t)kRefillIdle)) {
			uint32_t idx = 0xffffffffu;
			if (first_round) idx = gtid;
			else {
				if (pool_next == pool_end) { // this wave's next chunk of the list
					const uint64_t begin = (uint64_t)n_static + chunk * kCastChunk;
					chunk += n_waves;
					if (begin >= (uint64_t)total) exhausted = true;
					else {
						pool_next = (uint32_t)begin;
						pool_end = begin + kCastChunk < (uint64_t)total ? (uint32_t)(begin + kCastChunk) : total;
					}
				}
				const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << wl) - 1ull));
				const uint32_t take = n_idle < pool_end - pool_next ? n_idle : pool_end - pool_next;
				if (rank < take) idx = pool_next + rank;
				pool_next += take;
			}
			first_round = false;
			if (!has && idx < total && (wsu(a, WS_FLAGS, idx) & F_NEED_SHADOW)) {
				my = idx;
				const v3 ray_o = ws3(a, WS_SH_O, my), ray_d = ws3(a, WS_SH_D, my);
				int best = -1;
				float bt = wsf(a, WS_SH_T, my);
				intersect_linear<kLevel>(sh, ray_o, ray_d, bt, best);
				bvh_begin(w, sh, ray_o, ray_d, bt, best);
				has = true;
				if (!sh.n_bvh_nodes || best >= 0) { // nothing to walk: the round below finds the stack empty
					w.budget = 0;
					w.next = kBvhNone;
				}
			}
		}
		if (__ballot(has) == 0ull) {
			if (exhausted) break;
			continue; // (every lane idle and entries left: the refill above runs again)
		}
		// ---- one round of every lane's walk, the loop body of intersect(): down through nodes to a leaf
		// (the wave stays in the node loop until all its lanes have left it), the leaf's triangles, the
		// next candidate from the stack ----
		if (has) {
			bool done = false;
			while (!(w.next & kBvhLeafBit) && w.budget > 0) { // (see intersect)
				bvh_node_step<false, true>(w, sh, stk);
				if (w.next == kBvhNone) bvh_pop<true>(w, stk);
			}
			if (w.next != kBvhNone && (w.next & kBvhLeafBit)) {
				bvh_leaf_step(w, sh, tri_base);
				if (w.best >= 0) done = true; // a shadow ray needs one occluder, not the nearest
			}
			if (!done) {
				bvh_pop<true>(w, stk);
				if (w.next == kBvhNone) done = true;
			}
			if (done) {
				wsputu(a, WS_OCC, my, w.best >= 0 ? 1u : 0u);
				has = false;
			}
		}
	}
}

// ---- what k_wave_shade_a hands k_wave_guide, k_wave_cast and k_wave_shade_b through the workspace: stage_a's results, and which
// lane class finds what in which plane.  ws_load_stage_a is k_wave_shade_b's side of ws_store_stage_a, condition by condition ----
template <int kLevel, bool kGuide>
__device__ __forceinline__ void ws_store_stage_a(const RenderArgs &a, uint64_t tid, const StageA &A)
{
	// (storing a value for some lanes of a wave only saves nothing by itself -- the partial store touches the same
	// sectors -- which is why the two classes of lanes share planes instead: WS_U; making every lane store so that no
	// line is written in part was measured too: no different, 84.0 vs 84.8 ms per step)
	wsput3(a, WS_P, tid, A.p); wsput3(a, WS_NG, tid, A.ng);
	wsputu(a, WS_FLAGS, tid, A.flags);
	if (A.flags & F_SMP_TREE) { // (see WS_U)
		wsput3(a, WS_U, tid, A.n); wsput3(a, WS_U + 3, tid, A.wi); wsputu(a, WS_U + 6, tid, (uint32_t)A.mat);
		wsput3(a, WS_U + 7, tid, A.refl);
	} else {
		wsput3(a, WS_U, tid, A.wo); wsput3(a, WS_U + 3, tid, A.bsdf_w); wsput(a, WS_U + 6, tid, A.bsdf_pdf);
	}
	if (A.flags & F_HAS_LE) wsput3(a, WS_LE, tid, A.Le);
	if (!kGuide) wsput3(a, WS_DS_D, tid, A.ds_d); // (only k_wave_guide reads it)
	if (A.flags & F_NEE_LIVE) { // (what k_wave_shade_b reads of an emitter sample only when it can contribute)
		wsput(a, WS_DS_PDF, tid, A.ds_pdf); wsput3(a, WS_EM_W, tid, A.em_w);
		wsput3(a, WS_BV_EM, tid, A.bv_em); wsput(a, WS_BP_EM, tid, A.bp_em);
	}
	if (A.flags & F_NEED_SHADOW) {
		wsput3(a, WS_SH_O, tid, A.sh_o); wsput3(a, WS_SH_D, tid, A.sh_d); wsput(a, WS_SH_T, tid, A.sh_tmax);
	}
	if (kLevel >= 3) wsput(a, WS_ETA, tid, A.eta); // (:357: only the dielectrics of level 3 have an eta other than 1)
}
template <int kLevel>
__device__ __forceinline__ void ws_load_stage_a(const RenderArgs &a, uint64_t tid, StageA &A)
{
	A.flags = wsu(a, WS_FLAGS, tid);
	A.p = ws3(a, WS_P, tid); A.ng = ws3(a, WS_NG, tid);
	A.n = V(0, 0, 1); A.wi = V(0, 0, 1); A.mat = 0; A.refl = V(0, 0, 0);
	if (A.flags & F_SMP_TREE) { // (only these lanes evaluate their BSDF again)
		A.n = ws3(a, WS_U, tid); A.wi = ws3(a, WS_U + 3, tid);
		A.mat = (int)wsu(a, WS_U + 6, tid); A.refl = ws3(a, WS_U + 7, tid);
	}
	A.Le = (A.flags & F_HAS_LE) ? ws3(a, WS_LE, tid) : V(0, 0, 0);
	A.ds_d = V(0, 0, 0); // (stage_b does not read it: the record takes the canonical form k_wave_guide made)
	A.ds_pdf = 0.0f; A.em_w = V(0, 0, 0); A.bv_em = V(0, 0, 0); A.bp_em = 0.0f;
	if (A.flags & F_NEE_LIVE) {
		A.ds_pdf = wsf(a, WS_DS_PDF, tid); A.em_w = ws3(a, WS_EM_W, tid);
		A.bv_em = ws3(a, WS_BV_EM, tid); A.bp_em = wsf(a, WS_BP_EM, tid);
	}
	// (a tree-sampling lane's own BSDF sample is not used again: its direction comes from k_wave_guide, its
	// value and pdf from the evaluation in stage_b -- only the sample's eta is, :357)
	A.wo = V(0, 0, 0); A.bsdf_pdf = 0.0f; A.bsdf_w = V(0, 0, 0);
	if (A.flags & F_SMP_TREE) A.wo = ws3(a, WS_WO_T, tid);
	else { A.wo = ws3(a, WS_U, tid); A.bsdf_w = ws3(a, WS_U + 3, tid); A.bsdf_pdf = wsf(a, WS_U + 6, tid); }
	A.eta = kLevel >= 3 ? wsf(a, WS_ETA, tid) : 1.0f;
}

// ---- :189-220, 272-297 ----
// kGuide: the SD-tree calls of the bounce (stage_guide, otherwise k_wave_guide's) follow in the same kernel
template <int kLevel, bool kFirst, bool kGuide>
__global__ __launch_bounds__(kRBlock) void k_wave_shade_a(RenderArgs a)
{
	__shared__ float s_planes[kGuide ? 3 * kKdGridPlanes : 1];
	uint64_t tid;
	bool alive;
	if (!wave_entry<kFirst>(a, tid, alive)) return;
	if (kGuide) stage_kd_planes(s_planes, a.tree);
	if (!alive) return;
	Pcg32 rng;
	v3 ray_o, ray_d, thr = V(1, 1, 1), prev_p = V(0, 0, 0);
	float prev_pdf = 1.0f;
	bool prev_delta = true;
	HitRec h;
	if (!kFirst && a.perm) {
		// a sorted bounce: this thread serves the place the sort put k-th.  The one random pass over the state: the
		// path's record (k_wave_shade_b and k_wave_trace filled it) is one cache line; what k_wave_guide and
		// k_wave_shade_b need of it travels on at k (WS_FWD), so that nothing after this kernel looks through the permutation
		const uint4 *rec = st_rec(a.carry_in, tid < (uint64_t)a.n_sort ? (uint64_t)a.perm[tid] : tid);
		const uint4 q0 = rec[PS_RAY_O], q1 = rec[PS_RAY_D], q2 = rec[PS_THR], q3 = rec[PS_PREV], q4 = rec[PS_L], q5 = rec[PS_INC], q6 = rec[PS_HIT];
		rng.state = st_u64(q0.w, q1.w);
		rng.inc = st_u64(q5.x, q5.y);
		ray_o = st_v3(q0); ray_d = st_v3(q1);
		thr = st_v3(q2);
		prev_delta = st_delta(q2);
		prev_p = st_v3(q3);
		prev_pdf = st_wf(q3);
		h = st_hit(q6);
		ws_fwd_store(a, tid, q2, q4, q5);
	} else {
		const uint4 q0 = st_load(a.st_in, a, PS_RAY_O, tid), q1 = st_load(a.st_in, a, PS_RAY_D, tid);
		rng.state = st_u64(q0.w, q1.w);
		rng.inc = a.inc_in[tid];
		ray_o = st_v3(q0); ray_d = st_v3(q1);
		if (!kFirst) {
			const uint4 q2 = st_load(a.st_in, a, PS_THR, tid), q3 = st_load(a.st_in, a, PS_PREV, tid);
			thr = st_v3(q2);
			prev_delta = st_delta(q2);
			prev_p = st_v3(q3);
			prev_pdf = st_wf(q3);
		}
		h = ws_hit(a, tid);
	}
	StageA A;
	stage_a<kLevel>(a, rng, ray_o, ray_d, thr, prev_p, prev_pdf, prev_delta, h, (uint32_t)a.bounce, A);
	ws_store_stage_a<kLevel, kGuide>(a, tid, A);
	if (kGuide && guide_has_work(a, A.flags)) { // what k_wave_guide does, with its inputs still in registers
		GuideOut g;
		stage_guide(a, s_planes, rng, A.p, A.ds_d, (A.flags & F_SMP_TREE) ? V(0, 0, 0) : A.wo, A.flags, g);
		if (a.record && (A.flags & F_VALID)) store_slots(a, (kFirst ? 0 : records_before(a)) + tid, g);
		wsput(a, WS_PDF_NEE, tid, g.pdf_nee); wsput(a, WS_PDF_TREE, tid, g.pdf_tree);
		if (A.flags & F_SMP_TREE) wsput3(a, WS_WO_T, tid, g.wo);
	}
	wsputu(a, WS_RNG_LO, tid, (uint32_t)rng.state); wsputu(a, WS_RNG_HI, tid, (uint32_t)(rng.state >> 32));
}

// ---- :244, 301, 307 ----
// kGeo (pg_render_record_geometry): the vertex's geometry goes into geo.planes beside its accumulators (store_geo_position).
// The switch is a parameter of the KERNEL, and the default instantiation takes an empty second argument: a body shared by two
// kernels through a wrapper came out of the compiler with other code for the default one (k_wave_tail<2>: other registers).
template <bool kGeo> struct GeoArg {};
template <> struct GeoArg<true> { uint32_t *planes; };
template <bool kGeo = false>
__global__ __launch_bounds__(kRBlock) void k_wave_guide(RenderArgs a, GeoArg<kGeo> geo)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	uint64_t tid;
	bool alive;
	if (a.bounce == 0) { if (!wave_entry<true>(a, tid, alive)) return; }
	else if (!wave_entry<false>(a, tid, alive)) return;
	// The lane's inputs are ASKED FOR first -- together with its flags and ahead of the staging of the KD planes (round 6: the
	// listing showed staging -> barrier -> flags -> wait -> branch -> inputs -> wait, three round trips at the head of every
	// wave where one does): the planes hold a value for every live place, a lane without work throws its copies away.  (The
	// empty asm behind the barrier keeps the loads where they are written; the compiler would sink them into the branch.)
	// (unconditional: a load under a per-lane condition is merged with its default behind the branch, and that merge waits for
	// the load -- a lane past the list reads place 0's values, the list is not empty, and leaves below)
	const uint64_t it = alive ? tid : 0;
	const uint32_t flags = wsu(a, WS_FLAGS, it);
	v3 p_in = ws3(a, WS_P, it), ds_in = ws3(a, WS_DS_D, it), u_in = ws3(a, WS_U, it);
	uint32_t rng_lo = wsu(a, WS_RNG_LO, it), rng_hi = wsu(a, WS_RNG_HI, it);
	stage_kd_planes(s_planes, a.tree);
	if (!alive) return;
	asm volatile("" : "+v"(p_in.x), "+v"(p_in.y), "+v"(p_in.z), "+v"(ds_in.x), "+v"(ds_in.y), "+v"(ds_in.z), "+v"(u_in.x), "+v"(u_in.y),
	                  "+v"(u_in.z), "+v"(rng_lo), "+v"(rng_hi));
	if (!guide_has_work(a, flags)) return;
	Pcg32 rng;
	rng.state = st_u64(rng_lo, rng_hi);
	rng.inc = ws_fwd_inc(a, tid);
	GuideOut g;
	// (the BSDF-sampled direction of a lane that keeps it; a lane that samples the tree has none to evaluate)
	const v3 wo_in = (flags & F_SMP_TREE) ? V(0, 0, 0) : u_in;
	if constexpr (kGeo) {
		if (a.record && (flags & F_VALID)) store_geo_position(a, geo.planes, (a.bounce > 0 ? records_before(a) : 0) + tid, p_in);
	}
	stage_guide(a, s_planes, rng, p_in, ds_in, wo_in, flags, g);
	if (a.record && (flags & F_VALID)) store_slots(a, (a.bounce > 0 ? records_before(a) : 0) + tid, g); // the entry k_wave_shade_b fills for this vertex
	if constexpr (kGeo) {
		if (a.record && (flags & F_VALID)) store_geo_directions(a, geo.planes, (a.bounce > 0 ? records_before(a) : 0) + tid, g, (uint32_t)a.bounce);
	}
	wsput(a, WS_PDF_NEE, tid, g.pdf_nee); wsput(a, WS_PDF_TREE, tid, g.pdf_tree);
	if (flags & F_SMP_TREE) {
		wsput3(a, WS_WO_T, tid, g.wo);
		wsputu(a, WS_RNG_LO, tid, (uint32_t)rng.state); wsputu(a, WS_RNG_HI, tid, (uint32_t)(rng.state >> 32));
	}
}

// The survivors of a workgroup go to the next live list with their state (k_wave_shade_b, k_wave_shade): every thread of
// the workgroup calls this.  s_rec: kStage * 8 entries of LDS when the next bounce is sorted (a.carry_out), else unused.
template <int kStage>
__device__ __forceinline__ void append_survivors(const RenderArgs &a, bool cont, v3 ray_o, v3 ray_d, v3 thr, float ior, bool delta, v3 p_here,
                                                 float prev_pdf, v3 L, uint64_t lane, const Pcg32 &rng, uint32_t *s_wave, uint32_t &s_base,
                                                 uint32_t (*s_oct)[8], uint4 *s_rec)
{
	// entry k of the survivor's state (the path-state table above): the record takes all eight, the planes the first five
	const auto entry = [&](int k) {
		switch (k) {
		case PS_RAY_O: return st_q(ray_o, (uint32_t)rng.state);
		case PS_RAY_D: return st_q(ray_d, (uint32_t)(rng.state >> 32));
		case PS_THR: return st_q(thr, st_pack_ior(ior, delta));
		case PS_PREV: return st_q(p_here, __float_as_uint(prev_pdf));
		case PS_L: return st_q(L, (uint32_t)lane);
		case PS_INC: return make_uint4((uint32_t)rng.inc, (uint32_t)(rng.inc >> 32), 0u, 0u);
		default: return make_uint4(0u, 0u, 0u, 0u); // (PS_HIT: k_wave_trace; PS_SPARE)
		}
	};
	if (a.last) return; // nothing survives the last bounce
	const unsigned long long ballot = __ballot(cont);
	const unsigned wl = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	if (wl == 0) s_wave[wv] = (uint32_t)__popcll(ballot);
	// The survivors of a workgroup are appended grouped by the octant of their next direction (the order inside a
	// workgroup is free): on a sorted bounce the workgroup holds neighbours in space, and a wave of the next closest-hit
	// launch then walks the BVH from one corner in one direction -- k_wave_trace 17.5 -> 16.4 ms per step (two of the three
	// signs, so that a bin fills a wave: 16.7).  In list order the grouping changes nothing (round 2 measured that).
	const unsigned oct = (__float_as_uint(ray_d.x) >> 31) | ((__float_as_uint(ray_d.y) >> 31) << 1) | ((__float_as_uint(ray_d.z) >> 31) << 2);
	uint32_t rank_in_bin = 0;
	for (unsigned k = 0; k < 8; ++k) {
		const unsigned long long m = __ballot(cont && oct == k);
		if (wl == 0) s_oct[wv][k] = (uint32_t)__popcll(m);
		if (oct == k) rank_in_bin = (uint32_t)__popcll(m & ((1ull << wl) - 1ull));
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t tot = 0;
		for (int w = 0; w < kRBlock / 64; ++w) tot += s_wave[w];
		s_base = tot ? atomicAdd(&a.live_count[a.bounce], tot) : 0u;
	}
	__syncthreads();
	uint32_t off = s_base + rank_in_bin; // the survivor's place in the next list (whole lines: a wave's survivors are neighbours)
	if (cont) {
		for (unsigned k = 0; k < oct; ++k)
			for (unsigned w = 0; w < kRBlock / 64; ++w) off += s_oct[w][k]; // (every earlier bin of the workgroup)
		for (unsigned w = 0; w < wv; ++w) off += s_oct[w][oct];           // (this bin, the earlier waves)
	}
	if (a.carry_out) {
		// the next bounce is sorted: the state goes into ONE record per path and nowhere else -- the kernel that
		// looks through the permutation reads it as one cache line; k_wave_trace takes the ray from it and adds the hit.
		// The records are written as WHOLE lines, all 128 bytes of each, by consecutive threads, through LDS, kStage
		// records at a time: 96 of the 128 bytes -- by the lanes themselves or through LDS alike -- cost k_wave_shade_b
		// 13.6 -> 18.4 ms per step.  A line written in part is read, merged and written back.
		uint32_t tot = 0;
		for (int w = 0; w < kRBlock / 64; ++w) tot += s_wave[w];
		const uint32_t idx = cont ? off - s_base : 0xffffffffu;
		uint4 *dst = st_rec(a.carry_out, s_base);
		for (uint32_t h = 0; h < tot; h += (uint32_t)kStage) { // (uniform over the workgroup)
			if (h) __syncthreads(); // (the round before has been copied out)
			if (idx >= h && idx < h + (uint32_t)kStage) {
				uint4 *rec = st_rec(s_rec, idx - h);
#pragma unroll
				for (int k = 0; k < PS_ENTRIES; ++k) rec[k] = entry(k);
			}
			__syncthreads();
			const uint32_t n = tot - h < (uint32_t)kStage ? tot - h : (uint32_t)kStage;
			for (uint32_t j = threadIdx.x; j < n * PS_ENTRIES; j += kRBlock) { // (streaming stores: see PG_ST)
				const uint4 q = s_rec[j];
				const u32x4_t v = {q.x, q.y, q.z, q.w};
				__builtin_nontemporal_store(v, reinterpret_cast<u32x4_t *>(st_rec(dst, h) + j));
			}
		}
	} else if (cont) {
#pragma unroll
		for (int k = 0; k < PS_INC; ++k) st_store(a.st_out, a, k, off, entry(k));
		a.inc_out[off] = rng.inc;
	}
}

// ---- :247-261, 302-381 ----
template <int kLevel, bool kFirst>
__global__ __launch_bounds__(kRBlock) void k_wave_shade_b(RenderArgs a)
{
	__shared__ uint32_t s_wave[kRBlock / 64];
	__shared__ uint32_t s_base;
	__shared__ uint32_t s_oct[kRBlock / 64][8];
	extern __shared__ uint4 s_rec[]; // kRBlock * 8 entries when the next bounce is sorted (a.carry_out), else none
	uint64_t tid;
	bool alive;
	if (!wave_entry<kFirst>(a, tid, alive)) return;
	const uint64_t rec_base = kFirst ? 0 : records_before(a);
	bool cont = false;
	// what a survivor takes along to its place in the next list
	v3 ray_o = V(0, 0, 0), ray_d = V(0, 0, 1), thr = V(1, 1, 1), L = V(0, 0, 0), p_here = V(0, 0, 0);
	float ior = 1.0f, prev_pdf = 1.0f;
	bool delta = false;
	uint64_t lane = tid; // (the first list is in lane order)
	Pcg32 rng;
	rng.state = 0; rng.inc = 1;
	if (alive) {
		StageA A;
		ws_load_stage_a<kLevel>(a, tid, A);
		// (the accumulators: k_wave_guide has put them into the record list; its direction for the lanes that sample the tree)
		GuideOut g = guide_none(A.wo);
		if (guide_has_work(a, A.flags)) { g.pdf_nee = wsf(a, WS_PDF_NEE, tid); g.pdf_tree = wsf(a, WS_PDF_TREE, tid); }
		const bool occluded = (A.flags & F_NEED_SHADOW) && wsu(a, WS_OCC, tid) != 0u;
		rng.state = st_u64(wsu(a, WS_RNG_LO, tid), wsu(a, WS_RNG_HI, tid));
		rng.inc = ws_fwd_inc(a, tid);
		if (!kFirst) {
			uint4 q2, q4;
			if (a.perm) { // (a sorted bounce: k_wave_shade_a has brought them along)
				q2 = ws4(a, WS_FWD_THR, tid);
				q4 = ws4(a, WS_FWD_L, tid);
			} else {
				q2 = st_load(a.st_in, a, PS_THR, tid);
				q4 = st_load(a.st_in, a, PS_L, tid);
			}
			thr = st_v3(q2);
			ior = st_ior(q2);
			L = st_v3(q4);
			lane = st_lane(q4);
		}
		cont = stage_b<kLevel>(a, rng, thr, L, ior, A, g, occluded, lane, rec_base + tid, (uint32_t)a.bounce, ray_o, ray_d,
		                       prev_pdf, delta);
		p_here = A.p;
		if (kFirst) a.hit0[lane] = (A.flags & F_VALID) ? 1 : 0;
		if (!cont) end_path(a, lane, L);
	}
	append_survivors<kRBlock>(a, cont, ray_o, ray_d, thr, ior, delta, p_here, prev_pdf, L, lane, rng, s_wave, s_base, s_oct, s_rec);
}

// ---- :189-381 in one kernel: everything of a bounce but the closest hit ----
// stage_a, the SD-tree calls, the shadow ray (an any-hit walk inline) and stage_b on one lane's registers: none of the
// workspace planes the split kernels hand each other is written or read -- about 360 of the 900 bytes a lane and bounce move
// through HBM.  The price: the shadow ray is walked by the lane that made it (no handing of finished lanes' slots to other
// rays as in k_wave_cast), and the tree walks run at the occupancy the shading's registers leave.  LDS: the walk's stacks
// and the hottest BVH nodes, and -- over the same bytes, once every walk of the workgroup is done -- the survivors'
// records of a sorted next bounce.
constexpr int kShadeStage = 128; // survivors' records staged in LDS at a time (224 at a time: no gain, profiles/r05/ab_shade_stage224_rejected.txt)
// (kShadeTopNodes and kShadeStack, this kernel's share of LDS for the walk, are in pg_render_dev.hpp beside kBvhTopNodes)
// (the stash: the nine values of stage_a1 that only stage_b reads and the path's throughput; the radiance so far, the index of
// refraction and the lane stay in registers -- rounds 4-5 measured the other splits)
constexpr int kShadeStash = 12;
constexpr int kShadeWalkQuads = kShadeStack * kRBlock / 2 + kShadeTopNodes * kBvhNodeQuads + kShadeStash * kRBlock / 4;
constexpr int kShadeLdsQuads = kShadeStage * PS_ENTRIES > kShadeWalkQuads ? kShadeStage * PS_ENTRIES : kShadeWalkQuads;
// (122 vector registers, four waves per SIMD, which is also what 33 KB of LDS per workgroup allow.  Measured: staging the
// records 128 at a time -- 23 KB -- changes nothing by itself, and compiled for five waves on top of that the kernel spills
// 31 registers: 35.2 -> 37.6 ms per step.)
// The paths' 128-byte records of a sorted bounce are read THROUGH LDS by the wave as a whole: a lane that
// gathers the seven 16-byte entries of its own record makes seven vector loads that each touch 64 different cache lines --
// the compute unit's L1 looks up about one line per clock, so such a load holds the vector-memory path for 64 clocks however
// few bytes it wants -- where eight lanes that read one record's eight entries side by side touch 8 lines per load: the same
// 64 records in eight loads of 8 lines instead of seven of 64.  The entries cross to the lanes that own them through LDS
// ([entry][thread] planes over the bytes the walks' stacks and the stash use later: one more workgroup barrier, ahead of the
// staging of the BVH's top).
static_assert(PS_SPARE * kRBlock <= kShadeLdsQuads, "k_wave_shade: the records' seven entries per thread must fit the dynamic LDS");
template <int kLevel, bool kFirst>
__device__ __forceinline__ void shade_body(const RenderArgs &a)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	__shared__ uint32_t s_wave[kRBlock / 64];
	__shared__ uint32_t s_base;
	__shared__ uint32_t s_oct[kRBlock / 64][8];
	extern __shared__ uint4 s_dyn[]; // kShadeLdsQuads entries: [stacks kLdsStack * kRBlock * 8 B][BVH top][...], later the records
	uint64_t tid;
	bool alive;
	if (!wave_entry<kFirst>(a, tid, alive)) return;
	// Probe builds only (-DPG_SHADE_PHASES=1; the instrumented pass of such a build prints the shares under $PGSD_TRACE_SHADOW):
	// where a wave spends its life, DepthCounters::phase.  NOT in the product: the seven s_memtime stamps, behind a uniform
	// branch that is never taken in a timed pass, took k_wave_shade from 28.6 to 45-47 ms per step (profiles/r05/
	// ab_shade_early_staging.txt: every variant of that run carries them).
#ifndef PG_SHADE_PHASES
#define PG_SHADE_PHASES 0
#endif
#if PG_SHADE_PHASES
	// A wave keeps its stamps in its own row of LDS (one lane, plain stores: LDS operations of a wave complete in order) and
	// flushes the row once at the end, by one eight-lane atomic into its stripe.  (Round 5's probe added every stamp to ONE line
	// of device memory: its k_wave_shade ran eleven times slower than the product's.  And what made a probe build 1.7 times
	// slower even with its stamps idle was not the stamps at all: see live_final(), pg_render_dev.hpp.  With both repaired this
	// build's k_wave_shade takes 27.7 ms per step against the product's 27.5, stamping or not: profiles/r06/phase_probe.txt.)
	// Seven stamps behind the start: 0 the records + staging, 1 stage_a1, 2 the shadow walk, 3 stage_a2, 4 the SD-tree calls, 5 stage_b,
	// 6 the survivors' append (pg_kernels.hpp).
	__shared__ unsigned long long s_ph[kRBlock / 64][10]; // [0..6] the phases, [7] stamps taken, [8] the last stamp
	if ((threadIdx.x & 63u) == (unsigned)__builtin_ctzll(__ballot(1))) {
		s_ph[threadIdx.x >> 6][8] = (unsigned long long)clock64();
		s_ph[threadIdx.x >> 6][7] = 0ull;
	}
#define PG_PHASE(i)                                                                                                          \
	if (a.ph && (threadIdx.x & 63u) == (unsigned)__builtin_ctzll(__ballot(1))) {                                            \
		const unsigned long long t_now = (unsigned long long)clock64();                                                      \
		unsigned long long *row = s_ph[threadIdx.x >> 6];                                                                    \
		row[i] = t_now - row[8];                                                                                             \
		row[8] = t_now;                                                                                                      \
		row[7] |= 1ull << (i);                                                                                               \
	}
#else
#define PG_PHASE(i)
#endif
	// What the workgroup stages in LDS -- the KD grid's planes and the BVH's top -- is ASKED FOR first and written last: the loads
	// are in flight while the records make their own two round trips (the permutation, then the entries), instead of being
	// two more round trips behind them, each with a barrier of its own (an instrumented pass showed a quarter of a wave's life
	// gone before stage_a1 began: profiles/r05/shade_phases.txt).
	constexpr int kPlaneLoads = 1, kTopLoads = (kShadeTopNodes * kBvhNodeQuads + kRBlock - 1) / kRBlock;
	float pl_pre[kPlaneLoads];
	u32x4_t top_pre[kTopLoads];
#pragma unroll
	for (int k = 0; k < kPlaneLoads; ++k) pl_pre[k] = 0.0f;
#pragma unroll
	for (int k = 0; k < kTopLoads; ++k) top_pre[k] = u32x4_t{0u, 0u, 0u, 0u};
	const uint32_t n_top = a.shapes.n_bvh_nodes < kShadeTopNodes ? (uint32_t)a.shapes.n_bvh_nodes : (uint32_t)kShadeTopNodes;
#pragma unroll
	for (int k = 0; k < kPlaneLoads; ++k)
		if (a.tree.kd_grid != nullptr && threadIdx.x + k * kRBlock < 3u * kKdGridPlanes) pl_pre[k] = a.tree.kd_planes[threadIdx.x + k * kRBlock];
#pragma unroll
	for (int k = 0; k < kTopLoads; ++k)
		if (threadIdx.x + k * kRBlock < n_top * 8u) top_pre[k] = reinterpret_cast<const u32x4_t *>(a.shapes.bvh)[threadIdx.x + k * kRBlock];
	uint4 cq0 = make_uint4(0u, 0u, 0u, 0u), cq1 = cq0, cq2 = cq0, cq3 = cq0, cq4 = cq0, cq5 = cq0, cq6 = cq0;
	uint32_t coop_place = (uint32_t)tid;
	const bool coop = !kFirst && a.perm != nullptr; // (uniform)
	if (coop) {
		if (alive && tid < (uint64_t)a.n_sort) coop_place = a.perm[tid];
		if (!alive) coop_place = 0u; // (a lane past the list still serves its wave's loads: any record that exists)
		const uint32_t l = threadIdx.x & 63u, wbase = threadIdx.x & ~63u, q = l & 7u;
		// ALL EIGHT gathers are issued before the first of them is waited for (round 6).  Written as one loop -- gather, then store
		// under `q < 7` -- every round was a basic block of its own: permute, wait, gather, WAIT, store, eight round trips one
		// after the other at the head of every wave (the ISA showed it: eight `s_waitcnt vmcnt(0)` in a row).  The gather is
		// unconditional now (entry 7 of a record is its unused tail, in the same 128-byte line as the rest: loaded, not kept),
		// so nothing splits the loop, and the stores follow in a loop of their own.
		uint4 g[8];
#pragma unroll
		for (uint32_t k = 0; k < 8u; ++k) {
			const uint32_t j = k * 8u + (l >> 3);
			const uint32_t pj = (uint32_t)__shfl((int)coop_place, (int)j, 64);
			g[k] = gather16(st_rec(a.carry_in, pj, (int)q));
		}
#pragma unroll
		for (uint32_t k = 0; k < 8u; ++k)
			if (q < (uint32_t)PS_SPARE) s_dyn[q * kRBlock + wbase + k * 8u + (l >> 3)] = g[k];
		// (written and read by the same wave: its LDS operations complete in order, so no workgroup barrier -- but the lanes read
		// entries OTHER lanes wrote, which the memory model only orders through a release / acquire pair at wavefront scope; the
		// fences and the wave barrier emit no instruction, they pin the order for the compiler: ADVICE r5)
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		cq0 = s_dyn[PS_RAY_O * kRBlock + threadIdx.x]; cq1 = s_dyn[PS_RAY_D * kRBlock + threadIdx.x]; cq2 = s_dyn[PS_THR * kRBlock + threadIdx.x];
		cq3 = s_dyn[PS_PREV * kRBlock + threadIdx.x]; cq4 = s_dyn[PS_L * kRBlock + threadIdx.x]; cq5 = s_dyn[PS_INC * kRBlock + threadIdx.x];
		cq6 = s_dyn[PS_HIT * kRBlock + threadIdx.x];
		__syncthreads(); // every wave has its entries: the bytes become the BVH's top, the stacks and the stash
	}
	uint2 *s_stack = reinterpret_cast<uint2 *>(s_dyn);
	u32x4_t *s_top = reinterpret_cast<u32x4_t *>(s_dyn) + kShadeStack * kRBlock / 2;
	BvhStack stk = bvh_stack(s_stack + threadIdx.x, a.bvh_ovf, (uint32_t)tid * (uint32_t)kOvfStack, kShadeStack);
#pragma unroll
	for (int k = 0; k < kPlaneLoads; ++k)
		if (a.tree.kd_grid != nullptr && threadIdx.x + k * kRBlock < 3u * kKdGridPlanes) s_planes[threadIdx.x + k * kRBlock] = pl_pre[k];
	if (a.tree.kd_grid != nullptr) // (a workgroup smaller than the planes' count -- variant builds -- takes the rest here)
		for (uint32_t i = threadIdx.x + kPlaneLoads * kRBlock; i < 3u * kKdGridPlanes; i += kRBlock) s_planes[i] = a.tree.kd_planes[i];
#pragma unroll
	for (int k = 0; k < kTopLoads; ++k)
		if (threadIdx.x + k * kRBlock < n_top * 8u) s_top[threadIdx.x + k * kRBlock] = top_pre[k];
	__syncthreads();
	stk.top = (const LdsQuad *)s_top;
	stk.n_top = n_top;
	bool cont = false;
	v3 ray_o = V(0, 0, 0), ray_d = V(0, 0, 1), thr = V(1, 1, 1), L = V(0, 0, 0), p_here = V(0, 0, 0), prev_p = V(0, 0, 0);
	float ior = 1.0f, prev_pdf = 1.0f;
	bool delta = false, prev_delta = true;
	uint64_t lane = tid; // (the first list is in lane order)
	Pcg32 rng;
	rng.state = 0; rng.inc = 1;
	uint64_t rec_base = 0;
	if (!kFirst) {
		rec_base = records_before(a);
		// (the same number in every lane, but read by vector loads -- live_count is written by this very grid -- so the
		// compiler keeps it in two vector registers through the whole kernel unless it is told that it is uniform)
		rec_base = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)rec_base) |
		           ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(rec_base >> 32)) << 32);
	}
	if (alive) {
		// What a path carries from bounce to bounce is read ONCE, here: the ray, the sampler, the hit, the throughput, the index
		// of refraction, the radiance so far and the path's lane.  (Reading the last four a second time behind the walks, to keep
		// them out of the walks' registers, cost 1.25 ms per step -- two more gathers per lane; they wait in registers and, the
		// throughput, in the LDS stash: DESIGN 5.7.)
		HitRec h;
		const bool from_rec = !kFirst && a.perm != nullptr; // a sorted bounce: the path's 128-byte record, through the permutation
		uint32_t place = (uint32_t)tid; // (32-bit: a place in the live list; one register through the walks, not two)
		if (!coop && from_rec && tid < (uint64_t)a.n_sort) place = a.perm[tid];
		if (kFirst) {
			// The camera bounce: the ray is a function of the lane number, so it is made and walked HERE, on this kernel's own
			// stack and LDS top (the slim walk, as the shadow ray's below) -- ray, sampler and hit never leave the registers.  No
			// k_wave_trace runs ahead of this launch and nothing of st_in / inc_in / the hit planes is read or written: the next
			// bounce's set is written by append_survivors as ever.  Nothing else of a path is alive yet, so the walk is far from
			// the kernel's register peak.
			camera_ray(a, tid, rng, ray_o, ray_d);
			h.u = 0.0f; h.v = 0.0f;
			h.prim = intersect<kLevel, false, true>(a.shapes, ray_o, ray_d, __builtin_huge_valf(), h.t, stk, h.u, h.v);
		} else if (from_rec) {
			const uint4 *rec = st_rec(a.carry_in, place);
			uint4 q0, q1, q2, q3, q5, q6;
			if (coop) { q0 = cq0; q1 = cq1; q2 = cq2; q3 = cq3; q5 = cq5; q6 = cq6; }
			else { q0 = rec[PS_RAY_O]; q1 = rec[PS_RAY_D]; q2 = rec[PS_THR]; q3 = rec[PS_PREV]; q5 = rec[PS_INC]; q6 = rec[PS_HIT]; }
			rng.state = st_u64(q0.w, q1.w);
			rng.inc = st_u64(q5.x, q5.y);
			ray_o = st_v3(q0); ray_d = st_v3(q1);
			thr = st_v3(q2);
			{ const uint4 q4 = coop ? cq4 : rec[PS_L]; ior = st_ior(q2); L = st_v3(q4); lane = st_lane(q4); }
			prev_delta = st_delta(q2);
			prev_p = st_v3(q3);
			prev_pdf = st_wf(q3);
			h = st_hit(q6);
		} else {
			const uint4 q0 = st_load(a.st_in, a, PS_RAY_O, tid), q1 = st_load(a.st_in, a, PS_RAY_D, tid);
			rng.state = st_u64(q0.w, q1.w);
			rng.inc = a.inc_in[tid];
			ray_o = st_v3(q0); ray_d = st_v3(q1);
			const uint4 q2 = st_load(a.st_in, a, PS_THR, tid), q3 = st_load(a.st_in, a, PS_PREV, tid);
			thr = st_v3(q2);
			{ const uint4 q4 = st_load(a.st_in, a, PS_L, tid); ior = st_ior(q2); L = st_v3(q4); lane = st_lane(q4); }
			prev_delta = st_delta(q2);
			prev_p = st_v3(q3);
			prev_pdf = st_wf(q3);
			h = ws_hit(a, tid);
		}
		StageA A;
		PG_PHASE(0) // (in the first launch the camera ray's closest-hit walk falls into this phase, "records + staging")
		stage_a1<kLevel>(a, rng, ray_o, ray_d, thr, prev_p, prev_pdf, prev_delta, h, (uint32_t)a.bounce, A);
		// What stage_a1 leaves is PINNED here: every output is made now, so that its inputs die.  (Left alone the compiler
		// sinks the last operations of a value that is only read behind the walk -- the emitted radiance's three products, the
		// flag word's bits -- below the walk, and carries their more numerous inputs through it instead.)
		asm volatile("" : "+v"(A.flags), "+v"(A.wi.x), "+v"(A.wi.y), "+v"(A.wi.z), "+v"(A.p.x), "+v"(A.p.y), "+v"(A.p.z),
		                  "+v"(A.ng.x), "+v"(A.ng.y), "+v"(A.ng.z), "+v"(A.refl.x), "+v"(A.refl.y), "+v"(A.refl.z));
		asm volatile("" : "+v"(A.ds_d.x), "+v"(A.ds_d.y), "+v"(A.ds_d.z), "+v"(A.ds_pdf), "+v"(A.bp_em), "+v"(A.n.x), "+v"(A.n.y), "+v"(A.n.z));
		// nine values only stage_b reads wait in LDS while the two walks run (column threadIdx.x of a [9][kRBlock] array)
		float *stash = reinterpret_cast<float *>(s_dyn) + (kShadeStack * kRBlock * 2 + kShadeTopNodes * 32) + threadIdx.x;
		stash[0 * kRBlock] = A.Le.x; stash[1 * kRBlock] = A.Le.y; stash[2 * kRBlock] = A.Le.z;
		stash[3 * kRBlock] = A.bv_em.x; stash[4 * kRBlock] = A.bv_em.y; stash[5 * kRBlock] = A.bv_em.z;
		stash[6 * kRBlock] = A.em_w.x; stash[7 * kRBlock] = A.em_w.y; stash[8 * kRBlock] = A.em_w.z;
		// ... and with them what the path carries that only stage_b needs: throughput, radiance so far, index of refraction, lane
		// (round-4 measurement: reading these a second time from the path's record cost 1.25 ms per step -- two more 16-byte
		// gathers per lane in a kernel whose time follows its gathers -- where eight LDS words cost nothing)
		stash[9 * kRBlock] = thr.x; stash[10 * kRBlock] = thr.y; stash[11 * kRBlock] = thr.z;
		// The shadow ray is walked HERE, between the two halves of stage_a: the BSDF sample is not made yet and the SD-tree
		// calls have no results yet, so neither is alive across the walk -- the walk's 50 registers on top of everything a
		// bounce keeps were this kernel's register peak (123 with the walk at the end).  The walk draws no
		// sample, so the sampler's order is untouched.
		bool occluded = false;
		PG_PHASE(1)
		if (a.dc) { // (instrumented passes only: how full are the waves that walk?)
			const unsigned long long m = __ballot((A.flags & F_NEED_SHADOW) != 0u);
			if ((threadIdx.x & 63u) == (unsigned)__builtin_ctzll(__ballot(1))) {
				atomicAdd(&a.dc->body_waves, 1ull);
				if (m) { atomicAdd(&a.dc->shadow_waves, 1ull); atomicAdd(&a.dc->shadow_lanes, (unsigned long long)__popcll(m)); }
			}
		}
		if (A.flags & F_NEED_SHADOW) { // :213 test_visibility
			float th, bu, bv;
			occluded = intersect<kLevel, true, true>(a.shapes, A.sh_o, A.sh_d, A.sh_tmax, th, stk, bu, bv) >= 0;
		}
		PG_PHASE(2)
		// (the shading frame and the material row are functions of the normal and the material's number: made again from
		// them behind the walk -- a dozen operations and two loads -- instead of being carried through it, which is what
		// the compiler does unless it is told that these ARE new values)
		asm volatile("" : "+v"(A.n.x), "+v"(A.n.y), "+v"(A.n.z), "+v"(A.mat));
		stage_a2<kLevel>(a, rng, A);
		// (stage_a2's outputs pinned like stage_a1's: the nine products of to_world() were carried through the SD-tree walks
		// instead of the three sums)
		asm volatile("" : "+v"(A.wo.x), "+v"(A.wo.y), "+v"(A.wo.z), "+v"(A.bsdf_w.x), "+v"(A.bsdf_w.y), "+v"(A.bsdf_w.z),
		                  "+v"(A.bsdf_pdf), "+v"(A.flags));
		if (kLevel >= 3) asm volatile("" : "+v"(A.eta));
		GuideOut g = guide_none(A.wo);
		PG_PHASE(3)
		if (guide_has_work(a, A.flags)) stage_guide(a, s_planes, rng, A.p, A.ds_d, (A.flags & F_SMP_TREE) ? V(0, 0, 0) : A.wo, A.flags, g);
		if (a.record && (A.flags & F_VALID)) store_slots(a, rec_base + tid, g);
		PG_PHASE(4)
		asm volatile("" : "+v"(A.n.x), "+v"(A.n.y), "+v"(A.n.z), "+v"(A.mat)); // (the same behind the SD-tree walks, for stage_b's second BSDF evaluation)
		A.Le = V(stash[0 * kRBlock], stash[1 * kRBlock], stash[2 * kRBlock]);
		A.bv_em = V(stash[3 * kRBlock], stash[4 * kRBlock], stash[5 * kRBlock]);
		A.em_w = V(stash[6 * kRBlock], stash[7 * kRBlock], stash[8 * kRBlock]);
		thr = V(stash[9 * kRBlock], stash[10 * kRBlock], stash[11 * kRBlock]);
		cont = stage_b<kLevel>(a, rng, thr, L, ior, A, g, occluded, lane, rec_base + tid, (uint32_t)a.bounce, ray_o, ray_d, prev_pdf, delta);
		p_here = A.p;
		if (kFirst) a.hit0[lane] = (A.flags & F_VALID) ? 1 : 0;
		if (!cont) end_path(a, lane, L);
		PG_PHASE(5)
	}
	// (append_survivors' first barrier comes after every walk of the workgroup: from there on the stacks' bytes hold records)
	append_survivors<kShadeStage>(a, cont, ray_o, ray_d, thr, ior, delta, p_here, prev_pdf, L, lane, rng, s_wave, s_base, s_oct, s_dyn);
	PG_PHASE(6)
#undef PG_PHASE
#if PG_SHADE_PHASES
	if (a.ph && (threadIdx.x & 63u) < 8u) { // the wave's row, once: eight lanes, one line of the wave's stripe
		const unsigned long long *row = s_ph[threadIdx.x >> 6];
		const unsigned l = threadIdx.x & 63u;
		// (a slot whose stamp this wave never passed -- a wave without a live lane skips the body -- holds nothing of this launch)
		const unsigned long long v = l == 7u ? 1ull : ((row[7] >> l) & 1ull) ? row[l] : 0ull;
		atomicAdd(&a.ph[(size_t)((blockIdx.x * (kRBlock / 64) + (threadIdx.x >> 6)) & (unsigned)(kPhaseStripes - 1)) * kPhaseWords + l], v);
	}
#endif
}

// (The probe build's stamps cost the level-2 kernel one register more than five waves per SIMD leave -- 97: four waves, and the
// kernel 15 % -- so it is told the occupancy, as the level-3 kernel below is: 96 registers and a few spilled bytes.  A probe
// must run at the product's occupancy to say anything about the product.)
#if PG_SHADE_PHASES
#define PG_PROBE_WAVES __attribute__((amdgpu_waves_per_eu(5)))
#else
#define PG_PROBE_WAVES
#endif
template <int kLevel, bool kFirst>
__global__ __launch_bounds__(kRBlock) PG_PROBE_WAVES void k_wave_shade(RenderArgs a)
{
	shade_body<kLevel, kFirst>(a);
}
// Feature level 3 (torus: transmission, delta lobes, one-sided BSDFs) needs three registers more than five waves per SIMD leave
// (99 of 96); told the occupancy it is wanted at, the compiler finds an allocation of 96 without a byte of scratch.  (The
// same hint makes the level-2 kernel, which fits by itself at 96, spill 12 bytes per lane: it is left alone.)
template <bool kFirst>
__global__ __launch_bounds__(kRBlock) __attribute__((amdgpu_waves_per_eu(5))) void k_wave_shade_l3(RenderArgs a)
{
	shade_body<3, kFirst>(a);
}

// See tail_checkpoint (pg_render_dev.hpp): launched before the launches of bounce a.bounce with a grid
// for kTailPaths lanes.  When no more paths than that are alive every lane follows its own path to
// its end here, all stages in sequence with their intermediate results in registers; the state still
// goes through the per-lane arrays only at the start.  Record entries of the later bounces are handed
// out wave by wave behind the entries of bounce a.bounce (a.live_count[max_depth] counts them), and
// the survivors of every bounce are added to live_count[] as the per-bounce launches would have.
// kGeo (pg_render_record_geometry): as k_wave_guide's
template <int kLevel, bool kGeo = false>
__global__ __launch_bounds__(kRBlock) void k_wave_tail(RenderArgs a, GeoArg<kGeo> geo)
{
	__shared__ uint2 s_stack[kLdsStack][kRBlock];
	__shared__ float s_planes[3 * kKdGridPlanes];
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	const uint64_t live = (uint64_t)live_final(a, a.bounce - 1);
	if (live > kTailPaths || (uint64_t)blockIdx.x * kRBlock >= live) return;
	if (tail_took_over(a, a.bounce - 1)) return; // an earlier checkpoint already did
	stage_kd_planes(s_planes, a.tree);
	bool alive = tid < live;
	uint64_t lane = 0;
	const uint64_t rec_base = records_before(a);
	const uint64_t tail_base = rec_base + live; // behind the entries of bounce a.bounce
	uint64_t slot = rec_base + tid;
	const BvhStack stk = bvh_stack(&s_stack[0][threadIdx.x], a.bvh_ovf, (uint32_t)tid * (uint32_t)kOvfStack);
	Pcg32 rng;
	v3 ray_o = V(0, 0, 0), ray_d = V(0, 0, 1), thr = V(0, 0, 0), L = V(0, 0, 0), prev_p = V(0, 0, 0);
	float prev_pdf = 1.0f, ior = 1.0f;
	bool prev_delta = false;
	rng.state = 0; rng.inc = 1;
	if (alive) {
		uint4 q0, q1, q2, q3, q4;
		if (a.carry_in) { // the bounce taken over would have been a sorted one: its state is in the paths' records
			const uint4 *rec = st_rec(a.carry_in, tid);
			q0 = rec[PS_RAY_O]; q1 = rec[PS_RAY_D]; q2 = rec[PS_THR]; q3 = rec[PS_PREV]; q4 = rec[PS_L];
			const uint4 q5 = rec[PS_INC];
			rng.inc = st_u64(q5.x, q5.y);
		} else {
			q0 = st_load(a.st_in, a, PS_RAY_O, tid); q1 = st_load(a.st_in, a, PS_RAY_D, tid); q2 = st_load(a.st_in, a, PS_THR, tid);
			q3 = st_load(a.st_in, a, PS_PREV, tid); q4 = st_load(a.st_in, a, PS_L, tid);
			rng.inc = a.inc_in[tid];
		}
		rng.state = st_u64(q0.w, q1.w);
		ray_o = st_v3(q0); ray_d = st_v3(q1); thr = st_v3(q2); prev_p = st_v3(q3);
		ior = st_ior(q2);
		prev_delta = st_delta(q2);
		prev_pdf = st_wf(q3);
		L = st_v3(q4);
		lane = st_lane(q4);
	}
	for (int depth = a.bounce; depth < a.max_depth; ++depth) {
		if (alive) {
			HitRec h;
			h.u = 0.0f; h.v = 0.0f;
			h.prim = intersect<kLevel, false>(a.shapes, ray_o, ray_d, __builtin_huge_valf(), h.t, stk, h.u, h.v);
			StageA A;
			stage_a<kLevel>(a, rng, ray_o, ray_d, thr, prev_p, prev_pdf, prev_delta, h, (uint32_t)depth, A);
			bool occluded = false;
			if (A.flags & F_NEED_SHADOW) {
				float th, bu, bv;
				occluded = intersect<kLevel, true>(a.shapes, A.sh_o, A.sh_d, A.sh_tmax, th, stk, bu, bv) >= 0;
			}
			GuideOut g = guide_none(A.wo);
			if constexpr (kGeo) {
				if (a.record && (A.flags & F_VALID)) store_geo_position(a, geo.planes, slot, A.p);
			}
			if (guide_has_work(a, A.flags)) stage_guide(a, s_planes, rng, A.p, A.ds_d, A.wo, A.flags, g);
			if (a.record && (A.flags & F_VALID)) store_slots(a, slot, g);
			if constexpr (kGeo) {
				if (a.record && (A.flags & F_VALID)) store_geo_directions(a, geo.planes, slot, g, (uint32_t)depth);
			}
			bool delta;
			alive = stage_b<kLevel>(a, rng, thr, L, ior, A, g, occluded, lane, slot, (uint32_t)depth, ray_o, ray_d, prev_pdf, delta);
			prev_p = A.p;
			prev_delta = delta;
			if (!alive) end_path(a, lane, L);
		}
		if (!tail_next_slot(a, depth, alive, tail_base, slot)) break;
	}
}

// The grid of a persistent kernel: as many workgroups as the device holds at once (the occupancy the
// register count of this instantiation allows, asked of the runtime once), never more than the rays need.
template <class K>
static dim3 persistent_grid(K kernel, unsigned &cached_per_cu, unsigned n_cus, uint64_t n_rays)
{
	if (cached_per_cu == 0) {
		int nb = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kRBlock, 0) != hipSuccess || nb < 1) nb = 4;
		cached_per_cu = (unsigned)nb;
	}
	uint64_t blocks = (uint64_t)cached_per_cu * n_cus;
	const uint64_t need = (n_rays + kRBlock - 1) / kRBlock;
	if (blocks > need) blocks = need;
	return dim3((unsigned)(blocks ? blocks : 1));
}

// ---- launcher: one stage of one bounce (pg_render_pass wraps each in its timing events) ----
template <int kLevel>
static void launch_stage_level(WaveStage stage, bool first, const RenderArgs &a, dim3 grid, unsigned n_cus, hipStream_t s, uint32_t *geo)
{
	const dim3 block(kRBlock);
	static unsigned occ[2] = {0, 0}; // resident workgroups per CU of the two shadow-ray instantiations of this level
	// (kF: the instantiation for the first bounce or the one for the later ones)
#define PG_BY_FIRST(launch) do { if (first) { constexpr bool kF = true; launch; } else { constexpr bool kF = false; launch; } } while (0)
	switch (stage) {
	case WaveStage::Trace: PG_BY_FIRST(hipLaunchKernelGGL((k_wave_trace<kLevel, kF>), grid, block, 0, s, a)); break;
	case WaveStage::ShadeA:
		if (a.fuse_guide) PG_BY_FIRST(hipLaunchKernelGGL((k_wave_shade_a<kLevel, kF, true>), grid, block, 0, s, a));
		else PG_BY_FIRST(hipLaunchKernelGGL((k_wave_shade_a<kLevel, kF, false>), grid, block, 0, s, a));
		break;
	case WaveStage::Cast:
		PG_BY_FIRST(hipLaunchKernelGGL((k_wave_cast<kLevel, kF>), persistent_grid(k_wave_cast<kLevel, kF>, occ[kF ? 0 : 1], n_cus, a.n_lanes), block, 0, s, a));
		break;
	case WaveStage::Guide: // (geo: a geometry-recording pass, pg_render_record_geometry -- its Guide and Tail launches only)
		if (geo) hipLaunchKernelGGL(k_wave_guide<true>, grid, block, 0, s, a, GeoArg<true>{geo});
		else hipLaunchKernelGGL(k_wave_guide<false>, grid, block, 0, s, a, GeoArg<false>{});
		break;
	case WaveStage::ShadeB: {
		const size_t lds = a.carry_out ? (size_t)kRBlock * PS_ENTRIES * sizeof(uint4) : 0; // (the survivors' records of a sorted next bounce)
		PG_BY_FIRST(hipLaunchKernelGGL((k_wave_shade_b<kLevel, kF>), grid, block, lds, s, a));
		break;
	}
	case WaveStage::Tail:
		if (geo) hipLaunchKernelGGL((k_wave_tail<kLevel, true>), grid, block, 0, s, a, GeoArg<true>{geo});
		else hipLaunchKernelGGL((k_wave_tail<kLevel, false>), grid, block, 0, s, a, GeoArg<false>{});
		break;
	case WaveStage::Shade: {
		const size_t lds = (size_t)kShadeLdsQuads * sizeof(uint4);
		if constexpr (kLevel == 3) PG_BY_FIRST(hipLaunchKernelGGL((k_wave_shade_l3<kF>), grid, block, lds, s, a));
		else PG_BY_FIRST(hipLaunchKernelGGL((k_wave_shade<kLevel, kF>), grid, block, lds, s, a));
		break;
	}
	}
#undef PG_BY_FIRST
}

void launch_wave_stage(WaveStage stage, int level, bool first, const RenderArgs &a, unsigned grid_blocks, unsigned n_cus, hipStream_t s,
                       uint32_t *geo)
{
	if (level >= 3) launch_stage_level<3>(stage, first, a, dim3(grid_blocks), n_cus, s, geo);
	else launch_stage_level<2>(stage, first, a, dim3(grid_blocks), n_cus, s, geo);
}

int wave_workspace_planes() { return WS_COUNT; }

bool shade_phases_compiled_in() { return PG_SHADE_PHASES != 0; }

} // namespace pg
