// pg_render_stages.hpp -- the bounce of PathGuidingIntegrator.sample() (src/path_guiding_integrator.py:179-381) as device
// functions, stated once: camera_ray, stage_a1 / stage_a2 (surface, emission, emitter sample, BSDF sample, the lane's class),
// stage_guide (the SD-tree calls), store_slots and stage_b (mixture pdfs, radiance, the record, Russian roulette, the advance).
// Templates on the scene's feature level.  Every kernel that shades a vertex is assembled from them: the fused kernels of quad
// scenes (pg_render.hip, levels 0 and 1) and the kernels of the split pipeline (pg_render_wave.hip, levels 2 and 3).  What the
// kernels keep for themselves is where a path's state lives between bounces, who casts the rays, and the record's place in the
// list.  Arithmetic and sampler draw order are those of oracle/pg_oracle_render.c, operation by operation.
// (Level 0 -- all-diffuse quad scenes -- keeps the reflectance in the quad and names no row of the material table: StageA::mat
// is 0 there and material_of reads nothing of the table, see both.)
#pragma once
#include "pg_render_dev.hpp"

namespace pg {

// lane classes and switches a bounce decides in stage_a
enum : uint32_t {
	F_VALID = 1u,        // the ray hit something (:185)
	F_ACTIVE_NEXT = 2u,  // depth + 1 < max_depth and valid (:208)
	F_ACTIVE_EM = 4u,    // emitter sampling happened and ds.pdf != 0 (:210, 216)
	F_NEED_SHADOW = 8u,  // em_weight holds the unoccluded value: trace the shadow ray
	F_DS_DELTA = 16u,    // the emitter sample came from a delta light
	F_DELTA = 32u,       // the BSDF sample is a delta lobe (:282)
	F_DO_MIS = 64u,      // bsdf-mis or sdtree-mis lane (:283)
	F_SMP_TREE = 128u,   // sdtree-mis: the direction comes from the SD-tree (:297)
	F_BSDF_MIS = 256u,   // bsdf-mis: BSDF direction, SD-tree pdf (:293)
	F_NEE_LIVE = 512u,   // the emitter sample can contribute: its BSDF value is not zero (see stage_a)
	F_HAS_LE = 1024u,    // emitted radiance reached the path here (Le has a non-zero bit)
};

struct HitRec {
	int prim;
	float t, u, v;
};

struct StageA {
	v3 p, n, ng, wi, refl, Le, ds_d, em_w, bv_em, sh_o, sh_d, wo, bsdf_w;
	float ds_pdf, bp_em, sh_tmax, bsdf_pdf, eta;
	int mat;
	uint32_t flags;
};

struct GuideOut { // (as it is made: a vertex no SD-tree call has looked at -- unit pdfs, no accumulators)
	float nee_cx = 0.0f, nee_cy = 0.0f, wo_cx = 0.0f, wo_cy = 0.0f, pdf_nee = 1.0f, pdf_tree = 1.0f;
	v3 wo;
	// the record's accumulators in sdTree_current (kSlotNone / kSlotRoot / rec * 4 + child, pg_descent.hpp), found by
	// the walks of sdTree_prev this stage makes anyway; tree_flags = the KD leaf's quadtree, bit 31 = the vertex
	// lies inside the root box and is counted (kdtree.py:193)
	uint32_t slot_path = kSlotNone, slot_nee = kSlotNone, tree_flags = 0u;
};
__device__ __forceinline__ GuideOut guide_none(v3 wo) { GuideOut g; g.wo = wo; return g; } // ... with the direction the caller has

__device__ __forceinline__ Material material_of(const RenderArgs &a, int mat, v3 refl, int level)
{
	Material m;
	if (level == 0) { // (what surface_at<0> makes: no row of the table is read, a.mats may be anything)
		m.type = MAT_DIFFUSE; m.M = nullptr; m.one_sided = false;
	} else m = load_material(a.mats + (size_t)mat * kMaterialStride, level);
	m.refl = refl; // (as the surface left it: a texture's colour where there is one)
	return m;
}

// ---- :185-220 ----
// stage_a in two halves, so that a kernel can put something between them (k_wave_shade walks the shadow ray there, with
// the BSDF sample not made yet and so not alive): stage_a1 -- the surface, emitted radiance and its MIS weight, the
// emitter sample, the BSDF towards it, the shadow ray; stage_a2 -- the BSDF sample and the lane's class.  The sampler
// draws keep their order (:214 before :272, 286); stage_a = the two in sequence.
template <int kLevel>
__device__ __forceinline__ void stage_a1(const RenderArgs &a, Pcg32 &rng, v3 ray_o, v3 ray_d, v3 thr, v3 prev_p,
                                         float prev_bsdf_pdf, bool prev_delta, const HitRec &h, uint32_t depth, StageA &o)
{
	const Shapes &sh = a.shapes;
	const int D = a.max_depth;
	const bool valid = h.prim >= 0;
	Surface sf;
	sf.p = V(0, 0, 0); sf.n = V(0, 0, 1); sf.ng = V(0, 0, 1); sf.radiance = V(0, 0, 0); sf.is_em = false;
	sf.m.type = 0; sf.m.refl = V(0, 0, 0); sf.m.M = a.mats; sf.m.one_sided = false;
	if (valid) sf = surface_at<kLevel>(sh, a.mats, h.prim, ray_o, ray_d, h.t, h.u, h.v);
	const v3 p = sf.p, n = sf.n;
	const Material &mt = sf.m;
	const Frame fr = make_frame(n);
	const v3 wi = to_local(fr, V(-ray_d.x, -ray_d.y, -ray_d.z));
	const bool is_em = valid && sf.is_em;
	const float inv_em_count = 1.0f / (float)a.n_emitters; // only used when an emitter was hit
	// ---- :189-200 direct emission ----
	const v3 em_radiance = (is_em && wi.z > 0.0f) ? sf.radiance : V(0, 0, 0);
	float emitter_pdf = 0.0f;
	if (is_em && !prev_delta) emitter_pdf = emitter_hit_pdf<kLevel>(sh, h.prim, prev_p, p, n, inv_em_count);
	const float mis = mis_weight(prev_bsdf_pdf, emitter_pdf);
	o.Le = vmul(vscale(thr, mis), em_radiance);
	// ---- :207-220 emitter sampling ----
	const bool active_next = (depth + 1 < (uint32_t)D) && valid;
	bool active_em = active_next && (kLevel < 3 || material_is_smooth(mt)); // :210 BSDFFlags.Smooth
	const float e1 = rng.next_f32(), e2 = rng.next_f32(); // :214, unmasked
	bool ds_delta = false, need_shadow = false;
	o.ds_d = V(0, 0, 0); o.em_w = V(0, 0, 0); o.ds_pdf = 0.0f;
	o.sh_o = V(0, 0, 0); o.sh_d = V(0, 0, 1); o.sh_tmax = 0.0f;
	if (active_em)
		sample_emitter_ray<kLevel>(sh, a.dir_lights, a.emitters, a.n_emitters, p, sf.ng, e1, e2, o.ds_d, o.ds_pdf, o.em_w,
		                           ds_delta, need_shadow, o.sh_o, o.sh_d, o.sh_tmax);
	active_em = active_em && (o.ds_pdf != 0.0f); // :216
	const v3 wo_em = to_local(fr, o.ds_d);
	bsdf_eval_pdf<kLevel>(mt, wi, wo_em, active_em, o.bv_em, o.bp_em);
	// An emitter sample whose BSDF value is zero (the light is behind the surface) contributes
	// Lr_dir = ((thr mis_em) 0) em_weight = +0 whatever the visibility test and the SD-tree pdf of its
	// direction say -- as long as em_weight is finite, and it is unless the light point all but touches
	// the surface.  Such a lane needs neither the shadow ray nor the tree query: result-neutral, bit for
	// bit (the oracle performs both and multiplies by zero).
	const bool nee_live = active_em && !(o.bv_em.x == 0.0f && o.bv_em.y == 0.0f && o.bv_em.z == 0.0f && finite_f32(o.em_w.x) &&
	                                     finite_f32(o.em_w.y) && finite_f32(o.em_w.z));
	if (!nee_live) need_shadow = false;
	o.p = p; o.n = n; o.ng = sf.ng; o.wi = wi; o.refl = mt.refl;
	o.mat = (kLevel && valid) ? (int)((mt.M - a.mats) / kMaterialStride) : 0; // (level 0 has no rows: the quad holds its reflectance)
	asm volatile("" : "+v"(o.mat)); // (the row's NUMBER from here on, one register: not the 64-bit pointer it was made of, kept for later)
	o.flags = (valid ? F_VALID : 0u) | (active_next ? F_ACTIVE_NEXT : 0u) | (active_em ? F_ACTIVE_EM : 0u) |
	          (need_shadow ? F_NEED_SHADOW : 0u) | (ds_delta ? F_DS_DELTA : 0u) | (nee_live ? F_NEE_LIVE : 0u) |
	          ((__float_as_uint(o.Le.x) | __float_as_uint(o.Le.y) | __float_as_uint(o.Le.z)) != 0u ? F_HAS_LE : 0u);
}

// ---- :272-297 next direction (the surface comes back from what stage_a1 left in `o`: the Duff frame of the shading normal and
// the material row are functions of o.n and o.mat) ----
template <int kLevel>
__device__ __forceinline__ void stage_a2(const RenderArgs &a, Pcg32 &rng, StageA &o)
{
	const float f = a.frac;
	const bool active_next = (o.flags & F_ACTIVE_NEXT) != 0u;
	Material mt = material_of(a, o.mat, o.refl, kLevel);
	if (!(o.flags & F_VALID)) { mt.type = 0; mt.one_sided = false; } // (the ray left the scene: stage_a1's placeholder surface)
	const Frame fr = make_frame(o.n);
	float s1 = 0.0f, s2x = 0.0f, s2y = 0.0f;
	if (active_next) { // next_1d (lobe choice: only the dielectrics read it), next_2d
		if (kLevel >= 3) s1 = rng.next_f32();
		else rng.skip();
		s2x = rng.next_f32();
		s2y = rng.next_f32();
	}
	v3 wo_local;
	bool delta;
	bsdf_sample<kLevel>(mt, o.wi, s1, s2x, s2y, active_next, wo_local, o.bsdf_pdf, o.bsdf_w, o.eta, delta);
	o.wo = to_world(fr, wo_local);
	const bool do_mis = active_next && !delta && a.guided; // :283
	bool pick_tree = false;
	if (active_next) pick_tree = rng.next_f32() > f; // :286
	const bool smp_tree = pick_tree && do_mis;
	const bool bsdf_mis = do_mis && !smp_tree;
	o.flags |= (delta ? F_DELTA : 0u) | (do_mis ? F_DO_MIS : 0u) | (smp_tree ? F_SMP_TREE : 0u) | (bsdf_mis ? F_BSDF_MIS : 0u);
}

template <int kLevel>
__device__ __forceinline__ void stage_a(const RenderArgs &a, Pcg32 &rng, v3 ray_o, v3 ray_d, v3 thr, v3 prev_p,
                                        float prev_bsdf_pdf, bool prev_delta, const HitRec &h, uint32_t depth, StageA &o)
{
	stage_a1<kLevel>(a, rng, ray_o, ray_d, thr, prev_p, prev_bsdf_pdf, prev_delta, h, depth, o);
	stage_a2<kLevel>(a, rng, o);
}

// ---- :244, 301, 307: the SD-tree calls of a bounce (one KD descent) and the canonical coordinates of
// the two directions (dirToCanonical feeds the pdf queries and the record, :327, 338) ----
__device__ __forceinline__ bool guide_has_work(const RenderArgs &a, uint32_t flags)
{
	const bool do_record = a.record && (flags & F_VALID);
	return do_record || ((flags & F_NEE_LIVE) && a.guided) || (flags & (F_SMP_TREE | F_BSDF_MIS));
}

__device__ __forceinline__ void stage_guide(const RenderArgs &a, const float *s_planes, Pcg32 &rng, v3 p, v3 ds_d, v3 wo_in,
                                            uint32_t flags, GuideOut &g)
{
	const bool active_sd_em = (flags & F_NEE_LIVE) && a.guided; // (a dead emitter sample's pdf would multiply zero: stage_a)
	const bool do_record = a.record && (flags & F_VALID);
	const bool smp_tree = (flags & F_SMP_TREE) != 0u, bsdf_mis = (flags & F_BSDF_MIS) != 0u;
	// a recorded vertex names its accumulators (KDTree.addDataPropagate, kdtree.py:180-225): the leaf of its path
	// direction and, when the emitter sample can carry energy, the leaf of the emitter direction
	const bool nee_slot_wanted = do_record && a.store_nee && (flags & F_NEE_LIVE);
	TreeHead head = {kNoRecord, 0.0f};
	uint32_t tree_id = 0;
	uint32_t lv;
	unsigned c_kd = 0, c_kdq = 0, c_q = 0, c_qq = 0; // descent statistics for the byte model
	g = guide_none(wo_in);
	if (active_sd_em || (do_record && a.store_nee)) dir_to_canonical(ds_d.x, ds_d.y, ds_d.z, g.nee_cx, g.nee_cy);
	if (active_sd_em || smp_tree || bsdf_mis || do_record) { // one KD descent serves every query of the vertex
		KdNode leaf;
		const bool inside = inside_root(a.tree, p.x, p.y, p.z);
		kd_descend_grid(a.tree, s_planes, p.x, p.y, p.z, inside, leaf, lv);
		c_kd += lv; ++c_kdq;
		const uint2 hv = gather8(a.tree.head + leaf.tree);
		head.root_rec = hv.x;
		head.root_irr = __uint_as_float(hv.y);
		tree_id = leaf.tree; // (outside the box: node 0's stale tree, kdtree.py:224)
		g.tree_flags = tree_id | (inside ? 0x80000000u : 0u);
	}
	if (active_sd_em) { // :244
		g.pdf_nee = quad_pdf_t<true>(a.tree.rec, a.tree.jump, tree_id, head, g.nee_cx, g.nee_cy, lv, g.slot_nee);
		c_q += lv; ++c_qq;
	}
	if (smp_tree) { // :301
		float dx, dy, dz;
		quad_sample_t<true>(a.tree.rec, a.tree.jump, tree_id, head, rng, dx, dy, dz, g.pdf_tree, lv, g.slot_path);
		c_q += lv; ++c_qq;
		g.wo = V(dx, dy, dz);
	}
	if (bsdf_mis || do_record) dir_to_canonical(g.wo.x, g.wo.y, g.wo.z, g.wo_cx, g.wo_cy);
	if (bsdf_mis) { // :307
		g.pdf_tree = quad_pdf_t<true>(a.tree.rec, a.tree.jump, tree_id, head, g.wo_cx, g.wo_cy, lv, g.slot_path);
		c_q += lv; ++c_qq;
	}
	// the leaves no query has walked to (unguided iterations, delta lobes, the last vertex of a path): the two
	// walks of QuadTree.addDataPropagate (quadtree.py:443-464), in lock step
	const bool walk_path = do_record && !smp_tree && !bsdf_mis, walk_nee = nee_slot_wanted && !active_sd_em;
	if (walk_path || walk_nee) {
		LeafCursor cp = leaf_cursor(a.tree.jump, tree_id, head, g.wo_cx, g.wo_cy, walk_path);
		LeafCursor cn = leaf_cursor(a.tree.jump, tree_id, head, g.nee_cx, g.nee_cy, walk_nee);
		quad_find_leaf_slots2(a.tree.rec, cp, cn);
		if (walk_path) { g.slot_path = cursor_slot(cp); c_q += cp.levels; ++c_qq; }
		if (walk_nee) { g.slot_nee = cursor_slot(cn); c_q += cn.levels; ++c_qq; }
	}
	if (a.dc && c_kdq) { // instrumented passes only (pg_enable_depth_counters)
		atomicAdd(&a.dc->kd_levels, (unsigned long long)stat_levels(c_kd)); // (c_kd, c_q: sums of statistics words, pg_descent.hpp)
		atomicAdd(&a.dc->kd_queries, (unsigned long long)c_kdq);
		atomicAdd(&a.dc->quad_levels, (unsigned long long)stat_levels(c_q));
		atomicAdd(&a.dc->quad_queries, (unsigned long long)c_qq);
		atomicAdd(&a.dc->layout_bytes, (unsigned long long)(stat_bytes(c_kd) + stat_bytes(c_q)));
	}
}

// Streaming stores (the "nt" bit): what a kernel writes once for a LATER kernel to read -- the record list, the paths'
// records -- should not push the trees, the BVH nodes and the textures this kernel gathers from out of L2.  Measured:
// k_wave_shade 35.1 -> 34.3 ms per step.  (The same bit on the record's seven LOADS made them miss seven times:
// 35.1 -> 37.7.)
#define PG_ST(ptr, val) __builtin_nontemporal_store((val), (ptr))
// the accumulators of a recorded vertex go straight into the record list (pg_list_records, pg_kernels.hpp)
__device__ __forceinline__ void store_slots(const RenderArgs &a, uint64_t rec_slot, const GuideOut &g)
{
	PG_ST(reinterpret_cast<unsigned long long *>(a.r_slot + rec_slot), (unsigned long long)g.slot_path | ((unsigned long long)g.slot_nee << 32));
	PG_ST(a.r_tree + rec_slot, g.tree_flags);
}

// ---- :247-261, 302-381; returns whether the path continues, with its state for the next bounce in
// thr, L, ior, ray_o, ray_d, prev_pdf, delta_out ----
template <int kLevel>
__device__ __forceinline__ bool stage_b(const RenderArgs &a, Pcg32 &rng, v3 &thr, v3 &L, float &ior, const StageA &A,
                                        const GuideOut &g, bool occluded, uint64_t lane, uint64_t rec_slot, uint32_t depth,
                                        v3 &ray_o, v3 &ray_d, float &prev_pdf, bool &delta_out)
{
	const uint64_t N = a.n_lanes;
	const int D = a.max_depth;
	const float f = a.frac;
	const bool valid = (A.flags & F_VALID) != 0u;
	bool active_next = (A.flags & F_ACTIVE_NEXT) != 0u;
	const bool ds_delta = (A.flags & F_DS_DELTA) != 0u, delta = (A.flags & F_DELTA) != 0u;
	const bool do_mis = (A.flags & F_DO_MIS) != 0u, smp_tree = (A.flags & F_SMP_TREE) != 0u;
	const bool nee_live = (A.flags & F_NEE_LIVE) != 0u;
	const v3 em_weight = (occluded || !nee_live) ? V(0, 0, 0) : A.em_w;
	// ---- :223-256 NEE MIS against the mixture pdf ----
	const float pdf_diffuse = 1.0f; // :222-241
	const float sdtree_pdf_em = g.pdf_nee;
	// a lane without a live emitter sample: every factor stage_a computed for it is zero or multiplies
	// zero -- the same formula on zeros gives the same +0
	const float bp_em = nee_live ? A.bp_em : 0.0f, ds_pdf = nee_live ? A.ds_pdf : 0.0f;
	const v3 bv_em = nee_live ? A.bv_em : V(0, 0, 0);
	float surface_pdf_em = f * bp_em + ((1.0f - f) * sdtree_pdf_em) * pdf_diffuse;
	if (!a.guided) surface_pdf_em = bp_em;
	const float mis_em = (kLevel >= 3 && ds_delta && nee_live) ? 1.0f : mis_weight(ds_pdf, surface_pdf_em); // :253
	const v3 Lr_dir = vmul(vmul(vscale(thr, mis_em), bv_em), em_weight);
	const v3 Le = (A.flags & F_HAS_LE) ? A.Le : V(0, 0, 0);
	L = vadd(L, vadd(Le, Lr_dir)); // :261
	// ---- :302-311 ----
	v3 bsdf_weight = A.bsdf_w;
	float bsdf_pdf = A.bsdf_pdf;
	v3 bsdf_value = vscale(bsdf_weight, bsdf_pdf);
	float woPdf = bsdf_pdf;
	const v3 wo_world = g.wo;
	if (smp_tree) { // :302-304
		const Frame fr = make_frame(A.n);
		const v3 wo_local = to_local(fr, wo_world);
		const Material mt = material_of(a, A.mat, A.refl, kLevel);
		bsdf_eval_pdf<kLevel>(mt, A.wi, wo_local, true, bsdf_value, bsdf_pdf);
	}
	if (do_mis) { // :310-311
		woPdf = f * bsdf_pdf + (1.0f - f) * g.pdf_tree;
		bsdf_weight = vdivs(bsdf_value, woPdf);
		// deliberate deviation: 0/0 when a zero-energy tree proposes a direction below
		// the surface; the reference's throughput turns NaN there, here the path simply ends
		if (!(woPdf > 0.0f)) bsdf_weight = V(0, 0, 0);
	}
	// ---- :318-346 record (a list in visiting order, see pg_render.hip).  The list of the split pipeline holds what
	// processPathData (:434-453) needs of a vertex -- the throughputs, the BSDF weight, woPdf, the luminance of the
	// emitter sample's share -- and, instead of position and directions, the accumulators they lead to (store_slots) ----
	const bool do_record = a.record && valid;
	if (a.record) PG_ST(a.ray_of + rec_slot, valid ? (uint32_t)lane : 0xffffffffu);
	if (do_record) {
		const uint64_t S = N * (uint64_t)D;
		const uint64_t s = rec_slot;
		PG_ST(a.r_bsdf + s, bsdf_weight.x); PG_ST(a.r_bsdf + S + s, bsdf_weight.y); PG_ST(a.r_bsdf + 2 * S + s, bsdf_weight.z);
		PG_ST(a.r_tb + s, thr.x); PG_ST(a.r_tb + S + s, thr.y); PG_ST(a.r_tb + 2 * S + s, thr.z);
		PG_ST(a.r_tr + s, L.x); PG_ST(a.r_tr + S + s, L.y); PG_ST(a.r_tr + 2 * S + s, L.z);
		float nee_lum = 0.0f;
		if (a.store_nee) { // :336, and the NaN scrub + luminance of :467, 471 (the only use of the three channels)
			v3 rn = vdiv(Lr_dir, thr);
			if (rn.x != rn.x) rn.x = 0.0f;
			if (rn.y != rn.y) rn.y = 0.0f;
			if (rn.z != rn.z) rn.z = 0.0f;
			nee_lum = luminance(rn.x, rn.y, rn.z);
		}
		PG_ST(a.r_nee + s, nee_lum);
		PG_ST(a.r_wp + s, woPdf);
	}
	// ---- :352-381 advance ----
	if (kLevel >= 3) ior = ior * A.eta; // :357 (the BSDF sample's eta also when the direction came from the tree)
	thr = vmul(thr, bsdf_weight);
	const float tmax = max3(thr);
	active_next = active_next && (tmax != 0.0f);
	float rr_prob = tmax * (ior * ior);
	if (!(rr_prob < 0.95f)) rr_prob = 0.95f;
	const bool rr_active = depth >= (uint32_t)a.rr_depth;
	const float rr = rng.next_f32(); // :377, unmasked
	const bool rr_continue = rr < rr_prob;
	active_next = active_next && (!rr_active || rr_continue);
	// :352 spawn_ray: the vertex pushed off the surface along the geometric normal, towards wo
	float mag = (1.0f + max3(V(fabs_(A.p.x), fabs_(A.p.y), fabs_(A.p.z)))) * kRayEps;
	if (dot3(A.ng, wo_world) < 0.0f) mag = -mag;
	ray_o = vadd(A.p, vscale(A.ng, mag));
	ray_d = wo_world;
	prev_pdf = woPdf;
	delta_out = delta;
	return active_next;
}

// the camera ray of a lane (mi.render's sensor.sample_ray_differential: one 2-D jitter draw per sample)
__device__ __forceinline__ void camera_ray(const RenderArgs &a, uint64_t lane, Pcg32 &rng, v3 &ray_o, v3 &ray_d)
{
	const uint64_t pixel = global_pixel(a, lane / (uint64_t)a.spp);
	rng = lane_stream(a.seed, a.spp, a.batched, pixel, (uint32_t)(lane % (uint64_t)a.spp));
	const int W = a.cam.width, H = a.cam.height;
	const float px = (float)(pixel % (uint64_t)W), py = (float)(pixel / (uint64_t)W);
	const float jx = rng.next_f32(), jy = rng.next_f32();
	const float tan_y = a.cam.tan_half_fov_x / ((float)W / (float)H);
	const float cx = (1.0f - 2.0f * ((px + jx) / (float)W)) * a.cam.tan_half_fov_x;
	const float cy = (1.0f - 2.0f * ((py + jy) / (float)H)) * tan_y;
	const float len = __builtin_sqrtf((cx * cx + cy * cy) + 1.0f);
	const v3 dc = V(cx / len, cy / len, 1.0f / len);
	ray_d = vadd(vadd(vscale(ld3(a.cam.axis_x), dc.x), vscale(ld3(a.cam.axis_y), dc.y)), vscale(ld3(a.cam.axis_z), dc.z));
	ray_o = ld3(a.cam.origin);
}

} // namespace pg
