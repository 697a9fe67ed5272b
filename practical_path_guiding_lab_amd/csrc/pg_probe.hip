// pg_probe.hip -- pg_scene_intersect: the renderer's ray casting by itself, for tests.  One ray per lane through intersect<>
// of pg_render_dev.hpp -- the function the render kernels call, not a copy -- in the three forms those kernels give its walk:
// the ray-casting kernels' (kLdsStack stack entries and kBvhTopNodes nodes in LDS), k_wave_shade's (kShadeStack entries,
// kShadeTopNodes nodes, the kSlim walk) and one without staged nodes.  pg_bsdf_probe: the BSDF layer by itself -- one
// (material row, wi, wo, u) per lane through load_material, bsdf_eval_pdf<> and bsdf_sample<> of the same header.
// pg_surface_probe: the surface at a hit by itself -- one (shape, ray, t, barycentrics, previous vertex) per lane through
// surface_at<>, normal_at<>, make_frame, to_local, to_world and emitter_hit_pdf<> as stage_a1 calls them.
// pg_emitter_probe: emitter sampling by itself -- one (point, geometric normal, 2-D sample) per lane through
// sample_emitter_ray<> with the scene's own emitter list, directional lights and bounding sphere, as stage_a1 passes them.
// pg_vertex_probe: a vertex's bookkeeping by itself -- one lane per item through stage_b<> of pg_render_stages.hpp, fed with
// columns that hold what StageA, GuideOut and the path state hold, its record planes the caller's output planes.
// pg_head_probe: a vertex's head by itself -- one (ray, hit, path state, sampler) per lane through stage_a<> (stage_a1 then
// stage_a2) of the same header at the scene's feature level, every field of StageA an output column.
// Nothing of the product path launches these kernels.
#include <string>
#include <type_traits>
#include <vector>

#include "pg_render_dev.hpp"
#include "pg_render_stages.hpp"
#include "pg_scene_state.hpp"

using namespace pg;

namespace {

constexpr uint64_t kProbeMaxRays = 1ull << 20; // (kProbeMaxRays * kOvfStack < 2^32: BvhStack::ovf_first is a 32-bit entry index)
static_assert(kProbeMaxRays * (uint64_t)kOvfStack <= 0xffffffffull, "pg_scene_intersect: the overflow strips are indexed by 32 bits");

struct ProbeArgs {
	Shapes shapes;
	uint64_t n;
	const float *o, *d, *tmax; // (n,3), (n,3), (n)
	float *t, *uv;             // (n), (n,2)
	int32_t *prim;             // (n)
	uint2 *ovf;                // n * kOvfStack entries
};

// Every loop a lane runs here is bounded: intersect_linear by the shape counts, a leaf by its 1..8 triangles, and the walk by
// BvhWalk::budget -- the node loop and bvh_pop test it, and with the budget spent the outer loop of intersect() pops nothing
// and ends.  So a ray of NaNs or zeros, for which every box test says "maybe", ends after at most 8 * nodes + 8 steps; the
// stack cannot outgrow n_lds + kOvfStack entries whatever the ray is (pg_scene_set_ex has checked the tree for that).
template <int kLevel, bool kAny, int kForm>
__global__ __launch_bounds__(kRBlock) void k_probe_intersect(ProbeArgs p)
{
	constexpr int kStack = kForm == 1 ? kShadeStack : kLdsStack;
	constexpr int kTop = kForm == 1 ? kShadeTopNodes : kBvhTopNodes;
	__shared__ uint2 s_stack[kStack][kRBlock];
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	BvhStack stk = bvh_stack(&s_stack[0][threadIdx.x], p.ovf, (uint32_t)tid * (uint32_t)kOvfStack, kStack);
	if (kForm != 2) { // (form 2 leaves stk.n_top = 0: every node is read from memory)
		__shared__ u32x4_t s_top[kTop * kBvhNodeQuads];
		RenderArgs a;
		a.shapes = p.shapes;
		stage_bvh_top<kTop>(s_top, a, stk);
	}
	if (tid >= p.n) return;
	const v3 o = ld3(p.o + 3 * tid), d = ld3(p.d + 3 * tid);
	float t, bu = 0.0f, bv = 0.0f;
	const int prim = intersect<kLevel, kAny, kForm == 1>(p.shapes, o, d, p.tmax[tid], t, stk, bu, bv);
	p.t[tid] = t;
	p.prim[tid] = prim;
	p.uv[2 * tid] = bu;
	p.uv[2 * tid + 1] = bv;
}

template <int kLevel, bool kAny>
auto intersect_form(int form) -> void (*)(ProbeArgs)
{
	if (form == 0) return k_probe_intersect<kLevel, kAny, 0>;
	if (form == 1) return k_probe_intersect<kLevel, kAny, 1>;
	return k_probe_intersect<kLevel, kAny, 2>;
}

struct BsdfProbeArgs {
	uint64_t n;
	const float *mats;       // n_mat rows of kMaterialStride floats
	const int32_t *mat;      // (n) row of lane i: checked against n_mat on the host
	const float *wi, *wo, *u; // (n,3) each; u = (lobe sample, 2-D sample)
	float *value, *pdf;      // (n,3), (n): bsdf_eval_pdf
	float *s_wo, *s_pdf, *s_weight, *s_eta; // (n,3), (n), (n,3), (n): bsdf_sample
	int32_t *s_delta;        // (n)
};

// No loop but rc_sample_visible_11's three Newton steps; every address is a function of tid < n and of a checked row number.
template <int kLevel>
__global__ __launch_bounds__(kRBlock) void k_probe_bsdf(BsdfProbeArgs p)
{
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (tid >= p.n) return;
	const Material mt = load_material(p.mats + (uint64_t)p.mat[tid] * kMaterialStride, kLevel);
	const v3 wi = ld3(p.wi + 3 * tid), wo = ld3(p.wo + 3 * tid), u = ld3(p.u + 3 * tid);
	v3 value, o, weight;
	float pdf, s_pdf, eta;
	bool delta;
	bsdf_eval_pdf<kLevel>(mt, wi, wo, true, value, pdf);
	bsdf_sample<kLevel>(mt, wi, u.x, u.y, u.z, true, o, s_pdf, weight, eta, delta);
	p.value[3 * tid] = value.x; p.value[3 * tid + 1] = value.y; p.value[3 * tid + 2] = value.z;
	p.pdf[tid] = pdf;
	p.s_wo[3 * tid] = o.x; p.s_wo[3 * tid + 1] = o.y; p.s_wo[3 * tid + 2] = o.z;
	p.s_pdf[tid] = s_pdf;
	p.s_weight[3 * tid] = weight.x; p.s_weight[3 * tid + 1] = weight.y; p.s_weight[3 * tid + 2] = weight.z;
	p.s_eta[tid] = eta;
	p.s_delta[tid] = delta ? 1 : 0;
}

struct SurfaceProbeArgs {
	Shapes shapes;
	const float *mats;
	uint64_t n;
	int n_emitters;
	const int32_t *prim;            // (n) shape of lane i: checked against the shape count on the host
	const float *o, *d, *t, *uv, *ref; // (n,3), (n,3), (n), (n,2), (n,3)
	float *out;                     // (n, PG_SURFACE_PROBE_FLOATS)
	int32_t *flags;                 // (n,4)
};

// No loop; every address is a function of tid < n and of a checked shape number (the rows a shape names -- material, texture,
// texels -- were checked by pg_scene_set_ex, and texture_eval wraps its texel indices into the bitmap whatever the uv are).
template <int kLevel>
__global__ __launch_bounds__(kRBlock) void k_probe_surface(SurfaceProbeArgs p)
{
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (tid >= p.n) return;
	const int prim = p.prim[tid];
	const v3 ray_o = ld3(p.o + 3 * tid), ray_d = ld3(p.d + 3 * tid), prev_p = ld3(p.ref + 3 * tid);
	const Surface sf = surface_at<kLevel>(p.shapes, p.mats, prim, ray_o, ray_d, p.t[tid], p.uv[2 * tid], p.uv[2 * tid + 1]);
	const v3 n = sf.n;
	const Frame fr = make_frame(n);
	const v3 wi = to_local(fr, V(-ray_d.x, -ray_d.y, -ray_d.z));
	const v3 back = to_world(fr, wi);
	const v3 nat = normal_at<kLevel>(p.shapes, prim, sf.p);
	const float inv_em_count = 1.0f / (float)p.n_emitters; // only used when an emitter was hit (there is one, then)
	float emitter_pdf = 0.0f;
	if (sf.is_em) emitter_pdf = emitter_hit_pdf<kLevel>(p.shapes, prim, prev_p, sf.p, n, inv_em_count);
	float *o = p.out + (uint64_t)PG_SURFACE_PROBE_FLOATS * tid;
	o[0] = sf.p.x; o[1] = sf.p.y; o[2] = sf.p.z;
	o[3] = n.x; o[4] = n.y; o[5] = n.z;
	o[6] = sf.ng.x; o[7] = sf.ng.y; o[8] = sf.ng.z;
	o[9] = sf.m.refl.x; o[10] = sf.m.refl.y; o[11] = sf.m.refl.z;
	o[12] = sf.radiance.x; o[13] = sf.radiance.y; o[14] = sf.radiance.z;
	o[15] = nat.x; o[16] = nat.y; o[17] = nat.z;
	o[18] = emitter_pdf;
	o[19] = fr.s.x; o[20] = fr.s.y; o[21] = fr.s.z;
	o[22] = fr.t.x; o[23] = fr.t.y; o[24] = fr.t.z;
	o[25] = wi.x; o[26] = wi.y; o[27] = wi.z;
	o[28] = back.x; o[29] = back.y; o[30] = back.z;
	int32_t *f = p.flags + 4 * tid;
	f[0] = kLevel ? (int32_t)((sf.m.M - p.mats) / kMaterialStride) : -1; // (level 0 reads no row for a quad)
	f[1] = sf.m.type;
	f[2] = sf.m.one_sided ? 1 : 0;
	f[3] = sf.is_em ? 1 : 0;
}
static_assert(PG_SURFACE_PROBE_FLOATS == 31, "k_probe_surface writes 31 floats per lane");

struct EmitterProbeArgs {
	Shapes shapes;
	DirLights dir_lights;
	const int32_t *emitters;
	int n_emitters;
	uint64_t n;
	const float *p, *ng, *e; // (n,3), (n,3), (n,2)
	float *out;              // (n, PG_EMITTER_PROBE_FLOATS)
	int32_t *flags;          // (n,2)
};

// No loop and no BVH walk; every address is a function of tid < n but the emitter's row, whose number sample_emitter_ray
// clamps to [0, n_emitters) whatever e1 is (the host refuses an e outside [0, 1] all the same) and whose entry
// pg_scene_set_ex made from the scene's own counts: a flagged quad, a flagged sphere or -1 - k of a directional light k.
template <int kLevel>
__global__ __launch_bounds__(kRBlock) void k_probe_emitter(EmitterProbeArgs a)
{
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (tid >= a.n) return;
	const v3 p = ld3(a.p + 3 * tid), ng = ld3(a.ng + 3 * tid);
	v3 ds_d, em_w, sh_o, sh_d;
	float ds_pdf, sh_tmax;
	bool ds_delta, need_shadow;
	sample_emitter_ray<kLevel>(a.shapes, a.dir_lights, a.emitters, a.n_emitters, p, ng, a.e[2 * tid], a.e[2 * tid + 1], ds_d,
	                           ds_pdf, em_w, ds_delta, need_shadow, sh_o, sh_d, sh_tmax);
	float *o = a.out + (uint64_t)PG_EMITTER_PROBE_FLOATS * tid;
	o[0] = ds_d.x; o[1] = ds_d.y; o[2] = ds_d.z;
	o[3] = ds_pdf;
	o[4] = em_w.x; o[5] = em_w.y; o[6] = em_w.z;
	o[7] = sh_o.x; o[8] = sh_o.y; o[9] = sh_o.z;
	o[10] = sh_d.x; o[11] = sh_d.y; o[12] = sh_d.z;
	o[13] = sh_tmax;
	a.flags[2 * tid] = ds_delta ? 1 : 0;
	a.flags[2 * tid + 1] = need_shadow ? 1 : 0;
}
static_assert(PG_EMITTER_PROBE_FLOATS == 14, "k_probe_emitter writes 14 floats per lane");

struct VertexProbeArgs {
	RenderArgs a; // what stage_b reads of it: mats, n_lanes, max_depth (the record planes' stride only), frac, guided, record,
	              // store_nee, rr_depth and the record planes -- the caller's output planes, stride n
	pg_vertex_lanes in;
	pg_vertex_out out;
};
static_assert(sizeof(VertexProbeArgs) <= 4096, "kernel arguments are at most 4 KB");
static_assert(PG_VERTEX_VALID == F_VALID && PG_VERTEX_ACTIVE_NEXT == F_ACTIVE_NEXT && PG_VERTEX_DS_DELTA == F_DS_DELTA &&
                  PG_VERTEX_DELTA == F_DELTA && PG_VERTEX_DO_MIS == F_DO_MIS && PG_VERTEX_SMP_TREE == F_SMP_TREE &&
                  PG_VERTEX_NEE_LIVE == F_NEE_LIVE && PG_VERTEX_HAS_LE == F_HAS_LE,
              "include/pgsd.h names the lane classes of pg_render_stages.hpp");

// No loop (stage_b evaluates the BSDF, it does not sample: rc_sample_visible_11's Newton steps are not reached); every address is a
// function of tid < n -- the record entry's too: rec_slot = tid in planes of stride n_lanes * max_depth = n -- and of a checked
// row number, which material_of follows on PG_VERTEX_SMP_TREE lanes of levels 1..3 only.
template <int kLevel>
__global__ __launch_bounds__(kRBlock) void k_probe_vertex(VertexProbeArgs v)
{
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (tid >= v.a.n_lanes) return;
	const pg_vertex_lanes &in = v.in;
	StageA A;
	A.p = ld3(in.p + 3 * tid); A.n = ld3(in.n + 3 * tid); A.ng = ld3(in.ng + 3 * tid); A.wi = ld3(in.wi + 3 * tid);
	A.refl = ld3(in.refl + 3 * tid); A.Le = ld3(in.Le + 3 * tid);
	A.ds_d = V(0, 0, 0); A.sh_o = V(0, 0, 0); A.sh_d = V(0, 0, 1); A.sh_tmax = 0.0f; // (stage_b reads none of the four)
	A.em_w = ld3(in.em_w + 3 * tid); A.bv_em = ld3(in.bv_em + 3 * tid);
	A.wo = ld3(in.wo + 3 * tid); A.bsdf_w = ld3(in.bsdf_w + 3 * tid);
	A.ds_pdf = in.ds_pdf[tid]; A.bp_em = in.bp_em[tid]; A.bsdf_pdf = in.bsdf_pdf[tid]; A.eta = in.eta[tid];
	A.mat = in.mat[tid];
	A.flags = in.flags[tid];
	GuideOut g = guide_none(A.wo);
	g.pdf_nee = in.pdf_nee[tid];
	g.pdf_tree = in.pdf_tree[tid];
	Pcg32 rng;
	rng.state = in.rng_state[tid]; rng.inc = in.rng_inc[tid];
	v3 thr = ld3(in.thr + 3 * tid), L = ld3(in.L + 3 * tid), ray_o, ray_d;
	float ior = in.ior[tid], prev_pdf;
	bool delta_out;
	const bool go = stage_b<kLevel>(v.a, rng, thr, L, ior, A, g, in.occluded[tid] != 0, tid, tid, in.depth[tid], ray_o, ray_d, prev_pdf,
	                                delta_out);
	const pg_vertex_out &o = v.out;
	o.go[tid] = go ? 1 : 0;
	o.thr[3 * tid] = thr.x; o.thr[3 * tid + 1] = thr.y; o.thr[3 * tid + 2] = thr.z;
	o.L[3 * tid] = L.x; o.L[3 * tid + 1] = L.y; o.L[3 * tid + 2] = L.z;
	o.ior[tid] = ior;
	o.ray_o[3 * tid] = ray_o.x; o.ray_o[3 * tid + 1] = ray_o.y; o.ray_o[3 * tid + 2] = ray_o.z;
	o.ray_d[3 * tid] = ray_d.x; o.ray_d[3 * tid + 1] = ray_d.y; o.ray_d[3 * tid + 2] = ray_d.z;
	o.prev_pdf[tid] = prev_pdf;
	o.delta[tid] = delta_out ? 1 : 0;
	o.rng_state[tid] = rng.state;
}

struct HeadProbeArgs {
	RenderArgs a; // what stage_a reads of it: shapes, mats, dir_lights, emitters, n_emitters, max_depth, frac, guided
	uint64_t n;
	pg_head_lanes in;
	pg_head_out out;
};
static_assert(sizeof(HeadProbeArgs) <= 4096, "kernel arguments are at most 4 KB");
static_assert(PG_VERTEX_ACTIVE_EM == F_ACTIVE_EM && PG_VERTEX_NEED_SHADOW == F_NEED_SHADOW && PG_VERTEX_BSDF_MIS == F_BSDF_MIS,
              "include/pgsd.h names the lane classes of pg_render_stages.hpp");

// No loop but rc_sample_visible_11's three Newton steps; every address is a function of tid < n and of a checked shape number
// (the rows a shape names -- material, texture, texels -- were checked by pg_scene_set_ex, and texture_eval wraps its texel
// indices into the bitmap whatever the uv are) but the emitter's row, whose number sample_emitter_ray clamps to
// [0, n_emitters) whatever the lane's own sampler draws and whose entry pg_scene_set_ex made from the scene's own counts.
template <int kLevel>
__global__ __launch_bounds__(kRBlock) void k_probe_head(HeadProbeArgs v)
{
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (tid >= v.n) return;
	const pg_head_lanes &in = v.in;
	Pcg32 rng;
	rng.state = in.rng_state[tid]; rng.inc = in.rng_inc[tid];
	HitRec h;
	h.prim = in.prim[tid]; h.t = in.t[tid]; h.u = in.uv[2 * tid]; h.v = in.uv[2 * tid + 1];
	StageA A;
	stage_a<kLevel>(v.a, rng, ld3(in.ray_o + 3 * tid), ld3(in.ray_d + 3 * tid), ld3(in.thr + 3 * tid), ld3(in.prev_p + 3 * tid),
	                in.prev_bsdf_pdf[tid], in.prev_delta[tid] != 0, h, in.depth[tid], A);
	const pg_head_out &o = v.out;
	auto put = [tid](float *d, v3 s) { d[3 * tid] = s.x; d[3 * tid + 1] = s.y; d[3 * tid + 2] = s.z; };
	put(o.p, A.p); put(o.n, A.n); put(o.ng, A.ng); put(o.wi, A.wi); put(o.refl, A.refl); put(o.Le, A.Le); put(o.ds_d, A.ds_d);
	put(o.em_w, A.em_w); put(o.bv_em, A.bv_em); put(o.sh_o, A.sh_o); put(o.sh_d, A.sh_d); put(o.wo, A.wo); put(o.bsdf_w, A.bsdf_w);
	o.ds_pdf[tid] = A.ds_pdf; o.bp_em[tid] = A.bp_em; o.sh_tmax[tid] = A.sh_tmax; o.bsdf_pdf[tid] = A.bsdf_pdf; o.eta[tid] = A.eta;
	o.mat[tid] = A.mat;
	o.flags[tid] = A.flags;
	o.rng_state[tid] = rng.state;
}

// What every probe does before it reads an argument, in the order in which a caller sees the refusals: the context, the
// scene (where the probe reads one), the probe's first check of its own (own_first, own_last: the message, or nullptr where
// the check passes), the lane count, n == 0 (PG_OK: nothing is read), the pointers, its last check, the device.
// Returns kProbeGo where the probe is to go on, or what the probe returns.
constexpr int kProbeGo = 1;
int probe_ready(pg_context *ctx, const std::string &who, bool reads_scene, const char *own_first, uint64_t n, const char *lanes,
                bool null_pointer, const char *own_last = nullptr)
{
	if (!ctx) return PG_ERR_INVALID;
	if (reads_scene && (!ctx->render || !scene_state(ctx).have_scene)) return fail(ctx, PG_ERR_INVALID, who + ": call pg_scene_set first");
	if (own_first) return fail(ctx, PG_ERR_INVALID, who + ": " + own_first);
	if (n > kProbeMaxRays) return fail(ctx, PG_ERR_INVALID, who + ": at most 2^20 " + lanes + " in one call");
	if (n == 0) return PG_OK;
	if (null_pointer) return fail(ctx, PG_ERR_INVALID, who + ": NULL pointer");
	if (own_last) return fail(ctx, PG_ERR_INVALID, who + ": " + own_last);
	PG_HIP(ctx, hipSetDevice(ctx->device));
	return kProbeGo;
}

// One lane per item on `stream`, and the wait for it, of the kernel that kernel_of(std::integral_constant<int, level>()) names
// (level 0..3; anything else is 3's)
template <int kLevel> using Level = std::integral_constant<int, kLevel>;
template <class Args, class KernelOf>
int run_at_level(pg_context *ctx, int level, uint64_t n, void *stream, const Args &args, KernelOf kernel_of)
{
	void (*const kernel)(Args) = level == 0 ? kernel_of(Level<0>()) : level == 1 ? kernel_of(Level<1>())
	                             : level == 2 ? kernel_of(Level<2>()) : kernel_of(Level<3>());
	hipLaunchKernelGGL(kernel, dim3((unsigned)((n + kRBlock - 1) / kRBlock)), dim3(kRBlock), 0, (hipStream_t)stream, args);
	PG_HIP(ctx, hipGetLastError());
	PG_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
	return PG_OK;
}

} // namespace

int pg_vertex_probe(pg_context *ctx, uint64_t n, uint64_t n_mat, const float *d_materials, int32_t level,
                    const pg_vertex_lanes *lanes, float frac, int32_t guided, int32_t record, int32_t store_nee, int32_t rr_depth,
                    const pg_vertex_out *out, void *stream)
{
	bool null_pointer = !d_materials || !lanes || !out;
	if (lanes && out) {
		const pg_vertex_lanes &l = *lanes;
		const pg_vertex_out &o = *out;
		for (const void *q : {(const void *)l.thr, (const void *)l.L, (const void *)l.ior, (const void *)l.depth, (const void *)l.flags,
		                      (const void *)l.Le, (const void *)l.p, (const void *)l.n, (const void *)l.ng, (const void *)l.wi,
		                      (const void *)l.refl, (const void *)l.mat, (const void *)l.em_w, (const void *)l.bv_em,
		                      (const void *)l.bp_em, (const void *)l.ds_pdf, (const void *)l.bsdf_w, (const void *)l.bsdf_pdf,
		                      (const void *)l.eta, (const void *)l.wo, (const void *)l.pdf_nee, (const void *)l.pdf_tree,
		                      (const void *)l.occluded, (const void *)l.rng_state, (const void *)l.rng_inc, (const void *)o.go,
		                      (const void *)o.thr, (const void *)o.L, (const void *)o.ior, (const void *)o.ray_o, (const void *)o.ray_d,
		                      (const void *)o.prev_pdf, (const void *)o.delta, (const void *)o.rng_state, (const void *)o.ray_of,
		                      (const void *)o.r_bsdf, (const void *)o.r_tb, (const void *)o.r_tr, (const void *)o.r_nee,
		                      (const void *)o.r_wp})
			null_pointer = null_pointer || !q;
	}
	const int rc = probe_ready(ctx, "pg_vertex_probe", false, level < 0 || level > 3 ? "level must be 0, 1, 2 or 3" : nullptr, n, "lanes",
	                              null_pointer, n_mat == 0 || n_mat > 65536 ? "need 1..65536 material rows" : nullptr);
	if (rc != kProbeGo) return rc;
	PG_HIP(ctx, hipStreamSynchronize((hipStream_t)stream)); // (the caller's writes of the inputs, before the host reads them)
	// the rows and the row numbers are checked on the host before a lane follows them
	std::vector<float> rows(n_mat * kMaterialStride);
	PG_HIP(ctx, hipMemcpy(rows.data(), d_materials, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
	if (const char *err = check_material_rows(rows.data(), n_mat, 65536)) return fail(ctx, PG_ERR_INVALID, std::string("pg_vertex_probe: ") + err);
	std::vector<int32_t> index(n);
	PG_HIP(ctx, hipMemcpy(index.data(), lanes->mat, n * sizeof(int32_t), hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < n; ++i)
		if (index[i] < 0 || (uint64_t)index[i] >= n_mat) return fail(ctx, PG_ERR_INVALID, "pg_vertex_probe: material index outside the table");
	VertexProbeArgs v = {};
	v.in = *lanes;
	v.out = *out;
	v.a.mats = d_materials;
	v.a.n_lanes = n; v.a.max_depth = 1; // (planes of stride n_lanes * max_depth = n, and rec_slot = the lane)
	v.a.frac = frac; v.a.guided = guided ? 1 : 0; v.a.record = record ? 1 : 0; v.a.store_nee = store_nee ? 1 : 0; v.a.rr_depth = rr_depth;
	v.a.ray_of = out->ray_of; v.a.r_bsdf = out->r_bsdf; v.a.r_tb = out->r_tb; v.a.r_tr = out->r_tr; v.a.r_nee = out->r_nee; v.a.r_wp = out->r_wp;
	return run_at_level(ctx, level, n, stream, v, [](auto L) { return k_probe_vertex<decltype(L)::value>; });
}

int pg_head_probe(pg_context *ctx, uint64_t n, const pg_head_lanes *lanes, int32_t max_depth, float frac, int32_t guided,
                  const pg_head_out *out, void *stream)
{
	bool null_pointer = !lanes || !out;
	if (lanes && out) {
		const pg_head_lanes &l = *lanes;
		const pg_head_out &o = *out;
		for (const void *q : {(const void *)l.ray_o, (const void *)l.ray_d, (const void *)l.thr, (const void *)l.prev_p,
		                      (const void *)l.prev_bsdf_pdf, (const void *)l.prev_delta, (const void *)l.prim, (const void *)l.t,
		                      (const void *)l.uv, (const void *)l.depth, (const void *)l.rng_state, (const void *)l.rng_inc,
		                      (const void *)o.p, (const void *)o.n, (const void *)o.ng, (const void *)o.wi, (const void *)o.refl,
		                      (const void *)o.Le, (const void *)o.ds_d, (const void *)o.em_w, (const void *)o.bv_em, (const void *)o.sh_o,
		                      (const void *)o.sh_d, (const void *)o.wo, (const void *)o.bsdf_w, (const void *)o.ds_pdf, (const void *)o.bp_em,
		                      (const void *)o.sh_tmax, (const void *)o.bsdf_pdf, (const void *)o.eta, (const void *)o.mat,
		                      (const void *)o.flags, (const void *)o.rng_state})
			null_pointer = null_pointer || !q;
	}
	const int rc = probe_ready(ctx, "pg_head_probe", true, max_depth < 1 ? "max_depth must be at least 1" : nullptr, n, "lanes", null_pointer);
	if (rc != kProbeGo) return rc;
	const SceneState &sc = scene_state(ctx);
	PG_HIP(ctx, hipStreamSynchronize((hipStream_t)stream)); // (the caller's writes of the inputs, before the host reads them)
	// the shape numbers are checked on the host before a lane follows them (-1: the ray left the scene)
	const int64_t n_shapes = (int64_t)sc.n_quads + sc.n_spheres + 6 * (int64_t)sc.n_boxes + (int64_t)sc.n_tris;
	std::vector<int32_t> prim(n);
	PG_HIP(ctx, hipMemcpy(prim.data(), lanes->prim, n * sizeof(int32_t), hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < n; ++i)
		if (prim[i] < -1 || (int64_t)prim[i] >= n_shapes) return fail(ctx, PG_ERR_INVALID, "pg_head_probe: shape number outside the scene");
	// (no other input needs a check: the emitter's row comes from the lane's own sampler and is clamped to the scene's list,
	// and pg_surface_probe, pg_emitter_probe and pg_bsdf_probe send arbitrary floats through these functions)
	HeadProbeArgs v = {};
	v.in = *lanes;
	v.out = *out;
	v.n = n;
	v.a.shapes = scene_shapes(sc, true);
	v.a.mats = sc.mats.p;
	v.a.dir_lights.lights = sc.dir_lights.p;
	for (int c = 0; c < 4; ++c) v.a.dir_lights.bsphere[c] = sc.bsphere[c];
	v.a.emitters = sc.emitters.p; v.a.n_emitters = sc.n_emitters;
	v.a.max_depth = max_depth; v.a.frac = frac; v.a.guided = guided ? 1 : 0;
	return run_at_level(ctx, sc.general, n, stream, v, [](auto L) { return k_probe_head<decltype(L)::value>; });
}

int pg_emitter_probe(pg_context *ctx, uint64_t n, const float *d_p, const float *d_n, const float *d_e, float *d_out,
                     int32_t *d_flags, void *stream)
{
	const int rc = probe_ready(ctx, "pg_emitter_probe", true, nullptr, n, "lanes", !d_p || !d_n || !d_e || !d_out || !d_flags);
	if (rc != kProbeGo) return rc;
	const SceneState &sc = scene_state(ctx);
	PG_HIP(ctx, hipStreamSynchronize((hipStream_t)stream)); // (the caller's writes of the inputs, before the host reads them)
	// the samples are checked on the host: the emitter's index comes from e1
	std::vector<float> e(2 * n);
	PG_HIP(ctx, hipMemcpy(e.data(), d_e, e.size() * sizeof(float), hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < 2 * n; ++i)
		if (!(e[i] >= 0.0f && e[i] <= 1.0f)) return fail(ctx, PG_ERR_INVALID, "pg_emitter_probe: sample outside [0, 1]");
	// (the emitter list needs no check here: pg_scene_set_ex builds it itself from the flags of the quads and spheres it has
	// counted and from the number of directional lights, which set feature level 3 -- no caller's index enters it)
	EmitterProbeArgs a;
	a.shapes = scene_shapes(sc, false);
	a.dir_lights.lights = sc.dir_lights.p;
	for (int c = 0; c < 4; ++c) a.dir_lights.bsphere[c] = sc.bsphere[c];
	a.emitters = sc.emitters.p; a.n_emitters = sc.n_emitters;
	a.n = n; a.p = d_p; a.ng = d_n; a.e = d_e; a.out = d_out; a.flags = d_flags;
	return run_at_level(ctx, sc.general, n, stream, a, [](auto L) { return k_probe_emitter<decltype(L)::value>; });
}

int pg_surface_probe(pg_context *ctx, uint64_t n, const int32_t *d_prim, const float *d_origin, const float *d_dir,
                     const float *d_t, const float *d_uv, const float *d_ref, float *d_out, int32_t *d_flags, void *stream)
{
	const int rc = probe_ready(ctx, "pg_surface_probe", true, nullptr, n, "lanes",
	                              !d_prim || !d_origin || !d_dir || !d_t || !d_uv || !d_ref || !d_out || !d_flags);
	if (rc != kProbeGo) return rc;
	const SceneState &sc = scene_state(ctx);
	PG_HIP(ctx, hipStreamSynchronize((hipStream_t)stream)); // (the caller's writes of the inputs, before the host reads them)
	// the shape numbers are checked on the host before a lane follows them
	const int64_t n_shapes = (int64_t)sc.n_quads + sc.n_spheres + 6 * (int64_t)sc.n_boxes + (int64_t)sc.n_tris;
	std::vector<int32_t> prim(n);
	PG_HIP(ctx, hipMemcpy(prim.data(), d_prim, n * sizeof(int32_t), hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < n; ++i)
		if (prim[i] < 0 || (int64_t)prim[i] >= n_shapes) return fail(ctx, PG_ERR_INVALID, "pg_surface_probe: shape number outside the scene");
	SurfaceProbeArgs p;
	p.shapes = scene_shapes(sc, true);
	p.mats = sc.mats.p;
	p.n = n; p.n_emitters = sc.n_emitters; // (an emitter shape is in the scene's emitter list: n_emitters >= 1 wherever a lane divides by it)
	p.prim = d_prim; p.o = d_origin; p.d = d_dir; p.t = d_t; p.uv = d_uv; p.ref = d_ref; p.out = d_out; p.flags = d_flags;
	return run_at_level(ctx, sc.general, n, stream, p, [](auto L) { return k_probe_surface<decltype(L)::value>; });
}

int pg_bsdf_probe(pg_context *ctx, uint64_t n, uint64_t n_mat, const float *d_materials, const int32_t *d_material_index,
                  const float *d_wi, const float *d_wo, const float *d_u, int32_t level, float *d_value, float *d_pdf,
                  float *d_sampled_wo, float *d_sampled_pdf, float *d_weight, float *d_eta, int32_t *d_delta, void *stream)
{
	const int rc = probe_ready(ctx, "pg_bsdf_probe", false, level < 0 || level > 3 ? "level must be 0, 1, 2 or 3" : nullptr, n, "lanes",
	                              !d_materials || !d_material_index || !d_wi || !d_wo || !d_u || !d_value || !d_pdf || !d_sampled_wo ||
	                                  !d_sampled_pdf || !d_weight || !d_eta || !d_delta,
	                              n_mat == 0 || n_mat > 65536 ? "need 1..65536 material rows" : nullptr);
	if (rc != kProbeGo) return rc;
	PG_HIP(ctx, hipStreamSynchronize((hipStream_t)stream)); // (the caller's writes of the inputs, before the host reads them)
	// the rows and the row numbers are checked on the host before a lane follows them
	std::vector<float> rows(n_mat * kMaterialStride);
	PG_HIP(ctx, hipMemcpy(rows.data(), d_materials, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
	// (a probe has no textures: any index a scene could hold passes, and the kernel reads the row's plain reflectance)
	if (const char *err = check_material_rows(rows.data(), n_mat, 65536)) return fail(ctx, PG_ERR_INVALID, std::string("pg_bsdf_probe: ") + err);
	std::vector<int32_t> index(n);
	PG_HIP(ctx, hipMemcpy(index.data(), d_material_index, n * sizeof(int32_t), hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < n; ++i)
		if (index[i] < 0 || (uint64_t)index[i] >= n_mat) return fail(ctx, PG_ERR_INVALID, "pg_bsdf_probe: material index outside the table");
	BsdfProbeArgs p;
	p.n = n; p.mats = d_materials; p.mat = d_material_index; p.wi = d_wi; p.wo = d_wo; p.u = d_u;
	p.value = d_value; p.pdf = d_pdf; p.s_wo = d_sampled_wo; p.s_pdf = d_sampled_pdf; p.s_weight = d_weight; p.s_eta = d_eta;
	p.s_delta = d_delta;
	return run_at_level(ctx, level, n, stream, p, [](auto L) { return k_probe_bsdf<decltype(L)::value>; });
}

int pg_scene_intersect(pg_context *ctx, uint64_t n, const float *d_origin, const float *d_dir, const float *d_tmax,
                       int32_t any_hit, int32_t walk_form, float *d_t, int32_t *d_prim, float *d_uv, void *stream)
{
	const int rc = probe_ready(ctx, "pg_scene_intersect", true, walk_form < 0 || walk_form > 2 ? "walk_form must be 0, 1 or 2" : nullptr,
	                              n, "rays", !d_origin || !d_dir || !d_tmax || !d_t || !d_prim || !d_uv);
	if (rc != kProbeGo) return rc;
	const SceneState &sc = scene_state(ctx);
	ProbeArgs p;
	p.shapes = scene_shapes(sc, false);
	p.n = n; p.o = d_origin; p.d = d_dir; p.tmax = d_tmax; p.t = d_t; p.uv = d_uv; p.prim = d_prim;
	// the probe's own overflow strips, for this call only (freed on return, behind the wait for the kernel)
	DevBuf<uint2> ovf;
	PG_HIP(ctx, ovf.ensure((size_t)n * kOvfStack));
	p.ovf = ovf.p;
	return run_at_level(ctx, sc.general, n, stream, p, [&](auto L) {
		return any_hit ? intersect_form<decltype(L)::value, true>(walk_form) : intersect_form<decltype(L)::value, false>(walk_form);
	});
}
