// pg_render.hip -- wavefront renderer substrate around the SD-tree: what the reference's
// PathGuidingIntegrator.sample() (src/path_guiding_integrator.py:126-431) does per pass, with the
// Mitsuba calls it makes (scene.ray_intersect :185, emitter eval/pdf :189-198,
// sample_emitter_direction :213, bsdf.eval_pdf/sample :220, 272, 304, si.to_local/to_world/spawn_ray
// :219, 277, 352, sampler.next_1d/2d) implemented for the scene subset of scenes/cornell-box
// (quads, twosided diffuse BSDFs, a one-sided area emitter, perspective camera) and, in the
// kGeneral instantiations, of scenes/veach-mis (spheres, several emitters, Beckmann rough conductors).
//
// One kernel per bounce over the live rays.  The bounce itself is not written here: bounce_lane strings together the stages
// of pg_render_stages.hpp (camera_ray, stage_a1, stage_a2, stage_guide, store_slots, stage_b), the same functions the kernels
// of mesh scenes are made of (pg_render_wave.hip), at feature levels 0 and 1 -- so a bounce costs one KD descent and at most
// two quadtree descents per live lane, none for an emitter sample whose BSDF value is zero, and no intermediate wavefront
// buffers.  What is this file's own is where a path lives between bounces.  The first bounce generates its camera rays
// itself, every bounce appends its survivors to the live-ray list of the next one (one atomic per
// workgroup), and a path carries 57 B of state between bounces.  Path-vertex records go to a dense
// slot buffer (the reference's :318, stored depth-major here so that a wavefront's stores coalesce)
// that pg_process_and_splat consumes after the last bounce (:388-395).
//
// Arithmetic mirrors oracle/pg_oracle_render.c operation by operation (fp32, no contraction), so
// radiance, records and therefore the refined trees are bit-identical to the CPU restatement -- the oracle is the independent
// statement of the bounce; the device has one.
// (The microfacet helpers are inlined since round 5: kept out of line, every call cost the level-1 kernels a 32-byte
// stack frame in scratch memory -- profiles/r05/ab_fused_kernel_helpers_inlined.txt.  Registers of the kernels as they are
// now: profiles/fused_from_stages.)
#include "pg_render_stages.hpp"
#include "pg_scene_state.hpp"

namespace pg {


// One loop iteration of :179-381 for one live lane, assembled from the stages of pg_render_stages.hpp in the sequence of
// k_wave_tail's loop body; returns whether the path continues.  The fused kernels' own: the state planes (ray_d, thr, L,
// prev_p, prev_pdf, prev_quad, the sampler) indexed by lane, the ray origin made again from the previous vertex, ray casting
// without a BVH (feature levels 0 and 1 have no meshes), the radiance kept up to date in a.L.
// kFirst: the camera ray is generated here instead of being read back from a generate kernel.
// kGeneral: the scene has spheres or rough conductors (level 1); 0 compiles the all-diffuse quad scene only.
// stash (k_bounce; nullptr in the tail kernel): column threadIdx.x of a [kBounceStash][kRBlock] array in LDS, where what only
// stage_b reads waits while the SD-tree walks run -- this kernel leaves the LDS almost empty, and the walks are where its
// registers peak (tools/vgpr_liveness.py), as k_wave_shade parks its values around its walks.
constexpr int kBounceStash = 21;
typedef __attribute__((address_space(3))) float LdsFloat;
template <bool kFirst, int kGeneral, bool kStash = false>
__device__ __forceinline__ bool bounce_lane(const RenderArgs &a, const float *s_planes, const uint64_t lane,
                                            const uint64_t rec_slot, const uint32_t depth, LdsFloat *stash = nullptr)
{
	static_assert(kGeneral < 2, "mesh scenes run the split pipeline of pg_render_wave.hip");
	const uint64_t N = a.n_lanes;
	const Shapes &sh = a.shapes;
	Pcg32 rng;
	v3 ray_o, ray_d, thr, prev_p;
	float prev_pdf;
	if (kFirst) {
		camera_ray(a, lane, rng, ray_o, ray_d);
		thr = V(1, 1, 1);
		prev_p = V(0, 0, 0);
		prev_pdf = 1.0f;
	} else {
		rng.state = a.rng_state[lane];
		rng.inc = a.rng_inc[lane];
		ray_d = V(a.ray_d[lane], a.ray_d[N + lane], a.ray_d[2 * N + lane]);
		thr = V(a.thr[lane], a.thr[N + lane], a.thr[2 * N + lane]);
		prev_p = V(a.prev_p[lane], a.prev_p[N + lane], a.prev_p[2 * N + lane]);
		prev_pdf = a.prev_pdf[lane];
		// :352 spawn_ray of the previous vertex: the same three operations that produced the origin
		const uint32_t pq = a.prev_quad[lane];
		const v3 pn = normal_at<kGeneral>(sh, (int)pq, prev_p);
		float mag = (1.0f + max3(V(fabs_(prev_p.x), fabs_(prev_p.y), fabs_(prev_p.z)))) * kRayEps;
		if (dot3(pn, ray_d) < 0.0f) mag = -mag;
		ray_o = vadd(prev_p, vscale(pn, mag));
	}
	HitRec h;
	h.u = 0.0f; h.v = 0.0f;
	h.prim = intersect<kGeneral>(sh, ray_o, ray_d, __builtin_huge_valf(), h.t); // :185
	StageA A;
	// (no delta lobes at these levels: only the camera "vertex" counts as one)
	stage_a1<kGeneral>(a, rng, ray_o, ray_d, thr, prev_p, prev_pdf, kFirst, h, depth, A);
	if (kStash) { // what only stage_b reads of stage_a1's results and of the path's state: parked ahead of the shadow ray and the BSDF sample
		stash[0 * kRBlock] = thr.x; stash[1 * kRBlock] = thr.y; stash[2 * kRBlock] = thr.z;
		stash[3 * kRBlock] = A.Le.x; stash[4 * kRBlock] = A.Le.y; stash[5 * kRBlock] = A.Le.z;
		stash[6 * kRBlock] = A.bv_em.x; stash[7 * kRBlock] = A.bv_em.y; stash[8 * kRBlock] = A.bv_em.z;
		stash[9 * kRBlock] = A.em_w.x; stash[10 * kRBlock] = A.em_w.y; stash[11 * kRBlock] = A.em_w.z;
		stash[12 * kRBlock] = A.bp_em; stash[13 * kRBlock] = A.ds_pdf;
	}
	bool occluded = false;
	if (A.flags & F_NEED_SHADOW) { // :213 test_visibility
		float th;
		occluded = intersect<kGeneral, true>(sh, A.sh_o, A.sh_d, A.sh_tmax, th) >= 0;
	}
	stage_a2<kGeneral>(a, rng, A);
	if (kStash) { // ... and of stage_a2's, ahead of the SD-tree walks
		stash[14 * kRBlock] = A.bsdf_w.x; stash[15 * kRBlock] = A.bsdf_w.y; stash[16 * kRBlock] = A.bsdf_w.z; stash[17 * kRBlock] = A.bsdf_pdf;
		stash[18 * kRBlock] = A.wi.x; stash[19 * kRBlock] = A.wi.y; stash[20 * kRBlock] = A.wi.z;
	}
	// ---- the addresses of the state for the next bounce, and the radiance so far ----
	// (The addresses are made HERE, from the lane's number taken as a new value: left alone the compiler keeps the sixteen
	// 64-bit addresses it formed for the loads at the top -- the same planes -- alive through the whole bounce, 32 of this
	// kernel's 122 vector registers: tools/vgpr_liveness.py, DESIGN.md 5.7.  The radiance, which only stage_b reads, is not
	// loaded at the top for the same reason.  Level 1 asks for it ahead of the SD-tree walks, which hide the load -- its
	// registers peak in stage_a1; level 0, whose registers peak in the walks, behind them: profiles/fused_from_stages.)
	uint32_t lane32 = (uint32_t)lane;
	asm volatile("" : "+v"(lane32));
	const uint64_t ln = lane32;
	v3 L = V(0, 0, 0);
	if (!kFirst && kGeneral) L = V(a.L[ln], a.L[N + ln], a.L[2 * N + ln]);
	GuideOut g = guide_none(A.wo);
	if (guide_has_work(a, A.flags)) stage_guide(a, s_planes, rng, A.p, A.ds_d, (A.flags & F_SMP_TREE) ? V(0, 0, 0) : A.wo, A.flags, g);
	if (a.record && (A.flags & F_VALID)) store_slots(a, rec_slot, g);
	if (kStash) {
		thr = V(stash[0 * kRBlock], stash[1 * kRBlock], stash[2 * kRBlock]);
		A.Le = V(stash[3 * kRBlock], stash[4 * kRBlock], stash[5 * kRBlock]);
		A.bv_em = V(stash[6 * kRBlock], stash[7 * kRBlock], stash[8 * kRBlock]);
		A.em_w = V(stash[9 * kRBlock], stash[10 * kRBlock], stash[11 * kRBlock]);
		A.bp_em = stash[12 * kRBlock]; A.ds_pdf = stash[13 * kRBlock];
		A.bsdf_w = V(stash[14 * kRBlock], stash[15 * kRBlock], stash[16 * kRBlock]); A.bsdf_pdf = stash[17 * kRBlock];
		A.wi = V(stash[18 * kRBlock], stash[19 * kRBlock], stash[20 * kRBlock]);
	}
	if (!kFirst && !kGeneral) L = V(a.L[ln], a.L[N + ln], a.L[2 * N + ln]);
	// (ior, :357: every BSDF of these levels has eta 1, the running product stays exactly 1 and is not carried; the next origin
	// is made again from the vertex by the next bounce, above)
	float ior = 1.0f;
	bool delta;
	v3 next_o;
	const bool active_next = stage_b<kGeneral>(a, rng, thr, L, ior, A, g, occluded, ln, rec_slot, depth, next_o, ray_d, prev_pdf, delta);
	// ---- state for the next bounce; a path that ends here leaves only its radiance ----
	a.L[ln] = L.x; a.L[N + ln] = L.y; a.L[2 * N + ln] = L.z;
	if (kFirst) a.hit0[ln] = (A.flags & F_VALID) ? 1 : 0;
	if (active_next) {
		a.rng_state[ln] = rng.state;
		if (kFirst) a.rng_inc[ln] = rng.inc;
		a.ray_d[ln] = ray_d.x; a.ray_d[N + ln] = ray_d.y; a.ray_d[2 * N + ln] = ray_d.z;
		a.thr[ln] = thr.x; a.thr[N + ln] = thr.y; a.thr[2 * N + ln] = thr.z;
		a.prev_p[ln] = A.p.x; a.prev_p[N + ln] = A.p.y; a.prev_p[2 * N + ln] = A.p.z;
		a.prev_pdf[ln] = prev_pdf;
		a.prev_quad[ln] = (uint32_t)h.prim;
	}
	return active_next;
}

// One bounce of the wavefront: thread t serves the t-th entry of the live-ray list the previous
// bounce wrote, runs the loop body, and the survivors of a workgroup append themselves to the
// next list with one atomic per workgroup (order inside a workgroup is kept, so neighbouring
// pixels stay neighbours; the order of workgroups is free -- every lane's result depends on its
// own state only).
// (Scenes with triangle meshes do not come here: pg_render_wave.hip splits their bounce into a
// ray-casting, a shading and an SD-tree kernel.)
template <bool kFirst, int kGeneral>
__global__ __launch_bounds__(kRBlock) void k_bounce(RenderArgs a)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	__shared__ uint32_t s_wave[kRBlock / 64];
	__shared__ uint32_t s_base;
	__shared__ float s_stash[kBounceStash][kRBlock];
	uint64_t tid;
	bool alive;
	if (!wave_entry<kFirst>(a, tid, alive)) return; // whole workgroup past the list, or a tail launch is finishing these paths
	if (a.guided || a.record) stage_kd_planes(s_planes, a.tree); // (a recorded vertex descends the KD tree too: its accumulators)
	const uint64_t lane = alive ? (kFirst ? tid : (uint64_t)a.order_in[tid]) : 0;
	const uint64_t rec_base = kFirst ? 0 : records_before(a);
	bool cont = false;
	if (alive) cont = bounce_lane<kFirst, kGeneral, true>(a, s_planes, lane, rec_base + tid, (uint32_t)a.bounce, (LdsFloat *)&s_stash[0][threadIdx.x]);
	if (a.last) return; // nothing survives the last bounce
	const unsigned long long ballot = __ballot(cont);
	const unsigned wl = threadIdx.x & 63u, wv = threadIdx.x >> 6;
	if (wl == 0) s_wave[wv] = (uint32_t)__popcll(ballot);
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t tot = 0;
		for (int w = 0; w < kRBlock / 64; ++w) tot += s_wave[w];
		s_base = tot ? atomicAdd(&a.live_count[a.bounce], tot) : 0u;
	}
	__syncthreads();
	if (cont) {
		uint32_t off = s_base + (uint32_t)__popcll(ballot & ((1ull << wl) - 1ull));
		for (unsigned w = 0; w < wv; ++w) off += s_wave[w];
		a.order_out[off] = (uint32_t)lane;
	}
}

// See tail_checkpoint: launched before the per-bounce launch of bounce a.bounce with a grid for
// kTailPaths lanes.  The first bounce done here reads the live list like k_bounce would; after it a
// lane keeps its path (the state still goes through its global slots: the same thread reads back
// what it wrote).  Record entries of the later bounces are handed out wave by wave behind the
// entries of bounce a.bounce (a.live_count[max_depth] counts them), and the survivors of every
// bounce are added to live_count[] as the per-bounce launches would have, so the splat finds
// N + sum(live_count) entries and pg_render_live_counts reports the same numbers either way.
template <int kGeneral>
__global__ __launch_bounds__(kRBlock) void k_bounce_tail(RenderArgs a)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	const uint64_t live = (uint64_t)live_final(a, a.bounce - 1);
	if (live > kTailPaths || (uint64_t)blockIdx.x * kRBlock >= live) return;
	if (tail_took_over(a, a.bounce - 1)) return; // an earlier checkpoint already did
	if (a.guided || a.record) stage_kd_planes(s_planes, a.tree); // (a recorded vertex descends the KD tree too: its accumulators)
	bool alive = tid < live;
	const uint64_t lane = alive ? (uint64_t)a.order_in[tid] : 0;
	const uint64_t rec_base = records_before(a);
	const uint64_t tail_base = rec_base + live; // behind the entries of bounce a.bounce
	uint64_t slot = rec_base + tid;
	for (int depth = a.bounce; depth < a.max_depth; ++depth) {
		if (alive) alive = bounce_lane<false, kGeneral>(a, s_planes, lane, slot, (uint32_t)depth);
		if (!tail_next_slot(a, depth, alive, tail_base, slot)) break;
	}
}

// the split pipeline left the radiance of lane l in Lq[l] (one 16-byte entry, written where the path ended): the output
// column L (3, N), one thread per lane
__global__ __launch_bounds__(kRBlock) void k_layout_L(const uint4 *__restrict__ Lq, float *__restrict__ L, uint64_t N)
{
	const uint64_t i = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (i >= N) return;
	const uint4 q = Lq[i];
	L[i] = __uint_as_float(q.x); L[N + i] = __uint_as_float(q.y); L[2 * N + i] = __uint_as_float(q.z);
}

// :400-431: valid flag and per-pixel sums, samples of a pixel added in lane order
__global__ __launch_bounds__(kRBlock) void k_finish(RenderArgs a, uint8_t *__restrict__ valid_out,
                                                    float *__restrict__ sumL, float *__restrict__ sumL2)
{
	const uint64_t pix = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (pix >= a.n_pixels) return;
	const uint64_t N = a.n_lanes, P = a.film_pixels;
	const uint64_t gpix = global_pixel(a, pix); // the sums are full-film arrays
	const uint64_t first = pix * (uint64_t)a.spp;
	if (valid_out)
		for (int s = 0; s < a.spp; ++s) valid_out[first + s] = a.hit0[first + s];
	if (sumL && sumL2) {
		// the running sums stay in registers; the additions and their order are those of the reference
		float s1[3], s2[3];
		for (int c = 0; c < 3; ++c) { s1[c] = sumL[c * P + gpix]; s2[c] = sumL2[c * P + gpix]; }
		for (int s = 0; s < a.spp; ++s)
			for (int c = 0; c < 3; ++c) {
				const float v = a.L[c * N + first + s];
				s1[c] = s1[c] + v;
				s2[c] = s2[c] + v * v;
			}
		for (int c = 0; c < 3; ++c) { sumL[c * P + gpix] = s1[c]; sumL2[c * P + gpix] = s2[c]; }
	}
}

// k_layout_L and k_finish in ONE streaming pass, for the passes whose spp divides the workgroup (finish_streams): a workgroup
// takes kRBlock consecutive lanes -- whole pixels -- reads Lq and hit0 side by side, writes the three planes of L and the valid
// flags side by side, and hands the radiances through LDS to the threads that own a (pixel, channel) pair, which add the pixel's
// samples in lane order onto the running sums: k_finish's additions in k_finish's order.  (k_finish reads L back with one thread
// per pixel, its lanes spp floats apart: at 16 spp every load of a wave touches 64 lines.)  A pixel's samples stand spp + 1 words
// apart in LDS (spp 1: side by side), so the owners' reads spread over the banks.
__host__ __device__ constexpr int finish_pixel_stride(int spp) { return spp > 1 ? spp + 1 : 1; }
__host__ __device__ constexpr bool finish_streams(int spp) { return spp >= 1 && spp <= kRBlock && kRBlock % spp == 0; }
__global__ __launch_bounds__(kRBlock) void k_finish_stream(RenderArgs a, uint8_t *__restrict__ valid_out,
                                                           float *__restrict__ sumL, float *__restrict__ sumL2)
{
	__shared__ float s_L[3][kRBlock + kRBlock / 2]; // (the widest: spp 2, 128 pixels of stride 3)
	const uint64_t N = a.n_lanes, P = a.film_pixels;
	const uint64_t i = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	const uint32_t spp = (uint32_t)a.spp, stride = (uint32_t)finish_pixel_stride(a.spp);
	if (i < N) {
		const uint4 q = a.Lq[i];
		const float x = __uint_as_float(q.x), y = __uint_as_float(q.y), z = __uint_as_float(q.z);
		a.L[i] = x; a.L[N + i] = y; a.L[2 * N + i] = z;
		valid_out[i] = a.hit0[i];
		const uint32_t at = (threadIdx.x / spp) * stride + threadIdx.x % spp;
		s_L[0][at] = x; s_L[1][at] = y; s_L[2][at] = z;
	}
	__syncthreads();
	const uint32_t ppb = (uint32_t)kRBlock / spp; // pixels of a workgroup; pair c * ppb + p is channel c of its pixel p
	for (uint32_t k = threadIdx.x; k < 3u * ppb; k += (uint32_t)kRBlock) { // (more pairs than threads at 1 and 2 spp)
		const uint32_t c = k / ppb, p = k % ppb;
		const uint64_t pix = (uint64_t)blockIdx.x * ppb + p;
		if (pix >= a.n_pixels) continue;
		const uint64_t gpix = global_pixel(a, pix); // the sums are full-film arrays
		float s1 = sumL[c * P + gpix], s2 = sumL2[c * P + gpix];
		for (uint32_t s = 0; s < spp; ++s) {
			const float v = s_L[c][p * stride + s];
			s1 = s1 + v;
			s2 = s2 + v * v;
		}
		sumL[c * P + gpix] = s1; sumL2[c * P + gpix] = s2;
	}
}

// element-wise evaluation of the library's deterministic fp32 functions (pg_math_eval)
__global__ __launch_bounds__(kRBlock) void k_math_eval(int which, uint64_t n, const float *__restrict__ x,
                                                       float *__restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (i >= n) return;
	const float v = x[i];
	float r, c;
	switch (which) {
	case 0: r = exp_f32(v); break;
	case 1: r = log_f32(v); break;
	case 2: r = erf_f32(v); break;
	case 3: r = erfinv_f32(v); break;
	case 4: sincos_f32(v, r, c); break;
	default: sincos_f32(v, c, r); break;
	}
	out[i] = r;
}

__device__ __forceinline__ float tent1(float d)
{
	const float a = 1.0f - fabs_(d);
	return a > 0.0f ? a : 0.0f;
}

// hdrfilm with <rfilter type="tent"/>: gather form of ImageBlock::put -- pixel (x,y) collects the
// samples of its 3x3 neighbourhood (rows, then columns, then samples, ascending), so the sums have
// one order and need no atomics.  The film position of a sample is recomputed from its stream.
// Mitsuba's gaussian rfilter (hdrfilm's default, scenes/torus/scene.xml:46): stddev 0.5, radius 2
__device__ __forceinline__ float gauss1(float d)
{
	const float a = exp_f32(-2.0f * (d * d)) - exp_f32(-8.0f);
	return a > 0.0f ? a : 0.0f;
}

// kBatched (pg_film_batched): L holds spp one-sample passes traced together (pg_pass_params.batched); the film is
// developed for each of them by itself -- image s from the samples s of the neighbourhood, exactly what pg_film gives
// for the pass seed + s alone -- into out[s][3][W * H].
// With `acc` (pg_film_batched's accumulating form) the images are not written: image s is scaled and added to acc in pass
// order, acc = acc + image_s * scale in fp32 (the first one assigned when acc_set is 0) -- the running mean main.py keeps
// of an iteration's passes (:218-239), the very operations the host would make on the separate images.
template <int kFilter, bool kBatched> // kFilter: 0 tent (3x3 neighbourhood), 1 gaussian (5x5)
__global__ __launch_bounds__(kRBlock) void k_film(uint32_t seed, int spp, int W, int H,
                                                  const float *__restrict__ L, float *__restrict__ out,
                                                  uint32_t stripe_rows, uint32_t stripe_index, uint32_t stripe_count,
                                                  float *__restrict__ acc, float scale, int acc_set)
{
	constexpr int R = kFilter == 1 ? 2 : 1;
	const uint64_t npix = (uint64_t)W * (uint64_t)H, N = npix * (uint64_t)spp;
	const uint64_t o = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	if (o >= npix) return;
	const int x = (int)(o % (uint64_t)W), y = (int)(o / (uint64_t)W);
	// (pg_film_stripes: the pixels of this rank's bands only; the others keep what `out` held)
	if (stripe_count > 1u && ((uint32_t)y / stripe_rows) % stripe_count != stripe_index) return;
	const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
	for (int img = 0; img < (kBatched ? spp : 1); ++img) {
		float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, wsum = 0.0f;
		for (int ny = y - R; ny <= y + R; ++ny)
			for (int nx = x - R; nx <= x + R; ++nx) {
				if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
				const uint64_t pix = (uint64_t)ny * (uint64_t)W + (uint64_t)nx;
				for (int s = kBatched ? img : 0; s < (kBatched ? img + 1 : spp); ++s) {
					const uint64_t lane = pix * (uint64_t)spp + (uint64_t)s;
					Pcg32 rng = lane_stream(seed, spp, kBatched ? 1 : 0, pix, (uint32_t)s);
					const float jx = rng.next_f32(), jy = rng.next_f32();
					const float ddx = cx - ((float)nx + jx), ddy = cy - ((float)ny + jy);
					const float w = kFilter == 1 ? gauss1(ddx) * gauss1(ddy) : tent1(ddx) * tent1(ddy);
					a0 = a0 + w * L[lane];
					a1 = a1 + w * L[N + lane];
					a2 = a2 + w * L[2 * N + lane];
					wsum = wsum + w;
				}
			}
		const bool ok = wsum > 0.0f;
		const float r0 = ok ? a0 / wsum : 0.0f, r1 = ok ? a1 / wsum : 0.0f, r2 = ok ? a2 / wsum : 0.0f;
		if (kBatched && acc) {
			const float v0 = r0 * scale, v1 = r1 * scale, v2 = r2 * scale;
			const bool first = img == 0 && !acc_set;
			acc[o] = first ? v0 : acc[o] + v0;
			acc[npix + o] = first ? v1 : acc[npix + o] + v1;
			acc[2 * npix + o] = first ? v2 : acc[2 * npix + o] + v2;
		} else {
			float *dst = out + (uint64_t)img * 3u * npix;
			dst[o] = r0; dst[npix + o] = r1; dst[2 * npix + o] = r2;
		}
	}
}

// The same film by 16 x 16 pixel tiles, the samples' film positions made ONCE per tile.  k_film recomputes a sample's position
// (its stream's seeding and first two draws) in every pixel that looks at it -- nine times with the tent filter, 25 with the
// gaussian -- and that, not the 400 MB of radiance it reads, is where its 2.8 ms per 16-spp pass of a 1920 x 1080 film went.
// Here a workgroup first writes the positions of every sample of its tile and the filter's rim into LDS ([sample][pixel of
// the region], so that neighbouring threads read neighbouring words), then every pixel makes the very sums of k_film in their
// very order from those: the images are the same bit for bit.  Launched when the region's positions fit 64 KB of LDS
// (16 spp with either filter); k_film serves the rest.
constexpr int kFilmTile = 16;
template <int kFilter, bool kBatched>
__global__ __launch_bounds__(kFilmTile * kFilmTile) void k_film_tiled(uint32_t seed, int spp, int W, int H,
                                                                       const float *__restrict__ L, float *__restrict__ out,
                                                                       uint32_t stripe_rows, uint32_t stripe_index, uint32_t stripe_count,
                                                                       float *__restrict__ acc, float scale, int acc_set)
{
	constexpr int R = kFilter == 1 ? 2 : 1;
	constexpr int kSide = kFilmTile + 2 * R, kRegion = kSide * kSide;
	extern __shared__ float2 s_jit[]; // [spp][kRegion]
	const int tiles_x = (W + kFilmTile - 1) / kFilmTile;
	const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kFilmTile, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kFilmTile;
	for (int i = (int)threadIdx.x; i < kRegion * spp; i += kFilmTile * kFilmTile) {
		const int sidx = i / kRegion, p = i % kRegion;
		const int px = tx0 - R + p % kSide, py = ty0 - R + p / kSide;
		float2 j = make_float2(0.0f, 0.0f);
		if (px >= 0 && py >= 0 && px < W && py < H) {
			Pcg32 rng = lane_stream(seed, spp, kBatched ? 1 : 0, (uint64_t)py * (uint64_t)W + (uint64_t)px, (uint32_t)sidx);
			j.x = rng.next_f32();
			j.y = rng.next_f32();
		}
		s_jit[i] = j;
	}
	__syncthreads();
	const int x = tx0 + (int)(threadIdx.x % kFilmTile), y = ty0 + (int)(threadIdx.x / kFilmTile);
	if (x >= W || y >= H) return;
	if (stripe_count > 1u && ((uint32_t)y / stripe_rows) % stripe_count != stripe_index) return;
	const uint64_t npix = (uint64_t)W * (uint64_t)H, N = npix * (uint64_t)spp;
	const uint64_t o = (uint64_t)y * (uint64_t)W + (uint64_t)x;
	const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
	for (int img = 0; img < (kBatched ? spp : 1); ++img) {
		float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, wsum = 0.0f;
		for (int ny = y - R; ny <= y + R; ++ny)
			for (int nx = x - R; nx <= x + R; ++nx) {
				if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
				const uint64_t pix = (uint64_t)ny * (uint64_t)W + (uint64_t)nx;
				const int p = (ny - (ty0 - R)) * kSide + (nx - (tx0 - R));
				for (int sidx = kBatched ? img : 0; sidx < (kBatched ? img + 1 : spp); ++sidx) {
					const uint64_t lane = pix * (uint64_t)spp + (uint64_t)sidx;
					const float2 j = s_jit[sidx * kRegion + p];
					const float ddx = cx - ((float)nx + j.x), ddy = cy - ((float)ny + j.y);
					const float w = kFilter == 1 ? gauss1(ddx) * gauss1(ddy) : tent1(ddx) * tent1(ddy);
					a0 = a0 + w * L[lane];
					a1 = a1 + w * L[N + lane];
					a2 = a2 + w * L[2 * N + lane];
					wsum = wsum + w;
				}
			}
		const bool ok = wsum > 0.0f;
		const float r0 = ok ? a0 / wsum : 0.0f, r1 = ok ? a1 / wsum : 0.0f, r2 = ok ? a2 / wsum : 0.0f;
		if (kBatched && acc) {
			const float v0 = r0 * scale, v1 = r1 * scale, v2 = r2 * scale;
			const bool first = img == 0 && !acc_set;
			acc[o] = first ? v0 : acc[o] + v0;
			acc[npix + o] = first ? v1 : acc[npix + o] + v1;
			acc[2 * npix + o] = first ? v2 : acc[2 * npix + o] + v2;
		} else {
			float *dst = out + (uint64_t)img * 3u * npix;
			dst[o] = r0; dst[npix + o] = r1; dst[2 * npix + o] = r2;
		}
	}
}

} // namespace pg

using namespace pg;

// The buffers of one pass in flight.  pg_pass_params.slot picks one of two sets, so that two passes -- issued by the
// caller on two streams -- can be on the device at once: a pass is a chain of kernels bound by different units (BVH
// walks and SD-tree queries by the vector-memory path, shading by the vector ALUs and HBM, the splat by L2 atomics),
// and two chains out of step fill each other's gaps.  Everything a pass writes is in its set, except sdTree_current
// (integer atomics: any order) and the per-pixel sums (ordered between the sets by events, pg_render_pass).
struct PassBuf {
	// mesh scenes: ray origins, the per-bounce workspace and the BVH stacks' overflow strips (pg_render_wave.hip)
	DevBuf<uint4> st[2];       // two sets of five entries per path, swapped per bounce (pg_render_wave.hip, st_load)
	DevBuf<uint64_t> inc[2];   // and of the sampler increments
	DevBuf<uint32_t> ws;
	DevBuf<uint2> bvh_ovf;
	DevBuf<uint32_t> shadow_list;
	DevBuf<float> ray_d, thr, prev_p, prev_pdf;
	DevBuf<uint32_t> prev_quad;
	DevBuf<uint8_t> hit0;
	DevBuf<uint64_t> rng_state, rng_inc;
	DevBuf<uint32_t> order[2], live_count;
	DevBuf<uint32_t> ray_of;
	DevBuf<float> r_bsdf, r_tb, r_tr, r_nee, r_wp;
	// pg_render_sort: keys of the places (written by k_wave_trace), the sorted keys, the identity, the places in sorted
	// order, the sort's temporary storage (pg_sort.hip)
	DevBuf<uint16_t> sort_key, sort_key_out;
	DevBuf<uint32_t> sort_perm;
	DevBuf<uint4> carry[2]; // the paths' 128-byte records of a sorted bounce (RenderArgs::carry_in), two sets swapped per bounce:
	                        // k_wave_shade reads the records of its bounce and writes the next bounce's in one launch
	// which bounces are worth a sort is read off the PREVIOUS pass of this set: its live counts come back to the host
	// behind the pass (pinned memory, an event), and a bounce is sorted when at least kSortMinLive of the lanes were alive
	// going into it (scenes/torus: 24 % after the second bounce).  The sort itself covers n_sort places, a little more than
	// were alive then (wave_bounce), so its cost follows the live count; what a thin sorted bounce still pays whatever is
	// left are the sort's eight launches, the 65536 places of slack, and N-sized grids that find their lanes through the
	// permutation and their state in 128-byte records instead of planes
	uint32_t *h_live = nullptr;       // pinned, max_depth entries
	int h_live_n = 0;
	hipEvent_t ev_live = nullptr;
	bool live_pending = false, live_known = false;
	std::vector<uint32_t> live_prev;
	uint64_t live_prev_lanes = 0;
	DevBuf<uint4> Lq;    // the split pipeline's radiance by lane (RenderArgs::Lq)
	DevBuf<char> sort_tmp;
	size_t sort_tmp_bytes = 0;
	DevBuf<uint2> r_slot;   // the list names accumulators instead of positions and directions (pg_list_records)
	DevBuf<uint32_t> r_tree;
	// pg_render_record_geometry: kGeoPlanes planes beside the list (GEO_*, pg_render_dev.hpp), allocated only while the switch is
	// on; geo_lanes: the lanes of this set's most recent pass if it recorded geometry, else 0 (pg_render_export_records)
	DevBuf<uint32_t> r_geo;
	uint64_t geo_lanes = 0;
	int geo_depth = 0; // ... and its max_depth
	// pg_render_overlap: k_wave_guide beside k_wave_cast on a library-owned stream
	hipStream_t side = nullptr;
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;
	hipEvent_t ev_finish = nullptr; // recorded behind this set's k_finish: the other set's next k_finish waits for it
	bool finish_recorded = false;
	~PassBuf()
	{
		if (ev_fork) (void)hipEventDestroy(ev_fork);
		if (ev_join) (void)hipEventDestroy(ev_join);
		if (ev_finish) (void)hipEventDestroy(ev_finish);
		if (ev_live) (void)hipEventDestroy(ev_live);
		if (h_live) (void)hipHostFree(h_live);
		if (side) (void)hipStreamDestroy(side);
	}
};

// pg_render_sort: a bounce is sorted when at least 3/10 of the pass's lanes were alive going into it (last pass's counts)
constexpr uint64_t kSortMinLiveNum = 3, kSortMinLiveDen = 10;

// What an interval of pg_enable_kernel_timing is credited to (pg_read_kernel_timing): a quad scene's bounce (k_bounce_tail and
// k_bounce as one), the kernels of the split pipeline (timer_of) and its sorts, k_splat_list, and k_layout_L with k_finish (or k_finish_stream)
// (ShadeFirst: the joint form's first launch, k_wave_shade<., true> -- it walks the camera rays' closest hits itself, so it is
// the bounce's closest-hit pass and its shading kernel in one interval: counted as both, its time as shading)
enum class Timer { Bounce, Trace, ShadeA, ShadeFirst, Shadow, Guide, ShadeB, Tail, Sort, Splat, Finish };

// library-owned renderer state
struct pg_render_state {
	SceneState scene; // what pg_scene_set_ex (pg_scene.hip) made of the scene description
	DevBuf<float> ior;
	bool split_always = false; // pg_render_split_pipeline: quad scenes run the split pipeline too
	bool record_geometry = false; // pg_render_record_geometry, as the next pg_scene_set[_ex] will see it (SceneState::geometry)
	int overlap = 0;           // pg_render_overlap
	int stages = 0;            // pg_render_stages
	int sort = 0;              // pg_render_sort
	PassBuf pb[2];
	int last_slot = 0;         // of the most recent pass (pg_render_live_counts)
	// optional per-kernel timing: (kind, start, stop) event triples still to be read
	bool timing_on = false;
	struct Ev { Timer kind; hipEvent_t a, b; };
	std::vector<Ev> events;
	pg_kernel_timing acc = {};
};

namespace {
struct Timed { // records an event pair around a launch when timing is enabled
	pg_render_state *r;
	hipStream_t s;
	Timer kind;
	hipEvent_t a = nullptr, b = nullptr;
	Timed(pg_render_state *r_, hipStream_t s_, Timer kind_) : r(r_), s(s_), kind(kind_)
	{
		if (!r->timing_on) return;
		if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
		(void)hipEventRecord(a, s);
	}
	~Timed()
	{
		if (!a) return;
		(void)hipEventRecord(b, s);
		r->events.push_back({kind, a, b});
	}
};
} // namespace

static pg_render_state *rstate(pg_context *ctx)
{
	if (!ctx->render) ctx->render = new pg_render_state();
	return ctx->render;
}

SceneState &pg::scene_state(pg_context *ctx) { return rstate(ctx)->scene; }
bool pg::split_pipeline_always(pg_context *ctx) { return rstate(ctx)->split_always; }
bool pg::record_geometry_wanted(pg_context *ctx) { return rstate(ctx)->record_geometry; }

Shapes pg::scene_shapes(const SceneState &sc, bool shading_tables)
{
	Shapes shapes;
	shapes.quads = sc.quads.p; shapes.spheres = sc.spheres.p; shapes.boxes = sc.boxes.p; shapes.tris = sc.tris.p;
	shapes.tri_normals = shading_tables && sc.have_tri_normals ? sc.tri_normals.p : nullptr;
	shapes.tri_uvs = shading_tables && sc.have_tri_uvs ? sc.tri_uvs.p : nullptr;
	shapes.textures = shading_tables ? sc.textures.p : nullptr;
	shapes.texels = shading_tables ? sc.texels.p : nullptr;
	shapes.srgb_lut = shading_tables ? sc.srgb_lut.p : nullptr;
	shapes.bvh = sc.bvh.p; shapes.n_bvh_nodes = sc.n_bvh_nodes;
	shapes.n_quads = sc.n_quads; shapes.n_spheres = sc.n_spheres; shapes.n_boxes = sc.n_boxes;
	return shapes;
}

void pg::destroy_render_state(pg_context *ctx)
{
	delete ctx->render;
	ctx->render = nullptr;
}

// The buffers a pass over n_lanes lanes needs (the reference allocates its numRays x max_depth record
// arrays in setup(), path_guiding_integrator.py:93): per-lane path state, the live lists, the record
// list, and for mesh scenes the ray origins, the per-bounce workspace and the BVH stacks' overflow strips.
static int ensure_pass_buffers(pg_context *ctx, int slot, uint64_t N, bool record)
{
	pg_render_state *r = ctx->render;
	PassBuf &b = r->pb[slot];
	const int D = ctx->max_depth;
	const uint64_t S = N * (uint64_t)D;
	PG_HIP(ctx, b.hit0.ensure(N));
	if (r->scene.general < 2) {
		PG_HIP(ctx, b.ray_d.ensure(3 * N)); PG_HIP(ctx, b.thr.ensure(3 * N));
		PG_HIP(ctx, b.prev_p.ensure(3 * N)); PG_HIP(ctx, b.prev_pdf.ensure(N));
		PG_HIP(ctx, b.prev_quad.ensure(N)); PG_HIP(ctx, b.rng_state.ensure(N));
	} else {
		for (int k = 0; k < 2; ++k) { PG_HIP(ctx, b.st[k].ensure(5 * N)); PG_HIP(ctx, b.inc[k].ensure(N)); }
		PG_HIP(ctx, b.Lq.ensure(N));
		if (r->sort) { // pg_render_sort: keys, the sorted places, the paths' 128-byte records, the sort's temporary storage
			if (N > 0xfffffff0ull) return fail(ctx, PG_ERR_INVALID, "pg_render_sort: more than 2^32 lanes in one pass");
			PG_HIP(ctx, b.sort_key.ensure(N)); PG_HIP(ctx, b.sort_key_out.ensure(N)); PG_HIP(ctx, b.sort_perm.ensure(N));
			PG_HIP(ctx, b.carry[0].ensure(8 * N)); PG_HIP(ctx, b.carry[1].ensure(8 * N));
			const size_t need = sort_pairs_temp_bytes((uint32_t)N);
			if (need > b.sort_tmp_bytes) { PG_HIP(ctx, b.sort_tmp.ensure(need)); b.sort_tmp_bytes = need; }
		}
		PG_HIP(ctx, b.ws.ensure((size_t)wave_workspace_planes() * N));
		PG_HIP(ctx, b.shadow_list.ensure(N));
		// one overflow strip of the BVH stack per list position (closest-hit launches) or walking thread; a lane names its strip
		// by a 32-bit entry index (BvhStack::ovf_first)
		if ((N > kTailPaths ? N : (uint64_t)kTailPaths) * (uint64_t)kOvfStack > 0xffffffffull)
			return fail(ctx, PG_ERR_INVALID, "pg_render_pass: more lanes than the BVH stacks' overflow strips can be indexed for (2^32 / 28)");
		PG_HIP(ctx, b.bvh_ovf.ensure((size_t)kOvfStack * (N > kTailPaths ? N : kTailPaths)));
	}
	PG_HIP(ctx, b.rng_inc.ensure(N));
	PG_HIP(ctx, b.order[0].ensure(N)); PG_HIP(ctx, b.order[1].ensure(N));
	PG_HIP(ctx, b.live_count.ensure((size_t)D + 1 + 3 * (size_t)D));
	if (record) {
		PG_HIP(ctx, b.ray_of.ensure(S));
		PG_HIP(ctx, b.r_bsdf.ensure(3 * S)); PG_HIP(ctx, b.r_tb.ensure(3 * S)); PG_HIP(ctx, b.r_tr.ensure(3 * S));
		PG_HIP(ctx, b.r_wp.ensure(S));
		// (pg_list_records: 60 B per entry -- no position, no directions, one plane of radiance_nee)
		PG_HIP(ctx, b.r_nee.ensure(S));
		PG_HIP(ctx, b.r_slot.ensure(S)); PG_HIP(ctx, b.r_tree.ensure(S));
		if (r->scene.geometry) PG_HIP(ctx, b.r_geo.ensure((size_t)kGeoPlanes * S)); // (pg_render_record_geometry: 32 B more per entry)
	}
	return PG_OK;
}

// The checks of pg_render_pass's arguments, and the pass's pixel count P: the range, or this rank's rows of the stripes
// (P = 0: nothing to render)
static int check_pass(pg_context *ctx, const pg_pass_params *prm, const float *L_out, const float *sumL, const float *sumL2, uint64_t &P)
{
	if (!ctx) return PG_ERR_INVALID;
	if (!ctx->configured) return fail(ctx, PG_ERR_INVALID, "call pg_setup or pg_import first");
	if (!ctx->render || !ctx->render->scene.have_scene) return fail(ctx, PG_ERR_INVALID, "pg_render_pass: call pg_scene_set first");
	if (!prm || !L_out) return fail(ctx, PG_ERR_INVALID, "pg_render_pass: NULL pointer");
	if (prm->spp <= 0 || ctx->max_depth <= 0) return fail(ctx, PG_ERR_INVALID, "pg_render_pass: spp and max_depth must be > 0");
	if ((sumL == nullptr) != (sumL2 == nullptr)) return fail(ctx, PG_ERR_INVALID, "pg_render_pass: sumL and sumL2 go together");
	// (the pass's record list names accumulators, not positions and directions: it cannot be filtered, and must not pretend to
	// -- unless the scene was set with pg_render_record_geometry on: then the list keeps them)
	if (!ctx->is_final && ctx->filtered() && !ctx->render->scene.geometry)
		return fail(ctx, PG_ERR_INVALID, std::string("pg_render_pass: a recording pass cannot apply the splat filter set by pg_set_splat_filter (spatial ") +
		                                     (ctx->filter_spatial == PG_SPATIAL_OVERLAP_BOX ? "overlap box" : ctx->filter_spatial ? "stochastic box" : "nearest") + ", directional " +
		                                     (ctx->filter_directional ? "box" : "nearest") + "); reset it to nearest / nearest, record through pg_splat / pg_process_and_splat, or set the scene with pg_render_record_geometry on");
	PG_HIP(ctx, hipSetDevice(ctx->device));
	const pg_camera &cam = ctx->render->scene.cam;
	const uint64_t film = (uint64_t)cam.width * (uint64_t)cam.height;
	if (prm->pixel_begin > film || prm->pixel_count > film - prm->pixel_begin)
		return fail(ctx, PG_ERR_INVALID, "pg_render_pass: pixel range outside the film");
	P = prm->pixel_count ? prm->pixel_count : film - prm->pixel_begin; // 0 = to the end
	if (prm->stripe_count > 1) { // bands of stripe_rows rows dealt round-robin: this rank's rows
		if (prm->stripe_rows == 0 || prm->stripe_index >= prm->stripe_count || prm->pixel_begin != 0)
			return fail(ctx, PG_ERR_INVALID, "pg_render_pass: bad stripe parameters");
		uint64_t rows = 0;
		for (uint64_t row = 0; row < (uint64_t)cam.height; ++row)
			rows += (row / prm->stripe_rows) % prm->stripe_count == prm->stripe_index;
		if (prm->pixel_count && prm->pixel_count != rows * (uint64_t)cam.width)
			return fail(ctx, PG_ERR_INVALID, "pg_render_pass: pixel_count does not match the stripes of this rank");
		P = rows * (uint64_t)cam.width;
	}
	if (P == 0) return PG_OK;
	if (P * (uint64_t)prm->spp * (uint64_t)ctx->max_depth > 0xffffffffull)
		return fail(ctx, PG_ERR_INVALID, "pg_render_pass: more than 2^32 record slots in one pass");
	if (prm->slot < 0 || prm->slot > 1) return fail(ctx, PG_ERR_INVALID, "pg_render_pass: slot must be 0 or 1");
	return PG_OK;
}

// The kernels' argument block of a pass of P pixels in buffer set b, but for what changes per bounce
static RenderArgs pass_args(pg_context *ctx, const pg_pass_params *prm, PassBuf &b, uint64_t P, float *L_out)
{
	const pg_render_state *r = ctx->render;
	const int D = ctx->max_depth;
	RenderArgs a;
	a.tree = ctx->view();
	// the scene
	const SceneState &sc = r->scene;
	a.shapes = scene_shapes(sc, true);
	a.mats = sc.mats.p; a.emitters = sc.emitters.p; a.n_emitters = sc.n_emitters; a.ior = r->ior.p;
	a.dir_lights.lights = sc.dir_lights.p;
	for (int c = 0; c < 4; ++c) a.dir_lights.bsphere[c] = sc.bsphere[c];
	a.cam = sc.cam;
	// the pass
	a.n_lanes = P * (uint64_t)prm->spp; a.n_pixels = P; a.pixel_begin = prm->pixel_begin;
	a.stripe_rows = prm->stripe_rows; a.stripe_index = prm->stripe_index; a.stripe_count = prm->stripe_count;
	a.film_pixels = (uint64_t)r->scene.cam.width * (uint64_t)r->scene.cam.height;
	a.spp = prm->spp; a.max_depth = D; a.rr_depth = prm->rr_depth; a.seed = prm->seed; a.batched = prm->batched ? 1 : 0;
	a.guided = ctx->iteration > 1 ? 1 : 0; // :223, 250, 283
	a.record = ctx->is_final ? 0 : 1; a.store_nee = ctx->store_nee; a.frac = ctx->bsdf_fraction;
	a.dc = ctx->dc_on ? ctx->dc : nullptr;
	a.ph = ctx->ph_on ? ctx->ph_buf.p : nullptr;
	// pg_render_stages: the SD-tree calls in k_wave_shade / k_wave_shade_a, or in k_wave_guide of their own -- which
	// pg_render_overlap needs, to run them beside the shadow rays
	const bool wave = r->scene.general >= 2; // mesh scenes: the split pipeline
	a.fuse_guide = wave && r->stages < 2 && !(r->overlap & 1) ? 1 : 0;
	if (r->scene.geometry && a.record) a.fuse_guide = 0; // (pg_render_record_geometry: k_wave_guide<true> stores the geometry)
	// the buffer set
	a.ray_d = b.ray_d.p; a.thr = b.thr.p; a.L = L_out; a.prev_p = b.prev_p.p;
	a.prev_pdf = b.prev_pdf.p; a.prev_quad = b.prev_quad.p; a.hit0 = b.hit0.p;
	a.rng_state = b.rng_state.p; a.rng_inc = b.rng_inc.p; a.live_count = b.live_count.p;
	a.ray_of = b.ray_of.p; a.r_bsdf = b.r_bsdf.p; a.r_tb = b.r_tb.p;
	a.r_tr = b.r_tr.p; a.r_nee = b.r_nee.p; a.r_wp = b.r_wp.p;
	a.r_slot = b.r_slot.p; a.r_tree = b.r_tree.p;
	a.Lq = wave ? b.Lq.p : nullptr;
	a.ws = b.ws.p; a.bvh_ovf = b.bvh_ovf.p; a.shadow_list = b.shadow_list.p;
	a.cast_count = b.live_count.p + (D + 1);
	a.shadow_count = b.live_count.p + (D + 1) + 2 * D;
	a.st_in = nullptr; a.st_out = nullptr; a.inc_in = nullptr; a.inc_out = nullptr; // (set per bounce: wave_bounce)
	a.sort_key = nullptr; a.perm = nullptr; a.carry_in = nullptr; a.carry_out = nullptr; a.n_sort = 0;
	return a;
}

// Bounce `it` of a scene of the fused kernels: k_bounce, behind k_bounce_tail at a checkpoint, timed as one
static void quad_bounce(pg_render_state *r, const RenderArgs &a, int it, hipStream_t s)
{
	Timed t(r, s, Timer::Bounce);
	if (tail_checkpoint(it, a.max_depth)) { // finishes every path in one launch once few are left (see k_bounce_tail)
		const dim3 tgrid((unsigned)((kTailPaths + kRBlock - 1) / kRBlock));
		if (r->scene.general == 1) hipLaunchKernelGGL((k_bounce_tail<1>), tgrid, dim3(kRBlock), 0, s, a);
		else hipLaunchKernelGGL((k_bounce_tail<0>), tgrid, dim3(kRBlock), 0, s, a);
	}
	// every launch is sized for the whole wavefront: the live count is only known on the device,
	// and workgroups past it retire on their first instruction
	const dim3 grid((unsigned)((a.n_lanes + kRBlock - 1) / kRBlock));
	if (r->scene.general == 1) {
		if (it == 0) hipLaunchKernelGGL((k_bounce<true, 1>), grid, dim3(kRBlock), 0, s, a);
		else hipLaunchKernelGGL((k_bounce<false, 1>), grid, dim3(kRBlock), 0, s, a);
	} else {
		if (it == 0) hipLaunchKernelGGL((k_bounce<true, 0>), grid, dim3(kRBlock), 0, s, a);
		else hipLaunchKernelGGL((k_bounce<false, 0>), grid, dim3(kRBlock), 0, s, a);
	}
}

// pg_render_sort: is bounce `bounce` of a pass of N lanes in set b sorted?  Those from the second one (bounce 1) to the last one
// below sort_until, when enough lanes were alive going into it in the set's last pass (the choice changes no result: without
// counts every one of them is sorted)
static bool worth_sorting(const PassBuf &b, int bounce, int sort_until, uint64_t N)
{
	if (bounce < 1 || bounce >= sort_until) return false;
	return !b.live_known || (uint64_t)b.live_prev[bounce - 1] * kSortMinLiveDen >= N * kSortMinLiveNum;
}

// the timer of a wave stage's interval (the joint k_wave_shade counts as k_wave_shade_a: shade_ms and shade_a_ms)
static Timer timer_of(WaveStage stage)
{
	switch (stage) {
	case WaveStage::Trace: return Timer::Trace;
	case WaveStage::ShadeA: case WaveStage::Shade: return Timer::ShadeA;
	case WaveStage::Cast: return Timer::Shadow;
	case WaveStage::Guide: return Timer::Guide;
	case WaveStage::ShadeB: return Timer::ShadeB;
	case WaveStage::Tail: break;
	}
	return Timer::Tail;
}

// Bounce `it` of a mesh scene: the split pipeline's kernels (pg_render_wave.hip), each timed on its own -- the tail launch at
// a checkpoint; the closest hits (a sorted bounce: with the keys cleared before and the sort after; none for bounce 0 of the
// joint form, whose shading kernel walks the camera rays itself); then the joint shading kernel, or ShadeA, Cast, Guide (unless fused into ShadeA) and ShadeB.  pg_render_overlap runs Guide beside Cast on the
// set's side stream -- both read what ShadeA left and write planes of their own, one bound by divergent gathers into the
// tree, the other by the BVH walk's dependent loads -- except in a sorted bounce, where it runs after Cast on s.
static int wave_bounce(pg_context *ctx, PassBuf &b, RenderArgs &a, int it, int sort_until, hipStream_t s)
{
	pg_render_state *r = ctx->render;
	const uint64_t N = a.n_lanes;
	const unsigned blocks = (unsigned)((N + kRBlock - 1) / kRBlock);
	// pg_render_record_geometry: a recording pass runs the four-kernel form whatever pg_render_stages says -- its SD-tree calls
	// are k_wave_guide<true>'s and k_wave_tail<., true>'s, the only kernels that store a vertex's geometry
	uint32_t *const geo = r->scene.geometry && a.record ? b.r_geo.p : nullptr;
	auto launch = [&](WaveStage stage, hipStream_t on, unsigned grid_blocks) {
		Timed t(r, on, stage == WaveStage::Shade && it == 0 ? Timer::ShadeFirst : timer_of(stage));
		launch_wave_stage(stage, r->scene.general, it == 0, a, grid_blocks, (unsigned)ctx->n_cus, on, geo);
	};
	// the state set this bounce reads and the one its survivors are written to; the camera rays of the first
	// launch go to the set the first bounce reads
	a.st_in = b.st[it & 1].p; a.inc_in = b.inc[it & 1].p;
	a.st_out = b.st[(it + 1) & 1].p; a.inc_out = b.inc[(it + 1) & 1].p;
	const bool sorted = worth_sorting(b, it, sort_until, N);
	// (the state of a sorted bounce is in the paths' records: the tail launch reads it there)
	a.carry_in = sorted ? b.carry[it & 1].p : nullptr;
	a.sort_key = nullptr; a.perm = nullptr; a.carry_out = nullptr;
	if (tail_checkpoint(it, a.max_depth)) launch(WaveStage::Tail, s, (unsigned)((kTailPaths + kRBlock - 1) / kRBlock));
	a.sort_key = sorted ? b.sort_key.p : nullptr;
	a.carry_out = worth_sorting(b, it + 1, sort_until, N) ? b.carry[(it + 1) & 1].p : nullptr;
	const bool fork = (r->overlap & 1) && !sorted;
	if (fork && !b.side) {
		PG_HIP(ctx, hipStreamCreateWithFlags(&b.side, hipStreamNonBlocking));
		PG_HIP(ctx, hipEventCreateWithFlags(&b.ev_fork, hipEventDisableTiming));
		PG_HIP(ctx, hipEventCreateWithFlags(&b.ev_join, hipEventDisableTiming));
	}
	if (sorted) { // closest hits in list order (they write every live place's key), the sort, then everything else at k
		// the sort covers the first n_sort places: all N without counts of a previous pass, else a little more than
		// were alive then (a radix sort costs what its n costs).  Places beyond n_sort -- none, unless this pass keeps
		// more paths alive than the last -- are served in list order (k_wave_shade_a): correct either way.
		const uint64_t n_sort = b.live_known ? (uint64_t)b.live_prev[it - 1] + (uint64_t)b.live_prev[it - 1] / 32 + 65536 : N;
		a.n_sort = (uint32_t)(n_sort < N ? n_sort : N);
		PG_HIP(ctx, hipMemsetAsync(b.sort_key.p, 0xff, (size_t)a.n_sort * sizeof(uint16_t), s)); // (0xffff: a place without a path)
	}
	// (the joint form's first launch makes and walks the camera rays itself, shade_body<., true>: bounce 0 has no closest-hit
	// launch there and no Timer::Trace interval -- Timer::ShadeFirst counts the bounce)
	const bool joint = r->stages == 0 && !(r->overlap & 1) && !geo;
	if (!(joint && it == 0)) launch(WaveStage::Trace, s, blocks);
	if (sorted) {
		Timed t(r, s, Timer::Sort);
		PG_HIP(ctx, sort_places16(b.sort_tmp.p, b.sort_tmp_bytes, b.sort_key.p, b.sort_key_out.p, b.sort_perm.p, a.n_sort,
		                            a.live_count + (it - 1), s));
		a.perm = b.sort_perm.p;
	}
	if (joint) {
		launch(WaveStage::Shade, s, blocks);
		return PG_OK;
	}
	launch(WaveStage::ShadeA, s, blocks);
	if (fork) {
		PG_HIP(ctx, hipEventRecord(b.ev_fork, s));
		PG_HIP(ctx, hipStreamWaitEvent(b.side, b.ev_fork, 0));
		launch(WaveStage::Guide, b.side, blocks);
		PG_HIP(ctx, hipEventRecord(b.ev_join, b.side));
	}
	launch(WaveStage::Cast, s, blocks);
	if (fork) PG_HIP(ctx, hipStreamWaitEvent(s, b.ev_join, 0));
	else if (!a.fuse_guide) launch(WaveStage::Guide, s, blocks);
	launch(WaveStage::ShadeB, s, blocks);
	return PG_OK;
}

// the geometry planes of set b's list (stride S) as the splat kernels take them
static pg_list_geometry list_geometry(const PassBuf &b, uint64_t S)
{
	pg_list_geometry g;
	const float *f = reinterpret_cast<const float *>(b.r_geo.p);
	g.position = f + GEO_P * S; g.direction = f + GEO_WO * S; g.direction_nee = f + GEO_NEE * S;
	g.depth = b.r_geo.p + GEO_DEPTH * S;
	return g;
}

static pg_list_records list_records(const PassBuf &b)
{
	pg_list_records lr;
	lr.ray_of = b.ray_of.p; lr.bsdf = b.r_bsdf.p; lr.throughput_bsdf = b.r_tb.p; lr.throughput_radiance = b.r_tr.p;
	lr.nee_lum = b.r_nee.p; lr.wo_pdf = b.r_wp.p; lr.slot = b.r_slot.p; lr.tree = b.r_tree.p;
	return lr;
}

// Behind the bounces of a pass in buffer set `slot`: the splat of its records into sdTree_current, the output column of
// the split pipeline (k_layout_L), the valid flags and the per-pixel sums (k_finish) -- or k_finish_stream for all three
static int finish_pass(pg_context *ctx, int slot, const RenderArgs &a, uint8_t *valid_out, float *sumL, float *sumL2, hipStream_t s)
{
	pg_render_state *r = ctx->render;
	PassBuf &b = r->pb[slot];
	if (a.record) {
		Timed t(r, s, Timer::Splat);
		// the depth counters of an instrumented pass describe the bounce kernels only
		const pg_list_records lr = list_records(b);
		// (check_pass: a filter is set only with the geometry beside the list; on the initial tree every filter is the nearest deposit)
		if (r->scene.geometry && ctx->filtered_launch())
			launch_splat_list_filtered(ctx->view(), ctx->f.accum_view(), ctx->filter_args(), ctx->store_nee, a.n_lanes, a.max_depth, a.Lq, lr,
			                           list_geometry(b, a.n_lanes * (uint64_t)a.max_depth), b.live_count.p, ctx->n_cus, s);
		else
			launch_splat_list(ctx->view(), ctx->f.accum_view(), ctx->store_nee, a.n_lanes, a.max_depth, a.L, a.Lq, lr, b.live_count.p, ctx->n_cus, s);
		PG_HIP(ctx, hipGetLastError());
	}
	// (a mesh scene's pass with flags and sums whose spp divides the workgroup: one streaming kernel for both, below)
	const bool stream = r->scene.general >= 2 && a.Lq && valid_out && sumL && sumL2 && finish_streams(a.spp);
	if (r->scene.general >= 2 && !stream) {
		Timed t(r, s, Timer::Finish);
		hipLaunchKernelGGL(k_layout_L, dim3((unsigned)((a.n_lanes + kRBlock - 1) / kRBlock)), dim3(kRBlock), 0, s, b.Lq.p, a.L, a.n_lanes);
	}
	if (valid_out || sumL) {
		// the per-pixel sums are read, added to and written back (fp32: the order of the passes is part of the result,
		// :400-429): a pass of the other buffer set that was issued before this one finishes its sums first
		PassBuf &other = r->pb[1 - slot];
		if (sumL && other.finish_recorded) PG_HIP(ctx, hipStreamWaitEvent(s, other.ev_finish, 0));
		Timed t(r, s, Timer::Finish);
		if (stream)
			hipLaunchKernelGGL(k_finish_stream, dim3((unsigned)((a.n_lanes + kRBlock - 1) / kRBlock)), dim3(kRBlock), 0, s, a, valid_out,
			                   sumL, sumL2);
		else
			hipLaunchKernelGGL(k_finish, dim3((unsigned)((a.n_pixels + kRBlock - 1) / kRBlock)), dim3(kRBlock), 0, s, a, valid_out,
			                   sumL, sumL2);
		PG_HIP(ctx, hipGetLastError());
		if (sumL) {
			if (!b.ev_finish) PG_HIP(ctx, hipEventCreateWithFlags(&b.ev_finish, hipEventDisableTiming));
			PG_HIP(ctx, hipEventRecord(b.ev_finish, s));
			b.finish_recorded = true;
		}
	}
	return PG_OK;
}

// pg_render_sort decides which bounces to sort by the live counts of the set's previous pass (worth_sorting): they come
// back to the host behind a pass (pinned memory, an event) and are taken up by a later pass of the same size once there
static void take_live_counts(PassBuf &b, uint64_t N, int D)
{
	if (b.live_pending && hipEventQuery(b.ev_live) == hipSuccess) { // the previous pass's live counts have arrived
		b.live_prev.assign(b.h_live, b.h_live + b.h_live_n);
		b.live_pending = false;
		b.live_known = true;
	}
	if (b.live_known && (b.live_prev_lanes != N || (int)b.live_prev.size() != D)) b.live_known = false; // (another pass size)
}

static int send_live_counts(pg_context *ctx, PassBuf &b, uint64_t N, int D, hipStream_t s)
{
	if (!b.h_live || b.h_live_n != D) {
		if (b.h_live) (void)hipHostFree(b.h_live);
		b.h_live = nullptr;
		PG_HIP(ctx, hipHostMalloc((void **)&b.h_live, (size_t)D * sizeof(uint32_t)));
		b.h_live_n = D;
	}
	if (!b.ev_live) PG_HIP(ctx, hipEventCreateWithFlags(&b.ev_live, hipEventDisableTiming));
	if (!b.live_pending) {
		PG_HIP(ctx, hipMemcpyAsync(b.h_live, b.live_count.p, (size_t)D * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		PG_HIP(ctx, hipEventRecord(b.ev_live, s));
		b.live_pending = true;
		b.live_prev_lanes = N;
	}
	return PG_OK;
}

extern "C" {

int pg_render_pass(pg_context *ctx, const pg_pass_params *prm, float *L_out, uint8_t *valid_out, float *sumL,
                   float *sumL2, void *stream)
{
	uint64_t P = 0;
	int rc = check_pass(ctx, prm, L_out, sumL, sumL2, P);
	if (rc != PG_OK || P == 0) return rc;
	hipStream_t s = (hipStream_t)stream;
	pg_render_state *r = ctx->render;
	const int D = ctx->max_depth, slot = prm->slot;
	const uint64_t N = P * (uint64_t)prm->spp;
	PassBuf &b = r->pb[slot];
	r->last_slot = slot;
	if (sumL && (uint64_t)r->scene.cam.width * (uint64_t)r->scene.cam.height > ctx->num_rays)
		return fail(ctx, PG_ERR_INVALID, "pg_render_pass: sumL/sumL2 are sized by pg_setup's num_rays, which is smaller than the film");
	if ((rc = ensure_pass_buffers(ctx, slot, N, !ctx->is_final)) != PG_OK) return rc;
	// counters of a pass, zeroed together: live_count[D + 1] ([D]: entries handed out by the tail launch), then for
	// mesh scenes cast_count[2 D] and shadow_count[D] of the persistent ray-casting kernels
	PG_HIP(ctx, hipMemsetAsync(b.live_count.p, 0, ((size_t)D + 1 + 3 * (size_t)D) * sizeof(uint32_t), s));
	RenderArgs a = pass_args(ctx, prm, b, P, L_out);
	b.geo_lanes = r->scene.geometry && a.record ? N : 0; // (what pg_render_export_records may read of this set from now on)
	b.geo_depth = D;
	const bool wave = r->scene.general >= 2; // mesh scenes: the split pipeline
	// sorted bounces (pg_render_sort): from the second bounce (camera rays find neighbouring vertices by themselves) to
	// the bounce at whose end Russian roulette thins the list out, that one included: bounce rr_depth still shades every path
	// that came through bounce rr_depth - 1 and rolls the dice only behind that (stage_b).  So bounces 1 .. min(rr_depth,
	// D - 1) are candidates, and worth_sorting drops those of them that few lanes reach.
	const int sort_until = wave && r->sort ? (prm->rr_depth < D ? prm->rr_depth + 1 : D) : 0;
	if (sort_until > 1) take_live_counts(b, N, D);
	for (int it = 0; it < D; ++it) {
		a.bounce = it;
		a.last = it + 1 == D ? 1 : 0;
		a.order_in = b.order[it & 1].p;
		a.order_out = b.order[(it + 1) & 1].p;
		if (!wave) quad_bounce(r, a, it, s);
		else if ((rc = wave_bounce(ctx, b, a, it, sort_until, s)) != PG_OK) return rc;
	}
	PG_HIP(ctx, hipGetLastError());
	if ((rc = finish_pass(ctx, slot, a, valid_out, sumL, sumL2, s)) != PG_OK) return rc;
	if (sort_until > 1 && (rc = send_live_counts(ctx, b, N, D, s)) != PG_OK) return rc;
	if (r->timing_on) ++r->acc.passes;
	return PG_OK;
}

int pg_render_split_pipeline(pg_context *ctx, int32_t on)
{
	if (!ctx) return PG_ERR_INVALID;
	rstate(ctx)->split_always = on != 0;
	return PG_OK;
}

int pg_render_record_geometry(pg_context *ctx, int32_t on)
{
	if (!ctx) return PG_ERR_INVALID;
	rstate(ctx)->record_geometry = on != 0; // (takes effect at the next pg_scene_set[_ex]: split_pipeline_always)
	return PG_OK;
}

int pg_render_export_records(pg_context *ctx, int32_t slot, const pg_records_out *out, uint32_t *slot_out, uint32_t *d_count, void *stream)
{
	if (!ctx) return PG_ERR_INVALID;
	if (!ctx->configured) return fail(ctx, PG_ERR_INVALID, "call pg_setup or pg_import first");
	if (slot < 0 || slot > 1) return fail(ctx, PG_ERR_INVALID, "pg_render_export_records: slot must be 0 or 1");
	if (!out || !d_count || !out->position || !out->direction || !out->radiance || !out->wo_pdf || !out->direction_nee ||
	    !out->radiance_nee_lum)
		return fail(ctx, PG_ERR_INVALID, "pg_render_export_records: NULL pointer");
	if (!ctx->render || ctx->render->pb[slot].geo_lanes == 0)
		return fail(ctx, PG_ERR_INVALID, "pg_render_export_records: the most recent pass of this buffer set recorded no geometry "
		                                 "(a recording pass of a scene set with pg_render_record_geometry on does)");
	PG_HIP(ctx, hipSetDevice(ctx->device));
	const PassBuf &b = ctx->render->pb[slot];
	const uint64_t N = b.geo_lanes, S = N * (uint64_t)b.geo_depth;
	launch_export_list_records(N, b.geo_depth, b.Lq.p, list_records(b), list_geometry(b, S), b.live_count.p, *out, slot_out, d_count,
	                           ctx->n_cus, (hipStream_t)stream);
	PG_HIP(ctx, hipGetLastError());
	return PG_OK;
}

int pg_render_overlap(pg_context *ctx, int32_t mode)
{
	if (!ctx) return PG_ERR_INVALID;
	if (mode < 0 || mode > 1) return fail(ctx, PG_ERR_INVALID, "pg_render_overlap: mode must be 0 or 1");
	rstate(ctx)->overlap = mode; // (the side stream of a buffer set is made by the first pass that needs it)
	return PG_OK;
}

int pg_render_stages(pg_context *ctx, int32_t mode)
{
	if (!ctx) return PG_ERR_INVALID;
	if (mode < 0 || mode > 2) return fail(ctx, PG_ERR_INVALID, "pg_render_stages: mode must be 0, 1 or 2");
	rstate(ctx)->stages = mode;
	return PG_OK;
}

int pg_render_sort(pg_context *ctx, int32_t on)
{
	if (!ctx) return PG_ERR_INVALID;
	rstate(ctx)->sort = on != 0;
	return PG_OK;
}

int pg_render_reserve(pg_context *ctx, uint64_t n_lanes)
{
	if (!ctx) return PG_ERR_INVALID;
	if (!ctx->configured) return fail(ctx, PG_ERR_INVALID, "call pg_setup or pg_import first");
	if (!ctx->render || !ctx->render->scene.have_scene) return fail(ctx, PG_ERR_INVALID, "pg_render_reserve: call pg_scene_set first");
	if (ctx->max_depth <= 0 || n_lanes == 0) return fail(ctx, PG_ERR_INVALID, "pg_render_reserve: max_depth and n_lanes must be > 0");
	if (n_lanes * (uint64_t)ctx->max_depth > 0xffffffffull) return fail(ctx, PG_ERR_INVALID, "pg_render_reserve: more than 2^32 record slots in one pass");
	PG_HIP(ctx, hipSetDevice(ctx->device));
	// The pass buffers first: they are what this call is for, and what a pass cannot run without.
	const int rc = ensure_pass_buffers(ctx, 0, n_lanes, true); // (a second set, pg_pass_params.slot 1, is allocated by its first pass)
	if (rc != PG_OK) return rc;
	// Then, where memory is plentiful, the quadtree jump tables' buffer at its budget: while the SD-tree of a real render is
	// trained the tables grow towards it (64 KB per quadtree, 1.4 GB at the veach-ajar bench tree), and a fresh allocation of
	// hundreds of megabytes in the middle of a refine is the one thing that makes a 3 ms refine take 25 or 84 ms on some boxes
	// (bench.py's exchange_refine_ms on a slow-to-allocate box, round 5).  It is an OPTIMISATION of allocation time only -- the
	// resolution a forest gets is a function of the forest and the budget alone (pg_refine.hip), with or without it -- so it is
	// taken only
	//   * for a pass of a real render (>= 2^20 lanes) and unless $PGSD_JUMP_TABLE_RESERVE is 0,
	//   * AFTER the pass buffers, and only while the device still has four times the budget free: a context on a crowded
	//     device (ranks of a rehearsal sharing one GPU, a small-memory configuration) leaves the memory alone and its refines
	//     allocate what their forests need, as before round 5,
	//   * without ever failing the call: a refused allocation changes nothing.
	const char *rsv = getenv("PGSD_JUMP_TABLE_RESERVE");
	const bool want_reserve = !(rsv && rsv[0] == '0');
	if (want_reserve && n_lanes >= (1ull << 20) && ctx->f.jump.cap * sizeof(QuadJump) < ctx->jump_budget) {
		size_t free_b = 0, total_b = 0;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (uint64_t)free_b >= 4ull * ctx->jump_budget) {
			DevBuf<QuadJump> big;
			if (big.ensure((size_t)(ctx->jump_budget / sizeof(QuadJump))) == hipSuccess) {
				const size_t in_use = ctx->f.jump_valid ? ((size_t)ctx->f.n_trees << (2 * ctx->f.jump_bits)) : 0;
				// (synchronous copy + device synchronisation: nothing in flight reads the old table when it is freed with `big`)
				if ((in_use == 0 || hipMemcpy(big.p, ctx->f.jump.p, in_use * sizeof(QuadJump), hipMemcpyDeviceToDevice) == hipSuccess) &&
				    hipDeviceSynchronize() == hipSuccess)
					ctx->f.jump.swap(big);
				else (void)hipGetLastError();
			} else (void)hipGetLastError();
		} else (void)hipGetLastError();
	}
	return PG_OK;
}

int pg_film_tent(pg_context *ctx, uint32_t seed, int32_t spp, const float *L, float *image_out, void *stream)
{
	return pg_film(ctx, PG_FILTER_TENT, seed, spp, L, image_out, stream);
}

int pg_film(pg_context *ctx, int32_t filter, uint32_t seed, int32_t spp, const float *L, float *image_out, void *stream)
{
	return pg_film_stripes(ctx, filter, seed, spp, L, image_out, 0, 0, 0, stream);
}

static int film_launch(pg_context *ctx, int32_t filter, bool batched, uint32_t seed, int32_t spp, const float *L, float *image_out,
                       uint32_t stripe_rows, uint32_t stripe_index, uint32_t stripe_count, void *stream, float *acc = nullptr,
                       float scale = 1.0f, int acc_set = 0)
{
	if (!ctx) return PG_ERR_INVALID;
	if (!ctx->render || !ctx->render->scene.have_scene) return fail(ctx, PG_ERR_INVALID, "pg_film: call pg_scene_set first");
	if (!L || (!image_out && !acc) || spp <= 0) return fail(ctx, PG_ERR_INVALID, "pg_film: NULL pointer or spp <= 0");
	if (stripe_count > 1 && (stripe_rows == 0 || stripe_index >= stripe_count)) return fail(ctx, PG_ERR_INVALID, "pg_film_stripes: bad stripe parameters");
	if (filter != PG_FILTER_TENT && filter != PG_FILTER_GAUSSIAN) return fail(ctx, PG_ERR_INVALID, "pg_film: unknown filter");
	PG_HIP(ctx, hipSetDevice(ctx->device));
	const pg_camera &cam = ctx->render->scene.cam;
	const uint64_t npix = (uint64_t)cam.width * (uint64_t)cam.height;
	const dim3 grid((unsigned)((npix + kRBlock - 1) / kRBlock)), block(kRBlock);
	hipStream_t st = (hipStream_t)stream;
	// by tiles with the samples' film positions staged in LDS where those fit (k_film_tiled), else pixel by pixel
	const int side = kFilmTile + 2 * (filter == PG_FILTER_GAUSSIAN ? 2 : 1);
	const size_t lds = (size_t)side * side * (size_t)spp * sizeof(float2);
	if (lds <= 64 * 1024) {
		const dim3 tgrid((unsigned)(((cam.width + kFilmTile - 1) / kFilmTile) * ((cam.height + kFilmTile - 1) / kFilmTile))), tblock(kFilmTile * kFilmTile);
#define PG_FILM_T(F, B)                                                                                                              \
	do {                                                                                                                             \
		if (lds > 48 * 1024)                                                                                                         \
			PG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(k_film_tiled<F, B>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
		hipLaunchKernelGGL((k_film_tiled<F, B>), tgrid, tblock, lds, st, seed, spp, cam.width, cam.height, L, image_out, stripe_rows, stripe_index, \
		                   stripe_count, acc, scale, acc_set);                                                                        \
	} while (0)
		if (filter == PG_FILTER_GAUSSIAN) { if (batched) PG_FILM_T(1, true); else PG_FILM_T(1, false); }
		else { if (batched) PG_FILM_T(0, true); else PG_FILM_T(0, false); }
#undef PG_FILM_T
		PG_HIP(ctx, hipGetLastError());
		return PG_OK;
	}
#define PG_FILM(F, B) hipLaunchKernelGGL((k_film<F, B>), grid, block, 0, st, seed, spp, cam.width, cam.height, L, image_out, stripe_rows, stripe_index, stripe_count, acc, scale, acc_set)
	if (filter == PG_FILTER_GAUSSIAN) { if (batched) PG_FILM(1, true); else PG_FILM(1, false); }
	else { if (batched) PG_FILM(0, true); else PG_FILM(0, false); }
#undef PG_FILM
	PG_HIP(ctx, hipGetLastError());
	return PG_OK;
}

int pg_film_stripes(pg_context *ctx, int32_t filter, uint32_t seed, int32_t spp, const float *L, float *image_out,
                    uint32_t stripe_rows, uint32_t stripe_index, uint32_t stripe_count, void *stream)
{
	return film_launch(ctx, filter, false, seed, spp, L, image_out, stripe_rows, stripe_index, stripe_count, stream);
}

int pg_film_batched(pg_context *ctx, int32_t filter, uint32_t seed, int32_t n_passes, const float *L, float *images_out,
                    uint32_t stripe_rows, uint32_t stripe_index, uint32_t stripe_count, void *stream)
{
	return film_launch(ctx, filter, true, seed, n_passes, L, images_out, stripe_rows, stripe_index, stripe_count, stream);
}

int pg_film_batched_accumulate(pg_context *ctx, int32_t filter, uint32_t seed, int32_t n_passes, const float *L, float *acc_io,
                               float scale, int32_t acc_has_value, uint32_t stripe_rows, uint32_t stripe_index,
                               uint32_t stripe_count, void *stream)
{
	if (!acc_io) return fail(ctx, PG_ERR_INVALID, "pg_film_batched_accumulate: NULL accumulator");
	return film_launch(ctx, filter, true, seed, n_passes, L, nullptr, stripe_rows, stripe_index, stripe_count, stream, acc_io, scale,
	                   acc_has_value ? 1 : 0);
}

int pg_math_eval(pg_context *ctx, int32_t which, uint64_t n, const float *x, float *out, void *stream)
{
	if (!ctx) return PG_ERR_INVALID;
	if (which < 0 || which > 5 || (n && (!x || !out))) return fail(ctx, PG_ERR_INVALID, "pg_math_eval: bad arguments");
	if (n == 0) return PG_OK;
	PG_HIP(ctx, hipSetDevice(ctx->device));
	hipLaunchKernelGGL(k_math_eval, dim3((unsigned)((n + kRBlock - 1) / kRBlock)), dim3(kRBlock), 0, (hipStream_t)stream,
	                   which, n, x, out);
	PG_HIP(ctx, hipGetLastError());
	return PG_OK;
}

int pg_render_live_counts(pg_context *ctx, uint32_t *out, int32_t n)
{
	if (!ctx || !out || n < 0) return PG_ERR_INVALID;
	if (!ctx->render || !ctx->render->pb[ctx->render->last_slot].live_count.p) return fail(ctx, PG_ERR_INVALID, "pg_render_live_counts: no pass rendered yet");
	PassBuf &b = ctx->render->pb[ctx->render->last_slot];
	PG_HIP(ctx, hipSetDevice(ctx->device));
	PG_HIP(ctx, hipDeviceSynchronize());
	int m = n < ctx->max_depth ? n : ctx->max_depth;
	if ((size_t)m > b.live_count.cap) m = (int)b.live_count.cap;
	PG_HIP(ctx, hipMemcpy(out, b.live_count.p, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return PG_OK;
}

int pg_enable_kernel_timing(pg_context *ctx, int32_t on)
{
	if (!ctx) return PG_ERR_INVALID;
	rstate(ctx)->timing_on = on != 0;
	return PG_OK;
}

int pg_read_kernel_timing(pg_context *ctx, pg_kernel_timing *out, int32_t reset)
{
	if (!ctx || !out) return PG_ERR_INVALID;
	PG_HIP(ctx, hipSetDevice(ctx->device));
	pg_render_state *r = rstate(ctx);
	for (auto &e : r->events) {
		float ms = 0.0f;
		PG_HIP(ctx, hipEventSynchronize(e.b));
		PG_HIP(ctx, hipEventElapsedTime(&ms, e.a, e.b));
		switch (e.kind) {
		case Timer::Bounce: r->acc.bounce_ms += ms; ++r->acc.bounce_launches; break;
		case Timer::Trace: r->acc.trace_ms += ms; r->acc.bounce_ms += ms; ++r->acc.trace_launches; ++r->acc.bounce_launches; break;
		case Timer::ShadeA: r->acc.shade_ms += ms; r->acc.shade_a_ms += ms; r->acc.bounce_ms += ms; break;
		case Timer::ShadeFirst:
			r->acc.shade_ms += ms; r->acc.shade_a_ms += ms; r->acc.bounce_ms += ms; ++r->acc.trace_launches; ++r->acc.bounce_launches;
			break;
		case Timer::Shadow: r->acc.shadow_ms += ms; r->acc.bounce_ms += ms; break;
		case Timer::Guide: r->acc.guide_ms += ms; r->acc.bounce_ms += ms; ++r->acc.guide_launches; break;
		case Timer::ShadeB: r->acc.shade_ms += ms; r->acc.shade_b_ms += ms; r->acc.bounce_ms += ms; break;
		case Timer::Tail: r->acc.tail_ms += ms; r->acc.bounce_ms += ms; break;
		case Timer::Sort: r->acc.sort_ms += ms; r->acc.bounce_ms += ms; break;
		case Timer::Splat: r->acc.splat_ms += ms; ++r->acc.splat_launches; break;
		case Timer::Finish: r->acc.finish_ms += ms; break;
		}
		(void)hipEventDestroy(e.a);
		(void)hipEventDestroy(e.b);
	}
	r->events.clear();
	*out = r->acc;
	if (reset) r->acc = pg_kernel_timing{};
	return PG_OK;
}

} // extern "C"
