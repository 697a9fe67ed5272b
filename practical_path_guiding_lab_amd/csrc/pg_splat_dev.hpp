// pg_splat_dev.hpp -- what the recording kernels do to one record, stated once (pg_kernels_splat.hip: the nearest splats, the
// renderer's record list and the two compactions; pg_kernels_filter.hip: the box-filtered, jittered and overlap splats):
// processPathData and the keep test for a dense slot and for a list entry, the record's two quadtree leaves, what one
// (direction, weight) pair adds and where, the cooperative add that sends an accumulator's four words out in one
// wave-instruction, the first iteration's single-accumulator sum, a compacted output record, and the strided launch grid.
#pragma once

#include "pg_descent.hpp"
#include "pg_kernels.hpp"

namespace pg {

constexpr int kBlock = 256; // threads of every recording workgroup
static_assert(kBlock == kStageThreads, "stage_kd_planes copies one plane per thread");

constexpr uint32_t kNoRay = 0xffffffffu; // pg_list_records.ray_of: the path left the scene at this entry

__device__ __forceinline__ TreeHead load_head_s(const TreeHead *h, uint32_t t)
{
	const uint2 v = gather8(h + t);
	TreeHead r;
	r.root_rec = v.x;
	r.root_irr = __uint_as_float(v.y);
	return r;
}

struct SlotAdd { // what one (direction, weight) pair adds, and where
	long long *ptr; // accumulator base (kAccWords words), nullptr = nothing to add
	long long w0, w1, w2, w3;
};

// quadtree.py:398-441 for one (direction, weight) pair whose leaf has been found -- the root of quadtree `tree`, or the child
// that accumulator `slot` = rec * 4 + child names; `count` goes to word 3
__device__ __forceinline__ SlotAdd slot_add(const AccumView &a, bool is_root, uint32_t tree, uint32_t slot, float w, long long count)
{
	const Limbs q = quantize_weight(w);
	SlotAdd s;
	s.ptr = is_root ? a.root_acc + (size_t)kAccWords * tree : a.rec_acc + (size_t)kAccWords * slot;
	s.w0 = q.l0; s.w1 = q.l1; s.w2 = q.l2; s.w3 = count;
	return s;
}

// the same for a pair whose leaf a walk has just looked for
__device__ __forceinline__ SlotAdd plan_dir(const AccumView &a, uint32_t tree, const LeafCursor &c, float w, long long count)
{
	SlotAdd s = {nullptr, 0, 0, 0, 0};
	if (c.found) s = slot_add(a, c.is_root, tree, c.slot, w, count);
	return s;
}

// QuadTree.addDataPropagate's two leaf lookups (quadtree.py:389-464) in quadtree `tree`: the path direction's cursor in `cp`,
// the emitter direction's in `cn`.  The tree's head and the jump-table entries of the two directions need the tree's number
// only: three gathers in flight at once instead of the entries behind the head.  counted: the record's count goes to this
// tree -- to its fallback counter, should the path direction reach no leaf (outside the unit square).
__device__ __forceinline__ void find_record_leaves(const TreeView &t, const AccumView &a, int store_nee, uint32_t tree, bool counted,
                                                   float dx, float dy, float nx, float ny, TreeHead &head, LeafCursor &cp,
                                                   LeafCursor &cn)
{
	head = load_head_s(t.head, tree);
	const JumpPre pre_p = jump_prefetch(t.jump, tree, dx, dy, in_unit_square(dx, dy));
	const JumpPre pre_n = jump_prefetch(t.jump, tree, nx, ny, store_nee != 0 && in_unit_square(nx, ny));
	cp = leaf_cursor_pre(head, dx, dy, true, pre_p);
	cn = leaf_cursor_pre(head, nx, ny, store_nee != 0, pre_n);
	quad_find_leaf_slots2(t.rec, cp, cn);
	if (counted && !cp.found) atomicAdd(a.leaf_count + tree, 1ull);
}

// The exchange below stays inside one wave (each wave owns its 64 entries of s_val / s_ptr), and a
// wave's LDS operations execute in order: ordering the compiler's view is all that is needed, no
// workgroup barrier (which would make every wave wait for the slowest descent of the workgroup).
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// Every thread of the wave calls this (convergent).  Lane L of a wave issues word (L & 3) of
// the record held by lane r*16 + (L >> 2) in round r: the four words of one accumulator leave in
// one wave-instruction from four adjacent lanes.
__device__ __forceinline__ void coop_add(const SlotAdd &s, long long *s_val, unsigned long long *s_ptr)
{
	const unsigned t = threadIdx.x;
	wave_lds_sync(); // the previous call's reads are done
	s_val[4 * t + 0] = s.w0;
	s_val[4 * t + 1] = s.w1;
	s_val[4 * t + 2] = s.w2;
	s_val[4 * t + 3] = s.w3;
	const unsigned long long mine = reinterpret_cast<unsigned long long>(s.ptr);
	s_ptr[t] = mine;
	wave_lds_sync();
	const unsigned lane = t & 63u, wbase = t & ~63u, word = lane & 3u;
	// Lanes of a wave often add to the SAME accumulator (the NEE direction of a small light is the same for a whole surface;
	// coarse quadtree cells) -- and not only neighbouring lanes: a sorted bounce puts the vertices of one spatial cell side by
	// side, in no order inside the cell, so the same target comes back every few lanes.  Every lane finds the LOWEST lane of
	// its wave with its target (eight ballots on a hash of the address pick the candidates, the candidate's address is
	// compared: a collision of the hash only loses a merge), adds its four words to that lane's in LDS (64-bit integer adds:
	// exact, any order) and drops out -- one update per distinct target of the wave instead of one per run of neighbours
	// (rounds 1-5), which the memory side serialises.
	const unsigned hkey = (unsigned)((mine >> 5) ^ (mine >> 13) ^ (mine >> 21)) & 255u;
	unsigned long long peers = __ballot(mine != 0);
#pragma unroll
	for (int b = 0; b < 8; ++b) {
		const unsigned long long m = __ballot(mine != 0 && ((hkey >> b) & 1u));
		peers &= ((hkey >> b) & 1u) ? m : ~m;
	}
	const unsigned leader = mine != 0 ? (unsigned)__builtin_ctzll(peers) : lane; // (a lane with a target is its own peer)
	const bool follower = mine != 0 && leader != lane && s_ptr[wbase + leader] == mine;
	if (follower) {
		unsigned long long *dst = reinterpret_cast<unsigned long long *>(s_val + 4 * (wbase + leader));
		if (s.w0) atomicAdd(dst + 0, (unsigned long long)s.w0);
		if (s.w1) atomicAdd(dst + 1, (unsigned long long)s.w1);
		if (s.w2) atomicAdd(dst + 2, (unsigned long long)s.w2);
		if (s.w3) atomicAdd(dst + 3, (unsigned long long)s.w3);
	}
	wave_lds_sync(); // every follower has added
	if (follower) s_ptr[t] = 0;
	wave_lds_sync();
#pragma unroll
	for (unsigned r = 0; r < 4; ++r) {
		const unsigned src = wbase + r * 16u + (lane >> 2);
		const long long v = s_val[4 * src + word];
		long long *p = reinterpret_cast<long long *>(s_ptr[src]);
		if (p != nullptr && v != 0) atomicAdd(reinterpret_cast<unsigned long long *>(p + word), (unsigned long long)v);
	}
}

// processPathData's incident radiance of a vertex (path_guiding_integrator.py:434-453, :466): per channel, what the path
// gathered behind the vertex, divided back through the throughput and the bsdf ...
__device__ __forceinline__ float incident_channel(float lf, float throughput_radiance, float throughput_bsdf, float bsdf)
{
	float out = (lf - throughput_radiance) / throughput_bsdf;
	if (out != out) out = 0.0f;                         // :444
	float v = out / bsdf;
	if (v != v) v = 0.0f;                               // :449
	return v;
}

// ... and the luminance of the three, which the tree takes
__device__ __forceinline__ float incident_radiance(const float (&in)[3])
{
	float radiance = luminance(in[0], in[1], in[2]);    // :452
	if (radiance != radiance) radiance = 0.0f;          // :466
	return radiance;
}

// scatterDataIntoSDTree's filter (:470-478)
__device__ __forceinline__ bool keeps_record(float radiance, float nee_lum, float wo_pdf)
{
	const bool both_zero = (radiance == 0.0f) && (nee_lum == 0.0f); // :470-472
	return !both_zero && !(wo_pdf == 0.0f) && !(wo_pdf != wo_pdf);  // :475-478
}

// processPathData + the filter for slot g of the reference's dense record buffer.  Returns keep; outputs the tree's inputs.
__device__ __forceinline__ bool process_slot(uint64_t g, uint64_t S, uint64_t num_rays, uint64_t ray, bool active,
                                             const float *__restrict__ l_final, const pg_dense_records &r,
                                             float &radiance, float &nee_lum, float &wp)
{
	radiance = 0.0f; nee_lum = 0.0f; wp = 0.0f;
	if (!active) return false; // (an unused slot, or a path that left the scene: nothing to read)
	float in[3], nee[3];
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		in[ch] = incident_channel(l_final[ch * num_rays + ray], r.throughput_radiance[ch * S + g], r.throughput_bsdf[ch * S + g],
		                          r.bsdf[ch * S + g]);
		float e = r.radiance_nee[ch * S + g];
		if (e != e) e = 0.0f;                               // :467
		nee[ch] = e;
	}
	radiance = incident_radiance(in);
	nee_lum = luminance(nee[0], nee[1], nee[2]);
	wp = r.wo_pdf[g];
	return keeps_record(radiance, nee_lum, wp);
}

// The same for entry g of the renderer's record list (pg_list_records; planes of stride S).  The list is read once, front to
// back: streaming loads keep it from pushing the accumulators out of L2 (8.0 -> 7.65 ms per step).  The path's final
// radiance is the one gather: the 16-byte entry of l_final_q where the pass keeps one (the split pipeline), else the planar
// l_final.  Returns keep; `ray` is the entry's path.
__device__ __forceinline__ bool process_list_entry(uint64_t g, uint64_t S, uint64_t num_rays, const float *l_final,
                                                   const uint4 *l_final_q, const pg_list_records &r, uint32_t &ray,
                                                   float &radiance, float &nee_lum, float &wp)
{
#define PG_LD(p) __builtin_nontemporal_load(p)
	radiance = 0.0f; nee_lum = 0.0f; wp = 0.0f;
	ray = PG_LD(r.ray_of + g);
	if (ray == kNoRay) return false;
	float in[3], lf[3];
	if (l_final_q) {
		const uint4 q = l_final_q[ray];
		lf[0] = __uint_as_float(q.x); lf[1] = __uint_as_float(q.y); lf[2] = __uint_as_float(q.z);
	} else {
		lf[0] = l_final[ray]; lf[1] = l_final[num_rays + ray]; lf[2] = l_final[2 * num_rays + ray];
	}
#pragma unroll
	for (int ch = 0; ch < 3; ++ch)
		in[ch] = incident_channel(lf[ch], PG_LD(r.throughput_radiance + ch * S + g), PG_LD(r.throughput_bsdf + ch * S + g),
		                          PG_LD(r.bsdf + ch * S + g));
	radiance = incident_radiance(in);
	nee_lum = PG_LD(r.nee_lum + g);
	wp = PG_LD(r.wo_pdf + g);
#undef PG_LD
	return keeps_record(radiance, nee_lum, wp);
}

// entries of the list: the first bounce visits every path, bounce b + 1 the survivors of bounce b
__device__ __forceinline__ uint64_t list_entries(uint64_t num_rays, int32_t max_depth, const uint32_t *live_count)
{
	uint64_t total = num_rays;
	for (int b = 0; b + 1 < max_depth; ++b) total += live_count[b];
	return total;
}

__device__ __forceinline__ unsigned long long wave_sum_s(unsigned long long v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// First iteration: one KD leaf owning a single-leaf quadtree (kdtree.py:122, quadtree.py:355), so every record of the pass
// lands in the same accumulator.  One word takes ~11 ns per atomic: a thread sums its adds here, and the workgroup sends
// four atomics instead of two per record.
struct SingleLeafSum {
	long long v[4] = {0, 0, 0, 0};

	// (uniform over the workgroup: flush() holds barriers)
	static __device__ __forceinline__ bool applies(const TreeView &t) { return t.n_rec == 0 && t.n_trees == 1; }

	__device__ __forceinline__ void add(const SlotAdd &path, const SlotAdd &nee)
	{
		if (path.ptr) { v[0] += path.w0; v[1] += path.w1; v[2] += path.w2; v[3] += path.w3; }
		if (nee.ptr) { v[0] += nee.w0; v[1] += nee.w1; v[2] += nee.w2; v[3] += nee.w3; }
	}

	// every thread of the workgroup calls this, once, behind its loop; s_val: coop_add's exchange buffer
	__device__ __forceinline__ void flush(const AccumView &a, long long *s_val) const
	{
		__syncthreads();
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const unsigned long long sw = wave_sum_s((unsigned long long)v[k]);
			if ((threadIdx.x & 63) == 0) s_val[(threadIdx.x >> 6) * 4 + k] = (long long)sw;
		}
		__syncthreads();
		if (threadIdx.x < 4) {
			unsigned long long tot = 0;
			for (int w = 0; w < kBlock / 64; ++w) tot += (unsigned long long)s_val[w * 4 + threadIdx.x];
			if (tot) atomicAdd(reinterpret_cast<unsigned long long *>(a.root_acc + threadIdx.x), tot);
		}
	}
};

// kept record k of a compacted stream (pg_records_out, planes of stride S): entry g of the source planes with its processed values
__device__ __forceinline__ void store_kept_record(const pg_records_out &o, uint64_t k, uint64_t S, const float *position,
                                                  const float *direction, const float *direction_nee, uint64_t g, float radiance,
                                                  float wp, float nee_lum)
{
	o.position[k] = position[g];
	o.position[S + k] = position[S + g];
	o.position[2 * S + k] = position[2 * S + g];
	o.direction[k] = direction[g];
	o.direction[S + k] = direction[S + g];
	o.direction_nee[k] = direction_nee[g];
	o.direction_nee[S + k] = direction_nee[S + g];
	o.radiance[k] = radiance;
	o.wo_pdf[k] = wp;
	o.radiance_nee_lum[k] = nee_lum;
}

// A fixed grid striding over the 256-entry tiles of S slots (the list's length is known only on the device), enough
// workgroups per CU to even out tiles of unequal cost.  n_cus: the device's compute units, positive (pg_context: 256
// until pg_create has read the device's count).
constexpr unsigned kSplatGroupsPerCu = 64; // measured (round 2): 8 -> 847, 16 -> 798, 32 -> 746, 64 -> 726, 128 -> 755 us on cornell-box

static inline dim3 strided_grid(uint64_t S, int n_cus)
{
	const uint64_t tiles = (S + kBlock - 1) / kBlock, cap = (uint64_t)n_cus * kSplatGroupsPerCu;
	return dim3((unsigned)(tiles < cap ? tiles : cap));
}

static inline dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

} // namespace pg
