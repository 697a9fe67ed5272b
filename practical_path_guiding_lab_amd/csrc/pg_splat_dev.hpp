// pg_splat_dev.hpp -- device functions shared by the recording kernels (pg_kernels_splat.hip: nearest / nearest;
// pg_kernels_filter.hip: the box-filtered and jittered splats): what one (direction, weight) pair adds and where, the
// cooperative add that sends an accumulator's four words out in one wave-instruction, and processPathData for a dense slot.
#pragma once

#include "pg_descent.hpp"
#include "pg_kernels.hpp"

namespace pg {

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

// quadtree.py:398-441 for one (direction, weight) pair whose leaf has been found; `count` goes to word 3
__device__ __forceinline__ SlotAdd plan_dir(const AccumView &a, uint32_t tree, const LeafCursor &c, float w,
                                            long long count)
{
	SlotAdd s = {nullptr, 0, 0, 0, 0};
	if (!c.found) return s;
	const Limbs q = quantize_weight(w);
	s.ptr = c.is_root ? a.root_acc + (size_t)kAccWords * tree : a.rec_acc + (size_t)kAccWords * c.slot;
	s.w0 = q.l0; s.w1 = q.l1; s.w2 = q.l2; s.w3 = count;
	return s;
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

// processPathData + scatterDataIntoSDTree's filter for dense slot g
// (path_guiding_integrator.py:434-478).  Returns keep; outputs the tree's inputs.
__device__ __forceinline__ bool process_slot(uint64_t g, uint64_t S, uint64_t num_rays, uint64_t ray, bool active,
                                             const float *__restrict__ l_final, const pg_dense_records &r,
                                             float &radiance, float &nee_lum, float &wp)
{
	radiance = 0.0f; nee_lum = 0.0f; wp = 0.0f;
	if (!active) return false; // (an unused slot, or a path that left the scene: nothing to read)
	float in[3], nee[3];
#pragma unroll
	for (int ch = 0; ch < 3; ++ch) {
		float out = (l_final[ch * num_rays + ray] - r.throughput_radiance[ch * S + g]) / r.throughput_bsdf[ch * S + g];
		if (out != out) out = 0.0f;                         // :444
		float v = out / r.bsdf[ch * S + g];
		if (v != v) v = 0.0f;                               // :449
		in[ch] = v;
		float e = r.radiance_nee[ch * S + g];
		if (e != e) e = 0.0f;                               // :467
		nee[ch] = e;
	}
	radiance = luminance(in[0], in[1], in[2]);            // :452
	if (radiance != radiance) radiance = 0.0f;            // :466
	nee_lum = luminance(nee[0], nee[1], nee[2]);
	wp = r.wo_pdf[g];
	const bool both_zero = (radiance == 0.0f) && (nee_lum == 0.0f); // :470-472
	return active && !both_zero && !(wp == 0.0f) && !(wp != wp); // :475-478
}

} // namespace pg
