// pg_kernels_splat.hip -- recording into sdTree_current.
//
// The reference adds fp32 values with one float atomic per node on the root->leaf path
// (kdtree.py:199, quadtree.py:93): D_kd + 2*D_quad atomics per record, all records hitting the
// same root words.  Here a record touches only the accumulators of the two quadtree leaves its
// directions fall into: integer sums are order independent, so inner-node totals (and the KD
// counts, carried in word 3 of the path direction's accumulator) are formed once at refine time
// by a bottom-up pass, and the multi-GPU exchange is an exact int64 all-reduce.
//
// Scattered global atomics are the bound of this kernel (about 24 G sector-updates/s on MI355X,
// tools/atomic_probe.hip), and the hardware charges one update per 32-byte sector touched by a
// wave-instruction, not per lane.  A record's four words therefore go out from four ADJACENT lanes
// of one instruction (transposed through LDS): one update per direction instead of up to four.
#include "pg_descent.hpp"
#include "pg_kernels.hpp"
#include "pg_splat_dev.hpp"

namespace pg {

// KDTree.addDataPropagate (kdtree.py:180-225) + QuadTree.addDataPropagate (quadtree.py:389-464):
// finds where the record's two contributions go; the adds themselves are issued by coop_add
__device__ __forceinline__ void plan_record(const TreeView &t, const AccumView &a, const float *s_planes, int store_nee,
                                            float x, float y, float z, float dx, float dy, float radiance,
                                            float wo_pdf, float nx, float ny, float nee_lum, SlotAdd &path,
                                            SlotAdd &nee, unsigned &kd_lv, unsigned &q_lv, unsigned &q_q, unsigned &bytes)
{
	const bool inside = inside_root(t, x, y, z);
	KdNode leaf;
	uint32_t lv;
	kd_descend_grid(t, s_planes, x, y, z, inside, leaf, lv);
	kd_lv += stat_levels(lv); // (statistics words, pg_descent.hpp: a thread may plan many records, so they are unpacked here)
	bytes += stat_bytes(lv);
	const uint32_t tree = leaf.tree; // outside the bbox: node 0's (stale) tree (kdtree.py:224)
	const float w = wo_pdf > 0.0f ? radiance / wo_pdf : 0.0f;   // quadtree.py:451
	const float wn = wo_pdf > 0.0f ? nee_lum / wo_pdf : 0.0f;   // quadtree.py:462
	TreeHead head;
	LeafCursor cp, cn;
	find_record_leaves(t, a, store_nee, tree, inside, dx, dy, nx, ny, head, cp, cn);
	path = plan_dir(a, tree, cp, w, inside ? 1 : 0);
	q_lv += stat_levels(cp.levels);
	bytes += stat_bytes(cp.levels);
	++q_q;
	nee = plan_dir(a, tree, cn, wn, 0);
	if (store_nee) {
		q_lv += stat_levels(cn.levels);
		bytes += stat_bytes(cn.levels);
		++q_q;
	}
}

__device__ __forceinline__ void count_depths_s(DepthCounters *dc, unsigned kd_lv, unsigned kd_q,
                                               unsigned q_lv, unsigned q_q, unsigned bytes)
{
	if (dc == nullptr) return;
	const unsigned long long a = wave_sum_s(kd_lv), b = wave_sum_s(kd_q), c = wave_sum_s(q_lv), d = wave_sum_s(q_q);
	const unsigned long long e = wave_sum_s(bytes);
	if ((threadIdx.x & 63) == 0) {
		atomicAdd(&dc->kd_levels, a);
		atomicAdd(&dc->kd_queries, b);
		atomicAdd(&dc->quad_levels, c);
		atomicAdd(&dc->quad_queries, d);
		atomicAdd(&dc->layout_bytes, e);
	}
}

__global__ __launch_bounds__(kBlock) void k_splat(TreeView t, AccumView a, int store_nee, uint64_t m,
                                                  const float *__restrict__ pos, const float *__restrict__ dir,
                                                  const float *__restrict__ radiance,
                                                  const float *__restrict__ wo_pdf,
                                                  const float *__restrict__ dir_nee,
                                                  const float *__restrict__ nee_lum,
                                                  const uint32_t *__restrict__ d_count, DepthCounters *dc)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	__shared__ long long s_val[kBlock * 4];
	__shared__ unsigned long long s_ptr[kBlock];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
	const uint64_t valid = d_count ? (uint64_t)*d_count : m; // plane stride stays m
	unsigned kd_lv = 0, q_lv = 0, q_q = 0, did = 0, st_bytes = 0;
	SlotAdd path = {nullptr, 0, 0, 0, 0}, nee = {nullptr, 0, 0, 0, 0};
	if (i < valid && i < m) {
		const float nx = store_nee ? dir_nee[i] : 0.0f, ny = store_nee ? dir_nee[m + i] : 0.0f;
		const float nl = store_nee ? nee_lum[i] : 0.0f;
		plan_record(t, a, s_planes, store_nee, pos[i], pos[m + i], pos[2 * m + i], dir[i], dir[m + i], radiance[i],
		            wo_pdf[i], nx, ny, nl, path, nee, kd_lv, q_lv, q_q, st_bytes);
		did = 1;
	}
	coop_add(path, s_val, s_ptr);
	if (store_nee) coop_add(nee, s_val, s_ptr);
	count_depths_s(dc, kd_lv, did, q_lv, q_q, st_bytes);
}

// Stream compaction: thread-local keep flag -> workgroup prefix -> ONE atomic per workgroup
// (a single counter word serialises at ~11 ns per atomic: one per wave would dominate the kernel).
__global__ __launch_bounds__(kBlock) void k_process_records(uint64_t num_rays, int32_t max_depth,
                                                            const float *__restrict__ l_final,
                                                            pg_dense_records r, pg_records_out o,
                                                            uint32_t *__restrict__ d_count)
{
	__shared__ uint32_t s_wave[kBlock / 64];
	__shared__ uint32_t s_base;
	const uint64_t S = num_rays * (uint64_t)max_depth;
	const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
	float radiance = 0.0f, nee_lum = 0.0f, wp = 0.0f;
	// slot = ray*max_depth + depth, as the reference lays the buffer out (:318)
	const bool keep = g < S && process_slot(g, S, num_rays, g / (uint64_t)max_depth, r.active[g] != 0, l_final, r,
	                                        radiance, nee_lum, wp);
	const unsigned long long mask = __ballot(keep);
	const unsigned lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	if (lane == 0) s_wave[wid] = (uint32_t)__popcll(mask);
	__syncthreads();
	uint32_t off = 0, tot = 0;
#pragma unroll
	for (unsigned w = 0; w < kBlock / 64; ++w) {
		if (w < wid) off += s_wave[w];
		tot += s_wave[w];
	}
	if (threadIdx.x == 0) s_base = tot ? atomicAdd(d_count, tot) : 0;
	__syncthreads();
	if (keep) {
		const uint64_t k = (uint64_t)s_base + off +
		                   __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
		store_kept_record(o, k, S, r.position, r.direction, r.direction_nee, g, radiance, wp, nee_lum);
	}
}

// pg_render_export_records: the kept entries of a geometry-recording pass's list as k_process_records would have compacted
// them out of the dense buffer (any order), with their dense slots.  The list is long and strided over: one atomic on the
// counter per wave.
__global__ __launch_bounds__(kBlock) void k_export_list_records(uint64_t num_rays, int32_t max_depth, const uint4 *__restrict__ l_final_q,
                                                                pg_list_records r, pg_list_geometry geo,
                                                                const uint32_t *__restrict__ live_count, pg_records_out o,
                                                                uint32_t *__restrict__ slot_out, uint32_t *__restrict__ d_count)
{
	const uint64_t S = num_rays * (uint64_t)max_depth;
	const uint64_t total = list_entries(num_rays, max_depth, live_count);
	for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < total; base += (uint64_t)gridDim.x * kBlock) {
		const uint64_t g = base + threadIdx.x;
		float radiance = 0.0f, nee_lum = 0.0f, wp = 0.0f;
		uint32_t ray = 0;
		const bool keep = g < total && process_list_entry(g, S, num_rays, nullptr, l_final_q, r, ray, radiance, nee_lum, wp);
		const unsigned long long mask = __ballot(keep);
		if (mask == 0ull) continue;
		const unsigned lane = threadIdx.x & 63u, first = (unsigned)__builtin_ctzll(mask);
		uint32_t off = 0;
		if (lane == first) off = atomicAdd(d_count, (uint32_t)__popcll(mask));
		off = __shfl(off, (int)first, 64);
		if (keep) {
			// (k < S: the list has at most S entries, and every kept one is counted once)
			const uint64_t k = (uint64_t)off + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
			store_kept_record(o, k, S, geo.position, geo.direction, geo.direction_nee, g, radiance, wp, nee_lum);
			if (slot_out) slot_out[k] = (uint32_t)((uint64_t)ray * (uint64_t)max_depth + geo.depth[g]);
		}
	}
}

// The reference's dense record buffer behind pg_process_and_splat: slot = ray*max_depth + depth (:318), every slot
// visited.  (The library's own renderer does not come here: its list names the accumulators, k_splat_list below.)
// A strided grid: the jump grid's planes are staged once per workgroup instead of once per tile, and the first
// iteration's single accumulator gets four atomics per workgroup (SingleLeafSum).
__global__ __launch_bounds__(kBlock) void k_process_and_splat(TreeView t, AccumView a, int store_nee,
                                                              uint64_t num_rays, int32_t max_depth,
                                                              const float *__restrict__ l_final,
                                                              pg_dense_records r, DepthCounters *dc)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	__shared__ long long s_val[kBlock * 4];
	__shared__ unsigned long long s_ptr[kBlock];
	const uint64_t S = num_rays * (uint64_t)max_depth;
	const uint64_t total = S;
	stage_kd_planes(s_planes, t);
	const bool single = SingleLeafSum::applies(t);
	SingleLeafSum sum;
	unsigned kd_lv = 0, q_lv = 0, q_q = 0, did = 0, st_bytes = 0;
	for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < total; base += (uint64_t)gridDim.x * kBlock) {
		const uint64_t g = base + threadIdx.x;
		float radiance = 0.0f, nee_lum = 0.0f, wp = 0.0f;
		SlotAdd path = {nullptr, 0, 0, 0, 0}, nee = {nullptr, 0, 0, 0, 0};
		bool keep = false;
		if (g < total) keep = process_slot(g, S, num_rays, g / (uint64_t)max_depth, r.active[g] != 0, l_final, r, radiance, nee_lum, wp);
		if (keep) {
			plan_record(t, a, s_planes, store_nee, r.position[g], r.position[S + g], r.position[2 * S + g], r.direction[g],
			            r.direction[S + g], radiance, wp, r.direction_nee[g], r.direction_nee[S + g], nee_lum, path, nee,
			            kd_lv, q_lv, q_q, st_bytes);
			++did;
		}
		if (single) {
			sum.add(path, nee);
		} else {
			coop_add(path, s_val, s_ptr);
			if (store_nee) coop_add(nee, s_val, s_ptr);
		}
	}
	if (single) sum.flush(a, s_val);
	count_depths_s(dc, kd_lv, did, q_lv, q_q, st_bytes);
}

// The split render pipeline's list (pg_list_records): processPathData + the filter of scatterDataIntoSDTree
// (process_list_entry) + the adds of KDTree / QuadTree.addDataPropagate (kdtree.py:180-225, quadtree.py:389-464) at
// accumulators the entry names -- no tree is walked here: the bounce that made the vertex walked sdTree_prev to these
// very leaves for its pdfs (stage_guide).  What is left is one gather (the path's final radiance), the division chain,
// and the atomics.
__global__ __launch_bounds__(kBlock) void k_splat_list(TreeView t, AccumView a, int store_nee, uint64_t num_rays,
                                                       int32_t max_depth, const float *__restrict__ l_final,
                                                       const uint4 *__restrict__ l_final_q, pg_list_records r,
                                                       const uint32_t *__restrict__ live_count)
{
	__shared__ long long s_val[kBlock * 4];
	__shared__ unsigned long long s_ptr[kBlock];
	const uint64_t S = num_rays * (uint64_t)max_depth;
	const uint64_t total = list_entries(num_rays, max_depth, live_count);
	if ((uint64_t)blockIdx.x * kBlock >= total) return;
	const bool single = SingleLeafSum::applies(t);
	SingleLeafSum sum;
	for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < total; base += (uint64_t)gridDim.x * kBlock) {
		const uint64_t g = base + threadIdx.x;
		SlotAdd path = {nullptr, 0, 0, 0, 0}, nee = {nullptr, 0, 0, 0, 0};
		float radiance = 0.0f, nee_lum = 0.0f, wp = 0.0f;
		uint32_t ray = 0;
		if (g < total && process_list_entry(g, S, num_rays, l_final, l_final_q, r, ray, radiance, nee_lum, wp)) {
			const uint2 sl = r.slot[g];
			const uint32_t tf = __builtin_nontemporal_load(r.tree + g), tree = tf & 0x7fffffffu;
			const bool inside = (tf >> 31) != 0u;
			const float w = wp > 0.0f ? radiance / wp : 0.0f;  // quadtree.py:451
			const float wn = wp > 0.0f ? nee_lum / wp : 0.0f;  // quadtree.py:462
			if (sl.x != kSlotNone) path = slot_add(a, sl.x == kSlotRoot, tree, sl.x, w, inside ? 1 : 0);
			else if (inside) atomicAdd(a.leaf_count + tree, 1ull); // counted, but its direction reaches no leaf
			if (store_nee && sl.y != kSlotNone) nee = slot_add(a, sl.y == kSlotRoot, tree, sl.y, wn, 0);
		}
		if (single) {
			sum.add(path, nee);
		} else {
			coop_add(path, s_val, s_ptr);
			if (store_nee) coop_add(nee, s_val, s_ptr);
		}
	}
	if (single) sum.flush(a, s_val);
}

void launch_splat(const TreeView &t, const AccumView &a, int store_nee, uint64_t m, const pg_records &rec,
                  const uint32_t *d_count, DepthCounters *dc, hipStream_t s)
{
	if (m == 0) return;
	hipLaunchKernelGGL(k_splat, grid_for(m), dim3(kBlock), 0, s, t, a, store_nee, m, rec.position,
	                   rec.direction, rec.radiance, rec.wo_pdf, rec.direction_nee, rec.radiance_nee_lum,
	                   d_count, dc);
}

void launch_process_records(uint64_t num_rays, int32_t max_depth, const float *l_final,
                            const pg_dense_records &rec, const pg_records_out &out, uint32_t *d_count,
                            hipStream_t s)
{
	const uint64_t S = num_rays * (uint64_t)max_depth;
	(void)hipMemsetAsync(d_count, 0, sizeof(uint32_t), s);
	if (S == 0) return;
	hipLaunchKernelGGL(k_process_records, grid_for(S), dim3(kBlock), 0, s, num_rays, max_depth, l_final, rec,
	                   out, d_count);
}

void launch_export_list_records(uint64_t num_rays, int32_t max_depth, const uint4 *l_final_q, const pg_list_records &rec,
                                const pg_list_geometry &geo, const uint32_t *live_count, const pg_records_out &out, uint32_t *slot_out,
                                uint32_t *d_count, int n_cus, hipStream_t s)
{
	const uint64_t S = num_rays * (uint64_t)max_depth;
	(void)hipMemsetAsync(d_count, 0, sizeof(uint32_t), s);
	if (S == 0) return;
	hipLaunchKernelGGL(k_export_list_records, strided_grid(S, n_cus), dim3(kBlock), 0, s, num_rays, max_depth, l_final_q, rec, geo,
	                   live_count, out, slot_out, d_count);
}

void launch_splat_list(const TreeView &t, const AccumView &a, int store_nee, uint64_t num_rays, int32_t max_depth,
                       const float *l_final, const uint4 *l_final_q, const pg_list_records &rec, const uint32_t *live_count,
                       int n_cus, hipStream_t s)
{
	const uint64_t S = num_rays * (uint64_t)max_depth;
	if (S == 0) return;
	hipLaunchKernelGGL(k_splat_list, strided_grid(S, n_cus), dim3(kBlock), 0, s, t, a, store_nee, num_rays, max_depth, l_final,
	                   l_final_q, rec, live_count);
}

void launch_process_and_splat(const TreeView &t, const AccumView &a, int store_nee, uint64_t num_rays,
                              int32_t max_depth, const float *l_final, const pg_dense_records &rec,
                              DepthCounters *dc, int n_cus, hipStream_t s)
{
	const uint64_t S = num_rays * (uint64_t)max_depth;
	if (S == 0) return;
	hipLaunchKernelGGL(k_process_and_splat, strided_grid(S, n_cus), dim3(kBlock), 0, s, t, a, store_nee, num_rays, max_depth,
	                   l_final, rec, dc);
}

} // namespace pg
