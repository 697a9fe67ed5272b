// pg_lights_dev.hpp -- SELECT and PMF of include/ext/pg_lights.h as device functions, and the row of a position's KD leaf: what
// the kernels of pg_kernels_lights.hip (the sample, the pmf) and of pg_kernels_nee.hip (the resampled next-event estimation,
// include/ext/lights/pg_nee.h) share, so that the two callers agree by construction.  The text is the one pg_kernels_lights.hip
// held before the second caller came.
#pragma once

#include "pg_context.hpp"
#include "pg_descent.hpp"

namespace pg {

// what the sample and the pmf read of the state
struct LightsView {
	const uint32_t *rows; // [n_trees][L]
	uint32_t L;
	float Lf, invL, delta;
};

// ---- SELECT and PMF of the header --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lights_weight(const uint32_t *row, uint32_t j)
{
	const uint32_t c = row[j];
	return j ? c - row[j - 1u] : c;
}

// row == nullptr or K == 0: an unlearned leaf
__device__ __forceinline__ float lights_pmf(const LightsView &v, const uint32_t *row, uint32_t K, uint32_t j)
{
	if (j >= v.L) return 0.0f;
	if (K == 0u) return v.invL;
	const float share = (float)lights_weight(row, j) / (float)K;
	return (v.delta * v.invL) + ((1.0f - v.delta) * share);
}

__device__ __forceinline__ uint32_t lights_select(const LightsView &v, const uint32_t *row, uint32_t K, float u)
{
	const uint32_t last = v.L - 1u;
	if (K == 0u) {
		const uint32_t j = (uint32_t)(u * v.Lf);
		return j < last ? j : last;
	}
	if (u < v.delta) {
		const uint32_t j = (uint32_t)((u / v.delta) * v.Lf);
		return j < last ? j : last;
	}
	const float w = (u - v.delta) / (1.0f - v.delta);
	uint32_t t = (uint32_t)(w * 16777216.0f);
	if (t > 16777215u) t = 16777215u;
	const uint32_t x = (uint32_t)(((uint64_t)t * K) >> 24); // < K = row[last]
	uint32_t lo = 0u, hi = last;                             // row[hi] > x throughout
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (row[mid] > x) hi = mid;
		else lo = mid + 1u;
	}
	return lo;
}

// the row of the leaf that holds (x, y, z) and its K; nullptr and 0 outside the root box
__device__ __forceinline__ const uint32_t *lights_row(const TreeView &t, const float *s_planes, const LightsView &v, float x, float y,
                                                      float z, uint32_t &K)
{
	K = 0u;
	if (!inside_root(t, x, y, z)) return nullptr;
	KdNode leaf;
	uint32_t lv;
	kd_descend_grid(t, s_planes, x, y, z, true, leaf, lv);
	const uint32_t *row = v.rows + (size_t)leaf.tree * v.L;
	K = row[v.L - 1u];
	return row;
}

// the view of a context whose feature is on (host)
inline LightsView lights_view(const pg_context *ctx)
{
	const Lights &li = ctx->lights;
	LightsView v;
	v.rows = li.rows(ctx->f.n_trees);
	v.L = li.n_lights;
	v.Lf = (float)li.n_lights;
	v.invL = 1.0f / v.Lf;
	v.delta = li.prm.delta;
	return v;
}

} // namespace pg
