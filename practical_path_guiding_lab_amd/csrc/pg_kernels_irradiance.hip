// pg_kernels_irradiance.hip -- irradiance estimates per spatial leaf (include/pgsd_irradiance.h; not in the reference): the
// projection of every quadtree of sdTree_prev onto the nine spherical harmonics up to order 2 (the build), and the estimate and
// the roulette / splitting decision on it (one lane per query, wave64, 256-thread groups, the pattern of k_radiance).
//
// The build is a sum of exact integers (pgsd_irradiance.h): whatever order the leaves are visited in, the table is the same.  One
// launch per level of the forest: a lane per record takes its cell from the level above, hands its non-leaf children theirs, and
// projects its leaf children; the nine words of neighbouring lanes of a wave that share a tree are merged before the atomics.
// The query is bound like k_radiance with dir == NULL: the KD grid entry, then ONE round trip for the 48 bytes of the tree.
#include <cmath>
#include <vector>

#include "../../include/pgsd_irradiance.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_guide_dev.hpp"

namespace pg {

static_assert(kIrrStride * sizeof(float) == 3 * 16 && kIrrCoeffs <= kIrrStride, "a tree's coefficients leave as three 16-byte gathers");
constexpr uint32_t kIrrNoTree = 0xffffffffu; // a record no root reaches (the cells are set to it before every build)
constexpr uint32_t kIrrMaxDepth = 31;        // (ix, iy) of a cell are 32-bit: deeper than any descent of the library goes

// ---- the means of the nine polynomials over one cell: pgsd_irradiance.h, operation by operation (fp64, no contraction) ----
__device__ __forceinline__ double pow2_neg(uint32_t d) { return __longlong_as_double((long long)(1023 - (int)d) << 52); } // 2^-d

// asin z = atan2(z, s), s = sqrt(1 - z^2) >= 0
__device__ __forceinline__ double asin_zs(double z, double s)
{
	const double a = __builtin_fabs(z);
	const double hi = a > s ? a : s, lo = a > s ? s : a;
	double v = atan_unit(lo / hi);
	if (a > s) v = 1.57079632679489661923 - v;
	if (z < 0.0) v = -v;
	return v;
}

// sine and cosine of 2 pi f, f a dyadic fraction in [0, 2]: the reduction by quarter turns is exact, then the two series of
// sincos_f32 (pg_math.hpp) on |r| <= pi/4 and its selection by the quadrant, unrounded.  (The series are written out here: with
// sincos_f32 calling a shared copy, the register allocation of the renderer's kernels moved.)
__device__ __forceinline__ void turn(double f, double &s, double &c)
{
	const double k = __builtin_rint(4.0 * f);
	const double r = (f - k * 0.25) * 6.283185307179586;
	const double z = r * r;
	double ps = 1.0 / 355687428096000.0;
	ps = -1.0 / 1307674368000.0 + z * ps;
	ps = 1.0 / 6227020800.0 + z * ps;
	ps = -1.0 / 39916800.0 + z * ps;
	ps = 1.0 / 362880.0 + z * ps;
	ps = -1.0 / 5040.0 + z * ps;
	ps = 1.0 / 120.0 + z * ps;
	ps = -1.0 / 6.0 + z * ps;
	const double sr = r + r * (z * ps);
	double pc = -1.0 / 6402373705728000.0;
	pc = 1.0 / 20922789888000.0 + z * pc;
	pc = -1.0 / 87178291200.0 + z * pc;
	pc = 1.0 / 479001600.0 + z * pc;
	pc = -1.0 / 3628800.0 + z * pc;
	pc = 1.0 / 40320.0 + z * pc;
	pc = -1.0 / 720.0 + z * pc;
	pc = 1.0 / 24.0 + z * pc;
	pc = -0.5 + z * pc;
	const double cr = 1.0 + z * pc;
	const int q = (int)(long long)k & 3;
	s = (q == 0) ? sr : (q == 1) ? cr : (q == 2) ? -sr : -cr;
	c = (q == 0) ? cr : (q == 1) ? -sr : (q == 2) ? -cr : sr;
}

__device__ __forceinline__ void cell_means(uint32_t ix, uint32_t iy, uint32_t d, double m[9])
{
	const double w = pow2_neg(d);
	const double x0 = (double)ix * w, x1 = ((double)ix + 1.0) * w;
	const double y0 = (double)iy * w, y1 = ((double)iy + 1.0) * w;
	const double z0 = 2.0 * y0 - 1.0, z1 = 2.0 * y1 - 1.0;
	const double s0 = __builtin_sqrt(1.0 - z0 * z0), s1 = __builtin_sqrt(1.0 - z1 * z1);
	const double F0 = (z0 * s0 + asin_zs(z0, s0)) / 2.0, F1 = (z1 * s1 + asin_zs(z1, s1)) / 2.0;
	const double Zz = (z0 + z1) / 2.0;
	const double Zs = (F1 - F0) / (2.0 * w);
	const double Zzs = (0.0 - ((s1 * s1) * s1 - (s0 * s0) * s0)) / (6.0 * w);
	const double Zss = ((z1 - ((z1 * z1) * z1) / 3.0) - (z0 - ((z0 * z0) * z0) / 3.0)) / (2.0 * w);
	const double Z20 = ((z1 * z1 + z1 * z0) + z0 * z0) - 1.0;
	double sa0, ca0, sa1, ca1, sb0, cb0, sb1, cb1;
	turn(x0, sa0, ca0);
	turn(x1, sa1, ca1);
	turn(2.0 * x0, sb0, cb0);
	turn(2.0 * x1, sb1, cb1);
	const double C1 = (sa1 - sa0) / (6.283185307179586 * w), S1 = (ca0 - ca1) / (6.283185307179586 * w);
	const double C2 = (sb1 - sb0) / (12.566370614359172 * w), S2 = (cb0 - cb1) / (12.566370614359172 * w);
	m[0] = 1.0;
	m[1] = Zs * S1;
	m[2] = Zz;
	m[3] = Zs * C1;
	m[4] = (Zss * S2) / 2.0;
	m[5] = Zzs * S1;
	m[6] = Z20;
	m[7] = Zzs * C1;
	m[8] = Zss * C2;
}

// a leaf's share of the nine sums: q_j = rint(clamp((e / R) m_j) 2^50), added modulo 2^64
__device__ __forceinline__ void add_leaf(long long acc[9], float e, float R, uint32_t ix, uint32_t iy, uint32_t d)
{
	double m[9];
	cell_means(ix, iy, d, m);
	const double ratio = (double)e / (double)R;
#pragma unroll
	for (int j = 0; j < 9; ++j) {
		double t = ratio * m[j];
		if (!(t == t)) t = 0.0;
		t = t > 1024.0 ? 1024.0 : (t < -1024.0 ? -1024.0 : t);
		const long long q = (long long)__builtin_rint(t * 0x1.0p50); // |.| <= 2^60
		acc[j] = (long long)((unsigned long long)acc[j] + (unsigned long long)q);
	}
}

__device__ __forceinline__ bool irr_root_usable(float R) { return R > 0.0f && finite_f32(R); }

__device__ __forceinline__ void store16(void *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
	u32x4_t v;
	v.x = a; v.y = b; v.z = c; v.w = d;
	*reinterpret_cast<u32x4_t *>(p) = v;
}

// ---- the build -------------------------------------------------------------------------------------------------------------
// per tree: its sums start at zero; the root record of a tree that has one gets the whole square
__global__ __launch_bounds__(kQueryBlock) void k_irr_roots(const TreeHead *__restrict__ head, uint32_t n_trees, uint32_t n_rec,
                                                         long long *__restrict__ sums, uint4 *__restrict__ cells)
{
	const uint32_t t = blockIdx.x * kQueryBlock + threadIdx.x;
	if (t >= n_trees) return;
#pragma unroll
	for (uint32_t j = 0; j < kIrrCoeffs; ++j) sums[(size_t)t * kIrrCoeffs + j] = 0;
	const TreeHead h = load_head(head, t);
	if (h.root_rec != kNoRecord && h.root_rec < n_rec) store16(cells + h.root_rec, t, 0u, 0u, 0u);
}

// per record of one level [begin, end): children that have records get their cells (they lie in later levels: a child index
// that does not is not followed), leaf children are projected
__global__ __launch_bounds__(kQueryBlock) void k_irr_level(const QuadRec *__restrict__ rec, const TreeHead *__restrict__ head,
                                                         uint32_t n_trees, uint32_t n_rec, uint32_t begin, uint32_t end,
                                                         uint4 *__restrict__ cells, long long *__restrict__ sums)
{
	const uint32_t r = begin + blockIdx.x * kQueryBlock + threadIdx.x; // (begin + grid < 2^32 + 256: the host keeps n_rec below 2^32 - 16)
	uint32_t tree = kIrrNoTree;
	long long acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	if (r >= begin && r < end) {
		const uint4 c = gather16(cells + r);
		if (c.x < n_trees && c.w < kIrrMaxDepth) {
			tree = c.x;
			const uint32_t d = c.w + 1u;
			const QuadLoad q = load_rec(rec, r);
			const float R = load_head(head, tree).root_irr;
			const bool usable = irr_root_usable(R);
#pragma unroll 1
			for (int k = 0; k < 4; ++k) {
				const uint32_t ch = sel4u(k, q.c0, q.c1, q.c2, q.c3);
				const uint32_t ix = 2u * c.y + ((k == 0 || k == 3) ? 1u : 0u);
				const uint32_t iy = 2u * c.z + ((k == 0 || k == 1) ? 1u : 0u);
				if (ch != 0u) {
					if (ch >= end && ch < n_rec) store16(cells + ch, tree, ix, iy, d);
				} else if (usable) {
					add_leaf(acc, sel4f(k, q.i0, q.i1, q.i2, q.i3), R, ix, iy, d);
				}
			}
		}
	}
	// the lanes of a wave that stand side by side on one tree add once: a segmented sum towards the first lane of every run
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t prev = (uint32_t)__shfl_up((int)tree, 1);
	const bool first = lane == 0u || prev != tree;
	const unsigned long long firsts = __ballot(first);
	const unsigned long long above = lane == 63u ? 0ull : (firsts >> (lane + 1u));
	const uint32_t seg_end = above ? lane + 1u + (uint32_t)__builtin_ctzll(above) : 64u; // (exclusive)
#pragma unroll
	for (uint32_t off = 1; off < 64u; off <<= 1) {
#pragma unroll
		for (int j = 0; j < 9; ++j) {
			const long long o = __shfl_down(acc[j], off);
			if (lane + off < seg_end) acc[j] = (long long)((unsigned long long)acc[j] + (unsigned long long)o);
		}
	}
	if (first && tree != kIrrNoTree) {
		unsigned long long *dst = reinterpret_cast<unsigned long long *>(sums) + (size_t)tree * kIrrCoeffs;
#pragma unroll
		for (int j = 0; j < 9; ++j)
			if (acc[j] != 0) atomicAdd(dst + j, (unsigned long long)acc[j]);
	}
}

// per tree: a root that is the leaf is its own one cell; then the conversion
__global__ __launch_bounds__(kQueryBlock) void k_irr_finish(const TreeHead *__restrict__ head, const unsigned long long *__restrict__ wtab,
                                                          uint32_t n_trees, const long long *__restrict__ sums, float *__restrict__ tab)
{
	const uint32_t t = blockIdx.x * kQueryBlock + threadIdx.x;
	if (t >= n_trees) return;
	const TreeHead h = load_head(head, t);
	const uint2 wv = gather8(wtab + t);
	const unsigned long long N = ((unsigned long long)wv.y << 32) | wv.x;
	const float R = h.root_irr;
	float k[kIrrStride];
#pragma unroll
	for (uint32_t j = 0; j < kIrrStride; ++j) k[j] = 0.0f;
	if (N != 0ull && irr_root_usable(R)) {
		long long s[9];
		if (h.root_rec == kNoRecord) {
#pragma unroll
			for (int j = 0; j < 9; ++j) s[j] = 0;
			add_leaf(s, R, R, 0u, 0u, 0u);
		} else {
#pragma unroll
			for (int j = 0; j < 9; ++j) s[j] = sums[(size_t)t * kIrrCoeffs + j];
		}
		const double g[9] = {0.25, 0.5, 0.5, 0.5, 0.9375, 0.9375, 0.078125, 0.9375, 0.234375};
		const double ratio = (double)R / (double)N;
#pragma unroll
		for (int j = 0; j < 9; ++j) k[j] = (float)((((double)s[j] * 0x1.0p-50) * g[j]) * ratio);
	}
	float *dst = tab + (size_t)t * kIrrStride;
#pragma unroll
	for (int v = 0; v < 3; ++v)
		store16(dst + 4 * v, __float_as_uint(k[4 * v]), __float_as_uint(k[4 * v + 1]), __float_as_uint(k[4 * v + 2]),
		        __float_as_uint(k[4 * v + 3]));
}

// ---- the estimate and the decision -------------------------------------------------------------------------------------------
// normal == nullptr (uniform): the mean over all orientations, k0.
template <bool kDecide>
__global__ __launch_bounds__(kQueryBlock) void k_irradiance(TreeView t, const float *__restrict__ tab, uint64_t n,
                                                          const float *__restrict__ p, const float *__restrict__ normal,
                                                          const uint8_t *__restrict__ active, float *__restrict__ E_out, RrArgs rr)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = active ? active[i] != 0 : true;
	float E = 0.0f;
	uint32_t count = 1u;
	float scale = 1.0f;
	if (act) {
		// (everything that does not depend on the tree first: the loads leave before the descent's gathers)
		Pcg32 rng = {0ull, 0ull};
		float w = 0.0f, I = 0.0f;
		if (kDecide) {
			rng.state = rr.rng_state[i];
			rng.inc = rr.rng_inc[i];
			w = rr.weight[i];
			I = rr.reference[i];
		}
		const float x = p[i], y = p[n + i], z = p[2 * n + i];
		float nx = 0.0f, ny = 0.0f, nz = 0.0f;
		if (normal) { nx = normal[i]; ny = normal[n + i]; nz = normal[2 * n + i]; }
		KdNode leaf;
		uint32_t kd_lv;
		kd_descend_grid(t, s_planes, x, y, z, inside_root(t, x, y, z), leaf, kd_lv);
		// one round trip: three unconditional 16-byte gathers that need the leaf's tree number only
		const float *row = tab + (size_t)leaf.tree * kIrrStride;
		const uint4 a = gather16(row), b = gather16(row + 4), c = gather16(row + 8);
		const float k0 = __uint_as_float(a.x), k1 = __uint_as_float(a.y), k2 = __uint_as_float(a.z), k3 = __uint_as_float(a.w);
		const float k4 = __uint_as_float(b.x), k5 = __uint_as_float(b.y), k6 = __uint_as_float(b.z), k7 = __uint_as_float(b.w);
		const float k8 = __uint_as_float(c.x);
		float S = k0;
		if (normal) {
			S = S + k1 * ny;
			S = S + k2 * nz;
			S = S + k3 * nx;
			S = S + (k4 * nx) * ny;
			S = S + (k5 * ny) * nz;
			S = S + k6 * ((3.0f * nz) * nz - 1.0f);
			S = S + (k7 * nx) * nz;
			S = S + k8 * (nx * nx - ny * ny);
		}
		E = S > 0.0f ? S : 0.0f; // (NaN -> 0)
		if (!(finite_f32(nx) && finite_f32(ny) && finite_f32(nz))) E = 0.0f;
		if (kDecide) {
			const float xi = rng.next_f32(); // exactly one draw per active lane
			rr.rng_state[i] = rng.state;
			rr_decide(rr, xi, E, w, I, count, scale);
		}
	}
	if (E_out) E_out[i] = E;
	if (kDecide) {
		rr.count_out[i] = count;
		rr.scale_out[i] = scale;
	}
}

} // namespace pg

using namespace pg;

#define PG_IRRADIANCE_BUILT(ctx, who)                                                                                         \
	do {                                                                                                                      \
		PG_READY(ctx);                                                                                                        \
		if (!(ctx)->rad.irr.built)                                                                                            \
			return fail((ctx), PG_ERR_INVALID, who ": call pg_irradiance_build first (no build or pg_irradiance_import since sdTree_prev or its weights changed)"); \
	} while (0)

extern "C" {

int pg_irradiance_build(pg_context *ctx, void *stream)
{
	PG_READY(ctx);
	if (int rc = radiance_source(ctx, "pg_irradiance_build")) return rc; // (the table is projected with the statistical weights)
	Forest &f = ctx->f;
	Irradiance &ir = ctx->rad.irr;
	hipStream_t s = (hipStream_t)stream;
	const size_t levels = f.level_off.empty() ? 0 : f.level_off.size() - 1;
	if ((f.n_rec != 0 || levels != 0) && (levels == 0 || f.level_off[0] != 0 || f.level_off[levels] != f.n_rec))
		return fail(ctx, PG_ERR_INVALID, "pg_irradiance_build: the forest's level ranges do not cover its records (internal error)");
	ir.built = 0; // (a buffer that has to grow loses its contents)
	PG_HIP(ctx, ir.tab.ensure((size_t)f.n_trees * kIrrStride, 1.25));
	PG_HIP(ctx, ir.sums.ensure((size_t)f.n_trees * kIrrCoeffs, 1.25));
	PG_HIP(ctx, ir.cells.ensure(f.n_rec, 1.25));
	if (f.n_rec) PG_HIP(ctx, hipMemsetAsync(ir.cells.p, 0xff, (size_t)f.n_rec * sizeof(uint4), s));
	hipLaunchKernelGGL(k_irr_roots, query_grid(f.n_trees), dim3(kQueryBlock), 0, s, f.head.p, f.n_trees, f.n_rec, ir.sums.p, ir.cells.p);
	for (size_t l = 0; l < levels; ++l) {
		const uint32_t begin = f.level_off[l], end = f.level_off[l + 1];
		if (end <= begin) continue;
		hipLaunchKernelGGL(k_irr_level, query_grid(end - begin), dim3(kQueryBlock), 0, s, f.rec.p, f.head.p, f.n_trees, f.n_rec, begin, end,
		                   ir.cells.p, ir.sums.p);
	}
	hipLaunchKernelGGL(k_irr_finish, query_grid(f.n_trees), dim3(kQueryBlock), 0, s, f.head.p, ctx->rad.tab.p, f.n_trees, ir.sums.p, ir.tab.p);
	PG_LAUNCHED(ctx);
	ir.built = 1;
	return PG_OK;
}

int pg_irradiance_status(pg_context *ctx, int32_t *built)
{
	PG_READY(ctx);
	if (built) *built = ctx->rad.irr.built;
	return PG_OK;
}

int pg_irradiance_export(pg_context *ctx, uint64_t n_trees, float *h_coeff)
{
	PG_IRRADIANCE_BUILT(ctx, "pg_irradiance_export");
	if (n_trees != ctx->f.n_trees) return fail(ctx, PG_ERR_INVALID, "pg_irradiance_export: n_trees does not match pg_export_sizes' n_roots");
	if (!h_coeff) return fail(ctx, PG_ERR_INVALID, "pg_irradiance_export: NULL pointer");
	PG_HIP(ctx, hipDeviceSynchronize());
	std::vector<float> h((size_t)n_trees * kIrrStride);
	PG_HIP(ctx, hipMemcpy(h.data(), ctx->rad.irr.tab.p, h.size() * sizeof(float), hipMemcpyDeviceToHost));
	for (size_t t = 0; t < n_trees; ++t)
		for (uint32_t j = 0; j < kIrrCoeffs; ++j) h_coeff[t * kIrrCoeffs + j] = h[t * kIrrStride + j];
	return PG_OK;
}

int pg_irradiance_import(pg_context *ctx, uint64_t n_trees, const float *h_coeff)
{
	PG_READY(ctx);
	if (int rc = radiance_source(ctx, "pg_irradiance_import")) return rc; // (the table is projected with the statistical weights)
	if (n_trees != ctx->f.n_trees) return fail(ctx, PG_ERR_INVALID, "pg_irradiance_import: n_trees does not match pg_export_sizes' n_roots");
	if (!h_coeff) return fail(ctx, PG_ERR_INVALID, "pg_irradiance_import: NULL pointer");
	PG_HIP(ctx, hipDeviceSynchronize());
	Irradiance &ir = ctx->rad.irr;
	std::vector<float> h((size_t)n_trees * kIrrStride, 0.0f);
	for (size_t t = 0; t < n_trees; ++t)
		for (uint32_t j = 0; j < kIrrCoeffs; ++j) h[t * kIrrStride + j] = h_coeff[t * kIrrCoeffs + j];
	ir.built = 0;
	PG_HIP(ctx, upload(ir.tab, h, 1.25));
	ir.built = 1;
	return PG_OK;
}

int pg_irradiance_query(pg_context *ctx, uint64_t n, const float *p, const float *normal, const uint8_t *active, float *E_out,
                        void *stream)
{
	PG_IRRADIANCE_BUILT(ctx, "pg_irradiance_query");
	if (n && (!p || !E_out)) return fail(ctx, PG_ERR_INVALID, "pg_irradiance_query: NULL pointer");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_irradiance_query: too many lanes for one launch");
	if (n == 0) return PG_OK;
	RrArgs rr = {};
	hipLaunchKernelGGL(k_irradiance<false>, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), ctx->rad.irr.tab.p, n, p,
	                   normal, active, E_out, rr);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_irradiance_rr(pg_context *ctx, uint64_t n, const float *p, const float *normal, const float *weight, const float *reference,
                     const pg_rr_params *params, uint64_t *rng_state, const uint64_t *rng_inc, const uint8_t *active,
                     uint32_t *count_out, float *scale_out, float *E_out, void *stream)
{
	PG_IRRADIANCE_BUILT(ctx, "pg_irradiance_rr");
	RrArgs rr;
	if (int rc = rr_window(ctx, "pg_irradiance_rr", params, rr)) return rc;
	if (n && (!p || !weight || !reference || !rng_state || !rng_inc || !count_out || !scale_out))
		return fail(ctx, PG_ERR_INVALID, "pg_irradiance_rr: NULL pointer");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_irradiance_rr: too many lanes for one launch");
	if (n == 0) return PG_OK;
	rr.weight = weight; rr.reference = reference;
	rr.rng_state = rng_state; rr.rng_inc = rng_inc;
	rr.count_out = count_out; rr.scale_out = scale_out;
	hipLaunchKernelGGL(k_irradiance<true>, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), ctx->rad.irr.tab.p, n, p,
	                   normal, active, E_out, rr);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

} // extern "C"
