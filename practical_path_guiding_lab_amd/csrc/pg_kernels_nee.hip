// pg_kernels_nee.hip -- resampled next-event estimation (include/ext/lights/pg_nee.h, which states the semantics operation by
// operation): a light and a point on it per path vertex, by resampled importance sampling of M candidates drawn
// from the learned row of the vertex's KD leaf.  One lane per vertex, wave64, 256-thread groups.
//
// k_nee_resample follows k_lights_sample for the descent -- the staged KD planes, one descent, one row pointer, K read once --
// and pg_ris_dev.hpp for the resampling step (the weight, the reservoir's rule, W, and the stores that fit: the point goes
// where the direction calls have a direction, and the kept light stays here): the reservoir lives in registers and there is no
// per-candidate array, so nothing can spill.  Per candidate: SELECT and PMF of pg_lights_dev.hpp as they are (the binary search
// of the row is a chain of up to twelve dependent loads at L = 4096), then ONE gather of the light's 64-byte record as four
// 16-byte loads of one line.  Bound by the latency of those dependent loads; occupancy hides it (tests/test_nee_resources.py).
#include "../../include/ext/lights/pg_nee.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_lights_dev.hpp"
#include "pg_ris_dev.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace pg {

static_assert(PG_NEE_TABLE_WORDS == 12, "o, a, b, radiance, kind, two_sided");

// the host's twelve words of a light -> its record (the header's prepare step, one fp32 operation per operation it writes)
__global__ __launch_bounds__(kQueryBlock) void k_nee_prepare(const float *__restrict__ raw, NeeLight *__restrict__ tab, uint32_t n_lights)
{
	const uint32_t j = blockIdx.x * kQueryBlock + threadIdx.x;
	if (j >= n_lights) return;
	const float *h = raw + (size_t)PG_NEE_TABLE_WORDS * j;
	const float ax = h[3], ay = h[4], az = h[5], bx = h[6], by = h[7], bz = h[8];
	const uint32_t kind = __float_as_uint(h[10]), two_sided = __float_as_uint(h[11]);
	const float cx = ay * bz - az * by;
	const float cy = az * bx - ax * bz;
	const float cz = ax * by - ay * bx;
	const float len2 = (cx * cx + cy * cy) + cz * cz;
	const float len = __builtin_sqrtf(len2);
	const float area = kind ? 0.5f * len : len;
	NeeLight r;
	r.o[0] = h[0]; r.o[1] = h[1]; r.o[2] = h[2];
	r.a[0] = ax; r.a[1] = ay; r.a[2] = az;
	r.b[0] = bx; r.b[1] = by; r.b[2] = bz;
	r.N[0] = cx / len; r.N[1] = cy / len; r.N[2] = cz / len;
	r.invA = (len > 0.0f && finite_f32(len)) ? 1.0f / area : 0.0f;
	r.radiance = h[9];
	r.kind = kind;
	r.two_sided = two_sided;
	tab[j] = r;
}

// kCand: one of the cand_* outputs is given.
template <bool kCand>
__global__ __launch_bounds__(kQueryBlock) void k_nee_resample(TreeView t, LightsView v, const NeeLight *__restrict__ tab, uint64_t n,
                                                           pg_nee_args a, uint32_t M, float Mf)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = a.active ? a.active[i] != 0 : true;
	const float nx = a.normal[i], ny = a.normal[n + i], nz = a.normal[2 * n + i];
	// the reservoir: the kept light and point, its target and source, its index; as they stand: nothing kept
	uint32_t kj = PG_LIGHTS_NONE, kk = PG_RESAMPLE_NONE;
	float kyx = 0.0f, kyy = 0.0f, kyz = 0.0f, kwx = 0.0f, kwy = 0.0f, kwz = 0.0f, kdist = 0.0f, kt = 0.0f, ks = 0.0f, W = 0.0f;
	if (act && finite_f32(nx) && finite_f32(ny) && finite_f32(nz)) {
		const float px = a.p[i], py = a.p[n + i], pz = a.p[2 * n + i];
		uint32_t K;
		const uint32_t *row = lights_row(t, s_planes, v, px, py, pz, K);
		Pcg32 rng = {a.rng_state[i], a.rng_inc[i]};
		float wsum = 0.0f;
		for (uint32_t k = 0; k < M; ++k) {
			const float u = rng.next_f32();
			const uint32_t j = lights_select(v, row, K, u);
			const float pm = lights_pmf(v, row, K, j);
			float e1 = rng.next_f32();
			float e2 = rng.next_f32();
			// the record: one 64-byte line, four 16-byte loads
			const float4 *rec = reinterpret_cast<const float4 *>(tab + j);
			const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3]; // (o, a.x) (a.yz, b.xy) (b.z, N) (invA, radiance, kind, two_sided)
			if (__float_as_uint(r3.z) != 0u && e1 + e2 > 1.0f) {
				e1 = 1.0f - e1;
				e2 = 1.0f - e2;
			}
			const float yx = (r0.x + e1 * r0.w) + e2 * r1.z;
			const float yy = (r0.y + e1 * r1.x) + e2 * r1.w;
			const float yz = (r0.z + e1 * r1.y) + e2 * r2.x;
			const float vx = yx - px, vy = yy - py, vz = yz - pz;
			const float d2 = (vx * vx + vy * vy) + vz * vz;
			const float dist = __builtin_sqrtf(d2);
			const float wx = vx / dist, wy = vy / dist, wz = vz / dist;
			const float cs = (nx * wx + ny * wy) + nz * wz;
			float cl = -((r2.y * wx + r2.z * wy) + r2.w * wz);
			if (__float_as_uint(r3.w) != 0u) cl = __builtin_fabsf(cl);
			const float g = (d2 > 0.0f && cs > 0.0f && cl > 0.0f) ? (cs * cl) / d2 : 0.0f;
			const float tg = r3.y * g;
			const float s = pm * r3.x;
			const float wk = ris_weight(tg, s);
			if (ris_keep(rng, wk, wsum)) {
				kk = k;
				kj = j;
				kyx = yx; kyy = yy; kyz = yz;
				kt = tg;
				ks = s;
			}
			if (kCand) {
				if (a.cand_light_out) a.cand_light_out[(size_t)k * n + i] = j;
				ris_store_cand_vec(a.cand_point_out, n, i, k, yx, yy, yz);
				ris_store_cand_ts(a, n, i, k, tg, s);
			}
		}
		a.rng_state[i] = rng.state;
		if (kk != PG_RESAMPLE_NONE) {
			W = ris_W(wsum, Mf, kt);
			// w and dist of the kept point: the candidate's own operations again on the same numbers (the same bits), which spares
			// the loop four registers
			const float vx = kyx - px, vy = kyy - py, vz = kyz - pz;
			kdist = __builtin_sqrtf((vx * vx + vy * vy) + vz * vz);
			kwx = vx / kdist; kwy = vy / kdist; kwz = vz / kdist;
		}
	} else if (kCand) { // zeros in all the lane's candidate slots
		for (uint32_t k = 0; k < M; ++k) {
			if (a.cand_light_out) a.cand_light_out[(size_t)k * n + i] = 0u;
			ris_store_cand_vec(a.cand_point_out, n, i, k, 0.0f, 0.0f, 0.0f);
			ris_store_cand_ts(a, n, i, k, 0.0f, 0.0f);
		}
	}
	a.light_out[i] = kj;
	a.point_out[i] = kyx;
	a.point_out[n + i] = kyy;
	a.point_out[2 * n + i] = kyz;
	a.weight_out[i] = W;
	if (a.dir_out) {
		a.dir_out[i] = kwx;
		a.dir_out[n + i] = kwy;
		a.dir_out[2 * n + i] = kwz;
	}
	if (a.dist_out) a.dist_out[i] = kdist;
	ris_store_kept_tsi(a, i, kt, ks, kk);
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_nee_set_lights(pg_context *ctx, uint32_t n_lights, const float *h_table, void *stream)
{
	if (!ctx) return PG_ERR_INVALID;
	PG_HIP(ctx, hipSetDevice(ctx->device));
	Nee &ne = ctx->nee;
	if (n_lights == 0) {
		PG_HIP(ctx, hipDeviceSynchronize()); // (kernels that read the table have finished)
		ne.release();
		return PG_OK;
	}
	if (n_lights > PG_LIGHTS_MAX) return fail(ctx, PG_ERR_INVALID, "pg_nee_set_lights: more than PG_LIGHTS_MAX lights");
	if (!h_table) return fail(ctx, PG_ERR_INVALID, "pg_nee_set_lights: NULL table");
	for (uint32_t j = 0; j < n_lights; ++j) {
		const float *h = h_table + (size_t)PG_NEE_TABLE_WORDS * j;
		for (int k = 0; k < 9; ++k)
			if (!std::isfinite(h[k])) return fail(ctx, PG_ERR_INVALID, "pg_nee_set_lights: a coordinate is not finite");
		if (!std::isfinite(h[9]) || !(h[9] >= 0.0f))
			return fail(ctx, PG_ERR_INVALID, "pg_nee_set_lights: a radiance is negative or not finite");
		uint32_t kind, two_sided;
		memcpy(&kind, h + 10, sizeof kind);
		memcpy(&two_sided, h + 11, sizeof two_sided);
		if (kind > 1u) return fail(ctx, PG_ERR_INVALID, "pg_nee_set_lights: kind must be 0 (parallelogram) or 1 (triangle)");
		if (two_sided > 1u) return fail(ctx, PG_ERR_INVALID, "pg_nee_set_lights: two_sided must be 0 or 1");
	}
	PG_HIP(ctx, hipDeviceSynchronize()); // (kernels that read the table it replaces have finished)
	DevBuf<float> raw;
	hipError_t e = raw.ensure((size_t)n_lights * PG_NEE_TABLE_WORDS);
	if (e == hipSuccess) e = ne.tab.ensure(n_lights);
	if (e != hipSuccess) {
		ne.release();
		return hip_fail(ctx, e, "pg_nee_set_lights: table");
	}
	ne.n_lights = 0; // (until the records are written)
	PG_HIP(ctx, hipMemcpy(raw.p, h_table, (size_t)n_lights * PG_NEE_TABLE_WORDS * sizeof(float), hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_nee_prepare, dim3((n_lights + kQueryBlock - 1) / kQueryBlock), dim3(kQueryBlock), 0, (hipStream_t)stream, raw.p,
	                   ne.tab.p, n_lights);
	PG_LAUNCHED(ctx);
	PG_HIP(ctx, hipDeviceSynchronize()); // (the staging copy is freed behind it)
	ne.n_lights = n_lights;
	return PG_OK;
}

int pg_nee_status(pg_context *ctx, uint32_t *n_lights)
{
	if (!ctx) return PG_ERR_INVALID;
	if (!n_lights) return fail(ctx, PG_ERR_INVALID, "pg_nee_status: NULL pointer");
	*n_lights = ctx->nee.n_lights;
	return PG_OK;
}

int pg_nee_resample(pg_context *ctx, uint64_t n, const pg_nee_params *params, const pg_nee_args *args, void *stream)
{
	PG_READY(ctx);
	if (!params) return fail(ctx, PG_ERR_INVALID, "pg_nee_resample: NULL params");
	if (!args) return fail(ctx, PG_ERR_INVALID, "pg_nee_resample: NULL args");
	const pg_nee_params &prm = *params;
	const pg_nee_args &a = *args;
	if (ctx->nee.n_lights == 0) return fail(ctx, PG_ERR_INVALID, "pg_nee_resample: no light table: call pg_nee_set_lights first");
	if (!ctx->lights.on()) return fail(ctx, PG_ERR_INVALID, "pg_nee_resample: the lights feature is disabled: call pg_lights_enable first");
	if (ctx->lights.n_lights != ctx->nee.n_lights)
		return fail(ctx, PG_ERR_INVALID, "pg_nee_resample: n_lights of pg_lights_enable does not match the light table's");
	if (n && (!a.p || !a.normal || !a.rng_state || !a.rng_inc || !a.light_out || !a.point_out || !a.weight_out))
		return fail(ctx, PG_ERR_INVALID, "pg_nee_resample: NULL pointer");
	if (int rc = resample_candidates(ctx, "pg_nee_resample", prm.candidates)) return rc;
	if (prm.reserved[0] != 0u || prm.reserved[1] != 0u || prm.reserved[2] != 0u)
		return fail(ctx, PG_ERR_INVALID, "pg_nee_resample: reserved must be 0");
	if (int rc = resample_lanes(ctx, "pg_nee_resample", n)) return rc;
	if (n == 0) return PG_OK;
	const TreeView t = ctx->view();
	const LightsView v = lights_view(ctx);
	const hipStream_t s = (hipStream_t)stream;
	if (a.cand_light_out || a.cand_point_out || a.cand_target_out || a.cand_source_out)
		hipLaunchKernelGGL((k_nee_resample<true>), query_grid(n), dim3(kQueryBlock), 0, s, t, v, ctx->nee.tab.p, n, a, prm.candidates,
		                   (float)prm.candidates);
	else
		hipLaunchKernelGGL((k_nee_resample<false>), query_grid(n), dim3(kQueryBlock), 0, s, t, v, ctx->nee.tab.p, n, a, prm.candidates,
		                   (float)prm.candidates);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

} // extern "C"
