// pg_kernels_lights.hip -- light selection learned per KD leaf (include/ext/pg_lights.h, which states the semantics operation by
// operation): the sample, the pmf, the record, the build, the refine's carry, and the nine entry points.
// wave64, 256-thread groups.
//
// No existing kernel is touched: the kernels here use the descent of pg_descent.hpp and the quantisation of pg_math.hpp as they
// are, and the record repeats the three exact merge stages of k_fraction_record (pg_kernels_fraction.hip, whose head says why
// they exist) with the key tree * n_lights + light in the place of the tree:
//   1. the wave: lanes matched by key, a matched group's four words summed with shuffles;
//   2. the workgroup: leaders and unmatched lanes add into a hash table in LDS keyed by the key;
//   3. the device: behind the block's last tile, four adjacent lanes send an entry's four words in one wave-instruction.
// Every partial sum is a 64-bit integer add, so any order leaves the same words.  With many lights a wave's groups are smaller
// than the fraction's (the key is finer than the leaf), which moves work from stage 1 to stage 2; the table is the same size.
// (A copy, not a shared body -- DESIGN.md 5.23 -- so a fix to the stages here belongs in pg_kernels_fraction.hip too.)
//
// The table of a context is [ acc: n_trees x L x 4 int64 | rows: n_trees x L uint32 ] (pg_context.hpp: Lights): a leaf's row is
// contiguous, so the binary search of a sample touches log2(L) of its 4 L bytes and neighbours of a sorted wave share the lines.
#include "../../include/ext/pg_lights.h"
#include "pg_context.hpp"
#include "pg_descent.hpp"
#include "pg_lights_dev.hpp"

#include <cmath>
#include <vector>

namespace pg {

constexpr uint32_t kLightsNoKey = 0xffffffffu; // (never a key: tree * L + light < 2^31)
constexpr int kLightsWaveRounds = 4;           // distinct keys of a wave merged in registers; the rest go to the table lane by lane
constexpr int kLightsTableSlots = 512;         // LDS hash table of the workgroup: key -> four words
constexpr int kLightsProbes = 4;               // linear probes before a lane gives up on the table and adds to the device itself
constexpr unsigned kLightsGroupsPerCu = 8;
constexpr uint32_t kLightsWaveRow = 256;       // rows up to this long are built by one wave, longer ones by one workgroup
static_assert((kLightsTableSlots & (kLightsTableSlots - 1)) == 0 && kLightsTableSlots % (kQueryBlock / 4) == 0,
              "the flush takes 64 slots per pass");
static_assert(kQueryBlock == 256, "four waves per group: the build's LDS arrays");

// ---- sample and pmf ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kQueryBlock) void k_lights_sample(TreeView t, LightsView v, uint64_t n, const float *__restrict__ p,
                                                           const float *__restrict__ u, uint64_t *__restrict__ rng_state,
                                                           const uint64_t *__restrict__ rng_inc,
                                                           const uint8_t *__restrict__ active,
                                                           uint32_t *__restrict__ light_out, float *__restrict__ pmf_out)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = active ? active[i] != 0 : true;
	if (!act) {
		light_out[i] = PG_LIGHTS_NONE;
		pmf_out[i] = 0.0f;
		return;
	}
	float uu;
	if (u) uu = u[i]; // (uniform over the launch)
	else {
		Pcg32 rng;
		rng.state = rng_state[i];
		rng.inc = rng_inc[i];
		uu = rng.next_f32();
		rng_state[i] = rng.state;
	}
	if (!(uu >= 0.0f && uu < 1.0f)) uu = 0.0f;
	uint32_t K;
	const uint32_t *row = lights_row(t, s_planes, v, p[i], p[n + i], p[2 * n + i], K);
	const uint32_t j = lights_select(v, row, K, uu);
	light_out[i] = j;
	pmf_out[i] = lights_pmf(v, row, K, j);
}

__global__ __launch_bounds__(kQueryBlock) void k_lights_pmf(TreeView t, LightsView v, uint64_t n, const float *__restrict__ p,
                                                        const uint32_t *__restrict__ light, const uint8_t *__restrict__ active,
                                                        float *__restrict__ pmf_out)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	stage_kd_planes(s_planes, t);
	const uint64_t i = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
	if (i >= n) return;
	const bool act = active ? active[i] != 0 : true;
	const uint32_t j = light[i];
	float pmf = 0.0f;
	if (act && j < v.L) {
		uint32_t K;
		const uint32_t *row = lights_row(t, s_planes, v, p[i], p[n + i], p[2 * n + i], K);
		pmf = lights_pmf(v, row, K, j);
	}
	pmf_out[i] = pmf;
}

// ---- record --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long lights_wave_sum_u64(unsigned long long v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// stage 2: (key, w) into the workgroup's table; a lane that finds no slot within kLightsProbes adds to the device itself
__device__ __forceinline__ void lights_table_add(uint32_t *s_key, unsigned long long *s_val, long long *acc, uint32_t key,
                                                 const unsigned long long (&w)[4])
{
	uint32_t h = (key * 0x9e3779b1u) >> 23; // (top 9 bits: kLightsTableSlots = 512)
	static_assert(kLightsTableSlots == 512, "the hash takes nine bits");
	bool placed = false;
#pragma unroll
	for (int k = 0; k < kLightsProbes; ++k) {
		if (!placed) {
			const uint32_t prev = atomicCAS(&s_key[h], kLightsNoKey, key);
			if (prev == kLightsNoKey || prev == key) placed = true;
			else h = (h + 1u) & (kLightsTableSlots - 1);
		}
	}
	if (placed) { // (two branches, two address spaces: no pointer that is "LDS or device")
#pragma unroll
		for (int k = 0; k < 4; ++k)
			if (w[k]) atomicAdd(s_val + 4 * h + k, w[k]);
	} else {
		unsigned long long *dst = reinterpret_cast<unsigned long long *>(acc + (size_t)kAccWords * key);
#pragma unroll
		for (int k = 0; k < 4; ++k)
			if (w[k]) atomicAdd(dst + k, w[k]);
	}
}

__global__ __launch_bounds__(kQueryBlock) void k_lights_record(TreeView t, long long *__restrict__ acc, uint32_t L, uint64_t m,
                                                           pg_lights_records r, const uint32_t *__restrict__ d_count)
{
	__shared__ float s_planes[3 * kKdGridPlanes];
	__shared__ uint32_t s_key[kLightsTableSlots];
	__shared__ unsigned long long s_val[kLightsTableSlots * 4];
	for (int k = threadIdx.x; k < kLightsTableSlots; k += kQueryBlock) s_key[k] = kLightsNoKey;
	for (int k = threadIdx.x; k < kLightsTableSlots * 4; k += kQueryBlock) s_val[k] = 0ull;
	stage_kd_planes(s_planes, t); // (holds the barrier behind the table's initialisation)
	uint64_t valid = d_count ? (uint64_t)*d_count : m; // plane stride stays m
	if (valid > m) valid = m;
	const uint64_t tiles = (valid + kQueryBlock - 1) / kQueryBlock;
	const unsigned lane = threadIdx.x & 63u;
	for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (uniform over the workgroup)
		const uint64_t i = tile * kQueryBlock + threadIdx.x;
		uint32_t key = kLightsNoKey;
		Limbs q = {0, 0, 0};
		if (i < valid) {
			const float x = r.position[i], y = r.position[m + i], z = r.position[2 * m + i], value = r.value[i];
			const uint32_t light = r.light[i];
			if (inside_root(t, x, y, z) && light < L && finite_f32(value) && value >= 0.0f) {
				KdNode leaf;
				uint32_t lv;
				kd_descend_grid(t, s_planes, x, y, z, true, leaf, lv);
				key = leaf.tree * L + light;
				q = quantize_weight(value);
			}
		}
		unsigned long long w[4] = {(unsigned long long)q.l0, (unsigned long long)q.l1, (unsigned long long)q.l2,
		                           key != kLightsNoKey ? 1ull : 0ull};
		// stage 1: the wave's lanes matched by key.  `pending` lanes still hold a record nobody has taken over.
		bool pending = key != kLightsNoKey;
#pragma unroll 1
		for (int round = 0; round < kLightsWaveRounds; ++round) {
			const unsigned long long pend = __ballot(pending);
			if (pend == 0) break; // (uniform over the wave)
			const int lead = __builtin_ctzll(pend);
			const uint32_t lead_key = (uint32_t)__shfl((int)key, lead, 64);
			const bool peer = pending && key == lead_key;
			const unsigned long long peers = __ballot(peer);
			if (peers != (1ull << lead)) { // more than the leader: sum the group's words across the wave
				unsigned long long s[4];
#pragma unroll
				for (int k = 0; k < 4; ++k) s[k] = lights_wave_sum_u64(peer ? w[k] : 0ull);
				if (peer) {
#pragma unroll
					for (int k = 0; k < 4; ++k) w[k] = lane == (unsigned)lead ? s[k] : 0ull;
					if (lane != (unsigned)lead) key = kLightsNoKey; // (taken over by the leader)
				}
			}
			if (peer) {
				pending = false;
				if (key != kLightsNoKey) lights_table_add(s_key, s_val, acc, key, w); // the group's leader
			}
		}
		if (pending) lights_table_add(s_key, s_val, acc, key, w); // a wave of many keys: lane by lane
	}
	// stage 3: the table leaves the CU, four adjacent lanes per entry -- one sector update per distinct key of the workgroup
	__syncthreads();
	const unsigned word = threadIdx.x & 3u;
#pragma unroll 1
	for (int base = 0; base < kLightsTableSlots; base += kQueryBlock / 4) {
		const int slot = base + (int)(threadIdx.x >> 2);
		const uint32_t key = s_key[slot];
		const unsigned long long v = s_val[4 * slot + word];
		if (key != kLightsNoKey && v != 0ull)
			atomicAdd(reinterpret_cast<unsigned long long *>(acc + (size_t)kAccWords * key + word), v);
	}
}

// ---- build ---------------------------------------------------------------------------------------------------------------------
// m_j of the header from a light's four words
__device__ __forceinline__ float lights_mean(const long long *a, bool root)
{
	const long long w0 = a[0], w1 = a[1], w2 = a[2], count = a[3];
	float m = 0.0f;
	if (count > 0) m = i128_to_f32(limbs_resolve(w0, w1, w2)) / (float)count;
	if (root) m = __builtin_sqrtf(m);
	return (finite_f32(m) && m > 0.0f) ? m : 0.0f;
}

__device__ __forceinline__ uint32_t lights_quantum(float m, float M) { return (uint32_t)((m / M) * 65536.0f); }

__device__ __forceinline__ float lights_wave_max(float v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
	return v;
}

__device__ __forceinline__ uint32_t lights_wave_scan(uint32_t v, unsigned lane) // inclusive
{
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t up = (uint32_t)__shfl_up((int)v, o, 64);
		if (lane >= (unsigned)o) v += up;
	}
	return v;
}

// one wave per leaf: rows of up to kLightsWaveRow lights, in chunks of 64 with the carry in a register
__global__ __launch_bounds__(kQueryBlock) void k_lights_build_wave(const long long *__restrict__ acc, uint32_t *__restrict__ rows,
                                                               uint32_t n_trees, uint32_t L, int root)
{
	const unsigned lane = threadIdx.x & 63u;
	const uint64_t leaf = (uint64_t)blockIdx.x * (kQueryBlock / 64) + (threadIdx.x >> 6);
	if (leaf >= n_trees) return; // (uniform over the wave; no barrier below)
	const long long *a = acc + (size_t)leaf * L * kAccWords;
	uint32_t *row = rows + (size_t)leaf * L;
	float M = 0.0f;
	for (uint32_t j = lane; j < L; j += 64u) M = fmaxf(M, lights_mean(a + (size_t)kAccWords * j, root != 0));
	M = lights_wave_max(M);
	if (!(M > 0.0f)) return; // the leaf keeps its row
	uint32_t carry = 0u;
	for (uint32_t base = 0u; base < L; base += 64u) { // (uniform over the wave)
		const uint32_t j = base + lane;
		const uint32_t k = j < L ? lights_quantum(lights_mean(a + (size_t)kAccWords * j, root != 0), M) : 0u;
		const uint32_t s = lights_wave_scan(k, lane);
		if (j < L) row[j] = carry + s;
		carry += (uint32_t)__shfl((int)s, 63, 64);
	}
}

// one workgroup per leaf: longer rows, in chunks of 256 with the waves' totals in LDS
__global__ __launch_bounds__(kQueryBlock) void k_lights_build_group(const long long *__restrict__ acc, uint32_t *__restrict__ rows,
                                                                uint32_t L, int root)
{
	__shared__ float s_max[kQueryBlock / 64];
	__shared__ uint32_t s_tot[kQueryBlock / 64];
	const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const long long *a = acc + (size_t)blockIdx.x * L * kAccWords;
	uint32_t *row = rows + (size_t)blockIdx.x * L;
	float M = 0.0f;
	for (uint32_t j = threadIdx.x; j < L; j += kQueryBlock) M = fmaxf(M, lights_mean(a + (size_t)kAccWords * j, root != 0));
	M = lights_wave_max(M);
	if (lane == 0u) s_max[wave] = M;
	__syncthreads();
	M = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
	if (!(M > 0.0f)) return; // the leaf keeps its row (uniform over the workgroup)
	uint32_t carry = 0u;
	for (uint32_t base = 0u; base < L; base += kQueryBlock) { // (uniform over the workgroup)
		const uint32_t j = base + threadIdx.x;
		const uint32_t k = j < L ? lights_quantum(lights_mean(a + (size_t)kAccWords * j, root != 0), M) : 0u;
		const uint32_t s = lights_wave_scan(k, lane);
		if (lane == 63u) s_tot[wave] = s;
		__syncthreads();
		const uint32_t t0 = s_tot[0], t1 = s_tot[1], t2 = s_tot[2], t3 = s_tot[3];
		const uint32_t below = wave == 0u ? 0u : (wave == 1u ? t0 : (wave == 2u ? t0 + t1 : t0 + t1 + t2));
		if (j < L) row[j] = carry + below + s;
		carry += t0 + t1 + t2 + t3;
		__syncthreads(); // (s_tot is written again by the next chunk)
	}
}

// ---- tables ------------------------------------------------------------------------------------------------------------------
// zero words: every leaf unlearned with zero accumulators (pg_lights_enable), the accumulators of a refined forest or of an import
__global__ __launch_bounds__(kQueryBlock) void k_lights_zero(long long *__restrict__ tab, uint64_t words)
{
	for (uint64_t k = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x; k < words; k += (uint64_t)gridDim.x * kQueryBlock) tab[k] = 0;
}

// the rows of a refined forest: new leaf t has the row of old leaf tree_src[t] (pg_refine.hip)
__global__ __launch_bounds__(kQueryBlock) void k_lights_carry(const uint32_t *__restrict__ old_rows, uint32_t n_old,
                                                          const uint32_t *__restrict__ tree_src, uint32_t *__restrict__ new_rows,
                                                          uint32_t n_new, uint32_t L)
{
	const uint64_t entries = (uint64_t)n_new * L;
	for (uint64_t e = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x; e < entries; e += (uint64_t)gridDim.x * kQueryBlock) {
		const uint32_t t = (uint32_t)(e / L), j = (uint32_t)(e - (uint64_t)t * L);
		uint32_t src = tree_src[t];
		if (src >= n_old) src = 0; // (never: tree_src names pre-refine trees)
		new_rows[e] = old_rows[(size_t)src * L + j];
	}
}

// a grid-stride launch over `items`: as many groups as the device's CUs hold, at most
static dim3 lights_stride_grid(uint64_t items, int n_cus)
{
	const uint64_t blocks = (items + kQueryBlock - 1) / kQueryBlock, cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * kLightsGroupsPerCu;
	return dim3((unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap));
}

hipError_t launch_lights_carry(long long *old_tab, uint32_t n_old, const uint32_t *tree_src, long long *new_tab, uint32_t n_new,
                               uint32_t n_lights, int n_cus, hipStream_t s)
{
	if (n_new == 0 || n_lights == 0) return hipSuccess;
	const uint64_t entries = (uint64_t)n_new * n_lights;
	hipLaunchKernelGGL(k_lights_zero, lights_stride_grid(entries * kAccWords, n_cus), dim3(kQueryBlock), 0, s, new_tab, entries * kAccWords);
	hipLaunchKernelGGL(k_lights_carry, lights_stride_grid(entries, n_cus), dim3(kQueryBlock), 0, s, Lights::rows_of(old_tab, n_old, n_lights),
	                   n_old, tree_src, Lights::rows_of(new_tab, n_new, n_lights), n_new, n_lights);
	return hipGetLastError();
}

} // namespace pg

using namespace pg;

// PG_READY, and the feature is on
#define PG_LIGHTS_ON(ctx, who)                                                                              \
	do {                                                                                                    \
		PG_READY(ctx);                                                                                      \
		if (!(ctx)->lights.on()) return fail((ctx), PG_ERR_INVALID, who ": call pg_lights_enable first");  \
	} while (0)

extern "C" {

int pg_lights_enable(pg_context *ctx, uint32_t n_lights, const pg_lights_params *params)
{
	PG_READY(ctx);
	Lights &li = ctx->lights;
	if (n_lights == 0) {
		PG_HIP(ctx, hipDeviceSynchronize()); // (kernels that read the table have finished)
		li.disable();
		return PG_OK;
	}
	if (!params) return fail(ctx, PG_ERR_INVALID, "pg_lights_enable: NULL params");
	if (n_lights > PG_LIGHTS_MAX) return fail(ctx, PG_ERR_INVALID, "pg_lights_enable: more than PG_LIGHTS_MAX lights");
	if (!(params->delta >= 0.0f && params->delta <= 1.0f) || params->root > 1u || params->reserved != 0u)
		return fail(ctx, PG_ERR_INVALID, "pg_lights_enable: parameter out of range (pg_lights.h)");
	const uint64_t entries = (uint64_t)ctx->f.n_trees * n_lights;
	if (entries > kLightsMaxEntries) return fail(ctx, PG_ERR_INVALID, "pg_lights_enable: leaves x lights exceeds 2^31");
	PG_HIP(ctx, hipDeviceSynchronize());
	const size_t words = Lights::words(entries);
	hipError_t e = li.tab.ensure(words);
	if (e != hipSuccess) {
		li.disable();
		return hip_fail(ctx, e, "pg_lights_enable: table");
	}
	hipLaunchKernelGGL(k_lights_zero, lights_stride_grid(words, ctx->n_cus), dim3(kQueryBlock), 0, nullptr, li.tab.p, (uint64_t)words);
	PG_LAUNCHED(ctx);
	PG_HIP(ctx, hipDeviceSynchronize());
	li.prm = *params;
	li.n_lights = n_lights;
	return PG_OK;
}

int pg_lights_record(pg_context *ctx, uint64_t m, const pg_lights_records *rec, const uint32_t *d_count, void *stream)
{
	PG_LIGHTS_ON(ctx, "pg_lights_record");
	if (!rec) return fail(ctx, PG_ERR_INVALID, "pg_lights_record: NULL records");
	if (m && (!rec->position || !rec->light || !rec->value)) return fail(ctx, PG_ERR_INVALID, "pg_lights_record: NULL record column");
	if (m >= 0xffffffffull) return fail(ctx, PG_ERR_INVALID, "pg_lights_record: more than 2^32 - 1 records in one call");
	if (m == 0) return PG_OK;
	// a persistent grid: a block merges all its tiles in LDS before it sends a key's sum out
	const uint64_t tiles = (m + kQueryBlock - 1) / kQueryBlock, cap = (uint64_t)ctx->n_cus * kLightsGroupsPerCu;
	hipLaunchKernelGGL(k_lights_record, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(kQueryBlock), 0, (hipStream_t)stream,
	                   ctx->view(), ctx->lights.acc(), ctx->lights.n_lights, m, *rec, d_count);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_lights_build(pg_context *ctx, void *stream)
{
	PG_LIGHTS_ON(ctx, "pg_lights_build");
	const Lights &li = ctx->lights;
	const uint32_t n = ctx->f.n_trees, L = li.n_lights;
	if (L <= kLightsWaveRow)
		hipLaunchKernelGGL(k_lights_build_wave, dim3((n + kQueryBlock / 64 - 1) / (kQueryBlock / 64)), dim3(kQueryBlock), 0,
		                   (hipStream_t)stream, li.acc(), li.rows(n), n, L, (int)li.prm.root);
	else
		hipLaunchKernelGGL(k_lights_build_group, dim3(n), dim3(kQueryBlock), 0, (hipStream_t)stream, li.acc(), li.rows(n), L,
		                   (int)li.prm.root);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_lights_sample(pg_context *ctx, uint64_t n, const float *p, const float *u, uint64_t *rng_state, const uint64_t *rng_inc,
                     const uint8_t *active, uint32_t *light_out, float *pmf_out, void *stream)
{
	PG_LIGHTS_ON(ctx, "pg_lights_sample");
	if (n && (!p || !light_out || !pmf_out)) return fail(ctx, PG_ERR_INVALID, "pg_lights_sample: NULL pointer");
	if (n && !u && (!rng_state || !rng_inc)) return fail(ctx, PG_ERR_INVALID, "pg_lights_sample: neither u nor the sampler's streams");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_lights_sample: too many lanes for one launch");
	if (n == 0) return PG_OK;
	hipLaunchKernelGGL(k_lights_sample, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), lights_view(ctx), n, p, u,
	                   rng_state, rng_inc, active, light_out, pmf_out);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_lights_pmf(pg_context *ctx, uint64_t n, const float *p, const uint32_t *light, const uint8_t *active, float *pmf_out,
                  void *stream)
{
	PG_LIGHTS_ON(ctx, "pg_lights_pmf");
	if (n && (!p || !light || !pmf_out)) return fail(ctx, PG_ERR_INVALID, "pg_lights_pmf: NULL pointer");
	if (n > 0xffffffffull * kQueryBlock) return fail(ctx, PG_ERR_INVALID, "pg_lights_pmf: too many lanes for one launch");
	if (n == 0) return PG_OK;
	hipLaunchKernelGGL(k_lights_pmf, query_grid(n), dim3(kQueryBlock), 0, (hipStream_t)stream, ctx->view(), lights_view(ctx), n, p, light,
	                   active, pmf_out);
	PG_LAUNCHED(ctx);
	return PG_OK;
}

int pg_lights_accumulators(pg_context *ctx, int64_t **d_buffer, uint64_t *count)
{
	PG_LIGHTS_ON(ctx, "pg_lights_accumulators");
	if (!d_buffer || !count) return fail(ctx, PG_ERR_INVALID, "pg_lights_accumulators: NULL pointer");
	*d_buffer = reinterpret_cast<int64_t *>(ctx->lights.acc());
	*count = (uint64_t)ctx->f.n_trees * ctx->lights.n_lights * kAccWords;
	return PG_OK;
}

int pg_lights_status(pg_context *ctx, uint32_t *n_lights, uint64_t *n_learned_leaves)
{
	PG_READY(ctx);
	const Lights &li = ctx->lights;
	if (n_lights) *n_lights = li.n_lights;
	if (!n_learned_leaves) return PG_OK;
	*n_learned_leaves = 0;
	if (!li.on()) return PG_OK;
	const uint32_t n = ctx->f.n_trees, L = li.n_lights;
	PG_HIP(ctx, hipDeviceSynchronize());
	std::vector<uint32_t> last(n); // K of every leaf: the last column of the rows
	PG_HIP(ctx, hipMemcpy2D(last.data(), sizeof(uint32_t), li.rows(n) + (L - 1u), (size_t)L * sizeof(uint32_t), sizeof(uint32_t), n,
	                        hipMemcpyDeviceToHost));
	uint64_t learned = 0;
	for (uint32_t k : last) learned += k != 0u;
	*n_learned_leaves = learned;
	return PG_OK;
}

int pg_lights_export(pg_context *ctx, uint64_t n_trees, uint32_t n_lights, uint32_t *h_rows, int64_t *h_acc)
{
	PG_LIGHTS_ON(ctx, "pg_lights_export");
	const Lights &li = ctx->lights;
	if (n_trees != ctx->f.n_trees) return fail(ctx, PG_ERR_INVALID, "pg_lights_export: n_trees does not match pg_export_sizes' n_roots");
	if (n_lights != li.n_lights) return fail(ctx, PG_ERR_INVALID, "pg_lights_export: n_lights does not match pg_lights_enable's");
	if (!h_rows) return fail(ctx, PG_ERR_INVALID, "pg_lights_export: NULL pointer");
	const size_t entries = (size_t)n_trees * n_lights;
	PG_HIP(ctx, hipDeviceSynchronize());
	PG_HIP(ctx, hipMemcpy(h_rows, li.rows(ctx->f.n_trees), entries * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (h_acc) PG_HIP(ctx, hipMemcpy(h_acc, li.acc(), entries * kAccWords * sizeof(long long), hipMemcpyDeviceToHost));
	return PG_OK;
}

int pg_lights_import(pg_context *ctx, uint64_t n_trees, uint32_t n_lights, const uint32_t *h_rows)
{
	PG_LIGHTS_ON(ctx, "pg_lights_import");
	const Lights &li = ctx->lights;
	if (n_trees != ctx->f.n_trees) return fail(ctx, PG_ERR_INVALID, "pg_lights_import: n_trees does not match pg_export_sizes' n_roots");
	if (n_lights != li.n_lights) return fail(ctx, PG_ERR_INVALID, "pg_lights_import: n_lights does not match pg_lights_enable's");
	if (!h_rows) return fail(ctx, PG_ERR_INVALID, "pg_lights_import: NULL pointer");
	for (uint64_t t = 0; t < n_trees; ++t) {
		const uint32_t *row = h_rows + t * n_lights;
		uint32_t prev = 0;
		for (uint32_t j = 0; j < n_lights; ++j) {
			if (row[j] < prev) return fail(ctx, PG_ERR_INVALID, "pg_lights_import: a row does not ascend");
			if (row[j] - prev > PG_LIGHTS_WEIGHT_ONE) return fail(ctx, PG_ERR_INVALID, "pg_lights_import: a row's step exceeds 65536");
			prev = row[j];
		}
	}
	const size_t entries = (size_t)n_trees * n_lights;
	PG_HIP(ctx, hipDeviceSynchronize());
	hipLaunchKernelGGL(k_lights_zero, lights_stride_grid(entries * kAccWords, ctx->n_cus), dim3(kQueryBlock), 0, nullptr, li.acc(),
	                   (uint64_t)entries * kAccWords);
	PG_LAUNCHED(ctx);
	PG_HIP(ctx, hipMemcpy(li.rows(ctx->f.n_trees), h_rows, entries * sizeof(uint32_t), hipMemcpyHostToDevice));
	PG_HIP(ctx, hipDeviceSynchronize());
	return PG_OK;
}

} // extern "C"
