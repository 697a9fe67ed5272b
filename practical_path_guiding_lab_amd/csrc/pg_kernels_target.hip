// pg_kernels_target.hip -- the variance-aware guiding target (include/pgsd_target.h, which states the semantics operation by
// operation): one pass over the accumulators of sdTree_current that replaces every directional LEAF's sum S by
// 2^-depth * sqrt(S), and the two entry points.  wave64, 256-thread groups.
//
// No existing kernel is touched: the refine that follows resolves the interior nodes from the transformed leaves exactly as it
// resolves them from recorded ones (k_resolve_level, pg_refine.hip), so "sqrt at the leaves, then refine" is this one launch.
//
// k_target_second_moment: one lane per accumulator slot of [ n_rec * 4 record slots | n_trees root slots ] -- the slots are
// contiguous in the buffer, 32 bytes each, so slot i lives at word 4 i whichever kind it is.  Four adjacent lanes own the four
// children of one record: a wave covers sixteen whole 128-byte lines, and reads the sixteen records' child words beside them
// (4 bytes per slot: the second half of each QuadRec).  Whether a slot is a leaf is that child word (0), or the head's root_rec
// for a root slot; an interior slot's lane ends there, its sector is neither read nor written (rewriting it unchanged to keep
// every line whole was measured: 0.104 against 0.087 ms on the 215 MB of the veach-ajar bench forest, no difference on a forest
// that fits the caches -- DESIGN.md 5.17, profiles/target/).  The depth of a record's children is the level of the record + 1:
// the forest's at most kTargetLevels level offsets come by value (uniform, scalar registers), and a lane counts how many of
// them its record number has reached -- no divergence, no search, one launch for the whole forest (the refine's ~40 small
// launches are what make it latency-bound; this adds one).
// No LDS, no scratch, no atomics: nothing else runs on the buffer between the last record and the refine (pgsd_target.h).
#include "../../include/pgsd_target.h"
#include "pg_context.hpp"

namespace pg {

constexpr int kTBlock = 256;
constexpr int kTargetLevels = kMaxLevels + 1; // a refine stops below kMaxLevels - 2 record levels; an import may bring a few more

// first record of every level, ascending; entries past the forest's levels hold 0xffffffff (no record number reaches them)
struct TargetLevels {
	uint32_t off[kTargetLevels];
};

// an accumulator is two native 16-byte vectors (a load through a struct of words is four scalar loads: pg_tree.hpp)
typedef long long i64x2_t __attribute__((ext_vector_type(2)));

// the transform of pgsd_target.h: words 0..2 of a leaf at depth d
__device__ __forceinline__ Limbs second_moment_leaf(long long l0, long long l1, long long l2, uint32_t depth)
{
	const float s = i128_to_f32(limbs_resolve(l0, l1, l2));
	float t = s > 0.0f ? __builtin_sqrtf(s) : 0.0f;
	t = t * __uint_as_float((127u - depth) << 23); // 2^-depth, exact (depth < 127; t >= 2^-20 or 0: no denormal)
	return quantize_weight(t);
}

__global__ __launch_bounds__(kTBlock) void k_target_second_moment(const QuadRec *__restrict__ rec,
                                                                  const TreeHead *__restrict__ head,
                                                                  long long *__restrict__ acc, uint64_t n_rec_slots,
                                                                  uint64_t n_slots, TargetLevels lv)
{
	const uint64_t i = (uint64_t)blockIdx.x * kTBlock + threadIdx.x;
	if (i >= n_slots) return;
	bool leaf;
	uint32_t depth = 0;
	if (i < n_rec_slots) {
		const uint32_t r = (uint32_t)(i >> 2);
		// the record's child word, the second 16 bytes of QuadRec (what k_resolve_level reads): this lane's quarter of it
		leaf = reinterpret_cast<const uint32_t *>(rec + r)[4 + ((uint32_t)i & 3u)] == 0u;
#pragma unroll
		for (int l = 0; l < kTargetLevels; ++l) depth += r >= lv.off[l] ? 1u : 0u; // level + 1 (off[0] == 0 always counts)
	} else {
		leaf = head[i - n_rec_slots].root_rec == kNoRecord;
	}
	if (!leaf) return;
	i64x2_t *a = reinterpret_cast<i64x2_t *>(acc + i * kAccWords);
	const i64x2_t w01 = a[0];
	const i64x2_t w23 = a[1];
	const Limbs q = second_moment_leaf(w01.x, w01.y, w23.x, depth);
	i64x2_t o01, o23;
	o01.x = q.l0;
	o01.y = q.l1;
	o23.x = q.l2;
	o23.y = w23.y; // the count keeps its value
	a[0] = o01;
	a[1] = o23;
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_target_apply(pg_context *ctx, int32_t target, void *stream)
{
	PG_READY(ctx);
	if (target != PG_TARGET_SECOND_MOMENT) return fail(ctx, PG_ERR_INVALID, "pg_target_apply: unknown target (pgsd_target.h)");
	if (ctx->target_applied)
		return fail(ctx, PG_ERR_INVALID, "pg_target_apply: a target was already applied to these accumulators; refine first");
	const Forest &f = ctx->f;
	const size_t levels = f.level_off.size() - 1; // record levels
	if (levels > (size_t)kTargetLevels) return fail(ctx, PG_ERR_INVALID, "pg_target_apply: quadtree deeper than supported");
	TargetLevels lv;
	for (size_t l = 0; l < (size_t)kTargetLevels; ++l) lv.off[l] = l < levels ? f.level_off[l] : 0xffffffffu;
	const uint64_t n_rec_slots = (uint64_t)f.n_rec * 4, n_slots = f.n_acc();
	if (n_slots) {
		hipLaunchKernelGGL(k_target_second_moment, dim3((unsigned)((n_slots + kTBlock - 1) / kTBlock)), dim3(kTBlock), 0,
		                   (hipStream_t)stream, f.rec.p, f.head.p, f.acc.p, n_rec_slots, n_slots, lv);
		PG_LAUNCHED(ctx);
	}
	ctx->target_applied = target;
	return PG_OK;
}

int pg_target_applied(pg_context *ctx, int32_t *out)
{
	if (!ctx) return PG_ERR_INVALID;
	if (!out) return fail(ctx, PG_ERR_INVALID, "pg_target_applied: NULL pointer");
	*out = ctx->target_applied;
	return PG_OK;
}

} // extern "C"
