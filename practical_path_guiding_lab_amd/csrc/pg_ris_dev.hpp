// pg_ris_dev.hpp -- the resampling step of the calls that keep one of M candidates per lane by resampled importance sampling:
// pg_resample_cosine, pg_resample_lobe, pg_resample_interface and pg_nee_resample.  include/pg_resample.h states the semantics
// operation by operation (steps 3 and 4 of a candidate, the outputs behind the loop, the lane that is not served); the other
// three headers refer to it.  Here stand the constants of a call, a candidate's weight, the reservoir's update, W, and the
// stores; what differs per call -- which lanes are served, how a candidate is drawn, the density b -- stays in each kernel.
// The reservoir is the KERNEL's own scalars, assigned in the kernel: k_resample_lobe<false> is held to 96 registers, and a
// reservoir struct cost it 8 bytes of scratch per lane.
// The host's half -- the refusals and the fill of RisConsts -- is resample_consts (pg_context.hpp, pg_kernels_resample.hip).
#pragma once

#include "../../include/pg_resample.h"
#include "pg_math.hpp"

namespace pg {

// what a kernel needs beside the caller's arrays: the parameters and what follows from them alone (fp32, one rounding each)
struct RisConsts {
	uint32_t M;
	float Mf;         // (float)M
	float alpha, om;  // om = 1 - alpha
	float d4, omd;    // delta * INV_4PI, 1 - delta
};

// w of step 3: target over source, 0 where either is not positive or the ratio is not finite
__device__ __forceinline__ float ris_weight(float tg, float s)
{
	const float ratio = tg / s;
	return (s > 0.0f && tg > 0.0f && finite_f32(ratio)) ? ratio : 0.0f;
}

// step 4 behind the lane's one draw zeta: whether the candidate of weight wk is kept.  The caller then keeps k, the candidate's
// target and source and what else it carries (the direction; pg_nee_resample the light and the point) in its own scalars, in
// that order: the order of those assignments is worth registers
__device__ __forceinline__ bool ris_keep(Pcg32 &rng, float wk, float &wsum)
{
	const float zeta = rng.next_f32();
	wsum = wsum + wk;
	return wk > 0.0f && zeta * wsum < wk;
}

// W of a lane that kept a candidate
__device__ __forceinline__ float ris_W(float wsum, float Mf, float kt) { return (wsum / Mf) / kt; }

// candidate k's vector into a float[M][3][n] array that may be NULL (cand_dir_out; pg_nee_resample's cand_point_out)
__device__ __forceinline__ void ris_store_cand_vec(float *out, uint64_t n, uint64_t i, uint32_t k, float x, float y, float z)
{
	if (out) {
		float *o = out + ((size_t)k * 3u * n + i);
		o[0] = x;
		o[n] = y;
		o[2 * n] = z;
	}
}

// candidate k's target and source
template <class Args>
__device__ __forceinline__ void ris_store_cand_ts(const Args &a, uint64_t n, uint64_t i, uint32_t k, float tg, float s)
{
	if (a.cand_target_out) a.cand_target_out[(size_t)k * n + i] = tg;
	if (a.cand_source_out) a.cand_source_out[(size_t)k * n + i] = s;
}

// candidate k of a direction call, kept or not
template <class Args>
__device__ __forceinline__ void ris_store_cand(const Args &a, uint64_t n, uint64_t i, uint32_t k, float x, float y, float z, float tg,
                                               float s)
{
	ris_store_cand_vec(a.cand_dir_out, n, i, k, x, y, z);
	ris_store_cand_ts(a, n, i, k, tg, s);
}

// a lane that is not served: zeros in all its candidate slots
template <class Args>
__device__ __forceinline__ void ris_zero_cands(const Args &a, uint64_t n, uint64_t i, uint32_t M)
{
	for (uint32_t k = 0; k < M; ++k) ris_store_cand(a, n, i, k, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
}

// target, source and index of the kept candidate, or of "nothing kept" as the reservoir stood before the loop
template <class Args>
__device__ __forceinline__ void ris_store_kept_tsi(const Args &a, uint64_t i, float kt, float ks, uint32_t kk)
{
	if (a.target_out) a.target_out[i] = kt;
	if (a.source_out) a.source_out[i] = ks;
	if (a.index_out) a.index_out[i] = kk;
}

// the outputs of a direction call
template <class Args>
__device__ __forceinline__ void ris_store_kept(const Args &a, uint64_t n, uint64_t i, float kx, float ky, float kz, float W, float kt,
                                               float ks, uint32_t kk)
{
	a.dir_out[i] = kx;
	a.dir_out[n + i] = ky;
	a.dir_out[2 * n + i] = kz;
	a.weight_out[i] = W;
	ris_store_kept_tsi(a, i, kt, ks, kk);
}

} // namespace pg
