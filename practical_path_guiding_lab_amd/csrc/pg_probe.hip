// pg_probe.hip -- pg_scene_intersect: the renderer's ray casting by itself, for tests.  One ray per lane through intersect<>
// of pg_render_dev.hpp -- the function the render kernels call, not a copy -- in the three forms those kernels give its walk:
// the ray-casting kernels' (kLdsStack stack entries and kBvhTopNodes nodes in LDS), k_wave_shade's (kShadeStack entries,
// kShadeTopNodes nodes, the kSlim walk) and one without staged nodes.  Nothing of the product path launches this kernel.
#include "pg_render_dev.hpp"
#include "pg_scene_state.hpp"

using namespace pg;

namespace {

constexpr uint64_t kProbeMaxRays = 1ull << 20; // (kProbeMaxRays * kOvfStack < 2^32: BvhStack::ovf_first is a 32-bit entry index)
static_assert(kProbeMaxRays * (uint64_t)kOvfStack <= 0xffffffffull, "pg_scene_intersect: the overflow strips are indexed by 32 bits");

struct ProbeArgs {
	Shapes shapes;
	uint64_t n;
	const float *o, *d, *tmax; // (n,3), (n,3), (n)
	float *t, *uv;             // (n), (n,2)
	int32_t *prim;             // (n)
	uint2 *ovf;                // n * kOvfStack entries
};

// Every loop a lane runs here is bounded: intersect_linear by the shape counts, a leaf by its 1..8 triangles, and the walk by
// BvhWalk::budget -- the node loop and bvh_pop test it, and with the budget spent the outer loop of intersect() pops nothing
// and ends.  So a ray of NaNs or zeros, for which every box test says "maybe", ends after at most 8 * nodes + 8 steps; the
// stack cannot outgrow n_lds + kOvfStack entries whatever the ray is (pg_scene_set_ex has checked the tree for that).
template <int kLevel, bool kAny, int kForm>
__global__ __launch_bounds__(kRBlock) void k_probe_intersect(ProbeArgs p)
{
	constexpr int kStack = kForm == 1 ? kShadeStack : kLdsStack;
	constexpr int kTop = kForm == 1 ? kShadeTopNodes : kBvhTopNodes;
	__shared__ uint2 s_stack[kStack][kRBlock];
	const uint64_t tid = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
	BvhStack stk = bvh_stack(&s_stack[0][threadIdx.x], p.ovf, (uint32_t)tid * (uint32_t)kOvfStack, kStack);
	if (kForm != 2) { // (form 2 leaves stk.n_top = 0: every node is read from memory)
		__shared__ u32x4_t s_top[kTop * kBvhNodeQuads];
		RenderArgs a;
		a.shapes = p.shapes;
		stage_bvh_top<kTop>(s_top, a, stk);
	}
	if (tid >= p.n) return;
	const v3 o = ld3(p.o + 3 * tid), d = ld3(p.d + 3 * tid);
	float t, bu = 0.0f, bv = 0.0f;
	const int prim = intersect<kLevel, kAny, kForm == 1>(p.shapes, o, d, p.tmax[tid], t, stk, bu, bv);
	p.t[tid] = t;
	p.prim[tid] = prim;
	p.uv[2 * tid] = bu;
	p.uv[2 * tid + 1] = bv;
}

template <int kLevel, bool kAny>
void launch_form(int form, dim3 grid, hipStream_t s, const ProbeArgs &p)
{
	if (form == 0) hipLaunchKernelGGL((k_probe_intersect<kLevel, kAny, 0>), grid, dim3(kRBlock), 0, s, p);
	else if (form == 1) hipLaunchKernelGGL((k_probe_intersect<kLevel, kAny, 1>), grid, dim3(kRBlock), 0, s, p);
	else hipLaunchKernelGGL((k_probe_intersect<kLevel, kAny, 2>), grid, dim3(kRBlock), 0, s, p);
}

template <int kLevel>
void launch_any(bool any, int form, dim3 grid, hipStream_t s, const ProbeArgs &p)
{
	if (any) launch_form<kLevel, true>(form, grid, s, p);
	else launch_form<kLevel, false>(form, grid, s, p);
}

} // namespace

int pg_scene_intersect(pg_context *ctx, uint64_t n, const float *d_origin, const float *d_dir, const float *d_tmax,
                       int32_t any_hit, int32_t walk_form, float *d_t, int32_t *d_prim, float *d_uv, void *stream)
{
	if (!ctx) return PG_ERR_INVALID;
	if (!ctx->render || !scene_state(ctx).have_scene) return fail(ctx, PG_ERR_INVALID, "pg_scene_intersect: call pg_scene_set first");
	if (walk_form < 0 || walk_form > 2) return fail(ctx, PG_ERR_INVALID, "pg_scene_intersect: walk_form must be 0, 1 or 2");
	if (n > kProbeMaxRays) return fail(ctx, PG_ERR_INVALID, "pg_scene_intersect: at most 2^20 rays in one call");
	if (n == 0) return PG_OK;
	if (!d_origin || !d_dir || !d_tmax || !d_t || !d_prim || !d_uv) return fail(ctx, PG_ERR_INVALID, "pg_scene_intersect: NULL pointer");
	PG_HIP(ctx, hipSetDevice(ctx->device));
	const SceneState &sc = scene_state(ctx);
	ProbeArgs p;
	p.shapes.quads = sc.quads.p; p.shapes.spheres = sc.spheres.p; p.shapes.boxes = sc.boxes.p; p.shapes.tris = sc.tris.p;
	p.shapes.tri_normals = nullptr; p.shapes.tri_uvs = nullptr;
	p.shapes.textures = nullptr; p.shapes.texels = nullptr; p.shapes.srgb_lut = nullptr;
	p.shapes.bvh = sc.bvh.p; p.shapes.n_bvh_nodes = sc.n_bvh_nodes;
	p.shapes.n_quads = sc.n_quads; p.shapes.n_spheres = sc.n_spheres; p.shapes.n_boxes = sc.n_boxes;
	p.n = n; p.o = d_origin; p.d = d_dir; p.tmax = d_tmax; p.t = d_t; p.uv = d_uv; p.prim = d_prim;
	// the probe's own overflow strips, for this call only
	DevBuf<uint2> ovf;
	PG_HIP(ctx, ovf.ensure((size_t)n * kOvfStack));
	p.ovf = ovf.p;
	const dim3 grid((unsigned)((n + kRBlock - 1) / kRBlock));
	const hipStream_t s = (hipStream_t)stream;
	switch (sc.general) {
	case 0: launch_any<0>(any_hit != 0, walk_form, grid, s, p); break;
	case 1: launch_any<1>(any_hit != 0, walk_form, grid, s, p); break;
	case 2: launch_any<2>(any_hit != 0, walk_form, grid, s, p); break;
	default: launch_any<3>(any_hit != 0, walk_form, grid, s, p); break;
	}
	PG_HIP(ctx, hipGetLastError());
	PG_HIP(ctx, hipStreamSynchronize(s)); // (the strips are freed on return)
	return PG_OK;
}
