// pg_scene.hip -- pg_scene_set / pg_scene_set_ex (include/pgsd.h): a scene description becomes the context's scene in three
// stages.  check_and_pack: host code only -- every check of the description, and the host copies the library changes before
// they travel (pg_scene_layout.hpp names the columns).  upload: the one stage that touches the device.  Commit: counts, feature
// level and camera, assigned together behind the last upload (SceneState, pg_scene_state.hpp).
#include <math.h>

#include "pg_scene_layout.hpp"
#include "pg_scene_state.hpp"

namespace pg {
namespace {

// what check_and_pack makes of a description; the tables it leaves alone are uploaded from the caller's arrays
struct PackedScene {
	std::vector<float> quads;      // material indices made up where there is no table, diffuse reflectances mirrored in
	std::vector<float> mats;       // the material table, made up (quad i: diffuse QUAD_REFL) when absent
	std::vector<uint32_t> bvh;     // the boxes of absent children replaced by boxes no ray reaches
	std::vector<int32_t> emitters; // shape numbers of flagged quads, then flagged spheres, then -1-k for directional light k
	bool tri_normals = false, tri_uvs = false;
	int general = 0;               // feature level of the kernels (see intersect()): decided by the materials the shapes USE
	std::string error;             // the text of a refusal that is put together here (the others are literals)
};

// a finite float that is a whole number in [0, n): how the tables name a row of another table
bool is_index(float v, uint64_t n) { return v >= 0.0f && v < (float)n && v == (float)(uint64_t)v; }

// The tree the kernels walk with a fixed-size stack and trust: children follow their parent (no cycles, one parent each),
// leaves stay inside the triangle array, and no walk can have more than kBvhMaxWaiting siblings waiting on its stack.
// `nodes` is the copy that travels: an absent child gets a box no ray reaches, (+inf, -inf) on every axis, whatever the caller
// left there -- the walk then needs no test of the reference (bvh_node_step).
const char *check_bvh(std::vector<uint32_t> &nodes, uint64_t nn, uint64_t nt)
{
	std::vector<uint8_t> waiting(nn, 0); // siblings on the stack when the walk opens node i, at most
	std::vector<uint8_t> seen(nn, 0);
	seen[0] = 1;
	for (uint64_t i = 0; i < nn; ++i) {
		if (!seen[i]) return "pg_scene_set: BVH node without a parent";
		uint32_t *N = &nodes[i * kBvhStride];
		int kids = 0;
		for (int c = 0; c < BVH_WIDTH; ++c) kids += N[BVH_REFS + c] != kBvhNone;
		if (kids == 0) return "pg_scene_set: BVH node without children";
		const int below = (int)waiting[i] + kids - 1; // its other children wait while the walk is in one of them
		if (below > kBvhMaxWaiting) return "pg_scene_set: BVH too deep for the walk's stack (32 waiting siblings)";
		for (int c = 0; c < BVH_WIDTH; ++c) {
			const uint32_t ref = N[BVH_REFS + c];
			if (ref == kBvhNone) {
				for (int row = 0; row < BVH_BOX_ROWS; ++row)
					N[BVH_BOXES + row * BVH_WIDTH + c] = row < BVH_HI_ROW ? 0x7f800000u : 0xff800000u;
			} else if (ref & kBvhLeafBit) {
				if ((uint64_t)bvh_leaf_first(ref) + bvh_leaf_count(ref) > nt) return "pg_scene_set: BVH leaf outside the triangle array";
			} else {
				if (ref <= i || ref >= nn) return "pg_scene_set: BVH children must follow their parent";
				if (seen[ref]) return "pg_scene_set: BVH node with two parents";
				seen[ref] = 1;
				waiting[ref] = (uint8_t)below;
			}
		}
	}
	return nullptr;
}

// Stage 1, host code only: the error text of the first check the description fails, or nullptr and the packed scene.
const char *check_and_pack(const pg_scene_desc &sc, const pg_camera &cam, PackedScene &out)
{
	const uint64_t nq = sc.n_quads, ns = sc.n_spheres, nm = sc.n_materials, nb = sc.n_boxes;
	if (nq + ns + nb + sc.n_tris == 0 || nq > 4096 || ns > 4096 || nb > 4096 || (nq && !sc.quads) || (ns && !sc.spheres) || (nb && !sc.boxes))
		return "pg_scene_set: need 1..4096 quads, spheres and/or boxes";
	if ((nm && !sc.materials) || (!sc.materials && (ns || nb))) return "pg_scene_set: spheres and boxes need a material table";
	if (cam.width <= 0 || cam.height <= 0) return "pg_scene_set: bad film size";
	std::vector<float> &quads = out.quads, &mats = out.mats;
	quads.assign(sc.quads, sc.quads + nq * kQuadStride);
	if (sc.materials) {
		mats.assign(sc.materials, sc.materials + nm * kMaterialStride);
	} else {
		mats.assign(nq * kMaterialStride, 0.0f);
		for (uint64_t q = 0; q < nq; ++q) {
			for (int c = 0; c < 3; ++c) mats[q * kMaterialStride + MAT_REFL + c] = quads[q * kQuadStride + QUAD_REFL + c];
			quads[q * kQuadStride + QUAD_MATERIAL] = (float)q;
		}
	}
	const uint64_t n_mats = mats.size() / kMaterialStride;
	const uint64_t n_tex = sc.n_textures;
	if (n_tex > 65536 || (n_tex && (!sc.textures || !sc.srgb_lut))) return "pg_scene_set: textures need their table and the sRGB lookup table";
	for (uint64_t t = 0; t < n_tex; ++t) { // a texture's texels must lie inside the texel array
		const uint32_t *T = sc.textures + t * kTextureStride;
		const uint32_t w = T[TEX_WIDTH], h = T[TEX_HEIGHT];
		if (T[TEX_KIND] == TEX_BITMAP) {
			if (w == 0u || h == 0u || w > 65536u || h > 65536u || !sc.texels || (uint64_t)T[TEX_FIRST] + (uint64_t)w * h > sc.n_texels)
				return "pg_scene_set: bitmap texture outside the texel array";
		} else if (T[TEX_KIND] != TEX_CHECKERBOARD) return "pg_scene_set: unknown texture kind";
	}
	if (const char *why = check_material_rows(mats.data(), n_mats, n_tex)) return (out.error = std::string("pg_scene_set: ") + why).c_str();
	int general = ns > 0 ? 1 : 0;
	// the material row a shape names: false when it names none; raises the feature level to what the material needs
	auto use_material = [&](float mi) {
		if (!is_index(mi, n_mats)) return false;
		const float *M = &mats[(uint64_t)mi * kMaterialStride];
		if (M[MAT_TYPE] == (float)MAT_ROUGH_CONDUCTOR && general < 1) general = 1;
		if (M[MAT_TYPE] >= (float)MAT_CONDUCTOR || M[MAT_ONE_SIDED] != 0.0f) general = 3; // transmission, delta lobes, one-sided BSDFs
		return true;
	};
	const uint64_t nd = sc.n_dir_lights;
	if (nd > 64 || (nd && !sc.dir_lights)) return "pg_scene_set: at most 64 directional lights";
	if (nd && !(sc.bsphere[3] > 0.0f)) return "pg_scene_set: directional lights need the scene's bounding sphere";
	if (nd) general = 3;
	for (uint64_t q = 0; q < nq; ++q) {
		float *Q = &quads[q * kQuadStride];
		if (!use_material(Q[QUAD_MATERIAL])) return "pg_scene_set: quad material index out of range";
		const float *M = &mats[(uint64_t)Q[QUAD_MATERIAL] * kMaterialStride];
		if (M[MAT_TYPE] == (float)MAT_DIFFUSE) // (the quad-only kernels read the reflectance in the quad)
			for (int c = 0; c < 3; ++c) Q[QUAD_REFL + c] = M[MAT_REFL + c];
	}
	for (uint64_t s = 0; s < ns; ++s) {
		const float *S = sc.spheres + s * kSphereStride;
		if (!use_material(S[SPH_MATERIAL])) return "pg_scene_set: sphere material index out of range";
		if (!(S[SPH_RADIUS] > 0.0f)) return "pg_scene_set: sphere radius must be > 0";
	}
	for (uint64_t b = 0; b < nb; ++b) {
		const float *B = sc.boxes + b * kBoxStride;
		if (!use_material(B[BOX_MATERIAL])) return "pg_scene_set: box material index out of range";
		for (int k = 0; k < BOX_CHECKED; ++k)
			if (!(B[k] == B[k]) || fabsf(B[k]) > 3.0e38f) return "pg_scene_set: box transform is not finite";
	}
	const uint64_t nt = sc.n_tris, nn = sc.n_bvh_nodes;
	// (a leaf names its first triangle in kBvhFirstMask's bits; the walk addresses a node by a 32-bit byte offset: 2^25 nodes of 128 bytes)
	if ((nt == 0) != (nn == 0) || (nt && (!sc.tris || !sc.bvh)) || nt > kBvhFirstMask || nn > (1ull << 32) / kBvhNodeBytes)
		return "pg_scene_set: triangles and BVH nodes go together";
	if (nt && !sc.materials) return "pg_scene_set: meshes need a material table";
	if (nn) {
		out.bvh.assign(sc.bvh, sc.bvh + nn * kBvhStride);
		if (const char *err = check_bvh(out.bvh, nn, nt)) return err;
		for (uint64_t t = 0; t < nt; ++t)
			if (!use_material(sc.tris[t * kTriStride + TRI_MATERIAL])) return "pg_scene_set: triangle material index out of range";
		if (general < 2) general = 2;
	}
	out.general = general;
	out.tri_normals = nt && sc.tri_normals;
	// (a textured material on anything but a triangle with texture coordinates keeps its plain colour)
	out.tri_uvs = nt && sc.tri_uvs && n_tex;
	for (uint64_t q = 0; q < nq; ++q)
		if (quads[q * kQuadStride + QUAD_EMITTER] != 0.0f) out.emitters.push_back((int32_t)q);
	for (uint64_t s = 0; s < ns; ++s)
		if (sc.spheres[s * kSphereStride + SPH_EMITTER] != 0.0f) out.emitters.push_back((int32_t)(nq + s));
	for (uint64_t k = 0; k < nd; ++k) out.emitters.push_back(-1 - (int32_t)k);
	return nullptr;
}

// Stage 2: the tables of a checked description into the scene's device buffers (which grow as they must; a table the scene
// does not have keeps whatever buffer an earlier scene left)
int upload_tables(pg_context *ctx, SceneState &s, const pg_scene_desc &sc, const PackedScene &h)
{
	PG_HIP(ctx, hipSetDevice(ctx->device));
	PG_HIP(ctx, upload(s.dir_lights, sc.dir_lights, sc.n_dir_lights * kDirLightStride));
	PG_HIP(ctx, upload(s.quads, h.quads));
	PG_HIP(ctx, upload(s.spheres, sc.spheres, sc.n_spheres * kSphereStride));
	PG_HIP(ctx, upload(s.mats, h.mats));
	PG_HIP(ctx, upload(s.emitters, h.emitters));
	PG_HIP(ctx, upload(s.boxes, sc.boxes, sc.n_boxes * kBoxStride));
	PG_HIP(ctx, upload(s.tris, sc.tris, sc.n_tris * kTriStride));
	PG_HIP(ctx, upload(s.bvh, h.bvh));
	if (h.tri_normals) PG_HIP(ctx, upload(s.tri_normals, sc.tri_normals, sc.n_tris * kTriNormalStride));
	if (h.tri_uvs) {
		PG_HIP(ctx, upload(s.tri_uvs, sc.tri_uvs, sc.n_tris * kTriUvStride));
		PG_HIP(ctx, upload(s.textures, sc.textures, sc.n_textures * kTextureStride));
		PG_HIP(ctx, upload(s.texels, sc.texels, sc.n_texels));
		PG_HIP(ctx, upload(s.srgb_lut, sc.srgb_lut, 256));
	}
	return PG_OK;
}

} // namespace

// What a material row must satisfy before a kernel reads it (pg_scene_state.hpp): a known type, a microfacet alpha the
// distributions can divide by, a positive index ratio, a texture the scene has (index + 1; 0: none).
const char *check_material_rows(const float *mats, uint64_t n_mats, uint64_t n_tex)
{
	for (uint64_t m = 0; m < n_mats; ++m) {
		const float *M = &mats[m * kMaterialStride];
		const float type = M[MAT_TYPE];
		if (!is_index(type, MAT_ROUGH_DIELECTRIC + 1)) return "unknown material type";
		const bool rough = type == (float)MAT_ROUGH_CONDUCTOR || type == (float)MAT_ROUGH_DIELECTRIC;
		if (rough && !(fabsf(M[MAT_ALPHA]) > 0.0f && fabsf(M[MAT_ALPHA]) < 3.0e38f)) return "microfacet alpha must be finite and not 0";
		if ((type == (float)MAT_DIELECTRIC || type == (float)MAT_ROUGH_DIELECTRIC) && !(M[MAT_ETA] > 0.0f))
			return "dielectric index ratio must be > 0";
		if (!is_index(M[MAT_TEXTURE], n_tex + 1)) return "material texture index out of range"; // (index + 1; 0: none)
	}
	return nullptr;
}

} // namespace pg

using namespace pg;

extern "C" {

int pg_scene_set(pg_context *ctx, uint64_t n_quads, const float *h_quads, const pg_camera *cam)
{
	pg_scene_desc d = {};
	d.n_quads = n_quads; d.quads = h_quads;
	return pg_scene_set_ex(ctx, &d, cam);
}

int pg_scene_set_ex(pg_context *ctx, const pg_scene_desc *sc, const pg_camera *cam)
{
	if (!ctx) return PG_ERR_INVALID;
	if (!sc || !cam) return fail(ctx, PG_ERR_INVALID, "pg_scene_set: NULL pointer");
	PackedScene h;
	if (const char *err = check_and_pack(*sc, *cam, h)) return fail(ctx, PG_ERR_INVALID, err); // (the scene the context has stays)
	SceneState &s = scene_state(ctx);
	s.have_scene = false;
	const int rc = upload_tables(ctx, s, *sc, h);
	if (rc != PG_OK) return rc;
	// Stage 3, the commit
	s.n_quads = (int)sc->n_quads; s.n_spheres = (int)sc->n_spheres; s.n_boxes = (int)sc->n_boxes;
	s.n_bvh_nodes = (int)sc->n_bvh_nodes; s.n_emitters = (int)h.emitters.size(); s.n_tris = sc->n_tris;
	s.have_tri_normals = h.tri_normals; s.have_tri_uvs = h.tri_uvs;
	for (int c = 0; c < 4; ++c) s.bsphere[c] = sc->bsphere[c];
	s.geometry = record_geometry_wanted(ctx); // pg_render_record_geometry: implies the split pipeline
	s.general = (split_pipeline_always(ctx) || s.geometry) && h.general < 2 ? 2 : h.general; // pg_render_split_pipeline
	s.cam = *cam;
	s.have_scene = true;
	return PG_OK;
}

} // extern "C"
