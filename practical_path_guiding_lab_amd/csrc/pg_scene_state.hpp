// pg_scene_state.hpp -- the scene a context renders, as the library keeps it: the device copies of pg_scene_desc's tables
// (pg_scene_layout.hpp), their counts, the feature level of the kernels, the camera.  pg_scene.hip writes it (pg_scene_set_ex),
// pg_render.hip owns it (the first block of its renderer state) and hands it to the kernels (pass_args).
#pragma once

#include "pg_context.hpp"

namespace pg {

struct SceneState {
	DevBuf<float> quads, spheres, mats, boxes, tris, dir_lights, tri_normals, tri_uvs, srgb_lut;
	DevBuf<uint32_t> textures, texels, bvh;
	DevBuf<int32_t> emitters;
	// Everything below is assigned together, behind the last upload of a pg_scene_set_ex that went through; have_scene is false
	// from the first device call of an attempt on, so a failed one leaves a context WITHOUT a scene ("call pg_scene_set first"),
	// never one whose counts speak of tables that are gone.
	bool have_scene = false;
	bool have_tri_normals = false, have_tri_uvs = false;
	float bsphere[4] = {0, 0, 0, 0};
	int n_quads = 0, n_spheres = 0, n_emitters = 0, n_boxes = 0, n_bvh_nodes = 0;
	uint64_t n_tris = 0; // (host-side checks only: the kernels find triangles through the BVH)
	int general = 0; // feature level of the kernels to launch (0 cornell-box class, 1 veach-mis class, 2 meshes, 3 everything)
	bool geometry = false; // pg_render_record_geometry was on when the scene was set: recording passes keep the vertices' geometry
	pg_camera cam;
};

// pg_render.hip: the scene of the context's renderer state (made on first use), and its pg_render_split_pipeline and
// pg_render_record_geometry switches
SceneState &scene_state(pg_context *ctx);
bool split_pipeline_always(pg_context *ctx);
bool record_geometry_wanted(pg_context *ctx);
// ... and the one place that fills the kernels' view of its shapes (Shapes: pg_render_dev.hpp).  shading_tables false: what
// a kernel that only casts rays or samples emitters reads -- vertex normals, uvs, textures, texels and the sRGB table are null
struct Shapes;
Shapes scene_shapes(const SceneState &sc, bool shading_tables);

// pg_scene.hip: the checks pg_scene_set_ex applies to the rows of a material table (host memory, n_mats rows of
// kMaterialStride floats; n_tex: the textures a row may name) -- the bare reason of the first one a row fails
// ("unknown material type": the caller puts its own name in front), or nullptr
const char *check_material_rows(const float *mats, uint64_t n_mats, uint64_t n_tex);

} // namespace pg
