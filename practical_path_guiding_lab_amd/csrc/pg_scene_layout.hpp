// pg_scene_layout.hpp -- the layout of the scene tables of pg_scene_desc (include/pgsd.h), written once: the strides, the
// columns of a row of each table, the codes a column can hold, the words of a BVH reference.  pg_scene.hip checks and packs the
// tables through these names, the kernels (pg_render_dev.hpp, pg_render_wave.hip) read them through the same ones; the Python
// packers (scene.py, mesh.py) are held to the strides by tests/test_scene_layout.py.  Plain constants, host and device.
// (oracle/ keeps its own PGO_* constants on purpose: the checker shares no header with what it checks.)
#pragma once

#include <stdint.h>

#include "../../include/pgsd.h"

namespace pg {

// ---- strides (32-bit words of a row) ----
constexpr int kQuadStride = PG_QUAD_STRIDE;
constexpr int kSphereStride = PG_SPHERE_STRIDE;
constexpr int kMaterialStride = PG_MATERIAL_STRIDE;
constexpr int kTextureStride = PG_TEXTURE_STRIDE;
constexpr int kBoxStride = PG_BOX_STRIDE;
constexpr int kTriStride = PG_TRI_STRIDE;
constexpr int kBvhStride = PG_BVH_STRIDE;
constexpr int kDirLightStride = PG_DIRLIGHT_STRIDE;
constexpr int kTriNormalStride = 9; // pg_scene_desc::tri_normals: three unit vertex normals per triangle
constexpr int kTriUvStride = 6;     // pg_scene_desc::tri_uvs: uv0 uv1 uv2 per triangle

// ---- quad (parallelogram), floats ----
enum : int {
	QUAD_ORIGIN = 0,    // 0-2
	QUAD_E1 = 3,        // 3-5 first edge
	QUAD_E2 = 6,        // 6-8 second edge
	QUAD_NORMAL = 9,    // 9-11 unit normal (normalised e1 x e2)
	QUAD_INV_E1_2 = 12, // 1 / |e1|^2
	QUAD_INV_E2_2 = 13, // 1 / |e2|^2
	QUAD_AREA = 14,
	QUAD_EMITTER = 15,  // != 0: an area emitter
	QUAD_REFL = 16,     // 16-18 diffuse reflectance (the level-0 kernels read it here: pg_scene_set_ex mirrors the material's)
	QUAD_RADIANCE = 19, // 19-21 emitted radiance
	QUAD_MATERIAL = 22, // row of the material table
};

// ---- sphere, floats ----
enum : int {
	SPH_CENTRE = 0,   // 0-2
	SPH_RADIUS = 3,
	SPH_MATERIAL = 4,
	SPH_EMITTER = 5,  // != 0: an area emitter
	SPH_RADIANCE = 6, // 6-8
};

// ---- material, floats ----
enum : int {
	MAT_TYPE = 0,      // a MaterialType
	MAT_REFL = 1,      // 1-3 reflectance | specular_reflectance
	MAT_ALPHA = 4,     // > 0: Beckmann, < 0: GGX of roughness -alpha
	MAT_ETA = 5,       // 5-7 (dielectrics: word 5 = int_ior / ext_ior)
	MAT_K = 8,         // 8-10
	MAT_ONE_SIDED = 11, // != 0: not wrapped in `twosided`
	MAT_TEXTURE = 12,  // texture index + 1, 0: none
};
enum MaterialType : int { MAT_DIFFUSE = 0, MAT_ROUGH_CONDUCTOR = 1, MAT_CONDUCTOR = 2, MAT_DIELECTRIC = 3, MAT_ROUGH_DIELECTRIC = 4 };

// ---- texture descriptor, 32-bit words (floats as bit patterns); texture_eval loads it as 16-byte groups ----
enum : int {
	TEX_KIND = 0,     // a TextureKind
	TEX_WIDTH = 1,
	TEX_HEIGHT = 2,
	TEX_FIRST = 3,    // index of the first texel in pg_scene_desc::texels
	TEX_COLOR0 = 4,   // 4-6 checkerboard
	TEX_COLOR1 = 7,   // 7-9
	TEX_UV_SCALE = 10, // 10-11 to_uv
	TEX_UV_OFFSET = 12, // 12-13
};
enum TextureKind : uint32_t { TEX_BITMAP = 1u, TEX_CHECKERBOARD = 2u };

// ---- box ([-1, 1]^3 under an affine to_world), floats ----
enum : int {
	BOX_INV_ROWS = 0, // 0-8 rows of A = (linear part of to_world)^-1
	BOX_CENTRE = 9,   // 9-11 (local = A (p - c))
	BOX_NORMALS = 12, // 12-20 outward unit normals of the +x, +y, +z faces
	BOX_MATERIAL = 21,
	BOX_CHECKED = 21, // words [0, BOX_CHECKED) must be finite
};

// ---- triangle, floats ----
enum : int {
	TRI_V0 = 0,
	TRI_E1 = 3,     // v1 - v0
	TRI_E2 = 6,     // v2 - v0
	TRI_NORMAL = 9, // unit geometric normal
	TRI_MATERIAL = 12,
};

// ---- node of the four-wide BVH, 32-bit words: six rows of four child planes, then the four children ----
enum : int {
	BVH_BOXES = 0,   // 0-23 (f32) lo_x[4] lo_y[4] lo_z[4] hi_x[4] hi_y[4] hi_z[4]
	BVH_BOX_ROWS = 6,
	BVH_HI_ROW = 3,  // rows [0, 3) hold the low planes, [3, 6) the high ones
	BVH_REFS = 24,   // 24-27 (u32) the children: a node, a leaf, or kBvhNone
	BVH_WIDTH = 4,
};
constexpr uint32_t kBvhNone = 0xffffffffu;          // no child
constexpr uint32_t kBvhLeafBit = 0x80000000u;       // the reference names triangles, not a node:
constexpr int kBvhCountShift = 28;                  //   (count - 1) of them in bits 28-30 ...
constexpr uint32_t kBvhCountMask = 7u;
constexpr uint32_t kBvhFirstMask = 0x0fffffffu;     //   ... from this one on
constexpr uint32_t kBvhNodeBytes = (uint32_t)kBvhStride * 4u;
constexpr uint32_t kBvhRowBytes = (uint32_t)BVH_WIDTH * 4u; // a row of child planes = one 16-byte group
constexpr uint32_t kBvhRefsByte = (uint32_t)BVH_REFS * 4u;
constexpr int kBvhMaxWaiting = 32;                  // siblings a root-to-node path may leave waiting on the walk's stack (checked)
constexpr int kBvhNodeQuads = kBvhStride / 4;       // 16-byte groups of a node (the copy of the top nodes in LDS)
constexpr uint32_t bvh_leaf_first(uint32_t ref) { return ref & kBvhFirstMask; }
constexpr uint32_t bvh_leaf_count(uint32_t ref) { return ((ref >> kBvhCountShift) & kBvhCountMask) + 1u; }

// ---- directional light, floats ----
enum : int {
	DL_DIRECTION = 0,  // 0-2 unit direction the light travels in
	DL_IRRADIANCE = 3, // 3-5
};

} // namespace pg
