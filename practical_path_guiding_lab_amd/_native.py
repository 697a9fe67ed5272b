"""ctypes binding of libpgsd.so (include/pgsd.h).

The library is the product: if it is missing, cannot be loaded, or finds no gfx950 device, this
module raises.  There is deliberately no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
# PGSD_LIBRARY: another build of the same library (tools/build_variant.sh), for A/B measurements
LIB_PATH = os.environ.get("PGSD_LIBRARY") or os.path.join(_PKG, "libpgsd.so")
CSRC = os.path.join(_PKG, "csrc")

PG_OK = 0
PG_ACC_LIMBS = 3
PG_FRAC_BITS = 40
PG_SPATIAL_NEAREST, PG_SPATIAL_STOCHASTIC_BOX = 0, 1
PG_SPATIAL_OVERLAP_BOX = 3  # (2 is not assigned)
PG_DIRECTIONAL_NEAREST, PG_DIRECTIONAL_BOX = 0, 1


class PgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libpgsd error {code}: {msg}")
        self.code = code


class pg_records(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "position", "direction", "radiance", "wo_pdf", "direction_nee", "radiance_nee_lum")]


class pg_dense_records(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "active", "position", "direction", "bsdf", "throughput_bsdf", "throughput_radiance",
        "radiance_nee", "direction_nee", "wo_pdf")]


class pg_records_out(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "position", "direction", "radiance", "wo_pdf", "direction_nee", "radiance_nee_lum")]


class pg_fraction_params(C.Structure):  # include/pgsd_fraction.h
    _fields_ = [("theta0", C.c_float), ("learning_rate", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("epsilon", C.c_float), ("l2", C.c_float), ("loss", C.c_int32)]


class pg_fraction_records(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("position", "bsdf_pdf", "guide_pdf", "product", "wo_pdf", "is_delta")]


class pg_rr_params(C.Structure):  # include/pgsd_radiance.h
    _fields_ = [("window", C.c_float), ("max_split", C.c_uint32)]


class pg_bounce_args(C.Structure):  # include/pgsd_bounce.h
    _fields_ = [(n, C.c_void_p) for n in (
        "p", "dir_nee", "nee_active", "mode", "u_select", "u", "rng_state", "rng_inc", "lane_index", "d_lane_count",
        "dir_io", "select_out", "fraction_out", "pdf_nee_out", "pdf_out", "L_dir_out", "L_mean_out")]


class pg_resample_params(C.Structure):  # include/pg_resample.h
    _fields_ = [("candidates", C.c_uint32), ("alpha", C.c_float), ("delta", C.c_float), ("reserved", C.c_uint32)]


class pg_resample_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "p", "normal", "active", "rng_state", "rng_inc", "dir_out", "weight_out", "target_out", "source_out", "index_out",
        "cand_dir_out", "cand_target_out", "cand_source_out")]


class pg_resample_lobe_args(C.Structure):  # include/ext/guiding/pg_resample_lobe.h
    _fields_ = [(n, C.c_void_p) for n in (
        "p", "normal", "wi", "roughness", "specular", "active", "rng_state", "rng_inc", "dir_out", "weight_out", "target_out",
        "source_out", "index_out", "cand_dir_out", "cand_target_out", "cand_source_out")]


class pg_resample_interface_args(C.Structure):  # include/ext/guiding/pg_resample_interface.h
    _fields_ = [(n, C.c_void_p) for n in (
        "p", "normal", "wi", "roughness", "eta", "active", "rng_state", "rng_inc", "dir_out", "weight_out", "target_out",
        "source_out", "index_out", "eta_out", "cand_dir_out", "cand_target_out", "cand_source_out")]


class pg_lights_params(C.Structure):  # include/ext/pg_lights.h
    _fields_ = [("delta", C.c_float), ("root", C.c_uint32), ("reserved", C.c_uint32)]


class pg_lights_records(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("position", "light", "value")]


class pg_nee_params(C.Structure):  # include/ext/lights/pg_nee.h
    _fields_ = [("candidates", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class pg_nee_args(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "p", "normal", "active", "rng_state", "rng_inc", "light_out", "point_out", "weight_out", "dir_out", "dist_out", "target_out",
        "source_out", "index_out", "cand_light_out", "cand_point_out", "cand_target_out", "cand_source_out")]


class pg_vertex_lanes(C.Structure):  # include/pgsd.h: the columns of pg_vertex_probe, device pointers
    _fields_ = [(n, C.c_void_p) for n in (
        "thr", "L", "ior", "depth", "flags", "Le", "p", "n", "ng", "wi", "refl", "mat", "em_w", "bv_em", "bp_em", "ds_pdf",
        "bsdf_w", "bsdf_pdf", "eta", "wo", "pdf_nee", "pdf_tree", "occluded", "rng_state", "rng_inc")]


class pg_vertex_out(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "go", "thr", "L", "ior", "ray_o", "ray_d", "prev_pdf", "delta", "rng_state", "ray_of", "r_bsdf", "r_tb", "r_tr", "r_nee",
        "r_wp")]


class pg_head_lanes(C.Structure):  # include/pgsd.h: the columns of pg_head_probe, device pointers
    _fields_ = [(n, C.c_void_p) for n in (
        "ray_o", "ray_d", "thr", "prev_p", "prev_bsdf_pdf", "prev_delta", "prim", "t", "uv", "depth", "rng_state", "rng_inc")]


class pg_head_out(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "p", "n", "ng", "wi", "refl", "Le", "ds_d", "em_w", "bv_em", "sh_o", "sh_d", "wo", "bsdf_w", "ds_pdf", "bp_em", "sh_tmax",
        "bsdf_pdf", "eta", "mat", "flags", "rng_state")]


class pg_tree_sizes(C.Structure):
    _fields_ = [("n_kd", C.c_uint64), ("n_quad", C.c_uint64), ("n_roots", C.c_uint64)]


class pg_tree_columns(C.Structure):
    _fields_ = [
        ("kd_max_leaf_size", C.c_double),
        ("kd_max_depth", C.c_int32), ("quad_max_depth", C.c_int32), ("quad_store_nee", C.c_int32),
        ("kd_bbox_min", C.c_void_p), ("kd_bbox_max", C.c_void_p), ("kd_depth", C.c_void_p),
        ("kd_vert_count", C.c_void_p), ("kd_is_leaf", C.c_void_p), ("kd_quad_root_index", C.c_void_p),
        ("kd_child_left", C.c_void_p), ("kd_child_right", C.c_void_p),
        ("quad_root_node_index", C.c_void_p), ("quad_bbox_min", C.c_void_p), ("quad_bbox_max", C.c_void_p),
        ("quad_depth", C.c_void_p), ("quad_irradiance", C.c_void_p), ("quad_is_leaf", C.c_void_p),
        ("quad_threshold", C.c_void_p), ("quad_child", C.c_void_p * 4),
    ]


class pg_stats(C.Structure):
    _fields_ = [
        ("n_kd_nodes", C.c_uint64), ("n_kd_leaves", C.c_uint64), ("n_quad_records", C.c_uint64),
        ("n_quad_nodes", C.c_uint64), ("n_trees", C.c_uint64),
        ("mean_kd_leaf_depth", C.c_double), ("mean_quad_leaf_depth", C.c_double),
        ("max_kd_depth", C.c_uint32), ("max_quad_depth", C.c_uint32),
        ("bytes_kd", C.c_uint64), ("bytes_quad_records", C.c_uint64), ("bytes_accumulators", C.c_uint64),
        ("bytes_jump_tables", C.c_uint64), ("jump_bits", C.c_uint32), ("kd_grid_bits", C.c_uint32),
    ]


class pg_camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("axis_x", C.c_float * 3), ("axis_y", C.c_float * 3),
                ("axis_z", C.c_float * 3), ("tan_half_fov_x", C.c_float), ("width", C.c_int32), ("height", C.c_int32)]


class pg_scene_desc(C.Structure):
    _fields_ = [("n_quads", C.c_uint64), ("quads", C.c_void_p), ("n_spheres", C.c_uint64), ("spheres", C.c_void_p),
                ("n_materials", C.c_uint64), ("materials", C.c_void_p), ("n_boxes", C.c_uint64), ("boxes", C.c_void_p),
                ("n_tris", C.c_uint64), ("tris", C.c_void_p), ("n_bvh_nodes", C.c_uint64), ("bvh", C.c_void_p),
                ("n_dir_lights", C.c_uint64), ("dir_lights", C.c_void_p), ("bsphere", C.c_float * 4),
                ("tri_normals", C.c_void_p), ("tri_uvs", C.c_void_p), ("n_textures", C.c_uint64), ("textures", C.c_void_p),
                ("n_texels", C.c_uint64), ("texels", C.c_void_p), ("srgb_lut", C.c_void_p)]


class pg_pass_params(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("spp", C.c_int32), ("rr_depth", C.c_int32), ("slot", C.c_int32),
                ("pixel_begin", C.c_uint64), ("pixel_count", C.c_uint64),
                ("stripe_rows", C.c_uint32), ("stripe_index", C.c_uint32), ("stripe_count", C.c_uint32), ("batched", C.c_uint32)]


class pg_kernel_timing(C.Structure):
    _fields_ = [("bounce_ms", C.c_double), ("splat_ms", C.c_double), ("generate_ms", C.c_double),
                ("finish_ms", C.c_double), ("compact_ms", C.c_double), ("bounce_launches", C.c_uint64),
                ("splat_launches", C.c_uint64),
                ("passes", C.c_uint64),
                ("trace_ms", C.c_double), ("shade_ms", C.c_double), ("shadow_ms", C.c_double), ("guide_ms", C.c_double),
                ("tail_ms", C.c_double), ("trace_launches", C.c_uint64), ("guide_launches", C.c_uint64),
                ("shade_a_ms", C.c_double), ("shade_b_ms", C.c_double), ("sort_ms", C.c_double)]


class pg_depth_counters(C.Structure):
    _fields_ = [("kd_levels", C.c_uint64), ("kd_queries", C.c_uint64),
                ("quad_levels", C.c_uint64), ("quad_queries", C.c_uint64), ("layout_bytes", C.c_uint64)]


ABI_VERSION = 6  # PGSD_ABI_VERSION of include/pgsd.h these bindings match
PG_FRACTION_LOSS_KL, PG_FRACTION_LOSS_VARIANCE = 0, 1
PG_TARGET_SECOND_MOMENT = 1
PG_BOUNCE_NONE, PG_BOUNCE_PDF, PG_BOUNCE_SAMPLE, PG_BOUNCE_CHOOSE = 0, 1, 2, 3
PG_RESAMPLE_MAX_CANDIDATES, PG_RESAMPLE_NONE = 64, 0xFFFFFFFF
PG_LIGHTS_MAX, PG_LIGHTS_WEIGHT_ONE, PG_LIGHTS_NONE = 4096, 65536, 0xFFFFFFFF
PG_NEE_TABLE_WORDS = 12  # 32-bit words of pg_nee_set_lights' host table per light
PG_RESAMPLE_LOBE_MIN_ROUGHNESS = 1e-3  # (the header's 1e-3f: the float32 nearest to it)
PG_RESAMPLE_INTERFACE_MIN_ROUGHNESS = 1e-3  # (likewise)
PG_RESAMPLE_INTERFACE_MIN_ETA, PG_RESAMPLE_INTERFACE_MAX_ETA = 0.25, 4.0

V, U64, I32, U32, F32, P = C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_float, C.POINTER
_RR = [V, U64, V, V, V, V, P(pg_rr_params), V, V, V, V, V, V, V]  # pg_radiance_rr and pg_irradiance_rr
_FILM = [V, I32, U32, I32, V, V, U32, U32, U32, V]  # pg_film_stripes and pg_film_batched

# The public surface, declared once: header of include/ -> entry point -> argtypes, in the order of the headers and of their
# EXPORTS* tuples below.  lib() binds from it, source_hash() takes its headers from it, tests/test_abi.py holds every header, the
# library and the probe build to it.  restype is c_int unless RESTYPES says otherwise.
SURFACE = {
    "pgsd.h": {
        "pg_create": [P(V), C.c_int], "pg_destroy": [V], "pg_last_error": [V], "pg_abi_version": [],
        "pg_setup": [V, V, V, U64, I32, I32, I32, I32, F32], "pg_set_iteration": [V, I32, I32],
        "pg_get_leaf_node_index": [V, U64, V, V, V, V], "pg_sample": [V, U64, V, V, V, V, V, V, V],
        "pg_pdf": [V, U64, V, V, V, V, V], "pg_guide_bounce": [V, U64, V, V, V, V, V, V, V, V, V, V, V, V],
        "pg_compact_lanes": [V, U64, V, V, V, V, V], "pg_rng_seed": [V, U64, U32, U32, V, V, V],
        "pg_splat": [V, U64, P(pg_records), V, V],
        "pg_process_records": [V, U64, I32, V, P(pg_dense_records), P(pg_records_out), V, V],
        "pg_process_and_splat": [V, U64, I32, V, P(pg_dense_records), V], "pg_refine_and_swap": [V, V],
        "pg_accumulators": [V, P(V), P(U64)], "pg_export_sizes": [V, P(pg_tree_sizes)],
        "pg_export": [V, P(pg_tree_sizes), P(pg_tree_columns)], "pg_import": [V, P(pg_tree_sizes), P(pg_tree_columns)],
        "pg_export_accumulators": [V, P(pg_tree_sizes), V, V, V], "pg_get_stats": [V, P(pg_stats)],
        "pg_enable_depth_counters": [V, I32], "pg_read_depth_counters": [V, P(pg_depth_counters), I32],
        "pg_scene_set": [V, U64, V, P(pg_camera)], "pg_render_pass": [V, P(pg_pass_params), V, V, V, V, V],
        "pg_enable_kernel_timing": [V, I32], "pg_read_kernel_timing": [V, P(pg_kernel_timing), I32],
        "pg_render_live_counts": [V, P(U32), I32], "pg_film_tent": [V, U32, I32, V, V, V],
        "pg_math_eval": [V, I32, U64, V, V, V], "pg_scene_set_ex": [V, P(pg_scene_desc), P(pg_camera)],
        "pg_film": [V, I32, U32, I32, V, V, V], "pg_film_stripes": _FILM, "pg_film_batched": _FILM,
        "pg_film_batched_accumulate": [V, I32, U32, I32, V, V, F32, I32, U32, U32, U32, V],
        "pg_render_overlap": [V, I32], "pg_render_sort": [V, I32], "pg_render_stages": [V, I32],
        "pg_comm_unique_id": [V, V], "pg_comm_init": [V, I32, I32, V], "pg_comm_attach": [V, V, I32], "pg_comm_destroy": [V],
        "pg_allreduce": [V, V], "pg_render_reserve": [V, U64], "pg_render_split_pipeline": [V, I32],
        "pg_comm_info": [V, P(I32), P(I32)], "pg_exchange_pack": [V, P(V), P(U64), V], "pg_exchange_unpack": [V, V],
        "pg_exchange_pack_words": [V, U64, V], "pg_exchange_unpack_words": [V, U64, V], "pg_sort_places": [V, U64, V, V, V, V],
        "pg_debug_fail_alloc": [C.c_int64], "pg_debug_fail_alloc_pending": [],
        "pg_read_shade_phases": [V, P(U64), I32], "pg_set_splat_filter": [V, I32, I32, U32],
        "pg_render_record_geometry": [V, I32], "pg_render_export_records": [V, I32, P(pg_records_out), V, V, V],
        "pg_scene_intersect": [V, U64, V, V, V, I32, I32, V, V, V, V],
        "pg_bsdf_probe": [V, U64, U64, V, V, V, V, V, I32, V, V, V, V, V, V, V, V],
        "pg_surface_probe": [V, U64, V, V, V, V, V, V, V, V, V],
        "pg_emitter_probe": [V, U64, V, V, V, V, V, V],
        "pg_vertex_probe": [V, U64, U64, V, I32, P(pg_vertex_lanes), F32, I32, I32, I32, I32, P(pg_vertex_out), V],
        "pg_head_probe": [V, U64, P(pg_head_lanes), I32, F32, I32, P(pg_head_out), V],
    },
    "pgsd_warp.h": {  # sample warping: same library, same ABI version
        "pg_sample_warp": [V, U64, V, V, V, V, V, V], "pg_invert_warp": [V, U64, V, V, V, V, V, V],
        "pg_guide_bounce_warp": [V, U64, V, V, V, V, V, V, V, V, V, V, V],
    },
    "pgsd_fraction.h": {  # the BSDF sampling fraction learned per KD leaf
        "pg_fraction_enable": [V, P(pg_fraction_params)], "pg_fraction_query": [V, U64, V, V, V, V],
        "pg_fraction_record": [V, U64, P(pg_fraction_records), V, V], "pg_fraction_step": [V, V],
        "pg_fraction_accumulators": [V, P(V), P(U64)], "pg_fraction_export": [V, U64, V, V, V, V, V, V, V],
        "pg_fraction_import": [V, U64, V, V, V, V, V, V],
    },
    "pgsd_target.h": {  # the variance-aware guiding target: sqrt of the leaves' second moments
        "pg_target_apply": [V, I32, V], "pg_target_applied": [V, P(I32)],
    },
    "pgsd_radiance.h": {  # radiance estimates and guided Russian roulette / splitting
        "pg_radiance_enable": [V, I32], "pg_radiance_status": [V, P(I32), P(I32), P(I32)], "pg_radiance_export": [V, U64, V],
        "pg_radiance_import": [V, U64, V], "pg_radiance_query": [V, U64, V, V, V, V, V, V], "pg_radiance_rr": _RR,
    },
    "pgsd_bounce.h": {  # fraction, selection, guide bounce and radiance estimate behind one KD descent
        "pg_bounce": [V, U64, P(pg_bounce_args), V],
    },
    "pgsd_irradiance.h": {  # irradiance estimates per spatial leaf: order-2 spherical harmonics
        "pg_irradiance_build": [V, V], "pg_irradiance_status": [V, P(I32)], "pg_irradiance_export": [V, U64, V],
        "pg_irradiance_import": [V, U64, V], "pg_irradiance_query": [V, U64, V, V, V, V, V], "pg_irradiance_rr": _RR,
    },
}
RESTYPES = {"pg_last_error": C.c_char_p}  # (pg_abi_version returns the c_int of all the others: it only has no context to fail on)
EXPORTS, EXPORTS_WARP, EXPORTS_FRACTION, EXPORTS_TARGET, EXPORTS_RADIANCE, EXPORTS_BOUNCE, EXPORTS_IRRADIANCE = (
    tuple(entry_points) for entry_points in SURFACE.values())
# Entry points of the same library whose headers are not include/pgsd*.h: beside SURFACE, not in it, because the ABI tests pin
# SURFACE to that pattern and to its count.  lib() binds them after SURFACE, source_hash() hashes their headers
# after SURFACE's; their own test files hold them to the header and the two builds.
SURFACE_EXTRA = {
    "pg_resample.h": {  # product guiding for diffuse surfaces: resampled importance sampling of cosine and tree candidates
        "pg_resample_cosine": [V, U64, P(pg_resample_params), P(pg_resample_args), V],
    },
}
(EXPORTS_RESAMPLE,) = (tuple(entry_points) for entry_points in SURFACE_EXTRA.values())
# Entry points whose headers live in a subdirectory of include/, keyed by the header's path under include/: a third table, because
# the tests of SURFACE_EXTRA pin it to its one header and include/*.h to the headers there.  lib() binds it after
# the other two, source_hash() hashes its headers after theirs.
SURFACE_EXT = {
    "ext/pg_lights.h": {  # light selection for next-event estimation, learned per KD leaf
        "pg_lights_enable": [V, U32, P(pg_lights_params)], "pg_lights_record": [V, U64, P(pg_lights_records), V, V],
        "pg_lights_build": [V, V], "pg_lights_sample": [V, U64, V, V, V, V, V, V, V, V],
        "pg_lights_pmf": [V, U64, V, V, V, V, V], "pg_lights_accumulators": [V, P(V), P(U64)],
        "pg_lights_status": [V, P(U32), P(U64)], "pg_lights_export": [V, U64, U32, V, V],
        "pg_lights_import": [V, U64, U32, V],
    },
}
(EXPORTS_LIGHTS,) = (tuple(entry_points) for entry_points in SURFACE_EXT.values())
# Entry points of every LATER header, keyed by the header's path under include/ at ANY depth: a fourth table, because the tests of
# SURFACE_EXT pin it to its one header and include/*/*.h to that file, so this one's first header lies a directory deeper
# (DESIGN.md 5.24).  It is the LAST table: the next header JOINS it -- nothing pins it to one header, to one depth or its glob to
# one file, and its tests must not start to -- it does not get a fifth.  lib() binds it after the other three, source_hash()
# hashes its headers after theirs.
SURFACE_MORE = {
    "ext/guiding/pg_resample_lobe.h": {  # product guiding for glossy surfaces: resampling against a GGX reflection lobe
        "pg_resample_lobe": [V, U64, P(pg_resample_params), P(pg_resample_lobe_args), V],
    },
    "ext/guiding/pg_resample_interface.h": {  # product guiding through rough glass: the two-sided lobe of a rough dielectric
        "pg_resample_interface": [V, U64, P(pg_resample_params), P(pg_resample_interface_args), V],
    },
    "ext/lights/pg_nee.h": {  # resampled next-event estimation: a light and a point on it, from the learned rows and the geometry
        "pg_nee_set_lights": [V, U32, V, V], "pg_nee_status": [V, P(U32)],
        "pg_nee_resample": [V, U64, P(pg_nee_params), P(pg_nee_args), V],
    },
}
EXPORTS_MORE = tuple(name for entry_points in SURFACE_MORE.values() for name in entry_points)


def source_hash() -> str:
    """sha256 (16 hex digits) over the library's sources (csrc/*.hip, csrc/*.hpp, then the headers of SURFACE in its order, then
    those of SURFACE_EXTRA, then those of SURFACE_EXT, then those of SURFACE_MORE):
    names the code a profile was taken of (profiles/pmc_traffic.json) so that bench.py never pairs old counters with new kernels."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))
    files += [os.path.join(os.path.dirname(_PKG), "include", *header.split("/"))
              for header in list(SURFACE) + list(SURFACE_EXTRA) + list(SURFACE_EXT) + list(SURFACE_MORE)]
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def build(force: bool = False) -> str:
    """Compile libpgsd.so in-tree with hipcc --offload-arch=gfx950 (works without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    if force:
        cmd.append("-B")
    subprocess.run(cmd, check=True)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). This package has no fallback path.")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64; importing torch first makes
    # libpgsd.so bind to that copy instead of loading /opt/rocm's next to it (two runtimes in one
    # process cannot both open the device: the second one sees no GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.pg_abi_version.restype = C.c_int
    if L.pg_abi_version() != ABI_VERSION:  # (a library left over from an older build: its structs have other layouts)
        raise ImportError(f"{LIB_PATH} has ABI version {L.pg_abi_version()}, these bindings are written for {ABI_VERSION}: "
                          "rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`")
    for entry_points in list(SURFACE.values()) + list(SURFACE_EXTRA.values()) + list(SURFACE_EXT.values()) + list(
            SURFACE_MORE.values()):
        for name, argtypes in entry_points.items():
            fn = getattr(L, name)  # (a missing symbol is an AttributeError here)
            fn.argtypes = list(argtypes)
            fn.restype = RESTYPES.get(name, C.c_int)
    _lib = L
    return L


def check(ctx, rc: int):
    if rc != PG_OK:
        msg = lib().pg_last_error(ctx)
        raise PgError(rc, msg.decode() if msg else "")
