"""The Python packers of the scene tables (scene.py, mesh.py) and include/pgsd.h agree on every stride.
The library's own constants are defined FROM the header's macros (csrc/pg_scene_layout.hpp), so the header is the one
place all three layers meet.  No GPU, no library call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_strides():
    hdr = open(os.path.join(ROOT, "include", "pgsd.h")).read()
    return {name: int(value) for name, value in re.findall(r"^#define PG_([A-Z]+)_STRIDE (\d+)\s*$", hdr, flags=re.M)}


def test_python_strides_are_the_headers():
    from practical_path_guiding_lab_amd import mesh, scene

    strides = _header_strides()
    ours = {"QUAD": scene.QUAD_STRIDE, "SPHERE": scene.SPHERE_STRIDE, "MATERIAL": scene.MATERIAL_STRIDE,
            "TEXTURE": scene.TEXTURE_STRIDE, "BOX": scene.BOX_STRIDE, "DIRLIGHT": scene.DIRLIGHT_STRIDE,
            "TRI": mesh.TRI_STRIDE, "BVH": mesh.BVH_STRIDE}
    assert strides == ours      # every #define PG_*_STRIDE has its Python twin, and no value differs


def test_the_library_takes_its_strides_from_the_header():
    """csrc/ declares no stride of its own: pg_scene_layout.hpp defines each from the public macro."""
    csrc = os.path.join(ROOT, "practical_path_guiding_lab_amd", "csrc")
    layout = open(os.path.join(csrc, "pg_scene_layout.hpp")).read()
    names = {"QUAD": "kQuadStride", "SPHERE": "kSphereStride", "MATERIAL": "kMaterialStride", "TEXTURE": "kTextureStride",
             "BOX": "kBoxStride", "DIRLIGHT": "kDirLightStride", "TRI": "kTriStride", "BVH": "kBvhStride"}
    assert set(names) == set(_header_strides())
    for macro, k in names.items():
        assert re.search(r"^constexpr int %s = PG_%s_STRIDE;" % (k, macro), layout, flags=re.M), k
        for f in os.listdir(csrc):
            if f.endswith((".hip", ".hpp")) and f != "pg_scene_layout.hpp":
                assert not re.search(r"\b%s\s*=[^=]" % k, open(os.path.join(csrc, f)).read()), (f, k)


def test_packed_rows_have_the_declared_widths():
    from practical_path_guiding_lab_amd import mesh, scene

    sc = scene.Scene.__dataclass_fields__
    for field, width in (("spheres", scene.SPHERE_STRIDE), ("boxes", scene.BOX_STRIDE), ("tris", mesh.TRI_STRIDE),
                         ("bvh", mesh.BVH_STRIDE), ("dir_lights", scene.DIRLIGHT_STRIDE), ("textures", scene.TEXTURE_STRIDE)):
        assert sc[field].default_factory().shape == (0, width), field
    assert scene.diffuse_material((0.5, 0.5, 0.5)).shape == (scene.MATERIAL_STRIDE,)
    assert scene.directional_light((0, 0, 1), (1, 1, 1)).shape == (scene.DIRLIGHT_STRIDE,)
    box = scene.cornell_box(8, 8, 4, 8)
    assert box.quads.shape[1] == scene.QUAD_STRIDE
