"""Makes tests/golden/scene_xml_digests.json: what load_xml reads from the reference's own scene files for
veach-ajar (64x36) and torus (64x48), as the dtype, shape and SHA-256 of every array the tests compare with the
packaged scenes (scene.veach_ajar / scene.torus), so that the comparison runs without the reference's files.
The textures of veach-ajar alone are ~10 M texels: digests, not the arrays.  It is data of the reference, not code.

    python tests/golden/make_scene_xml_digests.py <root of the reference checkout>
"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from practical_path_guiding_lab_amd import scene as S  # noqa: E402


def digest(a):
    """{"dtype", "shape", "sha256"} of an array's bytes (C order): equal digests = equal arrays, bit for bit."""
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    scenes = os.path.join(sys.argv[1], "scenes")
    ajar = S.load_xml(os.path.join(scenes, "veach-ajar", "scene.xml"), 64, 36, skip_missing_meshes=True)
    torus = S.load_xml(os.path.join(scenes, "torus", "scene.xml"), 64, 48)
    out = {
        "veach-ajar 64x36": {
            "skipped": list(ajar.skipped),
            "arrays": {k: digest(getattr(ajar, k)) for k in ("tris", "bvh", "tri_uvs", "tri_normals", "materials", "quads", "bbox_min",
                                                             "bbox_max", "srgb_lut", "textures", "texels")},
            "camera": {k: digest(getattr(ajar.camera, k)) for k in ("origin", "axis_x", "axis_y", "axis_z", "tan_half_fov_x")},
        },
        "torus 64x48": {
            "width": int(torus.camera.width), "rfilter": torus.rfilter, "max_depth": int(torus.max_depth),
            "arrays": dict({k: digest(getattr(torus, k)) for k in ("bvh", "tri_normals", "dir_lights", "bbox_min", "bbox_max")},
                           tris_geometry=digest(torus.tris[:, :12]),
                           material_of_each_triangle=digest(torus.materials[torus.tris[:, 12].astype(int)])),
            "camera": {k: digest(getattr(torus.camera, k)) for k in ("origin", "axis_x", "axis_y", "axis_z")},
        },
    }
    dst = os.path.join(os.path.dirname(__file__), "scene_xml_digests.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
