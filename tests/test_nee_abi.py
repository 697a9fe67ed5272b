"""The ABI of include/ext/lights/pg_nee.h (no GPU needed): the header, its entry of _native.SURFACE_MORE and the two builds name the
same three calls with the same parameter counts; the structs have the header's layout."""
import ctypes
import os
import re

import abi_table
from abi_table import native  # noqa: F401  (the fixture)

HEADER = "ext/lights/pg_nee.h"
NAMES = [("pg_nee_set_lights", 4), ("pg_nee_status", 2), ("pg_nee_resample", 5)]
FIELDS = ["p", "normal", "active", "rng_state", "rng_inc", "light_out", "point_out", "weight_out", "dir_out", "dist_out", "target_out",
          "source_out", "index_out", "cand_light_out", "cand_point_out", "cand_target_out", "cand_source_out"]


def test_header_table_and_libraries_agree(native):  # noqa: F811
    assert os.path.exists(os.path.join(abi_table.INCLUDE, *HEADER.split("/")))
    assert HEADER in native.SURFACE_MORE                                                      # it joined the last table
    assert [(n, len(a)) for n, a in native.SURFACE_MORE[HEADER].items()] == NAMES
    assert abi_table.declarations(HEADER) == NAMES
    assert all(n in native.EXPORTS_MORE for n, _ in NAMES)
    product, probe, L = abi_table.product_library(native), abi_table.probe_library(native), native.lib()
    for name, n_params in NAMES:
        assert hasattr(product, name) and hasattr(probe, name), name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_params, name
    fn = L.pg_nee_resample
    assert fn.argtypes[2]._type_ is native.pg_nee_params and fn.argtypes[3]._type_ is native.pg_nee_args
    assert native.ABI_VERSION == abi_table.ABI_VERSION == 6
    text = abi_table.header_text(HEADER)
    assert '#include "../../pg_resample.h"' in text and '#include "../pg_lights.h"' in text
    mk = open(os.path.join(native.CSRC, "Makefile")).read()
    assert "pg_kernels_nee.hip" in re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()
    assert "pg_lights_dev.hpp" in re.search(r"^HDRS = (.*)$", mk, flags=re.M).group(1).split()


def test_struct_layout_and_constants(native):  # noqa: F811
    assert ctypes.sizeof(native.pg_nee_params) == 16 and ctypes.sizeof(native.pg_nee_args) == 17 * 8
    assert native.pg_nee_params.candidates.offset == 0 and native.pg_nee_params.reserved.offset == 4
    text = re.sub(r"/\*.*?\*/", "", abi_table.header_text(HEADER), flags=re.S)
    body = re.search(r"typedef struct pg_nee_args \{(.*?)\} pg_nee_args;", text, flags=re.S).group(1)
    names = re.findall(r"\*\s*([a-z_]+)\s*[,;]", body)
    assert names == [f[0] for f in native.pg_nee_args._fields_] == FIELDS
    assert all(f[1] is ctypes.c_void_p for f in native.pg_nee_args._fields_)
    body = re.search(r"typedef struct pg_nee_params \{(.*?)\} pg_nee_params;", text, flags=re.S).group(1)
    assert re.findall(r"uint32_t\s+([a-z_]+)(\[\d+\])?;", body) == [("candidates", ""), ("reserved", "[3]")]
    # reused, not restated
    assert "#define PG_RESAMPLE_NONE" not in text and "#define PG_LIGHTS_NONE" not in text and "#define PG_LIGHTS_MAX" not in text
    assert "#define PG_RESAMPLE_MAX_CANDIDATES" not in text
    assert "#define PG_NEE_TABLE_WORDS 12" in text and native.PG_NEE_TABLE_WORDS == 12


def test_the_header_says_what_is_not_built_and_when_the_estimator_is_unbiased():
    text = " ".join(re.sub(r"^ \*", "", abi_table.header_text(HEADER), flags=re.M).split())   # (without the comment's leading stars)
    assert "NOT BUILT" in text
    for what in ("spheres, point, directional and environment lights", "glossy lobe", "feeding the rows", "remapped u",
                 "compacted lane lists", "pg_render_pass"):
        assert what in text.split("NOT BUILT", 1)[1], what
    assert "EXACTLY FOUR draws" in text and "unbiased when every light has pm > 0" in text and "W = 1 / s_kept" in text
    for what in ("light_out, point_out or weight_out", "candidates outside 1..64", "no table set", "lights feature disabled",
                 "n > 2^32 - 1"):
        assert what in text.split("REFUSALS", 1)[1], what
