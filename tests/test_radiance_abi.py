"""include/pgsd_radiance.h and the bindings lay pg_rr_params out alike; the refusals that need no device (what every header
shares: tests/test_abi.py).  No GPU."""
import ctypes
import os
import re

from abi_table import native  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_header(native):
    assert ctypes.sizeof(native.pg_rr_params) == 8
    assert native.pg_rr_params.window.offset == 0 and native.pg_rr_params.max_split.offset == 4
    hdr = open(os.path.join(ROOT, "include", "pgsd_radiance.h")).read()
    body = re.search(r"typedef struct pg_rr_params \{(.*?)\} pg_rr_params;", hdr, flags=re.S).group(1)
    assert re.findall(r"^\s*(float|uint32_t)\s+(\w+);", body, flags=re.M) == [("float", "window"), ("uint32_t", "max_split")]


def test_refusals_that_need_no_device(native):
    L = native.lib()
    prm = native.pg_rr_params(5.0, 1)
    assert L.pg_radiance_enable(None, 1) == -1          # PG_ERR_INVALID: a NULL context
    assert L.pg_radiance_status(None, None, None, None) == -1
    assert L.pg_radiance_export(None, 0, None) == -1 and L.pg_radiance_import(None, 0, None) == -1
    assert L.pg_radiance_query(None, 0, None, None, None, None, None, None) == -1
    assert L.pg_radiance_rr(None, 0, None, None, None, None, ctypes.byref(prm), None, None, None, None, None, None, None) == -1
