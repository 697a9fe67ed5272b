"""include/pgsd_irradiance.h leaves the other headers alone; the refusals that need no device (what every header shares:
tests/test_abi.py).  No GPU."""
import ctypes
import os

from abi_table import native  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_leaves_the_other_headers_alone(native):
    hdr = open(os.path.join(ROOT, "include", "pgsd_irradiance.h")).read()
    assert '#include "pgsd_radiance.h"' in hdr and "typedef" not in hdr      # pg_rr_params is pgsd_radiance.h's
    for other in ("pgsd.h", "pgsd_radiance.h", "pgsd_bounce.h"):
        assert "irradiance_" not in open(os.path.join(ROOT, "include", other)).read()


def test_refusals_that_need_no_device(native):
    L = native.lib()
    prm = native.pg_rr_params(5.0, 1)
    assert L.pg_irradiance_build(None, None) == -1          # PG_ERR_INVALID: a NULL context
    assert L.pg_irradiance_status(None, None) == -1
    assert L.pg_irradiance_export(None, 0, None) == -1 and L.pg_irradiance_import(None, 0, None) == -1
    assert L.pg_irradiance_query(None, 0, None, None, None, None, None) == -1
    assert L.pg_irradiance_rr(None, 0, None, None, None, None, ctypes.byref(prm), None, None, None, None, None, None, None) == -1
