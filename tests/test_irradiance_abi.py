"""include/pgsd_irradiance.h, the bindings and the built library name the same entry points.  No GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from practical_path_guiding_lab_amd import _native

    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def test_header_symbols_are_exported(native):
    hdr = open(os.path.join(ROOT, "include", "pgsd_irradiance.h")).read()
    declared = re.findall(r"^(?:int|const char \*)\s*(pg_[a-z_0-9]+)\s*\(", hdr, flags=re.M)
    assert len(declared) == 6 and len(set(declared)) == 6
    assert set(declared) == set(native.EXPORTS_IRRADIANCE)
    others = (native.EXPORTS + native.EXPORTS_WARP + native.EXPORTS_FRACTION + native.EXPORTS_TARGET + native.EXPORTS_RADIANCE
              + native.EXPORTS_BOUNCE)
    assert not set(declared) & set(others)
    lib = ctypes.CDLL(native.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), name
    # the ABI version stays: entry points were added, nothing of the other headers changed
    assert native.lib().pg_abi_version() == native.ABI_VERSION == 6
    for name in declared:
        assert getattr(native.lib(), name).argtypes is not None and getattr(native.lib(), name).restype is ctypes.c_int


def test_the_probe_build_exports_them_too(native):
    probe = os.path.join(os.path.dirname(native.LIB_PATH), "libpgsd_phases.so")
    if not os.path.exists(probe):
        import subprocess
        subprocess.run(["make", "-C", native.CSRC, "-j4", "probe"], check=True, capture_output=True)
    lib = ctypes.CDLL(probe)
    for name in native.EXPORTS_IRRADIANCE:
        assert hasattr(lib, name), name


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
