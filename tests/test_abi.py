"""The C-ABI library loads without a GPU; every header of include/, the table of the bindings (_native.SURFACE), libpgsd.so and
the probe build name the same entry points with the same numbers of parameters.  No compute calls here (CPU box).
What only one header has -- its literal names, exact argtypes, struct layouts, refusals -- is in that feature's own test file."""
import ctypes
import glob
import os
import re

import pytest

import abi_table
from abi_table import native  # noqa: F401  (the fixture)


def test_the_table_covers_the_headers_on_disk(native):
    on_disk = sorted(os.path.basename(f) for f in glob.glob(os.path.join(abi_table.INCLUDE, "pgsd*.h")))
    assert on_disk == sorted(native.SURFACE) == sorted(abi_table.HEADERS)
    assert tuple(native.SURFACE) == abi_table.HEADERS                      # and in the order source_hash() has always hashed them
    # the build depends on the same set: whatever include/ holds
    mk = open(os.path.join(native.CSRC, "Makefile")).read()
    assert re.search(r"^HDRS = .*\$\(wildcard \.\./\.\./include/pgsd\*\.h\)$", mk, flags=re.M)
    # the names the tests, tools and test_entry.py read are the table's rows
    rows = (native.EXPORTS, native.EXPORTS_WARP, native.EXPORTS_FRACTION, native.EXPORTS_TARGET, native.EXPORTS_RADIANCE,
            native.EXPORTS_BOUNCE, native.EXPORTS_IRRADIANCE)
    assert rows == tuple(tuple(native.SURFACE[h]) for h in abi_table.HEADERS)
    assert sum(abi_table.COUNTS.values()) == abi_table.TOTAL == sum(len(r) for r in rows)
    # pairwise disjoint: no entry point belongs to two headers
    assert len(set().union(*map(set, rows))) == abi_table.TOTAL


@pytest.mark.parametrize("header", abi_table.HEADERS)
def test_header_symbols_are_exported(native, header):
    declared = abi_table.declarations(header)
    names = [n for n, _ in declared]
    assert names, "no declarations parsed from include/" + header
    # (comments hide no declaration and add none: the header's raw text gives the same names)
    assert names == re.findall(r"^(?:int|const char \*)\s*(pg_[a-z_0-9]+)\s*\(", abi_table.header_text(header), flags=re.M)
    assert len(names) == len(set(names)) == abi_table.COUNTS[header]
    bound = native.SURFACE[header]
    assert set(names) == set(bound) and len(bound) == len(names)
    for other in abi_table.HEADERS:
        if other != header:
            assert not set(names) & set(native.SURFACE[other]), other
            assert not set(names) & {n for n, _ in abi_table.declarations(other)}, other
    product, probe, L = abi_table.product_library(native), abi_table.probe_library(native), native.lib()
    for name, n_params in declared:
        assert hasattr(product, name) and hasattr(probe, name), name
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_char_p if name == "pg_last_error" else ctypes.c_int), name
        assert fn.argtypes is not None and len(fn.argtypes) == len(bound[name]) == n_params, name


def test_abi_version_and_loud_failure_without_gpu(native):
    L = native.lib()
    declared = int(re.search(r"^#define PGSD_ABI_VERSION (\d+)", abi_table.header_text("pgsd.h"), flags=re.M).group(1))
    assert L.pg_abi_version() == declared == native.ABI_VERSION == abi_table.ABI_VERSION == 6   # header, library and bindings agree
    assert abi_table.probe_library(native).pg_abi_version() == declared
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path is not reachable")
    h = ctypes.c_void_p()
    rc = L.pg_create(ctypes.byref(h), 0)
    assert rc == -5 and not h.value  # PG_ERR_NO_DEVICE
    assert b"no HIP device" in L.pg_last_error(None)
    from practical_path_guiding_lab_amd.sdtree import SDTree

    with pytest.raises(RuntimeError):
        SDTree()


def test_struct_layouts_match_header(native):
    # sizes the C side computes for the same structs (pointers 8 B, natural alignment)
    assert ctypes.sizeof(native.pg_records) == 6 * 8
    assert ctypes.sizeof(native.pg_dense_records) == 9 * 8
    assert ctypes.sizeof(native.pg_tree_sizes) == 24
    assert ctypes.sizeof(native.pg_tree_columns) == 8 + 3 * 4 + 4 + 19 * 8
    assert ctypes.sizeof(native.pg_stats) == 5 * 8 + 2 * 8 + 2 * 4 + 3 * 8 + 8 + 2 * 4
    assert ctypes.sizeof(native.pg_depth_counters) == 40
