"""include/pgsd_bounce.h and the bindings give pg_bounce the same arguments and lay pg_bounce_args out alike (what every header
shares: tests/test_abi.py).  No GPU."""
import ctypes
import os
import re

import pytest

from abi_table import native  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "pgsd_bounce.h")).read()


def test_header_symbol_is_exported(native, header):
    declared = re.findall(r"^(?:int|const char \*)\s*(pg_[a-z_0-9]+)\s*\(", header, flags=re.M)
    assert declared == ["pg_bounce"]
    assert native.lib().pg_bounce.argtypes == [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(native.pg_bounce_args), ctypes.c_void_p]


def test_struct_layout_matches_header(native, header):
    body = re.search(r"typedef struct pg_bounce_args \{(.*?)\} pg_bounce_args;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"^(const\s+)?(float|uint8_t|uint32_t|uint64_t)\s+(.*)$", decl, flags=re.S)
        assert m, decl
        for name in m.group(3).split(","):
            name = name.strip()
            assert name.startswith("*") and not name.startswith("**"), decl    # every member is one pointer
            fields.append(name[1:].strip())
    assert len(fields) == 17 and len(set(fields)) == 17
    A = native.pg_bounce_args
    assert [n for n, _ in A._fields_] == fields
    assert ctypes.sizeof(A) == 8 * len(fields)
    for k, name in enumerate(fields):
        assert getattr(A, name).offset == 8 * k and getattr(A, name).size == 8, name
    for name, value in (("NONE", 0), ("PDF", 1), ("SAMPLE", 2), ("CHOOSE", 3)):
        assert re.search(r"#define PG_BOUNCE_%s\s+%d\b" % (name, value), header)
        assert getattr(native, "PG_BOUNCE_" + name) == value


def test_refusals_that_need_no_device(native):
    L = native.lib()
    a = native.pg_bounce_args()
    assert L.pg_bounce(None, 0, None, None) == -1             # PG_ERR_INVALID: a NULL context
    assert L.pg_bounce(None, 0, ctypes.byref(a), None) == -1
    assert L.pg_bounce(None, 16, ctypes.byref(a), None) == -1
