"""Host side of the filters in recording render passes (no GPU): the two new exports, main.py's --splat-filter, the arithmetic
of the per-pass filter seed, and the Python layer's bookkeeping of the choice."""
import ctypes
import os
import sys

import pytest

from abi_table import COUNTS, native  # noqa: F401  (native: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_the_library_exports_what_the_header_declares(native):
    """(The count of pgsd.h's entry points and how it came about: tests/abi_table.py; header against library: tests/test_abi.py.)"""
    assert {"pg_render_record_geometry", "pg_render_export_records"} <= set(native.EXPORTS)
    L = native.lib()
    assert L.pg_render_record_geometry.argtypes == [ctypes.c_void_p, ctypes.c_int32]
    assert len(L.pg_render_export_records.argtypes) == 6
    # a NULL context is refused before anything touches a device
    assert L.pg_render_record_geometry(None, 1) == -1
    assert L.pg_render_export_records(None, 0, None, None, None, None) == -1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    n = COUNTS["pgsd.h"]
    assert "%d exports" % n in design and not [k for k in range(55, n) if "%d exports" % k in design]


def test_main_parses_the_splat_filter():
    import main

    ap = main.build_parser()
    assert ap.parse_args([]).splat_filter == ("nearest", "nearest")
    assert ap.parse_args(["--splat-filter", "stochastic,box"]).splat_filter == ("stochastic", "box")
    assert ap.parse_args(["--splat-filter", " nearest , box "]).splat_filter == ("nearest", "box")
    for bad in ("box,nearest", "stochastic", "stochastic,box,1", "gaussian,box", "stochastic,tent", ""):
        with pytest.raises(SystemExit):
            ap.parse_args(["--splat-filter", bad])
    # the default builds the scene exactly as before the option existed: no keyword at all, no geometry recording
    assert main.scene_options(("nearest", "nearest")) == {}
    for f in (("stochastic", "nearest"), ("nearest", "box"), ("stochastic", "box")):
        assert main.scene_options(f) == {"record_geometry": True}


def test_scene_and_integrator_keep_the_choice():
    from practical_path_guiding_lab_amd.render import WavefrontScene
    from practical_path_guiding_lab_amd.scene import cornell_box

    sc = cornell_box(8, 8, 4, 8)
    assert WavefrontScene(sc).record_geometry is False and WavefrontScene(sc).split_pipeline is False
    assert WavefrontScene(sc, record_geometry=True).record_geometry is True


def test_per_pass_filter_seed_arithmetic():
    from practical_path_guiding_lab_amd.render import pass_filter_seed

    assert pass_filter_seed(0, 0) == 0
    assert pass_filter_seed(11, 4242) == 4253
    assert pass_filter_seed(0xFFFFFFFF, 1) == 0                      # modulo 2^32
    assert pass_filter_seed(0xFFFFFFF0, 0x20) == 0x10
    assert pass_filter_seed(3, (1 << 32) + 5) == 8                   # a sampler seed beyond 32 bits counts by its low word
    assert pass_filter_seed(7, 100) != pass_filter_seed(7, 101)      # two passes of an iteration do not jitter alike
    assert all(0 <= pass_filter_seed(a, b) < (1 << 32) for a in (0, 1, 0xFFFFFFFF) for b in (0, 0xFFFFFFFF, 1 << 40))
