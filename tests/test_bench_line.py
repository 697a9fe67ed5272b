"""bench.py's stdout contract: ONE line, < 6 KB, strict JSON, carrying value / ms_per_step / roofline /
cpu_baseline -- the driver kept `parsed: null` for round 5's 22.9 KB line.  The formatter is run here on canned records (the
builder-run round-5 record committed under profiles/, a record padded with prose and non-finite numbers, a --gpus 8 record, the
--synthetic record): no GPU."""
import copy
import io
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 6000


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_line_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _strict(line):
    def fail(name):
        raise AssertionError("non-finite constant in the line: " + name)
    assert "\n" not in line and len(line.encode()) < LIMIT, len(line.encode())
    return json.loads(line, parse_constant=fail)


def _canned():
    return json.load(open(os.path.join(ROOT, "profiles", "r05", "bench_r05.json")))


def test_the_round_5_record_becomes_a_line_the_driver_can_read():
    B = _bench()
    assert B.COMPACT_LINE_MAX <= LIMIT
    full = _canned()
    assert len(json.dumps(full)) > 20000          # what the driver could not parse
    c = _strict(B.format_line(full))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in c, k
    assert c["value"] == full["value"] and c["ms_per_step"] == full["ms_per_step"] and c["schema"] == B.SCHEMA
    assert c["config"]["workload"].startswith("veach-ajar 1920x1080") and "model" not in c["config"]
    r = c["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_us", "layout_bytes_per_launch",
              "frac_model_8d", "value_region_kernel", "value_region_frac", "s1_pg_sample_frac"):
        assert k in r, k
    assert r["bound"] == "hbm" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and len(r["frac_basis"]) <= 120
    # recomputable: layout bytes per launch / the average launch / peak
    assert abs(r["layout_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9 / r["peak"] - r["frac"]) < 2e-3
    b = c["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in b, k
    assert b["kind"] == "port" and len(b["sample"]) <= 240
    assert all(isinstance(v, (int, float)) for v in c["kernels"].values())       # name -> ms per step, nothing else
    assert abs(sum(v for k, v in c["kernels"].items() if k != "k_wave_guide") - c["ms_per_step"]) < 0.05 * c["ms_per_step"]
    assert c["extra"]["source_hash"] == full["extra"]["source_hash"]
    # no prose anywhere but the few labelled strings
    def strings(x, path=""):
        if isinstance(x, dict):
            for k, v in x.items():
                yield from strings(v, path + "/" + k)
        elif isinstance(x, str):
            yield path, x
    assert max(len(s) for _, s in strings(c)) <= 300


def test_a_padded_record_with_non_finite_numbers_still_fits_and_parses():
    B = _bench()
    full = _canned()
    full["value_full_schedule"] = float("nan")
    full["roofline"]["traffic"] = float("inf")
    full["roofline"]["frac_counter_hi"] = float("-inf")
    full["config"]["workload"] = "w" * 5000
    full["cpu_baseline"]["sample"] = "s" * 5000
    full["extra"]["exchange"] = "x" * 5000
    full["roofline"]["note"] = "n" * 50000
    full["kernels"] = {"k_%03d" % i: {"ms_per_step": 0.5, "note": "z" * 999} for i in range(400)}   # would overflow: dropped, not truncated
    c = _strict(B.format_line(full))
    assert c["roofline"]["traffic"] is None and c["roofline"]["frac_counter_hi"] is None and c.get("value_full_schedule") is None
    assert c["value"] == full["value"] and "roofline" in c and "cpu_baseline" in c


def test_the_line_of_a_sharded_run_and_of_the_synthetic_workload():
    B = _bench()
    full = _canned()
    full.update({"n_gpus": 8, "ranks": 8})
    full["cpu_baseline"] = None                     # N > 1: no CPU leg
    full["config"].update({"pixels_per_rank_min": 259200, "pixels_per_rank_max": 259200, "steps_per_launch": 8, "passes_per_launch": 128})
    full["extra"].update({"rccl_ranks": 8, "exchange": "pg_allreduce (RCCL ncclAllReduce int64 issued by libpgsd.so)"})
    c = _strict(B.format_line(full))
    assert c["n_gpus"] == 8 and c["ranks"] == 8 and c["cpu_baseline"] is None
    assert c["extra"]["rccl_ranks"] == 8 and "RCCL" in c["extra"]["exchange"] and c["extra"]["exchange_bytes"] > 0
    assert c["config"]["pixels_per_rank_min"] == 259200 and c["config"]["steps_per_launch"] == 8
    synth = {"metric": "Msamples/s guided (SD-tree hot path only, synthetic pass)", "value": 1.0, "unit": "Msamples/s", "n_gpus": 1,
             "ranks": 1, "steps": 2, "warmup": 1, "ms_per_step": 3.0, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
             "dtype": "f32", "data": "synthetic", "config": {"workload": "C2-synthetic"},
             "roofline": {"bound": "hbm", "kernel": "k_guide_bounce", "achieved": 1.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.1, "traffic": None},
             "cpu_baseline": None, "kernels": {"k_guide_bounce": {"launches": 16, "avg_us": 100.0}}}
    c = _strict(B.format_line(synth))
    assert c["data"] == "synthetic" and c["kernels"]["k_guide_bounce"] == pytest.approx(0.8) and c["roofline"]["traffic"] is None


def test_emit_puts_the_full_record_in_a_file_and_one_line_on_stdout(tmp_path, monkeypatch, capsys):
    B = _bench()
    full = _canned()
    full["mse_vs_gt"] = float("nan")
    detail = str(tmp_path / "detail.json")
    B.emit(copy.deepcopy(full), detail)
    cap = capsys.readouterr()
    lines = cap.out.splitlines()
    assert len(lines) == 1 and cap.out.endswith("\n")
    _strict(lines[0])
    assert "full record" in cap.err and "{" not in cap.err            # stderr: a pointer to the file, written BEFORE the line
    d = json.load(open(detail), parse_constant=lambda n: pytest.fail(n))
    assert d["kernels_synthetic"] == full["kernels_synthetic"] and d["mse_vs_gt"] is None


def test_the_launcher_relays_exactly_that_one_line(tmp_path):
    """`python bench.py --gpus N` without a launcher: spawn_ranks relays rank 0's stdout; with the compact line as rank 0's only
    JSON the parent's stdout is that line and nothing else."""
    B = _bench()
    line = B.format_line(_canned())
    child = ("import os, sys\n"
             "if os.environ['RANK'] == '0':\n"
             "    sys.stderr.write('[bench] full record: somewhere\\n'); sys.stdout.write(sys.argv[1] + '\\n')\n")
    relay = io.StringIO()
    assert B.spawn_ranks([sys.executable, "-c", child, line], 2, relay=relay) == 0
    assert relay.getvalue() == line + "\n"
    _strict(relay.getvalue().rstrip("\n"))


def _parse(B, monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return B.parse()


LEGS = ("full_schedule", "synthetic_kernels", "other_configs", "pmc_in_run", "phase_probe", "spp1", "cpu")


def test_a_plain_run_measures_the_headline_only_and_full_runs_every_leg(monkeypatch, capsys):
    """Without --full every leg is off and one asked for by itself is refused; --full gives each its default (all on at N = 1 on
    the default scene), a leg switched off stays off; --steps below 1 is refused (ms_per_step is over the timed steps)."""
    B = _bench()
    a = _parse(B, monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.steps == 7 and a.warmup == 3 and all(getattr(a, k) == 0 for k in LEGS) and a.dump_outputs is None
    a = _parse(B, monkeypatch, ["--full"])
    assert a.full and all(getattr(a, k) == 1 for k in LEGS)
    a = _parse(B, monkeypatch, ["--full", "--cpu", "0", "--phase-probe", "0"])
    assert a.cpu == 0 and a.phase_probe == 0 and a.spp1 == 1 and a.full_schedule == 1
    assert _parse(B, monkeypatch, ["--phase-probe", "2"]).phase_probe == 2     # (the probe child: not a leg)
    assert _parse(B, monkeypatch, ["--dump-outputs", "d"]).dump_outputs == "d"
    for bad in (["--cpu", "1"], ["--full-schedule", "1"], ["--steps", "0"], ["--synthetic", "--dump-outputs", "d"]):
        with pytest.raises(SystemExit):
            _parse(B, monkeypatch, bad)
    capsys.readouterr()


def test_dump_step_outputs_takes_the_last_step_of_the_launch(tmp_path):
    """dump_step_outputs on a launch of 3 steps x 4 passes (lane = pixel * passes + pass): the pixel means and the seeded lanes
    are those of the last step's 4 passes; the same arrays give the same files; a 4K film stays under 64 MB."""
    import numpy as np
    import torch
    B = _bench()
    npix, spp, passes = 50, 4, 12
    L = torch.arange(3 * npix * passes, dtype=torch.float32).reshape(3, npix * passes) * 0.25
    valid = (torch.arange(npix * passes) % 3 != 0).to(torch.uint8)
    wrote = B.dump_step_outputs(str(tmp_path / "a"), L, valid, passes, spp)
    assert sorted(wrote) == ["radiance_pixel_mean", "radiance_sample", "sample_lane", "valid_sample"]
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in wrote}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    Ls = L.numpy().reshape(3, npix, passes)[:, :, passes - spp:]
    vs = valid.numpy().reshape(npix, passes)[:, passes - spp:]
    np.testing.assert_allclose(got["radiance_pixel_mean"], Ls.mean(axis=2).T, rtol=1e-6)
    lane = got["sample_lane"].astype(np.int64)
    assert (np.diff(lane) > 0).all() and len(lane) == npix * spp                  # (fewer lanes than DUMP_LANES: all of them)
    assert (got["radiance_sample"] == Ls[:, lane // spp, lane % spp].T).all() and (got["valid_sample"] == vs[lane // spp, lane % spp]).all()
    B.dump_step_outputs(str(tmp_path / "b"), L, valid, passes, spp)
    assert all((np.load(str(tmp_path / "b" / (k + ".npy"))) == a).all() for k, a in got.items())
    big = B.dump_step_outputs(str(tmp_path / "c"), torch.zeros(3, 3840 * 2160 * 2), torch.ones(3840 * 2160 * 2, dtype=torch.uint8), 2, 2)
    assert "pixel_index" in big and sum(big.values()) <= 64 << 20


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_run_after_run_with_and_without_full(tmp_path):
    """`bench.py --dump-outputs`: two plain runs and a --full run of the same arguments write the same arrays, bit for bit (the
    timed steps trace the same passes whatever else the run measures); the plain line carries ms_per_step over --steps steps."""
    import json
    import subprocess
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scene", "veach-ajar", "--res", "128", "--train-iters", "3",
            "--spp-per-pass", "4", "--steps", "3", "--warmup", "1"]
    full = ["--full", "--cpu", "0", "--full-schedule", "0", "--spp1", "0", "--other-configs", "0", "--synthetic-kernels", "0",
            "--pmc-in-run", "0", "--phase-probe", "0", "--detail", str(tmp_path / "detail.json")]
    lines = {}
    for name, extra in (("a", []), ("b", []), ("full", full)):
        p = subprocess.run(base + extra + ["--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        out = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, p.stdout
        lines[name] = _strict(out[0])
    for c in lines.values():
        assert c["steps"] == 3 and c["ms_per_step"] > 0 and c["metric"].startswith("Msamples/s guided, veach-ajar 128x72")
        assert c["value"] == pytest.approx(c["config"]["paths_per_step"] / c["ms_per_step"] / 1e3, rel=2e-3)
    assert lines["a"]["roofline"] is None and lines["a"]["cpu_baseline"] is None and lines["full"]["roofline"]["kernel"] == "k_wave_guide"
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["radiance_pixel_mean.npy", "radiance_sample.npy", "sample_lane.npy", "valid_sample.npy"]
    for n in names:
        a = np.load(str(tmp_path / "a" / n))
        assert a.dtype in (np.float32, np.float64)
        for other in ("b", "full"):
            assert np.array_equal(a.view(np.uint8), np.load(str(tmp_path / other / n)).view(np.uint8)), (n, other)
    assert np.load(str(tmp_path / "a" / "radiance_pixel_mean.npy")).shape == (128 * 72, 3)
    assert np.load(str(tmp_path / "a" / "valid_sample.npy")).any()
