#!/usr/bin/env python3
"""What the irradiance estimate (include/pgsd_irradiance.h) costs, one run, one JSON line on stdout.

  query  pg_irradiance_query (with a normal and without) and pg_irradiance_rr beside pg_radiance_query with and without a
         direction, all launched from the same build in the same job on the same positions;
  build  pg_irradiance_build beside pg_refine_and_swap of the same forest (the refine of an iteration that recorded nothing: the
         tree is rebuilt as it stands; timed once per round on a fresh copy of the forest, with host wall clocks around a
         synchronised call, as both calls allocate and launch many kernels).

Forests: tools/radiance_timing.py's -- s1 (workload.s1_balanced_tree() with loaded weights) and bench (veach-ajar at 1920 x 1080
after six rendered training iterations with the radiance feature on).

--lanes uniform positions in the forest's box, uniform unit normals / directions (default 2^22).  HIP events around single
launches: `--warmup` launches of each call, then `--launches` rounds in which the calls are timed one after the other
(interleaved, so a drift of the device's clocks meets them alike).  Per call: the minimum, the median and the maximum.

The expectation the numbers are held against: the irradiance query walks no quadtree, so its median should lie at or below
pg_radiance_query's with a direction and near the one without.

    python3 tools/irradiance_timing.py [--forest s1|bench|both] [--lanes N] [--launches 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def _stats(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def measure_query(torch, g, bmin, bmax, n, launches, warmup):
    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    lo = torch.tensor(bmin, dtype=torch.float32, device="cuda")[:, None]
    hi = torch.tensor(bmax, dtype=torch.float32, device="cuda")[:, None]
    P = (lo + Wk.s_uniform(n, 3, 3, device="cuda") * (hi - lo)).contiguous()
    D = Wk.s_directions_uniform(n, 4, device="cuda")
    smp = PCG32Sampler(g, n, seed=6)
    one = torch.ones(n, dtype=torch.float32, device="cuda")
    E = g.irradianceEstimate(P, D)
    ref = torch.full((n,), float(E.median()), dtype=torch.float32, device="cuda")    # q spread around 1: every branch runs
    calls = {
        "pg_radiance_query": lambda: g.radianceEstimate(P, D),
        "pg_radiance_query_mean_only": lambda: g.radianceEstimate(P),
        "pg_irradiance_query": lambda: g.irradianceEstimate(P, D),
        "pg_irradiance_query_no_normal": lambda: g.irradianceEstimate(P),
        "pg_irradiance_rr": lambda: g.irradianceRoulette(P, D, one, ref, smp, 5.0, 8),
    }
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(launches):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    out = {"lanes": n, "E_positive_share": round(float((E > 0).float().mean()), 4), "ms": {k: _stats(v) for k, v in ms.items()}}
    m = {k: v["median"] for k, v in out["ms"].items()}
    out["at_or_below_radiance_query_with_direction"] = bool(m["pg_irradiance_query"] <= m["pg_radiance_query"])
    out["median_ratio_to_radiance_query_mean_only"] = {k: round(v / m["pg_radiance_query_mean_only"], 3) for k, v in m.items()}
    return out


def measure_build(torch, g, rounds, warmup):
    """pg_irradiance_build beside pg_refine_and_swap, each on a copy of the forest loaded from the same export."""
    from practical_path_guiding_lab_amd.sdtree import SDTree
    cols, w = g.export(), g.radianceWeights()
    st = g.stats()
    ms = {"pg_irradiance_build": [], "pg_refine_and_swap": []}
    for r in range(warmup + rounds):
        t = SDTree(0)
        t.load(cols)
        t.radianceEnable()
        t.radianceLoadWeights(w)
        t.setIteration(3, False)
        t.irradianceBuild()          # (the first build of a context allocates its buffers; the timed one reuses them, as every
                                     #  later iteration's does where the forest did not outgrow them)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.irradianceBuild()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        t.refineAndPrepare()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r >= warmup:
            ms["pg_irradiance_build"].append((t1 - t0) * 1e3)
            ms["pg_refine_and_swap"].append((t2 - t1) * 1e3)
        del t
    out = {"forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes),
                      "mean_quad_leaf_depth": round(st.mean_quad_leaf_depth, 3)},
           "ms": {k: _stats(v) for k, v in ms.items()}}
    out["median_ratio_build_to_refine"] = round(out["ms"]["pg_irradiance_build"]["median"] / out["ms"]["pg_refine_and_swap"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forest", default="both", choices=["s1", "bench", "both"])
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--build-rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import radiance_timing as rt

    out = {"launches": a.launches, "warmup": a.warmup, "library": os.environ.get("PGSD_LIBRARY", "libpgsd.so")}
    for name, make in (("s1", rt.s1_forest), ("bench", rt.bench_forest)):
        if a.forest in (name, "both"):
            g, bmin, bmax, keep = make(torch)
            g.irradianceBuild()
            out[name] = {"query": measure_query(torch, g, bmin, bmax, a.lanes, a.launches, a.warmup),
                         "build": measure_build(torch, g, a.build_rounds, 2)}
            del g, keep
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
