#!/usr/bin/env python3
"""What the radiance estimate (include/pgsd_radiance.h) costs beside the two calls a host has today, one run, one JSON line on
stdout: pg_radiance_query with and without a direction and pg_radiance_rr, beside pg_pdf and pg_get_leaf_node_index of the same
build on the same inputs.

  s1     workload.s1_balanced_tree() at its stated size, with loaded weights;
  bench  the forest bench.py's default line times its steps on: veach-ajar at 1920 x 1080, six rendered training iterations
         with the feature on, so that the weights are the ones the refines carried.

--lanes uniform positions in the forest's box and uniform directions (default 2^22).  HIP events around single launches:
`--warmup` launches of each call, then `--launches` rounds in which the calls are timed one after the other (interleaved, so a
drift of the device's clocks meets them alike).  Per call: the minimum, the median and the maximum over the rounds.

The expectation the numbers are held against: with a direction, the query makes pg_pdf's gathers plus one 8-byte gather in the
same round trip, so its median should lie below pg_pdf's plus pg_get_leaf_node_index's -- what a pdf and a second descent cost.

    python3 tools/radiance_timing.py [--forest s1|bench|both] [--lanes N] [--launches 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def s1_forest(torch):
    import numpy as np

    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import SDTree
    g = SDTree(0)
    g.load(Wk.s1_balanced_tree())
    g.radianceEnable()
    g.radianceLoadWeights(np.full(int(g.sizes().n_roots), 1 << 20, np.uint64))
    return g, [Wk.S_BBOX[0]] * 3, [Wk.S_BBOX[1]] * 3, None


def bench_forest(torch):
    import numpy as np

    import bench
    from practical_path_guiding_lab_amd.integrator import PathGuidingIntegrator
    from practical_path_guiding_lab_amd.render import IndependentSampler, WavefrontScene
    width, _, depth = bench.SCENES["veach-ajar"]
    sc = bench.make_scene("veach-ajar", width, depth)
    integ = PathGuidingIntegrator({"max_depth": depth, "rr_depth": 8}, device=0)
    bmin, bmax = sc.bbox_min - np.float32(1e-4), sc.bbox_max + np.float32(1e-4)
    integ.setup(sc.camera.width * sc.camera.height, bmin, bmax, 20, 20, True, 0.5)
    integ.sdTree.radianceEnable()
    ws = WavefrontScene(sc)
    ws.reserve(integ, 16)
    cumm, iters = 0, 6
    for k in range(iters):                              # bench.py run_render: 2^(k+2) spp per iteration, 16 per launch
        integ.setIteration(k, False)
        spp = 2 ** (k + 2)
        chunk = min(16, spp)
        for i in range(spp // chunk):
            integ.sample(ws, IndependentSampler(chunk, cumm + i * chunk, batched=True))
        integ.refineAndPrepareSDTreeForNextIteration()
        cumm += spp
    torch.cuda.synchronize()
    return integ.sdTree, [float(v) for v in bmin], [float(v) for v in bmax], (integ, ws)


def measure(torch, g, bmin, bmax, n, launches, warmup):
    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import PCG32Sampler
    st = g.stats()
    lo = torch.tensor(bmin, dtype=torch.float32, device="cuda")[:, None]
    hi = torch.tensor(bmax, dtype=torch.float32, device="cuda")[:, None]
    P = (lo + Wk.s_uniform(n, 3, 3, device="cuda") * (hi - lo)).contiguous()
    D = Wk.s_directions_uniform(n, 4, device="cuda")
    smp = PCG32Sampler(g, n, seed=6)
    one = torch.ones(n, dtype=torch.float32, device="cuda")
    L_dir, L_mean = g.radianceEstimate(P, D)
    ref = torch.full((n,), float(L_mean.median()), dtype=torch.float32, device="cuda")    # q spread around 1: every branch runs
    calls = {
        "pg_pdf": lambda: g.pdf(P, D),
        "pg_get_leaf_node_index": lambda: g.getLeafNodeIndex(P),
        "pg_radiance_query": lambda: g.radianceEstimate(P, D),
        "pg_radiance_query_mean_only": lambda: g.radianceEstimate(P),
        "pg_radiance_rr": lambda: g.radianceRoulette(P, D, one, ref, smp, 5.0, 8),
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
    w = g.radianceWeights()
    out = {"lanes": n,
           "forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes), "jump_bits": int(st.jump_bits),
                      "mean_quad_leaf_depth": round(st.mean_quad_leaf_depth, 3), "weight_min": int(w.min()), "weight_max": int(w.max())},
           "L_dir_positive_share": round(float((L_dir > 0).float().mean()), 4),
           "ms": {k: {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)} for k, v in ms.items()}}
    m = {k: v["median"] for k, v in out["ms"].items()}
    out["pdf_plus_leaf_index_median_ms"] = round(m["pg_pdf"] + m["pg_get_leaf_node_index"], 4)
    out["query_below_pdf_plus_leaf_index"] = bool(m["pg_radiance_query"] < m["pg_pdf"] + m["pg_get_leaf_node_index"])
    out["median_ratio_to_pg_pdf"] = {k: round(v / m["pg_pdf"], 3) for k, v in m.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forest", default="both", choices=["s1", "bench", "both"])
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    out = {"launches": a.launches, "warmup": a.warmup, "library": os.environ.get("PGSD_LIBRARY", "libpgsd.so")}
    for name, make in (("s1", s1_forest), ("bench", bench_forest)):
        if a.forest in (name, "both"):
            g, bmin, bmax, keep = make(torch)
            out[name] = measure(torch, g, bmin, bmax, a.lanes, a.launches, a.warmup)
            del g, keep
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
