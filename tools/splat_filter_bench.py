#!/usr/bin/env python3
"""pg_splat through the training filters of pg_set_splat_filter on SURVEY 8(d)'s S3 input: the last S2 record stream
(2^24 records) replayed into the S2 forest, the input bench.py times for the nearest splat.

Per filter combination: ms per launch (HIP events around `--launches` back-to-back launches after warm-up) and, from the numpy
model of the filters (tests/filter_model.py) on the first `--model-records` records, the mean number of deposits a record makes.
A library without pg_set_splat_filter (an older build) is timed for nearest / nearest only.  One JSON line on stdout.

    python3 tools/splat_filter_bench.py [--launches 20] [--model-records 262144] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-records", type=int, default=1 << 18)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from practical_path_guiding_lab_amd import workload as Wk
    from practical_path_guiding_lab_amd.sdtree import SDTree

    dev = torch.device("cuda", 0)
    g = SDTree(0)
    g.setup([Wk.S_BBOX[0]] * 3, [Wk.S_BBOX[1]] * 3, 0, 0, 20, 20, True, 0.5)
    rec = None
    for k in range(Wk.S2_ITERATIONS):
        g.setIteration(k, False)
        rec = Wk.s2_record_stream(k, device=dev)
        g.addDataPropagate(rec)
        g.refineAndPrepare()
    g.setIteration(Wk.S2_ITERATIONS, False)
    m = int(rec["radiance"].shape[0])
    st = g.stats()
    out = {"records": m, "launches": a.launches,
           "forest": {"kd_leaves": int(st.n_kd_leaves), "quad_nodes": int(st.n_quad_nodes),
                      "mean_quad_leaf_depth": round(st.mean_quad_leaf_depth, 3), "max_quad_depth": int(st.max_quad_depth)},
           "ms": {}, "deposits_per_record": {}}
    combos = [("nearest", "nearest")]
    if hasattr(g, "setSplatFilter"):
        combos += [("nearest", "box"), ("stochastic", "nearest"), ("stochastic", "box")]
    for spatial, directional in combos:
        if hasattr(g, "setSplatFilter"):
            g.setSplatFilter(spatial, directional, seed=1)
        for _ in range(a.warmup):
            g.addDataPropagate(rec)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            g.addDataPropagate(rec)
        e1.record()
        e1.synchronize()
        out["ms"][spatial + "/" + directional] = round(e0.elapsed_time(e1) / a.launches, 4)
    if a.model_records > 0 and hasattr(g, "setSplatFilter"):
        import filter_model as fm

        n = min(a.model_records, m)
        cols = g.export()
        sub = {k: v[..., :n].cpu().numpy() for k, v in rec.items()}
        for spatial, directional in combos:
            r = fm.splat(cols, sub, spatial, directional, seed=1)
            out["deposits_per_record"][spatial + "/" + directional] = round(r["deposits"] / n, 4)
    near = out["ms"]["nearest/nearest"]
    out["ratio_to_nearest"] = {k: round(v / near, 3) for k, v in out["ms"].items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
